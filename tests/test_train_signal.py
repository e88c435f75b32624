r"""``fused.train_signal`` (Ktrs / Ktrsb: ``mrphy_train_signal_fwd`` / ``_bwd``) and ``fused.train_signal_rfgr`` on the device.

The yardstick is fp64 torch on the CPU on the same numbers: ``test_ab_train_host.torch_train`` followed by the complex
sum ``test_train_signal_host.torch_signal``, and autograd; never the new code or a composed device route.  The kernels
carry the recursion and every sum in fp64 and round each output once, so they are held to the kernel-alone gates of
``test_steadystate._gate``: fp64 max abs 1e-9 (a gradient in units of the yardstick's largest element), fp32 relative L2
1e-6.  End to end in fp32 (§11) the signal inherits the rounding of ``A`` amplified by the train's conditioning and is
held to three times what the reference's own all-fp32 route loses, the margin and reason of ``test_ab_train.py`` §8.
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_ab_rfgr import _counted
from test_ab_rfgr_host import fixture_inputs
from test_ab_train import ABSENT, KW, OPS, _identity, _kernel_problem, _same_bits
from test_ab_train_host import torch_train
from test_fused_traj import _problem
from test_steadystate import _form, _gate, _mode
from test_train_signal_host import demodulated, torch_signal

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
FWD, BWD = 'mrphy_train_signal_fwd', 'mrphy_train_signal_bwd'
LEAVES = ('A', 'B') + OPS


def _lib():
    return mrphy_amd.require_library()


S = int(_lib().mrphy_train_signal_ck_every())           # repetitions per checkpoint segment of the adjoint


def _sin(shape, dtype, a=0.37, b=0.3):
    n = 1
    for s in shape:
        n *= s
    return torch.sin(torch.arange(n, dtype=torch.float64) * a + b).reshape(shape).to(dtype)


@functools.lru_cache(maxsize=None)
def _rx(N, nM, nRx, tag):
    r"""A seeded complex receive map `(N, nM, xy)` (``nRx = 0``) or `(N, nM, xy, nRx)` in the data type; ``None`` for -1."""
    if nRx < 0:
        return None
    gen = torch.Generator().manual_seed(7000 + 100 * N + nM + 13 * nRx)
    shape = (N, nM, 2) + ((nRx,) if nRx else ())
    return (0.5 + torch.randn(shape, generator=gen, dtype=torch.float64)).to(DT[tag])


def _sig_shape(N, K, rx, Nd_ndim=1):
    return (N, 2, K) + ((rx.shape[-1],) if rx is not None and rx.ndim == Nd_ndim + 3 else ())


def _loss_weights(P, K, rx, w=None, v=None):
    N = P['A'].shape[0]
    nd = P['A'].ndim - 3
    w = _sin(_sig_shape(N, K, rx, nd), P['A'].dtype) if w is None else w
    v = _sin(tuple(P['B'].shape), P['A'].dtype, 0.53, 0.1) if v is None else v
    return w, v


def _yardstick(P, K, rx, use=OPS, w=None, v=None):
    r"""``sig``, ``Mlast`` and the gradients of ``(sig w).sum() + (Mlast v).sum()`` w.r.t. ``A, B``, the operands ``use`` and
    ``rx`` in fp64 on the CPU; operands not in ``use`` are absent."""
    w, v = _loss_weights(P, K, rx, w, v)
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    if rx is not None:
        L['rx'] = rx.double().clone().requires_grad_(True)
    Mt = torch_train(L['A'], L['B'], K, *(L.get(k) for k in OPS))
    sig = torch_signal(Mt, L.get('rx'))
    if K > 0:
        Mlast = Mt[..., -1, :]
    else:
        Mlast = (L['Mi'] if 'Mi' in L else torch.tensor([0., 0., 1.], dtype=torch.float64)).expand(P['B'].shape)
    loss = (sig * w.double()).sum() + (Mlast * v.double()).sum()
    if loss.requires_grad:
        loss.backward()
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['sig'], out['Mlast'] = sig.detach(), Mlast.detach()
    return out


@functools.lru_cache(maxsize=None)
def _cached_yardstick(N, nM, K, tag, nRx):
    P, _ = _kernel_problem(N, nM, K, tag)
    return _yardstick(P, K, _rx(N, nM, nRx, tag))


def _run(P, K, rx, use=OPS, over=None, w=None, v=None, n=True, leaves=None, loss=None, **kw):
    r"""The same through ``fused.train_signal`` on the device; ``over``: tensors that replace operands; ``leaves``: the
    names of the operands that require grad (all of them by default; the others' gradients come back ``None``);
    ``loss``: a callable that is handed ``sig, Mlast`` and runs the backward pass itself, instead of
    ``(sig w).sum() + (Mlast v).sum()``."""
    w, v = _loss_weights(P, K, rx, w, v)
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    if rx is not None:
        L['rx'] = dev(rx).clone().requires_grad_(wanted('rx'))
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    sig, Mlast = fused.train_signal(L['A'], L['B'], **({'n': K} if n else {}), **{KW[k]: L[k] for k in use},
                                    rx=L.get('rx'), return_last=True, **kw)
    if loss is not None:
        loss(sig, Mlast)
    elif sig.requires_grad:
        ((sig * dev(w)).sum() + (Mlast * dev(v)).sum()).backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['sig'], out['Mlast'] = sig.detach(), Mlast.detach()
    return out


def _gates(got, want, tag, what, keys=None):
    for k in (keys or want):
        print(f'{tag} {what} {k}: max abs {max_abs(got[k], want[k]):.3e} rel-L2 {rel_l2(got[k], want[k]):.3e}')
    for k in (keys or want):
        _gate(got[k], want[k], tag, f'{what}: {k}')


# =============================================================================================
# 1. values and all nine gradients
# =============================================================================================
SHAPES = [(1, 1, 1), (2, 100, 2), (2, 100, S + 1), (2, 200, 40), (1, 300, 3)]


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nRx', [-1, 0, 3, 8], ids=['norx', 'rx1', 'rx3', 'rx8'])
@pytest.mark.parametrize('N, nM, K', SHAPES, ids=['one', 'K2', 'KS1', 'K40', 'blocks2'])
def test_kernels_alone_against_the_fp64_recursion(tag, N, nM, K, nRx):
    r"""(1, 1, 1): one row; (2, 100, 2): a ragged tile per batch entry; (2, 100, S + 1): a second checkpoint segment of
    length 1; (2, 200, 40): several segments and tiles; (1, 300, 3): five tiles, the last ragged.  No map, one coil, 3
    coils (one pad coil at capacity 4) and 8 coils.  A second run gives the same bits."""
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, nRx, tag)
    want = _cached_yardstick(N, nM, K, tag, nRx)
    got = _run(P, K, rx, n=False)
    assert set(got) == set(want)
    assert got['sig'].dtype == got['Mlast'].dtype == DT[tag]
    assert got['sig'].shape == (N, 2, K) + ((nRx,) if nRx > 0 else ()) and got['Mlast'].shape == (N, nM, 3)
    _gates(got, want, tag, f'{(N, nM, K)} nRx {nRx}')
    for k in LEAVES + (('rx',) if rx is not None else ()):
        g = got['grad_' + k]
        assert g.shape == (rx if k == 'rx' else P[k]).shape and g.dtype == DT[tag] and float(g.abs().max()) > 0, k
    record(f'train_signal.{tag}.N{N}_nM{nM}_K{K}_rx{nRx}.sig',
           max_abs(got['sig'], want['sig']) if tag == 'f64' else rel_l2(got['sig'], want['sig']))
    _same_bits(got, _run(P, K, rx), 'a second run')


# =============================================================================================
# 2. absent operands
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(ABSENT))
def test_absent_operands(tag, case):
    r"""The five absences of ``test_ab_train.ABSENT`` against the yardstick with the same absence, three coils."""
    N, nM, K = 2, 100, S + 1
    P, _ = _kernel_problem(N, nM, K, tag)
    rx, use = _rx(N, nM, 3, tag), ABSENT[case]
    want, got = _yardstick(P, K, rx, use), _run(P, K, rx, use)
    assert set(got) == set(want) == {'sig', 'Mlast', 'grad_A', 'grad_B', 'grad_rx'} | {'grad_' + k for k in use}
    _gates(got, want, tag, case)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_no_receive_map_is_the_weight_one(tag):
    r"""``rx=None`` is an explicit ``(1, 0)`` on every spin, bit for bit, values and gradients."""
    N, nM, K = 2, 100, S + 1
    P, _ = _kernel_problem(N, nM, K, tag)
    one = torch.zeros((N, nM, 2), dtype=DT[tag])
    one[..., 0] = 1
    got, full = _run(P, K, None), _run(P, K, one)
    assert float(full.pop('grad_rx').abs().max()) > 0
    _same_bits(got, full, 'rx=None')


# =============================================================================================
# 3. operand forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_operand_forms(tag, form):
    r"""``T1``, ``T2`` in every broadcast form; ``rest`` `()` with ``phase`` `(1, K)` and ``Mi`` `(1, 1, 3)`, then full:
    the bits of the materialised call; each gradient has its operand's shape and is the materialised call's summed."""
    N, nM, K = 2, 100, S + 1
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, 3, tag)
    for small in (True, False):
        T1, T1m = _form(P['T1'], form)
        T2, T2m = _form(P['T2'], form)
        rest = P['rest'][0].clone() if small else P['rest'].clone()
        phase = P['phase'][:1].clone() if small else P['phase'].clone()
        Mi = P['Mi'][:1, :1].clone() if small else P['Mi'].clone()
        mat = _run(dict(P, T1=T1m, T2=T2m, rest=rest.expand(N).contiguous(), phase=phase.expand(N, K).contiguous(),
                        Mi=Mi.expand(N, nM, 3).contiguous()), K, rx)
        got = _run(P, K, rx, over=dict(T1=T1, T2=T2, rest=dev(rest), phase=dev(phase), Mi=dev(Mi)))
        what = (form, 'small' if small else 'full')
        for k in ('sig', 'Mlast', 'grad_A', 'grad_B', 'grad_df', 'grad_rx'):
            assert torch.equal(got[k], mat[k]), (what, k)
        for k, x in (('T1', T1), ('T2', T2), ('rest', rest), ('phase', phase), ('Mi', Mi)):
            g, m = got['grad_' + k], mat['grad_' + k]
            assert g.shape == x.shape and g.dtype == x.dtype, (what, k, g.shape)
            shp = tuple(x.shape) + (1,) * (m.ndim - x.ndim) if x.ndim else (1,) * m.ndim
            _gate(g, m.double().cpu().sum_to_size(shp).reshape(x.shape), tag, f'{what}: grad_{k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)`` with ``rx`` `(1, 10, 10, 2, 3)` shared by the batch: the bits of the flat `(N, 100)` call."""
    N, K = 2, S + 1
    P, _ = _kernel_problem(N, 100, K, tag)
    rx = _rx(N, 100, 3, tag)[:1].clone()
    flat = _run(P, K, rx.expand(N, 100, 2, 3).contiguous())
    Q = dict(P, A=P['A'].reshape(2, 10, 10, 3, 3), B=P['B'].reshape(2, 10, 10, 3), Mi=P['Mi'].reshape(2, 10, 10, 3),
             T1=P['T1'].reshape(2, 10, 10), T2=P['T2'].reshape(2, 10, 10), df=P['df'].reshape(2, 10, 10))
    w, v = _loss_weights(P, K, rx.expand(N, 100, 2, 3))
    got = _run(Q, K, rx.reshape(1, 10, 10, 2, 3), w=w, v=v.reshape(2, 10, 10, 3))
    assert got['sig'].shape == (N, 2, K, 3) and got['Mlast'].shape == (2, 10, 10, 3)
    assert torch.equal(got['sig'], flat['sig']) and torch.equal(got['Mlast'].reshape(2, 100, 3), flat['Mlast'])
    for k in ('A', 'B', 'Mi', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert torch.equal(got['grad_phase'], flat['grad_phase']) and got['grad_rest'].shape == (2,)
    _gate(got['grad_rest'], flat['grad_rest'], tag, 'grad_rest')          # (summed over the spins in another order)
    assert got['grad_rx'].shape == (1, 10, 10, 2, 3)
    _gate(got['grad_rx'].reshape(1, 100, 2, 3), flat['grad_rx'].double().cpu().sum(0, keepdim=True), tag, 'grad_rx')


# =============================================================================================
# 4. coils
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nRx', [3, 8, 9])
def test_every_coil_has_the_bits_of_its_one_coil_call(tag, nRx, monkeypatch):
    r"""``sig[..., c]`` of the 3-, 8- and 9-coil calls is the one-coil call's, bit for bit; the array's gradients are
    the sums of the one-coil calls' to the gate.  Nine coils are over the capacity: two launches each way."""
    N, nM, K = 2, 200, S + 3
    cap = int(_lib().mrphy_train_signal_max_rx(0 if tag == 'f32' else 1))
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, nRx, tag)
    w = _sin((N, 2, K, nRx), DT[tag])
    v = torch.zeros_like(P['B'])
    calls = _counted(monkeypatch, (FWD, BWD))
    got = _run(P, K, rx, w=w, v=v)
    assert dict(calls) == {FWD: -(-nRx // cap), BWD: -(-nRx // cap)}
    assert got['sig'].shape == (N, 2, K, nRx)
    total = None
    for c in range(nRx):
        one = _run(P, K, rx[..., c].contiguous(), w=w[..., c].contiguous(), v=v)
        assert torch.equal(one['sig'], got['sig'][..., c]), c
        assert torch.equal(one['Mlast'], got['Mlast']), c
        _gate(got['grad_rx'][..., c], one['grad_rx'], tag, f'grad_rx of coil {c}')
        g = {k: x.double().cpu() for k, x in one.items() if k.startswith('grad_') and k != 'grad_rx'}
        total = g if total is None else {k: total[k] + g[k] for k in g}
    _gates(got, total, tag, f'{nRx} coils vs the sum of the one-coil calls')


# =============================================================================================
# 5. known answers
# =============================================================================================
def _kwargs(D, use=OPS):
    return {KW[k]: D[k] for k in use}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_last_record_and_one_hot_map_are_ab_train_bit_for_bit(tag):
    r"""``Mlast`` is ``ab_train``'s last record; with the weight ``(1, 0)`` on one spin alone -- of the first tile, and
    of a later one -- ``sig[n, :, k]`` is that spin's ``Mt[n, s, k, :2]``: the other spins add exact zeros."""
    N, nM, K = 2, 200, 40
    P, _ = _kernel_problem(N, nM, K, tag)
    D = {k: dev(P[k]) for k in LEAVES}
    with torch.no_grad():
        Mt = fused.ab_train(D['A'], D['B'], **_kwargs(D))
        for s in (5, 70, 199):
            rx = torch.zeros((N, nM, 2), dtype=DT[tag])
            rx[:, s, 0] = 1
            sig, Mlast = fused.train_signal(D['A'], D['B'], **_kwargs(D), rx=dev(rx), return_last=True)
            assert torch.equal(Mlast, Mt[..., -1, :]), s
            assert torch.equal(sig, Mt[:, s, :, :2].movedim(-1, 1)), s


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_chained_calls_are_one_call(tag):
    r"""``K1 = 5`` repetitions, then ``K2 = S`` from ``Mlast``, against one call of ``K1 + K2`` with the concatenated
    phases.  fp64: the values bit for bit, and so the gradients that no sum over the repetitions splits -- ``grad_Mi``
    (the adjoint state handed from the second call to the first) and ``grad_phase``; ``grad_A, grad_B, grad_rest,
    grad_T1, grad_T2, grad_Δf, grad_rx`` are sums over k that the chain forms as (first call) + (second call) and the
    one call in one chain -- another association of the same terms, held to the gate.  fp32: everything to the gate
    (``Mlast`` is rounded to fp32 between the calls)."""
    N, nM, K1, K2 = 2, 200, 5, S
    K = K1 + K2
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, 3, tag)
    w, v = _loss_weights(P, K, rx)
    one = _run(P, K, rx, w=w, v=v)
    L = {k: dev(P[k]).clone().requires_grad_(True) for k in LEAVES}
    L['rx'] = dev(rx).clone().requires_grad_(True)
    kw = {KW[k]: L[k] for k in ('rest', 'T1', 'T2', 'df')}
    s1, M1 = fused.train_signal(L['A'], L['B'], Mi=L['Mi'], phase=L['phase'][:, :K1], rx=L['rx'], return_last=True, **kw)
    s2, M2 = fused.train_signal(L['A'], L['B'], Mi=M1, phase=L['phase'][:, K1:], rx=L['rx'], return_last=True, **kw)
    sig = torch.cat((s1, s2), dim=2)
    ((sig * dev(w)).sum() + (M2 * dev(v)).sum()).backward()
    two = {'grad_' + k: x.grad for k, x in L.items()}
    two['sig'], two['Mlast'] = sig.detach(), M2.detach()
    if tag == 'f64':
        for k in ('sig', 'Mlast', 'grad_Mi', 'grad_phase'):
            assert torch.equal(two[k], one[k]), k
    _gates(two, {k: x.double().cpu() for k, x in one.items()}, tag, 'chained vs one call')
    _gates(two, _yardstick(P, K, rx, w=w, v=v), tag, 'chained vs the yardstick')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_demodulation(tag):
    r"""``demod=True`` is ``exp(-iφ_k)`` applied in fp64 torch to the plain call's samples, and differentiable."""
    N, nM, K = 2, 100, S + 1
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, 3, tag)
    D = {k: dev(P[k]) for k in LEAVES}
    with torch.no_grad():
        plain = fused.train_signal(D['A'], D['B'], **_kwargs(D), rx=dev(rx))
        dem = fused.train_signal(D['A'], D['B'], **_kwargs(D), rx=dev(rx), demod=True)
    assert dem.shape == plain.shape and dem.dtype == DT[tag]
    _gate(dem.cpu(), demodulated(plain.cpu(), P['phase']), tag, 'demod vs exp(-iφ) in torch')
    # through autograd: the yardstick's demodulated loss
    w, v = _loss_weights(P, K, rx)
    L = {k: P[k].double().clone().requires_grad_(True) for k in LEAVES}
    Mt = torch_train(L['A'], L['B'], K, *(L[k] for k in OPS))
    z = torch_signal(Mt, rx.double())
    φ = L['phase'][:, None, :, None]
    zr, zi = z[:, 0], z[:, 1]
    c, s = torch.cos(φ[:, 0]), torch.sin(φ[:, 0])
    ((torch.stack((zr * c + zi * s, zi * c - zr * s), dim=1) * w.double()).sum() + (Mt[..., -1, :] * v.double()).sum()).backward()
    want = {'grad_' + k: x.grad for k, x in L.items()}
    got = _run(P, K, rx, demod=True)
    _gates(got, want, tag, 'demod', keys=list(want))


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_demodulated_linear_phase_is_an_off_resonance_in_the_rest(tag):
    r"""The set-up of ``test_ab_train.test_linear_phase_is_an_off_resonance_in_the_rest``: ``φ_k = kψ`` with
    ``ψ = 2π rest · 32 Hz``, the demodulated signal is the zero-phase train's at ``Δf + 32 Hz``; the other sign is O(1)
    away.  Held in units of the largest sample (a sum over 100 spins)."""
    Q = _identity(tag)
    K, δ = 24, 32.0
    φ = (2 * π * δ * Q['rest'].double())[:, None] * torch.arange(K, dtype=torch.float64)
    D = {k: dev(v) for k, v in Q.items()}
    rx = dev(_rx(2, 100, 3, tag))
    kw = dict(rest=D['rest'], T1=D['T1'], T2=D['T2'], rx=rx)
    with torch.no_grad():
        back = fused.train_signal(D['A'], D['B'], phase=dev(φ), Δf=D['df'], demod=True, **kw)
        plus = fused.train_signal(D['A'], D['B'], n=K, Δf=D['df'] + δ, **kw)
        minus = fused.train_signal(D['A'], D['B'], n=K, Δf=D['df'] - δ, **kw)
    scale = float(plus.abs().max())
    record(f'train_signal.{tag}.linear_phase_vs_shifted_df',
           max_abs(back, plus) / scale if tag == 'f64' else rel_l2(back, plus))
    _gate(back.cpu() / scale, plus.cpu() / scale, tag, 'demodulated vs the shifted Δf')
    assert max_abs(back, minus) / scale > 0.05


# =============================================================================================
# 6. a cotangent on one sample only
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('j', [0, S, S + 2], ids=['first', 'segment2', 'last'])
def test_cotangent_on_one_sample(tag, j):
    r"""``K = S + 3``; the weights on sample ``j`` alone -- the first, the first of the second checkpoint segment, the
    last -- and none on ``Mlast``: every gradient against the yardstick's, and ``grad_phase[:, k]`` is an exact zero for
    every ``k > j``."""
    N, nM, K = 2, 100, S + 3
    P, _ = _kernel_problem(N, nM, K, tag)
    rx = _rx(N, nM, 3, tag)
    w0, v = _loss_weights(P, K, rx)
    w = torch.zeros_like(w0)
    w[:, :, j] = w0[:, :, j]
    v = torch.zeros_like(v)
    want, got = _yardstick(P, K, rx, w=w, v=v), _run(P, K, rx, w=w, v=v)
    _gates(got, want, tag, f'sample {j}')
    assert float(got['grad_phase'][:, j + 1:].abs().sum()) == 0.0
    assert float(got['grad_phase'][:, j].abs().min()) > 0


# =============================================================================================
# 7. more tiles than partial rows
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _big(tag):
    r"""``N = 2, K = S + 3, nM = 64 P + 100`` with ``P`` the cap on the partial rows, read off the workspace query:
    every wave takes a second tile, the first 100 / 64 of them a third.  Seeded, never modified."""
    N, K = 2, S + 3
    lib = _lib()
    P_ = lib.mrphy_train_signal_workspace(0, 1, 1 << 30, 1, 1) // 8
    assert P_ == lib.mrphy_train_signal_workspace(0, 1, 1 << 29, 1, 1) // 8 and 64 <= P_ <= 1 << 14
    nM = 64 * P_ + 100
    gen = torch.Generator().manual_seed(77)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    P = dict(A=0.97 * Q, B=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             Mi=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             phase=2 * torch.randn((N, K), generator=gen, dtype=torch.float64),
             rest=torch.tensor([5e-3, 6.5e-3], dtype=torch.float64), T1=0.05 + 0.1 * rnd(N, nM),
             T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200)
    rx = 0.5 + torch.randn((N, nM, 2, 2), generator=gen, dtype=torch.float64)
    return {k: x.to(DT[tag]) for k, x in P.items()}, rx.to(DT[tag]), int(P_), K


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('loss', ['full', 'tail'])
def test_more_tiles_than_partial_rows(tag, loss):
    r"""``full``: every spin weighs in, the yardstick on all of them.  ``tail``: ``rx`` is zero on every spin of the
    first ``P`` tiles and ``Mlast`` has no weight there, so the yardstick is the last 100 spins alone -- what the waves
    add into their workspace rows on their later tiles must not disturb nor lose what the earlier tiles left."""
    P, rx, P_, K = _big(tag)
    N, nM = P['A'].shape[:2]
    head = 64 * P_
    w, v = _loss_weights(P, K, rx)
    if loss == 'tail':
        rx = rx.clone()
        rx[:, :head] = 0
        v = v.clone()
        v[:, :head] = 0
        Pt = {k: (x[:, head:] if k in ('A', 'B', 'Mi', 'T1', 'T2', 'df') else x) for k, x in P.items()}
        want = _yardstick(Pt, K, rx[:, head:], w=w, v=v[:, head:])
    else:
        want = _yardstick(P, K, rx, w=w, v=v)
        want = {k: (x[:, head:] if k in ('grad_A', 'grad_B') else x) for k, x in want.items()}
    got = _run(P, K, rx, w=w, v=v)
    got = {k: (x[:, head:] if k in ('grad_A', 'grad_B') else x) for k, x in got.items()}
    _gates(got, want, tag, f'{loss} (P = {P_}, nM = {nM})', keys=('sig', 'grad_A', 'grad_B', 'grad_phase', 'grad_rest'))


# =============================================================================================
# 8. empty problems   9. launch counts
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('what', ['K0', 'nM0'])
def test_empty_problem(tag, what):
    r"""No repetition and no spin: a signal of zeros in its shape, ``Mlast`` = ``Mi``; the backward runs and the
    gradients are zeros of the operands' shapes (at ``K = 0`` ``grad_Mi`` is the cotangent of ``Mlast``)."""
    P, _ = _kernel_problem(2, 100, 7, tag)
    if what == 'K0':
        K, E, rx = 0, dict(P, phase=P['phase'][:, :0]), _rx(2, 100, 3, tag)
    else:
        K, E = 7, {k: (v[:, :0] if k in ('A', 'B', 'Mi', 'T1', 'T2', 'df') else v) for k, v in P.items()}
        rx = _rx(2, 100, 3, tag)[:, :0]
    got = _run(E, K, rx, n=False)
    nM = E['A'].shape[1]
    assert got['sig'].shape == (2, 2, K, 3) and got['sig'].dtype == DT[tag] and float(got['sig'].abs().sum()) == 0.0
    assert got['Mlast'].shape == (2, nM, 3)
    if what == 'K0':
        assert torch.equal(got['Mlast'].cpu(), P['Mi'])
    for k in LEAVES + ('rx',):
        g = got['grad_' + k]
        assert g is not None and g.shape == (rx if k == 'rx' else E[k]).shape and g.dtype == DT[tag], k
        if not (what == 'K0' and k == 'Mi'):
            assert float(g.abs().sum()) == 0.0, k
    if what == 'K0':
        assert torch.equal(got['grad_Mi'].cpu(), _loss_weights(E, K, rx)[1])


def test_one_launch_each_way(monkeypatch):
    names = (FWD, BWD, 'mrphy_ab_train_fwd', 'mrphy_ab_train_bwd')
    calls = _counted(monkeypatch, names)
    P, _ = _kernel_problem(2, 100, 7, 'f32')
    _run(P, 7, _rx(2, 100, 3, 'f32'))
    assert dict(calls) == {FWD: 1, BWD: 1}
    calls.clear()
    lib = _lib()
    seen = []
    inner = getattr(lib, FWD)
    monkeypatch.setattr(lib, FWD, lambda *a: (seen.append(a), inner(*a))[1])
    A = dev(P['A']).requires_grad_(True)
    with torch.no_grad():
        fused.train_signal(A, dev(P['B']), n=3)
    assert dict(calls) == {FWD: 1}
    assert len(seen) == 1 and seen[0][23] is None, 'no_grad: a null checkpoint pointer'
    fused.train_signal(A, dev(P['B']), n=3)
    assert len(seen) == 2 and seen[1][23] is not None, 'a gradient is wanted: checkpoints'


# =============================================================================================
# 10. memory
# =============================================================================================
def test_nothing_of_the_size_of_the_records_is_allocated():
    r"""N = 1, nM = 4096, K = 128 in fp32, ``A``, ``B``, ``T1`` requiring grad: forward + backward raise the allocator's
    peak by less than half the bytes ``Mt`` alone would take (``K · nM · 3 · 4``); the composed route keeps ``Mt`` and
    its cotangent, four times that bound."""
    N, nM, K = 1, 4096, 128
    gen = torch.Generator().manual_seed(9)
    Qm = torch.linalg.qr(torch.randn((N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    A, B = dev((0.97 * Qm).float()).requires_grad_(True), dev(torch.randn((N, nM, 3), generator=gen)).requires_grad_(True)
    T1 = dev(0.05 + 0.1 * torch.rand((N, nM), generator=gen)).requires_grad_(True)
    T2, rest = dev(0.02 + 0.05 * torch.rand((N, nM), generator=gen)), dev(torch.tensor(5e-3))
    phase = dev(2 * torch.randn((N, K), generator=gen))
    w = dev(_sin((N, 2, K), torch.float32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sig = fused.train_signal(A, B, phase=phase, rest=rest, T1=T1, T2=T2)
    sig.backward(w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    records = K * N * nM * 3 * 4
    print(f'peak rise {rise} B; Mt would be {records} B')
    assert A.grad is not None and B.grad is not None and T1.grad is not None and float(T1.grad.abs().max()) > 0
    assert 0 < rise < records // 2, (rise, records)


# =============================================================================================
# 11. train_signal_rfgr end to end on the fixtures
# =============================================================================================
OUT = ('sig', 'grad_rf', 'grad_gr', 'grad_T1')


def _fixture_weights(dtype):
    return _sin((2, 2, 40), dtype, 0.41, 0.2)


def _fixture_run(Q):
    rf, gr, T1 = (dev(Q[k]).requires_grad_(True) for k in ('rf', 'gr', 'T1'))
    γ = dev(Q['γ'])
    sig = fused.train_signal_rfgr(rf, gr, dev(Q['loc']), phase=dev(Q['phase']), rest=dev(Q['rest']), T1=T1,
                                  T2=dev(Q['T2']), Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']))
    (sig * dev(_fixture_weights(sig.dtype))).sum().backward()
    return dict(sig=sig.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad)


def _oracle_signal(P):
    r"""The same by the CPU oracle in fp64: ``O.rfgr2beff -> O.beff2ab -> torch_train -> sum``, and autograd."""
    P = {k: v.double() for k, v in P.items()}
    rf, gr, T1 = (P[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1'))
    beff = O.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = O.beff2ab(beff, E1=torch.exp(-P['dt'][:, None] / T1), E2=torch.exp(-P['dt'][:, None] / P['T2']), γ=P['γ'],
                     dt=P['dt'])
    sig = torch_signal(torch_train(A, B, P['phase'].shape[1], None, P['phase'], P['rest'], T1, P['T2'], P['df']))
    (sig * _fixture_weights(torch.float64)).sum().backward()
    return dict(sig=sig.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad)


@pytest.mark.parametrize('tag_mode', MODES)
def test_against_the_reference_fixture(tag_mode):
    r"""``rx=None`` on the inputs of ``tests/golden/train_{f32,f64}.npz``.  fp64: ``sig`` against the sum over the spins of
    the fixture's ``Mt`` (the reference's simulators) at ``assert_close``'s fp64 gate, and ``grad_rf, grad_gr, grad_T1``
    of a seeded signal loss against the CPU oracle's.  fp32, precise and fast: the distance of ``sig`` to the fp64
    fixture's sum is held to 3 x the distance of the reference's own fp32 fixture's sum (8.0e-7 on the CPU: a bound of
    2.4e-6); every distance goes to the ledger."""
    tag, mode = _mode(tag_mode)
    G, G64 = golden(f'train_{tag}'), golden('train_f64')
    Q = fixture_inputs(G)
    with mode:
        got = _fixture_run(Q)
    assert set(got) == set(OUT) and got['sig'].shape == (2, 2, 40) and got['sig'].dtype == DT[tag]
    sum64 = torch_signal(t(G64['Mt']))
    if tag == 'f64':
        want = _oracle_signal(Q)
        d = record('train_signal.f64.fixture.sig', max_abs(got['sig'], sum64))
        print(f'f64 sig: {d:.3e} max abs from the sum of the reference fixture')
        assert_close(got['sig'], sum64, 'f64', 'sig vs the sum of the reference fixture')
        for k in OUT:
            record(f'train_signal.f64.fixture.{k}.vs_oracle', max_abs(got[k], want[k]))
            _gate(got[k], want[k], 'f64', f'{k} vs the CPU oracle')
        return
    ref = rel_l2(torch_signal(t(G['Mt']).double()), sum64)
    bound = 3 * ref
    record(f'train_signal.{tag_mode}.fixture.sig.reference_f32_vs_fixture64', ref)
    d = record(f'train_signal.{tag_mode}.fixture.sig.vs_fixture64', rel_l2(got['sig'], sum64), bound)
    wide = _oracle_signal(Q)
    for k in OUT:
        record(f'train_signal.{tag_mode}.fixture.{k}.vs_yardstick64_on_the_same_numbers', rel_l2(got[k], wide[k]))
    print(f'{tag_mode} sig: {d:.3e} from the sum of the fp64 fixture, bound {bound:.3e} (the reference: {ref:.3e})')
    assert d <= bound, f'sig: {d:.3e} from the fp64 fixture > 3 x the reference\'s own fp32 distance = {bound:.3e}'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_parallel_transmit_runs_through_the_fused_ab(tag, monkeypatch):
    r"""4 transmit coils with their ``b1Map`` (``test_fused_traj._problem(.., 'ptx4', 48)``), the fixture's rest and
    phases, 8 repetitions, 3 receive coils: ``A, B`` come from ``mrphy_ab_rfgr_mc_fwd``, and the signal is the
    yardstick's on ``beff2ab(rfgr2beff(.))`` of the device."""
    K = 8
    P = _problem(tag, 'ptx4', 48)
    Q = fixture_inputs(golden(f'train_{tag}'))
    rest, phase = dev(Q['rest']), dev(Q['phase'][:, :K].contiguous())
    γ, dt, T1, T2, df = (dev(P[k]) for k in ('γ', 'dt', 'T1', 'T2', 'df'))
    rx = _rx(2, 100, 3, tag)
    E1, E2 = torch.exp(-dt[:, None] / T1), torch.exp(-dt[:, None] / T2)
    consts = dict(γ2πdt=2 * π * _host.pad_trailing(γ, 2) * _host.pad_trailing(dt, 2), E1=E1, E2=E2, E1_1=E1 - 1)
    calls = _counted(monkeypatch, ('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd', 'mrphy_beff2ab', FWD, 'mrphy_ab_train_fwd'))
    with torch.no_grad():
        sig = fused.train_signal_rfgr(dev(P['rf']), dev(P['gr']), dev(P['loc']), phase=phase, rest=rest, T1=T1, T2=T2,
                                      Δf=df, rx=dev(rx), b1Map=dev(P['b1']), γ_beff=γ, consts=consts)
        assert dict(calls) == {'mrphy_ab_rfgr_mc_fwd': 1, FWD: 1}
        beff = beffective.rfgr2beff(dev(P['rf']), dev(P['gr']), dev(P['loc']), Δf=df, b1Map=dev(P['b1']), γ=γ)
        A, B = beffective.beff2ab(beff, E1=E1, E2=E2, γ=γ, dt=dt)
        want = torch_signal(torch_train(A.double(), B.double(), K, None, phase.double(), rest.double(), T1.double(),
                                        T2.double(), df.double()).cpu(), rx.double())
    assert sig.shape == (2, 2, K, 3) and sig.dtype == DT[tag]
    _gate(sig.cpu(), want, tag, 'sig under parallel transmit')
