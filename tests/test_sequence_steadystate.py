r"""``fused.sequence_steadystate`` (Ksqp, Ksqpl + Ksqsb: ``mrphy_sequence_steadystate_fwd`` / ``_bwd``) and
``fused.sequence_steadystate_rfgr`` on the device.

The yardstick is fp64 torch on the CPU on the same numbers, never the new code: ``test_ab_sequence_host.torch_sequence`` on
the start vectors ``0, e_x, e_y, e_z`` gives ``Ā, b̄``, ``torch.linalg.solve`` gives ``Mss`` and autograd of ``(Mss w).sum()``
the gradients (``test_sequence_steadystate_host.torch_steadystate``).  The kernels carry the period, the solve and every
sum in fp64 and round each output once, so they are held to the kernel-alone gates of ``test_steadystate._gate``: fp64
max abs 1e-9 (a gradient in units of the yardstick's largest element), fp32 relative L2 1e-6.  The shapes are
``test_sequence_signal.PROBLEMS`` seeded by its ``_kernel_problem`` (``A = 0.97 Q``: the condition number of ``I - Ā`` is at
most 1.8 at K = 11 and at most 1 / 0.03 at K = 1).  End to end in fp32 (§10) ``Mss`` inherits the rounding of ``A, B`` and is
held to three times what the same CPU route loses when it runs entirely in fp32, the margin and reason of
``test_ab_sequence.py`` §8.  Every distance goes to the ledger under ``seqss.*``.
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_ab_rfgr import _counted
from test_ab_rfgr_host import fixture_inputs
from test_ab_sequence import KW, _table
from test_ab_sequence_host import oracle_bank, torch_sequence
from test_ab_train import _same_bits
from test_fused_traj import _problem as _pulse_problem
from test_sequence_signal import PROBLEMS, S, _kernel_problem
from test_sequence_steadystate_host import torch_steadystate
from test_steadystate import _form, _gate, _mode
from test_steadystate import _kernel_problem as _pulse_steady_problem
from test_train_signal import _sin
from test_train_signal_host import torch_signal

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
FWD, BWD = 'mrphy_sequence_steadystate_fwd', 'mrphy_sequence_steadystate_bwd'
OTHERS = ('mrphy_ab_sequence_fwd', 'mrphy_ab_sequence_bwd', 'mrphy_sequence_signal_fwd', 'mrphy_ab_train_fwd',
          'mrphy_ab_train_bwd')
OPS = ('phase', 'rest', 'T1', 'T2', 'df')               # the optional operands; there is no Mi
LEAVES = ('A', 'B') + OPS
RUN = 'run'


def _weights(P):
    return _sin(tuple(P['B'].shape[1:]), P['A'].dtype)


def _yardstick(P, K, use=OPS, w=None, pulse=None):
    r"""``Mss`` and the gradients of ``(Mss w).sum()`` w.r.t. ``A, B`` and the operands ``use`` in fp64 on the CPU; operands
    not in ``use`` are absent."""
    w = _weights(P) if w is None else w
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    ops = {k: L.get(k) for k in OPS}
    if ops['rest'] is not None:
        ops['rest'] = _table(ops['rest'], K)
    Mss = torch_steadystate(L['A'], L['B'], K, P['pulse'] if pulse is None else pulse, *(ops[k] for k in OPS))
    (Mss * w.double()).sum().backward()
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['Mss'] = Mss.detach()
    return out


@functools.lru_cache(maxsize=None)
def _cached_yardstick(name, tag):
    return _yardstick(_kernel_problem(name, tag), PROBLEMS[name][0][3])


def _run(P, K, use=OPS, over=None, w=None, leaves=None, pulse=None):
    r"""The same through ``fused.sequence_steadystate`` on the device; ``over``: tensors that replace operands;
    ``leaves``: the names of the operands that require grad (all by default; the others' gradients come back ``None``)."""
    w = _weights(P) if w is None else w
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    Mss = fused.sequence_steadystate(L['A'], L['B'], pulse=list(P['pulse'] if pulse is None else pulse),
                                     **{KW[k]: L[k] for k in use})
    if Mss.requires_grad:
        (Mss * dev(w).reshape(Mss.shape)).sum().backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['Mss'] = Mss.detach()
    return out


def _gates(got, want, tag, what, keys=None, ledger=None):
    for k in (keys or want):
        ma, rl = max_abs(got[k], want[k]), rel_l2(got[k], want[k])
        print(f'{tag} {what} {k}: max abs {ma:.3e} rel-L2 {rl:.3e}')
        if ledger:
            record(f'seqss.{tag}.{ledger}.{k}', ma if tag == 'f64' else rl)
    for k in (keys or want):
        _gate(got[k], want[k], tag, f'{what}: {k}')


# =============================================================================================
# 1. values and all seven gradients
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_kernels_alone_against_the_fp64_solve(tag, name):
    r"""``one``: one row, a period of one repetition.  ``K2``: a ragged block per batch entry.  ``run`` / ``change`` at
    ``K = S + 3``: the second walk leaves a second checkpoint, with an equal run across the boundary / a change of pulse
    and of rest exactly at it; entry 1 is never played: its ``grad_A``, ``grad_B`` are exact zeros.  ``K40``: five
    checkpoints.  ``blocks2``: two blocks, the second ragged.  A second run gives the same bits."""
    (P_, N, nM, K), _ = PROBLEMS[name]
    P = _kernel_problem(name, tag)
    want = _cached_yardstick(name, tag)
    got = _run(P, K)
    assert set(got) == set(want)
    assert got['Mss'].dtype == DT[tag] and got['Mss'].shape == (N, nM, 3)
    _gates(got, want, tag, name, ledger=name)
    for k in LEAVES:
        g = got['grad_' + k]
        assert g.shape == P[k].shape and g.dtype == DT[tag] and float(g.abs().max()) > 0, k
    for p in range(P_):
        for k in ('A', 'B'):
            g = got['grad_' + k]
            if p in P['pulse']:
                assert float(g[p].abs().min()) > 0, (k, p)
            else:
                assert torch.equal(g[p], torch.zeros_like(g[p])), f'grad_{k}[{p}]: the schedule never plays it'
    if name in ('run', 'change'):
        assert 1 not in P['pulse']
    _same_bits(got, _run(P, K), 'a second run')


# =============================================================================================
# 2. absent operands and operand forms
# =============================================================================================
ABSENT = {
    'norest': ('phase',),
    'rest-noT': ('phase', 'rest', 'df'),
    'rest-nodf': ('phase', 'rest', 'T1', 'T2'),
    'nophase': ('rest', 'T1', 'T2', 'df'),
}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(ABSENT))
def test_absent_operands(tag, case):
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    use = ABSENT[case]
    want, got = _yardstick(P, K, use), _run(P, K, use)
    assert set(got) == set(want) == {'Mss', 'grad_A', 'grad_B'} | {'grad_' + k for k in use}
    _gates(got, want, tag, case, ledger=case)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', 'N', '1K', 'NK'])
def test_forms_of_rest(tag, form):
    r"""``rest`` as `()`, `(N,)`, `(1, K)`, `(N, K)`: the bits of the call with the table written out as `(N, K)`; the
    gradient has the operand's shape and is the yardstick's on that form."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    full = P['rest']
    x = {'0dim': full[0, 2], 'N': full[:, 2], '1K': full[:1], 'NK': full}[form].clone()
    mat = _run(dict(P, rest=_table(x, K).expand(N, K).contiguous()), K)
    got = _run(P, K, over=dict(rest=dev(x)))
    for k in mat:
        if k != 'grad_rest':
            assert torch.equal(got[k], mat[k]), (form, k)
    g = got['grad_rest']
    assert g.shape == x.shape and g.dtype == x.dtype and float(g.abs().min()) > 0
    _gates(got, _yardstick(dict(P, rest=x), K), tag, f'rest {form}', keys=['grad_rest'], ledger=f'rest_{form}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_operand_forms_of_the_spin_constants(tag, form):
    r"""``T1``, ``T2``, ``Δf`` in every broadcast form and ``phase`` `(1, K)`: the bits of the materialised call; each
    gradient has its operand's shape and is the materialised call's summed."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    (T1, T1m), (T2, T2m), (df, dfm) = (_form(P[k], form) for k in ('T1', 'T2', 'df'))
    phase = P['phase'][:1].clone()
    mat = _run(dict(P, T1=T1m, T2=T2m, df=dfm, phase=phase.expand(N, K).contiguous()), K)
    got = _run(P, K, over=dict(T1=T1, T2=T2, df=df, phase=dev(phase)))
    for k in ('Mss', 'grad_A', 'grad_B', 'grad_rest'):
        assert torch.equal(got[k], mat[k]), (form, k)
    for k, x in (('T1', T1), ('T2', T2), ('df', df), ('phase', phase)):
        g, m = got['grad_' + k], mat['grad_' + k]
        assert g.shape == x.shape and g.dtype == x.dtype, (form, k, g.shape)
        shp = tuple(x.shape) + (1,) * (m.ndim - x.ndim) if x.ndim else (1,) * m.ndim
        _gate(g, m.double().cpu().sum_to_size(shp).reshape(x.shape), tag, f'{form}: grad_{k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_offset_and_strided_operands_and_a_bank_that_is_a_view(tag):
    r"""Every operand a view into a larger buffer -- a storage offset, ``T1, T2, Δf`` strided besides --, the bank an
    ``.unflatten`` view: the bits of the plain call, the gradients in the operands' shapes."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    base = _run(P, K)

    def offset(x):                     # contiguous, 3 elements into a larger buffer
        buf = dev(torch.zeros(x.numel() + 5, dtype=x.dtype))
        view = buf[3:3 + x.numel()].view(x.shape)
        view.copy_(dev(x))
        return view.detach()

    def strided(x):                    # every other element of the last axis of a buffer twice as wide
        buf = dev(torch.zeros(tuple(x.shape[:-1]) + (2 * x.shape[-1],), dtype=x.dtype))
        view = buf[..., 1::2]
        view.copy_(dev(x))
        return view.detach()
    over = {k: offset(P[k]) for k in ('phase', 'rest')}
    over.update({k: strided(P[k]) for k in ('T1', 'T2', 'df')})
    over.update(A=offset(P['A'].flatten(0, 1)), B=offset(P['B'].flatten(0, 1)))
    assert all(not over[k].is_contiguous() for k in ('T1', 'T2', 'df')) and over['A'].storage_offset() == 3
    L = {k: x.requires_grad_(True) for k, x in over.items()}
    Mss = fused.sequence_steadystate(L['A'].unflatten(0, (P_, N)), L['B'].unflatten(0, (P_, N)), pulse=P['pulse'],
                                     **{KW[k]: L[k] for k in OPS})
    (Mss * dev(_weights(P))).sum().backward()
    assert torch.equal(Mss, base['Mss'])
    for k in LEAVES:
        g = L[k].grad
        assert g.shape == L[k].shape, k
        assert torch.equal(g.reshape(base['grad_' + k].shape), base['grad_' + k]), k


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)``: the bits of the flat `(N, 100)` call, the gradients in the operands' shapes."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    flat = _run(P, K)
    Q = dict(P, A=P['A'].reshape(P_, N, 10, 10, 3, 3), B=P['B'].reshape(P_, N, 10, 10, 3),
             T1=P['T1'].reshape(N, 10, 10), T2=P['T2'].reshape(N, 10, 10), df=P['df'].reshape(N, 10, 10))
    got = _run(Q, K, w=_weights(P).reshape(N, 10, 10, 3))
    assert got['Mss'].shape == (N, 10, 10, 3) and torch.equal(got['Mss'].reshape(N, 100, 3), flat['Mss'])
    for k in ('A', 'B', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert torch.equal(got['grad_phase'], flat['grad_phase']) and torch.equal(got['grad_rest'], flat['grad_rest'])


# =============================================================================================
# 3. partial requests
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('leaf', LEAVES)
def test_each_leaf_alone(tag, leaf):
    r"""One operand requires grad: its gradient is the yardstick's, the others come back ``None``."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    got = _run(P, K, leaves=(leaf,))
    want = _cached_yardstick(RUN, tag)
    for k in LEAVES:
        assert (got['grad_' + k] is None) == (k != leaf), k
    _gates(got, want, tag, f'{leaf} alone', keys=('Mss', 'grad_' + leaf))
    if leaf in ('A', 'B'):
        assert torch.equal(got['grad_' + leaf][1], torch.zeros_like(got['grad_' + leaf][1]))


def test_without_a_gradient_wanted_nothing_is_left_for_the_adjoint(monkeypatch):
    r"""No leaf requires grad, or ``no_grad``: the forward gets null pointers for ``per`` and ``ck`` (arguments 19, 20);
    with a leaf it gets both."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, 'f32')
    lib = mrphy_amd.require_library()
    seen = []
    inner = getattr(lib, FWD)
    monkeypatch.setattr(lib, FWD, lambda *a: (seen.append(a), inner(*a))[1])
    got = _run(P, K, leaves=())
    assert all(got['grad_' + k] is None for k in LEAVES) and not got['Mss'].requires_grad
    A = dev(P['A']).requires_grad_(True)
    with torch.no_grad():
        fused.sequence_steadystate(A, dev(P['B']), pulse=P['pulse'])
    assert len(seen) == 2 and all(s[19] is None and s[20] is None for s in seen)
    Mss = fused.sequence_steadystate(A, dev(P['B']), pulse=P['pulse'])
    assert len(seen) == 3 and seen[2][19] is not None and seen[2][20] is not None and Mss.requires_grad
    assert torch.equal(Mss.detach(), fused.sequence_steadystate(A.detach(), dev(P['B']), pulse=P['pulse']))


# =============================================================================================
# 4. the fixed point on the device
# =============================================================================================
def _kwargs(D, use=OPS):
    return {KW[k]: D[k] for k in use}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['run', 'K40'])
def test_one_more_period_returns_to_the_steady_state(tag, name):
    r"""``ab_sequence(…, Mi=Mss)``: its last record is ``Mss``, and its record 0 is the steady state of the period shifted
    by one repetition; the period played twice has the same steady state.  All at the gate."""
    (P_, N, nM, K), _ = PROBLEMS[name]
    P = _kernel_problem(name, tag)
    D = {k: dev(P[k]) for k in LEAVES}
    roll = lambda x: torch.roll(x, -1, dims=1)  # noqa: E731
    with torch.no_grad():
        Mss = fused.sequence_steadystate(D['A'], D['B'], pulse=P['pulse'], **_kwargs(D))
        Mt = fused.ab_sequence(D['A'], D['B'], pulse=P['pulse'], Mi=Mss, **_kwargs(D))
        shifted = fused.sequence_steadystate(D['A'], D['B'], pulse=P['pulse'][1:] + P['pulse'][:1], phase=roll(D['phase']),
                                             rest=roll(D['rest']), T1=D['T1'], T2=D['T2'], Δf=D['df'])
        twice = fused.sequence_steadystate(D['A'], D['B'], pulse=P['pulse'] * 2, phase=D['phase'].repeat(1, 2),
                                           rest=D['rest'].repeat(1, 2), T1=D['T1'], T2=D['T2'], Δf=D['df'])
    for what, a, b in (('last record', Mt[..., -1, :], Mss), ('record 0 vs the shifted period', Mt[..., 0, :], shifted),
                       ('doubled period', twice, Mss)):
        record(f'seqss.{tag}.fixed_point.{name}.{what.replace(" ", "_")}', max_abs(a, b) if tag == 'f64' else rel_l2(a, b))
        _gate(a, b.double().cpu(), tag, what)
    assert float((shifted - Mss).abs().max()) > 1e-3, 'the shift moves the state'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_period_of_one_pulse_is_ab_steadystate(tag):
    r"""``K = 1, P = 1``, no phase, one rest `(N,)`: ``sequence_steadystate`` and ``ab_steadystate`` on the same numbers, both
    against the yardstick, values and gradients."""
    N, nM = 2, 200
    P = _kernel_problem('K40', tag)
    Q = dict(A=P['A'][:1], B=P['B'][:1], rest=P['rest'][:, 2].clone(), T1=P['T1'], T2=P['T2'], df=P['df'], pulse=(0,))
    use = ('rest', 'T1', 'T2', 'df')
    want = _yardstick(Q, 1, use)
    got = _run(Q, 1, use)
    _gates(got, want, tag, 'K = 1', ledger='K1')
    L = {k: dev(Q[k]).clone().requires_grad_(True) for k in ('A', 'B') + use}
    Mss = fused.ab_steadystate(L['A'][0], L['B'][0], **_kwargs(L, use))
    (Mss * dev(_weights(Q))).sum().backward()
    old = {'grad_' + k: x.grad for k, x in L.items()}
    old['Mss'] = Mss.detach()
    _gates(old, want, tag, 'ab_steadystate')
    _gates(got, {k: x.double().cpu() for k, x in old.items()}, tag, 'K = 1 vs ab_steadystate')


# =============================================================================================
# 5. determinism
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_spin_does_not_depend_on_its_neighbours(tag):
    r"""The first 100 spins of ``blocks2`` run alone: ``Mss`` and every per-spin gradient have the bits they have in the
    full call (the sums over the spins, ``grad_phase`` and ``grad_rest``, have other terms); two runs give equal outputs."""
    (P_, N, nM, K), _ = PROBLEMS['blocks2']
    P = _kernel_problem('blocks2', tag)
    w = _weights(P)
    full = _run(P, K, w=w)
    _same_bits(full, _run(P, K, w=w), 'a second run')
    H = {k: (v[:, :, :100] if k in ('A', 'B') else v[:, :100] if k in ('T1', 'T2', 'df') else v) for k, v in P.items()}
    head = _run({k: (v.contiguous() if isinstance(v, torch.Tensor) else v) for k, v in H.items()}, K, w=w[:, :100].contiguous())
    assert torch.equal(head['Mss'], full['Mss'][:, :100])
    for k in ('A', 'B'):
        assert torch.equal(head['grad_' + k], full['grad_' + k][:, :, :100]), k
    for k in ('T1', 'T2', 'df'):
        assert torch.equal(head['grad_' + k], full['grad_' + k][:, :100]), k


# =============================================================================================
# 6. RF spoiling
# =============================================================================================
def _spoiling_phase(K, N=2):
    k = torch.arange(K, dtype=torch.int64)
    deg = (117 * k * (k + 1) // 2) % 360                     # exact: 117 k (k + 1) / 2 degrees modulo a turn
    return (deg.double() * (π / 180)).expand(N, K).contiguous()


def test_rf_spoiling_has_a_period_of_80():
    r"""fp64, ``N = 2, nM = 100``, the quadratic 117° schedule, one rest of 5 ms: ``Mss`` of the 80-repetition period against
    the yardstick and against ``ab_train`` over six periods, which contract by at most (0.97 e^(-5 ms / 0.15 s))^480 ≈
    5e-14 on the seeded constants; 40 repetitions are not a period."""
    P, _ = _pulse_steady_problem(2, 100, 'f64')
    assert float(P['T1'].max()) <= 0.15
    φ80, φ480 = _spoiling_phase(80), _spoiling_phase(480)
    assert torch.equal(φ480[:, 80:160], φ80) and not torch.equal(φ80[:, 40:], φ80[:, :40])
    rest = torch.tensor(5e-3, dtype=torch.float64)
    A, B, T1, T2, df = (dev(P[k]) for k in ('A', 'B', 'T1', 'T2', 'df'))
    with torch.no_grad():
        Mss = fused.sequence_steadystate(A[None], B[None], phase=dev(φ80), rest=dev(rest), T1=T1, T2=T2, Δf=df)
        Mt = fused.ab_train(A, B, n=480, phase=dev(φ480), rest=dev(rest), T1=T1, T2=T2, Δf=df)
        half = fused.sequence_steadystate(A[None], B[None], phase=dev(φ80[:, :40]), rest=dev(rest), T1=T1, T2=T2, Δf=df)
    want = torch_steadystate(P['A'][None], P['B'][None], 80, None, φ80, rest.reshape(1, 1).expand(1, 80), P['T1'], P['T2'],
                             P['df'])
    record('seqss.f64.spoiling.vs_yardstick', max_abs(Mss, want))
    record('seqss.f64.spoiling.vs_six_periods_of_ab_train', max_abs(Mss, Mt[..., -1, :]))
    _gate(Mss, want, 'f64', 'Mss of the 80-repetition period')
    _gate(Mss, Mt[..., -1, :].cpu(), 'f64', 'Mss vs ab_train over 480 repetitions')
    assert float((half - Mss).abs().max()) > 1e-4, '40 repetitions are not a period'


# =============================================================================================
# 7. chaining into sequence_signal
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_the_signal_of_the_steady_period_is_differentiable_through_Mi(tag):
    r"""``sequence_signal(A, B, Mi=sequence_steadystate(A, B, …), …)`` with ``(sig w).sum().backward()``: the gradients w.r.t.
    ``A, B, T1`` -- each the sum of the path through the period and the path through ``Mi`` -- against the yardstick's
    autograd of the same composition."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    w = _sin((N, 2, K), DT[tag])
    names = ('A', 'B', 'T1')
    L = {k: dev(P[k]).clone().requires_grad_(k in names) for k in LEAVES}
    Mss = fused.sequence_steadystate(L['A'], L['B'], pulse=P['pulse'], **_kwargs(L))
    sig = fused.sequence_signal(L['A'], L['B'], pulse=P['pulse'], Mi=Mss, **_kwargs(L))
    (sig * dev(w)).sum().backward()
    got = {'grad_' + k: L[k].grad for k in names}
    got['sig'] = sig.detach()
    Y = {k: P[k].double().clone().requires_grad_(k in names) for k in LEAVES}
    ops = (Y['phase'], Y['rest'], Y['T1'], Y['T2'], Y['df'])
    Mi = torch_steadystate(Y['A'], Y['B'], K, P['pulse'], *ops)
    osig = torch_signal(torch_sequence(Y['A'], Y['B'], K, P['pulse'], Mi, *ops), None)
    (osig * w.double()).sum().backward()
    want = {'grad_' + k: Y[k].grad for k in names}
    want['sig'] = osig.detach()
    _gates(got, want, tag, 'chained', ledger='chained')


# =============================================================================================
# 8. one call each way
# =============================================================================================
@pytest.mark.parametrize('name', ['K40', 'run', 'one'])
def test_one_call_each_way_whatever_the_schedule(name, monkeypatch):
    (P_, N, nM, K), _ = PROBLEMS[name]
    calls = _counted(monkeypatch, (FWD, BWD) + OTHERS)
    _run(_kernel_problem(name, 'f32'), K)
    assert dict(calls) == {FWD: 1, BWD: 1}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_parallel_transmit_runs_through_the_fused_ab(tag, monkeypatch):
    r"""4 transmit coils with their ``b1Map`` as a bank of two pulses -- the second at 0.6 of the first --, the fixture's
    rests and phases, a period of 8: ``A, B`` come from ONE ``mrphy_ab_rfgr_mc_fwd`` call on the batch ``P·N``, and ``Mss``
    is the yardstick's on ``beff2ab(rfgr2beff(.))`` of the device, entry by entry."""
    K, pulse = 8, [0, 1, 1, 0, 1, 0, 0, 1]
    P = _pulse_problem(tag, 'ptx4', 48)
    Q = fixture_inputs(golden(f'sequence_{tag}'))
    rest, phase = dev(Q['rest'][:, :K].contiguous()), dev(Q['phase'][:, :K].contiguous())
    γ, dt, T1, T2, df = (dev(P[k]) for k in ('γ', 'dt', 'T1', 'T2', 'df'))
    rf = torch.stack((dev(P['rf']), 0.6 * dev(P['rf'])))
    E1, E2 = torch.exp(-dt[:, None] / T1), torch.exp(-dt[:, None] / T2)
    consts = dict(γ2πdt=2 * π * _host.pad_trailing(γ, 2) * _host.pad_trailing(dt, 2), E1=E1, E2=E2, E1_1=E1 - 1)
    calls = _counted(monkeypatch, ('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd', 'mrphy_beff2ab', FWD) + OTHERS)
    with torch.no_grad():
        Mss = fused.sequence_steadystate_rfgr(rf, dev(P['gr'])[None], dev(P['loc']), pulse=pulse, phase=phase, rest=rest,
                                              T1=T1, T2=T2, Δf=df, b1Map=dev(P['b1']), γ_beff=γ, consts=consts)
        assert dict(calls) == {'mrphy_ab_rfgr_mc_fwd': 1, FWD: 1}
        AB = [beffective.beff2ab(beffective.rfgr2beff(rf[p], dev(P['gr']), dev(P['loc']), Δf=df, b1Map=dev(P['b1']), γ=γ),
                                 E1=E1, E2=E2, γ=γ, dt=dt) for p in range(2)]
        A, B = torch.stack([a for a, _ in AB]).double().cpu(), torch.stack([b for _, b in AB]).double().cpu()
        want = torch_steadystate(A, B, K, pulse, phase.double().cpu(), rest.double().cpu(), T1.double().cpu(),
                                 T2.double().cpu(), df.double().cpu())
    assert Mss.shape == (2, 100, 3) and Mss.dtype == DT[tag]
    _gate(Mss.cpu(), want, tag, 'Mss under parallel transmit')


# =============================================================================================
# 9. no spins
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_problem_without_spins(tag, monkeypatch):
    r"""``nM = 0``: an empty ``Mss``, the backward runs, the gradients are empty or zeros in the operands' shapes, and no
    kernel of another family stands in."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    E = {k: (v[:, :, :0] if k in ('A', 'B') else v[:, :0] if k in ('T1', 'T2', 'df') else v) for k, v in P.items()}
    calls = _counted(monkeypatch, OTHERS)
    got = _run(E, K, w=torch.zeros((N, 0, 3), dtype=DT[tag]))
    assert not calls
    assert got['Mss'].shape == (N, 0, 3) and got['Mss'].dtype == DT[tag]
    for k in LEAVES:
        g = got['grad_' + k]
        assert g is not None and g.shape == E[k].shape and g.dtype == DT[tag] and float(g.abs().sum()) == 0.0, k


# =============================================================================================
# 10. sequence_steadystate_rfgr end to end on the fixtures
# =============================================================================================
OUT = ('Mss', 'grad_rf', 'grad_gr', 'grad_T1', 'grad_rest')


def _fixture_weights(Q):
    return Q['w'][0]


@functools.lru_cache(maxsize=None)
def _fixture_yardstick(tag, K, dtype):
    r"""``oracle_bank`` + compose + solve and autograd of ``(Mss w).sum()`` on the CPU, on the inputs of the fixture ``tag``
    cut to a period of ``K`` repetitions, everything in ``dtype``."""
    Q = fixture_inputs(golden(f'sequence_{tag}'))
    Q = {k: (v if k == 'pulse' else v.to(dtype)) for k, v in Q.items()}
    rf, gr, T1, rest = (Q[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    A, B = oracle_bank(Q, rf, gr, T1)
    Mss = torch_steadystate(A, B, K, Q['pulse'].tolist()[:K], Q['phase'][:, :K], rest[:, :K], T1, Q['T2'], Q['df'])
    (Mss * _fixture_weights(Q)).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)


def _fixture_run(Q, K):
    rf, gr, T1, rest = (dev(Q[k]).requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    γ = dev(Q['γ'])
    Mss = fused.sequence_steadystate_rfgr(rf, gr[None], dev(Q['loc']), pulse=Q['pulse'][:K], phase=dev(Q['phase'])[:, :K],
                                          rest=rest[:, :K], T1=T1, T2=dev(Q['T2']), Δf=dev(Q['df']), b1Map=dev(Q['b1']),
                                          γ_beff=γ, γ=γ, dt=dev(Q['dt']))
    (Mss * dev(_fixture_weights(Q))).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)


@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('K', [24, 3])
def test_against_the_oracle_on_the_fixture_inputs(tag_mode, K):
    r"""The inputs of ``tests/golden/sequence_{f32,f64}.npz``, the period being the fixture's 24 repetitions and also its
    first 3 (``cond(I - Ā)`` is 1.002 at 24: the short period is there so that the solve matters).  fp64 at the project's
    gate.  fp32, precise and fast: the distance to the fp64 yardstick on the same numbers is held to 3 x what the same
    CPU route loses when it runs entirely in fp32, computed here each time (1.4e-6 for ``Mss`` to 6.4e-6 for ``grad_rest`` at
    K = 24); every distance goes to the ledger."""
    tag, mode = _mode(tag_mode)
    Q = fixture_inputs(golden(f'sequence_{tag}'))
    with mode:
        got = _fixture_run(Q, K)
    want = _fixture_yardstick(tag, K, torch.float64)
    assert set(got) == set(OUT) and got['Mss'].shape == (2, 100, 3)
    assert got['grad_rf'].shape == (3, 2, 2, 48) and got['grad_gr'].shape == (2, 3, 48) and got['grad_rest'].shape == (2, 24)
    assert float(got['grad_rest'][:, K:].abs().sum()) == 0.0 and float(got['grad_rest'][:, :K].abs().min()) > 0
    if tag == 'f64':
        for k in OUT:
            d = record(f'seqss.f64.fixture.K{K}.{k}', max_abs(got[k], want[k]))
            print(f'f64 K {K} {k}: {d:.3e} max abs from the oracle')
        for k in OUT:
            _gate(got[k], want[k], 'f64', f'{k} vs the oracle')
        return
    narrow = _fixture_yardstick(tag, K, torch.float32)
    bounds = {}
    for k in OUT:
        ref = record(f'seqss.{tag_mode}.fixture.K{K}.{k}.cpu_route_in_f32_vs_f64', rel_l2(narrow[k], want[k]))
        bounds[k] = 3 * ref
        d = record(f'seqss.{tag_mode}.fixture.K{K}.{k}.vs_yardstick64', rel_l2(got[k], want[k]), bounds[k])
        print(f'{tag_mode} K {K} {k}: {d:.3e} from the fp64 yardstick, bound {bounds[k]:.3e} (the CPU route in fp32: {ref:.3e})')
    for k in OUT:
        d = rel_l2(got[k], want[k])
        assert d <= bounds[k], f'{k}: {d:.3e} from the fp64 yardstick > 3 x the all-fp32 CPU route\'s distance = {bounds[k]:.3e}'


# =============================================================================================
# 11. memory
# =============================================================================================
def test_nothing_of_the_size_of_the_records_is_allocated():
    r"""P = 2, N = 1, nM = 4096, K = 256 in fp32 with ``A``, ``B``, ``T1`` requiring grad: forward + backward raise the
    allocator's peak by less than ``Mss`` and its cotangent + ``per`` + ``ck`` + ``λ`` + the bank's gradients + the two
    queried workspaces + 1 MB; one set of records (``K · nM · 3 · 4`` = 12.6 MB) would not fit."""
    P_, N, nM, K = 2, 1, 4096, 256
    lib = mrphy_amd.require_library()
    gen = torch.Generator().manual_seed(9)
    Qm = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    A = dev((0.97 * Qm).float().contiguous()).requires_grad_(True)
    B = dev(torch.randn((P_, N, nM, 3), generator=gen)).requires_grad_(True)
    T1 = dev(0.05 + 0.1 * torch.rand((N, nM), generator=gen)).requires_grad_(True)
    T2 = dev(0.02 + 0.05 * torch.rand((N, nM), generator=gen))
    rest = dev(2e-3 + 8e-3 * torch.rand((N, K), generator=gen))
    phase = dev(2 * torch.randn((N, K), generator=gen))
    pulse = [(k // 3) % P_ for k in range(K)]
    w = dev(_sin((N, nM, 3), torch.float32))
    rows = N * nM
    small = rows * 3 * 4
    allowed = 2 * small + 12 * rows * 8 + -(-K // S) * rows * 3 * 8 + small + P_ * rows * 12 * 4 + \
        lib.mrphy_sequence_signal_workspace(0, N, nM, K, 1) + lib.mrphy_sequence_signal_bank_workspace(0, P_, N, nM) + (1 << 20)
    records = K * rows * 3 * 4
    assert allowed < records
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Mss = fused.sequence_steadystate(A, B, pulse=pulse, phase=phase, rest=rest, T1=T1, T2=T2)
    Mss.backward(w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f'peak rise {rise} B, allowed {allowed} B; one set of records would be {records} B')
    assert A.grad is not None and B.grad is not None and float(T1.grad.abs().max()) > 0
    assert 0 < rise < allowed, (rise, allowed, records)
