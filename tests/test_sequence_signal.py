r"""``fused.sequence_signal`` (Ksqs / Ksqsb: ``mrphy_sequence_signal_fwd`` / ``_bwd``) and ``fused.sequence_signal_rfgr`` on
the device.

The yardstick is fp64 torch on the CPU on the same numbers: ``test_ab_sequence_host.torch_sequence``, then the complex
sum ``test_train_signal_host.torch_signal``, then autograd of ``(sig w).sum() + (Mlast v).sum()``; never the new code or a
composed device route.  The kernels carry the recursion and every sum in fp64 and round each output once, so they are
held to the kernel-alone gates of ``test_steadystate._gate``: fp64 max abs 1e-9 (a gradient in units of the yardstick's
largest element), fp32 relative L2 1e-6.  Where the design promises the bits of a sibling (``train_signal`` without a
schedule, ``ab_sequence``'s last record, a coil alone) the comparison is ``torch.equal``.  End to end in fp32 (§7) the
signal inherits the rounding of ``A`` amplified by the train's conditioning and is held to three times what the
reference's own all-fp32 route loses, the margin and reason of ``test_ab_sequence.py`` §8.  Every distance goes to the
ledger under ``seqsig.*``.
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_ab_rfgr import _counted
from test_ab_rfgr_host import fixture_inputs
from test_ab_sequence import KW, OPS, _table
from test_ab_sequence import _kernel_problem as _sequence_problem
from test_ab_sequence_host import oracle_bank, torch_sequence
from test_ab_train import ABSENT, _same_bits
from test_fused_traj import _problem as _pulse_problem
from test_steadystate import _form, _gate, _mode
from test_train_signal import _rx, _sin
from test_train_signal_host import demodulated, torch_signal

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
FWD, BWD = 'mrphy_sequence_signal_fwd', 'mrphy_sequence_signal_bwd'
BANK = 'mrphy_sequence_signal_bank_workspace'
OTHERS = ('mrphy_ab_sequence_fwd', 'mrphy_ab_sequence_bwd', 'mrphy_train_signal_fwd', 'mrphy_train_signal_bwd',
          'mrphy_ab_train_fwd', 'mrphy_ab_train_bwd')
LEAVES = ('A', 'B') + OPS


def _lib():
    return mrphy_amd.require_library()


S = int(_lib().mrphy_train_signal_ck_every())           # repetitions per checkpoint segment of the adjoint
assert S >= 4


def _cycle(n):
    return tuple((0, 2, 2, 0, 0, 2, 0)[i % 7] for i in range(n))


# name -> (P, N, nM, K), the schedule (None: test_ab_sequence's for that shape).  The issue's third shape asks for a run
# across the segment boundary k = S-1 | S and for a change of pulse (and of rest) exactly at k = S: one boundary cannot
# be both, so the shape comes twice.  Entry 1 is never played in either.
PROBLEMS = {
    'one': ((1, 1, 1, 1), None),
    'K2': ((2, 2, 100, 2), None),
    'run': ((3, 2, 100, S + 3), _cycle(S - 1) + (0, 0, 2, 0)),          # pulse[S-1] == pulse[S]; back to 0 after the 2
    'change': ((3, 2, 100, S + 3), _cycle(S - 1) + (2, 0, 0, 2)),       # pulse[S-1] != pulse[S]
    'K40': ((2, 2, 200, 40), None),
    'blocks2': ((2, 1, 300, 3), None),
}
RUN = 'run'


@functools.lru_cache(maxsize=None)
def _kernel_problem(name, tag):
    r"""Seeded as ``test_ab_sequence._kernel_problem`` (``rest[:, 1] = rest[:, 0]``, one ``rest_k = 0`` for ``K > 3``), with
    this file's schedules; ``run``: ``rest[:, S] = rest[:, S-1]``, no refresh across the boundary; ``change``: another rest at
    ``k = S``.  On the CPU in the data type, never modified."""
    shape, pulse = PROBLEMS[name]
    P = dict(_sequence_problem(shape, tag)[0])
    if pulse is not None:
        P['pulse'] = pulse
    if name == 'run':
        rest = P['rest'].clone()
        rest[:, S] = rest[:, S - 1]
        P['rest'] = rest
    if name == 'change':
        assert bool((P['rest'][:, S] != P['rest'][:, S - 1]).all())
    assert len(P['pulse']) == shape[3]
    return P


def _sig_shape(N, K, rx, nd=1):
    return (N, 2, K) + ((rx.shape[-1],) if rx is not None and rx.ndim == nd + 3 else ())


def _loss_weights(P, K, rx, w=None, v=None):
    N, nd = P['A'].shape[1], P['A'].ndim - 4
    w = _sin(_sig_shape(N, K, rx, nd), P['A'].dtype) if w is None else w
    v = _sin(tuple(P['B'].shape[1:]), P['A'].dtype, 0.53, 0.1) if v is None else v
    return w, v


def _yardstick(P, K, rx, use=OPS, w=None, v=None):
    r"""``sig``, ``Mlast`` and the gradients of ``(sig w).sum() + (Mlast v).sum()`` w.r.t. ``A, B``, the operands ``use`` and
    ``rx`` in fp64 on the CPU; operands not in ``use`` are absent."""
    w, v = _loss_weights(P, K, rx, w, v)
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    if rx is not None:
        L['rx'] = rx.double().clone().requires_grad_(True)
    ops = {k: L.get(k) for k in OPS}
    if ops['rest'] is not None:
        ops['rest'] = _table(ops['rest'], K)
    Mt = torch_sequence(L['A'], L['B'], K, P['pulse'], *(ops[k] for k in OPS))
    sig = torch_signal(Mt, L.get('rx'))
    if K > 0:
        Mlast = Mt[..., -1, :]
    else:
        Mlast = (L['Mi'] if 'Mi' in L else torch.tensor([0., 0., 1.], dtype=torch.float64)).expand(P['B'].shape[1:])
    loss = (sig * w.double()).sum() + (Mlast * v.double()).sum()
    if loss.requires_grad:
        loss.backward()
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['sig'], out['Mlast'] = sig.detach(), Mlast.detach()
    return out


@functools.lru_cache(maxsize=None)
def _cached_yardstick(name, tag, nRx):
    P = _kernel_problem(name, tag)
    shape = PROBLEMS[name][0]
    return _yardstick(P, shape[3], _rx(shape[1], shape[2], nRx, tag))


def _run(P, K, rx, use=OPS, over=None, w=None, v=None, pulse='own', n=False, leaves=None, loss=None, **kw):
    r"""The same through ``fused.sequence_signal`` on the device; ``over``: tensors that replace operands; ``pulse``: what is
    passed as the schedule instead of the problem's own; ``leaves``: the names of the operands that require grad (all by
    default; the others' gradients come back ``None``); ``loss``: a callable that is handed ``sig, Mlast`` and runs the
    backward pass itself, instead of ``(sig w).sum() + (Mlast v).sum()``."""
    w, v = _loss_weights(P, K, rx, w, v)
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    if rx is not None:
        L['rx'] = dev(rx).clone().requires_grad_(wanted('rx'))
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    sig, Mlast = fused.sequence_signal(L['A'], L['B'], pulse=list(P['pulse']) if isinstance(pulse, str) else pulse,
                                       **({'n': K} if n else {}), **{KW[k]: L[k] for k in use}, rx=L.get('rx'),
                                       return_last=True, **kw)
    if loss is not None:
        loss(sig, Mlast)
    elif sig.requires_grad:
        ((sig * dev(w)).sum() + (Mlast * dev(v)).sum()).backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['sig'], out['Mlast'] = sig.detach(), Mlast.detach()
    return out


def _gates(got, want, tag, what, keys=None, ledger=None):
    for k in (keys or want):
        ma, rl = max_abs(got[k], want[k]), rel_l2(got[k], want[k])
        print(f'{tag} {what} {k}: max abs {ma:.3e} rel-L2 {rl:.3e}')
        if ledger:
            record(f'seqsig.{tag}.{ledger}.{k}', ma if tag == 'f64' else rl)
    for k in (keys or want):
        _gate(got[k], want[k], tag, f'{what}: {k}')


# =============================================================================================
# 1. values and all nine gradients
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nRx', [-1, 0, 3, 8], ids=['norx', 'rx1', 'rx3', 'rx8'])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_kernels_alone_against_the_fp64_recursion(tag, name, nRx):
    r"""``one``: one row, one repetition.  ``K2`` with [1, 0]: a flush at the first step walked, a ragged tile per batch
    entry.  ``run`` / ``change`` at ``K = S + 3``: a run across the segment boundary with the rest unchanged there / a change
    of pulse and of rest exactly at ``k = S``; in both a return to an entry flushed before, a ``rest_k = 0``, and entry 1
    never played: its ``grad_A``, ``grad_B`` are exact zeros.  ``K40`` alternating: a flush per repetition over five
    segments.  ``blocks2`` with [1, 1, 0]: five tiles, the last ragged.  No map, one coil, 3 coils (one pad coil at
    capacity 4) and 8 coils.  Every gradient of a played entry is non-zero; a second run gives the same bits."""
    (P_, N, nM, K), _ = PROBLEMS[name]
    P = _kernel_problem(name, tag)
    rx = _rx(N, nM, nRx, tag)
    want = _cached_yardstick(name, tag, nRx)
    got = _run(P, K, rx)
    assert set(got) == set(want)
    assert got['sig'].dtype == got['Mlast'].dtype == DT[tag]
    assert got['sig'].shape == (N, 2, K) + ((nRx,) if nRx > 0 else ()) and got['Mlast'].shape == (N, nM, 3)
    _gates(got, want, tag, f'{name} nRx {nRx}', ledger=f'{name}_rx{nRx}')
    for k in OPS + (('rx',) if rx is not None else ()):
        g = got['grad_' + k]
        assert g.shape == (rx if k == 'rx' else P[k]).shape and g.dtype == DT[tag] and float(g.abs().max()) > 0, k
    for p in range(P_):
        for k in ('A', 'B'):
            g = got['grad_' + k]
            assert g.shape == P[k].shape and g.dtype == DT[tag]
            if p in P['pulse']:
                assert float(g[p].abs().min()) > 0, (k, p)
            else:
                assert torch.equal(g[p], torch.zeros_like(g[p])), f'grad_{k}[{p}]: the schedule never plays it'
    _same_bits(got, _run(P, K, rx), 'a second run')


# =============================================================================================
# 2. the same bits where the design promises them
# =============================================================================================
def _kwargs(D, use=OPS):
    return {KW[k]: D[k] for k in use}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nRx', [-1, 3], ids=['norx', 'rx3'])
def test_without_a_schedule_the_outputs_are_train_signals(tag, nRx):
    r"""``P = 1``, one ``rest`` `(N,)`, no ``pulse``: ``sig`` and ``Mlast`` are ``train_signal``'s by ``torch.equal``; and so
    with that rest written out as `(N, K)` and with a schedule of zeros."""
    N, nM, K = 2, 200, S + 3
    P = _sequence_problem((1, N, nM, K), tag)[0]
    D = {k: dev(v) for k, v in P.items() if k != 'pulse'}
    rest = D['rest'][:, 2].contiguous()
    rx = _rx(N, nM, nRx, tag)
    kw = dict(Mi=D['Mi'], phase=D['phase'], T1=D['T1'], T2=D['T2'], Δf=D['df'], rx=None if rx is None else dev(rx),
              return_last=True)
    with torch.no_grad():
        want = fused.train_signal(D['A'][0], D['B'][0], rest=rest, **kw)
        for given in (dict(rest=rest), dict(rest=rest[:, None].expand(N, K).contiguous()), dict(rest=rest, pulse=[0] * K)):
            got = fused.sequence_signal(D['A'], D['B'], **given, **kw)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), list(given)
    assert float(want[0].abs().max()) > 0


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['run', 'change', 'K40'])
def test_last_record_and_one_hot_map_are_ab_sequences_bit_for_bit(tag, name):
    r"""``Mlast`` is ``ab_sequence``'s last record; with the weight ``(1, 0)`` on one spin alone -- of the first tile, and of
    a later one -- ``sig[n, :, k]`` is that spin's ``Mt[n, s, k, :2]``: the other spins add exact zeros."""
    (P_, N, nM, K), _ = PROBLEMS[name]
    P = _kernel_problem(name, tag)
    D = {k: dev(P[k]) for k in LEAVES}
    with torch.no_grad():
        Mt = fused.ab_sequence(D['A'], D['B'], pulse=P['pulse'], **_kwargs(D))
        for s in (5, 70, nM - 1):
            rx = torch.zeros((N, nM, 2), dtype=DT[tag])
            rx[:, s, 0] = 1
            sig, Mlast = fused.sequence_signal(D['A'], D['B'], pulse=P['pulse'], **_kwargs(D), rx=dev(rx), return_last=True)
            assert torch.equal(Mlast, Mt[..., -1, :]), s
            assert torch.equal(sig, Mt[:, s, :, :2].movedim(-1, 1)), s


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('nRx', [3, 8, 9])
def test_every_coil_has_the_bits_of_its_one_coil_call(tag, nRx, monkeypatch):
    r"""``sig[..., c]`` of the 3-, 8- and 9-coil calls is the one-coil call's, bit for bit; the array's gradients are
    the sums of the one-coil calls' to the gate.  Nine coils are over the capacity: two launches each way."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    cap = int(_lib().mrphy_train_signal_max_rx(0 if tag == 'f32' else 1))
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, nRx, tag)
    w = _sin((N, 2, K, nRx), DT[tag])
    v = torch.zeros_like(P['B'][0])
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
# 3. requests and forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('leaf', LEAVES + ('rx',))
def test_each_leaf_alone(tag, leaf):
    r"""One operand requires grad: its gradient is the yardstick's, the others come back ``None``."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    got = _run(P, K, _rx(N, nM, 3, tag), leaves=(leaf,))
    want = _cached_yardstick(RUN, tag, 3)
    for k in LEAVES + ('rx',):
        assert (got['grad_' + k] is None) == (k != leaf), k
    _gates(got, want, tag, f'{leaf} alone', keys=('sig', 'Mlast', 'grad_' + leaf))
    if leaf in ('A', 'B'):
        assert torch.equal(got['grad_' + leaf][1], torch.zeros_like(got['grad_' + leaf][1]))


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_everything_but_the_bank_queries_no_bank_workspace(tag, monkeypatch):
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    want = _cached_yardstick(RUN, tag, 3)
    calls = _counted(monkeypatch, (FWD, BWD, BANK))
    got = _run(P, K, rx, leaves=OPS + ('rx',))
    assert dict(calls) == {FWD: 1, BWD: 1}, 'no bank workspace without grad_A, grad_B'
    assert got['grad_A'] is None and got['grad_B'] is None
    _gates(got, want, tag, 'all but the bank', keys=['grad_' + k for k in OPS + ('rx',)])
    calls.clear()
    got = _run(P, K, rx, leaves=('B',))
    assert dict(calls) == {FWD: 1, BWD: 1, BANK: 1}
    _gates(got, want, tag, 'B alone', keys=['grad_B'])


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('which', ['sig', 'Mlast', 'first', 'segment2', 'last'])
def test_cotangent_forms(tag, which):
    r"""A cotangent on ``sig`` alone (``Mlast`` never enters the loss: its cotangent is ``None``), on ``Mlast`` alone, and on
    one sample alone -- the first, the first of the second checkpoint segment, the last: every gradient against the
    yardstick's; ``grad_phase[:, k]`` and ``grad_rest[:, k]`` are exact zeros for every ``k`` after the sample."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    w0, v0 = _loss_weights(P, K, rx)
    w, v, loss = w0, torch.zeros_like(v0), None
    if which == 'sig':
        loss = lambda sig, Mlast: (sig * dev(w0)).sum().backward()  # noqa: E731
    elif which == 'Mlast':
        w, v = torch.zeros_like(w0), v0
        loss = lambda sig, Mlast: (Mlast * dev(v0)).sum().backward()  # noqa: E731
    else:
        j = {'first': 0, 'segment2': S, 'last': K - 1}[which]
        w = torch.zeros_like(w0)
        w[:, :, j] = w0[:, :, j]
    want, got = _yardstick(P, K, rx, w=w, v=v), _run(P, K, rx, w=w, v=v, loss=loss)
    _gates(got, want, tag, f'cotangent on {which}', ledger=f'cotangent_{which}')
    if which in ('first', 'segment2', 'last'):
        for k in ('grad_phase', 'grad_rest'):
            assert float(got[k][:, j + 1:].abs().sum()) == 0.0, k
        assert float(got['grad_phase'][:, j].abs().min()) > 0
    if which == 'Mlast':
        assert float(got['grad_rx'].abs().sum()) == 0.0


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', 'N', '1K', 'NK'])
def test_forms_of_rest(tag, form):
    r"""``rest`` as `()`, `(N,)`, `(1, K)`, `(N, K)`: the bits of the call with the table written out as `(N, K)`; the
    gradient has the operand's shape and is the yardstick's on that form (autograd folds it)."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    full = P['rest']
    x = {'0dim': full[0, 2], 'N': full[:, 2], '1K': full[:1], 'NK': full}[form].clone()
    mat = _run(dict(P, rest=_table(x, K).expand(N, K).contiguous()), K, rx)
    got = _run(P, K, rx, over=dict(rest=dev(x)))
    for k in mat:
        if k != 'grad_rest':
            assert torch.equal(got[k], mat[k]), (form, k)
    g = got['grad_rest']
    assert g.shape == x.shape and g.dtype == x.dtype and float(g.abs().min()) > 0
    want = _yardstick(dict(P, rest=x), K, rx)
    _gates(got, want, tag, f'rest {form}', keys=['grad_rest'], ledger=f'rest_{form}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(ABSENT))
def test_absent_operands(tag, case):
    r"""The five absences of ``test_ab_train.ABSENT`` against the yardstick with the same absence, three coils."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx, use = _rx(N, nM, 3, tag), ABSENT[case]
    want, got = _yardstick(P, K, rx, use), _run(P, K, rx, use)
    assert set(got) == set(want) == {'sig', 'Mlast', 'grad_A', 'grad_B', 'grad_rx'} | {'grad_' + k for k in use}
    _gates(got, want, tag, case)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_no_receive_map_is_the_weight_one(tag):
    r"""``rx=None`` is an explicit ``(1, 0)`` on every spin, bit for bit, values and gradients."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    one = torch.zeros((N, nM, 2), dtype=DT[tag])
    one[..., 0] = 1
    got, full = _run(P, K, None), _run(P, K, one)
    assert float(full.pop('grad_rx').abs().max()) > 0
    _same_bits(got, full, 'rx=None')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_broadcast_and_expanded_operands(tag, form):
    r"""``T1``, ``T2``, ``Δf`` in every broadcast form; ``phase`` `(1, K)`, ``Mi`` `(1, 1, 3)` and ``rx`` `(1, nM, 2, 3)`,
    then full: the bits of the materialised call; each gradient has its operand's shape and is the materialised call's
    summed."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx_full = _rx(N, nM, 3, tag)
    for small in (True, False):
        (T1, T1m), (T2, T2m), (df, dfm) = (_form(P[k], form) for k in ('T1', 'T2', 'df'))
        phase = P['phase'][:1].clone() if small else P['phase'].clone()
        Mi = P['Mi'][:1, :1].clone() if small else P['Mi'].clone()
        rx = rx_full[:1].clone() if small else rx_full.clone()
        w, v = _loss_weights(P, K, rx_full)
        mat = _run(dict(P, T1=T1m, T2=T2m, df=dfm, phase=phase.expand(N, K).contiguous(),
                        Mi=Mi.expand(N, nM, 3).contiguous()), K, rx.expand(N, nM, 2, 3).contiguous(), w=w, v=v)
        got = _run(P, K, None, over=dict(T1=T1, T2=T2, df=df, phase=dev(phase), Mi=dev(Mi), rx=dev(rx)), w=w, v=v)
        what = (form, 'small' if small else 'full')
        for k in ('sig', 'Mlast', 'grad_A', 'grad_B', 'grad_rest'):
            assert torch.equal(got[k], mat[k]), (what, k)
        for k, x in (('T1', T1), ('T2', T2), ('df', df), ('phase', phase), ('Mi', Mi), ('rx', rx)):
            g, m = got['grad_' + k], mat['grad_' + k]
            assert g.shape == x.shape and g.dtype == x.dtype, (what, k, g.shape)
            shp = tuple(x.shape) + (1,) * (m.ndim - x.ndim) if x.ndim else (1,) * m.ndim
            _gate(g, m.double().cpu().sum_to_size(shp).reshape(x.shape), tag, f'{what}: grad_{k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_offset_and_strided_operands(tag):
    r"""Every operand a view into a larger buffer -- a storage offset, ``rx`` and ``Mi`` strided besides --, the bank an
    ``.unflatten`` view: the bits of the plain call, the gradients in the operands' shapes."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    base = _run(P, K, rx)

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
    over = {k: offset(P[k]) for k in ('phase', 'rest', 'T1', 'T2', 'df')}
    over.update(Mi=strided(P['Mi']), rx=strided(rx), A=offset(P['A'].flatten(0, 1)), B=offset(P['B'].flatten(0, 1)))
    assert all(not x.is_contiguous() for x in (over['Mi'], over['rx'])) and over['A'].storage_offset() == 3
    L = {k: x.requires_grad_(True) for k, x in over.items()}
    sig, Mlast = fused.sequence_signal(L['A'].unflatten(0, (P_, N)), L['B'].unflatten(0, (P_, N)), pulse=P['pulse'],
                                       **{KW[k]: L[k] for k in OPS}, rx=L['rx'], return_last=True)
    w, v = _loss_weights(P, K, rx)
    ((sig * dev(w)).sum() + (Mlast * dev(v)).sum()).backward()
    assert torch.equal(sig, base['sig']) and torch.equal(Mlast, base['Mlast'])
    for k in LEAVES + ('rx',):
        g = L[k].grad
        assert g.shape == L[k].shape, k
        assert torch.equal(g.reshape(base['grad_' + k].shape), base['grad_' + k]), k


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)`` with ``rx`` `(1, 10, 10, 2, 3)` shared by the batch: the bits of the flat `(N, 100)` call."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)[:1].clone()
    flat = _run(P, K, rx.expand(N, 100, 2, 3).contiguous())
    Q = dict(P, A=P['A'].reshape(P_, N, 10, 10, 3, 3), B=P['B'].reshape(P_, N, 10, 10, 3), Mi=P['Mi'].reshape(N, 10, 10, 3),
             T1=P['T1'].reshape(N, 10, 10), T2=P['T2'].reshape(N, 10, 10), df=P['df'].reshape(N, 10, 10))
    w, v = _loss_weights(P, K, rx.expand(N, 100, 2, 3))
    got = _run(Q, K, rx.reshape(1, 10, 10, 2, 3), w=w, v=v.reshape(N, 10, 10, 3))
    assert got['sig'].shape == (N, 2, K, 3) and got['Mlast'].shape == (N, 10, 10, 3)
    assert torch.equal(got['sig'], flat['sig']) and torch.equal(got['Mlast'].reshape(N, 100, 3), flat['Mlast'])
    for k in ('A', 'B', 'Mi', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert torch.equal(got['grad_phase'], flat['grad_phase']) and torch.equal(got['grad_rest'], flat['grad_rest'])
    assert got['grad_rx'].shape == (1, 10, 10, 2, 3)
    _gate(got['grad_rx'].reshape(1, 100, 2, 3), flat['grad_rx'].double().cpu().sum(0, keepdim=True), tag, 'grad_rx')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_demodulation(tag):
    r"""``demod=True`` is ``exp(-iφ_k)`` applied in fp64 torch to the plain call's samples
    (``test_train_signal_host.demodulated``), and differentiable: the yardstick's demodulated loss."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    D = {k: dev(P[k]) for k in LEAVES}
    with torch.no_grad():
        plain = fused.sequence_signal(D['A'], D['B'], pulse=P['pulse'], **_kwargs(D), rx=dev(rx))
        dem = fused.sequence_signal(D['A'], D['B'], pulse=P['pulse'], **_kwargs(D), rx=dev(rx), demod=True)
    assert dem.shape == plain.shape and dem.dtype == DT[tag]
    _gate(dem.cpu(), demodulated(plain.cpu(), P['phase']), tag, 'demod vs exp(-iφ) in torch')
    w, v = _loss_weights(P, K, rx)
    L = {k: P[k].double().clone().requires_grad_(True) for k in LEAVES}
    Mt = torch_sequence(L['A'], L['B'], K, P['pulse'], *(L[k] for k in OPS))
    z = torch_signal(Mt, rx.double())
    φ = L['phase'][:, :, None]
    zr, zi, c, s = z[:, 0], z[:, 1], torch.cos(φ), torch.sin(φ)
    ((torch.stack((zr * c + zi * s, zi * c - zr * s), dim=1) * w.double()).sum() + (Mt[..., -1, :] * v.double()).sum()).backward()
    want = {'grad_' + k: x.grad for k, x in L.items()}
    got = _run(P, K, rx, demod=True)
    _gates(got, want, tag, 'demod', keys=list(want))


# =============================================================================================
# 4. more tiles than persistent waves
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _big(tag):
    r"""``N = 2, K = S + 1, nM = 64 Pw + 100`` with ``Pw`` the cap on the persistent waves, read off the workspace query, a
    bank of 2 and two coils: every wave takes a second tile, the first two of them a third, the last tile has 36 spins
    and 28 lanes past ``nM``.  Seeded, never modified."""
    P_, N, K = 2, 2, S + 1
    lib = _lib()
    Pw = lib.mrphy_sequence_signal_workspace(0, 1, 1 << 30, 1, 1) // 8
    assert Pw == lib.mrphy_sequence_signal_workspace(0, 1, 1 << 29, 1, 1) // 8 and 64 <= Pw <= 1 << 14
    nM = 64 * Pw + 100
    gen = torch.Generator().manual_seed(78)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    P = dict(A=0.97 * Q, B=torch.randn((P_, N, nM, 3), generator=gen, dtype=torch.float64),
             Mi=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             phase=2 * torch.randn((N, K), generator=gen, dtype=torch.float64), rest=2e-3 + 8e-3 * rnd(N, K),
             T1=0.05 + 0.1 * rnd(N, nM), T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200)
    rx = 0.5 + torch.randn((N, nM, 2, 2), generator=gen, dtype=torch.float64)
    P = {k: x.to(DT[tag]) for k, x in P.items()}
    P['pulse'] = tuple(int(k % 3 == 0) for k in range(K))          # 1, 0, 0, 1, ...: a run of zeros across k = S-1 | S
    return P, rx.to(DT[tag]), int(Pw), K


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('loss', ['full', 'tail'])
def test_more_tiles_than_persistent_waves(tag, loss):
    r"""``full``: every spin weighs in, the yardstick on all of them; the bank's gradients are compared on the spins past
    the first ``Pw`` tiles, the last spin among them -- the one the lanes past ``nM`` copy: a flush from them would add
    into its slots.  ``tail``: ``rx`` is zero on every spin of the first ``Pw`` tiles and ``Mlast`` has no weight there, so
    the yardstick is the last 100 spins alone -- what the waves add into their workspace rows on their later tiles must
    not disturb nor lose what the earlier tiles left."""
    P, rx, Pw, K = _big(tag)
    N, nM = P['A'].shape[1:3]
    head = 64 * Pw
    w, v = _loss_weights(P, K, rx)
    spins = ('A', 'B', 'Mi', 'T1', 'T2', 'df')
    cut = lambda k, x: x[:, :, head:] if k in ('A', 'B', 'grad_A', 'grad_B') else x[:, head:]  # noqa: E731
    if loss == 'tail':
        rx = rx.clone()
        rx[:, :head] = 0
        v = v.clone()
        v[:, :head] = 0
        Pt = {k: (cut(k, x) if k in spins else x) for k, x in P.items()}
        want = _yardstick(Pt, K, rx[:, head:], w=w, v=v[:, head:])
    else:
        want = _yardstick(P, K, rx, w=w, v=v)
        want = {k: (cut(k, x) if k in ('grad_A', 'grad_B') else x) for k, x in want.items()}
    got = _run(P, K, rx, w=w, v=v)
    if loss == 'tail':
        for k in ('grad_A', 'grad_B'):
            assert float(got[k][:, :, :head].abs().sum()) == 0.0, f'{k}: spins without a weight'
    got = {k: (cut(k, x) if k in ('grad_A', 'grad_B') else x) for k, x in got.items()}
    keys = ('sig', 'grad_A', 'grad_B', 'grad_phase', 'grad_rest')
    if loss == 'full':
        keys += ('grad_T1', 'grad_T2', 'grad_df', 'grad_Mi', 'grad_rx', 'Mlast')
    _gates(got, want, tag, f'{loss} (Pw = {Pw}, nM = {nM})', keys=keys, ledger=f'big_{loss}')


# =============================================================================================
# 5. two chained calls
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_chained_calls_are_one_call(tag):
    r"""``K1 = 3`` repetitions, then the other ``S`` from ``Mlast``, against the one call of ``run``.  fp64: the values bit for
    bit, and so the gradients that no sum over the repetitions splits -- ``grad_Mi`` (the adjoint state handed from the
    second call to the first), ``grad_phase`` and the per-repetition ``grad_rest``; the others are sums over k that the
    chain forms as (first call) + (second call): another association of the same terms, held to the gate.  fp32:
    everything to the gate (``Mlast`` is rounded to fp32 between the calls)."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    K1 = 3
    P = _kernel_problem(RUN, tag)
    rx = _rx(N, nM, 3, tag)
    w, v = _loss_weights(P, K, rx)
    one = _run(P, K, rx, w=w, v=v)
    L = {k: dev(P[k]).clone().requires_grad_(True) for k in LEAVES}
    L['rx'] = dev(rx).clone().requires_grad_(True)
    kw = dict(T1=L['T1'], T2=L['T2'], Δf=L['df'], rx=L['rx'], return_last=True)
    s1, M1 = fused.sequence_signal(L['A'], L['B'], pulse=P['pulse'][:K1], Mi=L['Mi'], phase=L['phase'][:, :K1],
                                   rest=L['rest'][:, :K1], **kw)
    s2, M2 = fused.sequence_signal(L['A'], L['B'], pulse=P['pulse'][K1:], Mi=M1, phase=L['phase'][:, K1:],
                                   rest=L['rest'][:, K1:], **kw)
    sig = torch.cat((s1, s2), dim=2)
    ((sig * dev(w)).sum() + (M2 * dev(v)).sum()).backward()
    two = {'grad_' + k: x.grad for k, x in L.items()}
    two['sig'], two['Mlast'] = sig.detach(), M2.detach()
    if tag == 'f64':
        for k in ('sig', 'Mlast', 'grad_Mi', 'grad_phase', 'grad_rest'):
            assert torch.equal(two[k], one[k]), k
    _gates(two, {k: x.double().cpu() for k, x in one.items()}, tag, 'chained vs one call')
    _gates(two, _cached_yardstick(RUN, tag, 3), tag, 'chained vs the yardstick')


# =============================================================================================
# 6. empty problems, launch counts, memory
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('what', ['K0', 'nM0'])
def test_empty_problem(tag, what, monkeypatch):
    r"""No repetition and no spin: a signal of zeros in its shape, ``Mlast`` = ``Mi``; the backward runs and the gradients
    are zeros of the operands' shapes (at ``K = 0`` ``grad_Mi`` is the cotangent of ``Mlast``); no kernel of another
    family stands in."""
    (P_, N, nM, K), _ = PROBLEMS[RUN]
    P = _kernel_problem(RUN, tag)
    if what == 'K0':
        K, E, rx = 0, dict(P, phase=P['phase'][:, :0], rest=P['rest'][:, :0], pulse=()), _rx(N, nM, 3, tag)
    else:
        E = {k: (v[:, :, :0] if k in ('A', 'B') else v[:, :0] if k in ('Mi', 'T1', 'T2', 'df') else v) for k, v in P.items()}
        rx = _rx(N, nM, 3, tag)[:, :0]
    calls = _counted(monkeypatch, OTHERS)
    got = _run(E, K, rx)
    assert not calls
    nM = E['A'].shape[2]
    assert got['sig'].shape == (N, 2, K, 3) and got['sig'].dtype == DT[tag] and float(got['sig'].abs().sum()) == 0.0
    assert got['Mlast'].shape == (N, nM, 3)
    if what == 'K0':
        assert torch.equal(got['Mlast'].cpu(), P['Mi'])
    for k in LEAVES + ('rx',):
        g = got['grad_' + k]
        assert g is not None and g.shape == (rx if k == 'rx' else E[k]).shape and g.dtype == DT[tag], k
        if not (what == 'K0' and k == 'Mi'):
            assert float(g.abs().sum()) == 0.0, k
    if what == 'K0':
        assert torch.equal(got['grad_Mi'].cpu(), _loss_weights(E, K, rx)[1])


@pytest.mark.parametrize('name', ['K40', 'run', 'one'])
def test_one_launch_each_way_whatever_the_schedule(name, monkeypatch):
    r"""One call of each entry point -- the main launch and its second passes -- and none of another family's, at a flush
    per repetition, at runs, at one repetition; without a gradient wanted the forward gets a null checkpoint pointer."""
    (P_, N, nM, K), _ = PROBLEMS[name]
    calls = _counted(monkeypatch, (FWD, BWD) + OTHERS)
    P = _kernel_problem(name, 'f32')
    _run(P, K, _rx(N, nM, 3, 'f32'))
    assert dict(calls) == {FWD: 1, BWD: 1}
    calls.clear()
    lib = _lib()
    seen = []
    inner = getattr(lib, FWD)
    monkeypatch.setattr(lib, FWD, lambda *a: (seen.append(a), inner(*a))[1])
    A = dev(P['A']).requires_grad_(True)
    with torch.no_grad():
        fused.sequence_signal(A, dev(P['B']), pulse=P['pulse'])
    assert dict(calls) == {FWD: 1}
    assert len(seen) == 1 and seen[0][25] is None, 'no_grad: a null checkpoint pointer'
    fused.sequence_signal(A, dev(P['B']), pulse=P['pulse'])
    assert len(seen) == 2 and seen[1][25] is not None, 'a gradient is wanted: checkpoints'


def test_nothing_of_the_size_of_the_records_is_allocated():
    r"""P = 2, N = 1, nM = 4096, K = 256 in fp32 with a pulse and a rest per repetition, ``A``, ``B``, ``T1`` and ``rest``
    requiring grad: forward + backward raise the allocator's peak by less than half the bytes ``Mt`` alone would take
    (``K · nM · 3 · 4``); the route through ``ab_sequence`` keeps ``Mt`` and its cotangent, four times that bound.  What
    there is: the fp64 checkpoints every ``S`` repetitions (a quarter of ``Mt``), the bank's gradients and their fp64
    workspace, the per-wave sums."""
    P_, N, nM, K = 2, 1, 4096, 256
    gen = torch.Generator().manual_seed(9)
    Qm = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    A = dev((0.97 * Qm).float()).requires_grad_(True)
    B = dev(torch.randn((P_, N, nM, 3), generator=gen)).requires_grad_(True)
    T1 = dev(0.05 + 0.1 * torch.rand((N, nM), generator=gen)).requires_grad_(True)
    T2 = dev(0.02 + 0.05 * torch.rand((N, nM), generator=gen))
    rest = dev(2e-3 + 8e-3 * torch.rand((N, K), generator=gen)).requires_grad_(True)
    phase = dev(2 * torch.randn((N, K), generator=gen))
    pulse = [(k // 3) % P_ for k in range(K)]
    w = dev(_sin((N, 2, K), torch.float32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sig = fused.sequence_signal(A, B, pulse=pulse, phase=phase, rest=rest, T1=T1, T2=T2)
    sig.backward(w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    records = K * N * nM * 3 * 4
    print(f'peak rise {rise} B; Mt would be {records} B')
    assert A.grad is not None and B.grad is not None and float(T1.grad.abs().max()) > 0 and float(rest.grad[:, 1:].abs().min()) > 0
    assert 0 < rise < records // 2, (rise, records)


# =============================================================================================
# 7. sequence_signal_rfgr end to end on the fixtures
# =============================================================================================
def _fixture_run(Q, rx):
    γ = dev(Q['γ'])
    return fused.sequence_signal_rfgr(dev(Q['rf']), dev(Q['gr'])[None], dev(Q['loc']), pulse=Q['pulse'],
                                      phase=dev(Q['phase']), rest=dev(Q['rest']), T1=dev(Q['T1']), T2=dev(Q['T2']),
                                      Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']),
                                      rx=None if rx is None else dev(rx))


@pytest.mark.parametrize('tag_mode', MODES)
@pytest.mark.parametrize('nRx', [-1, 3], ids=['norx', 'rx3'])
def test_against_the_reference_fixture(tag_mode, nRx):
    r"""The inputs of ``tests/golden/sequence_{f32,f64}.npz`` (the reference's simulators: 24 repetitions of a bank of three
    pulses with a rest per repetition) and a seeded ``rx = 0.5 + randn``, none and 3 coils; the expected signal is
    ``torch_signal`` of the fp64 fixture's records.  fp64 at the gate.  fp32, precise and fast: the distance to that signal
    is held to 3 x the distance of ``torch_signal`` of the reference's own fp32 records (1.3e-6 without a map, 1.6e-6
    with these 3 coils, computed here on the CPU); every distance goes to the ledger."""
    tag, mode = _mode(tag_mode)
    G, G64 = golden(f'sequence_{tag}'), golden('sequence_f64')
    Q = fixture_inputs(G)
    rx = _rx(2, 100, nRx, tag)
    with mode, torch.no_grad():
        sig = _fixture_run(Q, rx)
    assert sig.shape == (2, 2, 24) + ((3,) if nRx > 0 else ()) and sig.dtype == DT[tag]
    rx64 = None if rx is None else rx.double()
    sum64 = torch_signal(t(G64['Mt']).double(), rx64)
    if tag == 'f64':
        d = record(f'seqsig.f64.fixture.rx{nRx}.sig', max_abs(sig, sum64))
        print(f'f64 sig: {d:.3e} max abs from the signal of the reference fixture')
        _gate(sig.cpu(), sum64, 'f64', 'sig vs the signal of the reference fixture')
        return
    ref = rel_l2(torch_signal(t(G['Mt']).double(), rx64), sum64)
    bound = 3 * ref
    record(f'seqsig.{tag_mode}.fixture.rx{nRx}.sig.reference_f32_vs_fixture64', ref)
    d = record(f'seqsig.{tag_mode}.fixture.rx{nRx}.sig.vs_fixture64', rel_l2(sig, sum64), bound)
    print(f'{tag_mode} sig: {d:.3e} from the signal of the fp64 fixture, bound {bound:.3e} (the reference: {ref:.3e})')
    assert d <= bound, f'sig: {d:.3e} from the fp64 fixture > 3 x the reference\'s own fp32 distance = {bound:.3e}'


def test_fixture_gradients_reach_the_pulses_and_the_rests():
    r"""fp64, through ``ab_rfgr``'s adjoint: ``grad_rf`` (of the bank), ``grad_gr``, ``grad_T1`` and ``grad_rest`` of a seeded
    signal loss with 3 coils against the CPU oracle's bank (``test_ab_sequence_host.oracle_bank``), ``torch_sequence``,
    ``torch_signal`` and autograd, at the gate."""
    Q = fixture_inputs(golden('sequence_f64'))
    rx = _rx(2, 100, 3, 'f64')
    w = _sin((2, 2, 24, 3), torch.float64, 0.41, 0.2)
    rf, gr, T1, rest = (dev(Q[k]).clone().requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    γ = dev(Q['γ'])
    sig = fused.sequence_signal_rfgr(rf, gr[None], dev(Q['loc']), pulse=Q['pulse'], phase=dev(Q['phase']), rest=rest, T1=T1,
                                     T2=dev(Q['T2']), Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']),
                                     rx=dev(rx))
    (sig * dev(w)).sum().backward()
    got = dict(sig=sig.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)
    orf, ogr, oT1, orest = (Q[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    A, B = oracle_bank(Q, orf, ogr, oT1)
    osig = torch_signal(torch_sequence(A, B, 24, Q['pulse'].tolist(), None, Q['phase'], orest, oT1, Q['T2'], Q['df']), rx)
    (osig * w).sum().backward()
    want = dict(sig=osig.detach(), grad_rf=orf.grad, grad_gr=ogr.grad, grad_T1=oT1.grad, grad_rest=orest.grad)
    assert got['grad_rf'].shape == (3, 2, 2, 48) and got['grad_gr'].shape == (2, 3, 48) and got['grad_rest'].shape == (2, 24)
    _gates(got, want, 'f64', 'fixture vs the CPU oracle', ledger='fixture.vs_oracle')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_parallel_transmit_runs_through_the_fused_ab(tag, monkeypatch):
    r"""4 transmit coils with their ``b1Map`` (``test_fused_traj._problem(.., 'ptx4', 48)``) as a bank of two pulses -- the
    second at 0.6 of the first --, the fixture's rests and phases, 8 repetitions, 3 receive coils: ``A, B`` come from ONE
    ``mrphy_ab_rfgr_mc_fwd`` call on the batch ``P·N``, and the signal is the yardstick's on ``beff2ab(rfgr2beff(.))`` of
    the device, entry by entry."""
    K, pulse = 8, [0, 1, 1, 0, 1, 0, 0, 1]
    P = _pulse_problem(tag, 'ptx4', 48)
    Q = fixture_inputs(golden(f'sequence_{tag}'))
    rest, phase = dev(Q['rest'][:, :K].contiguous()), dev(Q['phase'][:, :K].contiguous())
    γ, dt, T1, T2, df = (dev(P[k]) for k in ('γ', 'dt', 'T1', 'T2', 'df'))
    rf = torch.stack((dev(P['rf']), 0.6 * dev(P['rf'])))
    rx = _rx(2, 100, 3, tag)
    E1, E2 = torch.exp(-dt[:, None] / T1), torch.exp(-dt[:, None] / T2)
    consts = dict(γ2πdt=2 * π * _host.pad_trailing(γ, 2) * _host.pad_trailing(dt, 2), E1=E1, E2=E2, E1_1=E1 - 1)
    calls = _counted(monkeypatch, ('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd', 'mrphy_beff2ab', FWD) + OTHERS)
    with torch.no_grad():
        sig = fused.sequence_signal_rfgr(rf, dev(P['gr'])[None], dev(P['loc']), pulse=pulse, phase=phase, rest=rest, T1=T1,
                                         T2=T2, Δf=df, rx=dev(rx), b1Map=dev(P['b1']), γ_beff=γ, consts=consts)
        assert dict(calls) == {'mrphy_ab_rfgr_mc_fwd': 1, FWD: 1}
        AB = [beffective.beff2ab(beffective.rfgr2beff(rf[p], dev(P['gr']), dev(P['loc']), Δf=df, b1Map=dev(P['b1']), γ=γ),
                                 E1=E1, E2=E2, γ=γ, dt=dt) for p in range(2)]
        A, B = torch.stack([a for a, _ in AB]).double().cpu(), torch.stack([b for _, b in AB]).double().cpu()
        want = torch_signal(torch_sequence(A, B, K, pulse, None, phase.double().cpu(), rest.double().cpu(),
                                           T1.double().cpu(), T2.double().cpu(), df.double().cpu()), rx.double())
    assert sig.shape == (2, 2, K, 3) and sig.dtype == DT[tag]
    _gate(sig.cpu(), want, tag, 'sig under parallel transmit')
