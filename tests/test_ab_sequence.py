r"""``fused.ab_sequence`` (Ksq / Ksqb: ``mrphy_ab_sequence_fwd`` / ``_bwd``) and ``fused.sequence_rfgr`` on the device.

What is claimed where.  The arithmetic per repetition is Ktr's / Ktrb's, so the kernels ALONE are held to their gate
(``test_steadystate._gate``): against the fp64 recursion in plain torch on the CPU
(``test_ab_sequence_host.torch_sequence``) on the same numbers, fp64 max abs 1e-9 and fp32 relative L2 1e-6, the records
and all eight gradients (§1 - §5).  The fp32 budget: an adjoint that reads fp32-rounded records and sums in fp64,
emulated on the CPU at the five shapes of §1, lies 1e-8 .. 4.3e-8 from exact autograd in every gradient, the
per-repetition ``grad_rest`` included -- a factor of 20 inside the gate.  End to end in fp32 (§8) the result inherits the
rounding of ``A`` amplified by the train's conditioning, so the distance to the fp64 fixture is held to three times what
the reference's own all-fp32 route loses on the same numbers, the margin and reason of ``test_ab_train.py`` §8.
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host, _lib
from test_ab_rfgr import _counted
from test_ab_rfgr_host import fixture_inputs
from test_ab_sequence_host import oracle_sequence, torch_sequence
from test_ab_train import ABSENT, _same_bits, _weights
from test_fused_traj import _problem
from test_steadystate import _form, _gate, _mode

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
OPS = ('Mi', 'phase', 'rest', 'T1', 'T2', 'df')       # the optional operands; A, B are always there
KW = dict(Mi='Mi', phase='phase', rest='rest', T1='T1', T2='T2', df='Δf')
FWD, BWD = 'mrphy_ab_sequence_fwd', 'mrphy_ab_sequence_bwd'

# (P, N, nM, K) -> the schedule
SCHEDULES = {
    (1, 1, 1, 1): (0,),
    (2, 2, 100, 2): (1, 0),
    (3, 2, 100, 7): (0, 2, 2, 0, 0, 2, 0),
    (2, 2, 200, 40): tuple(k % 2 for k in range(40)),
    (2, 1, 300, 3): (1, 1, 0),
}
SHAPES = list(SCHEDULES)
IDS = ['one', 'K2', 'K7', 'K40', 'blocks2']
S7 = (3, 2, 100, 7)


@functools.lru_cache(maxsize=None)
def _kernel_problem(shape, tag):
    r"""Seeded as ``test_ab_train._kernel_problem``: ``A = 0.97 Q`` per bank entry, ``B``, ``Mi``, phases ``2 randn``,
    ``rest = 2e-3 + 8e-3 rand(N, K)`` with ``rest[:, 1] = rest[:, 0]`` and, for ``K > 3``, ``rest[:, 3] = 0``, the other
    operands of the rest and time-major weights, in the data type, on the CPU; and the fp64 yardstick of the same
    numbers.  Computed once per shape, never modified."""
    P_, N, nM, K = shape
    gen = torch.Generator().manual_seed(1000000 * P_ + 100000 * N + 100 * nM + K)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    rest = 2e-3 + 8e-3 * rnd(N, K)
    if K > 1:
        rest[:, 1] = rest[:, 0]
    if K > 3:
        rest[:, 3] = 0
    P = dict(A=0.97 * Q, B=torch.randn((P_, N, nM, 3), generator=gen, dtype=torch.float64),
             Mi=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             phase=2 * torch.randn((N, K), generator=gen, dtype=torch.float64), rest=rest, T1=0.05 + 0.1 * rnd(N, nM),
             T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200, w=_weights(K, N, nM, torch.float64))
    P = {k: v.to(DT[tag]) for k, v in P.items()}
    P['pulse'] = SCHEDULES.get(shape, (0,) * K)
    return P, _yardstick(P, K)


def _table(rest, K):
    r"""``rest`` in any of its forms as the yardstick's `(N ⊻ 1, K)`."""
    return rest.reshape(-1, 1).expand(-1, K) if rest.ndim < 2 else rest


def _yardstick(P, K, use=OPS):
    r"""The records and the gradients of ``(Mt w).sum()`` w.r.t. ``A, B`` and the operands ``use`` by ``torch_sequence``
    and autograd in fp64 on the CPU; operands not in ``use`` are absent."""
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    ops = {k: L.get(k) for k in OPS}
    if ops['rest'] is not None:
        ops['rest'] = _table(ops['rest'], K)
    Mt = torch_sequence(L['A'], L['B'], K, P['pulse'], *(ops[k] for k in OPS))
    (Mt.movedim(-2, 0) * P['w'].double().reshape((K,) + Mt.shape[:-2] + (3,))).sum().backward()
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['Mt'] = Mt.detach()
    return out


def _run(P, K, use=OPS, over=None, pulse='own', n=False, leaves=None, loss=None):
    r"""The same through ``fused.ab_sequence`` on the device; ``over``: tensors that replace operands (operand forms);
    ``pulse``: what is passed as the schedule instead of the problem's own tuple; ``leaves``: the names of the operands
    that require grad (all of them by default; the others' gradients come back ``None``); ``loss``: a callable that is
    handed ``Mt`` and runs the backward pass itself, instead of ``(Mt w).sum()``."""
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    Mt = fused.ab_sequence(L['A'], L['B'], pulse=list(P['pulse']) if isinstance(pulse, str) else pulse,
                           **({'n': K} if n else {}), **{KW[k]: L[k] for k in use})
    if loss is not None:
        loss(Mt)
    elif Mt.requires_grad:
        (Mt.movedim(-2, 0) * dev(P['w']).reshape((K,) + Mt.shape[:-2] + (3,))).sum().backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['Mt'] = Mt.detach()
    return out


# =============================================================================================
# 1. values and all eight gradients
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_kernels_alone_against_the_fp64_recursion(tag, shape):
    r"""(1, 1, 1, 1) with [0]: nothing fetched ahead, nothing flushed before the end.  (2, 2, 100, 2) with [1, 0]: a flush
    at the first step walked, ragged blocks, two grid rows.  (3, 2, 100, 7) with [0, 2, 2, 0, 0, 2, 0]: runs of 1 and 2, a
    return to a slot already flushed, and entry 1 never played: its ``grad_A``, ``grad_B`` are exact zeros.
    (2, 2, 200, 40) alternating: a flush per repetition while the prefetch cycles.  (2, 1, 300, 3) with [1, 1, 0]: a second,
    ragged block.  The records and the gradients w.r.t. ``A, B, Mi, phase, rest, T1, T2, Δf``; every gradient is
    non-zero where an entry is played; a second run gives the same bits."""
    P_, N, nM, K = shape
    P, want = _kernel_problem(shape, tag)
    got = _run(P, K)
    assert got['Mt'].dtype == DT[tag] and got['Mt'].shape == (N, nM, K, 3) and set(got) == set(want)
    assert got['Mt'].movedim(-2, 0).is_contiguous(), 'time-major storage'
    for k in want:
        print(f'{tag} {shape} {k}: max abs {max_abs(got[k], want[k]):.3e} rel-L2 {rel_l2(got[k], want[k]):.3e}')
    for k in want:
        _gate(got[k], want[k], tag, k)
    for k in ('Mi', 'phase', 'rest', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == P[k].shape and float(got['grad_' + k].abs().max()) > 0, k
    for p in range(P_):
        for k in ('A', 'B'):
            g = got['grad_' + k]
            assert g.shape == P[k].shape
            if p in P['pulse']:
                assert float(g[p].abs().min()) > 0, (k, p)
            else:
                assert float(g[p].abs().max()) == 0.0, f'grad_{k}[{p}]: the schedule never plays it'
    record(f'sequence.{tag}.P{P_}_N{N}_nM{nM}_K{K}.Mt', max_abs(got['Mt'], want['Mt']) if tag == 'f64' else rel_l2(got['Mt'], want['Mt']))
    _same_bits(got, _run(P, K), 'a second run')


# =============================================================================================
# 2. Ktr's bits
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_without_a_schedule_the_records_are_ab_trains(tag):
    r"""``P = 1``, ``pulse=None``, ``rest`` `(N,)`: ``Mt`` is ``ab_train``'s by ``torch.equal``; and so it is with that rest
    written out as `(N, K)`."""
    K = 7
    P, _ = _kernel_problem((1, 2, 100, K), tag)
    D = {k: dev(v) for k, v in P.items() if k != 'pulse'}
    rest = D['rest'][:, 2].contiguous()
    kw = dict(Mi=D['Mi'], phase=D['phase'], T1=D['T1'], T2=D['T2'], Δf=D['df'])
    with torch.no_grad():
        want = fused.ab_train(D['A'][0], D['B'][0], rest=rest, **kw)
        assert torch.equal(fused.ab_sequence(D['A'], D['B'], rest=rest, **kw), want)
        assert torch.equal(fused.ab_sequence(D['A'], D['B'], rest=rest[:, None].expand(2, K).contiguous(), **kw), want)
        assert torch.equal(fused.ab_sequence(D['A'], D['B'], pulse=[0] * K, rest=rest, **kw), want)
    assert float(want.abs().max()) > 0


def test_fp64_schedule_is_the_chain_of_single_repetitions():
    r"""fp64, shape 3 of §1: the records ``torch.equal`` the chain of ``K`` calls ``ab_train(A[p_k], B[p_k], n=1,
    Mi=previous, phase=φ[:, k:k+1], rest=rest[:, k], ...)`` -- in fp64 nothing is rounded between the calls."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, 'f64')
    D = {k: dev(v) for k, v in P.items() if k != 'pulse'}
    kw = dict(T1=D['T1'], T2=D['T2'], Δf=D['df'])
    with torch.no_grad():
        got = fused.ab_sequence(D['A'], D['B'], pulse=P['pulse'], Mi=D['Mi'], phase=D['phase'], rest=D['rest'], **kw)
        M, chain = D['Mi'], []
        for k, p in enumerate(P['pulse']):
            M = fused.ab_train(D['A'][p], D['B'][p], n=1, Mi=M, phase=D['phase'][:, k:k + 1].contiguous(),
                               rest=D['rest'][:, k].contiguous(), **kw)[..., 0, :]
            chain.append(M)
    assert torch.equal(got, torch.stack(chain, dim=-2))


# =============================================================================================
# 3. absent operands and operand forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(ABSENT))
def test_absent_operands(tag, case):
    r"""The five absences of ``test_ab_train.ABSENT`` against the yardstick with the same absence; the absent operands
    get no gradient."""
    K = 7
    P, _ = _kernel_problem(S7, tag)
    use = ABSENT[case]
    want, got = _yardstick(P, K, use), _run(P, K, use, n='phase' not in use)
    assert set(got) == set(want) == {'Mt', 'grad_A', 'grad_B'} | {'grad_' + k for k in use}
    for k in want:
        _gate(got[k], want[k], tag, f'{case}: {k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_operand_forms_of_the_spin_constants(tag, form):
    r"""``T1``, ``T2``, ``Δf`` in every broadcast form of ``test_steadystate._form``: the bits of the materialised call;
    each gradient has its operand's own shape and is the materialised call's summed over the broadcast axes."""
    K = 7
    P, _ = _kernel_problem(S7, tag)
    (T1, T1m), (T2, T2m), (df, dfm) = (_form(P[k], form) for k in ('T1', 'T2', 'df'))
    mat = _run(dict(P, T1=T1m, T2=T2m, df=dfm), K)
    got = _run(P, K, over=dict(T1=T1, T2=T2, df=df))
    for k in ('Mt', 'grad_A', 'grad_B', 'grad_Mi', 'grad_phase', 'grad_rest'):
        assert torch.equal(got[k], mat[k]), (form, k)
    for k, x in (('T1', T1), ('T2', T2), ('df', df)):
        g, m = got['grad_' + k], mat['grad_' + k]
        assert g.shape == x.shape and g.dtype == x.dtype, (form, k, g.shape)
        shp = tuple(x.shape) + (1,) * (m.ndim - x.ndim) if x.ndim else (1,) * m.ndim
        _gate(g, m.double().cpu().sum_to_size(shp).reshape(x.shape), tag, f'{form}: grad_{k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', 'N', '1K', 'NK'])
def test_forms_of_rest(tag, form):
    r"""``rest`` as `()`, `(N,)`, `(1, K)`, `(N, K)`: the bits of the call with the table written out as `(N, K)`; the
    gradient has the operand's shape and is the written-out call's summed over what the form shares."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    full = P['rest']
    x = {'0dim': full[0, 2], 'N': full[:, 2], '1K': full[:1], 'NK': full}[form].clone()
    mat = _run(dict(P, rest=_table(x, K).expand(N, K).contiguous()), K)
    got = _run(P, K, over=dict(rest=dev(x)))
    for k in mat:
        if k != 'grad_rest':
            assert torch.equal(got[k], mat[k]), (form, k)
    g, m = got['grad_rest'], mat['grad_rest'].double().cpu()
    assert g.shape == x.shape and g.dtype == x.dtype
    want = {'0dim': m.sum(), 'N': m.sum(1), '1K': m.sum(0, keepdim=True), 'NK': m}[form]
    _gate(g, want, tag, f'{form}: grad_rest')
    assert float(g.abs().min()) > 0


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_forms_of_pulse_and_a_bank_that_is_a_view(tag):
    r"""``pulse`` as a list, a tuple, an int64 and an int32 CPU tensor; ``A, B`` as ``.unflatten`` views of `(P·N, …)`
    tensors (what ``ab_rfgr`` returns for the batch): all the bits of the plain call."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    base = _run(P, K)
    for pulse in (tuple(P['pulse']), torch.tensor(P['pulse'], dtype=torch.int64), torch.tensor(P['pulse'], dtype=torch.int32)):
        _same_bits(_run(P, K, pulse=pulse), base, type(pulse))
    A, B = (dev(P[k]).flatten(0, 1).clone().requires_grad_(True) for k in ('A', 'B'))
    Mt = fused.ab_sequence(A.unflatten(0, (P_, N)), B.unflatten(0, (P_, N)), pulse=P['pulse'],
                           **{KW[k]: dev(P[k]) for k in OPS})
    (Mt.movedim(-2, 0) * dev(P['w'])).sum().backward()
    assert torch.equal(Mt, base['Mt'])
    assert torch.equal(A.grad.unflatten(0, (P_, N)), base['grad_A']) and torch.equal(B.grad.unflatten(0, (P_, N)), base['grad_B'])


# =============================================================================================
# 4. two spatial dimensions
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)``: the bits of the flat `(N, 100)` call, gradients in the operands' shapes."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    flat = _run(P, K)
    Q = dict(P, A=P['A'].reshape(P_, N, 10, 10, 3, 3), B=P['B'].reshape(P_, N, 10, 10, 3), Mi=P['Mi'].reshape(N, 10, 10, 3),
             T1=P['T1'].reshape(N, 10, 10), T2=P['T2'].reshape(N, 10, 10), df=P['df'].reshape(N, 10, 10))
    got = _run(Q, K)
    assert got['Mt'].shape == (N, 10, 10, K, 3) and torch.equal(got['Mt'].reshape(N, 100, K, 3), flat['Mt'])
    for k in ('A', 'B', 'Mi', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert torch.equal(got['grad_phase'], flat['grad_phase']) and torch.equal(got['grad_rest'], flat['grad_rest'])


# =============================================================================================
# 5. a cotangent on one record only
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('j', [0, 3, 6])
def test_cotangent_on_one_record(tag, j):
    r"""The weights on record ``j`` alone: every gradient against the yardstick's, and ``grad_rest[:, k]``,
    ``grad_phase[:, k]`` are exact zeros for every ``k > j``."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    w = torch.zeros_like(P['w'])
    w[j] = P['w'][j]
    Pj = dict(P, w=w)
    want, got = _yardstick(Pj, K), _run(Pj, K)
    for k in want:
        _gate(got[k], want[k], tag, f'record {j}: {k}')
    for k in ('grad_phase', 'grad_rest'):
        assert float(got[k][:, j + 1:].abs().sum()) == 0.0, k
        assert float(got[k][:, j].abs().min()) > 0, k


# =============================================================================================
# 6. empty problems   7. call counts
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('what', ['K0', 'nM0'])
def test_empty_problem(tag, what, monkeypatch):
    r"""No repetition and no spin: correctly shaped empties; the backward runs, the gradients are zeros of the operands'
    shapes, and nothing is launched (the entry points return before their launches: refusals of
    ``test_ab_sequence_host``; here no kernel of another family stands in either)."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    if what == 'K0':
        K, E = 0, dict(P, phase=P['phase'][:, :0], rest=P['rest'][:, :0], w=P['w'][:0], pulse=())
    else:
        E = {k: (v[:, :, :0] if k in ('A', 'B', 'w') else v[:, :0] if k in ('Mi', 'T1', 'T2', 'df') else v)
             for k, v in P.items()}
    calls = _counted(monkeypatch, ('mrphy_ab_train_fwd', 'mrphy_ab_train_bwd', 'mrphy_freeprec_fwd'))
    got = _run(E, K)
    assert not calls
    nM = E['A'].shape[2]
    assert got['Mt'].shape == (N, nM, K, 3) and got['Mt'].dtype == DT[tag]
    for k in ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'df'):
        g = got['grad_' + k]
        assert g is not None and g.shape == E[k].shape and g.dtype == DT[tag], k
        assert float(g.abs().sum()) == 0.0, k


def test_one_launch_each_way_whatever_the_schedule(monkeypatch):
    calls = _counted(monkeypatch, (FWD, BWD, 'mrphy_ab_train_fwd', 'mrphy_ab_train_bwd'))
    shape = (2, 2, 200, 40)
    P, _ = _kernel_problem(shape, 'f32')
    _run(P, 40)
    assert dict(calls) == {FWD: 1, BWD: 1}
    calls.clear()
    with torch.no_grad():
        fused.ab_sequence(dev(P['A']), dev(P['B']), pulse=P['pulse'])
    assert dict(calls) == {FWD: 1}


# =============================================================================================
# 8. sequence_rfgr end to end on the fixtures
# =============================================================================================
OUT = ('Mt', 'grad_rf', 'grad_gr', 'grad_T1', 'grad_rest')


def _fixture_run(Q):
    rf, gr, T1, rest = (dev(Q[k]).requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    γ = dev(Q['γ'])
    Mt = fused.sequence_rfgr(rf, gr[None], dev(Q['loc']), pulse=Q['pulse'], phase=dev(Q['phase']), rest=rest, T1=T1,
                             T2=dev(Q['T2']), Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']))
    (Mt.movedim(-2, 0) * dev(Q['w'])).sum().backward()
    return dict(Mt=Mt.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)


@pytest.mark.parametrize('tag_mode', MODES)
def test_against_the_reference_fixture(tag_mode):
    r"""fp64: the records (the reference's simulators, 24 repetitions of a bank of three pulses with a rest per
    repetition) and ``grad_rf`` (of the bank), ``grad_gr``, ``grad_T1``, ``grad_rest`` at the project's gate.  fp32, precise
    and fast: the distances to the fp64 fixture go to the ledger and are held to 3 x ``distance_f32_vs_f64.*``, what the
    reference's own all-fp32 route loses on the same numbers."""
    tag, mode = _mode(tag_mode)
    G, G64 = golden(f'sequence_{tag}'), golden('sequence_f64')
    Q = fixture_inputs(G)
    with mode:
        got = _fixture_run(Q)
    assert set(got) == set(OUT) and got['Mt'].shape == (2, 100, 24, 3)
    assert got['grad_rf'].shape == (3, 2, 2, 48) and got['grad_gr'].shape == (2, 3, 48) and got['grad_rest'].shape == (2, 24)
    if tag == 'f64':
        for k in OUT:
            d = record(f'sequence.f64.fixture.{k}', max_abs(got[k], G[k]))
            print(f'f64 {k}: {d:.3e} max abs from the reference fixture')
        for k in OUT:
            assert_close(got[k], G[k], 'f64', f'{k} vs the reference fixture')
        return
    wide = oracle_sequence(Q, torch.float64)
    for k in OUT:
        bound = 3 * float(G[f'distance_f32_vs_f64.{k}'])
        record(f'sequence.{tag_mode}.fixture.{k}.vs_yardstick64_on_the_same_numbers', rel_l2(got[k], wide[k]))
        record(f'sequence.{tag_mode}.fixture.{k}.reference_f32_vs_fixture64', rel_l2(G[k], G64[k]))
        d = record(f'sequence.{tag_mode}.fixture.{k}.vs_fixture64', rel_l2(got[k], G64[k]), bound)
        print(f'{tag_mode} {k}: {d:.3e} from the fp64 fixture, bound {bound:.3e}')
    for k in OUT:
        d, bound = rel_l2(got[k], G64[k]), 3 * float(G[f'distance_f32_vs_f64.{k}'])
        assert d <= bound, f'{k}: {d:.3e} from the fp64 fixture > 3 x the reference\'s own fp32 distance = {bound:.3e}'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_parallel_transmit_runs_through_the_fused_ab(tag, monkeypatch):
    r"""4 transmit coils with their ``b1Map`` (``test_fused_traj._problem(.., 'ptx4', 48)``) as a bank of two pulses -- the
    second at 0.6 of the first --, the fixture's rests and phases, 8 repetitions: ``A, B`` come from ONE
    ``mrphy_ab_rfgr_mc_fwd`` call on the batch ``P·N``, and the records are the yardstick's on ``beff2ab(rfgr2beff(.))``
    of the device, entry by entry."""
    K, pulse = 8, [0, 1, 1, 0, 1, 0, 0, 1]
    P = _problem(tag, 'ptx4', 48)
    Q = fixture_inputs(golden(f'sequence_{tag}'))
    rest, phase = dev(Q['rest'][:, :K].contiguous()), dev(Q['phase'][:, :K].contiguous())
    γ, dt, T1, T2, df = (dev(P[k]) for k in ('γ', 'dt', 'T1', 'T2', 'df'))
    rf = torch.stack((dev(P['rf']), 0.6 * dev(P['rf'])))
    # beff2ab's own four constants, formed once on the device and handed over as `consts=`: A, B are then its bits
    E1, E2 = torch.exp(-dt[:, None] / T1), torch.exp(-dt[:, None] / T2)
    consts = dict(γ2πdt=2 * π * _host.pad_trailing(γ, 2) * _host.pad_trailing(dt, 2), E1=E1, E2=E2, E1_1=E1 - 1)
    calls = _counted(monkeypatch, ('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd', 'mrphy_beff2ab', FWD, 'mrphy_ab_train_fwd'))
    with torch.no_grad():
        Mt = fused.sequence_rfgr(rf, dev(P['gr'])[None], dev(P['loc']), pulse=pulse, phase=phase, rest=rest, T1=T1, T2=T2,
                                 Δf=df, b1Map=dev(P['b1']), γ_beff=γ, consts=consts)
        assert dict(calls) == {'mrphy_ab_rfgr_mc_fwd': 1, FWD: 1}
        AB = [beffective.beff2ab(beffective.rfgr2beff(rf[p], dev(P['gr']), dev(P['loc']), Δf=df, b1Map=dev(P['b1']), γ=γ),
                                 E1=E1, E2=E2, γ=γ, dt=dt) for p in range(2)]
        A, B = torch.stack([a for a, _ in AB]).double().cpu(), torch.stack([b for _, b in AB]).double().cpu()
        want = torch_sequence(A, B, K, pulse, None, phase.double().cpu(), rest.double().cpu(), T1.double().cpu(),
                              T2.double().cpu(), df.double().cpu())
    assert Mt.shape == (2, 100, K, 3) and Mt.dtype == DT[tag]
    _gate(Mt.cpu(), want, tag, 'Mt under parallel transmit')


# =============================================================================================
# 9. memory
# =============================================================================================
def test_nothing_per_repetition_is_kept_besides_the_output():
    r"""P = 4, N = 1, nM = 4096, K = 64 in fp32 with a rest per repetition, ``A``, ``B``, ``T1`` requiring grad as in
    ``test_ab_train``, the cotangent allocated beforehand (it counts among the inputs): over forward + backward the
    allocator's peak stays below the inputs, ``Mt`` and its cotangent, the bank's gradients and the fp64 workspace the
    query reports, plus 1 MB -- nothing of size ``K × spins`` is kept besides the output."""
    P_, N, nM, K = 4, 1, 4096, 64
    gen = torch.Generator().manual_seed(9)
    Qm = torch.linalg.qr(torch.randn((P_, N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    A = dev((0.97 * Qm).float()).requires_grad_(True)
    B = dev(torch.randn((P_, N, nM, 3), generator=gen)).requires_grad_(True)
    T1 = dev(0.05 + 0.1 * torch.rand((N, nM), generator=gen)).requires_grad_(True)
    T2 = dev(0.02 + 0.05 * torch.rand((N, nM), generator=gen))
    rest = dev(2e-3 + 8e-3 * torch.rand((N, K), generator=gen))
    phase = dev(2 * torch.randn((N, K), generator=gen))
    pulse = [(3 * k) % P_ for k in range(K)]
    w = dev(_weights(K, N, nM, torch.float32))
    torch.cuda.synchronize()
    inputs = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    Mt = fused.ab_sequence(A, B, pulse=pulse, phase=phase, rest=rest, T1=T1, T2=T2)
    Mt.backward(w.movedim(0, -2))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    records = K * N * nM * 3 * 4
    bank = P_ * N * nM * 12 * 4
    work = int(mrphy_amd.require_library().mrphy_ab_sequence_bwd_workspace(_lib.F32, P_, N, nM))
    assert work == P_ * 12 * N * nM * 8
    budget = inputs + records + bank + work + (1 << 20)                      # (w, the cotangent, is among the inputs)
    print(f'peak {peak} B; inputs {inputs} B, Mt {records} B, bank gradients {bank} B, workspace {work} B')
    assert A.grad is not None and B.grad is not None and float(T1.grad.abs().max()) > 0
    assert inputs + records <= peak < budget, (peak, budget)
