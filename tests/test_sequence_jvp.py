r"""``fused.ab_sequence_jvp`` (Ksqj: ``mrphy_ab_sequence_jvp_fwd``), ``fused.ab_rfgr_jvp`` and ``fused.sequence_rfgr_jvp`` on
the device.

What is claimed where.  Ksqj carries the tangents in fp64 beside Ksq's fp64 state and rounds each record once, so the
kernel ALONE is held to the family's gate (``test_steadystate._gate``) against ``torch.autograd.functional.jvp`` of the
recursion in plain torch on the CPU (``test_sequence_jvp_host.oracle_sequence_jvp``) on the same rounded numbers: fp64
max abs 1e-9 in units of ``max(1, max|want|)``, fp32 relative L2 1e-6 -- per group and direction, each against that
direction's own norm, because the groups' tangents differ by orders of magnitude (§1, §3, §4).  The bit-level claims of the
design are ``torch.equal`` (§2).  The dot-product identity with the adjoint Ksqb ties the two derivative kernels together
at 1e-12 (§5).  End to end from ``rf`` and ``gr`` (§6) fp32 inherits the rounding of ``A`` amplified by the train's
conditioning and the difference ``dMo|e_j - dMo|0``: the distance to the fp64 yardstick on the same numbers is held to
``max(REL32, 3 d32)``, where ``d32`` is what the yardstick's own all-fp32 forward-mode run on the CPU loses on those
numbers -- computed here from the oracle, never from the code under test; the margin and reason of ``test_ab_train.py`` §8
and ``test_ab_sequence.py`` §8."""
import functools

import pytest

from gpu_common import *  # noqa: F401,F403
from test_ab_sequence import SHAPES, IDS, S7, _kernel_problem
from test_ab_sequence_host import oracle_bank, torch_sequence
from test_sequence_jvp_host import (FIXTURE_GROUPS, FIXTURE_KEY, GROUPS, fixture_problem, oracle_bank_jvp,
                                    oracle_sequence_jvp)
from test_steadystate import _mode
from util import REL32

pytestmark = pytest.mark.gpu

KEY = dict(A='A', B='B', Mi='Mi', phase='phase', rest='rest', T1='T1', T2='T2', df='Δf')     # yardstick name -> keyword
SCALE = dict(A=1.0, B=1.0, Mi=1.0, phase=1.0, rest=3e-3, T1=0.05, T2=0.02, df=100.0)


def _gate(got, want, tag, what):
    r"""``test_steadystate._gate`` for a tangent: fp64 max abs <= 1e-9 in units of ``max(1, max|want|)``, fp32 relative
    L2 <= 1e-6 against the direction's own norm.  Returns the distance."""
    want = torch.as_tensor(want).detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), what
    if tag == 'f64':
        d = max_abs(got, want) / max(1.0, float(want.abs().max()) if want.numel() else 0.0)
        assert d <= 1e-9, f'{what}: max abs over max(1, max|want|) {d:.3e} > 1e-9'
    else:
        d = rel_l2(got, want)
        assert d <= 1e-6, f'{what}: rel-L2 {d:.3e} > 1e-6'
    return d


@functools.lru_cache(maxsize=None)
def _directions(shape, tag):
    r"""One seeded tangent per group, of its operand's shape, in the data type, on the CPU.  Never modified."""
    P, _ = _kernel_problem(shape, tag)
    gen = torch.Generator().manual_seed(77 + sum(shape))
    return {g: ((torch.rand(P[g].shape, generator=gen, dtype=torch.float64) * 2 - 1) * SCALE[g]).to(DT[tag]) for g in GROUPS}


def _stack(V, rows):
    r"""``tangents`` on the device for the directions ``rows``: each row is ``{group: factor}``, a direction that holds
    ``factor`` times the seeded tangent of each of its groups."""
    gs = [g for g in GROUPS if any(g in r for r in rows)]
    return {KEY[g]: dev(torch.stack([V[g] * r.get(g, 0.0) for r in rows])) for g in gs}


SINGLES = [{g: 1.0} for g in GROUPS]
ALL = {g: 1.0 for g in GROUPS}


def _call(P, tangents, use=GROUPS[2:], over=None):
    r"""``ab_sequence_jvp`` on the device on the problem ``P`` with the optional operands ``use`` (``over``: replacements,
    by keyword)."""
    kw = {KEY[k]: dev(P[k]) for k in use}
    kw.update(over or {})
    return fused.ab_sequence_jvp(dev(P['A']), dev(P['B']), tangents=tangents, pulse=list(P['pulse']), **kw)


def _want(P, K, direction, use=GROUPS[2:]):
    Q = {k: P[k] for k in ('A', 'B', 'pulse') + tuple(use)}
    return oracle_sequence_jvp(Q, K, direction)


# =============================================================================================
# 1. every group alone and all at once, at every shape
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_each_group_alone_and_all_at_once_against_the_oracle(tag, shape):
    r"""The shapes of ``test_ab_sequence`` §1 (one spin and one repetition; two grid rows; runs of 1 and 2 with a return and
    an entry never played, a zero rest and a run of equal rests; a reload per repetition; a second, ragged block), nine
    directions in one call -- the capacity 4 twice and the capacity 1 --: ``Mt`` is ``ab_sequence``'s by ``torch.equal``,
    each ``dMt[d]`` within the gate of the oracle; a second run gives the same bits."""
    P_, N, nM, K = shape
    P, _ = _kernel_problem(shape, tag)
    V = _directions(shape, tag)
    rows = SINGLES + [ALL]
    Mt, dMt = _call(P, _stack(V, rows))
    assert Mt.dtype == dMt.dtype == DT[tag] and Mt.shape == (N, nM, K, 3) and dMt.shape == (len(rows), N, nM, K, 3)
    assert not Mt.requires_grad and not dMt.requires_grad
    with torch.no_grad():
        plain = fused.ab_sequence(dev(P['A']), dev(P['B']), pulse=list(P['pulse']), **{KEY[k]: dev(P[k]) for k in GROUPS[2:]})
    assert torch.equal(Mt, plain), 'Mt is ab_sequence\'s, bit for bit'
    dist = {}
    for i, row in enumerate(rows):
        name = 'all' if len(row) > 1 else next(iter(row))
        want = _want(P, K, {g: V[g] for g in row})[1]
        assert float(want.norm()) > 0, name
        dist[name] = (dMt[i], want)
        print(f'{tag} {shape} {name}: max abs {max_abs(dMt[i], want):.3e} rel-L2 {rel_l2(dMt[i], want):.3e} '
              f'|want| max {float(want.abs().max()):.3e}')
    for name, (got, want) in dist.items():
        d = _gate(got, want, tag, f'dMt along {name}')
        record(f'sequence_jvp.{tag}.P{P_}_N{N}_nM{nM}_K{K}.{name}', d, 1e-9 if tag == 'f64' else 1e-6)
    Mt2, dMt2 = _call(P, _stack(V, rows))
    assert torch.equal(Mt2, Mt) and torch.equal(dMt2, dMt), 'a second run gives the same bits'


# =============================================================================================
# 2. bits
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_direction_has_the_bits_of_the_call_with_it_alone(tag):
    r"""``D`` in {1, 2, 3, 4, 5, 9}: every capacity, a capacity not filled, more directions than the largest one."""
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    rows = SINGLES + [ALL]
    alone = [_call(P, _stack(V, [r])) for r in rows]
    for Mt, _ in alone[1:]:
        assert torch.equal(Mt, alone[0][0])
    for D in (2, 3, 4, 5, 9):
        Mt, dMt = _call(P, _stack(V, rows[:D]))
        assert dMt.shape[0] == D and torch.equal(Mt, alone[0][0])
        for d in range(D):
            assert float(alone[d][1].abs().max()) > 0
            assert torch.equal(dMt[d], alone[d][1][0]), f'direction {d} of {D}'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_direction_scales_exactly_and_zero_tangents_give_zeros(tag):
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    scaled = lambda f: {g: f for g in GROUPS}  # noqa: E731
    _, dMt = _call(P, _stack(V, [ALL, scaled(2.0), scaled(0.125), scaled(-1.0), scaled(0.0)]))
    assert float(dMt[0].abs().min()) > 0
    assert torch.equal(dMt[1], 2 * dMt[0]) and torch.equal(dMt[2], 0.125 * dMt[0]) and torch.equal(dMt[3], -dMt[0])
    assert float(dMt[4].abs().max()) == 0.0, 'all-zero tangents give exact zeros'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_tangents_on_an_entry_never_played_give_exact_zeros(tag):
    P, _ = _kernel_problem(S7, tag)
    assert 1 not in P['pulse']
    V = _directions(S7, tag)
    dA, dB = torch.zeros_like(V['A']), torch.zeros_like(V['B'])
    dA[1], dB[1] = V['A'][1], V['B'][1]
    _, dMt = _call(P, dict(A=dev(dA[None]), B=dev(dB[None])))
    assert float(dMt.abs().max()) == 0.0
    dA[0] = V['A'][0]
    assert float(_call(P, dict(A=dev(dA[None])))[1].abs().max()) > 0


# =============================================================================================
# 3. special cases
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_a_run_of_equal_rests_with_differing_rest_tangents(tag):
    r"""One duration for all repetitions -- the rest's constants are formed once -- and a tangent of it per repetition: the
    tangents of the constants are not tied to the refresh."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    rest = P['rest'][:, 2].contiguous()
    assert float((V['rest'][:, 1:] - V['rest'][:, :-1]).abs().min()) > 0
    Mt, dMt = _call(P, dict(rest=dev(V['rest'][None])), over=dict(rest=dev(rest)))
    Q = dict(P, rest=rest[:, None].expand(N, K))
    want_Mt, want = _want(Q, K, dict(rest=V['rest']))
    _gate(dMt[0], want, tag, 'drest per repetition on one duration')
    _gate(Mt, want_Mt, tag, 'Mt')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_zero_rests(tag):
    r"""``rest_k = 0`` at every repetition: ``c = e1 = e2 = 1``, ``s = f3 = 0``, and the tangents w.r.t. ``rest``, ``T1``,
    ``T2``, ``Δf`` are those of the limit."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    assert float(P['rest'][:, 3].abs().max()) == 0, 'the seeded problem has a zero rest too'
    V = _directions(S7, tag)
    Q = dict(P, rest=torch.zeros_like(P['rest']))
    rows = [{g: 1.0} for g in ('rest', 'T1', 'T2', 'df')] + [ALL]
    _, dMt = _call(Q, _stack(V, rows))
    for i, row in enumerate(rows):
        want = _want(Q, K, {g: V[g] for g in row})[1]
        _gate(dMt[i], want, tag, f'zero rests: {sorted(row)}')
    assert float(dMt[0].abs().max()) > 0, 'a rest about to begin moves the records'
    for i in (1, 2, 3):
        assert float(dMt[i].abs().max()) == 0, 'T1, T2, Δf act through a rest of no duration: exact zeros'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_without_a_rest(tag):
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    use = ('Mi', 'phase')
    rows = [{g: 1.0} for g in ('A', 'B', 'Mi', 'phase')] + [{g: 1.0 for g in ('A', 'B', 'Mi', 'phase')}]
    Mt, dMt = _call(P, _stack(V, rows), use=use)
    with torch.no_grad():
        assert torch.equal(Mt, fused.ab_sequence(dev(P['A']), dev(P['B']), pulse=list(P['pulse']), Mi=dev(P['Mi']),
                                                 phase=dev(P['phase'])))
    for i, row in enumerate(rows):
        _gate(dMt[i], _want(P, K, {g: V[g] for g in row}, use)[1], tag, f'no rest: {sorted(row)}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_no_repetitions_give_empty_outputs(tag):
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    Mt, dMt = fused.ab_sequence_jvp(dev(P['A']), dev(P['B']), n=0, pulse=[], Mi=dev(P['Mi']),
                                    tangents=dict(A=dev(V['A'].expand(5, *V['A'].shape)), Mi=dev(V['Mi'].expand(5, 2, 100, 3))))
    assert Mt.shape == (2, 100, 0, 3) and dMt.shape == (5, 2, 100, 0, 3) and Mt.dtype == dMt.dtype == DT[tag]


# =============================================================================================
# 4. operand forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['1Nd', 'N1', 'none'])
def test_forms_of_Mi(tag, form):
    r"""``Mi`` `(1, *Nd, 3)` / `(N, 1, 3)` with a tangent in the same form, and ``None`` -- the value ``(0, 0, 1)`` -- with a
    full tangent."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    Mi, dMi = {'1Nd': (P['Mi'][:1], V['Mi'][:1]), 'N1': (P['Mi'][:, :1], V['Mi'][:, :1]), 'none': (None, V['Mi'])}[form]
    use = ('phase', 'rest', 'T1', 'T2', 'df')
    over = {} if Mi is None else dict(Mi=dev(Mi.contiguous()))
    Mt, dMt = _call(P, dict(Mi=dev(dMi.contiguous()[None])), use=use, over=over)
    Q = dict(P, Mi=None if Mi is None else Mi.expand(N, nM, 3))
    want_Mt, want = oracle_sequence_jvp(Q, K, dict(Mi=dMi.expand(N, nM, 3)))
    _gate(dMt[0], want, tag, f'Mi {form}')
    _gate(Mt, want_Mt, tag, 'Mt')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', 'N', '1K', 'NK'])
def test_forms_of_rest(tag, form):
    r"""``rest`` `()`, `(N,)`, `(1, K)`, `(N, K)` with its tangent in the same form."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    take = {'0dim': lambda x: x[0, 2], 'N': lambda x: x[:, 2], '1K': lambda x: x[:1], 'NK': lambda x: x}[form]
    rest, drest = take(P['rest']).contiguous(), take(V['rest']).contiguous()
    table = lambda x: x.reshape(-1, 1).expand(-1, K) if x.ndim < 2 else x  # noqa: E731
    Mt, dMt = _call(P, dict(rest=dev(drest[None])), over=dict(rest=dev(rest)))
    want_Mt, want = oracle_sequence_jvp(dict(P, rest=table(rest)), K, dict(rest=table(drest)))
    _gate(dMt[0], want, tag, f'rest {form}')
    _gate(Mt, want_Mt, tag, 'Mt')
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_broadcast_axes_views_and_a_0dim_constant(tag):
    r"""``T1`` 0-dim with ``dT1`` `(D, N, nM)`; tangents with broadcast axes of 1 (``dA`` `(D, 1, N, 1, 3, 3)`, ``dB``
    `(D, P, 1, nM, 1)`, ``dT2`` `(D, 1, 1)`, ``dΔf`` `(D,)`, ``dphase`` `(D, 1, K)`); and the same call on non-contiguous
    views of the operands and the tangents gives the same bits."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, tag)
    V = _directions(S7, tag)
    T1 = P['T1'][0, 0].clone()
    v = dict(A=V['A'][:1, :, :1], B=V['B'][:, :1, :, :1], T1=V['T1'], T2=V['T2'][:1, :1], df=V['df'][0, 0], phase=V['phase'][:1])
    tangents = {KEY[g]: dev(x.contiguous()[None]) for g, x in v.items()}
    Mt, dMt = _call(P, tangents, over=dict(T1=dev(T1)))
    full = dict(A=v['A'].expand(P_, N, nM, 3, 3), B=v['B'].expand(P_, N, nM, 3), T1=v['T1'], T2=v['T2'].expand(N, nM),
                df=v['df'].expand(N, nM), phase=v['phase'].expand(N, K))
    want_Mt, want = oracle_sequence_jvp(dict(P, T1=T1.expand(N, nM)), K, full)
    _gate(dMt[0], want, tag, 'broadcast tangents')
    _gate(Mt, want_Mt, tag, 'Mt')
    # views: A, B with the bank axis permuted in storage, tangents strided
    A_v = dev(P['A']).movedim(0, 1).contiguous().movedim(1, 0)
    B_v = dev(P['B']).movedim(0, 2).contiguous().movedim(2, 0)
    assert not A_v.is_contiguous() and not B_v.is_contiguous()
    strided = lambda x: torch.stack((x, x), dim=-1)[..., 0] if x.ndim else x  # noqa: E731
    tan_v = {k: strided(x) for k, x in tangents.items()}
    assert not tan_v['A'].is_contiguous() and not tan_v['T1'].is_contiguous()
    kw = {KEY[k]: dev(P[k]) for k in GROUPS[2:]}
    kw['T1'] = dev(T1)
    Mt_v, dMt_v = fused.ab_sequence_jvp(A_v, B_v, tangents=tan_v, pulse=list(P['pulse']), **kw)
    assert torch.equal(Mt_v, Mt) and torch.equal(dMt_v, dMt)


def test_half_inputs_are_computed_in_fp32():
    P, _ = _kernel_problem(S7, 'f32')
    V = _directions(S7, 'f32')
    A, B, dB = dev(P['A']).half(), dev(P['B']).half(), dev(V['B'][None]).half()
    Mt, dMt = fused.ab_sequence_jvp(A, B, tangents=dict(B=dB), pulse=list(P['pulse']))
    assert Mt.dtype == dMt.dtype == torch.float16
    Mt32, dMt32 = fused.ab_sequence_jvp(A.float(), B.float(), tangents=dict(B=dB.float()), pulse=list(P['pulse']))
    assert Mt32.dtype == torch.float32 and torch.equal(Mt, Mt32.half()) and torch.equal(dMt, dMt32.half())
    assert float(dMt.float().abs().max()) > 0


# =============================================================================================
# 5. the dot-product identity with the adjoint
# =============================================================================================
def test_dot_product_identity_with_the_adjoint():
    r"""fp64: ``<w, J v> = <J^T w, v>`` for one direction ``v`` holding all eight groups, ``J v`` from Ksqj and ``J^T w`` from
    Ksqb (``ab_sequence(...).backward`` under the cotangent ``w``); the two share no code beyond ``train_rep``.  Relative
    difference <= 1e-12."""
    P_, N, nM, K = S7
    P, _ = _kernel_problem(S7, 'f64')
    V = _directions(S7, 'f64')
    _, dMt = _call(P, _stack(V, [ALL]))
    w = dev(P['w']).reshape(K, N, nM, 3).movedim(0, -2)
    lhs = float((w.double().cpu() * dMt[0].double().cpu()).sum())
    L = {g: dev(P[g]).clone().requires_grad_(True) for g in GROUPS}
    Mt = fused.ab_sequence(L['A'], L['B'], pulse=list(P['pulse']), **{KEY[g]: L[g] for g in GROUPS[2:]})
    Mt.backward(w)
    parts = {g: float((L[g].grad.double().cpu() * V[g].double()).sum()) for g in GROUPS}
    rhs = sum(parts.values())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f'<w, J v> = {lhs:.17g}, <J^T w, v> = {rhs:.17g}, relative difference {rel:.3e}; per group {parts}')
    record('sequence_jvp.f64.dot_product_identity', rel, 1e-12)
    assert all(abs(x) > 0 for x in parts.values())
    assert rel <= 1e-12, rel


# =============================================================================================
# 6. from rf and gr: ab_rfgr_jvp and sequence_rfgr_jvp on the fixture's problem
# =============================================================================================
def _pulse_kw(Q):
    γ = dev(Q['γ'])
    return dict(T1=dev(Q['T1']), T2=dev(Q['T2']), Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']))


def _fixture_tangents(V, groups):
    r"""One direction per group of ``groups`` and one that holds them all, ``(D, *operand)`` on the device."""
    D = len(groups) + 1
    out = {}
    for i, g in enumerate(groups):
        t = torch.zeros((D,) + tuple(V[g].shape), dtype=V[g].dtype)
        t[i] = t[-1] = V[g]
        out[g] = dev(t)
    return out


def _bound32(tag_mode, name, got, P, direction, oracle, pick=lambda x: x):
    r"""fp32: the device's distance from the fp64 oracle on the same fp32 numbers against ``max(REL32, 3 d32)``, ``d32`` the
    oracle's own all-fp32 run's distance from it; both go to the ledger; asserted in precise mode."""
    want, own = pick(oracle(P, direction, torch.float64)), pick(oracle(P, direction, torch.float32))
    d32, d = rel_l2(own, want), rel_l2(got, want)
    bound = max(REL32, 3 * d32)
    record(f'sequence_jvp.{tag_mode}.fixture.{name}.oracle_f32_vs_f64', d32)
    record(f'sequence_jvp.{tag_mode}.fixture.{name}.vs_oracle64_on_the_same_numbers', d, bound if 'fast' not in tag_mode else None)
    print(f'{tag_mode} {name}: device {d:.3e} from the fp64 oracle, the oracle\'s own fp32 run {d32:.3e}, bound {bound:.3e}')
    return d, bound


@pytest.mark.parametrize('tag_mode', ['f64', 'f32-precise', 'f32-fast'])
def test_sequence_rfgr_jvp_against_the_oracle_on_the_fixtures_problem(tag_mode):
    r"""The fixture's problem (``sequence_f64.npz``, 50 spins; the oracle's tangents on it are pinned to the reference's by
    ``test_sequence_jvp_host.py``): six groups alone and all at once through ``ab_rfgr_jvp`` on the batch ``P·N`` and Ksqj.
    fp64 at the 1e-9 gate; fp32 precise at ``max(REL32, 3 d32)``; fp32 fast: ledger only."""
    tag, mode = _mode(tag_mode)
    P, V, _ = fixture_problem(DT[tag])
    names = list(FIXTURE_GROUPS) + ['all']
    with mode:
        Mt, dMt = fused.sequence_rfgr_jvp(dev(P['rf']), dev(P['gr'])[None], dev(P['loc']), tangents=_fixture_tangents(V, FIXTURE_GROUPS),
                                          pulse=P['pulse'], phase=dev(P['phase']), rest=dev(P['rest']), **_pulse_kw(P))
        with torch.no_grad():
            plain = fused.sequence_rfgr(dev(P['rf']), dev(P['gr'])[None], dev(P['loc']), pulse=P['pulse'], phase=dev(P['phase']),
                                        rest=dev(P['rest']), **_pulse_kw(P))
    assert torch.equal(Mt, plain) and dMt.shape == (7, 2, 50, 24, 3) and dMt.dtype == DT[tag]
    late = []
    for i, name in enumerate(names):
        direction = {g: V[g] for g in (FIXTURE_GROUPS if name == 'all' else (name,))}
        if tag == 'f64':
            want = oracle_bank_jvp(P, direction)[1]
            d = record(f'sequence_jvp.f64.fixture.{name}', max_abs(dMt[i], want) / max(1.0, float(want.abs().max())), 1e-9)
            print(f'f64 {name}: {d:.3e} of max(1, max|want|) from the oracle')
            late.append((d, 1e-9, name))
        else:
            late.append(_bound32(tag_mode, name, dMt[i], P, direction, oracle_bank_jvp, pick=lambda x: x[1]) + (name,))
    if tag_mode != 'f32-fast':
        for d, bound, name in late:
            assert d <= bound, f'{name}: {d:.3e} > {bound:.3e}'


def _oracle_ab_jvp(P, direction, dtype):
    r"""``(A, B, dA, dB)`` of bank entry 0 by ``jvp`` of ``oracle_bank`` in ``dtype``."""
    P = {k: (v if k == 'pulse' else v.to(dtype)) for k, v in P.items()}
    ks = list(direction)

    def f(*xs):
        q = dict(P, **{FIXTURE_KEY.get(g, g): x for g, x in zip(ks, xs)})
        A, B = oracle_bank(q, q['rf'][:1], q['gr'], q['T1'])
        return A[0], B[0]
    (A, B), (dA, dB) = torch.autograd.functional.jvp(f, tuple(P[FIXTURE_KEY.get(g, g)] for g in ks),
                                                     tuple(direction[g].to(dtype) for g in ks))
    return A, B, dA, dB


@pytest.mark.parametrize('tag_mode', ['f64', 'f32-precise', 'f32-fast'])
def test_ab_rfgr_jvp_against_the_oracle(tag_mode):
    r"""Bank entry 0 of the fixture's problem: ``A, B`` are ``ab_rfgr``'s bits; ``dA, dB`` along ``T1, T2, Δf, b1Map, rf`` and
    all of them against ``jvp`` of the oracle's ``rfgr2beff -> beff2ab``."""
    tag, mode = _mode(tag_mode)
    P, V, _ = fixture_problem(DT[tag])
    groups = ('T1', 'T2', 'Δf', 'b1Map', 'rf')
    V = dict(V, rf=V['rf'][0])
    with mode:
        A, B, dA, dB = fused.ab_rfgr_jvp(dev(P['rf'][0]), dev(P['gr']), dev(P['loc']), tangents=_fixture_tangents(V, groups),
                                         **_pulse_kw(P))
        with torch.no_grad():
            A0, B0 = fused.ab_rfgr(dev(P['rf'][0]), dev(P['gr']), dev(P['loc']), **_pulse_kw(P))
    assert torch.equal(A, A0) and torch.equal(B, B0)
    assert dA.shape == (6, 2, 50, 3, 3) and dB.shape == (6, 2, 50, 3)
    Vb = dict(V, rf=torch.cat((V['rf'][None], torch.zeros_like(P['rf'][1:]))))
    late = []
    for i, name in enumerate(groups + ('all',)):
        direction = {g: Vb[g] for g in (groups if name == 'all' else (name,))}
        for what, got, at in (('dA', dA[i], 2), ('dB', dB[i], 3)):
            if tag == 'f64':
                want = _oracle_ab_jvp(P, direction, torch.float64)[at]
                d = record(f'ab_rfgr_jvp.f64.{name}.{what}', max_abs(got, want) / max(1.0, float(want.abs().max())), 1e-9)
                late.append((d, 1e-9, f'{what} along {name}'))
            else:
                late.append(_bound32(tag_mode, f'ab_rfgr.{name}.{what}', got, P, direction, _oracle_ab_jvp,
                                     pick=lambda x, at=at: x[at]) + (f'{what} along {name}',))
    if tag_mode != 'f32-fast':
        for d, bound, name in late:
            assert d <= bound, f'{name}: {d:.3e} > {bound:.3e}'


def test_a_rest_off_resonance_of_its_own_is_routed_to_the_rests():
    r"""fp64, ``Δf_rest``: the key ``Δf`` feeds only the pulses, ``Δf_rest`` only the rests."""
    P, V, _ = fixture_problem()
    K = P['phase'].shape[1]
    dfr, ddfr = 0.5 * P['df'].flip(1), V['Δf'].flip(1)
    tangents = {'Δf': dev(torch.stack((V['Δf'], torch.zeros_like(ddfr), V['Δf']))),
                'Δf_rest': dev(torch.stack((torch.zeros_like(ddfr), ddfr, ddfr)))}
    Mt, dMt = fused.sequence_rfgr_jvp(dev(P['rf']), dev(P['gr'])[None], dev(P['loc']), tangents=tangents, pulse=P['pulse'],
                                      phase=dev(P['phase']), rest=dev(P['rest']), Δf_rest=dev(dfr), **_pulse_kw(P))

    def f(df, dr):
        A, B = oracle_bank(dict(P, df=df), P['rf'], P['gr'], P['T1'])
        return torch_sequence(A, B, K, P['pulse'].tolist(), None, P['phase'], P['rest'], P['T1'], P['T2'], dr)
    z = torch.zeros_like(ddfr)
    for i, (v1, v2) in enumerate(((V['Δf'], z), (z, ddfr), (V['Δf'], ddfr))):
        want_Mt, want = torch.autograd.functional.jvp(f, (P['df'], dfr), (v1, v2))
        assert float(want.abs().max()) > 0
        _gate(dMt[i], want, 'f64', f'Δf_rest routing, direction {i}')
    _gate(Mt, want_Mt, 'f64', 'Mt')
    assert rel_l2(dMt[0], dMt[1]) > 0.1, 'the two routes differ'


def test_parallel_transmit_is_not_implemented():
    P, V, _ = fixture_problem(torch.float32)
    rf = dev(P['rf'])[..., None].expand(3, 2, 2, 48, 2).contiguous()
    b1 = dev(P['b1'])[..., None].expand(2, 50, 2, 2).contiguous()
    kw = dict(_pulse_kw(P), b1Map=b1)
    with pytest.raises(NotImplementedError, match='parallel transmit'):
        fused.ab_rfgr_jvp(rf[0], dev(P['gr']), dev(P['loc']), tangents=dict(T1=dev(V['T1'][None])), **kw)
    with pytest.raises(NotImplementedError, match='parallel transmit'):
        fused.sequence_rfgr_jvp(rf, dev(P['gr'])[None], dev(P['loc']), tangents=dict(T1=dev(V['T1'][None])), pulse=P['pulse'],
                                phase=dev(P['phase']), rest=dev(P['rest']), **kw)
