r"""``fused.ab_train`` (Ktr / Ktrb: ``mrphy_ab_train_fwd`` / ``_bwd``) and ``fused.train_rfgr`` on the device.

What is claimed where.  The kernels carry the recursion in fp64 and round each record once, so ALONE they are held tight
(``test_steadystate._gate``): against the fp64 recursion in plain torch on the CPU (``test_ab_train_host.torch_train``)
on the same numbers, fp64 max abs 1e-9 and fp32 relative L2 1e-6, the records and all eight gradients (§1 - §5).  The
fp32 budget: the adjoint reads records rounded to fp32 (2^-24 relative each) and the sums run in fp64; the kernel's
arithmetic emulated on the CPU lies 2e-8 .. 8e-8 from exact autograd at (2, 200, 40), a factor of 12 inside the gate.
End to end in fp32 (§8) the result inherits the rounding of ``A`` amplified by the train's conditioning, so the distance
to the fp64 fixture is held to three times what the reference's own all-fp32 route loses on the same numbers, the margin
and reason of ``test_steadystate.py`` §5.
"""
import functools
from math import pi as π

import pytest

from gpu_common import *  # noqa: F401,F403
from mrphy_amd import _host
from test_ab_rfgr import _counted
from test_ab_rfgr_host import fixture_inputs
from test_ab_train_host import identity_problem, oracle_train, rz, torch_train
from test_fused_traj import _problem
from test_steadystate import _form, _gate, _mode
from test_steadystate_host import rest_period

pytestmark = pytest.mark.gpu

MODES = ['f64', 'f32-precise', 'f32-fast']
OPS = ('Mi', 'phase', 'rest', 'T1', 'T2', 'df')       # the optional operands; A, B are always there
KW = dict(Mi='Mi', phase='phase', rest='rest', T1='T1', T2='T2', df='Δf')
FWD, BWD = 'mrphy_ab_train_fwd', 'mrphy_ab_train_bwd'


def _weights(K, N, nM, dtype):
    return torch.sin(torch.arange(K * N * nM * 3, dtype=torch.float64) * 0.37 + 0.3).reshape(K, N, nM, 3).to(dtype)


@functools.lru_cache(maxsize=None)
def _kernel_problem(N, nM, K, tag):
    r"""Seeded ``A = 0.97 Q`` (``Q`` orthogonal), ``B``, ``Mi``, phases ``2 randn``, the rest's operands of
    ``test_steadystate._kernel_problem`` and time-major weights ``w`` in the data type, on the CPU; and the fp64
    yardstick of the same numbers.  Computed once per shape, never modified."""
    gen = torch.Generator().manual_seed(100000 * N + 100 * nM + K)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    P = dict(A=0.97 * Q, B=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             Mi=torch.randn((N, nM, 3), generator=gen, dtype=torch.float64),
             phase=2 * torch.randn((N, K), generator=gen, dtype=torch.float64),
             rest=torch.tensor([5e-3, 6.5e-3], dtype=torch.float64)[:N], T1=0.05 + 0.1 * rnd(N, nM),
             T2=0.02 + 0.05 * rnd(N, nM), df=(rnd(N, nM) * 2 - 1) * 200, w=_weights(K, N, nM, torch.float64))
    P = {k: v.to(DT[tag]) for k, v in P.items()}
    return P, _yardstick(P, K)


def _yardstick(P, K, use=OPS):
    r"""The records and the gradients of ``(Mt w).sum()`` w.r.t. ``A, B`` and the operands ``use`` by ``torch_train`` and
    autograd in fp64 on the CPU; operands not in ``use`` are absent."""
    L = {k: P[k].double().clone().requires_grad_(True) for k in ('A', 'B') + tuple(use)}
    Mt = torch_train(L['A'], L['B'], K, *(L.get(k) for k in OPS))
    (Mt.movedim(-2, 0) * P['w'].double().reshape((K,) + Mt.shape[:-2] + (3,))).sum().backward()
    # (an operand the result does not depend on -- a rest without relaxation or precession, anything at K = 0 -- has
    # gradient None in autograd; the kernel writes 0)
    out = {'grad_' + k: (torch.zeros_like(x) if x.grad is None else x.grad) for k, x in L.items()}
    out['Mt'] = Mt.detach()
    return out


def _run(P, K, use=OPS, over=None, n=True, leaves=None, loss=None):
    r"""The same through ``fused.ab_train`` on the device; ``over``: tensors that replace operands (operand forms);
    ``n``: whether ``n=K`` is passed (it must be when there is no ``phase``); ``leaves``: the names of the operands that
    require grad (all of them by default; the others' gradients come back ``None``); ``loss``: a callable that is handed
    ``Mt`` and runs the backward pass itself, instead of ``(Mt w).sum()``."""
    wanted = lambda k: leaves is None or k in leaves  # noqa: E731
    L = {k: dev(P[k]).clone().requires_grad_(wanted(k)) for k in ('A', 'B') + tuple(use)}
    for k, x in (over or {}).items():
        L[k] = x.requires_grad_(wanted(k))
    Mt = fused.ab_train(L['A'], L['B'], **({'n': K} if n else {}), **{KW[k]: L[k] for k in use})
    if loss is not None:
        loss(Mt)
    elif Mt.requires_grad:
        (Mt.movedim(-2, 0) * dev(P['w']).reshape((K,) + Mt.shape[:-2] + (3,))).sum().backward()
    out = {'grad_' + k: x.grad for k, x in L.items()}
    out['Mt'] = Mt.detach()
    return out


def _same_bits(a, b, what=''):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# =============================================================================================
# 1. values and all eight gradients
# =============================================================================================
SHAPES = [(1, 1, 1), (2, 100, 2), (2, 100, 7), (2, 200, 40), (1, 300, 3)]


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('N, nM, K', SHAPES, ids=['one', 'K2', 'K7', 'K40', 'blocks2'])
def test_kernels_alone_against_the_fp64_recursion(tag, N, nM, K):
    r"""(1, 1, 1): one row, one repetition -- nothing is fetched ahead, ``Mi`` is the only previous record.  (2, 100, 2)
    and (2, 100, 7): two batch entries, each a ragged block (100 of 256 threads) of its own grid row; K = 2 is the first
    length with a record to read back.  (2, 200, 40): long enough for the prefetch to cycle.  (1, 300, 3): a second,
    ragged block along the spins.  The records and the gradients w.r.t. ``A, B, Mi, phase, rest, T1, T2, Δf``; a second
    run gives the same bits."""
    P, want = _kernel_problem(N, nM, K, tag)
    got = _run(P, K, n=False)
    assert got['Mt'].dtype == DT[tag] and got['Mt'].shape == (N, nM, K, 3) and set(got) == set(want)
    assert got['Mt'].movedim(-2, 0).is_contiguous(), 'time-major storage'
    for k in want:
        print(f'{tag} {(N, nM, K)} {k}: max abs {max_abs(got[k], want[k]):.3e} rel-L2 {rel_l2(got[k], want[k]):.3e}')
        _gate(got[k], want[k], tag, k)
    for k in ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'df'):
        assert got['grad_' + k].shape == P[k].shape and float(got['grad_' + k].abs().max()) > 0, k
    record(f'train.{tag}.N{N}_nM{nM}_K{K}.Mt', max_abs(got['Mt'], want['Mt']) if tag == 'f64' else rel_l2(got['Mt'], want['Mt']))
    _same_bits(got, _run(P, K), 'a second run')


# =============================================================================================
# 2. absent operands
# =============================================================================================
ABSENT = {
    'norest': ('Mi', 'phase'),
    'rest-noT': ('Mi', 'phase', 'rest', 'df'),
    'rest-nodf': ('Mi', 'phase', 'rest', 'T1', 'T2'),
    'nophase': ('Mi', 'rest', 'T1', 'T2', 'df'),
    'noMi': ('phase', 'rest', 'T1', 'T2', 'df'),
}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(ABSENT))
def test_absent_operands(tag, case):
    r"""Each absence against the yardstick with the same absence; the absent operands get no gradient.  ``phase=None``
    is an explicit zero phase and ``Mi=None`` an explicit ``(0, 0, 1)``, bit for bit."""
    N, nM, K = 2, 100, 7
    P, _ = _kernel_problem(N, nM, K, tag)
    use = ABSENT[case]
    want, got = _yardstick(P, K, use), _run(P, K, use)
    assert set(got) == set(want) == {'Mt', 'grad_A', 'grad_B'} | {'grad_' + k for k in use}
    for k in want:
        _gate(got[k], want[k], tag, f'{case}: {k}')
    if case in ('nophase', 'noMi'):
        k = 'phase' if case == 'nophase' else 'Mi'
        explicit = torch.zeros_like(P[k])
        if k == 'Mi':
            explicit[..., 2] = 1
        full = _run(dict(P, **{k: explicit}), K)
        full.pop('grad_' + k)
        _same_bits(got, full, case)


# =============================================================================================
# 3. operand forms
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('form', ['0dim', '11', 'N1', 'NnM', 'expanded'])
def test_operand_forms(tag, form):
    r"""``T1``, ``T2`` in every broadcast form; ``rest`` `()` with ``phase`` `(1, K)` and ``Mi`` `(1, 1, 3)`, then ``rest``
    `(N,)` with ``phase`` `(N, K)` and ``Mi`` full: the result is the fully materialised call's bit for bit; each
    gradient has its operand's own shape and is the materialised call's gradient summed over the broadcast axes."""
    N, nM, K = 2, 100, 7
    P, _ = _kernel_problem(N, nM, K, tag)
    for small in (True, False):
        T1, T1m = _form(P['T1'], form)
        T2, T2m = _form(P['T2'], form)
        rest = P['rest'][0].clone() if small else P['rest'].clone()
        phase = P['phase'][:1].clone() if small else P['phase'].clone()
        Mi = P['Mi'][:1, :1].clone() if small else P['Mi'].clone()
        mat = _run(dict(P, T1=T1m, T2=T2m, rest=rest.expand(N).contiguous(), phase=phase.expand(N, K).contiguous(),
                        Mi=Mi.expand(N, nM, 3).contiguous()), K)
        got = _run(P, K, over=dict(T1=T1, T2=T2, rest=dev(rest), phase=dev(phase), Mi=dev(Mi)))
        what = (form, 'small' if small else 'full')
        for k in ('Mt', 'grad_A', 'grad_B', 'grad_df'):
            assert torch.equal(got[k], mat[k]), (what, k)
        for k, x in (('T1', T1), ('T2', T2), ('rest', rest), ('phase', phase), ('Mi', Mi)):
            g, m = got['grad_' + k], mat['grad_' + k]
            assert g.shape == x.shape and g.dtype == x.dtype, (what, k, g.shape)
            shp = tuple(x.shape) + (1,) * (m.ndim - x.ndim) if x.ndim else (1,) * m.ndim
            _gate(g, m.double().cpu().sum_to_size(shp).reshape(x.shape), tag, f'{what}: grad_{k}')


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_two_spatial_dimensions(tag):
    r"""``Nd = (10, 10)``: ``T1`` `(N, 10, 10)`, ``T2`` `(1, 10, 1)`, ``Mi`` `(N, 10, 10, 3)` -- the bits of the flat
    `(N, 100)` call, gradients in the operands' shapes."""
    K = 7
    P, _ = _kernel_problem(2, 100, K, tag)
    T2row = P['T2'].reshape(2, 10, 10)[:1, :, :1].clone()
    flat = _run(dict(P, T2=T2row.expand(2, 10, 10).reshape(2, 100).contiguous()), K)
    Q = dict(P, A=P['A'].reshape(2, 10, 10, 3, 3), B=P['B'].reshape(2, 10, 10, 3), Mi=P['Mi'].reshape(2, 10, 10, 3),
             T1=P['T1'].reshape(2, 10, 10), T2=T2row, df=P['df'].reshape(2, 10, 10))
    got = _run(Q, K)
    assert got['Mt'].shape == (2, 10, 10, K, 3) and torch.equal(got['Mt'].reshape(2, 100, K, 3), flat['Mt'])
    for k in ('A', 'B', 'Mi', 'T1', 'df'):
        assert got['grad_' + k].shape == Q[k].shape and torch.equal(got['grad_' + k].reshape(flat['grad_' + k].shape),
                                                                    flat['grad_' + k]), k
    assert torch.equal(got['grad_phase'], flat['grad_phase'])
    assert got['grad_T2'].shape == (1, 10, 1) and got['grad_rest'].shape == (2,)
    _gate(got['grad_T2'], flat['grad_T2'].double().cpu().reshape(2, 10, 10).sum_to_size(1, 10, 1), tag, 'grad_T2')
    _gate(got['grad_rest'], flat['grad_rest'], tag, 'grad_rest')          # (summed over the spins in another order)


# =============================================================================================
# 4. known answers on the device
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _identity(tag):
    Q = identity_problem()
    Q['df'] = torch.round(Q['df'] * 1024) / 1024          # on a 2^-10 grid: df and df + 32 are exact in fp32
    return {k: v.to(DT[tag]) for k, v in Q.items()}


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_zero_phase_train_ends_in_the_steady_state(tag):
    r"""Identity (a) of ``test_ab_train_host``: the last of 96 zero-phase records is ``fused.ab_steadystate`` of the same
    ``A, B`` (the yardstick: 8.9e-15 apart in exact arithmetic)."""
    Q = {k: dev(v) for k, v in _identity(tag).items()}
    kw = dict(rest=Q['rest'], T1=Q['T1'], T2=Q['T2'], Δf=Q['df'])
    with torch.no_grad():
        Mt = fused.ab_train(Q['A'], Q['B'], n=96, **kw)
        Mss = fused.ab_steadystate(Q['A'], Q['B'], **kw)
    assert Mt.shape == (2, 100, 96, 3)
    record(f'train.{tag}.last_of_96_vs_ab_steadystate', max_abs(Mt[..., -1, :], Mss) if tag == 'f64' else rel_l2(Mt[..., -1, :], Mss))
    _gate(Mt[..., -1, :].cpu(), Mss, tag, 'the last record vs Mss')
    assert max_abs(Mt[..., 0, :], Mss) > 1e-2


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_linear_phase_is_an_off_resonance_in_the_rest(tag):
    r"""Identity (b): ``φ_k = kψ``, the records rotated back by ``-φ_k`` (in torch, in fp64) are the zero-phase train with
    ``Δf' = Δf + ψ / (2π rest)``.  So that both trains get the SAME problem in fp32 too, ``ψ = 2π rest · 32 Hz`` per batch
    entry from the rest as stored (1.0 and 1.3 rad), ``Δf`` sits on a 2^-10 Hz grid (``Δf + 32`` is exact) and the phases
    are handed over in fp64.  The other sign is O(1) away."""
    Q = _identity(tag)
    K, δ = 24, 32.0
    φ = (2 * π * δ * Q['rest'].double())[:, None] * torch.arange(K, dtype=torch.float64)
    D = {k: dev(v) for k, v in Q.items()}
    kw = dict(rest=D['rest'], T1=D['T1'], T2=D['T2'])
    with torch.no_grad():
        Mt = fused.ab_train(D['A'], D['B'], phase=dev(φ), Δf=D['df'], **kw)
        back = rz(Mt.double(), -dev(φ)[:, None, :])
        plus = fused.ab_train(D['A'], D['B'], n=K, Δf=D['df'] + δ, **kw)
        minus = fused.ab_train(D['A'], D['B'], n=K, Δf=D['df'] - δ, **kw)
    assert torch.equal((D['df'] + δ).double().cpu(), Q['df'].double() + δ)
    record(f'train.{tag}.linear_phase_vs_shifted_df', max_abs(back, plus) if tag == 'f64' else rel_l2(back, plus))
    _gate(back.cpu(), plus, tag, 'rotated back vs the shifted Δf')
    assert max_abs(back, minus) > 0.1


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_record_0_is_one_period_from_Mi(tag):
    r"""K = 1 without a phase: ``A (F Mi + f) + B`` of the yardstick's ``rest_period``."""
    P, _ = _kernel_problem(2, 100, 7, tag)
    with torch.no_grad():
        Mt = fused.ab_train(dev(P['A']), dev(P['B']), n=1, Mi=dev(P['Mi']), rest=dev(P['rest']), T1=dev(P['T1']),
                            T2=dev(P['T2']), Δf=dev(P['df']))
    W = {k: v.double() for k, v in P.items()}
    F, f = rest_period(W['B'], W['rest'], W['T1'], W['T2'], W['df'])
    want = (W['A'] @ ((F @ W['Mi'][..., None]) + f[..., None]))[..., 0] + W['B']
    assert Mt.shape == (2, 100, 1, 3)
    _gate(Mt[..., 0, :].cpu(), want, tag, 'record 0')


# =============================================================================================
# 5. a cotangent on one record only
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('j', [0, 3, 6])
def test_cotangent_on_one_record(tag, j):
    r"""The weights on record ``j`` alone (the first, a middle one, the last of 7): every gradient against the
    yardstick's -- a cotangent sent to the wrong repetition is off by O(1) -- and ``grad_phase[:, k]`` is an exact zero
    for every ``k > j``."""
    N, nM, K = 2, 100, 7
    P, _ = _kernel_problem(N, nM, K, tag)
    w = torch.zeros_like(P['w'])
    w[j] = P['w'][j]
    Pj = dict(P, w=w)
    want, got = _yardstick(Pj, K), _run(Pj, K)
    for k in want:
        _gate(got[k], want[k], tag, f'record {j}: {k}')
    assert float(got['grad_phase'][:, j + 1:].abs().sum()) == 0.0
    assert float(got['grad_phase'][:, j].abs().min()) > 0


# =============================================================================================
# 6. empty problems   7. call counts
# =============================================================================================
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('what', ['K0', 'nM0'])
def test_empty_problem(tag, what):
    r"""No repetition (``phase`` of shape `(N, 0)`) and no spin: correctly shaped empties; the backward runs and the
    gradients are zeros of the operands' shapes."""
    P, _ = _kernel_problem(2, 100, 7, tag)
    if what == 'K0':
        K, E = 0, dict(P, phase=P['phase'][:, :0], w=P['w'][:0])
    else:
        K, E = 7, {k: (v[:, :0] if k in ('A', 'B', 'Mi', 'T1', 'T2', 'df') else v[:, :, :0] if k == 'w' else v)
                   for k, v in P.items()}
    got = _run(E, K, n=False)
    nM = E['A'].shape[1]
    assert got['Mt'].shape == (2, nM, K, 3) and got['Mt'].dtype == DT[tag]
    for k in ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'df'):
        g = got['grad_' + k]
        assert g is not None and g.shape == E[k].shape and g.dtype == DT[tag], k
        assert float(g.abs().sum()) == 0.0, k


def test_one_launch_each_way(monkeypatch):
    calls = _counted(monkeypatch, (FWD, BWD, 'mrphy_ab_steadystate_fwd', 'mrphy_freeprec_fwd'))
    P, _ = _kernel_problem(2, 100, 7, 'f32')
    _run(P, 7)
    assert dict(calls) == {FWD: 1, BWD: 1}
    calls.clear()
    with torch.no_grad():
        fused.ab_train(dev(P['A']), dev(P['B']), n=3)
    assert dict(calls) == {FWD: 1}


# =============================================================================================
# 8. train_rfgr end to end on the fixtures
# =============================================================================================
OUT = ('Mt', 'grad_rf', 'grad_gr', 'grad_T1')


def _fixture_run(Q):
    rf, gr, T1 = (dev(Q[k]).requires_grad_(True) for k in ('rf', 'gr', 'T1'))
    γ = dev(Q['γ'])
    Mt = fused.train_rfgr(rf, gr, dev(Q['loc']), phase=dev(Q['phase']), rest=dev(Q['rest']), T1=T1, T2=dev(Q['T2']),
                          Δf=dev(Q['df']), b1Map=dev(Q['b1']), γ_beff=γ, γ=γ, dt=dev(Q['dt']))
    (Mt.movedim(-2, 0) * dev(Q['w'])).sum().backward()
    return dict(Mt=Mt.detach(), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad)


@pytest.mark.parametrize('tag_mode', MODES)
def test_against_the_reference_fixture(tag_mode):
    r"""fp64: the records (the reference's simulators, 40 repetitions under the 117° and the linear schedule) and
    ``grad_rf``, ``grad_gr``, ``grad_T1`` -- ``T1`` through the pulse and through the rest -- at the project's gate.
    fp32, precise and fast: the distances to the fp64 fixture go to the ledger and are held to 3 x
    ``distance_f32_vs_f64.*``, what the reference's own all-fp32 route loses on the same numbers."""
    tag, mode = _mode(tag_mode)
    G, G64 = golden(f'train_{tag}'), golden('train_f64')
    Q = fixture_inputs(G)
    with mode:
        got = _fixture_run(Q)
    assert set(got) == set(OUT) and got['Mt'].shape == (2, 100, 40, 3)
    if tag == 'f64':
        for k in OUT:
            d = record(f'train.f64.fixture.{k}', max_abs(got[k], G[k]))
            print(f'f64 {k}: {d:.3e} max abs from the reference fixture')
        for k in OUT:
            assert_close(got[k], G[k], 'f64', f'{k} vs the reference fixture')
        return
    wide = oracle_train(Q, torch.float64)
    for k in OUT:
        bound = 3 * float(G[f'distance_f32_vs_f64.{k}'])
        record(f'train.{tag_mode}.fixture.{k}.vs_yardstick64_on_the_same_numbers', rel_l2(got[k], wide[k]))
        record(f'train.{tag_mode}.fixture.{k}.reference_f32_vs_fixture64', rel_l2(G[k], G64[k]))
        d = record(f'train.{tag_mode}.fixture.{k}.vs_fixture64', rel_l2(got[k], G64[k]), bound)
        print(f'{tag_mode} {k}: {d:.3e} from the fp64 fixture, bound {bound:.3e}')
    for k in OUT:
        d, bound = rel_l2(got[k], G64[k]), 3 * float(G[f'distance_f32_vs_f64.{k}'])
        assert d <= bound, f'{k}: {d:.3e} from the fp64 fixture > 3 x the reference\'s own fp32 distance = {bound:.3e}'


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_parallel_transmit_runs_through_the_fused_ab(tag, monkeypatch):
    r"""4 transmit coils with their ``b1Map`` (``test_fused_traj._problem(.., 'ptx4', 48)``), the fixture's rest and
    phases, 8 repetitions: ``A, B`` come from ``mrphy_ab_rfgr_mc_fwd``, and the records are the yardstick's on
    ``beff2ab(rfgr2beff(.))`` of the device."""
    K = 8
    P = _problem(tag, 'ptx4', 48)
    Q = fixture_inputs(golden(f'train_{tag}'))
    rest, phase = dev(Q['rest']), dev(Q['phase'][:, :K].contiguous())
    γ, dt, T1, T2, df = (dev(P[k]) for k in ('γ', 'dt', 'T1', 'T2', 'df'))
    # beff2ab's own four constants, formed once on the device and handed over as `consts=`: A, B are then its bits
    E1, E2 = torch.exp(-dt[:, None] / T1), torch.exp(-dt[:, None] / T2)
    consts = dict(γ2πdt=2 * π * _host.pad_trailing(γ, 2) * _host.pad_trailing(dt, 2), E1=E1, E2=E2, E1_1=E1 - 1)
    calls = _counted(monkeypatch, ('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd', 'mrphy_beff2ab', FWD))
    with torch.no_grad():
        Mt = fused.train_rfgr(dev(P['rf']), dev(P['gr']), dev(P['loc']), phase=phase, rest=rest, T1=T1, T2=T2, Δf=df,
                              b1Map=dev(P['b1']), γ_beff=γ, consts=consts)
        assert dict(calls) == {'mrphy_ab_rfgr_mc_fwd': 1, FWD: 1}
        beff = beffective.rfgr2beff(dev(P['rf']), dev(P['gr']), dev(P['loc']), Δf=df, b1Map=dev(P['b1']), γ=γ)
        A, B = beffective.beff2ab(beff, E1=E1, E2=E2, γ=γ, dt=dt)
        want = torch_train(A.double(), B.double(), K, None, phase.double(), rest.double(), T1.double(), T2.double(),
                           df.double())
    assert Mt.shape == (2, 100, K, 3) and Mt.dtype == DT[tag]
    _gate(Mt.cpu(), want, tag, 'Mt under parallel transmit')


# =============================================================================================
# 9. memory
# =============================================================================================
def test_nothing_per_repetition_is_kept_besides_the_output():
    r"""N = 1, nM = 4096, K = 64 in fp32, ``A``, ``B``, ``T1`` requiring grad, the cotangent allocated beforehand: forward
    + backward raise the allocator's peak by less than twice the bytes of ``Mt`` plus its cotangent -- autograd through
    K repetitions of torch ops would keep a dozen intermediates of a record's size per repetition."""
    N, nM, K = 1, 4096, 64
    gen = torch.Generator().manual_seed(9)
    Qm = torch.linalg.qr(torch.randn((N, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    A, B = dev((0.97 * Qm).float()).requires_grad_(True), dev(torch.randn((N, nM, 3), generator=gen)).requires_grad_(True)
    T1 = dev(0.05 + 0.1 * torch.rand((N, nM), generator=gen)).requires_grad_(True)
    T2, rest = dev(0.02 + 0.05 * torch.rand((N, nM), generator=gen)), dev(torch.tensor(5e-3))
    phase = dev(2 * torch.randn((N, K), generator=gen))
    w = dev(_weights(K, N, nM, torch.float32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Mt = fused.ab_train(A, B, phase=phase, rest=rest, T1=T1, T2=T2)
    Mt.backward(w.movedim(0, -2))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    records = K * N * nM * 3 * 4
    print(f'peak rise {rise} B; Mt {records} B')
    assert A.grad is not None and B.grad is not None and T1.grad is not None and float(T1.grad.abs().max()) > 0
    assert records <= rise < 2 * (records + records), (rise, records)
