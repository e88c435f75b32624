r"""``fused.ab_sequence_jvp`` / ``fused.ab_rfgr_jvp`` / ``fused.sequence_rfgr_jvp`` without a GPU: the yardstick of
``tests/test_sequence_jvp.py`` -- ``torch.autograd.functional.jvp`` of ``test_ab_sequence_host.torch_sequence`` in fp64
(:func:`oracle_sequence_jvp`), with the CPU oracle's bank in front of it (:func:`oracle_bank_jvp`) -- pinned to the
reference's own forward-mode tangents (``tests/golden/sequence_jvp_f64.npz``, ``make_golden_sequence_jvp.py``); the two
entry points ``mrphy_ab_sequence_jvp_*`` exported, declared and bound alike, the capacity query, what the launching one
refuses before any launch and the empty problems it accepts; the argument errors of the Python calls, each raised before
the device or the library is needed."""
import ctypes

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from test_ab_rfgr_host import _declared, fixture_inputs
from test_ab_sequence_host import oracle_bank, torch_sequence
from util import FAKE, assert_close, golden

NAMES = ('mrphy_ab_sequence_jvp_max_dirs', 'mrphy_ab_sequence_jvp_fwd')
GROUPS = ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'df')         # the eight tangent groups, the yardstick's names
EINVAL, EALIGN = -1, -2
BC0 = (None, 0, 0)
BCF = (FAKE, 0, 0)


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def _absent(k, Q, K):
    r"""The value an absent operand stands for, where a tangent of it is asked for."""
    N, spins = Q['B'].shape[1], Q['B'].shape[1:-1]
    if k == 'Mi':
        M = torch.zeros(spins + (3,), dtype=torch.float64)
        M[..., 2] = 1
        return M
    assert k in ('phase', 'df'), f'a tangent of {k} needs the operand'
    return torch.zeros((N, K) if k == 'phase' else spins, dtype=torch.float64)


def oracle_sequence_jvp(Q, K, direction):
    r"""``(Mt, dMt)`` `(N, *Nd, K, 3)` in fp64 on the CPU: ``torch.autograd.functional.jvp`` of ``torch_sequence`` on the
    operands ``Q`` as given, widened (``A, B`` with the bank axis, ``pulse`` a sequence of ints or ``None``, the others by
    the names of ``GROUPS``, ``None`` or missing = absent; ``rest`` `(N ⊻ 1, K)`), along ``direction``: ``{group: a tangent
    that broadcasts to its operand}``, absent groups zero."""
    ops = {k: (None if Q.get(k) is None else Q[k].detach().double()) for k in GROUPS}
    ks = [k for k in GROUPS if direction.get(k) is not None]
    for k in ks:
        if ops[k] is None:
            ops[k] = _absent(k, Q, K)

    def f(*xs):
        o = dict(ops, **dict(zip(ks, xs)))
        return torch_sequence(o['A'], o['B'], K, Q.get('pulse'), *(o[k] for k in GROUPS[2:]))
    if not ks:
        Mt = f()
        return Mt, torch.zeros_like(Mt)
    Mt, dMt = torch.autograd.functional.jvp(
        f, tuple(ops[k] for k in ks), tuple(direction[k].detach().double().expand(ops[k].shape).contiguous() for k in ks))
    return Mt.detach(), dMt.detach()


FIXTURE_GROUPS = ('T1', 'T2', 'Δf', 'b1Map', 'rf', 'rest')
FIXTURE_KEY = {'Δf': 'df', 'b1Map': 'b1'}
NM = 50


def fixture_problem(dtype=torch.float64):
    r"""The inputs of ``sequence_f64.npz``, the first 50 spins, and the fixture's directions, in ``dtype``."""
    P = fixture_inputs(golden('sequence_f64'))
    for k in ('loc', 'df', 'b1', 'T1', 'T2'):
        P[k] = P[k][:, :NM].contiguous()
    G = golden('sequence_jvp_f64')
    V = {g: torch.from_numpy(G[f'dir.{g}']).to(dtype) for g in FIXTURE_GROUPS}
    return {k: (v if k == 'pulse' else v.to(dtype)) for k, v in P.items()}, V, G


def oracle_bank_jvp(P, direction, dtype=torch.float64):
    r"""``(Mt, dMt)`` of the sequence from ``rf`` and ``gr``: ``jvp`` of ``oracle_bank`` -> ``torch_sequence`` on the inputs
    ``P`` of the fixture in ``dtype`` along ``direction`` (by the names of ``FIXTURE_GROUPS``); ``T1``, ``T2`` and ``Δf``
    act in the pulses and in the rests."""
    P = {k: (v if k == 'pulse' else v.to(dtype)) for k, v in P.items()}
    ks = [g for g in FIXTURE_GROUPS if direction.get(g) is not None]
    K = P['phase'].shape[1]

    def f(*xs):
        q = dict(P, **{FIXTURE_KEY.get(g, g): x for g, x in zip(ks, xs)})
        A, B = oracle_bank(q, q['rf'], q['gr'], q['T1'])
        return torch_sequence(A, B, K, P['pulse'].tolist(), None, q['phase'], q['rest'], q['T1'], q['T2'], q['df'])
    Mt, dMt = torch.autograd.functional.jvp(f, tuple(P[FIXTURE_KEY.get(g, g)] for g in ks),
                                            tuple(direction[g].to(dtype) for g in ks))
    return Mt.detach(), dMt.detach()


def test_the_oracles_tangent_is_the_references_per_group():
    P, V, G = fixture_problem()
    assert P['rf'].shape == (3, 2, 2, 48) and P['loc'].shape == (2, NM, 3) and P['phase'].shape == (2, 24)
    assert set(G) == {f'{w}.{g}' for w in ('dir', 'dMt') for g in FIXTURE_GROUPS}, 'arrays of the six groups only'
    want_Mt = golden('sequence_f64')['Mt'][:, :NM]
    for g in FIXTURE_GROUPS:
        assert G[f'dir.{g}'].shape == tuple(P[FIXTURE_KEY.get(g, g)].shape), g
        Mt, dMt = oracle_bank_jvp(P, {g: V[g]})
        assert G[f'dMt.{g}'].shape == (2, NM, 24, 3) == tuple(dMt.shape)
        assert float(torch.from_numpy(G[f'dMt.{g}']).abs().max()) > 0
        assert_close(dMt, G[f'dMt.{g}'], 'f64', f'the yardstick: dMt along {g}')
        assert_close(Mt, want_Mt, 'f64', 'the yardstick: Mt')


def test_the_yardstick_is_linear_in_the_direction_and_zero_on_an_entry_never_played():
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)  # noqa: E731
    K, pulse = 5, [0, 2, 2, 0, 2]
    Q = dict(A=0.9 * torch.linalg.qr(r(3, 2, 4, 3, 3))[0], B=r(3, 2, 4, 3), pulse=pulse, rest=5e-3 + 1e-3 * r(2, K).abs(),
             T1=0.1 + r(2, 4).abs(), T2=0.05 + r(2, 4).abs(), df=50 * r(2, 4))
    v = dict(A=r(3, 2, 4, 3, 3), T1=r(2, 4), phase=r(2, K), Mi=r(2, 4, 3), df=r(2, 4))
    _, one = oracle_sequence_jvp(Q, K, v)
    parts = sum(oracle_sequence_jvp(Q, K, {k: x})[1] for k, x in v.items())
    assert float((one - parts).abs().max()) <= 1e-12 * max(1.0, float(one.abs().max()))
    dA = torch.zeros(3, 2, 4, 3, 3, dtype=torch.float64)
    dA[1] = 1
    assert float(oracle_sequence_jvp(Q, K, dict(A=dA, B=dA[..., 0]))[1].abs().max()) == 0


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # the forward's arguments up to cs_sn; D, the six per-spin tables, the two fp64 tables with their strides; Mt, dMt;
    # the sizes and the stream
    fwd, jvp = list(_lib.PROTOTYPES['mrphy_ab_sequence_fwd'][1]), list(_lib.PROTOTYPES[NAMES[1]][1])
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert jvp == fwd[:21] + [i64] + [vp] * 6 + [vp, i64] * 2 + [vp, vp] + fwd[-4:]
    assert {f'tu_ab_sequence_jvp{m}.hip' for m in (1, 2, 4)} <= {u for u, _ in _lib.UNITS}     # one unit per capacity
    assert mrphy_amd.require_library().mrphy_abi_version() == _lib.ABI_VERSION == 5     # additive: the version stays


def test_capacity_query():
    lib = mrphy_amd.require_library()
    for code in (0, 1):
        assert lib.mrphy_ab_sequence_jvp_max_dirs(code) == 4, code
    for code in (-1, 2, 3, 4, 5, 17):               # data types only, as mrphy_ab_sequence_*
        assert lib.mrphy_ab_sequence_jvp_max_dirs(code) < 0, code


TABLES = ('dA', 'dB', 'dMi', 'dT1', 'dT2', 'ddf')


def _call(lib):
    r"""The entry point with fake pointers (never dereferenced: no call here is valid on a problem that is not empty)."""
    def jvp(A=FAKE, B=FAKE, P=3, pulse=FAKE, rs=FAKE, T1=BCF, T2=BCF, df=BCF, Mi=BCF, cs=FAKE, D=1, dphase=None,
            drest=None, Mt=FAKE, dMt=FAKE, N=2, nM=100, K=5, dtype=0, **tables):
        assert set(tables) <= set(TABLES)
        return lib.mrphy_ab_sequence_jvp_fwd(dtype, A, B, P, pulse, rs, 0, *T1, *T2, *df, *Mi, cs, 0, D,
                                             *(tables.get(k) for k in TABLES), dphase, 0, drest, 0, Mt, dMt, N, nM, K, None)
    return jvp


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    jvp = _call(lib)
    # 1. the forward's checks, in its order
    for dtype in (-1, 2, 3, 4, 5, 17):
        assert jvp(dtype=dtype) == EINVAL, ('dtype', dtype)
    assert jvp(N=-1) == EINVAL and jvp(nM=-1) == EINVAL and jvp(K=-1) == EINVAL and jvp(N=65536) == EINVAL
    assert jvp(P=0) == EINVAL and jvp(P=-2) == EINVAL and jvp(pulse=None) == EINVAL
    assert jvp(A=None) == EINVAL and jvp(B=None) == EINVAL
    assert jvp(rs=None) == EINVAL, 'T1, T2, df without a rest'
    assert jvp(T2=BC0) == EINVAL and jvp(T1=BC0) == EINVAL, 'T1 and T2: both or neither'
    # 2. the direction count against the capacity
    for dtype in (0, 1):
        cap = lib.mrphy_ab_sequence_jvp_max_dirs(dtype)
        for D in (0, -1, cap + 1, 64):
            assert jvp(D=D, dtype=dtype) == EINVAL, ('directions', D, dtype)
    # 3. a tangent whose operand the call does not have
    norelax = dict(T1=BC0, T2=BC0)
    assert jvp(dT1=FAKE, **norelax) == EINVAL and jvp(dT2=FAKE, **norelax) == EINVAL, 'dT1 / dT2 without T1'
    norest = dict(rs=None, T1=BC0, T2=BC0, df=BC0)
    for k in ('dT1', 'dT2', 'ddf'):
        assert jvp(**{k: FAKE}, **norest) == EINVAL, (k, 'without a rest table')
    assert jvp(drest=FAKE, **norest) == EINVAL, 'drest without a rest table'
    # 4. dMt is required (Mt is not: that call would be a launch, not made here)
    assert jvp(dMt=None) == EINVAL and jvp(dMt=None, Mt=None) == EINVAL
    # 5. alignment: the per-spin tables and the outputs in the data type, the two uniform tables fp64
    for dtype, odd in ((0, FAKE + 2), (1, FAKE + 4)):
        for k in TABLES:
            assert jvp(dtype=dtype, **{k: odd}) == EALIGN, (dtype, k)
        assert jvp(dtype=dtype, Mt=odd) == EALIGN and jvp(dtype=dtype, dMt=odd) == EALIGN
        assert jvp(dtype=dtype, A=odd) == EALIGN and jvp(dtype=dtype, rs=FAKE + 4) == EALIGN
        assert jvp(dtype=dtype, dphase=FAKE + 4) == EALIGN and jvp(dtype=dtype, drest=FAKE + 4) == EALIGN
    # a null pointer is reported before a misaligned one
    assert jvp(dMt=None, dA=FAKE + 2) == EINVAL and jvp(pulse=None, dMt=FAKE + 2) == EINVAL


def test_empty_problems_are_a_success_whatever_the_pointers_are():
    jvp = _call(mrphy_amd.require_library())
    null = dict(A=None, B=None, pulse=None, rs=None, T1=BCF, T2=BC0, df=BCF, Mi=BC0, cs=None, Mt=None, dMt=None)
    for size in (dict(nM=0), dict(N=0), dict(K=0), dict(N=0, nM=0, K=0)):
        assert jvp(**null, **size) == 0, size
        assert jvp(**null, **size, dT1=FAKE, drest=FAKE, D=9) == 0, size
    assert jvp(K=0, dtype=7) == EINVAL and jvp(N=0, nM=-1) == EINVAL and jvp(K=0, P=0) == EINVAL


# ---------------------------------------------------------------------------------------------
# argument errors of the Python calls
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    r"""The checks below must be made before the library is asked for."""
    def refuse():
        raise AssertionError('the library was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_library', refuse)


def _bank(P=3, N=2, nM=5, K=4):
    A = (torch.eye(3).expand(P, N, nM, 3, 3) * 0.9).contiguous()
    return dict(A=A, B=torch.zeros(P, N, nM, 3), pulse=[0, 1, 2, 1][:K], rest=torch.full((N, K), 5e-3),
                T1=torch.ones(N, nM), T2=torch.ones(N, nM), Δf=torch.zeros(N, nM))


@pytest.mark.usefixtures('no_library')
def test_directions_must_agree_and_keys_must_be_known():
    a = _bank()
    with pytest.raises(ValueError, match='Mi'):
        fused.ab_sequence_jvp(**a, tangents=dict(A=torch.zeros(2, 3, 2, 5, 3, 3), Mi=torch.zeros(3, 2, 5, 3)))
    with pytest.raises(ValueError, match='pulse'):
        fused.ab_sequence_jvp(**a, tangents=dict(pulse=torch.zeros(1, 4)))
    with pytest.raises(ValueError, match='df'):                    # the keyword's name is Δf
        fused.ab_sequence_jvp(**a, tangents=dict(df=torch.zeros(1, 2, 5)))
    for empty in ({}, dict(A=None, T1=None)):
        with pytest.raises(ValueError, match='no direction'):
            fused.ab_sequence_jvp(**a, tangents=empty)
    with pytest.raises(ValueError, match='tangents'):
        fused.ab_sequence_jvp(**a, tangents=None)
    with pytest.raises(ValueError, match='leading direction axis'):
        fused.ab_sequence_jvp(**a, tangents=dict(T1=torch.tensor(1.0)))
    with pytest.raises(ValueError, match='directions'):
        fused.ab_sequence_jvp(**a, tangents=dict(T1=torch.zeros(0, 2, 5)))


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('key, shape', [
    ('A', (1, 3, 2, 5, 3)), ('A', (1, 2, 2, 5, 3, 3)), ('A', (1, 3, 2, 4, 3, 3)), ('B', (1, 3, 2, 5, 2)), ('B', (3, 2, 5, 3)),
    ('Mi', (1, 2, 5, 2)), ('Mi', (1, 3, 5, 3)), ('phase', (1, 2, 3)), ('phase', (1, 3, 4)), ('phase', (1, 4)),
    ('rest', (1, 2, 3)), ('rest', (1, 3)), ('rest', (1, 2, 4, 1)), ('T1', (1, 2, 6)), ('T2', (1, 2, 5, 3)), ('Δf', (1, 3, 5))])
def test_a_tangent_that_does_not_broadcast_to_its_operand_is_refused(key, shape):
    with pytest.raises(ValueError, match=f"'{key}'.*does not broadcast"):
        fused.ab_sequence_jvp(**_bank(), tangents={key: torch.zeros(shape)})


@pytest.mark.usefixtures('no_library')
def test_tangents_of_operands_the_call_does_not_have_are_refused():
    a = _bank()
    norelax = {k: v for k, v in a.items() if k not in ('T1', 'T2')}
    for k in ('T1', 'T2'):
        with pytest.raises(ValueError, match=f"'{k}'.*without"):
            fused.ab_sequence_jvp(**norelax, tangents={k: torch.zeros(1, 2, 5)})
    norest = dict(A=a['A'], B=a['B'], pulse=a['pulse'])
    for k, shape in (('rest', (1, 2, 4)), ('Δf', (1, 2, 5))):
        with pytest.raises(ValueError, match=f"'{k}'.*without"):
            fused.ab_sequence_jvp(**norest, tangents={k: torch.zeros(shape)})
    # Mi and phase may come without their operand, Δf while a rest is given: these pass the checks and go on to ask for
    # device tensors
    noΔf = {k: v for k, v in a.items() if k != 'Δf'}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_sequence_jvp(**noΔf, tangents=dict(Mi=torch.zeros(1, 2, 5, 3), phase=torch.zeros(1, 1, 4),
                                                     Δf=torch.zeros(1, 1, 1)))


@pytest.mark.usefixtures('no_library')
def test_operand_checks_come_first_the_schedule_before_anything():
    a = _bank()
    a['pulse'] = [0, 1, 3, 1]
    with pytest.raises(ValueError, match='repetition 2'):
        fused.ab_sequence_jvp(**a, tangents=dict(bogus=torch.zeros(1)))
    a['pulse'] = [0, 1, 2]
    with pytest.raises(ValueError, match='`rest`'):
        fused.ab_sequence_jvp(**a, tangents=dict(bogus=torch.zeros(1)))
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match='repetition 2'):
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=[0, 1, 3], tangents=dict(bogus=torch.zeros(1)))


@pytest.mark.usefixtures('no_library')
def test_cpu_tensors_are_refused_as_the_other_fused_calls_refuse_them():
    a = _bank()
    with pytest.raises(RuntimeError, match='no CPU fallback') as plain:
        fused.ab_sequence(**a)
    with pytest.raises(RuntimeError, match='no CPU fallback') as jvp:
        fused.ab_sequence_jvp(**a, tangents=dict(T1=torch.ones(1, 1, 1), rest=torch.zeros(1)))
    assert str(jvp.value) == str(plain.value)
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    kw = dict(T1=a['T1'], T2=a['T2'])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.ab_rfgr_jvp(rf[0], gr[0], loc, tangents=dict(rf=torch.zeros(1, 2, 2, 16)), **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=a['pulse'], rest=a['rest'], tangents=dict(T1=torch.ones(1, 1, 1)), **kw)
    assert {'ab_sequence_jvp', 'ab_rfgr_jvp', 'sequence_rfgr_jvp'} <= set(fused.__all__)


@pytest.mark.usefixtures('no_library')
def test_rfgr_wrappers_check_their_keys_and_refuse_parallel_transmit():
    rf, gr, loc = torch.zeros(3, 2, 2, 16), torch.zeros(1, 2, 3, 16), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match='Mi'):
        fused.ab_rfgr_jvp(rf[0], gr[0], loc, tangents=dict(Mi=torch.zeros(1, 2, 5, 3)))
    with pytest.raises(ValueError, match='Δf_rest'):               # the key exists only beside the operand
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=[0, 1], tangents={'Δf_rest': torch.zeros(1, 2, 5)})
    with pytest.raises(ValueError, match='A'):                     # the bank is formed inside
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=[0, 1], tangents=dict(A=torch.zeros(1, 3, 2, 5, 3, 3)))
    with pytest.raises(ValueError, match="'rf'.*does not broadcast"):
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=[0, 1], tangents=dict(rf=torch.zeros(1, 2, 2, 16)))
    with pytest.raises(ValueError, match='directions'):
        fused.sequence_rfgr_jvp(rf, gr, loc, pulse=[0, 1], tangents=dict(rf=torch.zeros(2, 3, 2, 2, 16), Mi=torch.zeros(1, 2, 5, 3)))
    mc, b1 = torch.zeros(2, 2, 16, 4), torch.zeros(2, 5, 2, 4)
    with pytest.raises(NotImplementedError, match='parallel transmit'):
        fused.ab_rfgr_jvp(mc, gr[0], loc, b1Map=b1, tangents=dict(rf=torch.zeros(1, 2, 2, 16, 4)))
    with pytest.raises(NotImplementedError, match='parallel transmit'):
        fused.sequence_rfgr_jvp(mc.expand(3, 2, 2, 16, 4), gr, loc, pulse=[0, 1], b1Map=b1,
                                tangents=dict(Mi=torch.zeros(1, 2, 5, 3)))
