r"""``fused.blochsim_rfgr_jvp`` / ``fused.sensitivity_rfgr`` without a GPU: the CPU oracle's forward-mode tangent -- the
yardstick of ``tests/test_jvp.py`` -- pinned to the reference's own (``tests/golden/jvp_f64.npz``); the two entry points
``mrphy_blochsim_rfgr_jvp_*`` exported, declared and bound alike, the capacity query, and what the launching one refuses
before any launch, in the order of its checks; the argument errors of the Python call, each raised before the device or
the library is needed; the direction builder of ``sensitivity_rfgr``."""
import ctypes

import pytest
import torch

import bloch_oracle as O
import mrphy_amd
from mrphy_amd import _lib, fused
from test_moving_host import _declared
from util import FAKE, fused_ops, golden, rel_l2, t

NAMES = ('mrphy_blochsim_rfgr_jvp_max_dirs', 'mrphy_blochsim_rfgr_jvp_fwd')
GROUPS = ('Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'T1', 'T2')
EINVAL = -1
CODES = (0, 1, 2, 3, 4)     # MRPHY_F32, _F64, _F32_C64, _F32P, _F32P_C64


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def oracle_jvp(P, direction):
    r"""``(Mo, dMo)`` of the CPU oracle in fp64: ``torch.autograd.functional.jvp`` over ``O.rfgr2beff`` +
    ``O.blochsim_slow`` on the operands ``P`` (by the names of ``GROUPS``, plus ``γ``, ``dt``; fp32 operands widened),
    along ``direction``: ``{group: a tangent of its operand's shape}``, absent groups zero."""
    P = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in P.items()}
    ks = [k for k in GROUPS if direction.get(k) is not None]

    def f(*xs):
        q = dict(P, **dict(zip(ks, xs)))
        be = O.rfgr2beff(q['rf'], q['gr'], q['loc'], Δf=q['Δf'], b1Map=q['b1Map'], γ=q['γ'])
        return O.blochsim_slow(q['Mi'].clone(), be, T1=q['T1'], T2=q['T2'], γ=q['γ'], dt=q['dt'])
    Mo, dMo = torch.autograd.functional.jvp(f, tuple(P[k] for k in ks),
                                            tuple(direction[k].double().expand(P[k].shape).contiguous() for k in ks))
    return Mo.detach(), dMo.detach()


def test_the_oracles_tangent_is_the_references_per_group():
    r"""Relative L2 <= 1e-12 per group, and ``Mo`` likewise: the GPU tests' yardstick is the reference's derivative."""
    G = golden('jvp_f64')
    P = {k[3:]: t(v) for k, v in G.items() if k.startswith('in.')}
    for k in GROUPS:
        Mo, dMo = oracle_jvp(P, {k: t(G[f'dir.{k}'])})
        d = rel_l2(dMo, t(G[f'dMo.{k}']))
        assert d <= 1e-12, (k, d)
        assert float(dMo.norm()) > 0
    assert rel_l2(Mo, t(G['Mo'])) <= 1e-12


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
    # the static forward's dtype, Mi and operands; D and the nine tangent tables; Mo, dMo; the sizes and the stream
    st, args = list(_lib.PROTOTYPES['mrphy_blochsim_rfgr_fwd'][1]), list(_lib.PROTOTYPES[NAMES[1]][1])
    assert args == st[:24] + [ctypes.c_int64] + [ctypes.c_void_p] * 9 + [ctypes.c_void_p] * 2 + st[-5:]
    assert {f'tu_fused_jvp{m}_fwd.hip' for m in (1, 2, 4)} <= {u for u, _ in _lib.UNITS}     # one unit per capacity
    for m in (1, 2, 4):
        assert {mask for u, mask in _lib.UNITS if u == f'tu_fused_jvp{m}_fwd.hip'} >= {1 << c for c in CODES[:2]}
    assert mrphy_amd.require_library().mrphy_abi_version() == _lib.ABI_VERSION == 5     # additive: the version stays


def test_capacity_query():
    lib = mrphy_amd.require_library()
    for code in CODES:
        assert lib.mrphy_blochsim_rfgr_jvp_max_dirs(code) in (2, 4), code
    for code in (-1, 5, 17):
        assert lib.mrphy_blochsim_rfgr_jvp_max_dirs(code) < 0, code


TABLES = ('dMi', 'drf', 'dgr', 'dloc', 'ddf', 'db1', 'dE1', 'dE2', 'dE1m1')


def _call(lib):
    r"""The entry point with fake pointers (never dereferenced: no call here is valid on a problem that is not empty)."""
    def fwd(ops, D=1, Mi=FAKE, Mo=FAKE, dMo=FAKE, N=1, nM=64, nT=16, nC=1, dtype=0, **tables):
        assert set(tables) <= set(TABLES)
        return lib.mrphy_blochsim_rfgr_jvp_fwd(dtype, Mi, *ops, D, *(tables.get(k) for k in TABLES), Mo, dMo, N, nM, nT,
                                               nC, None)
    return fwd


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd = _call(lib)
    ok = fused_ops()
    relax = fused_ops(E1=FAKE, E2=FAKE, E1m1=FAKE)
    # 1. dtype and sizes
    for dtype in (-1, 5, 17):
        assert fwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
    assert fwd(ok, N=-1) == EINVAL and fwd(ok, nM=-64) == EINVAL and fwd(ok, nT=-16) == EINVAL, 'a negative size'
    # 2. the mode arguments, on an empty problem too
    for dtype in CODES:
        cap = lib.mrphy_blochsim_rfgr_jvp_max_dirs(dtype)
        for D in (0, -1, cap + 1, 64):
            for nM in (64, 0):
                assert fwd(ok, D=D, nM=nM, dtype=dtype) == EINVAL, ('directions', D, nM, dtype)
    assert fwd(ok, nC=2) == EINVAL and fwd(ok, nC=0) == EINVAL and fwd(ok, nM=0, nC=2) == EINVAL, 'one transmit coil'
    assert fwd(ok, db1=FAKE) == EINVAL and fwd(ok, db1=FAKE, nM=0) == EINVAL, 'db1 without b1'
    assert fwd(ok, ddf=FAKE) == EINVAL, 'ddf without gamma'
    for k in ('dE1', 'dE2', 'dE1m1'):
        assert fwd(ok, **{k: FAKE}) == EINVAL and fwd(ok, nM=0, **{k: FAKE}) == EINVAL, (k, 'without relaxation')
    # 3. empty problems: a success that launches nothing (the call runs at nT == 0, so it needs its pointers there)
    assert fwd(ok, nM=0, Mi=None, Mo=None, dMo=None) == 0 and fwd(ok, N=0) == 0
    assert fwd(relax, nM=0, dE1=FAKE, dE2=FAKE, dE1m1=FAKE) == 0
    assert fwd(fused_ops(b1=FAKE), nM=0, db1=FAKE) == 0 and fwd(fused_ops(df=FAKE, gamma=FAKE), nM=0, ddf=FAKE) == 0
    assert fwd(ok, nT=0, dMo=None) == EINVAL
    # 4. null pointers
    assert fwd(ok, Mi=None) == EINVAL and fwd(ok, dMo=None) == EINVAL, 'a null Mi / dMo'
    for what in (dict(loc=None), dict(g=None), dict(rf=None), dict(gr=None), dict(df=FAKE), dict(E1=FAKE, E1m1=FAKE)):
        assert fwd(fused_ops(**what)) == EINVAL, what
    # (more batch entries than a grid holds: refused by the launcher, before it launches)
    for D in (1, 2, 3, 4):
        if D <= lib.mrphy_blochsim_rfgr_jvp_max_dirs(0):
            assert fwd(ok, D=D, N=65536) == EINVAL, 'N > 65535'


# ---------------------------------------------------------------------------------------------
# argument errors of the Python call
# ---------------------------------------------------------------------------------------------
def _operands(dtype=torch.float32, N=2, Nd=(5,), nT=16, b1=True, relax=True):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(s, generator=g, dtype=dtype)  # noqa: E731
    a = dict(Mi=r(N, *Nd, 3), rf=r(N, 2, nT), gr=r(N, 3, nT), loc=r(N, *Nd, 3), Δf=r(N, *Nd), b1Map=r(N, *Nd, 2) if b1 else None)
    if relax:
        a.update(T1=1 + r(N, *Nd), T2=0.1 + r(N, *Nd))
    return a


@pytest.fixture
def no_library(monkeypatch):
    r"""The checks below must be made before the library is asked for."""
    def refuse():
        raise AssertionError('the library was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_library', refuse)


@pytest.mark.usefixtures('no_library')
def test_directions_must_agree_and_keys_must_be_known():
    a = _operands()
    with pytest.raises((ValueError, AssertionError), match='rf'):
        fused.blochsim_rfgr_jvp(**a, tangents=dict(Mi=torch.zeros(2, 2, 5, 3), rf=torch.zeros(3, 2, 2, 16)))
    with pytest.raises((ValueError, AssertionError), match='γ'):
        fused.blochsim_rfgr_jvp(**a, tangents=dict(γ=torch.zeros(1)))
    with pytest.raises((ValueError, AssertionError), match='E1'):      # the constants' keys belong to consts=
        fused.blochsim_rfgr_jvp(**a, tangents=dict(E1=torch.zeros(1, 2, 5)))
    with pytest.raises((ValueError, AssertionError), match='tangents'):
        fused.blochsim_rfgr_jvp(**a, tangents={})
    with pytest.raises((ValueError, AssertionError), match='tangents'):
        fused.blochsim_rfgr_jvp(**a, tangents=None)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('key, shape', [
    ('Mi', (1, 2, 5, 2)), ('Mi', (1, 2, 4, 3)), ('Mi', (1, 3, 5, 3)), ('Mi', (2, 5, 3)), ('rf', (1, 2, 2, 15)),
    ('rf', (1, 2, 3, 16)), ('gr', (1, 2, 2, 16)), ('loc', (1, 2, 5)), ('Δf', (1, 2, 4)), ('Δf', (1, 3, 5)), ('b1Map', (1, 2, 5, 3)),
    ('T1', (1, 2, 6)), ('T2', (1, 2, 5, 3))])
def test_a_tangent_that_does_not_broadcast_to_its_operand_is_refused(key, shape):
    with pytest.raises((ValueError, AssertionError), match=key):
        fused.blochsim_rfgr_jvp(**_operands(), tangents={key: torch.zeros(shape)})


@pytest.mark.usefixtures('no_library')
def test_tangents_of_operands_the_call_does_not_have_are_refused():
    with pytest.raises((ValueError, AssertionError), match='b1Map'):
        fused.blochsim_rfgr_jvp(**_operands(b1=False), tangents=dict(b1Map=torch.zeros(1, 2, 5, 2)))
    for k in ('T1', 'T2'):
        with pytest.raises((ValueError, AssertionError), match=k):
            fused.blochsim_rfgr_jvp(**_operands(relax=False), tangents={k: torch.zeros(1, 2, 5)})
    a = _operands(relax=False)
    consts = dict(γ2πdt=torch.tensor(0.1), E1=torch.full((2, 5), 0.99), E2=torch.full((2, 5), 0.9), E1_1=torch.full((2, 5), -0.01))
    with pytest.raises((ValueError, AssertionError), match='T1'):
        fused.blochsim_rfgr_jvp(**a, consts=consts, tangents=dict(T1=torch.zeros(1, 2, 5)))
    with pytest.raises((ValueError, AssertionError), match='E2'):      # consts= without relaxation
        fused.blochsim_rfgr_jvp(**a, consts=dict(γ2πdt=torch.tensor(0.1)), tangents=dict(E2=torch.zeros(1, 2, 5)))


@pytest.mark.usefixtures('no_library')
def test_parallel_transmit_is_not_implemented():
    a = _operands()
    a['rf'] = torch.zeros(2, 2, 16, 4)
    a['b1Map'] = torch.zeros(2, 5, 2, 4)
    with pytest.raises(NotImplementedError, match='parallel transmit'):
        fused.blochsim_rfgr_jvp(**a, tangents=dict(Mi=torch.zeros(1, 2, 5, 3)))


@pytest.mark.usefixtures('no_library')
def test_cpu_tensors_are_refused_as_the_other_fused_calls_refuse_them():
    a = _operands()
    with pytest.raises(RuntimeError, match='no CPU fallback') as static:
        fused.blochsim_rfgr(*(a[k] for k in ('Mi', 'rf', 'gr', 'loc')))
    with pytest.raises(RuntimeError, match='no CPU fallback') as jvp:
        fused.blochsim_rfgr_jvp(**a, tangents=dict(Mi=torch.zeros(1, 2, 5, 3), T1=torch.zeros(1, 1, 1)))
    assert str(jvp.value) == str(static.value)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.sensitivity_rfgr(**a)


# ---------------------------------------------------------------------------------------------
# the direction builder of sensitivity_rfgr
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrt', [('Δf', 'rf', 'T1', 'T2'), ('rf',), ('T2', 'Δf')])
def test_sensitivity_directions(wrt):
    rf = torch.rand(2, 2, 16, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    d = fused._sensitivity_directions(wrt, rf, 2)
    assert tuple(d) == tuple(wrt)
    D = len(wrt)
    for i, k in enumerate(wrt):
        assert d[k].dtype == rf.dtype
        if k == 'rf':
            assert d[k].shape == (D, 2, 2, 16) and torch.equal(d[k][i], rf)
        else:
            assert d[k].shape == (D, 1, 1) and float(d[k][i]) == 1.0
        others = torch.cat([d[k][:i], d[k][i + 1:]])
        assert float(others.abs().sum()) == 0, 'every table is zero in the other entries\' directions'
    assert fused.sensitivity_rfgr.__kwdefaults__['wrt'] == ('Δf', 'rf', 'T1', 'T2')


def test_sensitivity_directions_refuse_unknown_entries():
    rf = torch.zeros(1, 2, 8)
    for wrt in (('gr',), ('Δf', 'γ'), (), ('rf', 'rf')):
        with pytest.raises(ValueError, match='wrt'):
            fused._sensitivity_directions(wrt, rf, 2)
