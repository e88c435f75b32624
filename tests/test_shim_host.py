r"""``fused.blochsim_rfgr_shim`` without a GPU: the routing decision ``fused._decide_ext_route`` over its truth table; the
argument errors, each raised before the device or the library is needed; the composed route's channel-field helper; the
four entry points ``mrphy_blochsim_rfgr_shim_*`` exported, declared and bound alike, the capacity and workspace queries,
and what the two launching entry points refuse before any launch, in the order of their checks."""
import ctypes
import itertools

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from mrphy_amd.fused import _decide_ext_route, _shim_bz
from test_moving_host import _declared
from util import FAKE, fused_ops

NAMES = ('mrphy_blochsim_rfgr_shim_max_channels', 'mrphy_blochsim_rfgr_shim_bwd_workspace',
         'mrphy_blochsim_rfgr_shim_fwd', 'mrphy_blochsim_rfgr_shim_bwd')
EINVAL, ENOSPC = -1, -3
SEG = 16                    # mrphy_blochsim_rfgr_ck_every()
CODES = (0, 1, 2, 3, 4)     # MRPHY_F32, _F64, _F32_C64, _F32P, _F32P_C64


# ---------------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nT', [0, 1, 15, 16, 17, 40, 48, 1024, 1030])
def test_route_truth_table(nT):
    r"""Fused: one coil, ``nS`` within the capacity and no gradient at any length, or gradients among ``Mi, rf, gr, sh`` over
    whole segments; split: such gradients, more than a segment and a ragged tail, at the last segment boundary; composed:
    everything else -- parallel transmit, more channels than the capacity, a gradient the kernels do not form, fewer than
    16 steps with a gradient."""
    for one_coil, pulse_grad, other_grad in itertools.product((True, False), repeat=3):
        for nS, cap in ((1, 8), (3, 8), (8, 8), (9, 8), (5, 4), (4, 4), (17, 8)):
            got = _decide_ext_route(nT=nT, seg=SEG, one_coil=one_coil, fits=nS <= cap, pulse_grad=pulse_grad,
                                    other_grad=other_grad)
            if not one_coil or other_grad or nS > cap:
                want = ('composed', None)
            elif not pulse_grad:
                want = ('fused', False)
            elif nT % SEG == 0:
                want = ('fused', True)
            elif nT > SEG:
                want = ('split', nT // SEG * SEG)
            else:
                want = ('composed', None)
            assert got == want, (nT, one_coil, nS, cap, pulse_grad, other_grad)
    kw = dict(seg=SEG, one_coil=True, fits=3 <= 8, other_grad=False)
    assert _decide_ext_route(nT=40, pulse_grad=True, **kw) == ('split', 32)
    assert _decide_ext_route(nT=8, pulse_grad=True, **kw) == ('composed', None)
    assert _decide_ext_route(nT=8, pulse_grad=False, **kw) == ('fused', False)
    assert _decide_ext_route(nT=48, pulse_grad=True, **dict(kw, fits=9 <= 8)) == ('composed', None)


# ---------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------
def _operands(dtype=torch.float32, N=2, Nd=(5,), nT=16, nS=3):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(s, generator=g, dtype=dtype)  # noqa: E731
    return dict(Mi=r(N, *Nd, 3), rf=r(N, 2, nT), gr=r(N, 3, nT), loc=r(N, *Nd, 3), sh=r(N, nS, nT), shMap=r(N, *Nd, nS))


@pytest.fixture
def no_library(monkeypatch):
    r"""The checks below must be made before the library is asked for."""
    def refuse():
        raise AssertionError('the library was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_library', refuse)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('shape', [(3, 16), (2, 3, 16, 1), (3, 3, 16), (16,)])
def test_sh_of_the_wrong_rank_or_batch_is_refused(shape):
    a = _operands()
    a['sh'] = torch.zeros(shape)
    with pytest.raises(ValueError, match='sh'):
        fused.blochsim_rfgr_shim(**a)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('shape', [(2, 5), (2, 1, 5, 3), (3, 5, 3), (2, 4, 3), (5, 3)])
def test_shmap_of_the_wrong_rank_batch_or_spins_is_refused(shape):
    a = _operands()
    a['shMap'] = torch.zeros(shape)
    with pytest.raises(ValueError, match='shMap'):
        fused.blochsim_rfgr_shim(**a)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('which', ['sh', 'shMap'])
def test_sh_and_shmap_must_be_tensors(which):
    a = _operands()
    a[which] = None
    with pytest.raises(ValueError, match=which):
        fused.blochsim_rfgr_shim(**a)


@pytest.mark.usefixtures('no_library')
def test_channel_counts_and_pulse_lengths_must_agree():
    a = _operands()
    with pytest.raises(ValueError, match='channels'):
        fused.blochsim_rfgr_shim(**dict(a, sh=torch.zeros(2, 4, 16)))
    with pytest.raises(ValueError, match='channels'):
        fused.blochsim_rfgr_shim(**dict(a, shMap=torch.zeros(2, 5, 2)))
    with pytest.raises(ValueError, match='steps'):
        fused.blochsim_rfgr_shim(**dict(a, sh=torch.zeros(2, 3, 15)))
    with pytest.raises(ValueError, match='steps'):                    # half tensors take the same checks
        fused.blochsim_rfgr_shim(**{k: x.half() for k, x in dict(a, sh=torch.zeros(2, 3, 17)).items()})


@pytest.mark.usefixtures('no_library')
def test_cpu_tensors_are_refused_as_the_other_fused_calls_refuse_them():
    r"""With channels, with a shared waveform set and a shared map, and with none (``blochsim_rfgr``'s own refusal)."""
    a = _operands()
    with pytest.raises(RuntimeError, match='no CPU fallback') as static:
        fused.blochsim_rfgr(*(a[k] for k in ('Mi', 'rf', 'gr', 'loc')))
    for b in (a, dict(a, sh=a['sh'][:1], shMap=a['shMap'][:1]), _operands(nS=0), _operands(nS=9)):
        with pytest.raises(RuntimeError, match='no CPU fallback') as shim:
            fused.blochsim_rfgr_shim(**b)
        assert str(shim.value) == str(static.value)


# ---------------------------------------------------------------------------------------------
# the composed route's helper
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Nd', [(9,), (3, 2, 2)])
def test_shim_z_is_the_sum_over_channels(Nd):
    g = torch.Generator().manual_seed(5)
    N, nT, nS = 2, 24, 5
    m = torch.rand(N, *Nd, nS, generator=g, dtype=torch.float64) * 4 - 2
    for Np in (N, 1):
        sh = torch.rand(Np, nS, nT, generator=g, dtype=torch.float64) * 2 - 1
        for mm in (m, m[:1]):
            z = _shim_bz(sh, mm)
            assert z.shape == (max(Np, mm.shape[0]), *Nd, nT)
            want = sum(mm[..., k, None] * sh[:, k].reshape((Np,) + (1,) * len(Nd) + (nT,)) for k in range(nS))
            assert float((z - want).abs().max()) <= 1e-13 * float(want.abs().max())
    s, mg = sh.clone().requires_grad_(True), m.clone().requires_grad_(True)    # differentiable w.r.t. both
    _shim_bz(s, mg).sum().backward()
    assert float(s.grad.abs().max()) > 0 and float(mg.grad.abs().max()) > 0


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
    # the static counterparts' arguments plus (sh, sh_sn, shMap, nS), which follow the operands
    extra = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    for name, static in zip(NAMES[2:], ('mrphy_blochsim_rfgr_fwd', 'mrphy_blochsim_rfgr_bwd')):
        st, args = list(_lib.PROTOTYPES[static][1]), list(_lib.PROTOTYPES[name][1])
        assert args == st[:24] + extra + st[24:], name
    units = {u for u, _ in _lib.UNITS}
    assert {f'tu_fused_shim{m}_{d}.hip' for m in (2, 4, 8) for d in ('fwd', 'bwd')} <= units     # one unit per capacity
    assert mrphy_amd.require_library().mrphy_abi_version() == _lib.ABI_VERSION == 5     # additive: the version stays


def test_capacity_query():
    lib = mrphy_amd.require_library()
    for code in CODES:
        assert lib.mrphy_blochsim_rfgr_shim_max_channels(code) >= 2, code
    for code in (-1, 5, 17):
        assert lib.mrphy_blochsim_rfgr_shim_max_channels(code) == 0, code


def test_workspace_query_formula():
    r"""``(P, N, 5 + nS, nT)`` elements with ``P`` the persistent waves of ``mrphy_blochsim_rfgr_bwd``: its own query is the
    case of five rows."""
    lib = mrphy_amd.require_library()
    q = lib.mrphy_blochsim_rfgr_shim_bwd_workspace
    for code, size in zip(CODES, (4, 8, 4, 4, 4)):
        for N, nM, nT, nS in ((1, 64, 16, 1), (2, 343, 48, 3), (3, 65, 32, 8), (2, 64 * 5000, 16, 5)):
            P = min(-(-nM // 64), 2048)
            assert q(code, N, nM, nT, nS) == P * N * (5 + nS) * nT * size, (code, N, nM, nT, nS)
            assert q(code, N, nM, nT, nS) * 5 == lib.mrphy_blochsim_rfgr_bwd_workspace(code, N, nM, nT) * (5 + nS)
    assert q(0, 0, 64, 16, 3) == 0 and q(0, 1, 0, 16, 3) == 0 and q(0, 1, 64, 0, 3) == 0 and q(0, 1, 64, 16, -1) == 0
    for code in (-1, 5, 17):                                          # an unknown dtype code: 0, as the capacity query
        assert q(code, 2, 343, 48, 3) == 0, code
    assert q(0, -1, 64, 16, 3) == 0 and q(0, 1, -64, 16, 3) == 0 and q(0, 1, 64, -16, 3) == 0


def _calls(lib):
    r"""The two entry points with fake pointers (never dereferenced: no call here is valid on a problem that is not empty)."""
    fwd = lambda ops, sh=FAKE, sn=0, shMap=FAKE, nS=3, Mi=FAKE, Mo=FAKE, Mck=None, ck=0, N=1, nM=64, nT=SEG, nC=1, dtype=0: \
        lib.mrphy_blochsim_rfgr_shim_fwd(dtype, Mi, *ops, sh, sn, shMap, nS, Mo, Mck, ck, N, nM, nT, nC, None)  # noqa: E731
    bwd = lambda ops, sh=FAKE, sn=0, shMap=FAKE, nS=3, Mck=FAKE, gMo=FAKE, work=FAKE, wb=None, N=1, nM=64, nT=SEG, dtype=0: \
        lib.mrphy_blochsim_rfgr_shim_bwd(dtype, Mck, *ops, sh, sn, shMap, nS, gMo, FAKE, FAKE, FAKE, work,  # noqa: E731
                                         lib.mrphy_blochsim_rfgr_shim_bwd_workspace(0, N, nM, nT, nS) if wb is None else wb,
                                         N, nM, nT, None)
    return fwd, bwd


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ok = fused_ops()
    # 1. dtype and sizes
    for dtype in (-1, 5, 17):
        assert fwd(ok, dtype=dtype) == EINVAL and bwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
    assert fwd(ok, N=-1) == EINVAL and bwd(ok, nT=-SEG) == EINVAL, 'a negative size'
    # 2. the mode arguments, on an empty problem too
    for dtype in CODES:
        cap = lib.mrphy_blochsim_rfgr_shim_max_channels(dtype)
        for nS in (0, -1, cap + 1, 64):
            for nM in (64, 0):
                assert fwd(ok, nS=nS, nM=nM, dtype=dtype) == EINVAL, ('channels', nS, nM, dtype)
                assert bwd(ok, nS=nS, nM=nM, dtype=dtype, wb=1 << 30) == EINVAL, ('channels', nS, nM, dtype)
    assert fwd(ok, nC=2) == EINVAL and fwd(ok, nC=0) == EINVAL and fwd(ok, nM=0, nC=2) == EINVAL, 'one transmit coil'
    for ck in (0, 4, 12, -8):
        assert fwd(ok, Mck=FAKE, ck=ck) == EINVAL and fwd(ok, Mck=FAKE, ck=ck, nM=0) == EINVAL, ('checkpoints every', ck)
    for nT in (1, 7, SEG + 8, 50):
        assert bwd(ok, nT=nT) == EINVAL and bwd(ok, nT=nT, nM=0) == EINVAL, ('the adjoint takes whole segments', nT)
    # 3. empty problems: a success that launches nothing (the forward runs at nT == 0, so it needs its pointers there)
    assert fwd(ok, nM=0, sh=None, shMap=None, Mi=None, Mo=None) == 0 and fwd(ok, N=0) == 0
    assert bwd(ok, nM=0, sh=None, shMap=None) == 0 and bwd(ok, nT=0, sh=None, Mck=None) == 0 and bwd(ok, N=0) == 0
    assert bwd(ok, nM=0, wb=0, work=None) == 0, 'the empty problem comes before the pointers and the workspace'
    assert fwd(ok, nT=0, shMap=None) == EINVAL
    # 4. null pointers, before the workspace is looked at
    assert fwd(ok, sh=None) == EINVAL and fwd(ok, shMap=None) == EINVAL, 'a null sh / shMap'
    assert bwd(ok, sh=None) == EINVAL and bwd(ok, shMap=None) == EINVAL
    assert fwd(ok, Mi=None) == EINVAL and fwd(ok, Mo=None) == EINVAL, 'a null Mi / Mo'
    assert bwd(ok, Mck=None) == EINVAL and bwd(ok, gMo=None) == EINVAL and bwd(ok, work=None) == EINVAL
    assert bwd(ok, Mck=None, wb=0) == EINVAL and bwd(ok, sh=None, wb=0) == EINVAL
    for what in (dict(loc=None), dict(g=None), dict(rf=None), dict(gr=None), dict(df=FAKE), dict(E1=FAKE, E1m1=FAKE)):
        assert fwd(fused_ops(**what)) == EINVAL and bwd(fused_ops(**what)) == EINVAL, what
        assert bwd(fused_ops(**what), wb=0) == EINVAL, what
    # 5. the workspace
    for nS in (1, 3, 8):
        need = lib.mrphy_blochsim_rfgr_shim_bwd_workspace(0, 1, 64, SEG, nS)
        assert need > 0 and bwd(ok, nS=nS, wb=need - 1) == ENOSPC and bwd(ok, nS=nS, wb=0) == ENOSPC, 'a short workspace'
    # the workspace of the static adjoint is too short for any channel count
    assert bwd(ok, nS=1, wb=lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, SEG)) == ENOSPC
    # (more batch entries than a grid holds: refused by the launcher, before it launches)
    assert fwd(ok, N=65536) == EINVAL and bwd(ok, N=65536) == EINVAL, 'N > 65535'
