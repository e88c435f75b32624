r"""``fused.blochsim_rfgr_moving`` without a GPU: the routing decision ``fused._decide_ext_route`` over its truth table;
the argument errors, each raised before the device or the library is needed; the composed route's moving-z helper
against the closed form; the two entry points ``mrphy_blochsim_rfgr_moving_fwd`` / ``_bwd`` exported, declared and bound
alike, and what they refuse before any launch."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import mrphy_amd
from mrphy_amd import _lib, fused
from mrphy_amd.fused import _decide_ext_route, _moving_bz, _vel_dt
from util import FAKE, fused_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mrphy_blochsim_rfgr_moving_fwd', 'mrphy_blochsim_rfgr_moving_bwd')
EINVAL, ENOSPC = -1, -3
SEG = 16                    # mrphy_blochsim_rfgr_ck_every()


# ---------------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nT', [0, 1, 15, 16, 17, 40, 48, 1024, 1030])
def test_route_truth_table(nT):
    r"""Fused: one coil and no gradient at any length, or pulse gradients over whole segments (nT = 0 among them); split:
    such gradients, more than a segment and a ragged tail, at the last segment boundary; composed: everything else --
    parallel transmit, a gradient the kernels do not form, fewer than 16 steps with a gradient."""
    for one_coil, pulse_grad, other_grad in itertools.product((True, False), repeat=3):
        got = _decide_ext_route(nT=nT, seg=SEG, one_coil=one_coil, fits=True, pulse_grad=pulse_grad, other_grad=other_grad)
        if not one_coil or other_grad:
            want = ('composed', None)
        elif not pulse_grad:
            want = ('fused', False)
        elif nT % SEG == 0:
            want = ('fused', True)
        elif nT > SEG:
            want = ('split', nT // SEG * SEG)
        else:
            want = ('composed', None)
        assert got == want, (nT, one_coil, pulse_grad, other_grad)
    assert _decide_ext_route(nT=40, seg=SEG, one_coil=True, fits=True, pulse_grad=True, other_grad=False) == ('split', 32)
    assert _decide_ext_route(nT=8, seg=SEG, one_coil=True, fits=True, pulse_grad=True, other_grad=False) == ('composed', None)
    assert _decide_ext_route(nT=8, seg=SEG, one_coil=True, fits=True, pulse_grad=False, other_grad=False) == ('fused', False)


# ---------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------
def _operands(dtype=torch.float32, N=2, Nd=(5,), nT=16):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(s, generator=g, dtype=dtype)  # noqa: E731
    return dict(Mi=r(N, *Nd, 3), rf=r(N, 2, nT), gr=r(N, 3, nT), loc=r(N, *Nd, 3), vel=r(N, *Nd, 3))


@pytest.fixture
def no_library(monkeypatch):
    r"""The checks below must be made before the library is asked for."""
    def refuse():
        raise AssertionError('the library was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_library', refuse)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('shape', [(2, 5, 2), (2, 4, 3), (3, 5, 3), (2, 5), (2, 1, 5, 3), (2, 1, 3)])
def test_vel_of_the_wrong_shape_is_refused(shape):
    a = _operands()
    a['vel'] = torch.zeros(shape)
    with pytest.raises(ValueError, match='vel'):
        fused.blochsim_rfgr_moving(**a)


@pytest.mark.usefixtures('no_library')
def test_vel_must_be_a_tensor():
    a = _operands()
    a['vel'] = None
    with pytest.raises(ValueError, match='vel'):
        fused.blochsim_rfgr_moving(**a)


@pytest.mark.usefixtures('no_library')
@pytest.mark.parametrize('step0', [-1, -32, 1.0, 2.5, True, None, '3', torch.tensor(3)])
def test_step0_must_be_a_non_negative_int(step0):
    with pytest.raises(ValueError, match='step0'):
        fused.blochsim_rfgr_moving(**_operands(), step0=step0)


@pytest.mark.usefixtures('no_library')
def test_fp32_refuses_step_counts_beyond_2_to_the_23():
    r"""``step0 + t + 1/2`` is exact in fp32 below 2^23 only; fp64 has no such bound (it goes on to refuse the CPU tensors)."""
    a = _operands(nT=16)
    for step0 in ((1 << 23) - 16, 1 << 23, 1 << 40):
        with pytest.raises(ValueError, match='2\\*\\*23'):
            fused.blochsim_rfgr_moving(**a, step0=step0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):      # the largest count that passes
        fused.blochsim_rfgr_moving(**a, step0=(1 << 23) - 17)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.blochsim_rfgr_moving(**_operands(torch.float64), step0=1 << 40)
    with pytest.raises(ValueError, match='2\\*\\*23'):                # half tensors are computed in fp32
        fused.blochsim_rfgr_moving(**{k: x.half() for k, x in a.items()}, step0=1 << 23)


@pytest.mark.usefixtures('no_library')
def test_cpu_tensors_are_refused_as_the_other_fused_calls_refuse_them():
    a = _operands()
    with pytest.raises(RuntimeError, match='no CPU fallback') as moving:
        fused.blochsim_rfgr_moving(**a)
    with pytest.raises(RuntimeError, match='no CPU fallback') as static:
        fused.blochsim_rfgr(*(a[k] for k in ('Mi', 'rf', 'gr', 'loc')))
    assert str(moving.value) == str(static.value)


# ---------------------------------------------------------------------------------------------
# the composed route's helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Nd', [(9,), (3, 2, 2)])
@pytest.mark.parametrize('step0', [0, 32])
def test_moving_z_sums_to_the_first_moment(Nd, step0):
    r"""``sum_t _moving_bz[..., t] = m1 . vel dt`` with ``m1 = sum_t gr_t (step0 + t + 1/2)``, for a pulse per batch entry and
    a shared one; every element is ``(gr_t . vel dt)(step0 + t + 1/2)``."""
    g = torch.Generator().manual_seed(5)
    N, nT = 2, 24
    vel = torch.rand(N, *Nd, 3, generator=g, dtype=torch.float64) * 100 - 50
    loc, dt = torch.zeros(N, *Nd, 3, dtype=torch.float64), torch.tensor([4e-6], dtype=torch.float64)
    w = _vel_dt(vel, dt, loc)
    assert w.shape == loc.shape and torch.equal(w, vel * 4e-6)
    assert torch.equal(_vel_dt(vel[:1], dt, loc), (vel[:1] * 4e-6).expand(loc.shape))       # (1, *Nd, 3) broadcasts
    assert _vel_dt(vel.float(), dt.float(), loc.float()).dtype == torch.float32
    for Np in (N, 1):
        gr = torch.rand(Np, 3, nT, generator=g, dtype=torch.float64) * 2 - 1
        z = _moving_bz(gr, w, step0)
        assert z.shape == (N, *Nd, nT)
        τ = torch.arange(nT, dtype=torch.float64) + step0 + 0.5
        m1 = (gr * τ).sum(-1).expand(N, 3)
        want = (m1.reshape((N,) + (1,) * len(Nd) + (3,)) * w).sum(-1)
        assert float((z.sum(-1) - want).abs().max()) <= 1e-12 * float(want.abs().max())
        t = 7
        el = (gr[:, :, t].expand(N, 3).reshape((N,) + (1,) * len(Nd) + (3,)) * w).sum(-1) * (step0 + t + 0.5)
        assert float((z[..., t] - el).abs().max()) <= 1e-12 * float(el.abs().max())
    v = vel.clone().requires_grad_(True)                               # differentiable w.r.t. vel
    _moving_bz(gr, _vel_dt(v, dt, loc), step0).sum().backward()
    assert v.grad is not None and float(v.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'const void*': ctypes.c_void_p,
         'void*': ctypes.c_void_p}


def _declared(name):
    r"""(return type, [argument types]) of ``name`` as ``include/mrphy_hip.h`` declares it, as ctypes types."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrphy_hip.h')).read(), flags=re.S)
    m = re.search(r'\b(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, f'{name} is not declared in mrphy_hip.h'
    args = [re.sub(r'\s*\w+$', '', a.strip()).replace(' *', '*') for a in m.group(2).split(',')]
    return CTYPE[m.group(1)], [CTYPE[a] for a in args]


def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name, static in zip(NAMES, ('mrphy_blochsim_rfgr_fwd', 'mrphy_blochsim_rfgr_bwd')):
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
        # the static counterpart's arguments plus (vdt, step0), which follow the operands
        st = list(_lib.PROTOTYPES[static][1])
        assert len(args) == len(st) + 2
        assert args == st[:24] + [ctypes.c_void_p, ctypes.c_int64] + st[24:], name
    assert {'tu_fused_moving_fwd.hip', 'tu_fused_moving_bwd.hip'} <= {u for u, _ in _lib.UNITS}
    assert mrphy_amd.require_library().mrphy_abi_version() == _lib.ABI_VERSION == 5     # additive: the version stays


def _calls(lib):
    r"""The two entry points with fake pointers (never dereferenced: no call here is valid on a problem that is not empty)."""
    fwd = lambda ops, vdt=FAKE, step0=0, Mi=FAKE, Mo=FAKE, Mck=None, ck=0, N=1, nM=64, nT=SEG, nC=1, dtype=0: \
        lib.mrphy_blochsim_rfgr_moving_fwd(dtype, Mi, *ops, vdt, step0, Mo, Mck, ck, N, nM, nT, nC, None)  # noqa: E731
    bwd = lambda ops, vdt=FAKE, step0=0, Mck=FAKE, gMo=FAKE, work=FAKE, wb=None, N=1, nM=64, nT=SEG, dtype=0: \
        lib.mrphy_blochsim_rfgr_moving_bwd(dtype, Mck, *ops, vdt, step0, gMo, FAKE, FAKE, FAKE, work,  # noqa: E731
                                           lib.mrphy_blochsim_rfgr_bwd_workspace(0, N, nM, nT) if wb is None else wb,
                                           N, nM, nT, None)
    return fwd, bwd


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ok = fused_ops()
    for dtype in (-1, 5, 17):
        assert fwd(ok, dtype=dtype) == EINVAL and bwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
    assert fwd(ok, step0=-1) == EINVAL and bwd(ok, step0=-1) == EINVAL, 'a negative step0'
    assert fwd(ok, vdt=None) == EINVAL and bwd(ok, vdt=None) == EINVAL, 'a null vdt'
    assert fwd(ok, Mi=None) == EINVAL and fwd(ok, Mo=None) == EINVAL, 'a null Mi / Mo'
    assert bwd(ok, Mck=None) == EINVAL and bwd(ok, gMo=None) == EINVAL and bwd(ok, work=None) == EINVAL
    assert fwd(ok, nC=2) == EINVAL and fwd(ok, nC=0) == EINVAL, 'one transmit coil'
    assert fwd(ok, N=65536) == EINVAL and bwd(ok, N=65536) == EINVAL, 'N > 65535'
    assert fwd(ok, N=-1) == EINVAL and bwd(ok, nT=-SEG) == EINVAL, 'a negative size'
    for ck in (0, 4, 12, -8):
        assert fwd(ok, Mck=FAKE, ck=ck) == EINVAL, ('checkpoints every', ck)
    for nT in (1, 7, SEG + 8, 50):
        assert bwd(ok, nT=nT) == EINVAL, ('the adjoint takes whole segments', nT)
    need = lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, SEG)
    assert need > 0 and bwd(ok, wb=need - 1) == ENOSPC, 'a short workspace'
    for what in (dict(loc=None), dict(g=None), dict(rf=None), dict(gr=None), dict(df=FAKE), dict(E1=FAKE, E1m1=FAKE)):
        assert fwd(fused_ops(**what)) == EINVAL and bwd(fused_ops(**what)) == EINVAL, what
    # the float types form step0 + t + 1/2 exactly below 2^23 steps only; fp64 (code 1) goes on to its other checks
    big = (1 << 23) - SEG
    for dtype in (0, 2, 3, 4):
        assert fwd(ok, step0=big, dtype=dtype) == EINVAL and bwd(ok, step0=big, dtype=dtype) == EINVAL, dtype
    assert fwd(ok, step0=big, dtype=1, vdt=None) == EINVAL and fwd(ok, step0=big, dtype=1, nM=0) == 0
    # empty problems: a success that launches nothing (the forward runs at nT == 0, so it needs its pointers there)
    assert fwd(ok, nM=0, vdt=None, Mi=None, Mo=None) == 0 and fwd(ok, N=0) == 0
    assert bwd(ok, nM=0, vdt=None) == 0 and bwd(ok, nT=0, vdt=None, Mck=None) == 0 and bwd(ok, N=0) == 0
    assert fwd(ok, nT=0, vdt=None) == EINVAL
    # mode arguments are refused on an empty problem too
    assert fwd(ok, nM=0, step0=-1) == EINVAL and bwd(ok, nM=0, step0=-1) == EINVAL and fwd(ok, nM=0, nC=2) == EINVAL
