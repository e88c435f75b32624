r"""``fused.ab_rfgr`` under parallel transmit without a GPU: the four entry points ``mrphy_ab_rfgr_mc_max_coils`` /
``_mc_bwd_workspace`` / ``_mc_fwd`` / ``_mc_bwd`` are exported, declared and bound alike; the capacity per dtype code and
the workspace query; every refusal with fake pointers, before any launch; and the rows ``fused._decide_ab_route`` gains
with ``ptx_fused``, beside every row the sibling host tests pin, re-asserted with the default."""
import ctypes

import pytest

import mrphy_amd
from mrphy_amd import _lib
from mrphy_amd.fused import _decide_ab_route
from test_ab_rfgr_host import ROUTES as ROUTES_AB, _declared
from test_ab_spin_grads_host import ROUTES as ROUTES_SPIN
from util import FAKE, fused_ops

NAMES = ('mrphy_ab_rfgr_mc_max_coils', 'mrphy_ab_rfgr_mc_bwd_workspace', 'mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_mc_bwd')
EINVAL, ENOSPC = -1, -3
SEG = 16                    # mrphy_blochsim_rfgr_ck_every()
CODES = (_lib.F32, _lib.F64, _lib.F32_C64, _lib.F32P, _lib.F32P_C64)
TSIZE = {c: (8 if c == _lib.F64 else 4) for c in CODES}


def test_symbols_are_exported_declared_and_bound_alike():
    raw = ctypes.CDLL(mrphy_amd.build())
    for name in NAMES:
        assert hasattr(raw, name), f'{name} is not exported'
        assert name in _lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        res, args = _declared(name)
        assert (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1])) == (res, args), name
    # the one-coil entry points' arguments with the coil count before the stream
    for mc, one in (('mrphy_ab_rfgr_mc_fwd', 'mrphy_ab_rfgr_fwd'), ('mrphy_ab_rfgr_mc_bwd', 'mrphy_ab_rfgr_bwd')):
        a, b = list(_lib.PROTOTYPES[mc][1]), list(_lib.PROTOTYPES[one][1])
        assert a == b[:-1] + [ctypes.c_int64] + b[-1:], mc
    lib = mrphy_amd.require_library()
    assert lib.mrphy_abi_version() == _lib.ABI_VERSION == 5


def test_capacity_per_dtype_code():
    lib = mrphy_amd.require_library()
    for code in CODES:
        cap = lib.mrphy_ab_rfgr_mc_max_coils(code)
        assert cap == 8 if code != _lib.F64 else cap >= 4, (code, cap)
        assert cap <= lib.mrphy_blochsim_rfgr_mc_max_coils()         # the workspace rows and waves are K2b-mc's
    for code in (-1, 5, 17):
        assert lib.mrphy_ab_rfgr_mc_max_coils(code) == 0, code


def test_workspace_query_scales_with_3_plus_2nC_rows():
    lib = mrphy_amd.require_library()
    q = lib.mrphy_ab_rfgr_mc_bwd_workspace
    for code in CODES:
        for N, nM, nT in ((1, 64, SEG), (2, 100, 48), (1, 1 << 24, 32)):
            waves = q(code, N, nM, nT, 1) // (5 * N * nT * TSIZE[code])
            assert waves == min(-(-nM // 64), waves) and waves >= 1
            for nC in range(1, 9):
                assert q(code, N, nM, nT, nC) == waves * N * (3 + 2 * nC) * nT * TSIZE[code], (code, N, nM, nT, nC)
                assert q(code, N, nM, nT, nC) == lib.mrphy_blochsim_rfgr_mc_bwd_workspace(code, N, nM, nT, nC)
    for bad in ((0, 64, SEG, 4), (1, 0, SEG, 4), (1, 64, 0, 4), (1, 64, SEG, 0), (-1, 64, SEG, 4)):
        assert q(0, *bad) == 0, bad


def _calls(lib):
    r"""``fwd`` / ``bwd`` on N = 1, nM = 64, nT = 16, 4 coils with fake pointers (never dereferenced: no call here is
    valid on a problem that is not empty)."""
    def fwd(ops, A=FAKE, B=FAKE, ABck=None, ck=0, N=1, nM=64, nT=SEG, nC=4, dtype=0):
        return lib.mrphy_ab_rfgr_mc_fwd(dtype, *ops, A, B, ABck, ck, N, nM, nT, nC, None)

    def bwd(ops, ABck=FAKE, work=FAKE, wb=None, N=1, nM=64, nT=SEG, nC=4, dtype=0, gA=FAKE, gB=FAKE):
        wb = lib.mrphy_ab_rfgr_mc_bwd_workspace(0, N, nM, nT, nC) if wb is None else wb
        return lib.mrphy_ab_rfgr_mc_bwd(dtype, ABck, *ops, gA, gB, FAKE, FAKE, work, wb, N, nM, nT, nC, None)
    return fwd, bwd


OPERAND_FAULTS = {
    'loc null': dict(loc=None),
    'g null': dict(g=None),
    'rf null': dict(rf=None),
    'gr null': dict(gr=None),
    'b1 null': dict(b1=None),
    'df without gamma': dict(df=FAKE),
    'E1 without E2': dict(E1=FAKE, E1m1=FAKE),
    'E2 without E1': dict(E2=FAKE, E1m1=FAKE),
    'E1 and E2 without E1m1': dict(E1=FAKE, E2=FAKE),
    'E1m1 alone': dict(E1m1=FAKE),
}


@pytest.mark.parametrize('what', list(OPERAND_FAULTS))
def test_entry_points_check_their_operands(what):
    r"""The one-coil entry points' operand faults, and a null b1 map: MRPHY_EINVAL from both, whatever the workspace."""
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ops = fused_ops(**dict(dict(b1=FAKE), **OPERAND_FAULTS[what]))
    need = lib.mrphy_ab_rfgr_mc_bwd_workspace(0, 1, 64, SEG, 4)
    assert need > 0
    assert fwd(ops) == EINVAL
    assert bwd(ops, wb=need) == EINVAL and bwd(ops, wb=need - 1) == EINVAL


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    ok = fused_ops(b1=FAKE)
    for dtype in (-1, 5, 17):
        assert fwd(ok, dtype=dtype) == EINVAL and bwd(ok, dtype=dtype) == EINVAL, ('unknown dtype', dtype)
    assert fwd(ok, A=None) == EINVAL and fwd(ok, B=None) == EINVAL, 'a null output'
    assert bwd(ok, ABck=None) == EINVAL and bwd(ok, work=None) == EINVAL, 'null checkpoints / workspace'
    assert bwd(ok, gA=None, gB=None) == EINVAL, 'both cotangents null'
    assert fwd(ok, N=65536) == EINVAL and bwd(ok, N=65536) == EINVAL, 'N > 65535'
    assert fwd(ok, N=-1) == EINVAL and bwd(ok, nT=-SEG) == EINVAL, 'a negative size'
    for ck in (0, 4, 12, -8):
        assert fwd(ok, ABck=FAKE, ck=ck) == EINVAL, ('checkpoints every', ck)
    for nT in (1, 7, SEG + 8, 50):
        assert bwd(ok, nT=nT) == EINVAL, ('the adjoint takes whole segments', nT)
    for code in CODES:
        cap = lib.mrphy_ab_rfgr_mc_max_coils(code)
        for nC in (0, -1, cap + 1, 64):
            assert fwd(ok, nC=nC, dtype=code) == EINVAL, ('coil count', code, nC)
            assert bwd(ok, nC=nC, dtype=code, wb=1 << 40) == EINVAL, ('coil count', code, nC)
            # a mode argument: refused on an empty problem too
            assert fwd(ok, nC=nC, dtype=code, nM=0) == EINVAL and bwd(ok, nC=nC, dtype=code, nM=0, wb=0) == EINVAL
    for nC in (1, 3, 4, 8):
        need = lib.mrphy_ab_rfgr_mc_bwd_workspace(0, 1, 64, SEG, nC)
        assert bwd(ok, nC=nC, wb=need - 1) == ENOSPC and bwd(ok, nC=nC, wb=0) == ENOSPC, ('a short workspace', nC)
    # the workspace of 3 coils is short for 4
    assert bwd(ok, nC=4, wb=lib.mrphy_ab_rfgr_mc_bwd_workspace(0, 1, 64, SEG, 3)) == ENOSPC
    # ... the same with every other argument in order would be a launch: not made here


def test_empty_problems_are_a_success_whatever_the_operands_are():
    lib = mrphy_amd.require_library()
    fwd, bwd = _calls(lib)
    null = fused_ops(rf=None, gr=None, loc=None, g=None)
    assert fwd(null, A=None, B=None, nM=0) == 0 and fwd(null, A=None, B=None, N=0) == 0
    for kw in (dict(nM=0), dict(N=0), dict(nT=0)):
        assert bwd(null, ABck=None, work=None, wb=0, gA=None, gB=None, **kw) == 0, kw
    # the forward at nT == 0 with spins is NOT empty (it writes A = I, B = 0): it wants its outputs, loc, g and the map
    # -- but no pulse
    assert fwd(fused_ops(rf=None, gr=None, b1=FAKE), A=None, nT=0) == EINVAL
    assert fwd(fused_ops(rf=None, gr=None, b1=FAKE, g=None), nT=0) == EINVAL
    assert fwd(fused_ops(rf=None, gr=None), nT=0) == EINVAL


# ---------------------------------------------------------------------------------------------
# the routing decision
# ---------------------------------------------------------------------------------------------
PTX = dict(seg=SEG, one_coil=False, pulse_grad=False, maps_grad=False, consts_grad=False, ptx_fused=True)
ROUTES = [
    ('nT 48, no gradient', dict(PTX, nT=48), ('fused', False)),
    ('nT 50, no gradient', dict(PTX, nT=50), ('fused', False)),
    ('nT 48, pulse gradient', dict(PTX, nT=48, pulse_grad=True), ('fused', True)),
    ('nT 16, pulse gradient', dict(PTX, nT=16, pulse_grad=True), ('fused', True)),
    ('nT 50, pulse gradient', dict(PTX, nT=50, pulse_grad=True), ('split', 48)),
    ('nT 8, pulse gradient', dict(PTX, nT=8, pulse_grad=True), ('composed', None)),
    ('a map gradient', dict(PTX, nT=48, maps_grad=True), ('composed', None)),
    ('a map gradient the one-coil builds serve', dict(PTX, nT=48, maps_grad=True, spin_fused=True), ('composed', None)),
    ('a map gradient beside a pulse gradient', dict(PTX, nT=48, pulse_grad=True, maps_grad=True, spin_fused=True),
     ('composed', None)),
    ("a constants' gradient", dict(PTX, nT=48, consts_grad=True, spin_fused=True), ('composed', None)),
    ("a constants' gradient beside a pulse gradient, nT 50",
     dict(PTX, nT=50, pulse_grad=True, consts_grad=True, spin_fused=True), ('composed', None)),
    ('more coils than the capacity, or no map', dict(PTX, nT=48, pulse_grad=True, ptx_fused=False), ('composed', None)),
    # one coil: the flag changes nothing
    ('one coil, nT 50, pulse gradient', dict(PTX, nT=50, one_coil=True, pulse_grad=True), ('split', 48)),
    ('one coil, a map gradient', dict(PTX, nT=48, one_coil=True, maps_grad=True, spin_fused=True), ('fused', True)),
    ('one coil, a map gradient, no build', dict(PTX, nT=48, one_coil=True, maps_grad=True), ('composed', None)),
]


@pytest.mark.parametrize('what, facts, route', ROUTES, ids=[r[0] for r in ROUTES])
def test_ab_route_under_parallel_transmit(what, facts, route):
    assert _decide_ab_route(**facts) == route


@pytest.mark.parametrize('what, facts, route', ROUTES_AB + ROUTES_SPIN, ids=[r[0] for r in ROUTES_AB + ROUTES_SPIN])
def test_every_pinned_route_stands_with_the_default(what, facts, route):
    r"""Every tuple ``test_ab_rfgr_host.py`` / ``test_ab_spin_grads_host.py`` pin: unchanged without the keyword and with its
    default spelled out -- '4 coils' stays composed."""
    assert 'ptx_fused' not in facts
    assert _decide_ab_route(**facts) == route
    assert _decide_ab_route(**facts, ptx_fused=False) == route
