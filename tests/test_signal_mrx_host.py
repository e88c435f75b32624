r"""The multi-coil signal entry points without a GPU: the symbols and their capacity, the forward's workspace query, and
the argument errors of the C ABI (returned before any HIP call)."""
import pytest

import mrphy_amd
from mrphy_amd import _lib as L
from util import FAKE, FUSED_OPS_SET as _OPS_SET         # rf .. E1m1: rf, gr, loc and g present (fake), the rest absent

EINVAL, ENOSPC = -1, -3
NEW = ('mrphy_signal_rfgr_max_rx', 'mrphy_signal_rfgr_mrx_fwd_workspace', 'mrphy_signal_rfgr_mrx_fwd',
       'mrphy_signal_rfgr_mrx_bwd')


def _lib():
    return mrphy_amd.require_library()


def _code(dtype):
    return dtype if dtype in range(5) else 0


def _fwd(dtype=0, Mi=FAKE, sig=FAKE, every=1, N=1, nM=64, nT=16, nC=1, rx=FAKE, nRx=2, Mo=None, work=FAKE,
         work_bytes=None):
    lib = _lib()
    if work_bytes is None:
        work_bytes = lib.mrphy_signal_rfgr_mrx_fwd_workspace(_code(dtype), N, nM, nT, every, max(nRx, 1))
    return lib.mrphy_signal_rfgr_mrx_fwd(dtype, Mi, *_OPS_SET, rx, nRx, Mo, None, 0, sig, every, work, work_bytes,
                                         N, nM, nT, nC, None)


def _bwd(dtype=0, Mck=FAKE, gMo=FAKE, gsig=FAKE, every=1, N=1, nM=64, nT=16, rx=FAKE, nRx=2, work=FAKE, work_bytes=None):
    lib = _lib()
    if work_bytes is None:
        work_bytes = lib.mrphy_blochsim_rfgr_bwd_workspace(_code(dtype), N, nM, nT)
    return lib.mrphy_signal_rfgr_mrx_bwd(dtype, Mck, *_OPS_SET, rx, nRx, gMo, gsig, every, None, None, None, work,
                                         work_bytes, N, nM, nT, None)


def test_signal_mrx_symbols_and_capacity():
    r"""The four entry points are exported and bound; every dtype code takes at least two receive coils per launch, an
    unknown code none."""
    lib = _lib()
    for name in NEW:
        assert name in L.PROTOTYPES, name
        assert getattr(lib, name).argtypes == L.PROTOTYPES[name][1], name
    assert lib.mrphy_abi_version() == 5
    for code in range(5):
        assert lib.mrphy_signal_rfgr_max_rx(code) >= 2, code
    assert lib.mrphy_signal_rfgr_max_rx(L.F32) == lib.mrphy_signal_rfgr_max_rx(L.F32P_C64)   # the data type decides
    for code in (5, 7, -1):
        assert lib.mrphy_signal_rfgr_max_rx(code) == 0, code


@pytest.mark.parametrize('dtype', [0, 1, 3])
def test_signal_mrx_workspace_query(dtype):
    r"""sig_waves(nM) · N · 2 nRx · nRec elements: one wave at nM = 64, two at nM = 100; records, not steps; one coil is
    the one-coil query; nothing for an empty problem or no coil."""
    lib = _lib()
    ts = 8 if dtype == 1 else 4
    q = lib.mrphy_signal_rfgr_mrx_fwd_workspace
    for nRx in (1, 2, 3, lib.mrphy_signal_rfgr_max_rx(dtype)):
        assert q(dtype, 1, 64, 16, 1, nRx) == 1 * 1 * 2 * nRx * 16 * ts, nRx
        assert q(dtype, 2, 100, 50, 3, nRx) == 2 * 2 * 2 * nRx * 17 * ts, nRx
    for shape in ((1, 64, 16, 1), (2, 100, 50, 3)):
        assert q(dtype, *shape, 1) == lib.mrphy_signal_rfgr_fwd_workspace(dtype, *shape)
    assert q(dtype, 2, 100, 50, 3, 0) == 0 and q(dtype, 2, 100, 50, 0, 2) == 0 and q(dtype, 2, 0, 50, 3, 2) == 0


@pytest.mark.parametrize('dtype', [0, 1, 3])
def test_signal_mrx_entry_points_reject_bad_arguments_on_the_host(dtype):
    r"""No coil, more coils than one launch takes, a null rx or sig, every < 1, any transmit-coil count but one,
    N > 65535, an unknown dtype, an adjoint over a pulse that is not whole checkpoint segments or without a cotangent:
    MRPHY_EINVAL; a workspace one byte short: MRPHY_ENOSPC; an empty problem: 0 -- no HIP call in any of these (the
    pointers are fake)."""
    lib = _lib()
    cap = lib.mrphy_signal_rfgr_max_rx(dtype)
    ck = lib.mrphy_blochsim_rfgr_ck_every()
    for nRx in (0, -1, cap + 1):
        assert _fwd(dtype, nRx=nRx) == EINVAL, nRx
        assert _bwd(dtype, nRx=nRx) == EINVAL, nRx
    assert _fwd(dtype, rx=None) == EINVAL
    assert _fwd(dtype, sig=None) == EINVAL
    assert _fwd(dtype, Mi=None) == EINVAL
    assert _fwd(dtype, every=0) == EINVAL
    assert _fwd(dtype, nC=0) == EINVAL
    assert _fwd(dtype, nC=2) == EINVAL
    assert _fwd(dtype, N=65536) == EINVAL
    assert _fwd(dtype=7) == EINVAL
    assert _fwd(dtype, work=None) == EINVAL
    assert _fwd(dtype, nM=0, every=3) == 0                                  # empty: nothing to do, nothing touched
    assert _fwd(dtype, nT=0, every=3, sig=None, rx=None) == 0
    assert _fwd(dtype, nM=0, nRx=cap + 1) == EINVAL                         # a mode argument: rejected on an empty problem too

    assert _bwd(dtype, rx=None) == EINVAL
    assert _bwd(dtype, every=0) == EINVAL
    assert _bwd(dtype, nT=ck + 1) == EINVAL                                 # nT % 16
    assert _bwd(dtype, gMo=None, gsig=None) == EINVAL                       # no cotangent at all
    assert _bwd(dtype, Mck=None) == EINVAL
    assert _bwd(dtype, N=65536) == EINVAL
    assert _bwd(dtype=9) == EINVAL
    assert _bwd(dtype, every=2, nM=0) == 0
    assert _bwd(dtype, nT=0, rx=None, Mck=None) == 0

    for nRx in (2, 3, cap):
        need = lib.mrphy_signal_rfgr_mrx_fwd_workspace(dtype, 2, 100, 50, 3, nRx)
        assert _fwd(dtype, N=2, nM=100, nT=50, every=3, nRx=nRx, work_bytes=need - 1) == ENOSPC, nRx
    need_b = lib.mrphy_blochsim_rfgr_bwd_workspace(dtype, 1, 64, ck)
    assert need_b > 0
    assert _bwd(dtype, work_bytes=need_b - 1) == ENOSPC
    assert _bwd(dtype, gMo=None, work_bytes=need_b - 1) == ENOSPC
    assert _bwd(dtype, gsig=None, work_bytes=need_b - 1) == ENOSPC
