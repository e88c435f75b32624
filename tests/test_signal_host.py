r"""The signal entry points without a GPU: argument errors of the C ABI (returned before any HIP call) and the errors of
``fused.signal_rfgr`` that come before a kernel is chosen."""
import pytest
import torch

import mrphy_amd
from mrphy_amd import fused
from util import FAKE, FUSED_OPS_SET as _OPS_SET         # rf .. E1m1: rf, gr, loc and g present (fake), the rest absent

EINVAL, ENOSPC = -1, -3


def _lib():
    return mrphy_amd.require_library()


def _fwd(dtype=0, Mi=FAKE, sig=FAKE, every=1, N=1, nM=64, nT=16, nC=1, rx=None, Mo=None, work=FAKE, work_bytes=None):
    lib = _lib()
    if work_bytes is None:
        work_bytes = lib.mrphy_signal_rfgr_fwd_workspace(dtype if dtype in range(5) else 0, N, nM, nT, every)
    return lib.mrphy_signal_rfgr_fwd(dtype, Mi, *_OPS_SET, rx, Mo, None, 0, sig, every, work, work_bytes,
                                     N, nM, nT, nC, None)


def _bwd(dtype=0, Mck=FAKE, gMo=FAKE, gsig=FAKE, every=1, N=1, nM=64, nT=16, work=FAKE, work_bytes=None):
    lib = _lib()
    if work_bytes is None:
        work_bytes = lib.mrphy_blochsim_rfgr_bwd_workspace(dtype if dtype in range(5) else 0, N, nM, nT)
    return lib.mrphy_signal_rfgr_bwd(dtype, Mck, *_OPS_SET, None, gMo, gsig, every, None, None, None, work, work_bytes,
                                     N, nM, nT, None)


def test_signal_entry_points_reject_bad_arguments_on_the_host():
    r"""every < 1, a null sig, any coil count but one, an unknown dtype, N > 65535, an adjoint over a pulse that is not
    whole checkpoint segments or without a cotangent: MRPHY_EINVAL; an empty problem: 0 -- no HIP call in any of these."""
    assert _fwd(every=0) == EINVAL
    assert _fwd(every=-3) == EINVAL
    assert _fwd(sig=None) == EINVAL
    assert _fwd(Mi=None) == EINVAL
    assert _fwd(nC=0) == EINVAL
    assert _fwd(nC=2) == EINVAL                                             # parallel transmit: not in these kernels
    assert _fwd(dtype=7) == EINVAL
    assert _fwd(N=65536) == EINVAL
    assert _fwd(nM=-1) == EINVAL
    assert _fwd(nM=0, every=3) == 0                                         # empty: nothing to do
    assert _fwd(nT=0, every=3, sig=None) == 0

    ck = _lib().mrphy_blochsim_rfgr_ck_every()
    assert _bwd(every=0, nT=ck) == EINVAL
    assert _bwd(nT=ck + 1) == EINVAL                                        # nT % 16
    assert _bwd(nT=ck, gMo=None, gsig=None) == EINVAL                       # no cotangent at all
    assert _bwd(nT=ck, Mck=None) == EINVAL
    assert _bwd(dtype=9, nT=ck) == EINVAL
    assert _bwd(N=65536, nT=ck) == EINVAL
    assert _bwd(every=2, nM=0, nT=ck) == 0


@pytest.mark.parametrize('dtype', [0, 1, 3])
def test_signal_workspace_query_and_enospc(dtype):
    r"""The forward's workspace query is positive and counts records, not steps; one byte less than it -- and, for the
    adjoint, one byte less than K2b's query -- is MRPHY_ENOSPC, before any launch."""
    lib = _lib()
    ck = lib.mrphy_blochsim_rfgr_ck_every()
    need = lib.mrphy_signal_rfgr_fwd_workspace(dtype, 2, 100, 50, 3)
    assert need == 2 * 2 * 2 * 17 * (8 if dtype == 1 else 4)               # 2 waves x N x (re, im) x nRec elements
    assert lib.mrphy_signal_rfgr_fwd_workspace(dtype, 2, 100, 50, 0) == 0
    assert _fwd(dtype=dtype, N=2, nM=100, nT=50, every=3, work_bytes=need - 1) == ENOSPC
    assert _fwd(dtype=dtype, N=2, nM=100, nT=50, every=3, work=None, work_bytes=need) == EINVAL
    need_b = lib.mrphy_blochsim_rfgr_bwd_workspace(dtype, 1, 64, ck)
    assert need_b > 0
    assert _bwd(dtype=dtype, nT=ck, work_bytes=need_b - 1) == ENOSPC
    assert _bwd(dtype=dtype, nT=ck, gMo=None, work_bytes=need_b - 1) == ENOSPC
    assert _bwd(dtype=dtype, nT=ck, gsig=None, work_bytes=need_b - 1) == ENOSPC


def test_signal_python_errors():
    r"""CPU tensors raise (there is no CPU path); `every` must be an int >= 1; the function is exported."""
    assert 'signal_rfgr' in fused.__all__
    N, nM, nT = 1, 8, 16
    Mi, loc = torch.zeros(N, nM, 3), torch.zeros(N, nM, 3)
    rf, gr = torch.zeros(N, 2, nT), torch.zeros(N, 3, nT)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.signal_rfgr(Mi, rf, gr, loc, every=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.signal_rfgr(Mi, rf, gr, loc, rx=torch.zeros(N, nM, 2), return_Mo=True)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='every'):
            fused.signal_rfgr(Mi, rf, gr, loc, every=bad)
