r"""The trajectory entry points without a GPU: argument errors of the C ABI (returned before any HIP call) and the
errors of ``fused.blochsim_rfgr_traj`` that come before a kernel is chosen."""
import pytest
import torch

import mrphy_amd
from mrphy_amd import fused
from util import FAKE, FUSED_OPS_NULL as _OPS, fused_ops

EINVAL, ENOSPC = -1, -3


def _lib():
    return mrphy_amd.require_library()


# (the operand lists rf .. E1m1, all null or with fake pointers: util.py; sizes and trailing arguments chosen per call)
def _fwd(dtype=0, Mi=FAKE, Mt=FAKE, every=1, N=1, nM=64, nT=16, nC=1, b1=None):
    ops = fused_ops(b1=b1)
    return _lib().mrphy_blochsim_rfgr_traj_fwd(dtype, Mi, *ops, None, None, 0, Mt, every, N, nM, nT, nC, None)


def _bwd(dtype=0, every=1, N=1, nM=64, nT=16, work=None, work_bytes=0, nC=None):
    tail = [None, every, None, None, None, work, work_bytes, N, nM, nT]
    if nC is None:
        return _lib().mrphy_blochsim_rfgr_traj_bwd(dtype, None, *_OPS, *tail, None)
    return _lib().mrphy_blochsim_rfgr_mc_traj_bwd(dtype, None, *_OPS, *tail, nC, None)


def test_traj_entry_points_reject_bad_arguments_on_the_host():
    r"""every < 1, a null Mt, a coil count K2 / K2b cannot take, a pulse that is not whole checkpoint segments, an
    unknown dtype: MRPHY_EINVAL; a short workspace: MRPHY_ENOSPC; an empty problem: 0 -- no HIP call in any of these."""
    assert _fwd(every=0) == EINVAL
    assert _fwd(every=-3) == EINVAL
    assert _fwd(every=2, Mt=None) == EINVAL                                 # null Mt
    assert _fwd(every=2, Mi=None) == EINVAL
    assert _fwd(nC=0) == EINVAL                                             # no coil
    assert _fwd(nC=4, b1=None) == EINVAL                                    # pTx without a b1 map
    assert _fwd(dtype=7) == EINVAL                                          # unknown dtype
    assert _fwd(nM=-1) == EINVAL
    assert _fwd(nM=0, every=3) == 0                                         # empty: nothing to do
    assert _fwd(nT=0, every=3, Mt=None) == 0

    ck = _lib().mrphy_blochsim_rfgr_ck_every()
    assert _bwd(every=0, nT=ck) == EINVAL
    assert _bwd(every=1, nT=ck + 1) == EINVAL                               # nT % 16
    assert _bwd(every=1, nT=ck) == EINVAL                                   # null operands
    assert _bwd(dtype=9, nT=ck) == EINVAL
    assert _bwd(every=2, nM=0, nT=ck) == 0
    max_c = _lib().mrphy_blochsim_rfgr_mc_max_coils()
    assert _bwd(every=1, nT=ck, nC=max_c + 1) == EINVAL                     # too many coils for the pTx adjoint
    assert _bwd(every=1, nT=ck, nC=0) == EINVAL
    assert _bwd(every=0, nT=ck, nC=2) == EINVAL
    assert _bwd(every=1, nT=ck + 1, nC=2) == EINVAL
    assert _bwd(every=4, nM=0, nT=ck, nC=2) == 0


def test_traj_bwd_workspace_too_small_is_enospc():
    r"""With every operand present but the workspace one byte short of K2b's query: MRPHY_ENOSPC, before any launch."""
    lib = _lib()
    ck = lib.mrphy_blochsim_rfgr_ck_every()
    fake = FAKE
    ops = fused_ops()
    need = lib.mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, ck)
    assert need > 0
    tail = [fake, 1, None, None, None, fake, need - 1, 1, 64, ck]
    assert lib.mrphy_blochsim_rfgr_traj_bwd(0, fake, *ops, *tail, None) == ENOSPC
    ops_mc = fused_ops(b1=fake)
    need = lib.mrphy_blochsim_rfgr_mc_bwd_workspace(0, 1, 64, ck, 4)
    tail = [fake, 1, None, None, None, fake, need - 1, 1, 64, ck]
    assert lib.mrphy_blochsim_rfgr_mc_traj_bwd(0, fake, *ops_mc, *tail, 4, None) == ENOSPC


def test_traj_python_errors():
    r"""CPU tensors raise (there is no CPU path); `every` must be an int >= 1."""
    N, nM, nT = 1, 8, 16
    Mi, loc = torch.zeros(N, nM, 3), torch.zeros(N, nM, 3)
    rf, gr = torch.zeros(N, 2, nT), torch.zeros(N, 3, nT)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=2)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='every'):
            fused.blochsim_rfgr_traj(Mi, rf, gr, loc, every=bad)
