r"""``mrphy_blochsim_rfgr_consts_bwd`` and ``mrphy_signal_rfgr_consts_bwd`` on the host: what the ABI answers before any launch
(the pointers are fake and never dereferenced), the bindings, the build's unit list.  No GPU needed."""
import os

import pytest

import mrphy_amd
from mrphy_amd import _lib as L
from util import FAKE, FUSED_OPS_SET as _OPS_SET, fused_ops

EINVAL, ENOSPC = -1, -3
NEW = ('mrphy_blochsim_rfgr_consts_bwd', 'mrphy_signal_rfgr_consts_bwd')
NEW_UNITS = ('tu_fused_consts_bwd.hip', 'tu_signal_consts1_bwd.hip', 'tu_signal_consts2_bwd.hip',
             'tu_signal_consts4_bwd.hip', 'tu_signal_consts8_bwd.hip')


def _lib():
    return mrphy_amd.require_library()


def _code(dtype):
    return dtype if dtype in range(5) else 0


def _ws(dtype, N, nM, nT):
    return _lib().mrphy_blochsim_rfgr_bwd_workspace(_code(dtype), N, nM, nT)


def _maps(dtype=0, Mck=FAKE, gMo=FAKE, gMt=None, every=0, gb1=None, gC=FAKE, N=1, nM=64, nT=16, work=FAKE, work_bytes=None,
          ops=_OPS_SET):
    return _lib().mrphy_blochsim_rfgr_consts_bwd(dtype, Mck, *ops, gMo, gMt, every, None, None, None, None, None, gb1, gC,
                                                work, _ws(dtype, N, nM, nT) if work_bytes is None else work_bytes,
                                                N, nM, nT, None)


def _sig(dtype=0, Mck=FAKE, gMo=FAKE, gsig=FAKE, every=1, N=1, nM=64, nT=16, rx=FAKE, nRx=2, gC=FAKE, work=FAKE,
         work_bytes=None, ops=_OPS_SET):
    return _lib().mrphy_signal_rfgr_consts_bwd(dtype, Mck, *ops, rx, nRx, gMo, gsig, every, None, None, None, gC, work,
                                              _ws(dtype, N, nM, nT) if work_bytes is None else work_bytes, N, nM, nT, None)


def test_consts_symbols_prototypes_and_units():
    r"""The two entry points are exported with the declared prototypes -- ``mrphy_blochsim_rfgr_maps_bwd``'s and
    ``mrphy_signal_rfgr_mrx_bwd``'s with one more pointer, ``grad_consts``, in front of the workspace -- and declared in
    the header; the ABI version is still 5; the new units are in ``UNITS`` for every dtype code and their files exist."""
    lib = _lib()
    for name, base in zip(NEW, ('mrphy_blochsim_rfgr_maps_bwd', 'mrphy_signal_rfgr_mrx_bwd')):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
        bres, bargs = L.PROTOTYPES[base]
        at = len(bargs) - 6                                        # work, work_bytes, N, nM, nT, stream follow
        assert res == bres and args == bargs[:at] + [L._vp] + bargs[at:], name
    assert lib.mrphy_abi_version() == 5 == L.ABI_VERSION
    header = open(os.path.join(os.path.dirname(L._HERE), 'include', 'mrphy_hip.h')).read()
    for name in NEW:
        assert f'int {name}(int dtype,' in header, name
    assert '#define MRPHY_ABI_VERSION 5' in header
    listed = collections_of_units()
    for unit in NEW_UNITS:
        assert os.path.exists(os.path.join(L._CSRC, unit)), unit
        assert listed[unit] == {L._F32, L._F64, L._C64, L._P, L._PC64}, unit


def collections_of_units():
    out = {}
    for src, mask in L.UNITS:
        out.setdefault(src, set()).add(mask)
    return out


@pytest.mark.parametrize('dtype', [0, 1, 3])
def test_consts_entry_points_reject_bad_arguments_on_the_host(dtype):
    r"""What the sibling entry points refuse -- an unknown dtype, nT not whole checkpoint segments, every < 1 with a
    trajectory, both or neither cotangent, null Mck / work / operands, a coil count outside 1 .. capacity, a null rx for
    more than one coil, N > 65535 -- and a grad_b1 without a map: MRPHY_EINVAL; a workspace one byte short, after the null
    checks: MRPHY_ENOSPC; an empty problem: 0.  No HIP call in any of these."""
    lib = _lib()
    ck = lib.mrphy_blochsim_rfgr_ck_every()
    cap = lib.mrphy_signal_rfgr_max_rx(dtype)

    assert _maps(dtype=7) == EINVAL
    assert _maps(dtype, nT=ck + 1) == EINVAL
    assert _maps(dtype, gMo=None, gMt=FAKE, every=0) == EINVAL
    assert _maps(dtype, gMo=FAKE, gMt=FAKE, every=1) == EINVAL                # both cotangents
    assert _maps(dtype, gMo=None, gMt=None) == EINVAL                         # neither
    assert _maps(dtype, gb1=FAKE) == EINVAL                                   # a grad_b1 without a b1 map
    assert _maps(dtype, gb1=FAKE, nM=0) == EINVAL                             # a mode argument: on an empty problem too
    assert _maps(dtype, Mck=None) == EINVAL
    assert _maps(dtype, work=None) == EINVAL
    assert _maps(dtype, ops=fused_ops(loc=None)) == EINVAL
    assert _maps(dtype, ops=fused_ops(g=None)) == EINVAL
    assert _maps(dtype, ops=fused_ops(E1=FAKE)) == EINVAL                     # E1 without E2, E1m1
    assert _maps(dtype, ops=fused_ops(df=FAKE)) == EINVAL                     # df without gamma
    assert _maps(dtype, nM=0) == 0 and _maps(dtype, nT=0, Mck=None, work=None) == 0 and _maps(dtype, N=0) == 0
    need = _ws(dtype, 1, 64, ck)
    assert need > 0
    assert _maps(dtype, work_bytes=need - 1) == ENOSPC
    assert _maps(dtype, gMo=None, gMt=FAKE, every=3, work_bytes=need - 1) == ENOSPC
    assert _maps(dtype, gC=None, work_bytes=need - 1) == ENOSPC               # grad_consts is optional
    assert _maps(dtype, Mck=None, work_bytes=need - 1) == EINVAL              # null checks come first

    for nRx in (0, -1, cap + 1):
        assert _sig(dtype, nRx=nRx) == EINVAL, nRx
    assert _sig(dtype, nRx=cap + 1, nM=0) == EINVAL
    assert _sig(dtype=9) == EINVAL
    assert _sig(dtype, rx=None, nRx=2) == EINVAL                              # (1, 0) stands in for ONE coil only
    assert _sig(dtype, every=0) == EINVAL
    assert _sig(dtype, nT=ck + 1) == EINVAL
    assert _sig(dtype, gMo=None, gsig=None) == EINVAL
    assert _sig(dtype, Mck=None) == EINVAL
    assert _sig(dtype, work=None) == EINVAL
    assert _sig(dtype, N=65536) == EINVAL
    assert _sig(dtype, ops=fused_ops(loc=None)) == EINVAL
    assert _sig(dtype, every=2, nM=0) == 0 and _sig(dtype, nT=0, rx=None, Mck=None) == 0
    for nRx, rx in ((1, None), (1, FAKE), (2, FAKE), (cap, FAKE)):
        assert _sig(dtype, rx=rx, nRx=nRx, work_bytes=need - 1) == ENOSPC, nRx
    assert _sig(dtype, gMo=None, work_bytes=need - 1) == ENOSPC
    assert _sig(dtype, gsig=None, gC=None, work_bytes=need - 1) == ENOSPC
    assert _sig(dtype, Mck=None, work_bytes=need - 1) == EINVAL
