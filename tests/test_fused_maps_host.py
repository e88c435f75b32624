r"""``mrphy_blochsim_rfgr_maps_bwd`` without a GPU: the symbol and its prototype, the argument errors of the C ABI (returned
before any HIP call, with fake pointers) and the build list."""
import ctypes
import os
import re

import mrphy_amd
from mrphy_amd import _lib as L
from util import FAKE, FUSED_OPS_NULL as _OPS, fused_ops

EINVAL, ENOSPC = -1, -3
NAME = 'mrphy_blochsim_rfgr_maps_bwd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    return mrphy_amd.require_library()


def _ck():
    return _lib().mrphy_blochsim_rfgr_ck_every()


def _call(dtype=0, Mck=FAKE, ops=None, gMo=FAKE, gMt=None, every=0, gloc=FAKE, gBz=FAKE, gb1=None, work=FAKE,
          work_bytes=None, N=1, nM=64, nT=None):
    r"""One call with every operand present (fake pointers) unless the caller takes one away."""
    lib = _lib()
    nT = _ck() if nT is None else nT
    ops = fused_ops() if ops is None else ops
    if work_bytes is None:
        work_bytes = lib.mrphy_blochsim_rfgr_bwd_workspace(dtype if dtype in range(5) else 0, max(N, 0), max(nM, 0),
                                                           max(nT, 0))
    return getattr(lib, NAME)(dtype, Mck, *ops, gMo, gMt, every, None, None, None, gloc, gBz, gb1, work, work_bytes,
                              N, nM, nT, None)


def test_maps_bwd_is_exported_and_bound_with_the_declared_prototype():
    r"""The library exports the symbol, ``_lib.PROTOTYPES`` binds it with the argument list of the header -- dtype, Mck,
    the 22 operands, grad_Mo, grad_Mt, every, the six outputs, work, work_bytes, N, nM, nT, stream -- and the ABI version
    is still 5."""
    lib = _lib()
    assert lib.mrphy_abi_version() == 5 == L.ABI_VERSION
    res, args = L.PROTOTYPES[NAME]
    fn = getattr(lib, NAME)
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == list(args)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert list(args) == [ctypes.c_int, vp] + L._PULSE_OPS + [vp, vp, i64] + [vp] * 6 + [vp, ctypes.c_size_t] + [i64] * 3 + [vp]
    # ... which is what include/mrphy_hip.h declares: the parameters of the declaration, by their C types
    hdr = open(os.path.join(ROOT, 'include', 'mrphy_hip.h')).read()
    m = re.search(r'\bint ' + NAME + r'\(([^;]*)\);', hdr)
    assert m, 'declared in include/mrphy_hip.h'
    ctype = {'int': ctypes.c_int, 'int64_t': i64, 'size_t': ctypes.c_size_t, 'void*': vp}
    decl = [ctype[' '.join(q.replace('const ', '').split()[:-1])] for q in m.group(1).split(',')]
    assert decl == list(args)
    assert re.search(r'#define MRPHY_ABI_VERSION 5\b', hdr)


def test_maps_bwd_rejects_bad_arguments_on_the_host():
    r"""What ``mrphy_blochsim_rfgr_traj_bwd`` refuses -- an unknown dtype, a negative size, a pulse that is not whole
    checkpoint segments, every < 1 with a grad_Mt, null operands, a null Mck / workspace -- and what is this entry
    point's own: both or neither of grad_Mo and grad_Mt, a grad_b1 without a b1 operand.  MRPHY_EINVAL before any HIP
    call; a short workspace MRPHY_ENOSPC.  (More than one transmit coil cannot be passed: the entry point has no coil
    count, its rf is one coil's, as for ``mrphy_blochsim_rfgr_bwd``.)"""
    ck = _ck()
    assert _call(dtype=7) == EINVAL
    assert _call(nM=-1) == EINVAL
    assert _call(nT=ck + 1) == EINVAL                                       # nT % 16
    assert _call(nT=ck - 1) == EINVAL
    assert _call(gMo=None, gMt=FAKE, every=0) == EINVAL                     # every < 1 in the trajectory modes
    assert _call(gMo=None, gMt=FAKE, every=-2) == EINVAL
    assert _call(gMo=None, gMt=None) == EINVAL                              # no cotangent
    assert _call(gMo=FAKE, gMt=FAKE, every=1) == EINVAL                     # two cotangents
    assert _call(gb1=FAKE) == EINVAL                                        # grad_b1 without a b1 map
    assert _call(gb1=FAKE, gMo=None, gMt=FAKE, every=16) == EINVAL
    assert _call(ops=list(_OPS)) == EINVAL                                  # null operands
    for gone in ('rf', 'gr', 'loc', 'g'):
        assert _call(ops=fused_ops(**{gone: None})) == EINVAL, gone
    assert _call(ops=fused_ops(df=FAKE)) == EINVAL                          # df without gamma
    assert _call(ops=fused_ops(E1=FAKE)) == EINVAL                          # E1 without E2, E1m1
    assert _call(Mck=None) == EINVAL
    assert _call(work=None) == EINVAL
    need = _lib().mrphy_blochsim_rfgr_bwd_workspace(0, 1, 64, ck)
    assert need > 0
    assert _call(work_bytes=need - 1) == ENOSPC
    assert _call(work_bytes=need - 1, gMo=None, gMt=FAKE, every=3, ops=fused_ops(b1=FAKE), gb1=FAKE) == ENOSPC


def test_maps_bwd_empty_problem_is_a_success():
    r"""No spin, no batch entry or no step: 0, with every pointer null -- nothing is read or written."""
    for size in (dict(nM=0), dict(N=0), dict(nT=0)):
        for mode in (dict(gMo=None, gMt=None), dict(gMo=None, gMt=FAKE, every=5)):
            assert _call(Mck=None, ops=list(_OPS), gloc=None, gBz=None, work=None, work_bytes=0, **size, **mode) == 0
    assert _call(nM=0, gb1=FAKE) == EINVAL                                  # a mode error is one on an empty problem too


def test_maps_unit_is_in_the_build_list_with_five_masks():
    units = [(f, m) for f, m in L.UNITS if f == 'tu_fused_maps_bwd.hip']
    assert sorted(m for _, m in units) == sorted(m for f, m in L.UNITS if f == 'tu_fused_bwd.hip')
    assert len(units) == 5 and len({m for _, m in units}) == 5
    assert os.path.exists(os.path.join(ROOT, 'mrphy.py_amd', 'csrc', 'tu_fused_maps_bwd.hip'))
