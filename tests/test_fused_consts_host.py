r"""``mrphy_blochsim_rfgr_consts_bwd`` and ``mrphy_signal_rfgr_consts_bwd`` on the host: what the ABI answers before any launch
(the pointers are fake and never dereferenced), the bindings, the build's unit list; and the two forms of the CPU oracle
as yardsticks of the fused adjoints on every operand form and at zero field (``oracle_fused``,
``test_slow_oracle_at_zero_field``), which ``test_fused_grads_operands.py`` rests on.  No GPU needed."""
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


# ---------------------------------------------------------------------------------------------
# the two oracle forms as yardsticks of the fused adjoints on the operand zoo and at zero field
# ---------------------------------------------------------------------------------------------
FIELD_LEAVES = ('M0', 'rf', 'gr', 'loc', 'Δf', 'b1Map')            # the explicit oracle differentiates these
CONST_LEAVES = ('T1', 'T2', 'γ', 'dt', 'γ_beff')                   # only the slow (autograd) form differentiates these


def oracle_fused(v, sim, needs, ends=None, cot=None):
    r"""The fp64 CPU oracle of the fused simulators on an operand dict ``v`` (``cases.fused_operand_variants`` /
    ``zero_field_case``), every operand in the form it is given in and those named in ``needs`` as leaves of that form:
    ``{'out': trajectory (N, *Nd, nRec, 3), <name>: gradient}`` of ``<cot, out>`` (``cot`` defaults to ``w`` on the one
    record ``ends = [nT]``).

    ``sim = 'explicit'``: ``O.rfgr2beff`` + ``O.blochsim``, whose adjoint holds the analytic zero-field limit -- the
    yardstick for ``Mi, rf, gr, loc, Δf, b1Map``.  ``sim = 'slow'``: ``O.blochsim_slow`` and autograd, the only form that
    differentiates ``T1, T2, γ, dt`` -- take nothing but those from it where a step has zero field
    (``test_slow_oracle_at_zero_field``).  It relaxes its input in place when a segment's first step has no field
    anywhere, so every segment gets a fresh non-leaf copy; and it forms ``exp(-dt / T1)`` before any padding, so a batch
    ``dt`` is padded to ``(N, 1, ...)`` here."""
    import torch
    import bloch_oracle as O
    wide = lambda x: None if x is None else x.detach().double()  # noqa: E731
    Q = {k: wide(v.get(k)) for k in FIELD_LEAVES + CONST_LEAVES}
    for k in needs:
        if Q[k] is not None:
            Q[k] = Q[k].clone().requires_grad_(True)
    beff = O.rfgr2beff(Q['rf'], Q['gr'], Q['loc'], Δf=Q['Δf'], b1Map=Q['b1Map'], γ=Q['γ_beff'])
    nT, k = beff.shape[-2], beff.ndim - 2
    ends = [nT] if ends is None else list(ends)
    dt = Q['dt'] if Q['dt'].ndim == 0 else Q['dt'].reshape(tuple(Q['dt'].shape) + (k - Q['dt'].ndim) * (1,))
    step = O.blochsim if sim == 'explicit' else O.blochsim_slow
    recs, M, t0 = [], Q['M0'], 0
    for e in ends:
        M = step(M.clone(), beff[..., t0:e, :], T1=Q['T1'], T2=Q['T2'], γ=Q['γ'], dt=dt)
        recs.append(M)
        t0 = e
    out = torch.stack(recs, dim=-2)
    cot = wide(v['w']).unsqueeze(-2) if cot is None else wide(cot)
    (out * cot).sum().backward()
    res = {k: Q[k].grad for k in needs if Q[k] is not None}
    res['out'] = out.detach()
    return res


def zero_field_maps_case(dtype, nC, nT):
    r"""``cases.zero_field_case`` with ``Δf`` an exact-zero `(N, nM)` map: a leaf beside which the field is still zero."""
    import torch
    import cases
    v, zero = cases.zero_field_case(dtype, nC, nT)
    v['Δf'] = torch.zeros(v['loc'].shape[:2], dtype=dtype)
    return v, zero


@pytest.mark.parametrize('nC', [0, 1])
@pytest.mark.parametrize('nT', [48, 53])
def test_slow_oracle_at_zero_field(nC, nT):
    r"""What the GPU tests of the fused adjoints at zero field rest on (``test_fused_grads_operands.py``), pinned so that a
    change of the oracle cannot move their yardstick unseen:

    * ``O.blochsim_slow``'s gradients w.r.t. ``T1, T2, γ, dt`` on the exact-zero case are those of the same case with every
      zero field component replaced by 1e-9 G, to 1e-6 relative (measured: <= 8.6e-9, the size of the perturbation: nothing
      of the constants' gradients hangs on the branch autograd takes at ``|B| = 0``; a wrong branch would be O(1));
    * its gradients w.r.t. ``loc``, ``Δf`` (and ``b1Map``) are NOT the explicit adjoint's there: relative L2 (nC = 0 / 1)
      0.014 / 0.024 at nT = 48 and 0.099 / 0.082 at 53 (``loc``), 0.42 .. 0.46 (``Δf``), 0.035 and 0.013 (``b1Map``, nT =
      48 and 53) -- more than 1e3 times the fp32 gate 1e-5,
      so a kernel that returned the autograd zeros on those steps would miss the explicit yardstick by that much;
    * it raises on a leaf ``Mi`` when the first step has zero field everywhere (in-place relaxation of its input)."""
    import torch
    import bloch_oracle as O
    from util import rel_l2
    v, zero = zero_field_maps_case(torch.float64, nC, nT)
    assert bool(zero[:, 0].all())
    consts = ('T1', 'T2', 'γ', 'dt')
    slow = oracle_fused(v, 'slow', consts + ('loc', 'Δf', 'b1Map'))
    expl = oracle_fused(v, 'explicit', ('loc', 'Δf', 'b1Map'))
    assert float((slow['out'] - expl['out']).abs().max()) <= 1e-12

    # (a) the constants' gradients do not hang on the zero-field branch
    wide = lambda x: None if x is None else x.detach().double()  # noqa: E731
    Q = {k: wide(v[k]).clone().requires_grad_(k in consts) for k in consts}
    beff = O.rfgr2beff(wide(v['rf']), wide(v['gr']), wide(v['loc']), Δf=wide(v['Δf']), b1Map=wide(v['b1Map']),
                       γ=wide(v['γ_beff']))
    assert int((beff == 0).sum()) > 3 * 2 * len(zero[0].nonzero())
    beff = torch.where(beff == 0, torch.full_like(beff, 1e-9), beff)
    Mo = O.blochsim_slow(wide(v['M0']).clone(), beff, **Q)
    (Mo * wide(v['w'])).sum().backward()
    for k in consts:
        assert float(slow[k].abs().max()) > 0
        assert rel_l2(slow[k], Q[k].grad) <= 1e-6, (k, rel_l2(slow[k], Q[k].grad))

    # (b) its field gradients are wrong there
    seen = {k: rel_l2(slow[k], expl[k]) for k in ('loc', 'Δf') + (('b1Map',) if nC else ())}
    assert all(d > 1e3 * 1e-5 for d in seen.values()), seen

    # (c) the in-place relaxation
    Mi = wide(v['M0']).clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='in-place'):
        O.blochsim_slow(Mi, beff * 0, T1=wide(v['T1']), T2=wide(v['T2']), γ=wide(v['γ']), dt=wide(v['dt']))
    O.blochsim_slow(Mi + 0, beff * 0, T1=wide(v['T1']), T2=wide(v['T2']), γ=wide(v['γ']), dt=wide(v['dt']))
