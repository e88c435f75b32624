r"""Fused ``rf, gr -> Mo``: ``rfgr2beff`` + ``blochsim`` in one kernel, no ``Beff`` in HBM.

This is what ``mrphy.mobjs.SpinArray.applypulse`` does back-to-back (reference
``mobjs.py:435-446``: ``pulse2beff`` then ``sims.blochsim``).  The per-step field is assembled
in registers from the wave-uniform pulse sample and the lane's own ``loc, Δf/γ, b1Map``
(``beffective.py:137-165``), then the same step as ``mrphy_blochsim_fwd`` is applied; the result is
bit-identical to the two-kernel path.

Gradients w.r.t. ``Mi``, ``rf`` and ``gr`` (what pulse design differentiates) use the fused
adjoint ``mrphy_blochsim_rfgr_bwd``: the forward leaves a checkpoint of ``M`` every 16 steps
(0.75 B per spin-step instead of the 12 B/spin-step history plus the 24 B/spin-step of ``Beff`` and
``grad_Beff`` of the two-kernel path), each segment is recomputed in registers and swept backwards,
and ``grad_rf``/``grad_gr`` come out of a deterministic reduction over spins; parallel transmit
(``rf`` `(N,xy,nT,nCoils)` with a ``b1Map``, up to 8 coils) has its own kernel.  With one transmit coil
the same sweep also gives the gradients w.r.t. the spin-side maps ``loc``, ``Δf`` and ``b1Map``
(``mrphy_blochsim_rfgr_maps_bwd``): they are the per-step ``dL/dBeff`` the sweep holds in registers,
summed over time per spin in a fixed order, so neither ``Beff`` nor ``grad_Beff`` is ever written.
So do the gradients w.r.t. ``T1``, ``T2``, ``γ``, ``dt`` (or the entries of ``consts=``) and ``γ_beff``
(``mrphy_blochsim_rfgr_consts_bwd``, ``mrphy_signal_rfgr_consts_bwd``): the sweep sums the step constants'
gradients per spin as K3's ``mrphy_blochsim_bwd_consts`` does, and autograd carries them on to the operands.
Cases the fused adjoint does not cover (more coils, map or constants' gradients under parallel transmit, pulses
shorter than 16 steps with a map or constants' gradient) compose ``rfgr2beff`` and ``blochsim`` instead -- HIP
kernels as well; a pulse length that is not a multiple of 16 is split into a fused part and a tail
of at most 15 composed steps.

:func:`blochsim_rfgr_traj` is the same simulation with the magnetisation recorded during the pulse (the history
``Mhst`` the reference forms inside ``BlochSim.forward`` and drops, ``sims.py:83,131``), differentiable through the
trajectory kernels K2t / K2bt.

:func:`blochsim_rfgr_moving` is the same simulation for spins that move at constant velocity during the pulse (flow:
velocity-selective preparation, flow-compensated excitation, blood crossing a slice): each step's gradient field is
taken at the spin's midpoint position of that step, formed in registers (K2v), and the fused adjoint w.r.t. ``Mi``,
``rf``, ``gr`` re-forms it in its recompute and sweep (K2vb) -- no time-dependent ``Beff`` in memory.

:func:`blochsim_rfgr_shim` is the same simulation with extra longitudinal field channels, each a waveform times a map
at the spins (shim arrays, higher-order and concomitant terms, gradient nonlinearity, eddy currents): the lane keeps
its maps in registers and adds one FMA per channel and step (K2sh), and the fused adjoint returns the gradient w.r.t.
the waveforms beside those w.r.t. ``Mi``, ``rf``, ``gr`` (K2shb).

:func:`blochsim_rfgr_jvp` is the same simulation in forward mode: ``Mo`` and its directional derivatives along up to
four directions per launch -- tangents of ``Mi``, ``rf``, ``gr``, ``loc``, ``Δf``, ``b1Map``, ``T1``, ``T2`` -- carried in registers
beside the magnetisation, each step's rotation and its derivative shared by the directions (K2j); :func:`sensitivity_rfgr`
is one such call that returns per-spin sensitivity maps.

:func:`ab_sequence_jvp` is forward mode for the sequence family: :func:`ab_sequence`'s records and their derivatives along
up to four directions per launch -- tangents of ``A``, ``B``, ``Mi``, ``phase``, ``rest``, ``T1``, ``T2``, ``Δf`` -- from one pass (Ksqj);
:func:`ab_rfgr_jvp` and :func:`sequence_rfgr_jvp` put :func:`blochsim_rfgr_jvp` in front of it, from ``rf`` and ``gr``.

:func:`signal_rfgr` is the same simulation again, returning what a receive coil measures: the transverse
magnetisation summed over the spins at the trajectory's record steps (K2s, and the signal mode of K2b), without the
per-spin records in memory; the coils of a receive array share one simulation per launch.

:func:`ab_rfgr` is Hargreaves' propagator of the whole pulse per spin, ``M_after = A @ M_before + B``
(``beffective.beff2ab`` of ``beffective.rfgr2beff``), from the same operands: the four columns of ``[I | 0]`` share
each step's field and rotation (K2ab), and the gradients w.r.t. ``rf`` and ``gr`` come from a fused adjoint over the
four columns' checkpoints (K2abb) -- again without ``Beff``, a history or ``grad_Beff`` in memory.  The same sweep gives
the gradients w.r.t. ``loc``, ``Δf``, ``b1Map`` and ``γ_beff`` (``mrphy_ab_rfgr_maps_bwd``) and w.r.t. ``T1``, ``T2``, ``γ``,
``dt`` or the entries of ``consts=`` (``mrphy_ab_rfgr_consts_bwd``), as K2b's MAPS and CONSTS builds do for ``blochsim_rfgr``.
Parallel transmit (``rf`` `(N,xy,nT,nCoils)` with a ``b1Map``, up to ``mrphy_ab_rfgr_mc_max_coils`` coils: 8 in fp32, 4
in fp64) has kernels of its own for ``A, B`` and the pulse gradient (K2ab-mc / K2abb-mc, ``mrphy_ab_rfgr_mc_fwd`` /
``_mc_bwd``); more coils, and map or constants' gradients under parallel transmit, compose ``rfgr2beff`` + ``beff2ab``.

:func:`ab_steadystate` solves ``(I - A F) Mss = A f + B`` per spin for the magnetisation of a sequence that repeats the
pulse ``A, B`` after a rest ``F, f`` (``sims.freeprec``), with an adjoint w.r.t. ``A``, ``B`` and the rest's operands
(Kss / Kssb); :func:`steadystate_rfgr` is that on top of :func:`ab_rfgr`: ``Mss(rf, gr)`` and its gradient in closed
form instead of hundreds of simulated periods.

:func:`ab_train` is the transient of the same sequence: the state right after each of the first ``K`` repetitions, the
RF phase changing from one to the next (RF spoiling, phase-cycled bSSFP, a catalysed or inversion-prepared train), one
thread per spin with the recursion carried in fp64 and the records as the only saved state (Ktr / Ktrb);
:func:`train_rfgr` is that on top of :func:`ab_rfgr`.

:func:`train_signal` is that transient as a receiver sees it: per repetition the transverse magnetisation summed over
the spins, for one receive coil or an array, formed inside the kernel without the per-spin records in memory, with an
adjoint that recomputes the states per segment from fp64 checkpoints (Ktrs / Ktrsb); :func:`train_signal_rfgr` is
that on top of :func:`ab_rfgr`.

:func:`ab_sequence` is the transient of a sequence whose repetitions differ: each plays one pulse of a bank ``A, B``
after a rest of its own duration, by a host-side schedule (MR fingerprinting, prepared or variable-flip-angle trains),
still one launch each way (Ksq / Ksqb); :func:`sequence_rfgr` is that on top of one :func:`ab_rfgr` call for the bank.
"""
from math import pi as π, prod  # noqa: F401
from typing import NamedTuple, Optional

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib, _host
from ._consts import γH, dt0
from .beffective import _code

__all__ = ['blochsim_rfgr', 'blochsim_rfgr_jvp', 'sensitivity_rfgr', 'blochsim_rfgr_moving', 'blochsim_rfgr_shim', 'blochsim_rfgr_traj', 'signal_rfgr', 'ab_rfgr',
           'ab_steadystate', 'steadystate_rfgr', 'ab_train', 'train_rfgr', 'train_signal', 'train_signal_rfgr', 'ab_sequence', 'sequence_rfgr',
           'ab_sequence_jvp', 'ab_rfgr_jvp', 'sequence_rfgr_jvp',
           'sequence_signal', 'sequence_signal_rfgr', 'sequence_steadystate', 'sequence_steadystate_rfgr']


def _ptr(x):
    r"""What ctypes gets for ``x``: a tensor's address; ``None`` and plain numbers as they are."""
    return x.data_ptr() if isinstance(x, Tensor) else x


def _launch(name, device, *args):
    r"""Entry point ``name`` of the library on ``device`` and its current stream: ``args`` (a tensor passes as its
    address) followed by the stream; a non-zero return code raises."""
    lib = _lib.require_library()
    with torch.cuda.device(device):
        rc = getattr(lib, name)(*(_ptr(x) for x in args), _host.current_stream(device))
    _lib.check(rc, name)


def _forward_prep(lib, p, γ2πdt, E1, E2, E1_1, dtype, device, need):
    r"""What the two forwards share: the step constants and, if ``need``, the checkpoints the fused adjoint recomputes
    from.  Returns ``(code, alive, consts, Mck, ckpt)``: the dtype code, the constants' tensors (kept alive with
    ``consts``, their arguments ``g .. E1m1``) and the arguments ``(Mck, ck_every)``, ``(None, 0)`` without ``need``."""
    from . import sims
    code, g, e1, e2, e1m1 = sims._prep_constants(γ2πdt, E1, E2, E1_1, p.N, p.Nd, dtype, device)
    ck = int(lib.mrphy_blochsim_rfgr_ck_every())
    # one checkpoint per started segment: nCk = ceil(nT / ck_every) (include/mrphy_hip.h)
    Mck = torch.empty((-(-p.nT // ck), p.N * p.nM, 3), dtype=dtype, device=device) if need else None
    nul = _host.NULL_BC
    consts = (*g.args, *(e1.args if e1 else nul), *(e2.args if e2 else nul),
              e1m1.t.data_ptr() if e1m1 else None)
    ckpt = (Mck.data_ptr() if need else None, ck if need else 0)
    return code, (g, e1, e2, e1m1), consts, Mck, ckpt


def _likes(**given):
    r"""What the backward needs of the operands given (not ``None``) to shape their gradients: ``{name: (shape, dtype,
    device)}``."""
    return {k: (tuple(x.shape), x.dtype, x.device) for k, x in given.items() if x is not None}


def _fold_map_grads(gloc, gBz, gb1, p, likes):
    r"""``(grad_loc, grad_Δf, grad_b1Map)`` in the shapes, dtypes and on the devices the caller's operands had
    (``likes``: their entries of :func:`_likes`, ``None`` for an absent one): ``grad_Δf = gBz / γ_beff`` summed over the axes
    ``Δf`` was broadcast along (``beffective.py:161-165``); ``grad_b1Map`` likewise, with the trailing coil axis of
    length 1 if the map had one."""
    from .beffective import _sum_to
    out = [None, None, None]
    if gloc is not None:
        out[0] = gloc.to(device=likes[0][2], dtype=likes[0][1])
    if gBz is not None:
        out[1] = _sum_to(gBz / p.gam_v, likes[1][0]).to(device=likes[1][2], dtype=likes[1][1])
    if gb1 is not None:
        shape = likes[2][0]
        g = gb1[..., None] if len(shape) == 1 + len(p.Nd) + 2 else gb1
        out[2] = _sum_to(g, shape).to(device=likes[2][2], dtype=likes[2][1])
    return tuple(out)


def _fold_const_grads(gC, p, likes, needs):
    r"""``(grad_γ2πdt, grad_E1, grad_E2, grad_E1_1)`` from the per-spin ``gC`` `(N, *Nd, 4)` of the CONSTS builds: each
    summed over the axes its constant was broadcast along, in the constant's own shape and dtype and on its device
    (``likes``: their entries of :func:`_likes`, ``None`` for an absent one), ``None`` where ``needs`` does not ask -- as
    ``sims.BlochSimHIP.backward`` folds the ``gC`` of ``mrphy_blochsim_bwd_consts``."""
    from . import sims
    out = []
    for i, (like, want) in enumerate(zip(likes, needs)):
        if not want or like is None:
            out.append(None)
            continue
        c = torch.empty(like[0], dtype=like[1], device='meta')
        out.append(sims._reduce_to_const(gC[..., i], c, p.N, p.Nd).to(like[2]))
    return tuple(out)


def _fold_gamma_beff_grad(gBz, p, like):
    r"""``grad_γ_beff`` from ``gBz = dL/d(Δf / γ_beff)`` `(N, *Nd)`: ``-gBz·Δf / γ_beff²`` summed to ``γ_beff``'s own
    shape, as ``RfGr2BeffHIP.backward`` forms it (``beffective.py:161-167``)."""
    from .beffective import _sum_to
    return _sum_to(-gBz * p.df_v / (p.gam_v * p.gam_v), like[0]).to(device=like[2], dtype=like[1])


class _Saved(NamedTuple):
    r"""What a forward keeps for its backward besides the checkpoints."""
    p: object                 # the pulse on the spins (beffective._PulseOnSpins)
    code: int                 # the dtype code
    consts: tuple             # the constants' arguments g .. E1m1, pointing into ...
    alive: tuple              # ... these (g, E1, E2, E1m1; the signal: and rx)
    every: Optional[int]      # None: the plain call; else the record stride
    rx: tuple                 # the signal: (rx's pointer or None,), and the coil count for an array; else ()
    likes: dict               # _likes of the operands whose gradients the backward shapes, by argument name
    # a Bz-extended call: what it hands the library besides, by name and in the entry points' order (its tensors are kept
    # alive here) -- vdt, step0 (moving); sh, sh_sn, shMap, nS (shim)
    ext: dict = {}


SEG = 16                  # steps per checkpoint segment: mrphy_blochsim_rfgr_ck_every() (csrc/geom.hpp)
_CONSTS = ('γ2πdt', 'E1', 'E2', 'E1_1')
_MAPS = ('loc', 'Δf', 'b1Map')
# The adjoint entry points: what each takes between the operands and ``work, work_bytes, N, nM, nT[, nC], stream``, by
# the names of :func:`_fused_adjoint`'s values.
_PULSE_OUT = ('gMi', 'grf', 'ggr')
_AB_OUT = ('gA', 'gB', 'grf', 'ggr')
_ADJOINT_ARGS = {
    'mrphy_blochsim_rfgr_bwd': ('gMo', *_PULSE_OUT),
    'mrphy_blochsim_rfgr_moving_bwd': ('vdt', 'step0', 'gMo', *_PULSE_OUT),
    'mrphy_blochsim_rfgr_shim_bwd': ('sh', 'sh_sn', 'shMap', 'nS', 'gMo', *_PULSE_OUT),   # (`ggr`: the lead buffer)
    'mrphy_blochsim_rfgr_traj_bwd': ('gMt', 'every', *_PULSE_OUT),
    'mrphy_blochsim_rfgr_mc_bwd': ('gMo', *_PULSE_OUT),
    'mrphy_blochsim_rfgr_mc_traj_bwd': ('gMt', 'every', *_PULSE_OUT),
    'mrphy_blochsim_rfgr_maps_bwd': ('gMo', 'gMt', 'every', *_PULSE_OUT, 'gloc', 'gBz', 'gb1'),
    'mrphy_blochsim_rfgr_consts_bwd': ('gMo', 'gMt', 'every', *_PULSE_OUT, 'gloc', 'gBz', 'gb1', 'gC'),
    'mrphy_signal_rfgr_bwd': ('rx', 'gMo', 'gsig', 'every', *_PULSE_OUT),
    'mrphy_signal_rfgr_mrx_bwd': ('rx', 'nRx', 'gMo', 'gsig', 'every', *_PULSE_OUT),
    'mrphy_signal_rfgr_consts_bwd': ('rx', 'nRx', 'gMo', 'gsig', 'every', *_PULSE_OUT, 'gC'),
    'mrphy_ab_rfgr_bwd': _AB_OUT,
    'mrphy_ab_rfgr_mc_bwd': _AB_OUT,
    'mrphy_ab_rfgr_maps_bwd': (*_AB_OUT, 'gloc', 'gBz', 'gb1'),
    'mrphy_ab_rfgr_consts_bwd': (*_AB_OUT, 'gloc', 'gBz', 'gb1', 'gC'),
}
# The Bz-extended families -- one transmit coil, the pulse gradient only (:func:`_decide_ext_route`): the adjoint entry
# point, its workspace query and what the query takes after ``code, N, nM, nT``, by the names of ``_Saved.ext``.  With
# ``nS`` channels ``ggr`` is the lead buffer `(N, 3 + nS, nT)`: ``grad_gr``'s rows, then ``grad_sh``'s.
_EXT_FAMILIES = {
    'moving': ('mrphy_blochsim_rfgr_moving_bwd', 'mrphy_blochsim_rfgr_bwd_workspace', ()),
    'shim': ('mrphy_blochsim_rfgr_shim_bwd', 'mrphy_blochsim_rfgr_shim_bwd_workspace', ('nS',)),
}


def _need_γb(want, p):
    r"""Whether ``γ_beff`` gets a gradient: it is wanted and there is a ``Δf`` (without one the field does not depend on
    ``γ_beff``).  It is a fold of ``gBz``, which the adjoint then forms whether ``Δf`` wants its own or not."""
    return bool(want.get('γ_beff')) and p.df is not None


def _adjoint_name(family, spin, mc, mrx, traj):
    r"""The cheapest entry point of ``family`` ('blochsim', 'signal', 'ab') that serves a request: ``spin`` is ``'consts_'``
    (the CONSTS builds form the map sums too), ``'maps_'`` or ``''``; ``mc``: parallel transmit, where a map or constants'
    gradient is never wanted (:func:`_decide_route`, :func:`_decide_ab_route`); the signal's builds take one receive coil
    and an array alike, ``mrx`` says which the plain one is asked for."""
    if family in _EXT_FAMILIES:
        assert not (mc or spin or traj), f"fused.blochsim_rfgr_{family}: the adjoint w.r.t. the pulse of one transmit coil"
        return _EXT_FAMILIES[family][0]
    if family == 'signal':
        return 'mrphy_signal_rfgr_' + ('consts_' if spin == 'consts_' else 'mrx_' if mrx else '') + 'bwd'
    if family == 'ab':
        assert not (mc and spin), "fused.ab_rfgr: no map or constants' gradient under parallel transmit"
        return 'mrphy_ab_rfgr_' + ('mc_' if mc else spin) + 'bwd'
    return 'mrphy_blochsim_rfgr_' + (spin or ('mc_' if mc else '') + ('traj_' if traj else '')) + 'bwd'


def _fused_adjoint(s, Mck, family, want, gMo=None, gMt=None, gsig=None, gA=None, gB=None):
    r"""The one adjoint call of the six Functions: ``s`` the forward's :class:`_Saved`, ``Mck`` its checkpoints,
    ``family`` 'blochsim', 'moving', 'shim', 'signal' or 'ab', ``want`` the gradients wanted by argument name, ``gMo``,
    ``gMt``, ``gsig`` (``ab``: ``gA``, ``gB``) the cotangents received (contiguous, of the kernels' dtype).  Returns the raw
    gradients ``{name: tensor, or None where not wanted}``: per spin ``gMi`` (not ``ab``: it has no ``Mi``), ``gloc``,
    ``gBz`` (for ``Δf`` and ``γ_beff``), ``gb1``, ``gC``; per pulse ``grf`` `(N, 2, nT, nC)`, ``ggr`` `(N, 3, nT)` -- the shim
    call's lead buffer `(N, 3 + nS, nT)`, there when ``gr`` or ``sh`` wants a gradient."""
    lib = _lib.require_library()
    p, device, full = s.p, Mck.device, (s.p.N,) + s.p.Nd
    outs = dict(gMi=(want.get('Mi'), full + (3,)), grf=(want['rf'], (p.N, 2, p.nT, p.nC)),
                ggr=(want['gr'] or want.get('sh'), (p.N, 3 + s.ext.get('nS', 0), p.nT)),
                gloc=(want.get('loc'), full + (3,)), gBz=(want.get('Δf') or _need_γb(want, p), full),
                gb1=(want.get('b1Map'), full + (2,)), gC=(any(want[k] for k in _CONSTS), full + (4,)))
    out = {k: torch.empty(shape, dtype=Mck.dtype, device=device) if w else None for k, (w, shape) in outs.items()}
    if p.N * p.nM * p.nT == 0:
        # No spin or no step: the library's adjoints are no-ops then (``include/mrphy_hip.h``: an empty problem is a
        # success that writes nothing), so the gradients are written here -- ``Mo`` is ``Mi`` (``A = I, B = 0``) and
        # nothing depends on the pulse, the maps or the constants.
        for k, g in out.items():
            if g is not None:
                g.copy_(gMo.reshape(g.shape)) if k == 'gMi' and gMo is not None else g.zero_()
        return out
    mc, mrx = p.nC != 1, len(s.rx) > 1
    name = _adjoint_name(family, 'consts_' if out['gC'] is not None else
                         'maps_' if any(out[k] is not None for k in ('gloc', 'gBz', 'gb1')) else '', mc, mrx, gMt is not None)
    query, extra = _EXT_FAMILIES[family][1:] if family in _EXT_FAMILIES else (
        ('mrphy_ab_rfgr_mc_bwd_workspace' if family == 'ab' else 'mrphy_blochsim_rfgr_mc_bwd_workspace', ('nC',)) if mc
        else ('mrphy_blochsim_rfgr_bwd_workspace', ()))                      # (`mc`: per-coil sums)
    vals = dict(out, gMo=gMo, gMt=gMt, gsig=gsig, gA=gA, gB=gB, every=s.every or 0, rx=s.rx[0] if s.rx else None,
                nRx=s.rx[1] if mrx else 1, nC=p.nC, **s.ext)
    nbytes = int(getattr(lib, query)(s.code, p.N, p.nM, p.nT, *(vals[k] for k in extra)))
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    _launch(name, device, s.code, Mck, *p.k0_args(), *s.consts, *(vals[k] for k in _ADJOINT_ARGS[name]), work, work.numel(),
            p.N, p.nM, p.nT, *((p.nC,) if mc else ()))
    return out


def _fold_grads(raw, s, want):
    r"""``{argument name: gradient}`` from the raw gradients of :func:`_fused_adjoint`, in the shapes and dtypes the
    caller's operands had: ``Mi``, ``rf``, ``gr``, the shim call's ``sh``, the step constants, the spin-side maps and
    ``γ_beff`` -- what the backwards return."""
    from .beffective import _fold_pulse_grad
    g = dict(Mi=raw['gMi'])
    fold = lambda x, k, no_b1=False: _fold_pulse_grad(x, s.likes[k][0], s.likes[k][1], no_b1)  # noqa: E731
    lead = raw['ggr']                           # grad_gr's three rows; the shim call's lead buffer: then grad_sh's
    if raw['grf'] is not None:
        g['rf'] = fold(raw['grf'], 'rf', s.p.b1 is None)
    if lead is not None and want['gr']:
        g['gr'] = fold(lead[:, :3], 'gr')
    if lead is not None and want.get('sh'):
        g['sh'] = fold(lead[:, 3:], 'sh').to(s.likes['sh'][2])
    if raw['gC'] is not None:
        g.update(zip(_CONSTS, _fold_const_grads(raw['gC'], s.p, [s.likes.get(k) for k in _CONSTS],
                                                [want[k] for k in _CONSTS])))
    g.update(zip(_MAPS, _fold_map_grads(raw['gloc'], raw['gBz'] if want.get('Δf') else None, raw['gb1'], s.p,
                                        [s.likes.get(k) for k in _MAPS])))
    if _need_γb(want, s.p):
        g['γ_beff'] = _fold_gamma_beff_grad(raw['gBz'], s.p, s.likes['γ_beff'])
    return g


class BlochSimRfGrHIP(Function):
    r"""``M = BlochSimRfGrHIP.apply(Mi, rf, gr, pulse_on_spins, γ2πdt, E1, E2, E1_1, want_ckpt, every[, loc, Δf, b1Map])``

    ``every = None``: ``M`` is ``Mo`` (``mrphy_blochsim_rfgr_fwd`` / ``_bwd``); an int: the trajectory, time-major
    ``(nRec, N, *Nd, 3)`` (the ``_traj_`` entry points).  ``want_ckpt`` is decided by the caller
    (:func:`_route`: a gradient w.r.t. ``Mi``, ``rf`` or ``gr`` is wanted, grad mode is on and the fused adjoint
    covers the case) -- NOT re-derived from ``ctx.needs_input_grad``, which stays ``True`` under ``torch.no_grad()``.

    ``loc``, ``Δf``, ``b1Map``: the caller's own tensors, handed over only when one of them wants a gradient through
    the fused adjoint (one transmit coil; ``pulse_on_spins`` holds their detached, normalised copies, which is what
    the kernels read).  The backward then runs ``mrphy_blochsim_rfgr_maps_bwd`` in place of the two entry points
    above -- the same sweep, the same bits for ``grad_Mi``, ``grad_rf``, ``grad_gr``.  ``γ_beff`` likewise, when it
    wants a gradient and there is a ``Δf``: its gradient is a fold of the same ``gBz`` as ``Δf``'s.

    ``γ2πdt``, ``E1``, ``E2``, ``E1_1`` that require grad (:func:`_route` forms them with differentiable torch ops when
    ``T1, T2, γ, dt`` do; the entries of ``consts=`` are the caller's own) get their gradients from the same sweep
    again: ``mrphy_blochsim_rfgr_consts_bwd`` returns them per spin besides everything the entry points above return,
    bit for bit, and they are summed here over the axes each constant broadcasts along."""

    ARGS = ('Mi', 'rf', 'gr', 'p', 'γ2πdt', 'E1', 'E2', 'E1_1', 'want_ckpt', 'every', 'loc', 'Δf', 'b1Map', 'γ_beff')

    @staticmethod
    def forward(ctx, Mi, rf, gr, p, γ2πdt, E1, E2, E1_1, want_ckpt=False, every=None, loc=None, Δf=None, b1Map=None,
                γ_beff=None):
        lib = _lib.require_library()
        device, dtype = Mi.device, Mi.dtype
        code, alive, consts, Mck, ckpt = _forward_prep(lib, p, γ2πdt, E1, E2, E1_1, dtype, device, bool(want_ckpt))
        Mi_c = Mi.detach().contiguous()
        traj = every is not None
        M = (torch.empty((-(-p.nT // every), p.N) + p.Nd + (3,), dtype=dtype, device=device) if traj
             else torch.empty_like(Mi_c))
        # the trajectory's Mo is optional (it equals the last record): not asked for
        name, outs = (('mrphy_blochsim_rfgr_traj_fwd', (None, *ckpt, M, every)) if traj
                      else ('mrphy_blochsim_rfgr_fwd', (M, *ckpt)))
        _launch(name, device, code, Mi_c, *p.k0_args(), *consts, *outs, p.N, p.nM, p.nT, p.nC)
        if Mck is not None:                    # the checkpoints: a backward is wanted
            ctx.save_for_backward(Mck)
            ctx.saved = _Saved(p, code, consts, alive, every, (), _likes(
                rf=rf, gr=gr, loc=loc, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, γ2πdt=γ2πdt, E1=E1, E2=E2, E1_1=E1_1))
        return M

    @staticmethod
    def backward(ctx, grad_M):
        ARGS = BlochSimRfGrHIP.ARGS                   # (loc .. γ_beff: False where they were not handed over)
        want = dict(zip(ARGS, (*ctx.needs_input_grad, *(False,) * len(ARGS))))
        if not any(want.values()):
            return tuple(None for _ in ARGS)
        s = ctx.saved
        (Mck,) = ctx.saved_tensors
        traj = s.every is not None
        # the precise adjoint divides by E once (as the reference's does at every step): refuse E == 0 HERE, where it
        # matters -- the forward succeeds as the reference's does; cached per constants
        _host.require_invertible_relaxation(s.code, s.alive[1], s.alive[2],
                                            'fused.blochsim_rfgr_traj' if traj else 'fused.blochsim_rfgr')
        gM = grad_M.to(Mck.dtype).contiguous()  # the trajectory's: time-major, as the forward returned it -- free if so
        g = _fold_grads(_fused_adjoint(s, Mck, 'blochsim', want, **{'gMt' if traj else 'gMo': gM}), s, want)
        return tuple(g.get(k) for k in ARGS)


class SignalRfGrHIP(Function):
    r"""``sig, Mo = SignalRfGrHIP.apply(Mi, rf, gr, pulse_on_spins, rx, γ2πdt, E1, E2, E1_1, want_ckpt, every)``

    ``sig`` `(N, xy, nRec)`: the received signal (``mrphy_signal_rfgr_fwd`` / ``_bwd``), ``rx`` `(N, nM, xy)` contiguous
    or ``None``; one transmit coil.  With ``rx`` `(N, nM, xy, nRx)` contiguous, ``nRx`` up to
    ``mrphy_signal_rfgr_max_rx(code)``, ``sig`` is `(N, xy, nRec, nRx)`: every coil from one simulation, forward and
    adjoint (``mrphy_signal_rfgr_mrx_fwd`` / ``_mrx_bwd``), each coil's samples the bits the one-coil call gives.  Both
    outputs may carry a cotangent; an output the loss does not use costs nothing (its cotangent stays ``None``).
    ``want_ckpt`` as in :class:`BlochSimRfGrHIP`; so are the gradients of ``γ2πdt``, ``E1``, ``E2``, ``E1_1`` that require
    grad (``mrphy_signal_rfgr_consts_bwd``, for one coil and for an array, in place of the two adjoints above)."""

    ARGS = ('Mi', 'rf', 'gr', 'p', 'rx', 'γ2πdt', 'E1', 'E2', 'E1_1', 'want_ckpt', 'every')

    @staticmethod
    def forward(ctx, Mi, rf, gr, p, rx, γ2πdt, E1, E2, E1_1, want_ckpt=False, every=1):
        lib = _lib.require_library()
        device, dtype = Mi.device, Mi.dtype
        code, alive, consts, Mck, ckpt = _forward_prep(lib, p, γ2πdt, E1, E2, E1_1, dtype, device, bool(want_ckpt))
        mrx = (rx.shape[-1],) if rx is not None and rx.ndim == 4 else ()      # the coil count, for the _mrx_ entry points
        rxa = (None if rx is None else rx.data_ptr(), *mrx)
        Mi_c = Mi.detach().contiguous()
        sig = torch.empty((p.N, 2, -(-p.nT // every), *mrx), dtype=dtype, device=device)
        Mo = torch.empty_like(Mi_c)
        nbytes = int(lib.mrphy_signal_rfgr_mrx_fwd_workspace(code, p.N, p.nM, p.nT, every, *mrx) if mrx else
                     lib.mrphy_signal_rfgr_fwd_workspace(code, p.N, p.nM, p.nT, every))
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        if p.nT == 0:
            Mo.copy_(Mi_c)                      # no step, no record
        if p.N * p.nM * p.nT == 0:
            sig.zero_()                         # no spin: empty sums (the library writes nothing for an empty problem)
        name = 'mrphy_signal_rfgr_mrx_fwd' if mrx else 'mrphy_signal_rfgr_fwd'
        with torch.cuda.device(device):
            rc = getattr(lib, name)(code, Mi_c.data_ptr(), *p.k0_args(), *consts, *rxa, Mo.data_ptr(), *ckpt,
                                    sig.data_ptr(), every, work.data_ptr(), work.numel(),
                                    p.N, p.nM, p.nT, p.nC, _host.current_stream(device))
        _lib.check(rc, name)
        ctx.set_materialize_grads(False)
        if Mck is not None:                     # the checkpoints: a backward is wanted
            ctx.save_for_backward(Mck)
            ctx.saved = _Saved(p, code, consts, (*alive, rx), every, rxa,
                               _likes(rf=rf, gr=gr, γ2πdt=γ2πdt, E1=E1, E2=E2, E1_1=E1_1))
        return sig, Mo

    @staticmethod
    def backward(ctx, grad_sig, grad_Mo):
        want = dict(zip(SignalRfGrHIP.ARGS, ctx.needs_input_grad))
        if not any(want.values()) or (grad_sig is None and grad_Mo is None):
            return tuple(None for _ in SignalRfGrHIP.ARGS)
        s = ctx.saved
        (Mck,) = ctx.saved_tensors
        _host.require_invertible_relaxation(s.code, s.alive[1], s.alive[2], 'fused.signal_rfgr')
        cot = {k: None if x is None else x.to(Mck.dtype).contiguous() for k, x in (('gsig', grad_sig), ('gMo', grad_Mo))}
        g = _fold_grads(_fused_adjoint(s, Mck, 'signal', want, **cot), s, want)
        return tuple(g.get(k) for k in SignalRfGrHIP.ARGS)


class AbRfGrHIP(Function):
    r"""``A, B = AbRfGrHIP.apply(rf, gr, pulse_on_spins, γ2πdt, E1, E2, E1_1, want_ckpt)``

    Hargreaves' ``A`` `(N, *Nd, xyz, 3)`, ``B`` `(N, *Nd, xyz)` of the pulse on the spins (``mrphy_ab_rfgr_fwd``), one
    transmit coil; ``E1 = E2 = E1_1 = None`` is no relaxation.  Differentiable w.r.t. ``rf`` and ``gr``
    (``mrphy_ab_rfgr_bwd``); either output may go without a cotangent.  Several transmit coils (``pulse_on_spins.nC > 1``,
    which the caller has checked against ``mrphy_ab_rfgr_mc_max_coils``) run ``mrphy_ab_rfgr_mc_fwd`` / ``_mc_bwd`` instead:
    the same checkpoints, ``grad_rf`` `(N, 2, nT, nC)` folded to ``rf``'s own shape, the pulse gradient only.
    ``want_ckpt`` as in :class:`BlochSimRfGrHIP`: decided by the caller (:func:`_decide_ab_route`), and the pulse length
    is then a whole number of segments.

    ``loc``, ``Δf``, ``b1Map``, ``γ_beff``: the caller's own tensors, handed over only when one of them wants a gradient,
    as to :class:`BlochSimRfGrHIP`; ``γ2πdt``, ``E1``, ``E2``, ``E1_1`` that require grad likewise.  The backward makes ONE
    call, to the cheapest entry point that serves what is wanted: ``mrphy_ab_rfgr_bwd``, ``mrphy_ab_rfgr_maps_bwd`` (the
    maps) or ``mrphy_ab_rfgr_consts_bwd`` (the constants, with or without maps) -- the same sweep, the same bits for
    ``grad_rf`` and ``grad_gr`` -- and folds the per-spin gradients to the operands' own shapes."""

    ARGS = ('rf', 'gr', 'p', 'γ2πdt', 'E1', 'E2', 'E1_1', 'want_ckpt', 'loc', 'Δf', 'b1Map', 'γ_beff')

    @staticmethod
    def forward(ctx, rf, gr, p, γ2πdt, E1, E2, E1_1, want_ckpt=False, loc=None, Δf=None, b1Map=None, γ_beff=None):
        lib = _lib.require_library()
        device, dtype = p.device, p.dtype
        code, alive, consts, _, _ = _forward_prep(lib, p, γ2πdt, E1, E2, E1_1, dtype, device, False)
        ck = int(lib.mrphy_blochsim_rfgr_ck_every())
        # the four columns' checkpoints, one set per started segment: (ceil(nT / ck), 4, N nM, 3)
        ABck = torch.empty((-(-p.nT // ck), 4, p.N * p.nM, 3), dtype=dtype, device=device) if want_ckpt else None
        A = torch.empty((p.N,) + p.Nd + (3, 3), dtype=dtype, device=device)
        B = torch.empty((p.N,) + p.Nd + (3,), dtype=dtype, device=device)
        mc = p.nC != 1                          # parallel transmit: the `_mc_` entry points, which take the coil count
        name = 'mrphy_ab_rfgr_mc_fwd' if mc else 'mrphy_ab_rfgr_fwd'
        with torch.cuda.device(device):
            rc = getattr(lib, name)(code, *p.k0_args(), *consts, A.data_ptr(), B.data_ptr(),
                                    ABck.data_ptr() if want_ckpt else None, ck if want_ckpt else 0,
                                    p.N, p.nM, p.nT, *((p.nC,) if mc else ()), _host.current_stream(device))
        _lib.check(rc, name)
        ctx.set_materialize_grads(False)
        if want_ckpt:
            ctx.save_for_backward(ABck)
            ctx.saved = _Saved(p, code, consts, alive, None, (), _likes(
                rf=rf, gr=gr, loc=loc, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, γ2πdt=γ2πdt, E1=E1, E2=E2, E1_1=E1_1))
        return A, B

    @staticmethod
    def backward(ctx, grad_A, grad_B):
        ARGS = AbRfGrHIP.ARGS                         # (loc .. γ_beff: False where they were not handed over)
        want = dict(zip(ARGS, (*ctx.needs_input_grad, *(False,) * len(ARGS))))
        if not any(want.values()) or (grad_A is None and grad_B is None):
            return tuple(None for _ in ARGS)
        s = ctx.saved
        (ABck,) = ctx.saved_tensors
        _host.require_invertible_relaxation(s.code, s.alive[1], s.alive[2], 'fused.ab_rfgr')
        cot = {k: None if x is None else x.to(ABck.dtype).contiguous() for k, x in (('gA', grad_A), ('gB', grad_B))}
        g = _fold_grads(_fused_adjoint(s, ABck, 'ab', want, **cot), s, want)
        return tuple(g.get(k) for k in ARGS)


class _JoinAb(Function):
    r"""``A, B = _JoinAb.apply(A1, B1, A2, B2)``: the propagator of a head ``(A1, B1)`` followed by a tail ``(A2, B2)``,
    ``A = A2 @ A1``, ``B = A2 @ B1 + B2`` -- the join of :func:`ab_rfgr`'s split route.  Its backward forms the four
    3x3 products on CONTIGUOUS copies of the cotangents: left to autograd, the batched products take a cotangent in
    whatever strides the caller's loss gave it, and a permuted one rounds differently from a contiguous one of the same
    values (one ulp in fp64) -- the gradients then depended on the spelling of the cotangent."""

    @staticmethod
    def forward(ctx, A1, B1, A2, B2):
        ctx.save_for_backward(A1, B1, A2)
        return A2 @ A1, (A2 @ B1[..., None])[..., 0] + B2

    @staticmethod
    def backward(ctx, grad_A, grad_B):
        A1, B1, A2 = ctx.saved_tensors
        gA, gB = grad_A.contiguous(), grad_B.contiguous()
        A2t = A2.transpose(-1, -2)
        return (A2t @ gA, (A2t @ gB[..., None])[..., 0],
                gA @ A1.transpose(-1, -2) + gB[..., None] * B1[..., None, :], gB)


def _ab_spin_fused(dtype, consts_grad):
    r"""Whether K2abb's MAPS / CONSTS builds serve :func:`ab_rfgr`'s map and constants' gradients in ``dtype``: every
    build of the library does.  Kept as the seam through which ``tests/test_ab_spin_grads.py`` switches them off to
    obtain the composed route."""
    return True


def _decide_ab_route(*, nT, seg, one_coil, pulse_grad, maps_grad, consts_grad, spin_fused=False, ptx_fused=False):
    r"""The route of :func:`ab_rfgr` as a function of plain facts (``maps_grad``: a gradient w.r.t. ``loc``, ``Δf``,
    ``b1Map`` or a ``γ_beff`` that multiplies a ``Δf``; ``spin_fused``: the fused adjoint's MAPS / CONSTS builds serve
    the map and constants' gradients that are wanted -- :func:`ab_rfgr` says so, the default is the adjoint w.r.t. the
    pulse alone; ``ptx_fused``: several transmit coils with their ``b1Map``, no more than the parallel-transmit kernels
    K2ab-mc / K2abb-mc take -- the default keeps parallel transmit composed): ``('fused', want_ckpt)`` -- one transmit
    coil and either no gradient or gradients the fused adjoint serves over whole checkpoint segments, or such coils and
    at most a pulse gradient; ``('split', n1)`` -- such gradients, more than one segment's steps and a ragged last one:
    the first ``n1`` steps fused, the tail composed; ``('composed', None)`` -- everything else (a map or constants'
    gradient under parallel transmit among it): ``rfgr2beff`` + ``beff2ab``, whose autograd serves every operand."""
    spin_grad = maps_grad or consts_grad
    ptx = ptx_fused and not one_coil and not spin_grad
    if not (one_coil or ptx) or (spin_grad and not spin_fused):
        return 'composed', None
    if not (pulse_grad or spin_grad):
        return 'fused', False
    if nT % seg == 0:
        return 'fused', True
    if nT > seg:
        return 'split', (nT // seg) * seg
    return 'composed', None


def _decide_route(*, nT, seg, nC, one_coil, has_b1, f64, signal, ptx_max, pulse_grad, maps_grad, consts_grad, rx_grad,
                  γb_grad=False):
    r"""The decision of :func:`_route`, which explains it, as a function of plain facts (``ptx_max``: the coil limit of
    the parallel-transmit adjoint; ``maps_grad`` includes ``γb_grad``): ``('split', n1)``, ``('composed', None)`` or
    ``('fused', want_ckpt, maps_fused, γb_grad)`` -- run the Function, with checkpoints, handing it the maps and ``γ_beff``."""
    seg_ok = nT % seg == 0
    ptx = 1 < nC <= ptx_max and has_b1 and not signal
    fused_adjoint_ok = seg_ok and (one_coil or ptx)
    # the map gradients come out of the one-coil adjoint's sweep (the MAPS builds of K2b / K2bt); the signal call keeps
    # its composed route for them, whose trajectory takes this one
    maps_fused = maps_grad and one_coil and not signal
    # the constants' gradients likewise (the CONSTS builds), in the signal call as well -- but not under parallel transmit
    consts_fused = consts_grad and one_coil and (not signal or not maps_grad)
    if not seg_ok and nT > seg and not rx_grad and (not consts_grad or consts_fused) and \
            (maps_fused or ((pulse_grad or consts_fused) and not maps_grad and (one_coil or ptx))):
        return 'split', (nT // seg) * seg
    # fp64 with more than 8 transmit coils: the fused forward has no register build for it (it would spill),
    # the composed route does (k_rfgr2beff_steps / _pk + K1) and gives the same bits
    wide_f64 = (f64 and nC > 8) or (has_b1 and nC > 64)   # (> 64: coil-blocked K0 + K1)
    if (maps_grad and not (maps_fused and seg_ok)) or rx_grad or wide_f64 or (pulse_grad and not fused_adjoint_ok) \
            or (signal and nC != 1) or (consts_grad and not (consts_fused and seg_ok)):
        return 'composed', None
    return 'fused', (pulse_grad or maps_fused or consts_fused) and fused_adjoint_ok, maps_fused, γb_grad


def _requires_grad(x) -> bool:
    return torch.is_grad_enabled() and isinstance(x, Tensor) and x.requires_grad


class _PulseFacts(NamedTuple):
    r"""What :func:`_route` and :func:`ab_rfgr` know of a call before they decide its route."""
    p: object                 # the pulse on the spins, of the detached operands (beffective._PulseOnSpins)
    one_coil: bool            # one transmit coil: rf without a coil axis, or one whose coils a b1Map does not weight
    pulse_grad: bool          # Mi, rf or gr requires grad
    maps_grad: bool           # loc, Δf or b1Map does, or γb_grad
    γb_grad: bool             # γ_beff does and there is a Δf (without one the field does not depend on γ_beff)
    consts_grad: bool         # T1, T2, γ or dt does -- or an entry of consts=


def _pulse_facts(rf, gr, loc, kw, Mi=None):
    from . import beffective
    Δf, b1Map = kw['Δf'], kw['b1Map']
    γb_grad = _requires_grad(kw['γ_beff']) and Δf is not None
    maps_grad = any(_requires_grad(x) for x in (loc, Δf, b1Map)) or γb_grad
    pulse_grad = any(_requires_grad(x) for x in (Mi, rf, gr))
    consts_grad = any(_requires_grad(x) for x in (kw['consts'].values() if kw['consts'] is not None
                                                  else (kw['T1'], kw['T2'], kw['γ'], kw['dt'])))
    p = beffective._PulseOnSpins(rf.detach(), gr.detach(), loc.detach(), None if Δf is None else Δf.detach(),
                                 None if b1Map is None else b1Map.detach(), kw['γ_beff'].detach())
    one_coil = p.nC == 1 and (rf.ndim == 3 or b1Map is not None or rf.shape[-1] == 1)
    return _PulseFacts(p, one_coil, pulse_grad, maps_grad, γb_grad, consts_grad)


def _step_constants(kw, consts_grad, ndim, device):
    r"""``(γ2πdt, E1, E2, E1_1)`` of a call: the entries of ``consts=``; or, when one of ``T1, T2, γ, dt`` requires grad,
    differentiable tensors formed as ``slowsims.blochsim`` forms them -- ``relax_constants``' expressions on the same
    padded operands on the same device, so the values, and the result, are the bits of the call that does not
    differentiate them; or :func:`mrphy_amd.sims.relax_constants` itself."""
    from . import sims
    if kw['consts'] is not None:
        return tuple(kw['consts'].get(k) for k in _CONSTS)
    if consts_grad:
        cdev = _host.const_device(device)
        pad = lambda x: None if x is None else _host.pad_trailing(x.to(cdev), ndim)  # noqa: E731
        return sims._gamma_dt_constants(pad(kw['T1']), pad(kw['T2']), pad(kw['γ']), pad(kw['dt']))
    return sims.relax_constants(kw['T1'], kw['T2'], kw['γ'], kw['dt'], ndim, device)


def _route(Mi, rf, gr, loc, every, kw, signal=False, rx=None):
    r"""The routing :func:`blochsim_rfgr` (``every = None``), :func:`blochsim_rfgr_traj` and (``signal``, with its
    receive map ``rx``) :func:`signal_rfgr` share; the decision itself is :func:`_decide_route`'s.  Returns
    ``('split', n1)``: a gradient through the fused adjoint, but a length that is not a whole number of
    checkpoint segments -- the caller runs the first ``n1`` steps fused and composes the tail (autograd adds the two
    parts' gradients w.r.t. the maps); ``('composed', None)``: a case the fused kernels do not cover (gradients w.r.t.
    the spin-side maps under parallel transmit, in the signal call or with fewer than 16 steps, fp64 with more than 8
    coils, a pulse gradient the fused adjoint cannot form); or ``('fused', M)``, the result of :class:`BlochSimRfGrHIP` -- for the
    signal :class:`SignalRfGrHIP`'s ``(sig, Mo)``.  An ``rx`` with a coil axis of two or more runs one application per
    block of up to ``mrphy_signal_rfgr_max_rx(code)`` coils -- one forward and one backward launch for all of a
    block's coils; ``sig`` is the blocks' concatenated on the coil axis, ``Mo`` the first block's, and autograd adds the
    blocks' gradients.  The signal kernels take one transmit coil and form no gradient w.r.t. ``rx``: parallel transmit
    and that gradient are composed.

    ``consts_grad``: one of ``T1, T2, γ, dt`` -- or an entry of ``consts=`` -- requires grad.  With one transmit coil
    and whole segments the constants then reach the Function as differentiable tensors (formed as
    ``slowsims.blochsim`` forms them, with the values :func:`mrphy_amd.sims.relax_constants` gives) and its backward
    runs the CONSTS builds; every other case is composed, or split as above.  A ``γ_beff`` that requires grad where
    there is a ``Δf`` counts with the spin-side maps: its gradient is a fold of theirs."""
    _host.require_device_tensor(Mi, 'Mi')
    assert (kw['T1'] is None) == (kw['T2'] is None)
    lib = _lib.require_library()
    f = _pulse_facts(rf, gr, loc, kw, Mi)
    p, Δf, b1Map = f.p, kw['Δf'], kw['b1Map']
    decision = _decide_route(
        nT=p.nT, seg=int(lib.mrphy_blochsim_rfgr_ck_every()), nC=p.nC, one_coil=f.one_coil, has_b1=p.b1 is not None,
        f64=p.dtype == torch.float64, signal=signal, ptx_max=int(lib.mrphy_blochsim_rfgr_mc_max_coils()),
        pulse_grad=f.pulse_grad, maps_grad=f.maps_grad, consts_grad=f.consts_grad,
        rx_grad=signal and _requires_grad(rx), γb_grad=f.γb_grad)
    if decision[0] != 'fused':
        return decision
    _, want, maps_fused, _ = decision

    device, dtype = Mi.device, Mi.dtype
    assert p.device == device and p.dtype == dtype, "Mi and loc must share device and dtype"
    assert tuple(Mi.shape[:-1]) == (p.N,) + p.Nd
    γ2πdt, E1, E2, E1_1 = _step_constants(kw, f.consts_grad, 1 + len(p.Nd) + 2, device)
    if signal:
        apply = lambda r: SignalRfGrHIP.apply(Mi, rf, gr, p, r, γ2πdt, E1, E2, E1_1, want, every)  # noqa: E731
        if rx is None:
            return 'fused', apply(None)         # the plain sums
        # (N, *Nd, xy[, nRx]) -> (N, nM, xy, nRx), without a copy if it is contiguous already (the coil count spelled
        # out: a `-1` is ambiguous for a map without spins, nM == 0)
        nrx = rx.shape[-1] if rx.ndim == Mi.ndim + 1 else 1
        r = rx.detach().to(device=device, dtype=dtype).expand((p.N,) + p.Nd + tuple(rx.shape[1 + len(p.Nd):])) \
            .reshape(p.N, p.nM, 2, nrx)
        if nrx == 1:                            # one coil: the one-coil kernels, a coil axis kept if there was one
            sig, Mo = apply(r[..., 0].contiguous())
            return 'fused', (sig.unsqueeze(-1) if rx.ndim == Mi.ndim + 1 else sig, Mo)
        # (the capacity depends on the data type alone, not on the constants' precision)
        cap = int(lib.mrphy_signal_rfgr_max_rx(_code(dtype)))
        outs = [apply(r[..., c:c + cap].contiguous()) for c in range(0, nrx, cap)]
        return 'fused', (outs[0][0] if len(outs) == 1 else torch.cat([o[0] for o in outs], dim=-1), outs[0][1])
    maps = (loc, Δf, b1Map, kw['γ_beff'] if f.γb_grad else None) if maps_fused else ()
    return 'fused', BlochSimRfGrHIP.apply(Mi, rf, gr, p, γ2πdt, E1, E2, E1_1, want, every, *maps)


@_host.half_via_float
def blochsim_rfgr(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
) -> Tensor:
    r"""``blochsim(Mi, rfgr2beff(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ=γ_beff), T1=T1, T2=T2,
    γ=γ, dt=dt)`` without the intermediate tensor, differentiable w.r.t. ``Mi``, ``rf``, ``gr`` and the spin-side
    maps ``loc``, ``Δf``, ``b1Map`` (with one transmit coil through the fused adjoint, which sums the sweep's
    ``dL/dBeff`` over time per spin; parallel transmit and pulses shorter than 16 steps through ``rfgr2beff`` +
    ``blochsim``), and w.r.t. ``T1``, ``T2``, ``γ``, ``dt`` (or the entries of ``consts``) and ``γ_beff`` the same way:
with one transmit coil the fused adjoint returns the step constants' gradients per spin from the same sweep
(``mrphy_blochsim_rfgr_consts_bwd``), otherwise ``rfgr2beff`` + ``slowsims.blochsim`` do.

    ``Mi``: `(N, *Nd, xyz)`; the other arguments as in
    :func:`mrphy_amd.beffective.rfgr2beff` and :func:`mrphy_amd.sims.blochsim`.  ``consts``
    (``dict(γ2πdt=, E1=, E1_1=, E2=)``) replaces ``T1, T2, γ, dt`` as in
    :func:`mrphy_amd.sims.blochsim_consts`.
    """
    from . import beffective, sims, slowsims
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    route, out = _route(Mi, rf, gr, loc, None, kw)
    if route == 'split':
        # A pulse length that is not a whole number of checkpoint segments: the first
        # floor(nT/16)*16 steps go through the fused pair, the remaining <= 15 steps through
        # rfgr2beff + blochsim, whose Beff is then tiny.  Autograd chains the two; the forward is
        # the same step arithmetic throughout (bit-identical to a single pass).
        M1 = blochsim_rfgr(Mi, rf[:, :, :out], gr[:, :, :out], loc, **kw)
        return blochsim_rfgr(M1, rf[:, :, out:], gr[:, :, out:], loc, **kw)
    if route == 'composed':
        beff = beffective.rfgr2beff(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ=γ_beff, lazy=False)
        if consts is not None:
            return sims.blochsim_consts(Mi, beff, **consts)
        # (slowsims.blochsim is sims.blochsim unless T1, T2, γ or dt requires grad: then K3 returns their gradients too)
        return slowsims.blochsim(Mi, beff, T1=T1, T2=T2, γ=γ, dt=dt)
    return out


def _ext_forward(ctx, name, Mi, p, step_consts, want_ckpt, ext, likes):
    r"""The forward of the two Bz-extended Functions: :class:`BlochSimRfGrHIP`'s plain one with ``ext``'s values -- what the
    entry point ``name`` takes between the constants and ``Mo``, by name and in its order -- which the backward gets as
    ``_Saved.ext``."""
    device, dtype = Mi.device, Mi.dtype
    code, alive, consts, Mck, ckpt = _forward_prep(_lib.require_library(), p, *step_consts, dtype, device, bool(want_ckpt))
    Mi_c = Mi.detach().contiguous()
    Mo = torch.empty_like(Mi_c)
    _launch(name, device, code, Mi_c, *p.k0_args(), *consts, *ext.values(), Mo, *ckpt, p.N, p.nM, p.nT, p.nC)
    if Mck is not None:                         # the checkpoints: a backward is wanted
        ctx.save_for_backward(Mck)
        ctx.saved = _Saved(p, code, consts, alive, None, (), likes, ext)
    return Mo


def _ext_backward(ctx, Fn, family, grad_Mo):
    r"""The backward of the two Bz-extended Functions ``Fn``: the one adjoint call of ``family`` and its folds."""
    want = dict(zip(Fn.ARGS, ctx.needs_input_grad))
    if not any(want.values()):
        return tuple(None for _ in Fn.ARGS)
    s = ctx.saved
    (Mck,) = ctx.saved_tensors
    _host.require_invertible_relaxation(s.code, s.alive[1], s.alive[2], 'fused.blochsim_rfgr_' + family)
    gMo = grad_Mo.to(Mck.dtype).contiguous()
    g = _fold_grads(_fused_adjoint(s, Mck, family, want, gMo=gMo), s, want)
    return tuple(g.get(k) for k in Fn.ARGS)


class BlochSimRfGrMovingHIP(Function):
    r"""``Mo = BlochSimRfGrMovingHIP.apply(Mi, rf, gr, pulse_on_spins, vdt, step0, γ2πdt, E1, E2, E1_1, want_ckpt)``

    :class:`BlochSimRfGrHIP`'s plain call for spins that move: ``vdt`` `(N, *Nd, xyz)` contiguous, of the kernels' dtype,
    is the displacement per step, ``step0`` the number of steps played before this call
    (``mrphy_blochsim_rfgr_moving_fwd`` / ``_bwd``, one transmit coil).  Differentiable w.r.t. ``Mi``, ``rf`` and ``gr``;
    ``want_ckpt`` is the caller's decision (:func:`_decide_ext_route`), as there."""

    ARGS = ('Mi', 'rf', 'gr', 'p', 'vdt', 'step0', 'γ2πdt', 'E1', 'E2', 'E1_1', 'want_ckpt')

    @staticmethod
    def forward(ctx, Mi, rf, gr, p, vdt, step0, γ2πdt, E1, E2, E1_1, want_ckpt=False):
        return _ext_forward(ctx, 'mrphy_blochsim_rfgr_moving_fwd', Mi, p, (γ2πdt, E1, E2, E1_1), want_ckpt,
                            dict(vdt=vdt, step0=step0), _likes(rf=rf, gr=gr))

    @staticmethod
    def backward(ctx, grad_Mo):
        return _ext_backward(ctx, BlochSimRfGrMovingHIP, 'moving', grad_Mo)


def _decide_ext_route(*, nT, seg, one_coil, fits, pulse_grad, other_grad):
    r"""The route of :func:`blochsim_rfgr_moving` and :func:`blochsim_rfgr_shim` as a function of plain facts (``fits``:
    the kernels take the extension -- the ``nS >= 1`` channels are no more than one launch takes; motion always does;
    ``pulse_grad``: ``Mi``, ``rf``, ``gr`` or ``sh`` requires grad; ``other_grad``: ``vel``, ``shMap``, ``loc``, ``Δf``,
    ``b1Map``, ``γ_beff``, ``T1``, ``T2``, ``γ``, ``dt`` or an entry of ``consts`` does): ``('fused', want_ckpt)`` -- one
    transmit coil, an extension that fits and either no gradient, at any length, or pulse gradients over whole checkpoint
    segments; ``('split', n1)`` -- such gradients, more than one segment's steps and a ragged last one: the first ``n1``
    steps fused, the tail composed; ``('composed', None)`` -- everything else."""
    if not one_coil or not fits or other_grad:
        return 'composed', None
    if not pulse_grad:
        return 'fused', False
    if nT % seg == 0:
        return 'fused', True
    if nT > seg:
        return 'split', (nT // seg) * seg
    return 'composed', None


# The two routes under the names and facts they had as functions of their own (``nS`` channels against the capacity ``cap``
# of one launch): host tests written against those names keep importing them.
def _decide_moving_route(**facts):
    return _decide_ext_route(fits=True, **facts)


def _decide_shim_route(*, nS, cap, **facts):
    return _decide_ext_route(fits=nS <= cap, **facts)


def _bz_extended(Mi, rf, gr, loc, kw, *, fits, pulse_grad, other_grad, bz, again, apply):
    r"""What :func:`blochsim_rfgr_moving` and :func:`blochsim_rfgr_shim` do once their own arguments are checked: the
    facts, the route (:func:`_decide_ext_route`; ``fits`` as there, ``pulse_grad`` / ``other_grad``: an operand of the
    extension's own wants a gradient the kernels form / do not form) and the route taken.  Split:
    ``again(M, slice, n0)`` re-issues the call from ``M`` on that slice of the time axis, ``n0`` steps into the pulse.
    Composed: ``rfgr2beff``, ``bz(beff)`` -- what the extension adds to its z component -- then ``blochsim``.  Fused:
    ``apply(p, step_constants, want_ckpt)``, the extension's Function."""
    from . import beffective, sims, slowsims
    assert (kw['T1'] is None) == (kw['T2'] is None)
    f = _pulse_facts(rf, gr, loc, kw, Mi)
    p = f.p
    route, arg = _decide_ext_route(nT=p.nT, seg=SEG, one_coil=f.one_coil, fits=fits, pulse_grad=f.pulse_grad or pulse_grad,
                                   other_grad=f.maps_grad or f.consts_grad or other_grad)
    if route == 'split':
        return again(again(Mi, slice(None, arg), 0), slice(arg, None), arg)
    if route == 'composed':
        beff = beffective.rfgr2beff(rf, gr, loc, Δf=kw['Δf'], b1Map=kw['b1Map'], γ=kw['γ_beff'], lazy=False)
        beff = beff + torch.nn.functional.pad(bz(beff).unsqueeze(-1), (2, 0))   # out of place: beff may be saved upstream
        if kw['consts'] is not None:
            return sims.blochsim_consts(Mi, beff, **kw['consts'])
        return slowsims.blochsim(Mi, beff, T1=kw['T1'], T2=kw['T2'], γ=kw['γ'], dt=kw['dt'])
    device, dtype = Mi.device, Mi.dtype
    assert p.device == device and p.dtype == dtype, "Mi and loc must share device and dtype"
    assert tuple(Mi.shape[:-1]) == (p.N,) + p.Nd
    assert int(_lib.require_library().mrphy_blochsim_rfgr_ck_every()) == SEG
    return apply(p, _step_constants(kw, False, 1 + len(p.Nd) + 2, device), arg)


def _check_moving(Mi, gr, loc, vel, step0):
    r"""The argument checks of :func:`blochsim_rfgr_moving` that need neither the device nor the library."""
    if not isinstance(vel, Tensor) or vel.ndim != loc.ndim or vel.shape[-1] != 3 or \
            vel.shape[0] not in (1, loc.shape[0]) or tuple(vel.shape[1:-1]) != tuple(loc.shape[1:-1]):
        raise ValueError(f"mrphy_amd: `vel` must be (N ⊻ 1, *Nd, xyz) beside loc {tuple(loc.shape)}, got "
                         f"{tuple(vel.shape) if isinstance(vel, Tensor) else vel!r}")
    if isinstance(step0, bool) or not isinstance(step0, int) or step0 < 0:
        raise ValueError(f"mrphy_amd: `step0` must be an int >= 0, got {step0!r}")
    if Mi.dtype != torch.float64 and gr.shape[2] + step0 >= 1 << 23:
        raise ValueError(f"mrphy_amd: nT + step0 = {gr.shape[2] + step0} must stay below 2**23 in fp32, where "
                         "step0 + t + 1/2 is exact; use fp64 for longer pulses")


def _vel_dt(vel, dt, loc):
    r"""``vel·dt`` `(N, *Nd, xyz)` in ``loc``'s dtype: the displacement per step, formed in fp64 and rounded once (``dt`` is
    `()` ⊻ `(N ⊻ 1,)`, right-padded).  Differentiable w.r.t. both."""
    dt = _host.pad_trailing(torch.as_tensor(dt).to(vel.device), vel.ndim)
    if vel.dtype == dt.dtype == loc.dtype:      # one multiplication in the data type is the fp64 product rounded once
        return (vel * dt).expand(loc.shape)
    return (vel.double() * dt.double()).to(loc.dtype).expand(loc.shape)


def _moving_bz(gr, w, step0):
    r"""What motion adds to the z component of ``rfgr2beff``'s field: ``(gr_t · w)(step0 + t + ½)`` `(N, *Nd, nT)` for
    ``gr`` `(N ⊻ 1, xyz, nT)` and the displacement per step ``w`` `(N, *Nd, xyz)`.  Plain torch, differentiable.  The product
    is formed on CONTIGUOUS copies: a batched product takes a view in whatever strides it has, and a permuted ``vel`` or a
    time slice of a longer ``gr`` rounds differently (``grad_gr``, one ulp) from contiguous tensors of the same values -- the
    tail of a split length then depended on the spelling of its operands (as :class:`_JoinAb`)."""
    nT = gr.shape[2]
    τ = (torch.arange(nT, dtype=torch.float64, device=w.device) + (step0 + 0.5)).to(w.dtype)
    z = torch.matmul(w.reshape(w.shape[0], -1, 3).contiguous(), gr.to(device=w.device, dtype=w.dtype).contiguous()) * τ
    return z.reshape(tuple(w.shape[:-1]) + (nT,))


@_host.half_via_float
def blochsim_rfgr_moving(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, vel: Tensor, *, step0: int = 0,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
) -> Tensor:
    r""":func:`blochsim_rfgr` for spins that move at constant velocity while the pulse plays (flowing blood; the
    reference declares ``SpinBolus`` for them, ``mobjs.py:968-973``, and gives it no body).  A spin that is at ``loc`` when
    step 0 begins sees, during step ``t`` of this call, the gradient at its midpoint position

        ``pos_t = loc + (vel·dt)·(step0 + t + ½)``,  ``Bz_t = gr_t · pos_t + Δf/γ_beff``

    -- exact for a piecewise-constant gradient: with ``rf = 0`` and no relaxation the transverse phase is
    ``-2π γ dt (m₀·loc + m₁·vel·dt)``, ``m₀ = Σ gr_t``, ``m₁ = Σ gr_t (step0 + t + ½)``.  ``Bxy`` is unchanged: a ``b1Map``
    is sampled at ``loc`` (the map does not move with the spin).

    ``vel``: `(N ⊻ 1, *Nd, xyz)`, "cm/s".  ``dt`` always sets the displacement ``vel·dt`` (formed in fp64, rounded once
    to the data type), with ``consts=`` too.  ``step0``: the steps played before this call; a pulse chained over
    several calls (``step0 = 0``, then ``step0 = n1`` on the rest) gives the single call's bits, because the position is
    formed in closed form at every step, never as a running sum.  ``nT + step0`` must stay below ``2**23`` in fp32.
    Everything else as :func:`blochsim_rfgr`; ``vel = 0`` gives its bits.

    Routes.  One transmit coil, and no gradient or gradients among ``Mi``, ``rf``, ``gr``: the fused kernels K2v / K2vb
    (``mrphy_blochsim_rfgr_moving_fwd`` / ``_bwd``), a pulse length that is not a multiple of 16 split into a fused part
    and a composed tail of at most 15 steps at ``step0 + n1``.  Everything else -- parallel transmit, fewer than 16 steps
    with a gradient, a gradient w.r.t. ``vel``, ``loc``, ``Δf``, ``b1Map``, ``γ_beff``, ``T1``, ``T2``, ``γ``, ``dt`` or
    ``consts`` -- is composed: ``rfgr2beff`` at the static ``loc``, the moving part ``(gr_t · vel·dt)(step0 + t + ½)`` added to
    its z component in torch, then ``blochsim``; autograd serves every operand there.  The composed forward equals the
    kernels' to tolerance, not bit for bit (it rounds ``gr·loc`` and the moving part separately).

    Out of scope: acceleration or arbitrary trajectories; the trajectory, signal and ``ab_rfgr`` forms for moving
    spins; gradients w.r.t. ``vel``, ``loc`` and the maps inside the kernel; parallel transmit inside the kernel; a binding
    of ``SpinBolus`` (there is no body to bind); a CPU path.
    """
    _check_moving(Mi, gr, loc, vel, step0)
    _host.require_device_tensor(Mi, 'Mi')
    _host.require_device_tensor(vel, 'vel')
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)

    def apply(p, step_consts, want_ckpt):
        with torch.no_grad():
            vdt = _vel_dt(vel.to(Mi.device), dt, loc).contiguous()
        return BlochSimRfGrMovingHIP.apply(Mi, rf, gr, p, vdt, step0, *step_consts, want_ckpt)

    return _bz_extended(
        Mi, rf, gr, loc, kw, fits=True, pulse_grad=False, other_grad=any(_requires_grad(x) for x in (vel, γ_beff, dt)),
        bz=lambda beff: _moving_bz(gr, _vel_dt(vel, dt, loc), step0),
        again=lambda M, sl, n0: blochsim_rfgr_moving(M, rf[:, :, sl], gr[:, :, sl], loc, vel, step0=step0 + n0, **kw),
        apply=apply)


class BlochSimRfGrShimHIP(Function):
    r"""``Mo = BlochSimRfGrShimHIP.apply(Mi, rf, gr, sh, pulse_on_spins, shMap, γ2πdt, E1, E2, E1_1, want_ckpt)``

    :class:`BlochSimRfGrHIP`'s plain call with ``nS`` extra Bz field channels: ``sh`` `(N ⊻ 1, nS, nT)` their waveforms,
    ``shMap`` `(N, nM, nS)` contiguous, of the kernels' dtype, their maps (``mrphy_blochsim_rfgr_shim_fwd`` / ``_bwd``, one
    transmit coil, ``nS`` within ``mrphy_blochsim_rfgr_shim_max_channels``).  Differentiable w.r.t. ``Mi``, ``rf``, ``gr`` and
    ``sh``; ``want_ckpt`` is the caller's decision (:func:`_decide_ext_route`), as there."""

    ARGS = ('Mi', 'rf', 'gr', 'sh', 'p', 'shMap', 'γ2πdt', 'E1', 'E2', 'E1_1', 'want_ckpt')

    @staticmethod
    def forward(ctx, Mi, rf, gr, sh, p, shMap, γ2πdt, E1, E2, E1_1, want_ckpt=False):
        sh_c = sh.detach().to(device=Mi.device, dtype=Mi.dtype).contiguous()
        sh_sn = sh_c.stride(0) if (sh_c.shape[0] == p.N and p.N > 1) else 0
        return _ext_forward(ctx, 'mrphy_blochsim_rfgr_shim_fwd', Mi, p, (γ2πdt, E1, E2, E1_1), want_ckpt,
                            dict(sh=sh_c, sh_sn=sh_sn, shMap=shMap, nS=sh_c.shape[1]), _likes(rf=rf, gr=gr, sh=sh))

    @staticmethod
    def backward(ctx, grad_Mo):
        return _ext_backward(ctx, BlochSimRfGrShimHIP, 'shim', grad_Mo)


def _check_shim(Mi, gr, loc, sh, shMap):
    r"""The argument checks of :func:`blochsim_rfgr_shim` that need neither the device nor the library."""
    N = loc.shape[0]
    if not isinstance(sh, Tensor) or sh.ndim != 3 or sh.shape[0] not in (1, N):
        raise ValueError(f"mrphy_amd: `sh` must be (N ⊻ 1, nS, nT) beside loc {tuple(loc.shape)}, got "
                         f"{tuple(sh.shape) if isinstance(sh, Tensor) else sh!r}")
    if not isinstance(shMap, Tensor) or shMap.ndim != loc.ndim or shMap.shape[0] not in (1, N) or \
            tuple(shMap.shape[1:-1]) != tuple(loc.shape[1:-1]):
        raise ValueError(f"mrphy_amd: `shMap` must be (N ⊻ 1, *Nd, nS) beside loc {tuple(loc.shape)}, got "
                         f"{tuple(shMap.shape) if isinstance(shMap, Tensor) else shMap!r}")
    if sh.shape[1] != shMap.shape[-1]:
        raise ValueError(f"mrphy_amd: `sh` has {sh.shape[1]} channels, `shMap` {shMap.shape[-1]}")
    if sh.shape[2] != gr.shape[2]:
        raise ValueError(f"mrphy_amd: `sh` has {sh.shape[2]} steps, `gr` {gr.shape[2]}")


def _shim_bz(sh, shMap):
    r"""What the channels add to the z component of ``rfgr2beff``'s field: ``Σ_k sh[k, t]·shMap[k]`` `(N, *Nd, nT)` for
    ``sh`` `(N ⊻ 1, nS, nT)` and ``shMap`` `(N ⊻ 1, *Nd, nS)`.  Plain torch, differentiable w.r.t. both.  On CONTIGUOUS copies,
    as :func:`_moving_bz`: a permuted ``shMap`` or a slice of a longer ``sh`` otherwise changes the last bit of the sum, and of
    ``grad_sh``."""
    lead, nS = tuple(shMap.shape[:-1]), shMap.shape[-1]
    z = torch.einsum('nmk,nkt->nmt', shMap.reshape(lead[0], -1, nS).contiguous(),
                     sh.to(device=shMap.device, dtype=shMap.dtype).contiguous())
    return z.reshape((z.shape[0],) + lead[1:] + (sh.shape[2],))


@_host.half_via_float
def blochsim_rfgr_shim(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, sh: Tensor, shMap: Tensor, *,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
) -> Tensor:
    r""":func:`blochsim_rfgr` with ``nS`` extra longitudinal field channels, each a waveform times a map:

        ``Bz_t = gr_t · loc + Σ_k sh[k, t]·shMap[k] + Δf/γ_beff``,  ``k < nS``

    -- fields whose shape in space is not linear and whose amplitude changes during the pulse: shim-array and local-B0-coil
    excitation, second-order and nonlinear gradient encoding, concomitant (Maxwell) fields (four channels,
    ``(x²+y²)``, ``z²``, ``xz``, ``yz``, whose waveforms the caller forms from ``gr``), gradient nonlinearity, eddy-current
    terms, and motion along given directions (``loc + Σ_k c_k(t)·d_k`` gives the channels ``gr_t·c_k(t)`` with maps
    ``d_k``; :func:`blochsim_rfgr_moving` is the three-channel special case).  ``Bxy`` is unchanged.

    ``sh``: `(N ⊻ 1, nS, nT)`, the channels' waveforms in any unit; ``shMap``: `(N ⊻ 1, *Nd, nS)`, Gauss per that unit at
    each spin.  Everything else as :func:`blochsim_rfgr`; ``nS = 0`` returns its result.  The kernels form ``Bz_t`` as
    :func:`blochsim_rfgr`'s value followed by one FMA per channel in ascending ``k``, so channels whose waveforms or maps
    are all zero leave its bits -- in ``Mo`` and in the gradients w.r.t. ``Mi``, ``rf``, ``gr`` -- and all-zero channels
    appended after the real ones change no bit of any result.  Both are statements about finite operands, up to the sign of
    a zero: ``0·inf`` is NaN (a build of a larger capacity multiplies the last channel's samples by zero maps), and
    ``fma(s, 0, -0.0)`` is ``+0.0``.

    Routes.  One transmit coil, ``nS`` within the capacity (``mrphy_blochsim_rfgr_shim_max_channels``: 8), and no gradient
    or gradients among ``Mi``, ``rf``, ``gr``, ``sh``: the fused kernels K2sh / K2shb (``mrphy_blochsim_rfgr_shim_fwd`` /
    ``_bwd``), a pulse length that is not a multiple of 16 split into a fused part and a composed tail of at most 15
    steps.  Everything else -- parallel transmit, more channels than the capacity, fewer than 16 steps with a gradient,
    a gradient w.r.t. ``shMap``, ``loc``, ``Δf``, ``b1Map``, ``γ_beff``, ``T1``, ``T2``, ``γ``, ``dt`` or ``consts`` -- is
    composed: ``rfgr2beff``, ``einsum(shMap, sh)`` added to its z component in torch, then ``blochsim``; autograd serves
    every operand there.  The composed route equals the kernels to tolerance, not bit for bit.

    Out of scope: gradients w.r.t. ``shMap`` and the other spin-side operands inside the kernel; parallel transmit
    inside the kernel; more channels than the capacity in one launch; the trajectory, signal and ``ab_rfgr`` forms with
    channels; a CPU path.
    """
    _check_shim(Mi, gr, loc, sh, shMap)
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    nS = sh.shape[1]
    if nS == 0:
        return blochsim_rfgr(Mi, rf, gr, loc, **kw)
    _host.require_device_tensor(Mi, 'Mi')
    _host.require_device_tensor(sh, 'sh')
    _host.require_device_tensor(shMap, 'shMap')
    cap = int(_lib.require_library().mrphy_blochsim_rfgr_shim_max_channels(_code(loc.dtype)))

    def apply(p, step_consts, want_ckpt):
        with torch.no_grad():                   # (N, *Nd, nS) contiguous in the kernels' dtype, as vdt of the moving call
            maps = shMap.to(device=Mi.device, dtype=Mi.dtype).expand((p.N,) + p.Nd + (nS,)).contiguous()
        return BlochSimRfGrShimHIP.apply(Mi, rf, gr, sh, p, maps, *step_consts, want_ckpt)

    return _bz_extended(
        Mi, rf, gr, loc, kw, fits=nS <= cap, pulse_grad=_requires_grad(sh),
        other_grad=any(_requires_grad(x) for x in (shMap, γ_beff)),
        bz=lambda beff: _shim_bz(sh, shMap.to(device=beff.device, dtype=beff.dtype)),
        again=lambda M, sl, n0: blochsim_rfgr_shim(M, rf[:, :, sl], gr[:, :, sl], loc, sh[:, :, sl], shMap, **kw),
        apply=apply)


# Forward mode (K2j).  The operands a direction may have a tangent of, and what each tangent's table is per spin / per step
# after the batch axis: the entry point's argument order.
_JVP_KEYS = ('Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'T1', 'T2')
_JVP_CONST_KEYS = ('E1', 'E2', 'E1_1')
_JVP_TABLES = ('Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'E1', 'E2', 'E1_1')


def _check_tangents(Mi, rf, gr, loc, tangents, Δf, b1Map, T1, T2, consts):
    r"""The argument checks of :func:`blochsim_rfgr_jvp` that need neither the device nor the library.  Returns ``(D,
    {key: tangent (D, *full)})``: the direction count and each given tangent as a view broadcast to the FULL shape of its
    operand -- ``(N, *Nd, xyz)`` for ``Mi`` and ``loc``, ``(N, xy, nT)`` / ``(N, xyz, nT)`` for ``rf`` / ``gr``, ``(N, *Nd, xy)``
    for ``b1Map``, ``(N, *Nd)`` for ``Δf`` and the constants -- whatever axes of the operand itself are broadcast."""
    if not isinstance(tangents, dict):
        raise ValueError(f"mrphy_amd: `tangents` must be a dict of tensors with a leading direction axis, got {tangents!r}")
    if rf.ndim == 4 and rf.shape[-1] != 1:
        raise NotImplementedError('parallel transmit')
    keys = _JVP_KEYS[:6] + (_JVP_CONST_KEYS if consts is not None else _JVP_KEYS[6:])
    given = {k: v for k, v in tangents.items() if v is not None}
    for k in given:
        if k in ('T1', 'T2') and consts is not None:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` together with `consts=`: its keys are {_JVP_CONST_KEYS}")
        if k not in keys:
            raise ValueError(f"mrphy_amd: `tangents` has an unknown key {k!r}; the keys are {keys}")
    if 'b1Map' in given and b1Map is None:
        raise ValueError("mrphy_amd: `tangents['b1Map']` without a `b1Map`")
    relax = consts.get('E1') is not None if consts is not None else T1 is not None
    for k in ('T1', 'T2') + _JVP_CONST_KEYS:
        if k in given and not relax:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` without relaxation (no `T1`, `T2` / `E1`, `E2`)")
    if not given:
        raise ValueError("mrphy_amd: `tangents` holds no direction")
    N, Nd, nT = loc.shape[0], tuple(loc.shape[1:-1]), gr.shape[2]
    spins = (N,) + Nd
    full = dict(Mi=spins + (3,), loc=spins + (3,), rf=(N, 2, nT), gr=(N, 3, nT), b1Map=spins + (2,))
    D, out = None, {}
    for k, v in given.items():
        if not isinstance(v, Tensor) or v.ndim < 1:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` must be a tensor with a leading direction axis, got {v!r}")
        if D is None:
            D = v.shape[0]
        if v.shape[0] != D or D < 1:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` has {v.shape[0]} directions, the others {D}")
        want = full.get(k, spins)
        t = v.float() if v.dtype in (torch.float16, torch.bfloat16) else v      # (half tensors are computed in fp32)
        if k in ('rf', 'b1Map') and t.ndim == len(want) + 2 and t.shape[-1] == 1:
            t = t[..., 0]                           # the coil axis of one coil
        if k not in full:                           # Δf and the constants: right-padded, as their operands are
            while t.ndim > 1 + len(want) and t.shape[-1] == 1:
                t = t[..., 0]
            if t.ndim <= 1 + len(want):
                t = _host.pad_trailing(t, 1 + len(want))
        if t.ndim != 1 + len(want) or any(a not in (1, b) for a, b in zip(t.shape[1:], want)):
            raise ValueError(f"mrphy_amd: `tangents['{k}']` {tuple(v.shape)} does not broadcast to (D, "
                             f"{', '.join(map(str, want))})")
        out[k] = t.expand((D,) + want)
    return D, out


def _relax_tangents(tan, kw, p):
    r"""``{'E1': dE1, 'E2': dE2, 'E1_1': dE1m1}`` `(D, N, *Nd)` from the tangents of ``T1, T2``: ``dE = E·dt/T²·dT`` with the
    ``E`` :func:`mrphy_amd.sims.relax_constants` gives, formed in fp64; ``E1 - 1`` moves as ``E1`` does."""
    from . import sims
    lead = 1 + len(p.Nd)
    _, E1, E2, _ = sims.relax_constants(kw['T1'], kw['T2'], kw['γ'], kw['dt'], lead + 2, p.device)
    out = {}
    for k, E, e in (('T1', E1, 'E1'), ('T2', E2, 'E2')):
        if k in tan:
            dev = tan[k].device
            spin = lambda x: _host.pad_trailing(torch.as_tensor(x).detach().to(dev).double(), lead + 2)[..., 0, 0]  # noqa: E731
            T = spin(kw[k])
            out[e] = tan[k].double() * (spin(E) * spin(kw['dt']) / (T * T))
    if 'E1' in out:
        out['E1_1'] = out['E1']
    return out


@_host.half_via_float
def blochsim_rfgr_jvp(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *, tangents: dict,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
):
    r"""``(Mo, dMo)``: :func:`blochsim_rfgr`'s ``Mo``, bit for bit, and its forward-mode tangents (Jacobian-vector
    products) along ``D`` directions, ``dMo`` `(D, N, *Nd, xyz)`, from one pass of the fused kernel K2j
    (``mrphy_blochsim_rfgr_jvp_fwd``) -- no checkpoints, no backward sweep, no finite differences.

    ``tangents``: a dict with keys among ``'Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'T1', 'T2'`` (with ``consts=``:
    ``'E1', 'E2', 'E1_1'`` in place of ``'T1', 'T2'``).  Each value has a leading direction axis ``D``, the same for all
    keys, followed by its operand's shape, where every broadcastable axis may be 1 (``drf`` `(D, 1, xy, nT)`; ``dT1``
    `(D, N, *Nd)` beside a 0-dim ``T1``).  A missing key or ``None`` is a zero tangent.  ``dMo[d]`` is the derivative of
    ``Mo`` along direction ``d``: for a per-spin quantity the Jacobian is block-diagonal per spin, so the direction "all
    ones" returns the whole sensitivity map (:func:`sensitivity_rfgr`); for ``rf``, ``gr`` it is ``J·v`` of a
    Gauss-Newton or CG step on the linearised excitation, the partner of the adjoint's ``Jᵀ·w``.

    The kernel shares each primal step among up to ``mrphy_blochsim_rfgr_jvp_max_dirs`` (4) directions in registers;
    more directions run in blocks of that many.  ``dMo[d]`` does not depend on which directions ride along: it has the
    bits of the call with direction ``d`` alone, scales exactly with powers of two and is exactly zero for zero tangents.
    The tangent arithmetic is plain FMAs in the data type in both fp32 modes.

    Neither output requires grad and the inputs are detached: reverse-over-forward differentiation is not offered.
    Not covered: tangents w.r.t. ``γ``, ``dt``, ``γ_beff``; parallel transmit (``NotImplementedError``: there is no
    composed forward-mode route to fall back to); ``torch.func.jvp`` / ``torch.autograd.forward_ad`` through the
    library's Functions; the trajectory and signal families (``A, B`` and the sequence: :func:`ab_rfgr_jvp`,
    :func:`ab_sequence_jvp`); a CPU path."""
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    assert (T1 is None) == (T2 is None)
    D, tan = _check_tangents(Mi, rf, gr, loc, tangents, Δf, b1Map, T1, T2, consts)
    _host.require_device_tensor(Mi, 'Mi')
    for k, v in tan.items():
        _host.require_device_tensor(v, f"tangents['{k}']")
    with torch.no_grad():
        if 'Δf' in tan and Δf is None:              # a tangent of the off-resonance at Δf = 0: the same field bits
            kw['Δf'] = torch.zeros((), dtype=loc.dtype, device=loc.device)
        f = _pulse_facts(rf, gr, loc, kw, Mi)
        p = f.p
        device, dtype = Mi.device, Mi.dtype
        assert p.device == device and p.dtype == dtype, "Mi and loc must share device and dtype"
        assert tuple(Mi.shape[:-1]) == (p.N,) + p.Nd and p.nC == 1
        lib = _lib.require_library()
        step_consts = _step_constants(kw, False, 1 + len(p.Nd) + 2, device)
        code, alive, cargs, _, _ = _forward_prep(lib, p, *step_consts, dtype, device, False)
        if consts is None:
            tan.update(_relax_tangents(tan, kw, p))
        tail = dict(Mi=(3,), loc=(3,), rf=(2, p.nT), gr=(3, p.nT), b1Map=(2,))
        tables = [None if k not in tan else
                  tan[k].detach().to(device=device, dtype=dtype)
                  .reshape((D, p.N) + ((p.nM,) + tail.get(k, ()) if k not in ('rf', 'gr') else tail[k])).contiguous()
                  for k in _JVP_TABLES]
        Mi_c = Mi.detach().contiguous()
        Mo = torch.empty_like(Mi_c)
        dMo = torch.empty((D, p.N) + p.Nd + (3,), dtype=dtype, device=device)
        cap = int(lib.mrphy_blochsim_rfgr_jvp_max_dirs(code))
        assert cap >= 1
        for d0 in range(0, D, cap):                 # blocks of the capacity; Mo from the first
            n = min(cap, D - d0)
            _launch('mrphy_blochsim_rfgr_jvp_fwd', device, code, Mi_c, *p.k0_args(), *cargs, n,
                    *(None if t is None else t[d0:d0 + n] for t in tables), Mo if d0 == 0 else None, dMo[d0:d0 + n],
                    p.N, p.nM, p.nT, p.nC)
        del alive
    return Mo, dMo


_SENSITIVITIES = ('Δf', 'rf', 'T1', 'T2')


def _sensitivity_directions(wrt, rf: Tensor, n_spin_axes: int) -> dict:
    r"""The ``tangents`` of :func:`sensitivity_rfgr`: one direction per entry of ``wrt``, in its order.  ``'rf'``: ``drf = rf``
    (the relative transmit scale); ``'Δf'``, ``'T1'``, ``'T2'``: ones, broadcast over the batch and the spins
    `(D, 1, *1)`.  Every table is zero in the directions of the other entries.  Plain torch, any device."""
    wrt = tuple(wrt)
    D = len(wrt)
    if D == 0 or len(set(wrt)) != D:
        raise ValueError(f"mrphy_amd: `wrt` must name each sensitivity once, got {wrt!r}")
    out = {}
    for i, k in enumerate(wrt):
        if k not in _SENSITIVITIES:
            raise ValueError(f"mrphy_amd: `wrt` has an unknown entry {k!r}; the entries are {_SENSITIVITIES}")
        if k == 'rf':
            t = torch.zeros((D,) + tuple(rf.shape), dtype=rf.dtype, device=rf.device)
            t[i] = rf.detach()
        else:
            t = torch.zeros((D,) + (1,) * n_spin_axes, dtype=rf.dtype, device=rf.device)
            t[i] = 1
        out[k] = t
    return out


def sensitivity_rfgr(Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *, wrt=_SENSITIVITIES, **kw):
    r"""``(Mo, {name: map})``: per-spin sensitivity maps `(N, *Nd, xyz)` of ``Mo``, one :func:`blochsim_rfgr_jvp` call with
    one direction per entry of ``wrt``: ``'Δf'``: ``∂Mo/∂Δf`` per Hz; ``'rf'``: ``∂Mo/∂ln s`` at ``s = 1`` for ``rf → s·rf``,
    the relative transmit scale (with or without a ``b1Map``); ``'T1'``, ``'T2'``: per second.  ``kw``: the keyword
    arguments of :func:`blochsim_rfgr` (``T1``, ``T2`` must be given for their maps; not ``consts=``)."""
    tangents = _sensitivity_directions(wrt, rf, loc.ndim - 1)
    Mo, dMo = blochsim_rfgr_jvp(Mi, rf, gr, loc, tangents=tangents, **kw)
    return Mo, {k: dMo[i] for i, k in enumerate(wrt)}


def _traj_ends(nT: int, every: int) -> list:
    r"""``s_j = min((j+1)·every, nT)``, j = 0 .. ceil(nT/every)-1: record j is M after ``s_j`` steps."""
    return [min(e, nT) for e in range(every, nT + every, every)]


def _traj_by_segments(Mi, rf, gr, loc, ends, kw):
    r"""The trajectory composed of :func:`blochsim_rfgr` calls, one per record segment, stacked time-major
    ``(len(ends), N, *Nd, 3)``.  Correct and differentiable in every case :func:`blochsim_rfgr` covers (gradients
    w.r.t. the spin-side maps, any coil count, any length), but it launches one simulation per record: the route of
    the cases the trajectory kernels do not cover, and the tests' yardstick."""
    out, M, t = [], Mi, 0
    for e in ends:
        M = blochsim_rfgr(M, rf[:, :, t:e], gr[:, :, t:e], loc, **kw)
        out.append(M)
        t = e
    return torch.stack(out)


@_host.half_via_float
def blochsim_rfgr_traj(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *, every: int = 1,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
) -> Tensor:
    r"""The magnetisation trajectory of :func:`blochsim_rfgr`: ``Mt`` `(N, *Nd, nRec, xyz)`, ``nRec =
    ceil(nT / every)``, where ``Mt[..., j, :]`` is M after step ``min((j+1)·every, nT) - 1`` -- so the last record
    is the final state, equal to ``blochsim_rfgr(...)`` bit for bit, and ``every = 1`` gives the reference's
    history ``Mhst`` (``sims.py:83``).  Differentiable w.r.t. ``Mi``, ``rf``, ``gr`` and the spin-side maps ``loc``,
    ``Δf``, ``b1Map`` and the constants ``T1``, ``T2``, ``γ``, ``dt`` (or the entries of ``consts``), ``γ_beff`` (one
    transmit coil: the fused adjoint, one launch whatever ``every`` is and whichever of them require grad); operands,
    dtypes, ``consts`` and the precision mode as :func:`blochsim_rfgr`.

    Layout: the result is a view ``.movedim(0, -2)`` of time-major storage `(nRec, N, *Nd, 3)` -- each record is
    one contiguous block, which the kernel writes with coalesced per-wave stores.  ``Mt.movedim(-2, 0)`` gives the
    contiguous tensor back; a loss that keeps that layout hands its gradient to the adjoint without a copy.

    The cases the fused adjoint does not cover (gradients w.r.t. ``loc``/``Δf``/``b1Map`` or the constants under parallel
    transmit or with fewer than 16 steps, a parallel-transmit gradient with more coils than
    ``mrphy_blochsim_rfgr_mc_max_coils()``, fp64 with more than 8 coils) run one
    :func:`blochsim_rfgr` per record segment and stack the results: correct and differentiable, slower.  A pulse
    length that is not a multiple of the 16-step checkpoint segment is split as :func:`blochsim_rfgr` splits it.
    """
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"mrphy_amd: `every` must be an int >= 1, got {every!r}")
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    route, out = _route(Mi, rf, gr, loc, every, kw)
    if route == 'fused':
        return out.movedim(0, -2)
    ends = _traj_ends(gr.shape[2], every)
    if route == 'split':
        # fused part of floor(nT/16)*16 steps + composed tail of <= 15: the part's records up to n1, its final state
        # (a record only if it falls on one) carries on into the tail's records
        n1 = out
        Mt1 = blochsim_rfgr_traj(Mi, rf[:, :, :n1], gr[:, :, :n1], loc, every=every, **kw).movedim(-2, 0)
        keep = sum(1 for e in ends if e <= n1)
        tail = [e - n1 for e in ends if e > n1]
        Mt2 = _traj_by_segments(Mt1[-1], rf[:, :, n1:], gr[:, :, n1:], loc, tail, kw)
        return torch.cat((Mt1[:keep], Mt2)).movedim(0, -2)
    return _traj_by_segments(Mi, rf, gr, loc, ends, kw).movedim(0, -2)


def _signal_of(Mt, rx):
    r"""The signal of a time-major trajectory ``Mt`` `(nRec, N, *Nd, xyz)` in torch: `(N, xy, nRec)`, or
    `(N, xy, nRec, nRx)` for ``rx`` `(N, *Nd, xy, nRx)` -- the complex product ``rx · (Mx + i My)`` (no conjugate) summed
    over ``*Nd``."""
    nRec, N, Nd = Mt.shape[0], Mt.shape[1], tuple(Mt.shape[2:-1])
    Mx, My = Mt[..., 0].reshape(nRec, N, -1), Mt[..., 1].reshape(nRec, N, -1)
    if rx is None:
        return torch.stack((Mx.sum(-1), My.sum(-1)), dim=0).permute(2, 0, 1)
    coils = rx.ndim == Mt.ndim
    r = rx.to(device=Mt.device, dtype=Mt.dtype).expand((N,) + Nd + tuple(rx.shape[1 + len(Nd):])) \
        .reshape(N, -1, 2, rx.shape[-1] if coils else 1)
    rr, ri = r[:, :, 0], r[:, :, 1]
    ein = lambda m, c: torch.einsum('jns,nsc->njc', m, c)  # noqa: E731
    sig = torch.stack((ein(Mx, rr) - ein(My, ri), ein(My, rr) + ein(Mx, ri)), dim=1)
    return sig if coils else sig[..., 0]


def _signal_composed(Mi, rf, gr, loc, every, rx, kw):
    r"""``(sig, Mo)`` as :func:`blochsim_rfgr_traj` followed by the product with ``rx`` and the sum over spins in torch:
    correct and differentiable wherever the trajectory is (parallel transmit, gradients w.r.t. the spin-side maps and
    w.r.t. ``rx``), at the price of the trajectory in memory -- the route of the cases the signal kernels do not cover,
    and the tests' yardstick."""
    Mt = blochsim_rfgr_traj(Mi, rf, gr, loc, every=every, **kw).movedim(-2, 0)
    return _signal_of(Mt, rx), Mt[-1]


@_host.half_via_float
def signal_rfgr(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *, every: int = 1, rx: Optional[Tensor] = None,
    return_Mo: bool = False,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
):
    r"""The signal a receive coil measures during the pulse of :func:`blochsim_rfgr`: the transverse magnetisation
    summed over the spins ``*Nd`` at the record steps of :func:`blochsim_rfgr_traj` (``nRec = ceil(nT / every)``,
    record ``j`` from M after step ``min((j+1)·every, nT) - 1``), weighted by the receive map ``rx`` as ``b1Map``
    weights ``rf`` (a complex product, no conjugate):

        ``sig[n, 0, j] = Σ_s rx_re·Mx − rx_im·My``,  ``sig[n, 1, j] = Σ_s rx_re·My + rx_im·Mx``.

    ``rx``: `(N, *Nd, xy)` or `(N, *Nd, xy, nRx)`, the layout of ``b1Map``; ``None`` is ``(1, 0)``, the plain sums of
    ``Mx`` and ``My``.  Returns ``sig`` `(N, xy, nRec)` -- `(N, xy, nRec, nRx)` when ``rx`` has a coil axis -- the layout
    of ``rf``; with ``return_Mo=True`` ``(sig, Mo)``, where ``Mo`` equals ``blochsim_rfgr(...)`` bit for bit, so a
    sequence can carry on from it.  Differentiable w.r.t. ``Mi``, ``rf``, ``gr`` and the constants ``T1``, ``T2``, ``γ``,
    ``dt`` (or the entries of ``consts``) through both outputs -- what a fit of T1 / T2 maps to a measured signal
    differentiates -- inside the signal kernels (``mrphy_signal_rfgr_consts_bwd``, every coil capacity); the other
    arguments, the dtypes, ``consts`` and the precision mode as :func:`blochsim_rfgr_traj`.  The reference has no
    counterpart (it forms ``Mhst`` and drops it, ``sims.py:83,131``): this is an extension.

    The sum is formed inside the kernel (K2s; the adjoint is a mode of K2b): no trajectory is written to memory, the
    order of summation is fixed, and the same inputs give the same bits.  Covered: one transmit coil with or without
    ``b1Map``, fp32 in both precision modes and fp64.  Several receive coils share one simulation, forward and
    adjoint: up to ``mrphy_signal_rfgr_max_rx`` coils (8) per launch, more in blocks of that many, and every coil's
    samples are the bits a call with that coil alone gives.  A gradient with a pulse length that is not a
    multiple of the 16-step checkpoint segment is split as :func:`blochsim_rfgr_traj` splits it.  Parallel transmit,
    gradients w.r.t. ``loc``/``Δf``/``b1Map``/``rx`` (and w.r.t. a ``γ_beff`` that multiplies a ``Δf``: a fold of
    ``Δf``'s) and fp64 above 8 coils compose :func:`blochsim_rfgr_traj` with
    the product and the sum in torch (with one transmit coil and map gradients that trajectory is one fused forward
    and one fused adjoint, not one simulation per record).  On a spin axis sharded over GPUs the signal is the sum of the ranks' signals
    (``dist.all_reduce_pulse_grads`` reduces tensors of this size).
    """
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"mrphy_amd: `every` must be an int >= 1, got {every!r}")
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    _host.require_device_tensor(Mi, 'Mi')
    if rx is not None:
        assert rx.ndim in (Mi.ndim, Mi.ndim + 1) and rx.shape[Mi.ndim - 1] == 2, "rx must be (N, *Nd, xy[, nRx])"
    route, out = _route(Mi, rf, gr, loc, every, kw, signal=True, rx=rx)
    if route == 'fused':
        sig, Mo = out
    elif route == 'split':
        # fused part of floor(nT/16)*16 steps + composed tail of <= 15: the part's records up to n1 (its own last record
        # is one of them only if it falls on one), its final state carries on into the tail's records
        n1, ends = out, _traj_ends(gr.shape[2], every)
        sig1, M1 = signal_rfgr(Mi, rf[:, :, :n1], gr[:, :, :n1], loc, every=every, rx=rx, return_Mo=True, **kw)
        keep = sum(1 for e in ends if e <= n1)
        Mt2 = _traj_by_segments(M1, rf[:, :, n1:], gr[:, :, n1:], loc, [e - n1 for e in ends if e > n1], kw)
        sig, Mo = torch.cat((sig1[:, :, :keep], _signal_of(Mt2, rx)), dim=2), Mt2[-1]
    else:
        sig, Mo = _signal_composed(Mi, rf, gr, loc, every, rx, kw)
    return (sig, Mo) if return_Mo else sig


def _ab_composed(rf, gr, loc, kw, cs, consts_grad):
    r"""``A, B`` as ``rfgr2beff`` followed by ``beff2ab``'s kernels on the step constants ``cs = (γ2πdt, E1, E2, E1_1)``
    (``E1 = None``: no relaxation, i.e. factors of one and a zero offset): differentiable w.r.t. every operand, at the
    price of ``Beff`` and, with gradients, the columns' history in memory -- the route of the cases the fused kernels do
    not cover, and the tests' yardstick."""
    from . import beffective
    beff = beffective.rfgr2beff(rf, gr, loc, Δf=kw['Δf'], b1Map=kw['b1Map'], γ=kw['γ_beff'], lazy=False)
    γ2πdt, E1, E2, E1_1 = cs
    if E1 is None:
        E1 = E2 = torch.ones((), dtype=beff.dtype, device=beff.device)
        E1_1 = torch.zeros((), dtype=beff.dtype, device=beff.device)
    return beffective._Beff2AB.apply(beff, γ2πdt, E1, E2, E1_1,
                                     torch.is_grad_enabled() and (beff.requires_grad or consts_grad))


@_host.half_via_float
def ab_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
):
    r"""Hargreaves' propagator of the whole pulse per spin, ``M_after = A @ M_before + B``
    (`doi:10.1002/mrm.1170 <https://doi.org/10.1002/mrm.1170>`_), from ``rf`` and ``gr``: what
    ``beffective.beff2ab(beffective.rfgr2beff(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ=γ_beff), ...)`` gives -- bit for bit
    with the same step constants -- without the intermediate ``Beff``.  It is what a loss on the elements of the
    rotation ``A`` needs (refocusing and inversion pulses), and what a steady state ``(I - A)^-1 B`` is composed from.

    Operands exactly as :func:`blochsim_rfgr` without ``Mi`` (shapes, broadcasting, dtypes, ``consts`` and the
    precision mode); ``T1 = T2 = None`` is no relaxation: ``A`` is then a pure rotation and ``B`` an exact zero.
    Returns ``A`` `(N, *Nd, xyz, 3)` and ``B`` `(N, *Nd, xyz)` in the dtype of ``loc``, as ``beffective.beff2ab`` lays
    them out; :func:`mrphy_amd.slowsims.blochsim_ab` consumes them unchanged.

    With one transmit coil (with or without ``b1Map``) one kernel carries the four columns of ``[I | 0]`` through the
    pulse: one field and one rotation per step for all four (K2ab).  Gradients w.r.t. ``rf`` and ``gr`` come from a
    fused adjoint (K2abb) over checkpoints of the four columns every 16 steps -- a quarter of ``Beff``'s bytes, where
    ``beff2ab``'s own adjoint keeps ``Beff`` and four times as much history -- deterministically: the same inputs give
    the same bits.  A pulse length that is not a multiple of 16 is split: the whole segments fused, the tail of at most
    15 steps through ``rfgr2beff`` + ``beff2ab``, joined as ``A = A_tail @ A_head``, ``B = A_tail @ B_head + B_tail``
    (:class:`_JoinAb`: its adjoint works on contiguous cotangents, so the bits do not depend on the strides of the loss's).
    Gradients w.r.t. ``loc``, ``Δf``, ``b1Map``, ``γ_beff`` and w.r.t. ``T1``, ``T2``, ``γ``, ``dt`` (or the entries of
    ``consts=``) come out of the same adjoint sweep, summed over time per spin in a fixed order (K2abb's MAPS and CONSTS
    builds: one forward, one adjoint call, still no ``Beff``); on the split route autograd adds the two parts'.  ``A, B``
    are the bits of the call that does not differentiate them.

    Parallel transmit -- ``rf`` `(N ⊻ 1, xy, nT, nCoils)` with a ``b1Map`` `(N ⊻ 1, *Nd ⊻ 1, xy, nCoils)`, 2 coils up to
    ``mrphy_ab_rfgr_mc_max_coils`` (8 in fp32, 4 in fp64) -- runs the same two kernels with the coil sum in the field
    (K2ab-mc) and a per-coil reduction over the spins (K2abb-mc): ``A, B`` still bit for bit ``beff2ab(rfgr2beff(.))``,
    ``grad_rf`` in the shape of ``rf`` and ``grad_gr`` deterministic, the same split of a ragged length, no ``Beff`` in
    memory.  What stays composed (``rfgr2beff`` + ``beff2ab``, HIP kernels as well, whose autograd serves every operand):
    more coils than that capacity; multi-coil ``rf`` without a ``b1Map`` (the coils add); gradients w.r.t. ``loc``, ``Δf``,
    ``b1Map``, ``γ_beff`` or ``T1``, ``T2``, ``γ``, ``dt`` under parallel transmit; any gradient of a pulse with fewer than 16
    steps.
    """
    _host.require_device_tensor(loc, 'loc')
    assert (T1 is None) == (T2 is None)
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    lib = _lib.require_library()
    f = _pulse_facts(rf, gr, loc, kw)
    p = f.p
    route, out = _decide_ab_route(
        nT=p.nT, seg=int(lib.mrphy_blochsim_rfgr_ck_every()), one_coil=f.one_coil, pulse_grad=f.pulse_grad,
        maps_grad=f.maps_grad, consts_grad=f.consts_grad, spin_fused=_ab_spin_fused(p.dtype, f.consts_grad),
        ptx_fused=b1Map is not None and 2 <= p.nC <= int(lib.mrphy_ab_rfgr_mc_max_coils(_code(p.dtype))))
    if route == 'split':
        # whole segments fused, the tail of <= 15 steps composed; the step map of the tail acts on the head's
        A1, B1 = ab_rfgr(rf[:, :, :out], gr[:, :, :out], loc, **kw)
        A2, B2 = ab_rfgr(rf[:, :, out:], gr[:, :, out:], loc, **kw)
        return _JoinAb.apply(A1, B1, A2, B2)
    cs = _step_constants(kw, f.consts_grad, 1 + len(p.Nd) + 2, p.device)
    if route == 'composed':
        return _ab_composed(rf, gr, loc, kw, cs, f.consts_grad)
    maps = (loc, Δf, b1Map, γ_beff if f.γb_grad else None) if f.maps_grad else ()
    return AbRfGrHIP.apply(rf, gr, p, *cs, out, *maps)


def _rest_operands(A, rest, T1, T2, Δf):
    r"""``(N, Nd, nM, code, keep, args)``: the arguments ``rest .. df_sm`` of the entry points that take Hargreaves'
    ``A`` `(N, *Nd, 3, 3)` and a rest period, and the tensors that keep their pointers alive."""
    device, dtype = A.device, A.dtype
    N, Nd = A.shape[0], tuple(A.shape[1:-2])
    d = None
    if rest is not None:
        d = rest.detach().to(device=device, dtype=dtype).reshape(-1).contiguous()
        assert d.numel() in (1, N), "rest must be () or (N ⊻ 1,)"
    consts, cargs = _const_operands(A, T1, T2, Δf)
    args = (None if d is None else d.data_ptr(), 1 if (d is not None and d.numel() == N and N > 1) else 0, *cargs)
    return N, Nd, prod(Nd), _code(dtype), (d,) + consts, args


def _const_operands(A, T1, T2, Δf):
    r"""``(keep, args)``: the arguments ``T1 .. df_sm`` of the same entry points, null where an operand is absent."""
    N, Nd = A.shape[0], tuple(A.shape[1:-2])
    keep = tuple(None if c is None else _host.Bcast(c.detach(), N, Nd, A.dtype, A.device) for c in (T1, T2, Δf))
    return keep, tuple(x for c in keep for x in (c.args if c else _host.NULL_BC))


def _state_operands(a, Mi, phase):
    r"""``(mi, cs)`` of the train family: ``Mi`` `(N ⊻ 1, nM ⊻ 1, 3)` in the data type and the fp64 table
    ``(cos φ, sin φ)`` `(N ⊻ 1, K, 2)`, formed here once per call with torch ops; ``None`` for an absent operand."""
    device, dtype = a.device, a.dtype
    Nd = tuple(a.shape[1:-2])
    mi = cs = None
    if Mi is not None:
        mi = Mi.detach().to(device=device, dtype=dtype)
        if all(d == 1 for d in mi.shape[1:-1]):
            mi = mi.reshape(mi.shape[0], 1, 3).contiguous()
        else:
            mi = mi.expand((mi.shape[0],) + Nd + (3,)).reshape(mi.shape[0], prod(Nd), 3).contiguous()
    if phase is not None:
        φ = phase.detach().to(device=device, dtype=torch.float64)
        cs = torch.stack((torch.cos(φ), torch.sin(φ)), dim=-1).contiguous()
    return mi, cs


def _over_n(x, N):
    r"""The element stride of ``x`` `(N ⊻ 1, …)` over the batch: 0 where it broadcasts."""
    return x.stride(0) if (x.shape[0] == N and N > 1) else 0


def _phase_args(cs, N):
    r"""The arguments ``cs, cs_sn`` of the train and the sequence family's entry points."""
    return (None, 0) if cs is None else (cs.data_ptr(), _over_n(cs, N))


def _state_args(mi, cs, N):
    r"""The arguments ``Mi .. cs_sn`` of the same entry points: pointers and element strides, 0 where it broadcasts."""
    return ((None, 0, 0) if mi is None else (mi.data_ptr(), _over_n(mi, N), 3 if mi.shape[1] > 1 else 0)) + \
        _phase_args(cs, N)


def _rest_table(a, rest, K):
    r"""``rs`` `(N ⊻ 1, K)` fp64 on the device, as the sequence family takes ``rest``: rounded to the data type (what
    ``ab_train`` hands its kernel) and widened, a duration that does not change written out over ``K``; ``None`` without
    a rest."""
    if rest is None:
        return None
    d = rest.detach().to(device=a.device, dtype=a.dtype).double()
    d = d.reshape(-1, 1) if d.ndim < 2 else d
    return d.expand(d.shape[0], K).contiguous()


def _sequence_args(a, rs, T1, T2, Δf, mi, cs, sched_dev, with_mi=True):
    r"""``(N, Nd, nM, code, keep, head, tail)`` of the sequence family's entry points for the bank ``a``
    `(P, N, *Nd, 3, 3)`: ``head`` is ``P, pulse`` and ``tail`` is ``rs .. cs_sn`` -- the rest table, the constants, the
    state --, ``with_mi=False``: without ``Mi, Mi_sn, Mi_sm`` (a steady state has none)."""
    N, Nd = a.shape[1], tuple(a.shape[2:-2])
    keep, consts = _const_operands(a[0], T1, T2, Δf)
    head = (a.shape[0], None if sched_dev is None else sched_dev.data_ptr())
    table = (None, 0) if rs is None else (rs.data_ptr(), _over_n(rs, N))
    state = _state_args(mi, cs, N) if with_mi else _phase_args(cs, N)
    return N, Nd, prod(Nd), _code(a.dtype), keep, head, table + consts + state


def _rx_operand(a, rx):
    r"""``(r, nRx)``: ``rx`` as `(N, nM, 2, nRx)` contiguous in the data type of ``a`` `(N, *Nd, 3, 3)``; ``(None, 1)``
    for ``None``."""
    if rx is None:
        return None, 1
    N, Nd = a.shape[0], tuple(a.shape[1:-2])
    r = rx.detach().to(device=a.device, dtype=a.dtype)
    nRx = r.shape[-1] if r.ndim == len(Nd) + 3 else 1
    r = r.expand((N,) + Nd + tuple(r.shape[1 + len(Nd):])).reshape(N, prod(Nd), 2, nRx).contiguous()
    return r, nRx


def _grad_wanted(*operands) -> bool:
    r"""Whether a backward may follow: grad mode is on and an operand requires grad."""
    return torch.is_grad_enabled() and any(isinstance(x, Tensor) and x.requires_grad for x in operands)


def _train_spins(A, B, bank=False):
    r"""``(N, Nd)`` of ``A, B`` as the train family takes them, ``bank``: with the bank axis in front; their shapes
    checked against each other."""
    lead = 'P, N' if bank else 'N'
    assert (not bank or A.ndim >= 4) and A.shape[-2:] == (3, 3) and tuple(B.shape) == tuple(A.shape[:-1]), \
        f"A {tuple(A.shape)} must be ({lead}, *Nd, 3, 3) and B {tuple(B.shape)} ({lead}, *Nd, 3)"
    return A.shape[int(bank)], tuple(A.shape[1 + int(bank):-2])


def _check_train_operands(A, B, N, Nd, Mi, rest, T1, T2, Δf):
    r"""What :func:`ab_train`, :func:`train_signal` and :func:`ab_sequence` require of their operands alike, once the
    number of repetitions is known."""
    _host.require_device_tensor(A, 'A')
    _host.require_device_tensor(B, 'B')
    assert A.dtype == B.dtype and A.device == B.device, "A and B must share dtype and device"
    assert (T1 is None) == (T2 is None)  # both or neither
    assert rest is not None or (T1 is None and Δf is None), "T1, T2, Δf describe the rest period: give `rest`"
    if Mi is not None:
        assert Mi.ndim == 2 + len(Nd) and Mi.shape[-1] == 3 and Mi.shape[0] in (1, N) and \
            all(m in (1, d) for m, d in zip(Mi.shape[1:-1], Nd)), \
            f"Mi {tuple(Mi.shape)} must be (N ⊻ 1, *Nd ⊻ 1, 3) for spins {(N,) + Nd}"


def _new_grads(empty, dtype, device, **shapes):
    r"""``{name: tensor}`` for the raw gradients of an ``A, B``-level adjoint: ``shapes[name]`` is the shape, or a false
    value for a gradient that is not wanted (``None``).  An ``empty`` problem launches nothing: its gradients are the
    zeros of a sum without terms."""
    new = torch.zeros if empty else torch.empty
    return {k: new(tuple(sh), dtype=dtype, device=device) if sh else None for k, sh in shapes.items()}


def _fold_rest_consts(gC, consts, need_c, N, Nd):
    r"""The gradients of the rest's operands ``consts`` (``rest, T1, T2, Δf``, or the last three) from the per-spin
    ``gC`` `(N, *Nd, len(consts))`: each summed over the axes its operand broadcasts along, ``None`` where ``need_c`` does
    not ask."""
    from . import sims
    return tuple(sims._reduce_to_const(gC[..., i], c, N, Nd).to(c.device) if want else None
                 for i, (c, want) in enumerate(zip(consts, need_c)))


def _fold_to_operand(g, x, acc=None):
    r"""``g`` summed over the axes ``x`` broadcasts along -- accumulated in ``acc``, by default in ``g``'s own dtype --, in
    ``x``'s shape and dtype and on its device."""
    if tuple(g.shape) != tuple(x.shape):
        g = (g if acc is None else g.to(acc)).sum_to_size(tuple(x.shape))
    return g.to(device=x.device, dtype=x.dtype)


def _fold_per_repetition(g, x):
    r"""The gradient of ``phase`` or ``rest`` from the kernel's per-spin ``g`` `(K, N, nM)`: summed in fp64 over the
    spins, then over what ``x`` shares -- ``x`` `(N ⊻ 1, K)`, or a duration `()` ⊻ `(N ⊻ 1,)` that the repetitions share too."""
    g = torch.sum(g, dim=-1, dtype=torch.float64).T      # (N, K)
    g = g.sum_to_size(tuple(x.shape)) if x.ndim == 2 else g.sum(1).sum_to_size(tuple(x.shape) or (1,))
    return g.reshape(x.shape).to(device=x.device, dtype=x.dtype)


class AbSteadyStateHIP(Function):
    r"""``Mss = AbSteadyStateHIP.apply(A, B, rest, T1, T2, Δf)`` -- see :func:`ab_steadystate`.  The backward
    (``mrphy_ab_steadystate_bwd``) recomputes ``Mss`` from the inputs: nothing else is saved."""

    @staticmethod
    def forward(ctx, A, B, rest, T1, T2, Δf):
        lib = _lib.require_library()
        device = A.device
        a, b = A.detach().contiguous(), B.detach().contiguous()
        N, Nd, nM, code, keep, args = _rest_operands(a, rest, T1, T2, Δf)
        Mss = torch.empty_like(b)
        with torch.cuda.device(device):
            rc = lib.mrphy_ab_steadystate_fwd(code, a.data_ptr(), b.data_ptr(), *args, Mss.data_ptr(), N, nM,
                                              _host.current_stream(device))
        _lib.check(rc, 'mrphy_ab_steadystate_fwd')
        del keep
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, b)
        ctx.consts = (rest, T1, T2, Δf)
        return Mss

    @staticmethod
    def backward(ctx, grad_Mss):
        need = ctx.needs_input_grad
        consts = ctx.consts
        need_c = [w and c is not None for w, c in zip(need[2:6], consts)]
        if grad_Mss is None or not (need[0] or need[1] or any(need_c)):
            return (None,) * 6
        lib = _lib.require_library()
        a, b = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, args = _rest_operands(a, *consts)
        g = grad_Mss.detach().to(dtype).contiguous()
        o = _new_grads(False, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape,
                       gC=any(need_c) and (N,) + Nd + (4,))
        with torch.cuda.device(device):
            rc = lib.mrphy_ab_steadystate_bwd(code, a.data_ptr(), b.data_ptr(), g.data_ptr(), *args, _ptr(o['gA']),
                                              _ptr(o['gB']), _ptr(o['gC']), N, nM, _host.current_stream(device))
        _lib.check(rc, 'mrphy_ab_steadystate_bwd')
        del keep
        return (o['gA'], o['gB']) + _fold_rest_consts(o['gC'], consts, need_c, N, Nd)


@_host.half_via_float
def ab_steadystate(
    A: Tensor, B: Tensor, *,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None
) -> Tensor:
    r"""The steady state of a sequence that repeats every period -- a rest of duration ``rest``
    (``sims.freeprec(M, rest, T1=T1, T2=T2, Δf=Δf)``: ``M⁻ = F M + f``), then the pulse ``M = A M⁻ + B`` -- from
    Hargreaves' ``A, B`` (:func:`ab_rfgr`, ``beffective.beff2ab``, or a product of several): the solution of

        ``(I - A F) Mss = A f + B``,

    one thread per spin (``mrphy_ab_steadystate_fwd``).  ``Mss`` is the state right AFTER the pulse;
    ``sims.freeprec(Mss, rest, ...)`` is the one before it.

    Usage:
        ``Mss = ab_steadystate(A, B, *, rest, T1, T2, Δf)``
    Inputs:
        - ``A``: `(N, *Nd, xyz, 3)`, ``B``: `(N, *Nd, xyz)`, as :func:`ab_rfgr` returns them.
    Optionals (shapes and broadcasting exactly as ``sims.freeprec``):
        - ``rest``: `()` ⊻ `(N ⊻ 1,)`, "Sec"; ``None`` = no rest period: ``Mss = (I - A)^-1 B`` of whatever period the
          caller composed (several pulses: ``A2 @ A1``, ``A2 @ B1 + B2``).  ``T1, T2, Δf`` must then be ``None`` too.
        - ``T1``, ``T2``: `()` ⊻ `(N ⊻ 1, *Nd ⊻ 1,)`, "Sec"; both ``None`` = no relaxation during the rest.
        - ``Δf``: `(N ⊻ 1, *Nd ⊻ 1,)`, "Hz"; ``None`` = no precession during the rest.
    Outputs:
        - ``Mss``: `(N, *Nd, xyz)`.

    Differentiable w.r.t. ``A``, ``B`` and whichever of ``rest, T1, T2, Δf`` require grad
    (``mrphy_ab_steadystate_bwd``: one transposed 3×3 solve per spin, ``Mss`` recomputed).  The kernels compute in
    fp64 whatever the data type and round the outputs once; in fp32 ``Mss`` still inherits the rounding of ``A``
    amplified by the condition number of ``I - A F``, about ``1 / (1 - exp(-rest/T1))``.  A singular system (no
    relaxation in the pulse nor in the rest) gives non-finite values: nothing synchronises with the host to detect it.
    """
    _host.require_device_tensor(A, 'A')
    _host.require_device_tensor(B, 'B')
    assert A.dtype == B.dtype and A.device == B.device, "A and B must share dtype and device"
    assert A.shape[-2:] == (3, 3) and tuple(B.shape) == tuple(A.shape[:-1]), \
        f"A {tuple(A.shape)} must be (N, *Nd, 3, 3) and B {tuple(B.shape)} (N, *Nd, 3)"
    assert (T1 is None) == (T2 is None)  # both or neither
    assert rest is not None or (T1 is None and Δf is None), "T1, T2, Δf describe the rest period: give `rest`"
    return AbSteadyStateHIP.apply(A, B, rest, T1, T2, Δf)


@_host.half_via_float
def steadystate_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
) -> Tensor:
    r"""The steady-state magnetisation of a pulse repeated every ``rest + nT·dt`` (bSSFP, SPGR / FLASH, any train of
    identical excitations), from ``rf`` and ``gr``:

        ``ab_steadystate(*ab_rfgr(rf, gr, loc, ...), rest=rest, T1=T1, T2=T2, Δf=Δf if Δf_rest is None else Δf_rest)``

    -- the closed form of what hundreds of repetitions of ``blochsim_rfgr`` + ``sims.freeprec`` converge to.

    Operands of the pulse exactly as :func:`ab_rfgr`; ``rest`` `()` ⊻ `(N ⊻ 1,)` "Sec", ``T1`` and ``T2`` are required
    (a steady state needs relaxation).  ``Δf_rest`` `(N ⊻ 1, *Nd ⊻ 1,)` "Hz" lets the rest period precess differently
    from the pulse: an RF phase increment or an unbalanced gradient moment per period, expressed in Hz; by default the
    rest precesses with ``Δf``.  Returns ``Mss`` `(N, *Nd, xyz)`: the state right AFTER the pulse;
    ``sims.freeprec(Mss, rest, T1=T1, T2=T2, Δf=...)`` is the one before it.

    Every route of :func:`ab_rfgr` (fused, split, composed) serves it, so gradients reach every operand ``ab_rfgr``
    serves -- with one transmit coil ``T1, T2, Δf, b1Map, loc`` as well as ``rf, gr`` through the fused adjoint, without
    ``Beff`` in memory; under parallel transmit (2 coils up to ``ab_rfgr``'s capacity, with their ``b1Map``) ``rf`` and ``gr``
    through its parallel-transmit adjoint, the spin-side operands through the composed route -- and ``rest, T1, T2, Δf`` /
    ``Δf_rest`` through the rest period as well: ``T1`` and ``T2``, shared
    by the pulse and the rest, receive the sum of both paths.  fp32: the solve itself runs in
    fp64, but ``Mss`` inherits the rounding of the fp32 ``A`` amplified by the conditioning of ``I - A F``, about
    ``1 / (1 - exp(-rest/T1))``: relative errors of a few 1e-6 at a factor of 50, 3e-5 at 170 -- for any fp32 route,
    the reference's operations included.
    """
    assert rest is not None and T1 is not None and T2 is not None, \
        "steadystate_rfgr: a steady state needs relaxation -- `rest`, `T1` and `T2` are required"
    A, B = ab_rfgr(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    return ab_steadystate(A, B, rest=rest, T1=T1, T2=T2, Δf=Δf if Δf_rest is None else Δf_rest)


class AbTrainHIP(Function):
    r"""``Mt = AbTrainHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, K)`` -- see :func:`ab_train`; ``Mt`` is time-major
    `(K, N, *Nd, xyz)`.  The backward (``mrphy_ab_train_bwd``) reads the states from ``Mt`` itself: besides the inputs,
    the output is all that is saved."""

    @staticmethod
    def forward(ctx, A, B, Mi, phase, rest, T1, T2, Δf, K):
        device = A.device
        a, b = A.detach().contiguous(), B.detach().contiguous()
        N, Nd, nM, code, keep, args = _rest_operands(a, rest, T1, T2, Δf)
        mi, cs = _state_operands(a, Mi, phase)
        Mt = torch.empty((K,) + tuple(b.shape), dtype=b.dtype, device=device)
        _launch('mrphy_ab_train_fwd', device, code, a, b, *args, *_state_args(mi, cs, N), Mt, N, nM, K)
        del keep
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, b, Mt, mi, cs)
        ctx.consts = (rest, T1, T2, Δf)
        ctx.state = (Mi, phase, K)
        return Mt

    @staticmethod
    def backward(ctx, grad_Mt):
        need = ctx.needs_input_grad
        consts = ctx.consts
        Mi, phase, K = ctx.state
        need_c = [w and c is not None for w, c in zip(need[4:8], consts)]
        need_mi, need_φ = need[2] and Mi is not None, need[3] and phase is not None
        if grad_Mt is None or not (need[0] or need[1] or need_mi or need_φ or any(need_c)):
            return (None,) * 9
        a, b, Mt, mi, cs = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, args = _rest_operands(a, *consts)
        g = grad_Mt.detach().to(dtype).contiguous()
        o = _new_grads(N * nM * K == 0, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape,
                       gC=any(need_c) and (N,) + Nd + (4,), gMi=need_mi and b.shape, gφ=need_φ and (K, N, nM))
        _launch('mrphy_ab_train_bwd', device, code, a, b, g, *args, *_state_args(mi, cs, N), Mt,
                *(o[k] for k in ('gA', 'gB', 'gC', 'gMi', 'gφ')), N, nM, K)
        del keep
        # grad_Mi is summed over those who share Mi in the data type; grad_phase over the spins in fp64
        return (o['gA'], o['gB'], _fold_to_operand(o['gMi'], Mi) if need_mi else None,
                _fold_per_repetition(o['gφ'], phase) if need_φ else None) + \
            _fold_rest_consts(o['gC'], consts, need_c, N, Nd) + (None,)


def _train_length(n, phase, N):
    r"""``K`` of :func:`ab_train` from ``n`` and ``phase``, checked as ``every`` of :func:`blochsim_rfgr_traj`."""
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n < 0):
        raise ValueError(f"mrphy_amd: `n` must be an int >= 0, got {n!r}")
    if phase is None:
        if n is None:
            raise ValueError("mrphy_amd: the number of repetitions is unknown: give `n`, `phase` (N ⊻ 1, K) or both")
        return n
    if phase.ndim != 2 or phase.shape[0] not in (1, N):
        raise ValueError(f"mrphy_amd: `phase` {tuple(phase.shape)} must be (N ⊻ 1, K) with N = {N}")
    if n is not None and n != phase.shape[1]:
        raise ValueError(f"mrphy_amd: `n` = {n} disagrees with `phase` {tuple(phase.shape)}: K = {phase.shape[1]}")
    return int(phase.shape[1])


@_host.half_via_float
def ab_train(
    A: Tensor, B: Tensor, *, n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None
) -> Tensor:
    r"""The transient of a sequence that repeats a pulse ``K`` times -- what :func:`ab_steadystate` is the limit of, and
    what exists where no one-period steady state does (RF spoiling).  Per spin, from ``M_0 = Mi``, for ``k = 0 … K-1``:

        ``M⁻ = F M_k + f``  -- the rest, ``sims.freeprec(M_k, rest, T1=T1, T2=T2, Δf=Δf)``, exactly as in
        :func:`ab_steadystate`;

        ``M_{k+1} = Rz(φ_k) [A Rz(-φ_k) M⁻ + B]``  -- the pulse ``A, B`` (:func:`ab_rfgr`, ``beffective.beff2ab``) played
        with its ``rf`` multiplied by ``exp(iφ_k)``; ``Rz(φ) = [[c, -s, 0], [s, c, 0], [0, 0, 1]]``.

    Record ``k`` is ``M_{k+1}``, the state right AFTER pulse ``k`` (as ``Mss`` of :func:`ab_steadystate`).

    Usage:
        ``Mt = ab_train(A, B, *, n, Mi, phase, rest, T1, T2, Δf)``
    Inputs:
        - ``A``: `(N, *Nd, xyz, 3)`, ``B``: `(N, *Nd, xyz)`, as :func:`ab_rfgr` returns them.
    Optionals:
        - ``n``: int, the number of repetitions ``K``; at least one of ``n`` and ``phase`` is given, and they agree.
        - ``Mi``: `(N ⊻ 1, *Nd ⊻ 1, xyz)`; ``None`` = ``(0, 0, 1)``.
        - ``phase``: `(N ⊻ 1, K)`, "rad"; ``None`` = all zeros.
        - ``rest``, ``T1``, ``T2``, ``Δf``: shapes, broadcasting and absences exactly as :func:`ab_steadystate`
          (``rest=None``: no rest period, ``T1, T2, Δf`` must then be ``None``; ``T1, T2`` both or neither).
    Outputs:
        - ``Mt``: `(N, *Nd, K, xyz)`.

    Layout: the result is a view ``.movedim(0, -2)`` of time-major storage `(K, N, *Nd, 3)`, as
    :func:`blochsim_rfgr_traj` returns its trajectory: each record is one contiguous block.  ``Mt.movedim(-2, 0)`` gives
    the contiguous tensor back; a loss that keeps that layout hands its gradient to the adjoint without a copy.

    One kernel, one thread per spin (``mrphy_ab_train_fwd``): all arithmetic in fp64 whatever the data type, the state
    carried in fp64 from one repetition to the next, each record rounded once on its store; ``cos φ, sin φ`` are formed
    once per call in fp64.  Differentiable w.r.t. ``A``, ``B``, ``Mi``, ``phase``, ``rest``, ``T1``, ``T2`` and ``Δf``
    (``mrphy_ab_train_bwd``: one sweep down the repetitions that reads the states from ``Mt`` itself -- nothing per
    repetition is kept besides the output --, deterministic).  In fp32 errors of ``A`` are amplified as in
    :func:`ab_steadystate`, by about ``1 / (1 - contraction)``.

    Out of scope: thinning the records (``every``); demodulating the records by ``-φ_k`` (one elementwise torch op on
    ``Mt``).  A flip angle or ``rest`` per repetition (the pulse is then not one ``A, B``) is :func:`ab_sequence`; the
    sum over the spins inside the kernel is :func:`train_signal`.
    """
    N, Nd = _train_spins(A, B)
    K = _train_length(n, phase, N)
    _check_train_operands(A, B, N, Nd, Mi, rest, T1, T2, Δf)
    return AbTrainHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, K).movedim(0, -2)


@_host.half_via_float
def train_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
) -> Tensor:
    r"""The magnetisation right after each of the first ``K`` repetitions of a pulse, the RF phase ``phase[:, k]``
    changing from one to the next (RF-spoiled gradient echo, phase-cycled bSSFP, the approach to a steady state), from
    ``rf`` and ``gr``:

        ``ab_train(*ab_rfgr(rf, gr, loc, ...), n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2,
        Δf=Δf if Δf_rest is None else Δf_rest)``

    built as :func:`steadystate_rfgr` is on :func:`ab_steadystate`.  Operands of the pulse exactly as :func:`ab_rfgr`,
    those of the train as :func:`ab_train`; ``Δf_rest`` as in :func:`steadystate_rfgr`.  Relaxation is not required: a
    transient exists without it.  Returns ``Mt`` `(N, *Nd, K, xyz)`, a ``.movedim(0, -2)`` view of time-major storage.

    Every route of :func:`ab_rfgr` (fused, split, composed; parallel transmit) serves it, so gradients reach every
    operand ``ab_rfgr`` serves, and ``Mi, phase, rest, T1, T2, Δf`` / ``Δf_rest`` through the train: ``T1`` and ``T2``,
    shared by the pulse and the rest, receive the sum of both paths.  Out of scope as in :func:`ab_train`.
    """
    A, B = ab_rfgr(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    return ab_train(A, B, n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2, Δf=Δf if Δf_rest is None else Δf_rest)


class AbSequenceHIP(Function):
    r"""``Mt = AbSequenceHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, K, sched)`` -- see :func:`ab_sequence`; ``A, B``
    carry the bank axis in front, ``sched`` is the checked schedule (an int32 CPU tensor `(K,)`, or ``None`` for all
    zeros), ``Mt`` is time-major `(K, N, *Nd, xyz)`.  The backward (``mrphy_ab_sequence_bwd``) reads the states from
    ``Mt`` itself, as :class:`AbTrainHIP`; its only scratch is the fp64 workspace of the bank's gradients."""

    @staticmethod
    def forward(ctx, A, B, Mi, phase, rest, T1, T2, Δf, K, sched):
        device = A.device
        a, b = A.detach().contiguous(), B.detach().contiguous()
        sched_dev = None if sched is None else sched.to(device)
        rs = _rest_table(a, rest, K)
        mi, cs = _state_operands(a[0], Mi, phase)
        N, Nd, nM, code, keep, head, tail = _sequence_args(a, rs, T1, T2, Δf, mi, cs, sched_dev)
        Mt = torch.empty((K,) + tuple(b.shape[1:]), dtype=b.dtype, device=device)
        _launch('mrphy_ab_sequence_fwd', device, code, a, b, *head, *tail, Mt, N, nM, K)
        del keep
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, b, Mt, mi, cs, rs, sched_dev)
        ctx.consts = (T1, T2, Δf)
        ctx.state = (Mi, phase, rest, K)
        return Mt

    @staticmethod
    def backward(ctx, grad_Mt):
        need = ctx.needs_input_grad
        consts = ctx.consts
        Mi, phase, rest, K = ctx.state
        need_c = [w and c is not None for w, c in zip(need[5:8], consts)]
        need_mi, need_φ, need_r = need[2] and Mi is not None, need[3] and phase is not None, need[4] and rest is not None
        if grad_Mt is None or not (need[0] or need[1] or need_mi or need_φ or need_r or any(need_c)):
            return (None,) * 10
        lib = _lib.require_library()
        a, b, Mt, mi, cs, rs, sched_dev = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, head, tail = _sequence_args(a, rs, *consts, mi, cs, sched_dev)
        g = grad_Mt.detach().to(dtype).contiguous()
        o = _new_grads(N * nM * K == 0, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape,
                       gC=any(need_c) and (N,) + Nd + (3,), gr=need_r and (K, N, nM), gMi=need_mi and b.shape[1:],
                       gφ=need_φ and (K, N, nM))
        nbytes = int(lib.mrphy_ab_sequence_bwd_workspace(code, a.shape[0], N, nM)) if (need[0] or need[1]) else 0
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=device) if nbytes else None
        _launch('mrphy_ab_sequence_bwd', device, code, a, b, *head, g, *tail, Mt,
                *(o[k] for k in ('gA', 'gB', 'gC', 'gr', 'gMi', 'gφ')), work, nbytes, N, nM, K)
        del keep, work
        # grad_Mi is summed over those who share Mi in the data type; grad_phase and grad_rest over the spins in fp64
        return (o['gA'], o['gB'], _fold_to_operand(o['gMi'], Mi) if need_mi else None,
                _fold_per_repetition(o['gφ'], phase) if need_φ else None,
                _fold_per_repetition(o['gr'], rest) if need_r else None) + \
            _fold_rest_consts(o['gC'], consts, need_c, N, Nd) + (None, None)


def _sequence_schedule(pulse, P):
    r"""``pulse`` of :func:`ab_sequence` checked on the host: an int32 CPU tensor `(K,)`, or ``None`` (all zeros)."""
    if pulse is None:
        if P != 1:
            raise ValueError(f"mrphy_amd: `pulse` is required with a bank of P = {P} pulses: which one does repetition 0 play?")
        return None
    if isinstance(pulse, Tensor):
        if pulse.device.type != 'cpu':
            raise ValueError(f"mrphy_amd: `pulse` is a host-side schedule: a CPU tensor, got one on {pulse.device}")
        if pulse.ndim != 1:
            raise ValueError(f"mrphy_amd: `pulse` {tuple(pulse.shape)} must be (K,)")
        if pulse.dtype.is_floating_point or pulse.dtype.is_complex or pulse.dtype == torch.bool:
            raise ValueError(f"mrphy_amd: `pulse` must hold integers: repetition 0"
                             f"{f' is {pulse[0].item()!r}' if pulse.numel() else ''} of dtype {pulse.dtype}")
        sched = pulse.detach().to(torch.int64)
    else:
        import numbers
        entries = list(pulse)
        for k, x in enumerate(entries):
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise ValueError(f"mrphy_amd: `pulse` must hold integers: repetition {k} is {x!r}")
        sched = torch.tensor([int(x) for x in entries], dtype=torch.int64)
    bad = ((sched < 0) | (sched >= P)).nonzero()
    if bad.numel():
        k = int(bad[0])
        raise ValueError(f"mrphy_amd: repetition {k} plays `pulse` = {int(sched[k])}, outside the bank [0, {P})")
    return sched.to(torch.int32).contiguous()


def _sequence_length(n, sched, phase, N):
    r"""``K`` of :func:`ab_sequence` from ``n``, ``pulse`` and ``phase``, in the style of :func:`_train_length`."""
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n < 0):
        raise ValueError(f"mrphy_amd: `n` must be an int >= 0, got {n!r}")
    if phase is not None and (phase.ndim != 2 or phase.shape[0] not in (1, N)):
        raise ValueError(f"mrphy_amd: `phase` {tuple(phase.shape)} must be (N ⊻ 1, K) with N = {N}")
    given = [(f"`{name}`{what}", k) for name, what, k in (
        ('n', '' if n is None else f' = {n}', n),
        ('pulse', '' if sched is None else f' ({sched.numel()},)', None if sched is None else int(sched.numel())),
        ('phase', '' if phase is None else f' {tuple(phase.shape)}', None if phase is None else int(phase.shape[1])))
        if k is not None]
    if not given:
        raise ValueError("mrphy_amd: the number of repetitions is unknown: give `n`, `pulse` (K,), `phase` (N ⊻ 1, K) "
                         "or several")
    for what, k in given[1:]:
        if k != given[0][1]:
            raise ValueError(f"mrphy_amd: {given[0][0]} disagrees with {what}: K = {given[0][1]} or {k}?")
    return given[0][1]


def _period_length(n, sched, phase, N):
    r"""``K`` of :func:`sequence_steadystate`: :func:`_sequence_length`, and a period needs a repetition."""
    K = _sequence_length(n, sched, phase, N)
    if K == 0:
        raise ValueError("mrphy_amd: a period needs a repetition: K = 0")
    return K


def _check_rx(rx, N, Nd, nb):
    r"""``rx`` of :func:`train_signal` and :func:`sequence_signal` against the spins; ``nb``: the dimensions of one
    entry's ``B`` `(N, *Nd, xyz)`."""
    if rx is not None:
        if rx.ndim not in (nb, nb + 1) or rx.shape[0] not in (1, N) or \
                tuple(rx.shape[1:nb]) != Nd + (2,) or (rx.ndim == nb + 1 and rx.shape[-1] < 1):
            raise ValueError(f"mrphy_amd: `rx` {tuple(rx.shape)} must be (N ⊻ 1, *Nd, xy) or (N ⊻ 1, *Nd, xy, nRx) "
                             f"for spins {(N,) + Nd}")


def _sequence_operands(A, B, pulse, n, phase, rest, T1, T2, Δf, Mi, period=False, rx=None):
    r"""``(N, Nd, sched, K)`` of :func:`ab_sequence`, :func:`sequence_signal` and :func:`sequence_steadystate`
    (``period``: ``K = 0`` is refused), every operand checked in the order the three document: the bank's shapes, the
    schedule, the length, ``rest``, ``rx`` where there is one, then what :func:`_check_train_operands` requires."""
    N, Nd, sched, K = _sequence_shapes(A, B, pulse, n, phase, rest, period, rx)
    _check_train_operands(A, B, N, Nd, Mi, rest, T1, T2, Δf)
    return N, Nd, sched, K


def _sequence_shapes(A, B, pulse, n, phase, rest, period=False, rx=None):
    r"""The part of :func:`_sequence_operands` that looks at shapes and the schedule only, not at devices."""
    N, Nd = _train_spins(A, B, bank=True)
    sched = _sequence_schedule(pulse, A.shape[0])
    K = (_period_length if period else _sequence_length)(n, sched, phase, N)
    if rest is not None and (rest.ndim > 2 or (rest.ndim == 1 and rest.shape[0] not in (1, N)) or
                             (rest.ndim == 2 and (rest.shape[0] not in (1, N) or rest.shape[1] != K))):
        raise ValueError(f"mrphy_amd: `rest` {tuple(rest.shape)} must be (), (N ⊻ 1,) or (N ⊻ 1, K) with N = {N}, K = {K}")
    _check_rx(rx, N, Nd, B.ndim - 1)
    return N, Nd, sched, K


@_host.half_via_float
def ab_sequence(
    A: Tensor, B: Tensor, *, pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None,
    phase: Optional[Tensor] = None, rest: Optional[Tensor] = None, T1: Optional[Tensor] = None,
    T2: Optional[Tensor] = None, Δf: Optional[Tensor] = None
) -> Tensor:
    r"""The transient of a sequence whose repetitions differ: repetition ``k`` plays pulse ``pulse[k]`` of a bank after
    a rest of its own duration -- MR fingerprinting, an inversion- or T2-prepared train, variable flip angles, dummy or
    catalysing pulses before a train.  Per spin, from ``M_0 = Mi``, for ``k = 0 … K-1``:

        ``M⁻ = F_k M_k + f_k``  -- ``sims.freeprec(M_k, rest_k, T1=T1, T2=T2, Δf=Δf)``, exactly as in :func:`ab_train`;

        ``M_{k+1} = Rz(φ_k) [A_p Rz(-φ_k) M⁻ + B_p]``, ``p = pulse[k]``.

    Record ``k`` is ``M_{k+1}``.  With ``P = 1`` and one ``rest`` it is :func:`ab_train`, bit for bit.

    Usage:
        ``Mt = ab_sequence(A, B, *, pulse, n, Mi, phase, rest, T1, T2, Δf)``
    Inputs:
        - ``A``: `(P, N, *Nd, xyz, 3)`, ``B``: `(P, N, *Nd, xyz)`: a bank of ``P ≥ 1`` pulses, the bank axis in front --
          :func:`ab_rfgr`'s output for a batch of ``P·N`` entries is one by ``.unflatten(0, (P, N))``, a view.
    Optionals:
        - ``pulse``: a sequence of ints or an integer CPU tensor `(K,)`, each in ``[0, P)``: a host-side schedule, one for
          all batch entries, checked before anything else and copied to the device once per call.  ``None`` = all
          zeros, with ``P == 1`` only.
        - ``n``: int; ``K`` comes from ``n``, ``pulse`` and ``phase``: at least one is given, and all given agree.
        - ``Mi``: `(N ⊻ 1, *Nd ⊻ 1, xyz)`; ``None`` = ``(0, 0, 1)``.  ``phase``: `(N ⊻ 1, K)`, "rad"; ``None`` = zeros.
        - ``rest``: `()` ⊻ `(N ⊻ 1,)`, "Sec", the same before every pulse as in :func:`ab_train`; or `(N ⊻ 1, K)`, one
          duration per repetition.  A 1-d tensor always has the first meaning, also when ``N == K``.  ``rest_k = 0`` is
          legal: no rest before pulse ``k``.  ``None``: no rest period at all.
        - ``T1``, ``T2``, ``Δf``: shapes, broadcasting and absences exactly as :func:`ab_train`.
    Outputs:
        - ``Mt``: `(N, *Nd, K, xyz)`, the ``.movedim(0, -2)`` view of time-major storage, as :func:`ab_train` returns.

    One kernel whatever the schedule (Ksq, ``mrphy_ab_sequence_fwd``): :func:`ab_train`'s repetition in fp64, the lane
    reloading ``A_p, B_p`` when ``pulse[k]`` changes and re-forming the rest's constants when ``rest_k`` changes; a run of
    equal repetitions costs what :func:`ab_train` costs.  Differentiable w.r.t. ``A``, ``B`` (the whole bank: an entry the
    schedule never plays gets an exactly-zero gradient), ``Mi``, ``phase``, ``rest`` (in the form given), ``T1``, ``T2``
    and ``Δf`` (Ksqb, ``mrphy_ab_sequence_bwd``: one sweep down the repetitions on the records themselves; the bank's
    gradients go through an fp64 workspace of ``P·12`` numbers per spin, nothing of size ``K × spins`` is kept besides
    the output), deterministic.

    Out of scope: a schedule per batch entry; thinning the records; reading out at an echo time after the pulse
    (``sims.freeprec`` on the records, an elementwise operation); a CPU path.  The received signal of such a sequence
    summed inside the kernel is :func:`sequence_signal`; the steady state of the ``K`` repetitions played as one period
    is :func:`sequence_steadystate`.
    """
    *_, sched, K = _sequence_operands(A, B, pulse, n, phase, rest, T1, T2, Δf, Mi)
    return AbSequenceHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, K, sched).movedim(0, -2)


def _sequence_bank(rf, gr, loc, pulse, *, Δf, b1Map, γ_beff, T1, T2, γ, dt, consts):
    r"""``(A, B, sched)`` of :func:`sequence_rfgr` and its siblings: the schedule checked on the host before any work on
    the device, then ONE :func:`ab_rfgr` call on the batch ``P·N`` whose ``A, B`` are viewed as the bank
    `(P, N, *Nd, …)`."""
    assert rf.ndim in (4, 5) and gr.ndim == 4 and gr.shape[0] in (1, rf.shape[0]) and gr.shape[1] == rf.shape[1], \
        f"rf {tuple(rf.shape)} must be (P, N, xy, nT[, nCoils]) and gr {tuple(gr.shape)} (P ⊻ 1, N, xyz, nT)"
    P, N = rf.shape[0], rf.shape[1]
    sched = _sequence_schedule(pulse, P)          # before any work on the device
    over = lambda x: x.expand((P,) + tuple(x.shape)).flatten(0, 1)  # noqa: E731
    # a spin-side operand: repeated over the bank where it has the batch axis, left to broadcast where it has not
    side = lambda x: over(x) if (isinstance(x, Tensor) and x.ndim >= 1 and x.shape[0] == N and N > 1) else x  # noqa: E731
    A, B = ab_rfgr(rf.flatten(0, 1), over(gr[0]) if gr.shape[0] == 1 else gr.flatten(0, 1), over(loc), Δf=side(Δf),
                   b1Map=side(b1Map), γ_beff=side(γ_beff), T1=side(T1), T2=side(T2), γ=side(γ), dt=side(dt),
                   consts=None if consts is None else {k: side(v) for k, v in consts.items()})
    return A.unflatten(0, (P, N)), B.unflatten(0, (P, N)), sched


@_host.half_via_float
def sequence_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
) -> Tensor:
    r"""The magnetisation right after each repetition of a sequence that plays a bank of pulses by a schedule, from
    ``rf`` `(P, N, xy, nT[, nCoils])` and ``gr`` `(P ⊻ 1, N, xyz, nT)`: ONE :func:`ab_rfgr` call on the batch ``P·N``
    (``rf.flatten(0, 1)``, the spin-side operands ``loc, Δf, b1Map, T1, T2, γ, dt, γ_beff`` / ``consts`` repeated over
    ``P``), its ``A, B`` viewed as the bank, then :func:`ab_sequence` -- built as :func:`train_rfgr` is on
    :func:`ab_train`.  Operands of the pulses as :func:`ab_rfgr`, those of the train as :func:`ab_sequence`; ``Δf_rest``
    as in :func:`steadystate_rfgr`.  Returns ``Mt`` `(N, *Nd, K, xyz)`.

    Every route of :func:`ab_rfgr` (fused, split, composed; parallel transmit) serves it, so gradients reach ``rf``, ``gr``
    and every operand ``ab_rfgr`` differentiates -- a flip-angle schedule ``rf = s[:, None, None, None] * rf0`` gets
    ``∂/∂s`` by autograd -- and ``Mi, phase, rest, T1, T2, Δf`` / ``Δf_rest`` through the train: ``T1`` and ``T2`` receive the
    sum of the pulses' and the rests' paths.  :func:`ab_rfgr`'s limit on the batch is inherited: ``P·N ≤ 65535``.  Out of
    scope as in :func:`ab_sequence`; the signal of the sequence is :func:`sequence_signal_rfgr`.
    """
    A, B, sched = _sequence_bank(rf, gr, loc, pulse, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt,
                                 consts=consts)
    return ab_sequence(A, B, pulse=sched, n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2,
                       Δf=Δf if Δf_rest is None else Δf_rest)


# Forward mode of the sequence (Ksqj).  The operands a direction may have a tangent of, in the entry point's order.
_SEQ_JVP_KEYS = ('A', 'B', 'Mi', 'T1', 'T2', 'Δf', 'phase', 'rest')


def _given_tangents(tangents, keys):
    r"""``(D, {key: tangent})`` of a ``tangents`` dict: the entries that are not ``None``, each a tensor with the same
    leading direction axis ``D >= 1``, half tensors widened to fp32; a key outside ``keys`` is a ``ValueError``."""
    if not isinstance(tangents, dict):
        raise ValueError(f"mrphy_amd: `tangents` must be a dict of tensors with a leading direction axis, got {tangents!r}")
    given = {k: v for k, v in tangents.items() if v is not None}
    for k in given:
        if k not in keys:
            raise ValueError(f"mrphy_amd: `tangents` has an unknown key {k!r}; the keys are {tuple(keys)}")
    if not given:
        raise ValueError("mrphy_amd: `tangents` holds no direction")
    D = None
    for k, v in given.items():
        if not isinstance(v, Tensor) or v.ndim < 1:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` must be a tensor with a leading direction axis, got {v!r}")
        D = v.shape[0] if D is None else D
        if v.shape[0] != D or D < 1:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` has {v.shape[0]} directions, the others {D}")
        if v.dtype in (torch.float16, torch.bfloat16):
            given[k] = v.float()
    return D, given


def _check_sequence_tangents(tangents, P, N, Nd, K, rest, T1, Δf):
    r"""The argument checks of :func:`ab_sequence_jvp` that need neither the device nor the library.  Returns ``(D,
    {key: tangent})`` with each given tangent as a view broadcast to ``(D, P, N, *Nd, 3, 3)`` / ``(D, P, N, *Nd, 3)`` for
    ``A`` / ``B``, ``(D, N, *Nd, 3)`` for ``Mi``, ``(D, N, *Nd)`` for ``T1, T2, Δf`` and ``(D, N ⊻ 1, K)`` for ``phase`` and
    ``rest`` (a duration that the repetitions share written out over ``K``)."""
    D, given = _given_tangents(tangents, _SEQ_JVP_KEYS)
    if 'rest' in given and rest is None:
        raise ValueError("mrphy_amd: `tangents['rest']` without a `rest`")
    for k in ('T1', 'T2'):
        if k in given and T1 is None:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` without `T1`, `T2`")
    if 'Δf' in given and rest is None:
        raise ValueError("mrphy_amd: `tangents['Δf']` without a `rest`: nothing precesses")
    spins = (N,) + Nd
    full = dict(A=(P,) + spins + (3, 3), B=(P,) + spins + (3,), Mi=spins + (3,), T1=spins, T2=spins, Δf=spins)
    out = {}
    for k, t in given.items():
        shape = tuple(t.shape)
        if k in ('phase', 'rest'):
            if k == 'rest' and t.ndim <= 2:               # (D,) ⊻ (D, N ⊻ 1): one duration for all repetitions
                t = t.reshape(D, -1, 1)
            ok = t.ndim == 3 and t.shape[1] in (1, N) and (t.shape[2] == K or (k == 'rest' and t.shape[2] == 1))
            want = ('N ⊻ 1', 'K')
            if ok:
                t = t.expand(D, t.shape[1], K)
        else:
            want = full[k]
            if k in ('T1', 'T2', 'Δf'):                   # right-padded, as their operands are
                while t.ndim > 1 + len(want) and t.shape[-1] == 1:
                    t = t[..., 0]
                if t.ndim <= 1 + len(want):
                    t = _host.pad_trailing(t, 1 + len(want))
            ok = t.ndim == 1 + len(want) and all(a in (1, b) for a, b in zip(t.shape[1:], want))
            if ok:
                t = t.expand((D,) + want)
        if not ok:
            raise ValueError(f"mrphy_amd: `tangents['{k}']` {shape} does not broadcast to (D, {', '.join(map(str, want))})")
        out[k] = t
    return D, out


@_host.half_via_float
def ab_sequence_jvp(
    A: Tensor, B: Tensor, *, tangents: dict, pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None,
    phase: Optional[Tensor] = None, rest: Optional[Tensor] = None, T1: Optional[Tensor] = None,
    T2: Optional[Tensor] = None, Δf: Optional[Tensor] = None
):
    r"""``(Mt, dMt)``: :func:`ab_sequence`'s ``Mt`` `(N, *Nd, K, xyz)`, bit for bit, and its forward-mode tangents
    (Jacobian-vector products) along ``D`` directions, ``dMt`` `(D, N, *Nd, K, xyz)`: the derivative of every record of
    the transient, from one pass of one kernel (Ksqj, ``mrphy_ab_sequence_jvp_fwd``) -- no backward sweep, no finite
    differences.  Operands exactly as :func:`ab_sequence`.

    ``tangents``: a dict with keys among ``'A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'Δf'``, as in
    :func:`blochsim_rfgr_jvp`: each value has a leading direction axis ``D``, the same for all keys, followed by its
    operand's shape in any form the operand may take, where every broadcastable axis may be 1 (``dT1`` `(D, N, *Nd)`
    beside a 0-dim ``T1``; ``drest`` `(D,)`, `(D, N ⊻ 1)` or `(D, N ⊻ 1, K)`).  A missing key or ``None`` is a zero
    tangent.  ``Mi`` and ``phase`` may have a tangent without being given (their absences are the values ``(0, 0, 1)`` and
    ``0``), ``Δf`` may while ``rest`` is given (it counts as 0); ``rest``, ``T1``, ``T2`` need their operand.  For a per-spin
    quantity the Jacobian is block-diagonal per spin, so the direction "all ones" returns the whole sensitivity map
    ``∂M_k/∂T1`` of every spin and repetition -- what a Cramér-Rao analysis of a schedule starts from, where reverse mode
    needs ``3·K`` backward passes --, and ``dMt`` along a direction ``v`` is the ``J·v`` of a Gauss-Newton step, the
    partner of the adjoint's ``Jᵀ·w``.

    The kernel carries up to ``mrphy_ab_sequence_jvp_max_dirs`` (4) directions beside the state; more run in blocks of
    that many, ``Mt`` from the first.  The tangents of the rest's ``cos, sin, E1, E2`` are products of those numbers: no
    transcendental function is called for a tangent.  ``dMt[d]`` has the bits of the call with direction ``d`` alone,
    scales exactly with powers of two, is exactly zero for zero tangents, and a tangent on a bank entry the schedule
    never plays contributes exact zeros.  fp64 inside, one rounding per record, as :func:`ab_sequence`.

    The argument checks come in this order: the bank's shapes, the schedule, the length and ``rest`` as
    :func:`ab_sequence` makes them, the tangents (``ValueError``: an unknown key, unequal ``D``, no direction, a shape that
    does not broadcast, a tangent whose operand is missing), then devices and dtypes.  Neither output requires grad and
    the inputs are detached: reverse-over-forward is not offered.  Not covered: ``torch.func.jvp`` /
    ``torch.autograd.forward_ad`` through the library's Functions; tangents of :func:`sequence_signal`,
    :func:`sequence_steadystate`, :func:`ab_steadystate`; a schedule per batch entry; a CPU path."""
    N, Nd, sched, K = _sequence_shapes(A, B, pulse, n, phase, rest)
    D, tan = _check_sequence_tangents(tangents, A.shape[0], N, Nd, K, rest, T1, Δf)
    _check_train_operands(A, B, N, Nd, Mi, rest, T1, T2, Δf)
    for k, v in tan.items():
        _host.require_device_tensor(v, f"tangents['{k}']")
    with torch.no_grad():
        device, dtype = A.device, A.dtype
        a, b = A.detach().contiguous(), B.detach().contiguous()
        sched_dev = None if sched is None else sched.to(device)
        rs = _rest_table(a, rest, K)
        mi, cs = _state_operands(a[0], Mi, phase)
        N, Nd, nM, code, keep, head, tail = _sequence_args(a, rs, T1, T2, Δf, mi, cs, sched_dev)
        P, rows = a.shape[0], N * nM
        per_spin = dict(A=(D, P, rows, 9), B=(D, P, rows, 3), Mi=(D, rows, 3), T1=(D, rows), T2=(D, rows), Δf=(D, rows))
        tables = [None if k not in tan else tan[k].detach().to(device=device, dtype=dtype).reshape(per_spin[k]).contiguous()
                  for k in _SEQ_JVP_KEYS[:6]]
        # the block-uniform tables: rounded to the data type and widened, as rs is
        uniform = [None if k not in tan else tan[k].detach().to(device=device, dtype=dtype).double().contiguous()
                   for k in ('phase', 'rest')]
        Mt = torch.empty((K,) + tuple(b.shape[1:]), dtype=dtype, device=device)
        dMt = torch.empty((D, K) + tuple(b.shape[1:]), dtype=dtype, device=device)
        lib = _lib.require_library()
        cap = int(lib.mrphy_ab_sequence_jvp_max_dirs(code))
        assert cap >= 1
        for d0 in range(0, D, cap):                 # blocks of the capacity; Mt from the first
            nd = min(cap, D - d0)
            blk = lambda t: None if t is None else t[d0:d0 + nd]  # noqa: E731
            uni = [x for t in uniform for x in ((None, 0) if t is None else (blk(t), _over_n(t[0], N)))]
            _launch('mrphy_ab_sequence_jvp_fwd', device, code, a, b, *head, *tail, nd, *(blk(t) for t in tables), *uni,
                    Mt if d0 == 0 else None, dMt[d0:d0 + nd], N, nM, K)
        del keep
    return Mt.movedim(0, -2), dMt.movedim(1, -2)


def _over_bank(x, P, N, axis=0):
    r"""A spin-side operand (``axis = 0``) or its tangent (``axis = 1``, after the direction axis) for a batch of ``P·N``
    entries: repeated over ``P`` where it has the batch axis ``N > 1`` at ``axis``, left to broadcast where it has not."""
    if not isinstance(x, Tensor) or x.ndim <= axis or x.shape[axis] != N or N == 1:
        return x
    lead = tuple(x.shape[:axis])
    return x.unsqueeze(axis).expand(lead + (P,) + tuple(x.shape[axis:])).flatten(axis, axis + 1)


@_host.half_via_float
def ab_rfgr_jvp(
    rf: Tensor, gr: Tensor, loc: Tensor, *, tangents: dict,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
):
    r"""``(A, B, dA, dB)``: :func:`ab_rfgr`'s ``A`` `(N, *Nd, xyz, 3)`, ``B`` `(N, *Nd, xyz)` (its bits) and their
    forward-mode tangents ``dA`` `(D, N, *Nd, xyz, 3)`, ``dB`` `(D, N, *Nd, xyz)` along ``D`` directions.  A composition,
    no kernel of its own: ONE :func:`blochsim_rfgr_jvp` call on the batch ``4·N`` with ``Mi ∈ {0, e_x, e_y, e_z}``, whose
    ``dMo`` are the tangents of ``B`` and of ``A e_j + B``: ``dB = dMo|₀``, ``dA[..., :, j] = dMo|e_j − dMo|₀``.
    ``tangents``: :func:`blochsim_rfgr_jvp`'s keys without ``'Mi'``.  Its limits are inherited: one transmit coil
    (``NotImplementedError('parallel transmit')``) and ``4·N ≤ 65535``.  In fp32 the difference rounds at the level of
    ``|dMo|``, as any column of ``A`` obtained from two simulations does."""
    if rf.ndim == 4 and rf.shape[-1] != 1:
        raise NotImplementedError('parallel transmit')
    if isinstance(tangents, dict) and tangents.get('Mi') is not None:
        raise ValueError(f"mrphy_amd: `tangents` has an unknown key 'Mi': A and B do not depend on a state; the keys are "
                         f"{_JVP_KEYS[1:]}")
    kw = dict(Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    N, Nd = loc.shape[0], tuple(loc.shape[1:-1])
    side = lambda x: _over_bank(x, 4, N)  # noqa: E731
    over = lambda x: x.expand((4,) + tuple(x.shape)).flatten(0, 1)  # noqa: E731
    Mi = torch.zeros((4, N) + Nd + (3,), dtype=loc.dtype, device=loc.device)
    for j in range(3):
        Mi[1 + j, ..., j] = 1
    tan = {k: _over_bank(v, 4, N, axis=1) for k, v in (tangents.items() if isinstance(tangents, dict) else ())}
    kw4 = {k: side(v) for k, v in kw.items() if k != 'consts'}
    kw4['consts'] = None if consts is None else {k: side(v) for k, v in consts.items()}
    _, dMo = blochsim_rfgr_jvp(Mi.flatten(0, 1), over(rf) if rf.shape[0] == N else rf, over(gr) if gr.shape[0] == N else gr,
                               over(loc), tangents=tan if isinstance(tangents, dict) else tangents, **kw4)
    with torch.no_grad():
        det = lambda x: x.detach() if isinstance(x, Tensor) else x  # noqa: E731
        A, B = ab_rfgr(det(rf), det(gr), det(loc), **{k: det(v) for k, v in kw.items() if k != 'consts'},
                       consts=None if consts is None else {k: det(v) for k, v in consts.items()})
    dMo = dMo.unflatten(1, (4, N))
    dB = dMo[:, 0]
    dA = torch.stack([dMo[:, 1 + j] - dB for j in range(3)], dim=-1)
    return A, B, dA, dB


_SEQ_RFGR_BANK_KEYS = ('rf', 'gr', 'loc', 'b1Map', 'Δf', 'T1', 'T2')
_SEQ_RFGR_TRAIN_KEYS = ('Mi', 'phase', 'rest')


@_host.half_via_float
def sequence_rfgr_jvp(
    rf: Tensor, gr: Tensor, loc: Tensor, *, tangents: dict,
    pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
):
    r"""``(Mt, dMt)`` of :func:`sequence_rfgr` in forward mode: ONE :func:`ab_rfgr_jvp` call on the batch ``P·N`` forms
    the bank ``A, B`` `(P, N, *Nd, …)` and its tangents, :func:`ab_sequence_jvp` follows.  Operands exactly as
    :func:`sequence_rfgr`.  ``tangents``: a dict with one leading direction axis ``D`` for all keys:

      - ``'rf'`` `(D, P, N, xy, nT)`, ``'gr'`` `(D, P ⊻ 1, N, xyz, nT)`, ``'loc'``, ``'b1Map'`` feed the bank;
      - ``'T1'``, ``'T2'``, ``'Δf'`` feed both the pulses and the rests -- with ``Δf_rest`` given, ``'Δf'`` feeds only the
        pulses and the key ``'Δf_rest'`` the rests;
      - ``'Mi'``, ``'phase'``, ``'rest'`` feed the train.

    Any broadcastable axis may be 1.  The limits of :func:`ab_rfgr_jvp` are inherited with the batch ``P·N``: one
    transmit coil, ``4·P·N ≤ 65535``; ``consts=`` carries no tangents here.  Returns ``Mt`` `(N, *Nd, K, xyz)` and
    ``dMt`` `(D, N, *Nd, K, xyz)`."""
    if rf.ndim == 5 and rf.shape[-1] != 1:
        raise NotImplementedError('parallel transmit')
    assert rf.ndim in (4, 5) and gr.ndim == 4 and gr.shape[0] in (1, rf.shape[0]) and gr.shape[1] == rf.shape[1], \
        f"rf {tuple(rf.shape)} must be (P, N, xy, nT[, 1]) and gr {tuple(gr.shape)} (P ⊻ 1, N, xyz, nT)"
    P, N = rf.shape[0], rf.shape[1]
    sched = _sequence_schedule(pulse, P)          # before any work on the device
    rest_key = 'Δf' if Δf_rest is None else 'Δf_rest'
    keys = _SEQ_RFGR_BANK_KEYS + _SEQ_RFGR_TRAIN_KEYS + (('Δf_rest',) if Δf_rest is not None else ())
    D, given = _given_tangents(tangents, keys)
    bank = {k: given[k] for k in _SEQ_RFGR_BANK_KEYS if k in given}
    for k, lead in (('rf', P), ('gr', gr.shape[0])):     # the bank axis of the pulse tangents, flattened into the batch
        if k in bank:
            t = bank[k]
            op = rf if k == 'rf' else gr
            if t.ndim != op.ndim + 1 or any(a not in (1, b) for a, b in zip(t.shape[1:], op.shape)):
                raise ValueError(f"mrphy_amd: `tangents['{k}']` {tuple(t.shape)} does not broadcast to (D, "
                                 f"{', '.join(map(str, op.shape))})")
            bank[k] = t.expand((D, P) + tuple(op.shape[1:])).flatten(1, 2)
    for k in ('loc', 'b1Map', 'Δf', 'T1', 'T2'):
        if k in bank:
            bank[k] = _over_bank(bank[k], P, N, axis=1)
    side = lambda x: _over_bank(x, P, N)  # noqa: E731
    over = lambda x: x.expand((P,) + tuple(x.shape)).flatten(0, 1)  # noqa: E731
    ops = dict(Δf=side(Δf), b1Map=side(b1Map), γ_beff=side(γ_beff), T1=side(T1), T2=side(T2), γ=side(γ), dt=side(dt),
               consts=None if consts is None else {k: side(v) for k, v in consts.items()})
    rf_b, gr_b = rf.flatten(0, 1), over(gr[0]) if gr.shape[0] == 1 else gr.flatten(0, 1)
    train = {k: given[k] for k in _SEQ_RFGR_TRAIN_KEYS + ('T1', 'T2') if k in given}
    if rest_key in given:
        train['Δf'] = given[rest_key]
    if bank:
        A, B, dA, dB = ab_rfgr_jvp(rf_b, gr_b, over(loc), tangents=bank, **ops)
        train['A'], train['B'] = dA.unflatten(1, (P, N)), dB.unflatten(1, (P, N))
    else:
        with torch.no_grad():
            A, B = ab_rfgr(rf_b, gr_b, over(loc), **ops)
    return ab_sequence_jvp(A.unflatten(0, (P, N)), B.unflatten(0, (P, N)), tangents=train, pulse=sched, n=n, Mi=Mi,
                           phase=phase, rest=rest, T1=T1, T2=T2, Δf=Δf if Δf_rest is None else Δf_rest)


def _signal_buffers(query, code, b, mi, rx, nRx, K, want_ckpt):
    r"""``(sig, Mlast, ck, work)`` of a signal forward for the spins of ``b`` `(N, *Nd, 3)`: the samples (zeros for an
    empty problem, which launches nothing), the last state (``Mi`` for ``K = 0``), the fp64 checkpoints if wanted and
    the workspace of the sums as the query ``query`` of the library sizes it."""
    lib = _lib.require_library()
    device, dtype = b.device, b.dtype
    N, Nd = b.shape[0], tuple(b.shape[1:-1])
    nM = prod(Nd)
    coils = () if rx is None or rx.ndim == b.ndim else (nRx,)
    sig = (torch.zeros if N * nM * K == 0 else torch.empty)((N, 2, K, *coils), dtype=dtype, device=device)
    Mlast = torch.empty_like(b)
    if K == 0:                              # no repetition: the state is still Mi
        Mlast.copy_(torch.tensor((0., 0., 1.), dtype=dtype, device=device) if mi is None else
                    mi.reshape((mi.shape[0],) + (Nd if mi.shape[1] > 1 else (1,) * len(Nd)) + (3,)))
    S = int(lib.mrphy_train_signal_ck_every())
    ck = torch.empty((-(-K // S), N * nM, 3), dtype=torch.float64, device=device) if want_ckpt else None
    nbytes = int(query(code, N, nM, K, 2 * nRx))
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return sig, Mlast, ck, work


def _signal_cotangents(grad_sig, grad_Mlast, N, K, nRx, dtype):
    r"""``(gs, gl)`` as the signal adjoints read them: the cotangent of the signal as the wave-uniform table
    `(N, K, nRx, 2)` in fp64, that of ``Mlast`` contiguous in the data type; ``None`` for an absent one."""
    gs = None if grad_sig is None else \
        grad_sig.detach().to(torch.float64).reshape(N, 2, K, nRx).permute(0, 2, 3, 1).contiguous()
    gl = None if grad_Mlast is None else grad_Mlast.detach().to(dtype).contiguous()
    return gs, gl


def _fold_signal_grads(o, gl, K, N, Nd, Mi, phase, rx):
    r"""``(gMi, gφ, grx)`` of a signal adjoint from its raw gradients ``o``: an operand shared by spins or batch entries
    gets the sum over those who share it, accumulated in fp64 (``grad_phase`` is summed over the spins by the kernel);
    ``None`` where ``o`` holds none.  Without a repetition ``Mlast`` is ``Mi``."""
    f64 = torch.float64
    gMi = gφ = grx = None
    if o['gMi'] is not None:
        gMi = _fold_to_operand(gl if (K == 0 and gl is not None) else o['gMi'], Mi, f64)
    if o['gφ'] is not None:
        gφ = _fold_to_operand(o['gφ'], phase, f64)
    if o['grx'] is not None:
        grx = _fold_to_operand(o['grx'].reshape((N,) + Nd + tuple(rx.shape[1 + len(Nd):])), rx, f64)
    return gMi, gφ, grx


class TrainSignalHIP(Function):
    r"""``sig, Mlast = TrainSignalHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, rx, K, want_ckpt)`` -- see
    :func:`train_signal`.  ``rx`` `(N ⊻ 1, *Nd, xy)` or `(N ⊻ 1, *Nd, xy, nRx)` with ``nRx`` up to
    ``mrphy_train_signal_max_rx``, or ``None``; ``sig`` `(N, xy, K)` / `(N, xy, K, nRx)`, ``Mlast`` `(N, *Nd, xyz)`.
    Both outputs may carry a cotangent.  With ``want_ckpt`` the forward (``mrphy_train_signal_fwd``) leaves the fp64
    state every ``mrphy_train_signal_ck_every()`` repetitions, all the adjoint (``mrphy_train_signal_bwd``) reads
    besides the inputs; without it nothing per spin is written but ``Mlast``."""

    ARGS = ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'Δf', 'rx', 'K', 'want_ckpt')

    @staticmethod
    def forward(ctx, A, B, Mi, phase, rest, T1, T2, Δf, rx, K, want_ckpt):
        lib = _lib.require_library()
        a, b = A.detach().contiguous(), B.detach().contiguous()
        N, Nd, nM, code, keep, args = _rest_operands(a, rest, T1, T2, Δf)
        mi, cs = _state_operands(a, Mi, phase)
        r, nRx = _rx_operand(a, rx)
        sig, Mlast, ck, work = _signal_buffers(lib.mrphy_train_signal_workspace, code, b, mi, rx, nRx, K, want_ckpt)
        _launch('mrphy_train_signal_fwd', a.device, code, a, b, *args, *_state_args(mi, cs, N), r, nRx, sig, Mlast, ck,
                work, work.numel(), N, nM, K)
        del keep
        ctx.set_materialize_grads(False)
        if want_ckpt:
            ctx.save_for_backward(a, b, mi, cs, r, ck)
            ctx.consts = (rest, T1, T2, Δf)
            ctx.state = (Mi, phase, rx, K, nRx)
        return sig, Mlast

    @staticmethod
    def backward(ctx, grad_sig, grad_Mlast):
        need = ctx.needs_input_grad
        none = (None,) * len(TrainSignalHIP.ARGS)
        if not any(need) or (grad_sig is None and grad_Mlast is None):
            return none
        consts = ctx.consts
        Mi, phase, rx, K, nRx = ctx.state
        need_c = [w and c is not None for w, c in zip(need[4:8], consts)]
        need_mi, need_φ, need_rx = need[2] and Mi is not None, need[3] and phase is not None, need[8] and rx is not None
        if not (need[0] or need[1] or need_mi or need_φ or need_rx or any(need_c)):
            return none
        lib = _lib.require_library()
        a, b, mi, cs, r, ck = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, args = _rest_operands(a, *consts)
        gs, gl = _signal_cotangents(grad_sig, grad_Mlast, N, K, nRx, dtype)
        empty = N * nM * K == 0
        o = _new_grads(empty, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape, gMi=need_mi and b.shape,
                       gφ=need_φ and (N, K), grx=need_rx and (N, nM, 2, nRx))
        # per spin in fp64 whatever the data type: summed over the spins that share the operand, then rounded once
        o.update(_new_grads(empty, torch.float64, device, gC=any(need_c) and (N,) + Nd + (4,)))
        nbytes = int(lib.mrphy_train_signal_workspace(code, N, nM, K, 1)) if need_φ else 0
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        _launch('mrphy_train_signal_bwd', device, code, a, b, gs, gl, *args, *_state_args(mi, cs, N), r, nRx, ck,
                *(o[k] for k in ('gA', 'gB', 'gC', 'gMi', 'gφ', 'grx')), work, work.numel(), N, nM, K)
        del keep
        gMi, gφ, grx = _fold_signal_grads(o, gl, K, N, Nd, Mi, phase, rx)
        return (o['gA'], o['gB'], gMi, gφ) + _fold_rest_consts(o['gC'], consts, need_c, N, Nd) + (grx, None, None)


def _train_signal_max_rx(dtype) -> int:
    return int(_lib.require_library().mrphy_train_signal_max_rx(_code(dtype)))


def _signal_by_coil_blocks(Fn, head, rx, tail, nb):
    r"""``sig, Mlast`` of ``Fn.apply(*head, rx, *tail)`` for any number of coils: above the capacity of a launch, blocks
    of that many coils, one simulation each -- a coil's sums do not depend on the other coils -- with the samples
    joined along the coil axis and ``Mlast`` of the first block.  ``nb``: the dimensions of one entry's ``B``."""
    cap = _train_signal_max_rx(head[0].dtype)
    if rx is None or rx.ndim != nb + 1 or rx.shape[-1] <= cap:
        return Fn.apply(*head, rx, *tail)
    parts = [Fn.apply(*head, rx[..., c:c + cap], *tail) for c in range(0, rx.shape[-1], cap)]
    return torch.cat([p[0] for p in parts], dim=-1), parts[0][1]


def _demodulate(sig, phase):
    r"""``sig`` `(N, xy, K[, nRx])` with sample ``k`` multiplied by ``exp(-iφ_k)``, formed in fp64 and rounded once;
    ``sig`` itself without a ``phase``."""
    if phase is None:
        return sig
    φ = phase.to(device=sig.device, dtype=torch.float64).reshape(phase.shape + (1,) * (sig.ndim - 3))
    c, s = torch.cos(φ), torch.sin(φ)
    s0, s1 = sig[:, 0].to(torch.float64), sig[:, 1].to(torch.float64)
    return torch.stack((s0 * c + s1 * s, s1 * c - s0 * s), dim=1).to(sig.dtype)


@_host.half_via_float
def train_signal(
    A: Tensor, B: Tensor, *, n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, rx: Optional[Tensor] = None, demod: bool = False, return_last: bool = False
):
    r"""The signal a receive coil measures after each of the ``K`` repetitions of :func:`ab_train`: the transverse
    magnetisation of record ``k`` (``M_{k+1}``, right after pulse ``k``) summed over the spins ``*Nd``, weighted by the
    receive map ``rx`` as :func:`signal_rfgr` weights it (a complex product, no conjugate):

        ``sig[n, 0, k] = Σ_s rx_re·Mx − rx_im·My``,  ``sig[n, 1, k] = Σ_s rx_re·My + rx_im·Mx``.

    The recursion, the operands ``A, B, n, Mi, phase, rest, T1, T2, Δf``, their shapes, broadcasting and absences are
    exactly :func:`ab_train`'s.

    Usage:
        ``sig = train_signal(A, B, *, n, Mi, phase, rest, T1, T2, Δf, rx, demod)``
        ``sig, Mlast = train_signal(..., return_last=True)``
    Optionals besides :func:`ab_train`'s:
        - ``rx``: `(N ⊻ 1, *Nd, xy)` or `(N ⊻ 1, *Nd, xy, nRx)`, the layout of ``b1Map``; ``None`` = ``(1, 0)``, the plain
          sums of ``Mx`` and ``My``.
        - ``demod``: multiply sample ``k`` by ``exp(-iφ_k)``, so that the receiver follows the RF phase (``φ_k`` is
          shared by the spins, so this commutes with the sum: torch ops on the small result, through autograd).
        - ``return_last``: also return ``Mlast`` `(N, *Nd, xyz)`, the last record -- :func:`ab_train`'s bit for bit --,
          so that a sequence can carry on from it as ``Mi`` of the next call: segments with different pulses (a
          variable flip angle) chain this way.  For ``K = 0`` it is ``Mi`` expanded, or ``(0, 0, 1)``.
    Outputs:
        - ``sig``: `(N, xy, K)`, or `(N, xy, K, nRx)` when ``rx`` has a coil axis.

    The sum is formed inside the kernel (Ktrs, ``mrphy_train_signal_fwd``): the recursion is Ktr's, in fp64 whatever
    the data type; per repetition the lane's products go through an LDS tile into fp64 partial sums per wave, a second
    pass adds those in a fixed order and rounds once.  No float atomics, the same inputs give the same bits, and nothing
    of size ``K × spins`` is written: with a gradient wanted, the fp64 state every ``mrphy_train_signal_ck_every()``
    repetitions.  Up to ``mrphy_train_signal_max_rx`` coils (8) share one simulation per launch, more run in blocks of
    that many; every coil's samples are the bits a call with that coil alone gives.

    Differentiable w.r.t. ``A, B, Mi, phase, rest, T1, T2, Δf`` and ``rx`` through both outputs
    (Ktrsb, ``mrphy_train_signal_bwd``: Ktrb's sweep on states recomputed per segment from the checkpoints; the
    gradient of the phase is summed over the spins inside the kernel; deterministic).  With the gradient w.r.t. ``rx``
    a proton density, a coil sensitivity and an echo time stay in torch on per-spin tensors: the signal at an echo time
    ``TE`` after the pulse is this one with ``rx · exp(-TE/T2) · exp(-i2πΔf·TE)`` for ``rx``.

    Out of scope as :func:`ab_train`: thinning the records.  A flip angle or ``rest`` per repetition within one call is
    :func:`sequence_signal`.
    """
    N, Nd = _train_spins(A, B)
    K = _train_length(n, phase, N)
    _check_rx(rx, N, Nd, B.ndim)
    _check_train_operands(A, B, N, Nd, Mi, rest, T1, T2, Δf)
    head = (A, B, Mi, phase, rest, T1, T2, Δf)
    sig, Mlast = _signal_by_coil_blocks(TrainSignalHIP, head, rx, (K, _grad_wanted(*head, rx)), B.ndim)
    if demod:
        sig = _demodulate(sig, phase)
    return (sig, Mlast) if return_last else sig


@_host.half_via_float
def train_signal_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, rx: Optional[Tensor] = None, demod: bool = False, return_last: bool = False,
    b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
):
    r"""The signal of the first ``K`` repetitions of a pulse (SPGR with RF spoiling, phase-cycled bSSFP, an
    inversion-prepared train), from ``rf`` and ``gr``:

        ``train_signal(*ab_rfgr(rf, gr, loc, ...), n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2,
        Δf=Δf if Δf_rest is None else Δf_rest, rx=rx, demod=demod, return_last=return_last)``

    built as :func:`train_rfgr` is on :func:`ab_train`.  Operands of the pulse exactly as :func:`ab_rfgr`, those of the
    train and of the receiver as :func:`train_signal`; ``Δf_rest`` as in :func:`steadystate_rfgr`.  Every route of
    :func:`ab_rfgr` (fused, split, composed; parallel transmit) serves it, so gradients reach every operand ``ab_rfgr``
    serves, and ``Mi, phase, rest, T1, T2, Δf`` / ``Δf_rest``, ``rx`` through the train: ``T1`` and ``T2``, shared by the
    pulse and the rest, receive the sum of both paths.
    """
    A, B = ab_rfgr(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt, consts=consts)
    return train_signal(A, B, n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2,
                        Δf=Δf if Δf_rest is None else Δf_rest, rx=rx, demod=demod, return_last=return_last)


def _fold_repetition_sums(g, x):
    r"""The gradient of ``rest`` from the kernel's sums over the spins ``g`` `(N, K)` fp64: folded in fp64 over what ``x``
    shares -- ``x`` `(N ⊻ 1, K)`, or a duration `()` ⊻ `(N ⊻ 1,)` that the repetitions share too -- and rounded once."""
    g = g.sum_to_size(tuple(x.shape)) if x.ndim == 2 else g.sum(1).sum_to_size(tuple(x.shape) or (1,))
    return g.reshape(x.shape).to(device=x.device, dtype=x.dtype)


def _sweep_scratch(code, a, N, Nd, nM, K, empty, need_c, need_φ, need_r, need_bank):
    r"""``(o, work, bank, nbank)``: what a launch of Ksqsb's sweep (``mrphy_sequence_signal_bwd``, and
    ``mrphy_sequence_steadystate_bwd`` which hands over to it) needs besides its outputs in the data type.  ``o`` holds
    ``gC`` per spin and ``gφ``, ``gr`` summed over the spins by the kernel, in fp64 whatever the data type (``None`` where
    not needed); ``work`` is the workspace of those sums, ``bank`` the fp64 workspace of ``nbank`` bytes of the gradients
    of the bank ``a`` (``None``, 0 without ``need_bank``)."""
    lib = _lib.require_library()
    device, f64 = a.device, torch.float64
    o = _new_grads(empty, f64, device, gC=any(need_c) and (N,) + Nd + (3,), gφ=need_φ and (N, K), gr=need_r and (N, K))
    nQ = int(bool(need_φ)) + int(bool(need_r))
    nbytes = int(lib.mrphy_sequence_signal_workspace(code, N, nM, K, nQ)) if nQ else 0
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    nbank = int(lib.mrphy_sequence_signal_bank_workspace(code, a.shape[0], N, nM)) if need_bank else 0
    bank = torch.empty(nbank // 8, dtype=f64, device=device) if nbank else None
    return o, work, bank, nbank


def _fold_sweep_grads(o, rest, consts, need_c, N, Nd):
    r"""``(gr, (gT1, gT2, gΔf))`` from :func:`_sweep_scratch`'s ``gr`` and ``gC``: each folded in fp64 over those who
    share the operand, then rounded once; ``None`` where ``o`` holds none.  (``gφ`` folds as any sum does:
    :func:`_fold_to_operand`.)"""
    gr = None if o['gr'] is None else _fold_repetition_sums(o['gr'], rest)
    return gr, _fold_rest_consts(o['gC'], consts, need_c, N, Nd)


class SequenceSignalHIP(Function):
    r"""``sig, Mlast = SequenceSignalHIP.apply(A, B, Mi, phase, rest, T1, T2, Δf, rx, K, sched, want_ckpt)`` -- see
    :func:`sequence_signal`.  ``A, B`` carry the bank axis in front and ``sched`` is the checked schedule as for
    :class:`AbSequenceHIP`; ``rx``, ``sig``, ``Mlast`` and ``want_ckpt`` as for :class:`TrainSignalHIP`.  The forward
    (``mrphy_sequence_signal_fwd``) leaves the fp64 state every ``mrphy_train_signal_ck_every()`` repetitions when a
    gradient is wanted, all the adjoint (``mrphy_sequence_signal_bwd``) reads besides the inputs; the adjoint's scratch
    is the fp64 workspace of the bank's gradients and the per-wave sums of ``grad_phase`` and ``grad_rest``."""

    ARGS = ('A', 'B', 'Mi', 'phase', 'rest', 'T1', 'T2', 'Δf', 'rx', 'K', 'sched', 'want_ckpt')

    @staticmethod
    def forward(ctx, A, B, Mi, phase, rest, T1, T2, Δf, rx, K, sched, want_ckpt):
        lib = _lib.require_library()
        device = A.device
        a, b = A.detach().contiguous(), B.detach().contiguous()
        sched_dev = None if sched is None else sched.to(device)
        rs = _rest_table(a, rest, K)
        mi, cs = _state_operands(a[0], Mi, phase)
        N, Nd, nM, code, keep, head, tail = _sequence_args(a, rs, T1, T2, Δf, mi, cs, sched_dev)
        r, nRx = _rx_operand(a[0], rx)
        sig, Mlast, ck, work = _signal_buffers(lib.mrphy_sequence_signal_workspace, code, b[0], mi, rx, nRx, K, want_ckpt)
        _launch('mrphy_sequence_signal_fwd', device, code, a, b, *head, *tail, r, nRx, sig, Mlast, ck, work, work.numel(),
                N, nM, K)
        del keep
        ctx.set_materialize_grads(False)
        if want_ckpt:
            ctx.save_for_backward(a, b, mi, cs, rs, sched_dev, r, ck)
            ctx.consts = (T1, T2, Δf)
            ctx.state = (Mi, phase, rest, rx, K, nRx)
        return sig, Mlast

    @staticmethod
    def backward(ctx, grad_sig, grad_Mlast):
        need = ctx.needs_input_grad
        none = (None,) * len(SequenceSignalHIP.ARGS)
        if not any(need) or (grad_sig is None and grad_Mlast is None):
            return none
        consts = ctx.consts
        Mi, phase, rest, rx, K, nRx = ctx.state
        need_c = [w and c is not None for w, c in zip(need[5:8], consts)]
        need_mi, need_φ, need_r = need[2] and Mi is not None, need[3] and phase is not None, need[4] and rest is not None
        need_rx = need[8] and rx is not None
        if not (need[0] or need[1] or need_mi or need_φ or need_r or need_rx or any(need_c)):
            return none
        a, b, mi, cs, rs, sched_dev, r, ck = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, head, tail = _sequence_args(a, rs, *consts, mi, cs, sched_dev)
        gs, gl = _signal_cotangents(grad_sig, grad_Mlast, N, K, nRx, dtype)
        empty = N * nM * K == 0
        o = _new_grads(empty, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape,
                       gMi=need_mi and b.shape[1:], grx=need_rx and (N, nM, 2, nRx))
        o64, work, bank, nbank = _sweep_scratch(code, a, N, Nd, nM, K, empty, need_c, need_φ, need_r, need[0] or need[1])
        o.update(o64)
        _launch('mrphy_sequence_signal_bwd', device, code, a, b, *head, gs, gl, *tail, r, nRx, ck,
                *(o[k] for k in ('gA', 'gB', 'gC', 'gr', 'gMi', 'gφ', 'grx')), work, work.numel(), bank, nbank, N, nM, K)
        del keep, work, bank
        gMi, gφ, grx = _fold_signal_grads(o, gl, K, N, Nd, Mi, phase, rx)
        gr, gconsts = _fold_sweep_grads(o, rest, consts, need_c, N, Nd)
        return (o['gA'], o['gB'], gMi, gφ, gr) + gconsts + (grx, None, None, None)


@_host.half_via_float
def sequence_signal(
    A: Tensor, B: Tensor, *, pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None,
    phase: Optional[Tensor] = None, rest: Optional[Tensor] = None, T1: Optional[Tensor] = None,
    T2: Optional[Tensor] = None, Δf: Optional[Tensor] = None, rx: Optional[Tensor] = None, demod: bool = False,
    return_last: bool = False
):
    r"""The signal a receive coil measures after each of the ``K`` repetitions of :func:`ab_sequence` -- what one fits
    to a measured MR-fingerprinting, inversion- or T2-prepared or variable-flip-angle train: the transverse
    magnetisation of record ``k`` summed over the spins ``*Nd``, weighted by the receive map ``rx`` exactly as
    :func:`train_signal` weights it,

        ``sig[n, 0, k] = Σ_s rx_re·Mx − rx_im·My``,  ``sig[n, 1, k] = Σ_s rx_re·My + rx_im·Mx``.

    Usage:
        ``sig = sequence_signal(A, B, *, pulse, n, Mi, phase, rest, T1, T2, Δf, rx, demod)``
        ``sig, Mlast = sequence_signal(..., return_last=True)``

    The sequence-side operands ``A`` `(P, N, *Nd, xyz, 3)`, ``B`` `(P, N, *Nd, xyz)`, ``pulse``, ``n``, ``Mi``, ``phase``,
    ``rest`` (`()`, `(N ⊻ 1,)` or `(N ⊻ 1, K)`), ``T1``, ``T2``, ``Δf`` -- shapes, broadcasting, absences, the host-side
    check of the schedule and its errors -- are exactly :func:`ab_sequence`'s.  The receiver-side operands ``rx``
    (`(N ⊻ 1, *Nd, xy)` or `(N ⊻ 1, *Nd, xy, nRx)`, ``None`` = ``(1, 0)``), ``demod``, ``return_last``, the output
    ``sig`` `(N, xy, K[, nRx])`, ``Mlast`` `(N, *Nd, xyz)`, the blocks of ``mrphy_train_signal_max_rx`` coils above that
    many, and the cases ``K = 0`` and no spins are exactly :func:`train_signal`'s.

    The sum is formed inside the kernel (Ksqs, ``mrphy_sequence_signal_fwd``): :func:`train_signal`'s frame around
    :func:`ab_sequence`'s repetition.  The state has :func:`ab_sequence`'s bits -- ``Mlast`` is its last record --, a
    coil's samples are those of a call with that coil alone, and with ``P = 1`` and one ``rest`` both outputs are
    :func:`train_signal`'s, bit for bit.  No float atomics, the same inputs give the same bits, and nothing of size
    ``K × spins`` is written: with a gradient wanted, the fp64 state every ``mrphy_train_signal_ck_every()`` repetitions.

    Differentiable through both outputs w.r.t. ``A``, ``B`` (the whole bank: an entry the schedule never plays gets an
    exactly-zero gradient), ``Mi``, ``phase``, ``rest`` (in the form given), ``T1``, ``T2``, ``Δf`` and ``rx`` (Ksqsb,
    ``mrphy_sequence_signal_bwd``: :func:`train_signal`'s sweep per segment on states recomputed from the checkpoints,
    with :func:`ab_sequence`'s refreshes; the bank's gradients go through an fp64 workspace of ``P·12`` numbers per
    spin; the gradients of ``phase`` and ``rest`` are summed over the spins inside the kernel per repetition and folded
    over what shares the operand in fp64; deterministic).

    Out of scope: a schedule per batch entry; thinning the samples; a readout at an echo time inside the kernel
    (``rx · exp(-TE/T2) · exp(-i2πΔf·TE)`` for ``rx``, in torch, as :func:`train_signal` documents); a gradient of
    ``rest`` per spin; a CPU path.  The signal of the steady period is this function with
    ``Mi=sequence_steadystate(...)``.
    """
    *_, sched, K = _sequence_operands(A, B, pulse, n, phase, rest, T1, T2, Δf, Mi, rx=rx)
    head = (A, B, Mi, phase, rest, T1, T2, Δf)
    sig, Mlast = _signal_by_coil_blocks(SequenceSignalHIP, head, rx, (K, sched, _grad_wanted(*head, rx)), B.ndim - 1)
    if demod:
        sig = _demodulate(sig, phase)
    return (sig, Mlast) if return_last else sig


@_host.half_via_float
def sequence_signal_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    pulse=None, n: Optional[int] = None, Mi: Optional[Tensor] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, rx: Optional[Tensor] = None, demod: bool = False, return_last: bool = False,
    b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
):
    r"""The signal of a sequence that plays a bank of pulses by a schedule, from ``rf`` `(P, N, xy, nT[, nCoils])` and
    ``gr`` `(P ⊻ 1, N, xyz, nT)`: ONE :func:`ab_rfgr` call on the batch ``P·N`` exactly as :func:`sequence_rfgr` makes
    it, its ``A, B`` viewed as the bank, then :func:`sequence_signal`.  Operands of the pulses as :func:`ab_rfgr`, those
    of the sequence and of the receiver as :func:`sequence_signal`; ``Δf_rest`` as in :func:`steadystate_rfgr`.

    Every route of :func:`ab_rfgr` (fused, split, composed; parallel transmit) serves it, so gradients reach ``rf``,
    ``gr`` and every operand ``ab_rfgr`` differentiates -- a flip-angle schedule ``rf = s[:, None, None, None] * rf0``
    gets ``∂/∂s`` by autograd -- and ``Mi, phase, rest, T1, T2, Δf`` / ``Δf_rest``, ``rx`` through the sequence.
    :func:`ab_rfgr`'s limit on the batch is inherited: ``P·N ≤ 65535``.  Out of scope as in :func:`sequence_signal`.
    """
    A, B, sched = _sequence_bank(rf, gr, loc, pulse, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt,
                                 consts=consts)
    return sequence_signal(A, B, pulse=sched, n=n, Mi=Mi, phase=phase, rest=rest, T1=T1, T2=T2,
                           Δf=Δf if Δf_rest is None else Δf_rest, rx=rx, demod=demod, return_last=return_last)


class SequenceSteadyStateHIP(Function):
    r"""``Mss = SequenceSteadyStateHIP.apply(A, B, phase, rest, T1, T2, Δf, K, sched, want)`` -- see
    :func:`sequence_steadystate`.  ``A, B`` carry the bank axis in front and ``sched`` is the checked schedule as for
    :class:`AbSequenceHIP`.  With ``want`` the forward (``mrphy_sequence_steadystate_fwd``) also leaves the composed
    period ``per`` `(12, N·nM)` and the fp64 states ``ck`` every ``mrphy_train_signal_ck_every()`` repetitions of the
    period started at ``Mss``, all the adjoint (``mrphy_sequence_steadystate_bwd``) reads besides the inputs; the
    adjoint's scratch is ``λ``, the fp64 workspace of the bank's gradients and the per-wave sums of ``grad_phase`` and
    ``grad_rest``, as :class:`SequenceSignalHIP`'s."""

    ARGS = ('A', 'B', 'phase', 'rest', 'T1', 'T2', 'Δf', 'K', 'sched', 'want')

    @staticmethod
    def forward(ctx, A, B, phase, rest, T1, T2, Δf, K, sched, want):
        lib = _lib.require_library()
        device = A.device
        a, b = A.detach().contiguous(), B.detach().contiguous()
        sched_dev = None if sched is None else sched.to(device)
        rs = _rest_table(a, rest, K)
        _, cs = _state_operands(a[0], None, phase)
        N, Nd, nM, code, keep, head, ops = _sequence_args(a, rs, T1, T2, Δf, None, cs, sched_dev, with_mi=False)
        Mss = torch.empty_like(b[0])
        per = ck = None
        if want:
            S = int(lib.mrphy_train_signal_ck_every())
            per = torch.empty((12, N * nM), dtype=torch.float64, device=device)
            ck = torch.empty((-(-K // S), N * nM, 3), dtype=torch.float64, device=device)
        _launch('mrphy_sequence_steadystate_fwd', device, code, a, b, *head, *ops, Mss, per, ck, N, nM, K)
        del keep
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(a, b, cs, rs, sched_dev, per, ck)
            ctx.consts = (T1, T2, Δf)
            ctx.state = (phase, rest, K)
        return Mss

    @staticmethod
    def backward(ctx, grad_Mss):
        need = ctx.needs_input_grad
        none = (None,) * len(SequenceSteadyStateHIP.ARGS)
        if not any(need) or grad_Mss is None:
            return none
        consts = ctx.consts
        phase, rest, K = ctx.state
        need_c = [w and c is not None for w, c in zip(need[4:7], consts)]
        need_φ, need_r = need[2] and phase is not None, need[3] and rest is not None
        if not (need[0] or need[1] or need_φ or need_r or any(need_c)):
            return none
        a, b, cs, rs, sched_dev, per, ck = ctx.saved_tensors
        device, dtype = a.device, a.dtype
        N, Nd, nM, code, keep, head, ops = _sequence_args(a, rs, *consts, None, cs, sched_dev, with_mi=False)
        g = grad_Mss.detach().to(dtype).contiguous()
        lam = torch.empty_like(g)
        empty = N * nM == 0
        o = _new_grads(empty, dtype, device, gA=need[0] and a.shape, gB=need[1] and b.shape)
        o64, work, bank, nbank = _sweep_scratch(code, a, N, Nd, nM, K, empty, need_c, need_φ, need_r, need[0] or need[1])
        o.update(o64)
        _launch('mrphy_sequence_steadystate_bwd', device, code, a, b, *head, g, *ops, per, ck, lam,
                *(o[k] for k in ('gA', 'gB', 'gC', 'gr', 'gφ')), work, work.numel(), bank, nbank, N, nM, K)
        del keep, work, bank, lam
        gφ = _fold_to_operand(o['gφ'], phase, torch.float64) if need_φ else None
        gr, gconsts = _fold_sweep_grads(o, rest, consts, need_c, N, Nd)
        return (o['gA'], o['gB'], gφ, gr) + gconsts + (None, None, None)


@_host.half_via_float
def sequence_steadystate(
    A: Tensor, B: Tensor, *, pulse=None, n: Optional[int] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None
) -> Tensor:
    r"""The steady state of a sequence whose PERIOD is the ``K`` repetitions of :func:`ab_sequence` -- RF-spoiled SPGR,
    phase-cycled bSSFP, interleaved flip angles or TRs (AFI, VFA pairs), a fingerprinting train played back to back, a
    prepared train with a recovery delay.  Per spin, repetition ``k`` is :func:`ab_sequence`'s affine map

        ``M⁻ = F_k M + f_k``,  ``M' = Rz(φ_k) [A_p Rz(-φ_k) M⁻ + B_p]``, ``p = pulse[k]``;

    the ``K`` of them compose to ``Φ(M) = Ā M + b̄``, and

        ``Mss = (I - Ā)⁻¹ b̄``.

    ``Mss`` is the state right AFTER the last repetition of the period, which is also the state before the rest of
    repetition 0: the convention of :func:`ab_steadystate`'s ``Mss`` and record ``K-1`` of :func:`ab_sequence`.
    ``ab_sequence(A, B, ..., Mi=Mss)`` gives the states after each repetition of the steady period and
    ``sequence_signal(A, B, ..., Mi=Mss)`` its signal, with gradients flowing through ``Mi`` into this function.

    Usage:
        ``Mss = sequence_steadystate(A, B, *, pulse, n, phase, rest, T1, T2, Δf)``

    The operands ``A`` `(P, N, *Nd, xyz, 3)`, ``B`` `(P, N, *Nd, xyz)`, ``pulse``, ``n``, ``phase``, ``rest`` (`()`,
    `(N ⊻ 1,)` or `(N ⊻ 1, K)`), ``T1``, ``T2``, ``Δf`` -- shapes, broadcasting, absences, the host-side check of the
    schedule and its errors -- are exactly :func:`ab_sequence`'s.  There is no ``Mi``: a steady state has forgotten it.
    ``K = 0`` is a ``ValueError``: a period needs a repetition.  Returns ``Mss`` `(N, *Nd, xyz)`.

    The caller supplies one WHOLE period.  RF spoiling with the quadratic 117° increment,
    ``φ_k = 117° · k (k + 1) / 2``: ``φ(k + 80) - φ(k) ≡ 0 (mod 360°)`` for every ``k`` and 40 is not a period, so the
    period is 80 repetitions -- ``phase`` `(N ⊻ 1, 80)` -- and there is no one-pulse steady state.

    One kernel (Ksqp, ``mrphy_sequence_steadystate_fwd``): one thread per spin carries four fp64 columns through
    :func:`ab_sequence`'s repetition -- the affine column and the three columns of ``I`` through the linear part; nothing
    is obtained as a difference -- and solves in :func:`ab_steadystate`'s cofactor form, all in fp64, rounded once.
    Nothing of size ``K × spins`` is written.  Differentiable w.r.t. ``A``, ``B`` (the whole bank: an entry the schedule
    never plays gets an exactly-zero gradient), ``phase``, ``rest`` (in the form given), ``T1``, ``T2`` and ``Δf``
    (``mrphy_sequence_steadystate_bwd``: ``λ = (I - Ā)⁻ᵀ g`` per spin, then :func:`sequence_signal`'s sweep over the
    period started at ``Mss``, from fp64 checkpoints the forward left when a gradient was wanted; deterministic).

    The kernels compute in fp64 whatever the data type and round the outputs once; in fp32 ``Mss`` still inherits the
    rounding of ``A``, ``B`` amplified by the condition number of ``I - Ā``, about ``1 / (1 - exp(-Σ_k rest_k / T1))``
    for pulses that do not relax much.  A singular system (no relaxation in the pulses nor in the rests) gives non-finite
    values: nothing synchronises with the host to detect it.

    Out of scope: a schedule per batch entry; returning ``Ā, b̄``; a signal summed inside the same launch (that is
    :func:`sequence_signal` with ``Mi=Mss``); a CPU path.
    """
    *_, sched, K = _sequence_operands(A, B, pulse, n, phase, rest, T1, T2, Δf, None, period=True)
    want = _grad_wanted(A, B, phase, rest, T1, T2, Δf)
    return SequenceSteadyStateHIP.apply(A, B, phase, rest, T1, T2, Δf, K, sched, want)


@_host.half_via_float
def sequence_steadystate_rfgr(
    rf: Tensor, gr: Tensor, loc: Tensor, *,
    pulse=None, n: Optional[int] = None, phase: Optional[Tensor] = None,
    rest: Optional[Tensor] = None, T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None, Δf_rest: Optional[Tensor] = None
) -> Tensor:
    r"""The steady state of a period that plays a bank of pulses by a schedule, from ``rf`` `(P, N, xy, nT[, nCoils])`
    and ``gr`` `(P ⊻ 1, N, xyz, nT)`: ONE :func:`ab_rfgr` call on the batch ``P·N`` exactly as :func:`sequence_rfgr`
    makes it, its ``A, B`` viewed as the bank, then :func:`sequence_steadystate`.  Operands of the pulses as
    :func:`ab_rfgr`, those of the period as :func:`sequence_steadystate`; ``rest``, ``T1`` and ``T2`` are required and
    ``Δf_rest`` is as in :func:`steadystate_rfgr`.  Returns ``Mss`` `(N, *Nd, xyz)`, the state right after the last
    repetition of the period.

    Every route of :func:`ab_rfgr` (fused, split, composed; parallel transmit) serves it, so gradients reach ``rf``,
    ``gr`` and every operand ``ab_rfgr`` differentiates, and ``phase, rest, T1, T2, Δf`` / ``Δf_rest`` through the period:
    ``T1`` and ``T2`` receive the sum of the pulses' and the rests' paths.  :func:`ab_rfgr`'s limit on the batch is
    inherited: ``P·N ≤ 65535``.  The fp32 note and what is out of scope as in :func:`sequence_steadystate`.
    """
    assert rest is not None and T1 is not None and T2 is not None, \
        "sequence_steadystate_rfgr: a steady state needs relaxation -- `rest`, `T1` and `T2` are required"
    if rf.ndim in (4, 5):                         # the schedule and the length before any work on the device
        _period_length(n, _sequence_schedule(pulse, rf.shape[0]), phase, rf.shape[1])
    A, B, sched = _sequence_bank(rf, gr, loc, pulse, Δf=Δf, b1Map=b1Map, γ_beff=γ_beff, T1=T1, T2=T2, γ=γ, dt=dt,
                                 consts=consts)
    return sequence_steadystate(A, B, pulse=sched, n=n, phase=phase, rest=rest, T1=T1, T2=T2,
                                Δf=Δf if Δf_rest is None else Δf_rest)
