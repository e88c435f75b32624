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
(``rf`` `(N,xy,nT,nCoils)` with a ``b1Map``, up to 8 coils) has its own kernel.  Cases the fused
adjoint does not cover (more coils, gradients w.r.t. the spin-side maps) compose ``rfgr2beff`` and
``blochsim`` instead -- HIP kernels as well; a pulse length that is not a multiple of 16 is split
into a fused part and a tail of at most 15 composed steps.

:func:`blochsim_rfgr_traj` is the same simulation with the magnetisation recorded during the pulse (the history
``Mhst`` the reference forms inside ``BlochSim.forward`` and drops, ``sims.py:83,131``), differentiable through the
trajectory kernels K2t / K2bt.
"""
from math import pi as π, prod  # noqa: F401
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib, _host
from ._consts import γH, dt0

__all__ = ['blochsim_rfgr', 'blochsim_rfgr_traj']


class BlochSimRfGrHIP(Function):
    r"""``M = BlochSimRfGrHIP.apply(Mi, rf, gr, pulse_on_spins, γ2πdt, E1, E2, E1_1, want_ckpt, every)``

    ``every = None``: ``M`` is ``Mo`` (``mrphy_blochsim_rfgr_fwd`` / ``_bwd``); an int: the trajectory, time-major
    ``(nRec, N, *Nd, 3)`` (the ``_traj_`` entry points).  ``want_ckpt`` is decided by the caller
    (:func:`_route`: a gradient w.r.t. ``Mi``, ``rf`` or ``gr`` is wanted, grad mode is on and the fused adjoint
    covers the case) -- NOT re-derived from ``ctx.needs_input_grad``, which stays ``True`` under ``torch.no_grad()``."""

    @staticmethod
    def forward(ctx, Mi, rf, gr, p, γ2πdt, E1, E2, E1_1, want_ckpt=False, every=None):
        from . import sims
        lib = _lib.require_library()
        device, dtype = Mi.device, Mi.dtype
        code, g, e1, e2, e1m1 = sims._prep_constants(γ2πdt, E1, E2, E1_1, p.N, p.Nd, dtype, device)
        Mi_c = Mi.detach().contiguous()
        traj = every is not None
        M = (torch.empty((-(-p.nT // every), p.N) + p.Nd + (3,), dtype=dtype, device=device) if traj
             else torch.empty_like(Mi_c))
        need = bool(want_ckpt)
        ck = int(lib.mrphy_blochsim_rfgr_ck_every())
        # one checkpoint per started segment: nCk = ceil(nT / ck_every) (include/mrphy_hip.h)
        Mck = (torch.empty((-(-p.nT // ck), p.N * p.nM, 3), dtype=dtype, device=device)
               if need else None)
        nul = _host.NULL_BC
        consts = (*g.args, *(e1.args if e1 else nul), *(e2.args if e2 else nul),
                  e1m1.t.data_ptr() if e1m1 else None)
        ckpt = (Mck.data_ptr() if need else None, ck if need else 0)
        # the trajectory's Mo is optional (it equals the last record): not asked for
        name, outs = (('mrphy_blochsim_rfgr_traj_fwd', (None, *ckpt, M.data_ptr(), every)) if traj
                      else ('mrphy_blochsim_rfgr_fwd', (M.data_ptr(), *ckpt)))
        with torch.cuda.device(device):
            rc = getattr(lib, name)(code, Mi_c.data_ptr(), *p.k0_args(), *consts, *outs,
                                    p.N, p.nM, p.nT, p.nC, _host.current_stream(device))
        _lib.check(rc, name)
        if need:
            ctx.save_for_backward(Mck)
            ctx.keep = (p, code, consts, (g, e1, e2, e1m1), rf.shape, gr.shape, rf.dtype, gr.dtype, every)
        return M

    @staticmethod
    def backward(ctx, grad_M):
        from .beffective import _fold_pulse_grad
        need_Mi, need_rf, need_gr = ctx.needs_input_grad[0:3]
        if not (need_Mi or need_rf or need_gr):
            return (None,) * 10
        lib = _lib.require_library()
        (Mck,) = ctx.saved_tensors
        p, code, consts, _alive, rf_shape, gr_shape, rf_dtype, gr_dtype, every = ctx.keep
        traj = every is not None
        # the precise adjoint divides by E once (as the reference's does at every step): refuse E == 0 HERE, where it
        # matters -- the forward succeeds as the reference's does; cached per constants
        _host.require_invertible_relaxation(code, _alive[1], _alive[2],
                                            'fused.blochsim_rfgr_traj' if traj else 'fused.blochsim_rfgr')
        device, dtype = Mck.device, Mck.dtype
        gM = grad_M.to(dtype).contiguous()      # the trajectory's: time-major, as the forward returned it -- free if so
        gMi = torch.empty((p.N,) + p.Nd + (3,), dtype=dtype, device=device) if need_Mi else None
        g_rf = torch.empty((p.N, 2, p.nT, p.nC), dtype=dtype, device=device) if need_rf else None
        g_gr = torch.empty((p.N, 3, p.nT), dtype=dtype, device=device) if need_gr else None
        outs = (gMi.data_ptr() if need_Mi else None, g_rf.data_ptr() if need_rf else None,
                g_gr.data_ptr() if need_gr else None)
        tr = (every,) if traj else ()
        if p.nC == 1:
            nbytes = int(lib.mrphy_blochsim_rfgr_bwd_workspace(code, p.N, p.nM, p.nT))
            name, nc = ('mrphy_blochsim_rfgr_traj_bwd' if traj else 'mrphy_blochsim_rfgr_bwd'), ()
        else:                                   # parallel transmit: per-coil sums in the kernel
            nbytes = int(lib.mrphy_blochsim_rfgr_mc_bwd_workspace(code, p.N, p.nM, p.nT, p.nC))
            name, nc = ('mrphy_blochsim_rfgr_mc_traj_bwd' if traj else 'mrphy_blochsim_rfgr_mc_bwd'), (p.nC,)
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            rc = getattr(lib, name)(code, Mck.data_ptr(), *p.k0_args(), *consts, gM.data_ptr(), *tr, *outs,
                                    work.data_ptr(), work.numel(), p.N, p.nM, p.nT, *nc,
                                    _host.current_stream(device))
        _lib.check(rc, name)
        return (gMi,
                _fold_pulse_grad(g_rf, rf_shape, rf_dtype, p.b1 is None) if need_rf else None,
                _fold_pulse_grad(g_gr, gr_shape, gr_dtype, False) if need_gr else None,
                None, None, None, None, None, None, None)


def _route(Mi, rf, gr, loc, every, kw):
    r"""The routing :func:`blochsim_rfgr` (``every = None``) and :func:`blochsim_rfgr_traj` share.  Returns
    ``('split', n1)``: a pulse gradient through the fused adjoint, but a length that is not a whole number of
    checkpoint segments -- the caller runs the first ``n1`` steps fused and composes the tail; ``('composed', None)``:
    a case the fused kernels do not cover (gradients w.r.t. the spin-side maps, fp64 with more than 8 coils, a pulse
    gradient the fused adjoint cannot form); or ``('fused', M)``, the result of :class:`BlochSimRfGrHIP`."""
    from . import beffective, sims
    _host.require_device_tensor(Mi, 'Mi')
    Δf, b1Map, T1, T2 = kw['Δf'], kw['b1Map'], kw['T1'], kw['T2']
    assert (T1 is None) == (T2 is None)
    lib = _lib.require_library()
    grad_on = torch.is_grad_enabled()
    rq = lambda x: grad_on and isinstance(x, Tensor) and x.requires_grad  # noqa: E731
    maps_grad = any(rq(x) for x in (loc, Δf, b1Map))
    pulse_grad = any(rq(x) for x in (Mi, rf, gr))
    p = beffective._PulseOnSpins(rf.detach(), gr.detach(), loc.detach(),
                                 None if Δf is None else Δf.detach(),
                                 None if b1Map is None else b1Map.detach(), kw['γ_beff'].detach())
    seg = int(lib.mrphy_blochsim_rfgr_ck_every())
    seg_ok = p.nT % seg == 0
    one_coil = p.nC == 1 and (rf.ndim == 3 or b1Map is not None or rf.shape[-1] == 1)
    ptx = 1 < p.nC <= int(lib.mrphy_blochsim_rfgr_mc_max_coils()) and p.b1 is not None
    fused_adjoint_ok = seg_ok and (one_coil or ptx)
    if pulse_grad and not maps_grad and not seg_ok and (one_coil or ptx) and p.nT > seg:
        return 'split', (p.nT // seg) * seg
    # fp64 with more than 8 transmit coils: the fused forward has no register build for it (it would spill),
    # the composed route does (k_rfgr2beff_steps / _pk + K1) and gives the same bits
    wide_f64 = (p.dtype == torch.float64 and p.nC > 8) or (p.b1 is not None and p.nC > 64)   # (> 64: coil-blocked K0 + K1)
    if maps_grad or wide_f64 or (pulse_grad and not fused_adjoint_ok):
        return 'composed', None

    device, dtype = Mi.device, Mi.dtype
    assert p.device == device and p.dtype == dtype, "Mi and loc must share device and dtype"
    assert tuple(Mi.shape[:-1]) == (p.N,) + p.Nd
    if kw['consts'] is not None:
        γ2πdt, E1, E2, E1_1 = (kw['consts'].get(k) for k in ('γ2πdt', 'E1', 'E2', 'E1_1'))
    else:
        γ2πdt, E1, E2, E1_1 = sims.relax_constants(T1, T2, kw['γ'], kw['dt'], 1 + len(p.Nd) + 2, device)
    return 'fused', BlochSimRfGrHIP.apply(Mi, rf, gr, p, γ2πdt, E1, E2, E1_1, pulse_grad and fused_adjoint_ok, every)


@_host.half_via_float
def blochsim_rfgr(
    Mi: Tensor, rf: Tensor, gr: Tensor, loc: Tensor, *,
    Δf: Optional[Tensor] = None, b1Map: Optional[Tensor] = None, γ_beff: Tensor = γH,
    T1: Optional[Tensor] = None, T2: Optional[Tensor] = None,
    γ: Tensor = γH, dt: Tensor = dt0, consts: Optional[dict] = None
) -> Tensor:
    r"""``blochsim(Mi, rfgr2beff(rf, gr, loc, Δf=Δf, b1Map=b1Map, γ=γ_beff), T1=T1, T2=T2,
    γ=γ, dt=dt)`` without the intermediate tensor, differentiable w.r.t. ``Mi``, ``rf``, ``gr``.

    ``Mi``: `(N, *Nd, xyz)`; the other arguments as in
    :func:`mrphy_amd.beffective.rfgr2beff` and :func:`mrphy_amd.sims.blochsim`.  ``consts``
    (``dict(γ2πdt=, E1=, E1_1=, E2=)``) replaces ``T1, T2, γ, dt`` as in
    :func:`mrphy_amd.sims.blochsim_consts`.
    """
    from . import beffective, sims
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
        return sims.blochsim(Mi, beff, T1=T1, T2=T2, γ=γ, dt=dt)
    return out


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
    history ``Mhst`` (``sims.py:83``).  Differentiable w.r.t. ``Mi``, ``rf``, ``gr`` (and, through the composed
    route, the spin-side maps); operands, dtypes, ``consts`` and the precision mode as :func:`blochsim_rfgr`.

    Layout: the result is a view ``.movedim(0, -2)`` of time-major storage `(nRec, N, *Nd, 3)` -- each record is
    one contiguous block, which the kernel writes with coalesced per-wave stores.  ``Mt.movedim(-2, 0)`` gives the
    contiguous tensor back; a loss that keeps that layout hands its gradient to the adjoint without a copy.

    The cases the fused adjoint does not cover (gradients w.r.t. ``loc``/``Δf``/``b1Map``, a parallel-transmit
    gradient with more coils than ``mrphy_blochsim_rfgr_mc_max_coils()``, fp64 with more than 8 coils) run one
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
