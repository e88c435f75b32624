r"""Fixtures for ``fused.steadystate_rfgr`` from the live reference (tianrluo/MRphy.py, importable read-only where
``$MRPHY_REFERENCE`` points; the default is ``make_golden_ab_rfgr.REF``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_steadystate.py

writes ``tests/golden/steadystate_f32.npz`` and ``steadystate_f64.npz``: inputs and outputs only.  Problem: the amplitudes
of ``make_golden_ab_rfgr.inputs()`` (N = 2, nM = 100, nT = 48, one transmit coil with a ``b1Map``, ``Δf``), with
T1 in [0.05, 0.15] s, T2 in [0.02, 0.07] s, a rest of (5 ms, 6.5 ms) per batch entry before each pulse, and the weights
``w = sin(0.37 i + 0.3)`` of the loss ``(Mss w).sum()``.

Expected ``Mss`` (fp64): the reference's own ``sims.freeprec`` -> ``sims.blochsim`` iterated from ``[0, 0, 1]`` until the
last period's move bounds the distance left to the fixed point by 1e-13 (``iterated``; at most 2000 periods; asserted).  Expected ``grad_rf``, ``grad_gr``
(fp64): autograd through the reference's ``rfgr2beff`` -> ``beff2ab`` and ``torch.linalg.solve`` of
``(I - A F) Mss = A f + B``; this closed form is asserted to equal the iterated state to 1e-12.  The fp32 file holds
the reference's closed-form run in fp32 on the fp32 inputs, and its relative L2 distances from the fp64 run on the
same numbers as ``distance_f32_vs_f64.*``: what an all-fp32 route of the reference's own operations loses to the
conditioning of ``I - A F`` (``kappa_max``, asserted <= 100), the yardstick of the fp32 end-to-end test.

Last run: 685 periods, closed form vs iterated 9.3e-14 max abs, kappa_max 44.3; reference fp32 vs its fp64 run on the
same inputs: Mss 3.246e-06, grad_rf 2.492e-06, grad_gr 3.554e-06.
"""
import os
import sys
from math import pi as π

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ab_rfgr import N, NM, REF, inputs as ab_inputs, rel_l2  # noqa: E402

SEED = 31
MAX_PERIODS = 2000


def inputs():
    r"""The problem in fp64."""
    P = {k: v for k, v in ab_inputs().items() if k in ('rf', 'gr', 'loc', 'df', 'b1', 'γ', 'dt')}
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    P['T1'], P['T2'] = 0.05 + 0.1 * rnd(N, NM), 0.02 + 0.05 * rnd(N, NM)
    P['E1'], P['E2'] = torch.exp(-P['dt'][:, None] / P['T1']), torch.exp(-P['dt'][:, None] / P['T2'])
    P['rest'] = torch.tensor([5e-3, 6.5e-3], dtype=torch.float64)
    P['w'] = torch.sin(torch.arange(N * NM * 3, dtype=torch.float64) * 0.37 + 0.3).reshape(N, NM, 3)
    return P


def rest_period(P):
    r"""``F`` (N, nM, 3, 3), ``f`` (N, nM, 3) of ``sims.freeprec(M, rest, T1, T2, Δf)``: ``M⁻ = F M + f``."""
    rest = P['rest'][:, None]
    φ = -2 * π * P['df'] * rest
    E1r, E2r, c, s = torch.exp(-rest / P['T1']), torch.exp(-rest / P['T2']), torch.cos(φ), torch.sin(φ)
    o = torch.zeros_like(c)
    F = torch.stack((torch.stack((E2r * c, -E2r * s, o), -1), torch.stack((E2r * s, E2r * c, o), -1),
                     torch.stack((o, o, E1r), -1)), -2)
    return F, torch.stack((o, o, -torch.expm1(-rest / P['T1'])), -1)


def closed_form(ref, P):
    r"""``Mss, grad_rf, grad_gr, kappa`` by the reference's ``rfgr2beff`` -> ``beff2ab`` and ``torch.linalg.solve``, with
    autograd through all of it, in the dtype of ``P``."""
    rf, gr = P['rf'].clone().requires_grad_(True), P['gr'].clone().requires_grad_(True)
    beff = ref.beffective.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = ref.beffective.beff2ab(beff, E1=P['E1'], E2=P['E2'], γ=P['γ'], dt=P['dt'])
    F, f = rest_period(P)
    C = torch.eye(3, dtype=A.dtype) - A @ F
    Mss = torch.linalg.solve(C, (A @ f[..., None])[..., 0] + B)
    (Mss * P['w']).sum().backward()
    return dict(Mss=Mss.detach(), grad_rf=rf.grad, grad_gr=gr.grad), float(torch.linalg.cond(C.detach().double()).max())


def iterated(ref, P):
    r"""The state right after the pulse that ``freeprec`` -> ``blochsim`` converges to from ``[0, 0, 1]``.  The period
    contracts by at most ``ρ = max exp(-TR/T1)`` (0.966 here), so a last move of ``step`` leaves the state up to
    ``step ρ / (1 - ρ)`` from the fixed point -- 28 steps' worth: the iteration stops when THAT is below 1e-13."""
    ρ = float(torch.exp(-(P['rest'][:, None] + P['rf'].shape[2] * P['dt'][:, None]) / P['T1']).max())
    with torch.no_grad():
        beff = ref.beffective.rfgr2beff(P['rf'], P['gr'], P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
        M = torch.zeros((N, NM, 3), dtype=torch.float64)
        M[..., 2] = 1
        for n in range(1, MAX_PERIODS + 1):
            M1 = ref.sims.blochsim(ref.sims.freeprec(M, P['rest'], T1=P['T1'], T2=P['T2'], Δf=P['df']), beff,
                                   T1=P['T1'], T2=P['T2'], γ=P['γ'], dt=P['dt'])
            step = float((M1 - M).abs().max())
            M = M1
            if step * ρ / (1 - ρ) < 1e-13:
                return M, n
    raise AssertionError(f'no steady state within {MAX_PERIODS} periods: the last one moved the state by {step:.1e}')


def main():
    sys.path.insert(0, REF)
    import mrphy as ref
    P64 = inputs()
    P32 = {k: v.float() for k, v in P64.items()}
    out64, κ = closed_form(ref, P64)
    Mit, n = iterated(ref, P64)
    d = float((out64['Mss'] - Mit).abs().max())
    print(f'{n} periods; closed form vs iterated: {d:.1e} max abs; kappa_max {κ:.1f}')
    assert d <= 1e-12 and κ <= 100
    out64['Mss'] = Mit
    out32, κ32 = closed_form(ref, P32)
    assert all(v.dtype == torch.float32 for v in out32.values())
    out32_wide, _ = closed_form(ref, {k: v.double() for k, v in P32.items()})      # fp64 on the SAME numbers
    dist = {k: rel_l2(out32[k], out32_wide[k]) for k in out32}
    print('reference fp32 vs its fp64 run on the same inputs (relative L2):')
    for k, v in dist.items():
        print(f'  {k:8s} {v:.3e}')
    for tag, P, out in (('f32', P32, out32), ('f64', P64, out64)):
        z = {f'in.{k}': v.numpy() for k, v in P.items()}
        z.update({k: v.numpy() for k, v in out.items()})
        z['kappa_max'] = np.float64(κ)
        if tag == 'f32':
            z.update({f'distance_f32_vs_f64.{k}': np.float64(v) for k, v in dist.items()})
        path = os.path.join(HERE, f'steadystate_{tag}.npz')
        np.savez_compressed(path, **z)
        print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
