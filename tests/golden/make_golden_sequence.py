r"""Fixtures for ``fused.sequence_rfgr`` from the live reference (tianrluo/MRphy.py, importable read-only where
``$MRPHY_REFERENCE`` points; the default is ``make_golden_ab_rfgr.REF``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sequence.py

writes ``tests/golden/sequence_f32.npz`` and ``sequence_f64.npz``: inputs and outputs only.  Problem: the amplitudes of
``make_golden_ab_rfgr.inputs()`` (N = 2, nM = 100, nT = 48, one transmit coil with a ``b1Map``, ``Δf``) as a bank of
P = 3 pulses -- its ``rf`` scaled by (1, 0.5, 1.6), one ``gr`` for all --, T1 in [10, 20] ms, T2 in [5, 10] ms (the same
in the pulses and in the rests), K = 24 repetitions from ``[0, 0, 1]`` by the schedule ``PULSE`` (single repetitions,
runs of two, returns to entries played before), a rest ``rest[n, k]`` seeded in [2, 8] ms before each pulse with
``rest[:, 5] = rest[:, 4]`` and ``rest[:, 9] = 0``, the RF phase ``φ_k = 117° k (k + 1) / 2`` for batch entry 0 and
``φ_k = 0.7 k`` rad for entry 1 (both stored modulo 2π), and the weights ``w = sin(0.37 i + 0.3)`` over the time-major
records `(K, N, nM, 3)` of the loss ``(Mt w).sum()``.

Expected ``Mt`` `(N, nM, K, 3)`: the reference's own ``sims.freeprec(M, rest[:, k])`` ->
``beffective.rfgr2beff(rf[pulse_k] e^{iφ_k}, ...)`` -> ``sims.blochsim``, per repetition.  Expected ``grad_rf`` (of the
bank), ``grad_gr``, ``grad_T1``, ``grad_rest`` `(N, K)`: the reference's autograd through its plain differentiable
operations of the same train -- ``slowsims.freeprec`` -> ``rfgr2beff`` -> ``beffective.beff2ab`` ->
``slowsims.blochsim_ab`` --, whose records are asserted to equal the simulated ones to 1e-12.  The fp32 file holds the
same two runs in fp32 on the fp32 inputs, and their relative L2 distances from the fp64 run on the same numbers as
``distance_f32_vs_f64.*``, as ``make_golden_train.py`` stores them.

Last run: differentiable route vs simulated records 4.0e-15 max abs; reference fp32 vs its fp64 run on the same inputs:
Mt 1.599e-06, grad_rf 1.854e-06, grad_gr 2.368e-06, grad_T1 1.991e-06, grad_rest 2.033e-06.
"""
import os
import sys
from math import pi as π

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ab_rfgr import N, NM, REF, inputs as ab_inputs, rel_l2  # noqa: E402
from make_golden_train import rotated  # noqa: E402

SEED = 53
K = 24
SCALES = (1.0, 0.5, 1.6)
PULSE = (0, 1, 1, 2, 0, 0, 2, 2, 1, 0, 2, 1, 1, 0, 0, 2, 1, 2, 2, 0, 1, 0, 1, 2)


def inputs():
    r"""The problem in fp64 (``pulse`` int64)."""
    P = {k: v for k, v in ab_inputs().items() if k in ('rf', 'gr', 'loc', 'df', 'b1', 'γ', 'dt')}
    P['rf'] = torch.stack([s * P['rf'] for s in SCALES])
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    P['T1'], P['T2'] = 0.01 + 0.01 * rnd(N, NM), 0.005 + 0.005 * rnd(N, NM)
    P['rest'] = 2e-3 + 6e-3 * rnd(N, K)
    P['rest'][:, 5] = P['rest'][:, 4]
    P['rest'][:, 9] = 0
    k = torch.arange(K, dtype=torch.float64)
    P['phase'] = torch.remainder(torch.stack((117 * π / 180 * k * (k + 1) / 2, 0.7 * k)), 2 * π)
    P['pulse'] = torch.tensor(PULSE, dtype=torch.int64)
    P['w'] = torch.sin(torch.arange(K * N * NM * 3, dtype=torch.float64) * 0.37 + 0.3).reshape(K, N, NM, 3)
    return P


def cast(P, dtype):
    return {k: (v if k == 'pulse' else v.to(dtype)) for k, v in P.items()}


def simulated(ref, P):
    r"""``Mt`` `(N, nM, K, 3)` by the reference's simulators, in the dtype of ``P``."""
    with torch.no_grad():
        M = torch.zeros((N, NM, 3), dtype=P['rf'].dtype)
        M[..., 2] = 1
        out = []
        for k in range(K):
            rf = rotated(P['rf'][int(P['pulse'][k])], P['phase'][:, k])
            beff = ref.beffective.rfgr2beff(rf, P['gr'], P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
            M = ref.sims.blochsim(ref.sims.freeprec(M, P['rest'][:, k], T1=P['T1'], T2=P['T2'], Δf=P['df']), beff,
                                  T1=P['T1'], T2=P['T2'], γ=P['γ'], dt=P['dt'])
            out.append(M)
    return torch.stack(out, dim=-2)


def differentiable(ref, P):
    r"""``Mt`` and the gradients of ``(Mt w).sum()`` by the reference's plain torch operations and autograd."""
    rf, gr, T1, rest = (P[k].clone().requires_grad_(True) for k in ('rf', 'gr', 'T1', 'rest'))
    E1, E2 = torch.exp(-P['dt'][:, None] / T1), torch.exp(-P['dt'][:, None] / P['T2'])
    M = torch.zeros((N, NM, 3), dtype=rf.dtype)
    M[..., 2] = 1
    out = []
    for k in range(K):
        beff = ref.beffective.rfgr2beff(rotated(rf[int(P['pulse'][k])], P['phase'][:, k]), gr, P['loc'], Δf=P['df'],
                                        b1Map=P['b1'], γ=P['γ'])
        A, B = ref.beffective.beff2ab(beff, E1=E1, E2=E2, γ=P['γ'], dt=P['dt'])
        M = ref.slowsims.blochsim_ab(ref.slowsims.freeprec(M, rest[:, k], T1=T1, T2=P['T2'], Δf=P['df']), A, B)
        out.append(M)
    Mt = torch.stack(out, dim=0)
    (Mt * P['w']).sum().backward()
    return dict(Mt=Mt.detach().movedim(0, -2), grad_rf=rf.grad, grad_gr=gr.grad, grad_T1=T1.grad, grad_rest=rest.grad)


def run(ref, P):
    out = differentiable(ref, P)
    sim = simulated(ref, P)
    d = float((out['Mt'] - sim).abs().max())
    out['Mt'] = sim.contiguous()
    return out, d


def main():
    sys.path.insert(0, REF)
    import mrphy as ref
    P64 = inputs()
    P32 = cast(P64, torch.float32)
    out64, d = run(ref, P64)
    print(f'differentiable route vs simulated records: {d:.1e} max abs')
    assert d <= 1e-12
    out32, _ = run(ref, P32)
    assert all(v.dtype == torch.float32 for v in out32.values())
    out32_wide, _ = run(ref, cast(P32, torch.float64))                     # fp64 on the SAME numbers
    dist = {k: rel_l2(out32[k], out32_wide[k]) for k in out32}
    print('reference fp32 vs its fp64 run on the same inputs (relative L2):')
    for k, v in dist.items():
        print(f'  {k:9s} {v:.3e}')
    for tag, P, out in (('f32', P32, out32), ('f64', P64, out64)):
        z = {f'in.{k}': v.numpy() for k, v in P.items()}
        z.update({k: v.numpy() for k, v in out.items()})
        if tag == 'f32':
            z.update({f'distance_f32_vs_f64.{k}': np.float64(v) for k, v in dist.items()})
        path = os.path.join(HERE, f'sequence_{tag}.npz')
        np.savez_compressed(path, **z)
        print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
