r"""Fixtures for ``fused.ab_rfgr`` from the live reference (tianrluo/MRphy.py, importable read-only where
``$MRPHY_REFERENCE`` points, by default /root/reference): its own ``beffective.rfgr2beff`` -> ``beffective.beff2ab`` and
its own autograd through both, on one small problem.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ab_rfgr.py

writes ``tests/golden/ab_rfgr_f32.npz`` and ``ab_rfgr_f64.npz``: the inputs (seeded / closed formulas, below), the
weights ``wA``, ``wB``, and the reference's ``A``, ``B`` and ``grad_rf``, ``grad_gr`` of the loss
``(A wA).sum() + (B wB).sum()``.  Case: N = 2, nM = 100, nT = 48, one transmit coil with a ``b1Map``, ``Δf`` and per-spin
``E1``, ``E2``.  Runs only where the reference exists (never on the GPU box); only inputs and outputs are stored.

Condition checked here, and printed: the reference's own fp32 result on the fp32 inputs lies within a tenth of the
fp32 gate (relative L2 1e-6) of its fp64 result on the same numbers, for each of the four outputs -- so a kernel held
to 1e-5 against the fp32 fixture is held to the function, not to the reference's rounding.  Last run: A 4.0e-7,
B 2.4e-7, grad_rf 5.4e-7, grad_gr 8.3e-7 (also stored as ``distance_f32_vs_f64.*`` in ``ab_rfgr_f32.npz``).
"""
import os
import sys
from math import pi as π

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MRPHY_REFERENCE', '/root/reference')
N, NM, NT = 2, 100, 48
SEED = 20
GATE32 = 1e-5


def inputs():
    r"""The problem in fp64: the amplitudes of ``tests/test_fused_traj._problem`` (rf up to 3 G, gr up to 1 G/cm, loc up to
    6 cm, Δf up to 200 Hz, |b1| up to 1.4), dt = 4 us."""
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    P = dict(rf=(rnd(N, 2, NT) * 2 - 1) * 3, gr=rnd(N, 3, NT) * 2 - 1, loc=(rnd(N, NM, 3) * 2 - 1) * 6,
             df=(rnd(N, NM) * 2 - 1) * 200, b1=rnd(N, NM, 2) * 2 - 1)
    P['γ'], P['dt'] = torch.tensor(4257.6, dtype=torch.float64), torch.tensor([4e-6], dtype=torch.float64)
    T1, T2 = 0.5 + rnd(N, NM), 0.02 + 0.1 * rnd(N, NM)
    P['E1'], P['E2'] = torch.exp(-P['dt'][:, None] / T1), torch.exp(-P['dt'][:, None] / T2)
    idx = lambda n: torch.arange(n, dtype=torch.float64)  # noqa: E731
    P['wA'] = torch.sin(idx(N * NM * 9) * 0.61 + 1).reshape(N, NM, 3, 3)
    P['wB'] = torch.sin(idx(N * NM * 3) * 0.37 + 0.3).reshape(N, NM, 3)
    return P


def reference_run(ref, P):
    r"""``A, B, grad_rf, grad_gr`` by the reference's own functions and autograd, in the dtype of ``P``."""
    rf, gr = P['rf'].clone().requires_grad_(True), P['gr'].clone().requires_grad_(True)
    beff = ref.beffective.rfgr2beff(rf, gr, P['loc'], Δf=P['df'], b1Map=P['b1'], γ=P['γ'])
    A, B = ref.beffective.beff2ab(beff, E1=P['E1'], E2=P['E2'], γ=P['γ'], dt=P['dt'])
    ((A * P['wA']).sum() + (B * P['wB']).sum()).backward()
    return dict(A=A.detach(), B=B.detach(), grad_rf=rf.grad, grad_gr=gr.grad)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    sys.path.insert(0, REF)
    import mrphy as ref
    P64 = inputs()
    P32 = {k: v.float() for k, v in P64.items()}
    out32 = reference_run(ref, P32)
    assert all(v.dtype == torch.float32 for v in out32.values()), {k: v.dtype for k, v in out32.items()}
    out32_wide = reference_run(ref, {k: v.double() for k, v in P32.items()})      # fp64 on the SAME numbers
    dist = {k: rel_l2(out32[k], out32_wide[k]) for k in out32}
    print('reference fp32 vs its fp64 run on the same inputs (relative L2; a tenth of the gate is %.0e):' % (GATE32 / 10))
    for k, d in dist.items():
        print(f'  {k:8s} {d:.3e}')
    assert max(dist.values()) <= GATE32 / 10, 'lower the amplitudes: the fp32 fixture is not the function to a tenth of the gate'
    for tag, P, out in (('f32', P32, out32), ('f64', P64, reference_run(ref, P64))):
        z = {f'in.{k}': v.numpy() for k, v in P.items()}
        z.update({k: v.numpy() for k, v in out.items()})
        if tag == 'f32':
            z.update({f'distance_f32_vs_f64.{k}': np.float64(d) for k, d in dist.items()})
        path = os.path.join(HERE, f'ab_rfgr_{tag}.npz')
        np.savez_compressed(path, **z)
        print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
