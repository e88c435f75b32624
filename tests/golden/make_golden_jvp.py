r"""Fixture for ``fused.blochsim_rfgr_jvp`` from the live reference (tianrluo/MRphy.py, importable read-only where
``$MRPHY_REFERENCE`` points, by default /root/reference): forward-mode tangents of its own ``beffective.rfgr2beff`` ->
``slowsims.blochsim`` under ``torch.autograd.functional.jvp``, in fp64, on one small problem.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jvp.py

writes ``tests/golden/jvp_f64.npz``: the inputs (seeded, the amplitudes of ``make_golden_ab_rfgr.py``), one seeded direction
per group -- ``Mi, rf, gr, loc, Δf, b1Map, T1, T2``, eight in all -- the reference's ``Mo`` and one ``dMo`` per group, the
other groups' tangents zero.  Case: N = 2, nM = 130, nT = 48, one transmit coil with a ``b1Map``, ``Δf`` and per-spin
``T1``, ``T2``.  Runs only where the reference exists (never on the GPU box); only arrays are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MRPHY_REFERENCE', '/root/reference')
N, NM, NT = 2, 130, 48
SEED = 31
GROUPS = ('Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'T1', 'T2')


def inputs():
    r"""The problem in fp64 (rf up to 3 G, gr up to 1 G/cm, loc up to 6 cm, Δf up to 200 Hz, |b1| up to 1.4, dt = 4 us) and
    one direction per group, each of the size of its operand."""
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    P = dict(Mi=rnd(N, NM, 3), rf=(rnd(N, 2, NT) * 2 - 1) * 3, gr=rnd(N, 3, NT) * 2 - 1, loc=(rnd(N, NM, 3) * 2 - 1) * 6,
             Δf=(rnd(N, NM) * 2 - 1) * 200, b1Map=rnd(N, NM, 2) * 2 - 1, T1=0.5 + rnd(N, NM), T2=0.02 + 0.1 * rnd(N, NM))
    P['γ'], P['dt'] = torch.tensor(4257.6, dtype=torch.float64), torch.tensor([4e-6], dtype=torch.float64)
    scale = dict(Mi=1.0, rf=3.0, gr=1.0, loc=6.0, Δf=200.0, b1Map=1.0, T1=1.0, T2=0.1)
    V = {k: (rnd(*P[k].shape) * 2 - 1) * scale[k] for k in GROUPS}
    return P, V


def simulate(ref, P, **over):
    q = dict(P, **over)
    beff = ref.beffective.rfgr2beff(q['rf'], q['gr'], q['loc'], Δf=q['Δf'], b1Map=q['b1Map'], γ=q['γ'])
    return ref.slowsims.blochsim(q['Mi'].clone(), beff, T1=q['T1'], T2=q['T2'], γ=q['γ'], dt=q['dt'])


def main():
    sys.path.insert(0, REF)
    import mrphy as ref
    P, V = inputs()
    z = {f'in.{k}': v.numpy() for k, v in P.items()}
    z.update({f'dir.{k}': v.numpy() for k, v in V.items()})
    for k in GROUPS:
        Mo, dMo = torch.autograd.functional.jvp(lambda x: simulate(ref, P, **{k: x}), P[k], V[k])
        z[f'dMo.{k}'] = dMo.numpy()
        print(f'  {k:6s} |dMo| / |Mo| = {float(dMo.norm() / Mo.norm()):.3e}')
    z['Mo'] = Mo.numpy()
    path = os.path.join(HERE, 'jvp_f64.npz')
    np.savez_compressed(path, **z)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
