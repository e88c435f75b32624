r"""Fixture for ``fused.sequence_rfgr_jvp`` / ``fused.ab_sequence_jvp`` from the live reference (tianrluo/MRphy.py,
importable read-only where ``$MRPHY_REFERENCE`` points; the default is ``make_golden_ab_rfgr.REF``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sequence_jvp.py

writes ``tests/golden/sequence_jvp_f64.npz``: arrays only.  Problem: the inputs of ``sequence_f64.npz``
(``make_golden_sequence.py``: P = 3 pulses, N = 2, nT = 48, K = 24, its schedule, rests and phases), the first ``NM`` = 50
spins.  The inputs are not stored again: the test slices them from ``sequence_f64.npz``.

Stored: one seeded direction per group among ``T1, T2, Δf, b1Map, rf, rest`` (``dir.*``, each of the size of its operand)
and the tangent of the records along it with the other groups' tangents zero (``dMt.*`` `(N, NM, K, 3)`), by
``torch.autograd.functional.jvp`` through the reference's own operations in fp64: ``beffective.rfgr2beff`` ->
``beffective.beff2ab`` per bank entry, then per repetition ``slowsims.freeprec`` and ``slowsims.blochsim_ab`` between the
two rotations by the RF phase.  ``T1``, ``T2`` and ``Δf`` act in the pulses and in the rests.  The records of that route are
asserted to equal the stored ``Mt`` of ``sequence_f64.npz`` to 1e-12.  Runs only where the reference exists.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ab_rfgr import REF  # noqa: E402

NM = 50
SEED = 71
GROUPS = ('T1', 'T2', 'Δf', 'b1Map', 'rf', 'rest')
KEY = {'Δf': 'df', 'b1Map': 'b1'}                      # the group's name among the fixture's inputs
SCALE = dict(T1=0.01, T2=0.005, Δf=200.0, b1Map=1.0, rf=3.0, rest=6e-3)


def inputs():
    with np.load(os.path.join(HERE, 'sequence_f64.npz'), allow_pickle=False) as z:
        P = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('in.')}
        Mt = torch.from_numpy(z['Mt'])[:, :NM]
    for k in ('loc', 'df', 'b1', 'T1', 'T2'):
        P[k] = P[k][:, :NM].contiguous()
    gen = torch.Generator().manual_seed(SEED)
    V = {g: (torch.rand(P[KEY.get(g, g)].shape, generator=gen, dtype=torch.float64) * 2 - 1) * SCALE[g] for g in GROUPS}
    return P, V, Mt


def rz(M, φ):
    c, s = torch.cos(φ)[:, None], torch.sin(φ)[:, None]
    return torch.stack((c * M[..., 0] - s * M[..., 1], s * M[..., 0] + c * M[..., 1], M[..., 2]), dim=-1)


def records(ref, P):
    r"""``Mt`` `(N, NM, K, 3)` by the reference's operations on the inputs ``P``."""
    E1, E2 = torch.exp(-P['dt'][:, None] / P['T1']), torch.exp(-P['dt'][:, None] / P['T2'])
    bank = [ref.beffective.beff2ab(ref.beffective.rfgr2beff(P['rf'][p], P['gr'], P['loc'], Δf=P['df'], b1Map=P['b1'],
                                                            γ=P['γ']), E1=E1, E2=E2, γ=P['γ'], dt=P['dt'])
            for p in range(P['rf'].shape[0])]
    M = torch.zeros(P['loc'].shape, dtype=P['loc'].dtype)
    M[..., 2] = 1
    out = []
    for k, p in enumerate(P['pulse'].tolist()):
        φ = P['phase'][:, k]
        Mm = ref.slowsims.freeprec(M, P['rest'][:, k], T1=P['T1'], T2=P['T2'], Δf=P['df'])
        M = rz(ref.slowsims.blochsim_ab(rz(Mm, -φ), *bank[p]), φ)
        out.append(M)
    return torch.stack(out, dim=-2)


def main():
    sys.path.insert(0, REF)
    import mrphy as ref
    P, V, Mt = inputs()
    z = {f'dir.{g}': V[g].numpy() for g in GROUPS}
    for g in GROUPS:
        got, dMt = torch.autograd.functional.jvp(lambda x: records(ref, dict(P, **{KEY.get(g, g): x})), P[KEY.get(g, g)], V[g])
        d = float((got - Mt).abs().max())
        assert d <= 1e-12, d
        z[f'dMt.{g}'] = dMt.numpy()
        print(f'  {g:6s} |dMt| / |Mt| = {float(dMt.norm() / got.norm()):.3e}   records vs sequence_f64.npz {d:.1e}')
    path = os.path.join(HERE, 'sequence_jvp_f64.npz')
    np.savez_compressed(path, **z)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
