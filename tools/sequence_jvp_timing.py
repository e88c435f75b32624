r"""What ``fused.ab_sequence_jvp`` (Ksqj) costs next to the route there was before it: the ``2·D`` calls of
``fused.ab_sequence`` of a central difference.

    python tools/sequence_jvp_timing.py [--n 64] [--K 256] [--P 16] [--reps 10] [--out FILE.json]

Shape and problem: ``tools/ab_sequence_timing.py``'s (n^3 spins x K repetitions of a bank of P pulses, its sinusoidal
flip-angle schedule quantised to the bank, its rests between 8 and 12 ms, the quadratic phase schedule), fp32.
``D = 4`` directions: "all ones" in ``T1``, in ``T2`` and in ``Δf`` (the per-spin sensitivity maps) and a seeded tangent
``dA, dB`` of the whole bank.  Routes, alternating in one process:

  (jvp) one ``fused.ab_sequence_jvp`` call: ``Mt`` and ``dMt`` `(4, N, nM, K, 3)`;
  (fd8) the eight ``fused.ab_sequence`` forwards of a central difference on operands perturbed beforehand (forming
        them and the four differences is NOT timed: the comparison favours this route), each result dropped at once;
  (fwd) one ``fused.ab_sequence`` forward, for scale.

HIP events around each route (the Python layer included), three warm-up rounds, then ``--reps`` rounds; per route the
median, min, max and quartiles and the allocator's peak above what was held before the call.  The kernels alone: HIP
events around every entry-point call inside the routes (``fused._launch`` wrapped), summed per route and round.  The one
condition of the feature: the range (min - max) of (jvp) lies wholly below that of (fd8).  Then, per direction, the
relative L2 distance of the central difference from Ksqj's tangent over a ladder of steps and the best of them.
Nothing is asserted: the file records what comes out.  Needs the GPU; there is no other path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrphy_amd import fused  # noqa: E402
from ab_sequence_timing import problem, rel_l2  # noqa: E402

DIRS = ('T1', 'T2', 'Δf', 'A,B')
STEPS = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4)         # relative to the operand's largest |element|


def directions(P, dev, dtype):
    r"""The tangents of the four directions: ones `(4, 1, 1)` in ``T1, T2, Δf`` and a seeded ``dA, dB`` of the bank."""
    gen = torch.Generator().manual_seed(12)
    one = lambda i: torch.eye(4, dtype=dtype, device=dev)[:, i].reshape(4, 1, 1)  # noqa: E731
    dA = torch.zeros((4,) + tuple(P['A'].shape), dtype=dtype, device=dev)
    dB = torch.zeros((4,) + tuple(P['B'].shape), dtype=dtype, device=dev)
    dA[3] = torch.randn(P['A'].shape, generator=gen, dtype=torch.float64).to(device=dev, dtype=dtype)
    dB[3] = 0.1 * torch.randn(P['B'].shape, generator=gen, dtype=torch.float64).to(device=dev, dtype=dtype)
    return {'T1': one(0), 'T2': one(1), 'Δf': one(2), 'A': dA, 'B': dB}


def perturbed(P, tan, d, h):
    r"""The operands of ``ab_sequence`` moved by ``±h`` along direction ``d`` (``h`` absolute)."""
    out = []
    for s in (1.0, -1.0):
        q = dict(A=P['A'], B=P['B'], T1=P['T1'], T2=P['T2'], Δf=P['df'])
        for k in (('T1',), ('T2',), ('Δf',), ('A', 'B'))[d]:
            q[k] = q[k] + s * h * tan[k][d]
        out.append(q)
    return out


def scale_of(P, d):
    return float(max(P[k].abs().max() for k in (('T1',), ('T2',), ('df',), ('A', 'B'))[d]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--P', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_jvp_timing.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/sequence_jvp_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev, dtype = torch.device('cuda:0'), torch.float32
    P = problem(args.n, args.K, args.P, dtype, dev)
    tan = directions(P, dev, dtype)
    kw = dict(pulse=P['pulse'], phase=P['phase'], rest=P['rest'])
    fd_ops = [q for d in range(4) for q in perturbed(P, tan, d, 1e-2 * scale_of(P, d))]

    # the kernels alone: events around every entry-point call
    spans, launch = [], fused._launch

    def timed_launch(*a):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch(*a)
        t1.record()
        spans.append((t0, t1))
    fused._launch = timed_launch

    def jvp():
        fused.ab_sequence_jvp(P['A'], P['B'], tangents=tan, T1=P['T1'], T2=P['T2'], Δf=P['df'], **kw)

    def fd8():
        for q in fd_ops:
            fused.ab_sequence(**q, **kw)

    def fwd():
        fused.ab_sequence(P['A'], P['B'], T1=P['T1'], T2=P['T2'], Δf=P['df'], **kw)

    runs = {'jvp': jvp, 'fd8': fd8, 'fwd': fwd}
    times, kernels, peaks = {k: [] for k in runs}, {k: [] for k in runs}, {}
    with torch.no_grad():
        for r in range(3 + args.reps):
            for k, run in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                del spans[:]
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                peaks[k] = torch.cuda.max_memory_allocated() - base
                if r >= 3:
                    times[k].append(t0.elapsed_time(t1))
                    kernels[k].append(sum(a.elapsed_time(b) for a, b in spans))
    fused._launch = launch

    def stats(ts):
        q = statistics.quantiles(ts, n=4)
        return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0], 'q3_ms': q[2]}
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'K': args.K, 'P': args.P, 'reps': args.reps,
           'dtype': 'float32', 'directions': list(DIRS), 'record_bytes': args.K * args.n ** 3 * 3 * 4,
           'bank_entries_played': len(set(P['pulse'])), 'routes': {}}
    for k in runs:
        res['routes'][k] = dict(stats(times[k]), kernels_only=stats(kernels[k]), peak_bytes_above_inputs=peaks[k])
    j, f = res['routes']['jvp'], res['routes']['fd8']
    res['jvp_over_fd8'] = j['median_ms'] / f['median_ms']
    res['kernels_jvp_over_fd8'] = j['kernels_only']['median_ms'] / f['kernels_only']['median_ms']
    res['condition_jvp_range_wholly_below_fd8'] = j['max_ms'] < f['min_ms']
    print({k: (round(v['median_ms'], 3), round(v['min_ms'], 3), round(v['max_ms'], 3), 'kernels',
               round(v['kernels_only']['median_ms'], 3)) for k, v in res['routes'].items()},
          'condition met:', res['condition_jvp_range_wholly_below_fd8'], flush=True)

    # the central difference's distance from the tangent, per direction over a ladder of steps
    with torch.no_grad():
        _, dMt = fused.ab_sequence_jvp(P['A'], P['B'], tangents=tan, T1=P['T1'], T2=P['T2'], Δf=P['df'], **kw)
        res['central_difference'] = {}
        for d, name in enumerate(DIRS):
            ladder = {}
            for s in STEPS:
                h = s * scale_of(P, d)
                plus, minus = perturbed(P, tan, d, h)
                fd = (fused.ab_sequence(**plus, **kw).double() - fused.ab_sequence(**minus, **kw).double()) / (2 * h)
                ladder[f'{s:g}'] = rel_l2(fd, dMt[d])
                del fd
            best = min(ladder, key=ladder.get)
            res['central_difference'][name] = {'rel_l2_by_relative_step': ladder, 'best_step': best, 'best': ladder[best]}
            print(name, 'central difference, best step', best, f'{ladder[best]:.3e}', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f_:
        json.dump(res, f_, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
