r"""What ``fused.train_signal`` costs next to the route users had before it: ``fused.ab_train`` followed by the product
with the receive map and the sum over the spins in torch.

    python tools/train_signal_timing.py [--n 64] [--K 256] [--reps 10] [--out FILE.json]
    python tools/train_signal_timing.py --kernels-only              (the program to put under rocprofv3 --kernel-trace)
    python tools/train_signal_timing.py --trace DIR [--out FILE]    (condense that trace: Ktrs / Ktrsb alone)

Shape: n^3 spins x K repetitions, fp32 and fp64, the problem of ``tools/ab_train_timing.py`` (seeded ``A = 0.97 Q``,
``B``, per-spin ``T1, T2, Δf``, a rest of 5 ms, the quadratic 117° phase schedule, from ``(0, 0, 1)``) with a seeded
complex receive map of 1 and of 8 coils; the forward alone (``torch.no_grad``) and forward + backward of
``(sig w).sum()`` w.r.t. ``A, B, T1, T2``.  Contenders, in the same process at the same commit:

  ``fused``     ``fused.train_signal`` (Ktrs / Ktrsb and their second passes);
  ``composed``  ``fused.ab_train`` (Ktr / Ktrb) and ``fused._signal_of`` on its time-major records.

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the contenders; reported per contender: median, min, max and the quartiles of the rounds, the allocator's
peak above what was allocated before the call, and the relative L2 distance of ``fused``'s results from ``composed``'s.
These times include the Python layer; ``--kernels-only`` runs ``fused`` alone, 8 x forward + backward per data type and
coil count, for the kernels' own durations.  Nothing is asserted: the file records what comes out.  Needs the GPU.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrphy_amd import fused  # noqa: E402
from ab_train_timing import REST, problem, rel_l2, rounds  # noqa: E402

COILS = (1, 8)
WRT = ['A', 'B', 'T1', 'T2']


def receiver(P, n, K, nRx, dtype, dev):
    gen = torch.Generator().manual_seed(11)
    rx = (0.5 + torch.randn((1, n ** 3, 2, nRx), generator=gen, dtype=torch.float64)).to(device=dev, dtype=dtype)
    w = torch.sin(torch.arange(2 * K * nRx, dtype=torch.float64, device=dev) * 0.37 + 0.3).to(dtype).reshape(1, 2, K, nRx)
    return rx, w


def contenders(P, rx, w):
    last = {}
    kw = dict(phase=P['phase'], rest=P['rest'], Δf=P['df'])

    def run_fused(A, B, T1, T2):
        last['fused'] = sig = fused.train_signal(A, B, T1=T1, T2=T2, rx=rx, **kw)
        return (sig * w).sum()

    def run_composed(A, B, T1, T2):
        Mt = fused.ab_train(A, B, T1=T1, T2=T2, **kw).movedim(-2, 0)
        last['composed'] = sig = fused._signal_of(Mt, rx)
        return (sig * w).sum()

    return {'fused': run_fused, 'composed': run_composed}, last


def condense(trace_dir, out):
    r"""Durations of the kernels of tu_train_signal.hip from a ``rocprofv3 --kernel-trace --output-format csv`` directory:
    per kernel, in launch order, the median of all but the first two launches and (min - max) of all."""
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r['Kernel_Name']
            if 'k_train_signal' not in name:
                continue
            short = name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            t0, t1 = int(r['Start_Timestamp']), int(r['End_Timestamp'])
            rows.setdefault(short, []).append((t0, (t1 - t0) / 1e6))
    res = {'tool': 'rocprofv3 --kernel-trace -- python tools/train_signal_timing.py --kernels-only',
           'shape': '64^3 spins x K = 256, N = 1; gradients w.r.t. A, B, T1, T2; 1 and 8 receive coils',
           'method': '8 launches of each kernel per data type and coil count in one process; median of the last 6, '
                     '(min - max) of all 8; kernel durations only',
           'kernels': {}}
    for name, xs in sorted(rows.items()):
        ms = [d for _, d in sorted(xs)]
        # the second pass serves every coil count and both outputs under one name: kept as one list, in launch order
        res['kernels'][name] = {'launches': len(ms), 'median_ms': statistics.median(ms[2:] or ms), 'min_ms': min(ms),
                                'max_ms': max(ms)} if 'p2' not in name else {'launches': len(ms), 'ms_in_launch_order': ms}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--trace', default=None, help='a rocprofv3 --kernel-trace output directory to condense')
    args = ap.parse_args()
    if args.trace:
        return condense(args.trace, args.out or os.path.join(ROOT, 'profiles', 'train_signal_rocprof.json'))
    out_path = args.out or os.path.join(ROOT, 'profiles', 'train_signal_timing.json')
    assert torch.cuda.is_available(), 'tools/train_signal_timing.py measures on the GPU'
    dev = torch.device('cuda:0')
    if args.kernels_only:
        for dtype in (torch.float32, torch.float64):
            P = problem(args.n, args.K, dtype, dev)
            for nRx in COILS:
                rx, w = receiver(P, args.n, args.K, nRx, dtype, dev)
                runs, _ = contenders(P, rx, w)
                xs = [P[k].detach().requires_grad_(True) for k in WRT]
                for _ in range(8):
                    torch.autograd.grad(runs['fused'](*xs), xs)
                    torch.cuda.synchronize()
            del P, rx, w, runs, xs
            torch.cuda.empty_cache()
        return
    assert args.reps >= 10, 'the median of at least ten rounds'
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'K': args.K, 'reps': args.reps, 'rest_s': REST,
           'wrt': WRT, 'dtypes': {}}
    for name, dtype in (('float32', torch.float32), ('float64', torch.float64)):
        P = problem(args.n, args.K, dtype, dev)
        del P['w']                                                  # ab_train_timing's per-record weights: not used here
        torch.cuda.empty_cache()
        res['dtypes'][name] = {'record_bytes': args.K * args.n ** 3 * 3 * P['A'].element_size()}
        for nRx in COILS:
            rx, w = receiver(P, args.n, args.K, nRx, dtype, dev)
            runs, last = contenders(P, rx, w)
            xs = [P[k] for k in WRT]
            out = res['dtypes'][name][f'rx{nRx}'] = {}
            for grad in (False, True):
                what, grads = rounds(runs, xs, grad, args.reps)
                what['fused_over_composed'] = what['fused']['median_ms'] / what['composed']['median_ms']
                what['ranges_overlap'] = not (what['fused']['max_ms'] < what['composed']['min_ms'])
                if grad:
                    out['distance_of_fused_from_composed'] = dict(sig=rel_l2(last['fused'], last['composed']), **{
                        'grad_' + k: rel_l2(ga, gb) for k, ga, gb in zip(WRT, grads['fused'], grads['composed'])})
                out['forward+backward' if grad else 'forward'] = what
                print(name, f'rx{nRx}', 'fwd+bwd' if grad else 'fwd',
                      {k: (round(v['median_ms'], 3), round(v['min_ms'], 3), round(v['max_ms'], 3),
                           v['peak_bytes_above_inputs']) for k, v in what.items() if isinstance(v, dict)}, flush=True)
            del rx, w, runs, last, xs, grads
            torch.cuda.empty_cache()
        del P
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', out_path)


if __name__ == '__main__':
    main()
