r"""What ``fused.ab_sequence`` costs next to the route there was before it, and next to ``fused.ab_train`` where the
schedule is not used.

    python tools/ab_sequence_timing.py [--n 64] [--K 256] [--P 16] [--reps 10] [--out FILE.json] [--kernels-only]

Shape: n^3 spins x K repetitions of a bank of P pulses, fp32 and fp64: seeded ``A_p = 0.97 Q_p`` (``Q_p`` orthogonal) and
``B_p``, per-spin ``T1``, ``T2`` and ``Δf``, the quadratic 117° phase schedule, from ``(0, 0, 1)``.  The schedule is a
sinusoidal flip-angle pattern quantised to the bank, ``pulse_k = round((P - 1) (1 + sin(2π k / 50)) / 2)``, and the rest
varies between 8 and 12 ms, ``rest_k = 10 ms + 2 ms sin(2π k / 37 + 1)``: no two neighbouring repetitions are equal.
The forward alone (``torch.no_grad``) and forward + backward of ``(Mt w).sum()`` w.r.t. ``A, B, T1, T2, rest``, ``w``
time-major.  Routes:

  (a) ``fused.ab_sequence`` (Ksq / Ksqb), one launch each way;
  (b) the route there was: ``fused.ab_train`` per run of equal ``(pulse, rest)``, chained through ``Mi``, the records
      joined by ``torch.cat`` -- on this schedule one call per repetition.  The bank is unbound once
      (``A.unbind(0)``), so that its gradient is one ``stack`` and not a bank-sized scatter per repetition;
  (c) the degenerate schedule, ``P = 1`` and one ``rest`` (10 ms): ``c_seq`` = ``fused.ab_sequence``, ``c_train`` =
      ``fused.ab_train`` on the same numbers -- what the schedule costs when it is not used.

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the routes in one process; reported per route: median, min, max and the quartiles of the rounds and, for (a)
and (b), the allocator's peak above what was allocated before the call; the ratios (a)/(b), (a)/(c_seq) and
c_seq/c_train, whether the ranges of (a) and (b) overlap, and the distance of (a)'s results from (b)'s.  These times
include the Python layer.  ``--kernels-only`` runs forward + backward of (a), c_seq (with and without the gradient
w.r.t. ``rest``) and c_train and nothing else: the program to put under ``rocprofv3 --kernel-trace`` for the kernels' own durations.  Nothing is asserted: the
file records what comes out.  Needs the GPU; there is no other path.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
from math import pi as π

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from mrphy_amd import fused  # noqa: E402

WRT = ('A', 'B', 'T1', 'T2', 'rest')


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def problem(n, K, P_, dtype, dev):
    gen = torch.Generator().manual_seed(11)
    nM = n ** 3
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((P_, 1, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    k = torch.arange(K, dtype=torch.float64)
    P = dict(A=0.97 * Q, B=0.1 * torch.randn((P_, 1, nM, 3), generator=gen, dtype=torch.float64),
             T1=0.05 + 0.1 * rnd(1, nM), T2=0.02 + 0.05 * rnd(1, nM), df=(rnd(1, nM) * 2 - 1) * 200,
             rest=(10e-3 + 2e-3 * torch.sin(2 * π * k / 37 + 1))[None],
             phase=torch.remainder(117 * π / 180 * k * (k + 1) / 2, 2 * π)[None])
    P = {k_: v.to(device=dev, dtype=dtype) for k_, v in P.items()}
    P['pulse'] = torch.round((P_ - 1) * (1 + torch.sin(2 * π * k / 50)) / 2).to(torch.int64).tolist()
    P['w'] = torch.sin(torch.arange(K * nM * 3, dtype=torch.float64, device=dev) * 0.37 + 0.3).to(dtype).reshape(K, 1, nM, 3)
    return P


def runs_of(pulse, rest_host):
    r"""``[(k0, k1, p)]``: the runs of equal ``(pulse_k, rest_k)``."""
    out, k0 = [], 0
    for k in range(1, len(pulse) + 1):
        if k == len(pulse) or pulse[k] != pulse[k0] or rest_host[k] != rest_host[k0]:
            out.append((k0, k, pulse[k0]))
            k0 = k
    return out


def routes(P, K):
    last = {}
    runs = runs_of(P['pulse'], P['rest'][0].tolist())

    def sequence(A, B, T1, T2, rest):
        return fused.ab_sequence(A, B, pulse=P['pulse'], phase=P['phase'], rest=rest, T1=T1, T2=T2, Δf=P['df']).movedim(-2, 0)

    def chained(A, B, T1, T2, rest):
        As, Bs, M, out = A.unbind(0), B.unbind(0), None, []
        for k0, k1, p in runs:
            Mt = fused.ab_train(As[p], Bs[p], Mi=M, phase=P['phase'][:, k0:k1], rest=rest[:, k0], T1=T1, T2=T2,
                                Δf=P['df']).movedim(-2, 0)
            M = Mt[-1]
            out.append(Mt)
        return torch.cat(out)

    def a(*xs):
        last['a'] = Mt = sequence(*xs)
        return (Mt * P['w']).sum()

    def b(*xs):
        last['b'] = Mt = chained(*xs)
        return (Mt * P['w']).sum()

    def c_seq(A1, B1, T1, T2, rest0):
        Mt = fused.ab_sequence(A1, B1, phase=P['phase'], rest=rest0, T1=T1, T2=T2, Δf=P['df'])
        return (Mt.movedim(-2, 0) * P['w']).sum()

    def c_train(A0, B0, T1, T2, rest0):
        Mt = fused.ab_train(A0, B0, phase=P['phase'], rest=rest0, T1=T1, T2=T2, Δf=P['df'])
        return (Mt.movedim(-2, 0) * P['w']).sum()

    # each route with the operands it differentiates: (c) on entry 0 of the bank and one rest of 10 ms
    xs = [P[k] for k in WRT]
    rest0 = torch.full((), 10e-3, dtype=P['rest'].dtype, device=P['rest'].device)
    xs_seq = [P['A'][:1].contiguous(), P['B'][:1].contiguous(), P['T1'], P['T2'], rest0]
    xs_train = [P['A'][0].contiguous(), P['B'][0].contiguous(), P['T1'], P['T2'], rest0]
    return {'a': (a, xs), 'b': (b, xs), 'c_seq': (c_seq, xs_seq), 'c_train': (c_train, xs_train)}, last, len(runs)


def timed(run, xs, grad):
    r"""Milliseconds of one call between two HIP events, the allocator's peak above the bytes held before the call, and
    the gradients w.r.t. ``xs`` (or None)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    if grad:
        xs = [x.detach().requires_grad_(True) for x in xs]
        t0.record()
        g = torch.autograd.grad(run(*xs), xs)
        t1.record()
    else:
        with torch.no_grad():
            t0.record()
            run(*xs)
            t1.record()
        g = None
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), torch.cuda.max_memory_allocated() - base, g


def rounds(runs, grad, reps):
    times, peaks, grads = {k: [] for k in runs}, {}, {}
    for r in range(3 + reps):                                   # three warm-up rounds, then alternate
        for k, (run, xs) in runs.items():
            ms, peaks[k], g = timed(run, xs, grad)
            if k in ('a', 'b'):
                grads[k] = g
            del g
            if r >= 3:
                times[k].append(ms)
    what = {}
    for k, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0], 'q3_ms': q[2]}
        if k in ('a', 'b'):
            what[k]['peak_bytes_above_inputs'] = peaks[k]
    return what, grads


def condense(trace_dir, out):
    r"""Durations of Ksq / Ksqb, the second pass and Ktr / Ktrb from a ``rocprofv3 --kernel-trace --output-format csv``
    directory of a ``--kernels-only`` run: per kernel and data type its launches in order -- 8 on the schedule (a), then
    for Ksq / Ksqb 8 on the degenerate one (c_seq) and 8 more of it without ``grad_rest``; Ktr / Ktrb: the 8 of c_train
    --, the median of all but the first two of each eight and (min - max) of the eight."""
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r['Kernel_Name']
            if 'k_ab_sequence' not in name and 'k_ab_train' not in name:
                continue
            short = name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            t0, t1 = int(r['Start_Timestamp']), int(r['End_Timestamp'])
            rows.setdefault(short, []).append((t0, (t1 - t0) / 1e6))
    res = {'tool': 'rocprofv3 --kernel-trace -- python tools/ab_sequence_timing.py --kernels-only',
           'shape': '64^3 spins x K = 256, N = 1, a bank of 16; gradients w.r.t. A, B, T1, T2, rest',
           'method': '8 launches per kernel, data type and schedule in one process; median of the last 6, (min - max) of '
                     'all 8; kernel durations only', 'kernels': {}}
    for name, xs in sorted(rows.items()):
        ms = [d for _, d in sorted(xs)]
        parts = {'schedule': ms[:8], 'degenerate': ms[8:16], 'degenerate_without_grad_rest': ms[16:24]} \
            if 'k_ab_sequence' in name else {'train': ms[:8]}
        res['kernels'][name] = {k: {'launches': len(v), 'median_ms': statistics.median(v[2:] or v), 'min_ms': min(v),
                                    'max_ms': max(v)} for k, v in parts.items() if v}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--P', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ab_sequence_timing.json'))
    ap.add_argument('--kernels-only', action='store_true',
                    help='8 x forward + backward of (a), c_seq and c_train per data type and nothing else: the program '
                         'to put under `rocprofv3 --kernel-trace`')
    ap.add_argument('--trace', default=None, help='a rocprofv3 --kernel-trace output directory to condense into --out')
    args = ap.parse_args()
    if args.trace:
        return condense(args.trace, args.out)
    assert torch.cuda.is_available(), 'tools/ab_sequence_timing.py measures on the GPU'
    dev = torch.device('cuda:0')
    if args.kernels_only:
        for dtype in (torch.float32, torch.float64):
            P = problem(args.n, args.K, args.P, dtype, dev)
            runs, _, _ = routes(P, args.K)
            for k in ('a', 'c_seq', 'c_train'):
                run, xs = runs[k]
                xs = [x.detach().requires_grad_(True) for x in xs]
                for _ in range(8):
                    torch.autograd.grad(run(*xs), xs)
                    torch.cuda.synchronize()
                if k == 'c_seq':                 # ... and without grad_rest, Ktrb's outputs: what the record of it costs
                    for _ in range(8):
                        torch.autograd.grad(run(*xs[:4], xs[4].detach()), xs[:4])
                        torch.cuda.synchronize()
            del P, xs, runs
            torch.cuda.empty_cache()
        return
    assert args.reps >= 10, 'the median of at least ten rounds'
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'K': args.K, 'P': args.P, 'reps': args.reps,
           'wrt': list(WRT), 'dtypes': {}}
    for name, dtype in (('float32', torch.float32), ('float64', torch.float64)):
        P = problem(args.n, args.K, args.P, dtype, dev)
        runs, last, ncalls = routes(P, args.K)
        out = res['dtypes'][name] = {'calls_of_b_each_way': ncalls, 'bank_entries_played': len(set(P['pulse'])),
                                     'record_bytes': args.K * args.n ** 3 * 3 * P['A'].element_size()}
        for grad in (False, True):
            what, grads = rounds(runs, grad, args.reps)
            what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
            what['ranges_of_a_and_b_overlap'] = not (what['a']['max_ms'] < what['b']['min_ms'] or
                                                     what['b']['max_ms'] < what['a']['min_ms'])
            what['a_over_c_seq'] = what['a']['median_ms'] / what['c_seq']['median_ms']
            what['c_seq_over_c_train'] = what['c_seq']['median_ms'] / what['c_train']['median_ms']
            what['c_train_max_over_min'] = what['c_train']['max_ms'] / what['c_train']['min_ms']
            if grad:
                out['distance_of_a_from_b'] = dict(Mt=rel_l2(last['a'], last['b']), **{
                    'grad_' + k: rel_l2(ga, gb) for k, ga, gb in zip(WRT, grads['a'], grads['b'])})
            out['forward+backward' if grad else 'forward'] = what
            print(name, 'fwd+bwd' if grad else 'fwd', {k: round(v['median_ms'], 3) for k, v in what.items()
                                                       if isinstance(v, dict)}, flush=True)
            del grads
        del P, runs, last
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
