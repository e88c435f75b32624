r"""What ``fused.ab_train`` costs next to the same recursion as a Python loop of elementwise torch ops on the device.

    python tools/ab_train_timing.py [--n 64] [--K 256] [--reps 10] [--out FILE.json] [--kernels-only]

Shape: n^3 spins x K repetitions, fp32 and fp64, seeded ``A = 0.97 Q`` (``Q`` orthogonal) and ``B``, per-spin ``T1``,
``T2`` and ``Δf``, a rest of 5 ms, the quadratic 117° phase schedule, from ``(0, 0, 1)``; the forward alone
(``torch.no_grad``) and forward + backward of ``(Mt w).sum()`` w.r.t. ``A, B, T1, T2``, ``w`` time-major.  Contenders:

  (a) ``fused.ab_train`` (Ktr / Ktrb);
  (b) the recursion in plain torch on the device: ``F, f`` of the rest once, then per repetition ``Rz(-φ)``, the 3x3
      product with ``A``, ``+ B``, ``Rz(φ)`` and a ``torch.stack`` of the records, autograd through all of it.

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the contenders in one process; reported per contender: median, min, max and the quartiles of the rounds, the
allocator's peak above what was allocated before the call, and the relative L2 distance of (a)'s results from (b)'s.
At this shape the loss ``(Mt w).sum()`` moves more bytes than the kernels, so (a) is also timed without it, as
``a_cot``: the forward alone, and forward + backward with the cotangent ``w`` handed over as it is.  From those come the
rates the times stand for: the forward stores ``K·rows·3`` elements, and the adjoint -- ``a_cot``'s forward + backward
minus its forward -- reads twice that (the records and their cotangents); both next to the HBM peak the README quotes
(8 TB/s).  These times include the Python layer (the operands' preparation, the phase table, the folds of the
gradients), which at this size is longer than the kernels: ``--kernels-only`` runs (a) alone, to be put under
``rocprofv3 --kernel-trace`` for the kernels' own durations (``profiles/ab_train_rocprof.json``).  Nothing is asserted:
the file records what comes out.  Needs the GPU; there is no other path.
"""
import argparse
import json
import os
import statistics
import sys
from math import pi as π

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from mrphy_amd import fused  # noqa: E402

REST = 5e-3
HBM_PEAK = 8e12


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def problem(n, K, dtype, dev):
    gen = torch.Generator().manual_seed(7)
    nM = n ** 3
    rnd = lambda *s: torch.rand(s, generator=gen, dtype=torch.float64)  # noqa: E731
    Q = torch.linalg.qr(torch.randn((1, nM, 3, 3), generator=gen, dtype=torch.float64))[0]
    k = torch.arange(K, dtype=torch.float64)
    P = dict(A=0.97 * Q, B=0.1 * torch.randn((1, nM, 3), generator=gen, dtype=torch.float64), T1=0.05 + 0.1 * rnd(1, nM),
             T2=0.02 + 0.05 * rnd(1, nM), df=(rnd(1, nM) * 2 - 1) * 200, rest=torch.tensor(REST, dtype=torch.float64),
             phase=torch.remainder(117 * π / 180 * k * (k + 1) / 2, 2 * π)[None])
    P = {k_: v.to(device=dev, dtype=dtype) for k_, v in P.items()}
    P['w'] = torch.sin(torch.arange(K * nM * 3, dtype=torch.float64, device=dev) * 0.37 + 0.3).to(dtype).reshape(K, 1, nM, 3)
    return P


def torch_train(A, B, K, phase, rest, T1, T2, df):
    r"""The records, time-major `(K, 1, nM, 3)`, by elementwise torch ops (``M_0 = (0, 0, 1)``)."""
    θ = -2 * π * df * rest
    E1r, E2r, c, s, f3 = torch.exp(-rest / T1), torch.exp(-rest / T2), torch.cos(θ), torch.sin(θ), -torch.expm1(-rest / T1)
    cφ, sφ = torch.cos(phase), torch.sin(phase)
    x, y, z = torch.zeros_like(c), torch.zeros_like(c), torch.ones_like(c)
    out = []
    for k in range(K):
        x, y, z = E2r * (c * x - s * y), E2r * (s * x + c * y), E1r * z + f3
        ck, sk = cφ[:, k, None], sφ[:, k, None]
        M = torch.stack((ck * x + sk * y, ck * y - sk * x, z), -1)
        M = (A @ M[..., None])[..., 0] + B
        x, y, z = ck * M[..., 0] - sk * M[..., 1], sk * M[..., 0] + ck * M[..., 1], M[..., 2]
        out.append(torch.stack((x, y, z), -1))
    return torch.stack(out)


def contenders(P, K):
    last = {}

    def a(A, B, T1, T2):
        last['a'] = Mt = fused.ab_train(A, B, phase=P['phase'], rest=P['rest'], T1=T1, T2=T2, Δf=P['df']).movedim(-2, 0)
        return (Mt * P['w']).sum()

    def b(A, B, T1, T2):
        last['b'] = Mt = torch_train(A, B, K, P['phase'], P['rest'], T1, T2, P['df'])
        return (Mt * P['w']).sum()

    def a_cot(A, B, T1, T2):
        r"""(a) with the cotangent ``w`` handed to the adjoint as it is: no loss, no product, nothing but Ktr and Ktrb and
        the Python layer around them."""
        return fused.ab_train(A, B, phase=P['phase'], rest=P['rest'], T1=T1, T2=T2, Δf=P['df']).movedim(-2, 0)

    return {'a': a, 'b': b}, {'a_cot': a_cot}, last


def timed(run, xs, grad, cot=None):
    r"""Milliseconds of one call between two HIP events, the allocator's peak above the bytes held before the call, and
    the gradients w.r.t. ``xs`` (or None).  ``cot``: ``run`` returns the records and this is their cotangent."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    if grad:
        xs = [x.detach().requires_grad_(True) for x in xs]
        t0.record()
        g = torch.autograd.grad(run(*xs), xs, grad_outputs=cot)
        t1.record()
    else:
        with torch.no_grad():
            t0.record()
            run(*xs)
            t1.record()
        g = None
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), torch.cuda.max_memory_allocated() - base, g


def rounds(runs, xs, grad, reps, cot=None):
    times, peaks, grads = {k: [] for k in runs}, {}, {}
    for r in range(3 + reps):                                   # three warm-up rounds, then alternate
        for k, run in runs.items():
            ms, peaks[k], grads[k] = timed(run, xs, grad, cot if k.endswith('_cot') else None)
            if r >= 3:
                times[k].append(ms)
    what = {}
    for k, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0], 'q3_ms': q[2],
                   'peak_bytes_above_inputs': peaks[k]}
    return what, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ab_train_timing.json'))
    ap.add_argument('--kernels-only', action='store_true',
                    help='8 x (a_cot forward + backward) per data type and nothing else: the program to put under '
                         '`rocprofv3 --kernel-trace` for the durations of Ktr / Ktrb without the Python layer')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/ab_train_timing.py measures on the GPU'
    if args.kernels_only:
        for dtype in (torch.float32, torch.float64):
            P = problem(args.n, args.K, dtype, torch.device('cuda:0'))
            xs = [P[k].detach().requires_grad_(True) for k in ('A', 'B', 'T1', 'T2')]
            _, direct, _ = contenders(P, args.K)
            for _ in range(8):
                torch.autograd.grad(direct['a_cot'](*xs), xs, grad_outputs=P['w'])
                torch.cuda.synchronize()
            del P, xs, direct
            torch.cuda.empty_cache()
        return
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'K': args.K, 'reps': args.reps, 'rest_s': REST,
           'wrt': ['A', 'B', 'T1', 'T2'], 'hbm_peak_bytes_per_s': HBM_PEAK, 'dtypes': {}}
    for name, dtype in (('float32', torch.float32), ('float64', torch.float64)):
        P = problem(args.n, args.K, dtype, dev)
        runs, direct, last = contenders(P, args.K)
        xs = [P['A'], P['B'], P['T1'], P['T2']]
        out = res['dtypes'][name] = {}
        record_bytes = args.K * args.n ** 3 * 3 * P['A'].element_size()
        out['record_bytes'] = record_bytes
        for grad in (False, True):
            what, grads = rounds(dict(runs, **direct), xs, grad, args.reps, P['w'])
            what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
            if grad:
                out['distance_of_a_from_b'] = dict(Mt=rel_l2(last['a'], last['b']), **{
                    'grad_' + k: rel_l2(ga, gb) for k, ga, gb in zip(res['wrt'], grads['a'], grads['b'])})
            else:
                fwd_ms = what['a_cot']['median_ms']
                what['a_cot']['store_bytes_per_s'] = record_bytes / (fwd_ms * 1e-3)
                what['a_cot']['store_over_hbm_peak'] = record_bytes / (fwd_ms * 1e-3) / HBM_PEAK
            out['forward+backward' if grad else 'forward'] = what
            print(name, 'fwd+bwd' if grad else 'fwd', {k: round(v['median_ms'], 3) for k, v in what.items()
                                                       if isinstance(v, dict)}, flush=True)
        # the adjoint alone: (a) with the cotangent handed over, minus the same call's forward -- both without a loss
        fb = out['forward+backward']['a_cot']
        s = max(fb['median_ms'] - fwd_ms, 1e-9) * 1e-3
        fb['backward_ms_by_difference'] = fb['median_ms'] - fwd_ms
        fb['adjoint_read_bytes_per_s_by_difference'] = 2 * record_bytes / s
        fb['adjoint_read_over_hbm_peak_by_difference'] = 2 * record_bytes / s / HBM_PEAK
        del P, runs, direct, last, xs, grads
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
