r"""What ``fused.sequence_steadystate`` costs next to the route there was before it.

    python tools/sequence_steadystate_timing.py [--n 64] [--K 80] [--P 16] [--reps 10] [--limit 240] [--out FILE.json]

Shape: n^3 spins, a period of K = 80 repetitions with the quadratic 117° phase schedule (its period), the bank of P = 16
pulses, the flip-angle schedule and the rests of ``tools/ab_sequence_timing.py`` (seeded ``A_p = 0.97 Q_p``, ``B_p``,
per-spin ``T1, T2, Δf``, ``rest_k`` between 8 and 12 ms), fp32 and fp64; the bank is made contiguous once, outside the
timed calls.  The forward alone (``torch.no_grad``) and forward + backward of ``(Mss w).sum()`` w.r.t.
``A, B, T1, T2, rest``.  Routes:

  ``fused``    = ``fused.sequence_steadystate`` (Ksqp; Ksqpl + Ksqsb and their second passes);
  ``composed`` = the route there was before it: ``fused.ab_sequence`` on the four start vectors ``0, e_x, e_y, e_z``, the
                 differences of the last records as ``Ā``, then ``fused.ab_steadystate(Ā, b̄, rest=None)``.

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the routes in one process; reported per route: median, min, max and the quartiles of the rounds, the
allocator's peak above what was allocated before the call, whether the two ranges overlap and the distance of
``fused``'s results from ``composed``'s.  These times include the Python layer.  Every data type is measured by a child
process of its own under a time limit of ``--limit`` seconds; the first child that fails or runs out of time ends the
tool, and nothing more is started on the GPU.  Nothing is asserted: the file records what comes out.  Needs the GPU;
there is no other path.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DTYPES = {'float32': torch.float32, 'float64': torch.float64}
WRT = ('A', 'B', 'T1', 'T2', 'rest')


def routes(P, w):
    from mrphy_amd import fused
    last = {}
    kw = dict(pulse=P['pulse'], phase=P['phase'], Δf=P['df'])
    starts = torch.zeros((4, 1, 1, 3), dtype=w.dtype, device=w.device)
    for j in range(3):
        starts[j + 1, ..., j] = 1

    def a_fused(A, B, T1, T2, rest):
        last['a'] = Mss = fused.sequence_steadystate(A, B, rest=rest, T1=T1, T2=T2, **kw)
        return (Mss * w).sum()

    def a_composed(A, B, T1, T2, rest):
        ends = [fused.ab_sequence(A, B, Mi=Mi, rest=rest, T1=T1, T2=T2, **kw)[..., -1, :] for Mi in starts]
        b = ends[0]
        Abar = torch.stack([e - b for e in ends[1:]], dim=-1)
        last['b'] = Mss = fused.ab_steadystate(Abar, b)
        return (Mss * w).sum()

    # the keys 'a' and 'b' are the two whose peaks and gradients ab_sequence_timing.rounds keeps
    xs = [P[k] for k in WRT]
    return {'a': (a_fused, xs), 'b': (a_composed, xs)}, last


def measure(args, name):
    r"""One data type, in this process: ``{'forward': ..., 'forward+backward': ..., ...}``."""
    # imported here: the parent process, which only starts the children, never loads the library
    from ab_sequence_timing import problem, rel_l2, rounds
    assert torch.cuda.is_available(), 'tools/sequence_steadystate_timing.py measures on the GPU'
    dev, dtype = torch.device('cuda:0'), DTYPES[name]
    P = problem(args.n, args.K, args.P, dtype, dev)
    del P['w']                                                  # ab_sequence_timing's per-record weights: not used here
    P['A'] = P['A'].contiguous()                                # torch.linalg.qr returns column-major matrices
    nM = args.n ** 3
    w = torch.sin(torch.arange(nM * 3, dtype=torch.float64, device=dev) * 0.37 + 0.3).to(dtype).reshape(1, nM, 3)
    torch.cuda.empty_cache()
    runs, last = routes(P, w)
    out = {'device': torch.cuda.get_device_name(0), 'bank_entries_played': len(set(P['pulse'])),
           'record_bytes': args.K * nM * 3 * P['A'].element_size()}
    names = {'a': 'fused', 'b': 'composed'}
    for grad in (False, True):
        what, grads = rounds(runs, grad, args.reps)
        what = {names[k]: v for k, v in what.items()}
        f, c = what['fused'], what['composed']
        what['fused_over_composed'] = f['median_ms'] / c['median_ms']
        what['ranges_overlap'] = not (f['max_ms'] < c['min_ms'] or c['max_ms'] < f['min_ms'])
        if grad:
            out['distance_of_fused_from_composed'] = dict(Mss=rel_l2(last['a'], last['b']), **{
                'grad_' + k: rel_l2(ga, gb) for k, ga, gb in zip(WRT, grads['a'], grads['b'])})
        out['forward+backward' if grad else 'forward'] = what
        print(name, 'fwd+bwd' if grad else 'fwd',
              {k: (round(v['median_ms'], 3), round(v['min_ms'], 3), round(v['max_ms'], 3)) for k, v in what.items()
               if isinstance(v, dict)}, flush=True)
        del grads
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=80)
    ap.add_argument('--P', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--limit', type=float, default=240, help='seconds one data type may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_steadystate_timing.json'))
    ap.add_argument('--one', metavar='DTYPE', default=None,
                    help='measure one data type in this process and print the JSON (what the tool runs as its children)')
    args = ap.parse_args()
    assert args.reps >= 10, 'the median of at least ten rounds'
    if args.one:
        print('RESULT ' + json.dumps(measure(args, args.one)), flush=True)
        return 0
    # the parent never touches the GPU: one child per data type, each under its own time limit
    res = {'n': args.n, 'K': args.K, 'P': args.P, 'reps': args.reps, 'wrt': list(WRT), 'dtypes': {}}
    for name in DTYPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--n', str(args.n), '--K', str(args.K), '--P', str(args.P),
               '--reps', str(args.reps), '--one', name]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f'{name}: no result within {args.limit} s; nothing more is started', file=sys.stderr)
            return 124
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        sys.stdout.write(''.join(ln + '\n' for ln in r.stdout.splitlines() if not ln.startswith('RESULT ')))
        if r.returncode != 0 or not lines:
            print(f'{name}: the child ended with {r.returncode}; nothing more is started\n{r.stderr[-2000:]}',
                  file=sys.stderr)
            return r.returncode or 1
        one = json.loads(lines[-1][len('RESULT '):])
        res['device'] = one.pop('device')
        res['dtypes'][name] = one
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
