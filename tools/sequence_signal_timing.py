r"""What ``fused.sequence_signal`` costs next to the route there was before it, and next to ``fused.train_signal`` where the
schedule is not used.

    python tools/sequence_signal_timing.py [--n 64] [--K 256] [--P 16] [--reps 10] [--limit 240] [--out FILE.json]

Shape: n^3 spins x K repetitions of a bank of P pulses, fp32 and fp64, the problem of ``tools/ab_sequence_timing.py``
(seeded ``A_p = 0.97 Q_p``, ``B_p``, per-spin ``T1, T2, Δf``, the quadratic 117° phase schedule, the sinusoidal flip-angle
schedule quantised to the bank and ``rest_k`` between 8 and 12 ms: no two neighbouring repetitions are equal), with the
seeded complex receive map of ``tools/train_signal_timing.py`` for 1 and for 8 coils.  The forward alone
(``torch.no_grad``) and forward + backward of ``(sig w).sum()`` w.r.t. ``A, B, T1, T2, rest``.  Routes:

  (a) ``fused`` = ``fused.sequence_signal`` (Ksqs / Ksqsb and their second passes) against ``composed`` = the route there
      was before it, ``fused.ab_sequence`` (Ksq / Ksqb) followed by ``fused._signal_of`` on its time-major records;
  (b) the degenerate schedule, ``P = 1`` and one ``rest`` (10 ms): ``b_seq`` = ``fused.sequence_signal``, ``b_train`` =
      ``fused.train_signal`` on the same numbers -- what the schedule costs when it is not used, as a ratio.

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the routes in one process; reported per route: median, min, max and the quartiles of the rounds and, for (a),
the allocator's peak above what was allocated before the call, whether the ranges of ``fused`` and ``composed`` overlap
and the distance of ``fused``'s results from ``composed``'s.  These times include the Python layer.  Every data type and
coil count is measured by a child process of its own under a time limit of ``--limit`` seconds; the first child that
fails or runs out of time ends the tool, and nothing more is started on the GPU.  Nothing is asserted: the file records
what comes out.  Needs the GPU; there is no other path.
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
COILS = (1, 8)
WRT = ('A', 'B', 'T1', 'T2', 'rest')


def routes(P, rx, w):
    from mrphy_amd import fused
    last = {}
    kw = dict(phase=P['phase'], Δf=P['df'])

    def a_fused(A, B, T1, T2, rest):
        last['a'] = sig = fused.sequence_signal(A, B, pulse=P['pulse'], rest=rest, T1=T1, T2=T2, rx=rx, **kw)
        return (sig * w).sum()

    def a_composed(A, B, T1, T2, rest):
        Mt = fused.ab_sequence(A, B, pulse=P['pulse'], rest=rest, T1=T1, T2=T2, **kw).movedim(-2, 0)
        last['b'] = sig = fused._signal_of(Mt, rx)
        return (sig * w).sum()

    def b_seq(A1, B1, T1, T2, rest0):
        return (fused.sequence_signal(A1, B1, rest=rest0, T1=T1, T2=T2, rx=rx, **kw) * w).sum()

    def b_train(A0, B0, T1, T2, rest0):
        return (fused.train_signal(A0, B0, rest=rest0, T1=T1, T2=T2, rx=rx, **kw) * w).sum()

    # each route with the operands it differentiates: (b) on entry 0 of the bank and one rest of 10 ms.  The keys 'a'
    # and 'b' are the two whose peaks and gradients ab_sequence_timing.rounds keeps: fused and composed of (a).
    xs = [P[k] for k in WRT]
    rest0 = torch.full((), 10e-3, dtype=P['rest'].dtype, device=P['rest'].device)
    xs_seq = [P['A'][:1].contiguous(), P['B'][:1].contiguous(), P['T1'], P['T2'], rest0]
    xs_train = [P['A'][0].contiguous(), P['B'][0].contiguous(), P['T1'], P['T2'], rest0]
    return {'a': (a_fused, xs), 'b': (a_composed, xs), 'b_seq': (b_seq, xs_seq), 'b_train': (b_train, xs_train)}, last


def measure(args, name, nRx):
    r"""One data type and coil count, in this process: ``{'forward': ..., 'forward+backward': ..., ...}``."""
    # imported here: the parent process, which only starts the children, never loads the library
    from ab_sequence_timing import problem, rel_l2, rounds
    from train_signal_timing import receiver
    assert torch.cuda.is_available(), 'tools/sequence_signal_timing.py measures on the GPU'
    dev, dtype = torch.device('cuda:0'), DTYPES[name]
    P = problem(args.n, args.K, args.P, dtype, dev)
    del P['w']                                                  # ab_sequence_timing's per-record weights: not used here
    torch.cuda.empty_cache()
    rx, w = receiver(P, args.n, args.K, nRx, dtype, dev)
    runs, last = routes(P, rx, w)
    out = {'device': torch.cuda.get_device_name(0), 'bank_entries_played': len(set(P['pulse'])),
           'record_bytes': args.K * args.n ** 3 * 3 * P['A'].element_size()}
    names = {'a': 'fused', 'b': 'composed'}
    for grad in (False, True):
        what, grads = rounds(runs, grad, args.reps)
        what = {names.get(k, k): v for k, v in what.items()}
        f, c = what['fused'], what['composed']
        what['fused_over_composed'] = f['median_ms'] / c['median_ms']
        what['ranges_overlap'] = not (f['max_ms'] < c['min_ms'] or c['max_ms'] < f['min_ms'])
        what['b_seq_over_b_train'] = what['b_seq']['median_ms'] / what['b_train']['median_ms']
        if grad:
            out['distance_of_fused_from_composed'] = dict(sig=rel_l2(last['a'], last['b']), **{
                'grad_' + k: rel_l2(ga, gb) for k, ga, gb in zip(WRT, grads['a'], grads['b'])})
        out['forward+backward' if grad else 'forward'] = what
        print(name, f'rx{nRx}', 'fwd+bwd' if grad else 'fwd',
              {k: (round(v['median_ms'], 3), round(v['min_ms'], 3), round(v['max_ms'], 3)) for k, v in what.items()
               if isinstance(v, dict)}, flush=True)
        del grads
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--P', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--limit', type=float, default=240, help='seconds one data type and coil count may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_signal_timing.json'))
    ap.add_argument('--one', nargs=2, metavar=('DTYPE', 'NRX'), default=None,
                    help='measure one data type and coil count in this process and print the JSON (what the tool runs as '
                         'its children)')
    args = ap.parse_args()
    assert args.reps >= 10, 'the median of at least ten rounds'
    if args.one:
        print('RESULT ' + json.dumps(measure(args, args.one[0], int(args.one[1]))), flush=True)
        return 0
    # the parent never touches the GPU: one child per data type and coil count, each under its own time limit
    res = {'n': args.n, 'K': args.K, 'P': args.P, 'reps': args.reps, 'wrt': list(WRT), 'dtypes': {}}
    for name in DTYPES:
        for nRx in COILS:
            cmd = [sys.executable, os.path.abspath(__file__), '--n', str(args.n), '--K', str(args.K), '--P', str(args.P),
                   '--reps', str(args.reps), '--one', name, str(nRx)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f'{name} rx{nRx}: no result within {args.limit} s; nothing more is started', file=sys.stderr)
                return 124
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
            sys.stdout.write(''.join(ln + '\n' for ln in r.stdout.splitlines() if not ln.startswith('RESULT ')))
            if r.returncode != 0 or not lines:
                print(f'{name} rx{nRx}: the child ended with {r.returncode}; nothing more is started\n{r.stderr[-2000:]}',
                      file=sys.stderr)
                return r.returncode or 1
            one = json.loads(lines[-1][len('RESULT '):])
            res['device'] = one.pop('device')
            d = res['dtypes'].setdefault(name, {'record_bytes': one.pop('record_bytes'),
                                                'bank_entries_played': one.pop('bank_entries_played')})
            one.pop('record_bytes', None), one.pop('bank_entries_played', None)
            d[f'rx{nRx}'] = one
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
