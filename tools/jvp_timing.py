r"""What forward-mode tangents cost in ``fused.blochsim_rfgr_jvp``, and what the route there was before it costs.

    python tools/jvp_timing.py [--n 64] [--nT 1024] [--reps 10] [--out FILE.json]

Shape: n^3 spins x nT steps, fp32, one transmit coil with a ``b1Map`` and per-spin ``T1 / T2`` (the synthetic cube and pulse
of ``mrphy_amd.synth``), in ``precision('precise')`` and ``('fast')``.  Cases: ``D`` = 1, 2, 4 directions with all eight
tangent groups present (seeded), and ``D`` = 4 with only ``rf``, ``gr`` present.  Contenders:

  (a) ``fused.blochsim_rfgr_jvp`` (K2j), one call for the ``D`` directions;
  (b) the route that existed before: central differences, ``2 D`` calls of ``fused.blochsim_rfgr`` (K2) on operands moved
      by ``± h`` along each direction -- the moved operands are formed outside the timed region;
  (c) one ``fused.blochsim_rfgr`` call, the floor of the primal.

HIP events around each contender, three warm-up rounds, then ``--reps`` rounds that alternate the contenders in one
process; reported per contender: median, min, max and the quartiles of the rounds, the ratios a / b and a / c, and the
one condition -- at ``D`` = 4 in precise mode (a)'s range of rounds lies wholly below (b)'s.  Also recorded: the relative
L2 distance of (b)'s central difference from (a)'s tangent per direction over a ladder of step sizes ``h`` (relative to
the operands' scale), and the best of them: what accuracy the previous route had at its best.  ``PREDICTED`` is a / b
written down before the first measurement, from instruction counts; it is copied into the
result beside the measured one.  No time is fixed in advance.  Needs the GPU; there is no other path.
-> ``profiles/jvp_timing.json``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import mrphy_amd  # noqa: E402
from mrphy_amd import fused, synth  # noqa: E402

# a / b predicted before anything was timed: about 41 VALU instructions per primal step, 12 shared for S', C', 50 per
# direction -- (41 + 12 + 50 D) / (2 D 41): {D: ratio}
PREDICTED = {1: 1.26, 2: 0.93, 4: 0.77}
GROUPS = ('Mi', 'rf', 'gr', 'loc', 'Δf', 'b1Map', 'T1', 'T2')
SCALE = dict(Mi=1.0, rf=0.1, gr=1.0, loc=1.0, Δf=100.0, b1Map=0.2, T1=0.3, T2=0.03)
H_LADDER = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4)


def problem(n, nT, dev):
    sp = synth.cube_spins(n, dtype=torch.float32, device=dev)
    p = synth.pulse(nT, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(5)
    b1 = (torch.rand((1, n ** 3, 2), generator=gen, dtype=torch.float64) * 0.4 + 0.8).float().to(dev)
    ops = dict(Mi=sp['M0'], rf=p['rf'], gr=p['gr'], loc=sp['loc'], Δf=sp['Δf'], b1Map=b1, T1=sp['T1'], T2=sp['T2'])
    return ops, dict(γ_beff=sp['γ'], γ=sp['γ'], dt=p['dt'])


def directions(ops, D, groups, dev):
    gen = torch.Generator().manual_seed(9)
    return {k: ((torch.rand((D,) + tuple(ops[k].shape), generator=gen, dtype=torch.float64) * 2 - 1) * SCALE[k]).float().to(dev)
            for k in groups}


def forward(ops, rest):
    return fused.blochsim_rfgr(ops['Mi'], ops['rf'], ops['gr'], ops['loc'], Δf=ops['Δf'], b1Map=ops['b1Map'], T1=ops['T1'],
                               T2=ops['T2'], **rest)


def moved(ops, V, d, h):
    return dict(ops, **{k: ops[k] + h * v[d] for k, v in V.items()})


def timed(run):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        t0.record()
        out = run()
        t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def rel_l2(x, y):
    x, y = x.detach().double(), y.detach().double()
    return float((x - y).norm() / y.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jvp_timing.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/jvp_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    ops, rest = problem(args.n, args.nT, dev)
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'cases': {}}
    for name, D, groups in (('D1.all', 1, GROUPS), ('D2.all', 2, GROUPS), ('D4.all', 4, GROUPS), ('D4.rf_gr', 4, ('rf', 'gr'))):
        V = directions(ops, D, groups, dev)
        per = res['cases'][name] = {'D': D, 'groups': list(groups), 'predicted_a_over_b': PREDICTED[D], 'modes': {}}
        for mode in ('precise', 'fast'):
            with mrphy_amd.precision(mode), torch.no_grad():
                pm = [(moved(ops, V, d, 1e-2), moved(ops, V, d, -1e-2)) for d in range(D)]
                runs = {'a': lambda: fused.blochsim_rfgr_jvp(ops['Mi'], ops['rf'], ops['gr'], ops['loc'], tangents=V, Δf=ops['Δf'],
                                                             b1Map=ops['b1Map'], T1=ops['T1'], T2=ops['T2'], **rest)[1],
                        'b': lambda: [forward(q, rest) for pair in pm for q in pair],
                        'c': lambda: forward(ops, rest)}
                times = {k: [] for k in runs}
                for r in range(3 + args.reps):                           # three warm-up rounds, then alternate
                    for k, run in runs.items():
                        ms, out = timed(run)
                        if r >= 3:
                            times[k].append(ms)
                        if k == 'a':
                            dMo = out
                del pm
                what = per['modes'][mode] = {}
                for k, ts in times.items():
                    q = statistics.quantiles(ts, n=4)
                    what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0],
                               'q3_ms': q[2]}
                what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
                what['a_over_c'] = what['a']['median_ms'] / what['c']['median_ms']
                what['a_range_wholly_below_b_range'] = what['a']['max_ms'] < what['b']['min_ms']
                # what the central difference was worth: its distance from the tangent per step size, direction 0
                ladder = {}
                for h in H_LADDER:
                    up, dn = forward(moved(ops, V, 0, h), rest), forward(moved(ops, V, 0, -h), rest)
                    ladder[f'{h:g}'] = rel_l2((up - dn) / (2 * h), dMo[0])
                what['central_difference_from_tangent'] = ladder
                what['central_difference_best'] = min(ladder.values())
                print(name, mode, {k: f"{v['median_ms']:.3f} ({v['min_ms']:.3f} - {v['max_ms']:.3f})" for k, v in what.items()
                                   if isinstance(v, dict) and 'median_ms' in v},
                      'a/b', round(what['a_over_b'], 3), 'a/c', round(what['a_over_c'], 2), 'a below b:',
                      what['a_range_wholly_below_b_range'], 'best central difference', f"{what['central_difference_best']:.2e}",
                      flush=True)
        del V
        torch.cuda.empty_cache()
    d4 = res['cases']['D4.all']['modes']['precise']
    res['condition_D4_precise_a_wholly_below_b'] = d4['a_range_wholly_below_b_range']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
