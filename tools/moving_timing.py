r"""What motion costs in ``fused.blochsim_rfgr_moving``, and what the route there was before it costs.

    python tools/moving_timing.py [--n 64] [--nT 1024] [--reps 10] [--out FILE.json]

Shape: n^3 spins x nT steps, fp32, one transmit coil with a ``b1Map`` and per-spin ``T1 / T2`` (the synthetic cube and pulse
of ``mrphy_amd.synth``), velocities seeded uniform in +-50 cm/s per component, in ``precision('precise')`` and ``('fast')``,
the forward alone (``torch.no_grad``) and forward + backward of ``(Mo w).sum()`` w.r.t. ``rf`` and ``gr``.  Contenders:

  (a) ``fused.blochsim_rfgr_moving`` (K2v; K2v with checkpoints + K2vb);
  (b) ``fused.blochsim_rfgr`` on the same static problem (K2; K2 with checkpoints + K2b): (a) over (b) is what motion costs;
  (c) the composed route, which is what there was before: ``rfgr2beff`` at the static ``loc``, the moving part
      ``(gr_t . vel dt)(t + 1/2)`` added to its z component in torch, then ``sims.blochsim`` -- ``Beff`` and, with gradients,
      ``grad_Beff`` and the history in memory.

HIP events around each call (the loss and its backward included, the same small torch kernels for all three), three
warm-up rounds, then ``--reps`` rounds that alternate the contenders in one process; reported per contender: median, min,
max and the quartiles of the rounds, the allocator's peak over one call, the ratios a / b and c / a, whether (c) is slower
than (a) beyond the rounds' spread, and the relative L2 distance of (a)'s ``Mo`` and gradients from (c)'s (from (b)'s they
differ by the motion).  No time is fixed in advance.  Needs the GPU; there is no other path.
-> ``profiles/moving_timing.json``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import mrphy_amd  # noqa: E402
from mrphy_amd import beffective, fused, sims, synth  # noqa: E402


def problem(n, nT, dev):
    sp = synth.cube_spins(n, dtype=torch.float32, device=dev)
    p = synth.pulse(nT, dtype=torch.float32, device=dev)
    nM = n ** 3
    gen = torch.Generator().manual_seed(5)
    b1 = (torch.rand((1, nM, 2), generator=gen, dtype=torch.float64) * 0.4 + 0.8).float().to(dev)
    vel = ((torch.rand((1, nM, 3), generator=gen, dtype=torch.float64) * 2 - 1) * 50).float().to(dev)
    w = torch.sin(torch.arange(nM * 3, dtype=torch.float64) * 0.61 + 1).reshape(1, nM, 3).float().to(dev)
    return sp, p, b1, vel, w


def contenders(sp, p, b1, vel, w):
    r"""``{name: run(rf, gr) -> loss}`` -- each also leaves its ``Mo`` in ``last[name]``."""
    γ, dt = sp['γ'], p['dt']
    kw = dict(Δf=sp['Δf'], b1Map=b1, γ_beff=γ, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
    last = {}

    def a(rf, gr):
        last['a'] = Mo = fused.blochsim_rfgr_moving(sp['M0'], rf, gr, sp['loc'], vel, **kw)
        return (Mo * w).sum()

    def b(rf, gr):
        last['b'] = Mo = fused.blochsim_rfgr(sp['M0'], rf, gr, sp['loc'], **kw)
        return (Mo * w).sum()

    def c(rf, gr):
        beff = beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], b1Map=b1, γ=γ, lazy=False)
        z = fused._moving_bz(gr, fused._vel_dt(vel, dt, sp['loc']), 0)
        beff = beff + torch.nn.functional.pad(z.unsqueeze(-1), (2, 0))
        last['c'] = Mo = sims.blochsim(sp['M0'], beff, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
        return (Mo * w).sum()

    return {'a': a, 'b': b, 'c': c}, last


def timed(run, rf, gr, grad):
    r"""Milliseconds of one call between two HIP events; the gradients (or None)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if grad:
        rf, gr = rf.detach().requires_grad_(True), gr.detach().requires_grad_(True)
        t0.record()
        g = torch.autograd.grad(run(rf, gr), (rf, gr))
        t1.record()
    else:
        with torch.no_grad():
            t0.record()
            run(rf, gr)
            t1.record()
        g = None
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), g


def rel_l2(x, y):
    x, y = x.detach().double(), y.detach().double()
    return float((x - y).norm() / y.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moving_timing.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/moving_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    sp, p, b1, vel, w = problem(args.n, args.nT, dev)
    rf, gr = p['rf'], p['gr']
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'beff_bytes': 12 * args.n ** 3 * args.nT, 'max_abs_vel_dt_cm': float((vel.abs().max() * p['dt'].max())),
           'modes': {}}
    for mode in ('precise', 'fast'):
        with mrphy_amd.precision(mode):
            runs, last = contenders(sp, p, b1, vel, w)
            out = res['modes'][mode] = {}
            for grad in (False, True):
                times = {k: [] for k in runs}
                grads = {}
                for r in range(3 + args.reps):                       # three warm-up rounds, then alternate
                    for k, run in runs.items():
                        ms, g = timed(run, rf, gr, grad)
                        if r >= 3:
                            times[k].append(ms)
                        grads[k] = g
                what = out['forward+backward' if grad else 'forward'] = {}
                for k, ts in times.items():
                    q = statistics.quantiles(ts, n=4)
                    what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts),
                               'q1_ms': q[0], 'q3_ms': q[2]}
                dist = {'Mo.a_from_c': rel_l2(last['a'], last['c']), 'Mo.a_from_b': rel_l2(last['a'], last['b'])}
                if grad:
                    dist.update({f'grad_{n}.a_from_{k}': rel_l2(grads['a'][i], grads[k][i])
                                 for k in ('c', 'b') for i, n in enumerate(('rf', 'gr'))})
                grads.clear()
                last.clear()
                for k in runs:                                        # the allocator's peak over one call
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    timed(runs[k], rf, gr, grad)
                    last.clear()
                    what[k]['peak_bytes'] = torch.cuda.max_memory_allocated() - base
                what['distance'] = dist
                what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
                what['c_over_a'] = what['c']['median_ms'] / what['a']['median_ms']
                spread = max(what[k]['max_ms'] - what[k]['min_ms'] for k in ('a', 'c'))
                what['c_slower_than_a_beyond_the_spread'] = what['c']['median_ms'] > what['a']['median_ms'] + spread
                print(mode, 'fwd+bwd' if grad else 'fwd', {k: round(v['median_ms'], 3) for k, v in what.items()
                                                           if isinstance(v, dict) and 'median_ms' in v},
                      'a/b', round(what['a_over_b'], 3), 'c/a', round(what['c_over_a'], 2), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
