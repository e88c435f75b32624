r"""What extra Bz field channels cost in ``fused.blochsim_rfgr_shim``, and what the route there was before it costs.

    python tools/shim_timing.py [--n 64] [--nT 1024] [--reps 10] [--channels 2 4 8] [--out FILE.json]

Shape: n^3 spins x nT steps, fp32, one transmit coil with a ``b1Map`` and per-spin ``T1 / T2`` (the synthetic cube and pulse
of ``mrphy_amd.synth``), ``nS`` = 2, 4, 8 channels with waveforms seeded uniform in +-1 and maps seeded uniform in +-0.05 G
per unit, in ``precision('precise')`` and ``('fast')``, the forward alone (``torch.no_grad``) and forward + backward of
``(Mo w).sum()`` w.r.t. ``rf``, ``gr`` and ``sh``.  Contenders:

  (a) ``fused.blochsim_rfgr_shim`` (K2sh; K2sh with checkpoints + K2shb);
  (b) ``fused.blochsim_rfgr`` on the same problem without channels (K2; K2 with checkpoints + K2b), the floor: (a) over
      (b) is what the channels cost;
  (c) the composed route, which is what there was before: ``rfgr2beff``, ``einsum(shMap, sh)`` added to its z component in
      torch, then ``sims.blochsim`` -- ``Beff`` and, with gradients, ``grad_Beff`` and the history in memory.

HIP events around each call (the loss and its backward included, the same small torch kernels for all three), three
warm-up rounds, then ``--reps`` rounds that alternate the contenders in one process; reported per contender: median, min,
max and the quartiles of the rounds, the allocator's peak over one call, the ratios a / b and c / a, the one condition --
(a)'s range of rounds lies wholly below (c)'s -- and the relative L2 distance of (a)'s ``Mo`` and gradients from (c)'s.
``PREDICTED`` is the ratio a / b written down before the first measurement, from the step loops' instruction counts
(DESIGN.md section 3, K2sh / K2shb); it is copied into the result beside the measured one.  No time is fixed in advance.
Needs the GPU; there is no other path.  -> ``profiles/shim_timing.json``."""
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

# a / b predicted before anything was timed, from instruction counts: the capacity's MS FMAs per step (2, 4, 8 for
# nS = 2, 4, 8) on K2's step of 41 VALU instructions (precise, relaxation, b1 map: DESIGN.md section 3, K2v) forward; in
# the adjoint 2 MS per step (recompute and sweep) on the segment's 3 400 instructions per 16 steps, a quarter of forward +
# backward being the forward: {nS: (forward, forward + backward)}
PREDICTED = {2: (1.05, 1.03), 4: (1.10, 1.05), 8: (1.20, 1.11)}


def problem(n, nT, nS, dev):
    sp = synth.cube_spins(n, dtype=torch.float32, device=dev)
    p = synth.pulse(nT, dtype=torch.float32, device=dev)
    nM = n ** 3
    gen = torch.Generator().manual_seed(5)
    b1 = (torch.rand((1, nM, 2), generator=gen, dtype=torch.float64) * 0.4 + 0.8).float().to(dev)
    sh = (torch.rand((1, nS, nT), generator=gen, dtype=torch.float64) * 2 - 1).float().to(dev)
    m = ((torch.rand((1, nM, nS), generator=gen, dtype=torch.float64) * 2 - 1) * 0.05).float().to(dev)
    w = torch.sin(torch.arange(nM * 3, dtype=torch.float64) * 0.61 + 1).reshape(1, nM, 3).float().to(dev)
    return sp, p, b1, sh, m, w


def contenders(sp, p, b1, m, w):
    r"""``{name: run(rf, gr, sh) -> loss}`` -- each also leaves its ``Mo`` in ``last[name]``."""
    γ, dt = sp['γ'], p['dt']
    kw = dict(Δf=sp['Δf'], b1Map=b1, γ_beff=γ, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
    last = {}

    def a(rf, gr, sh):
        last['a'] = Mo = fused.blochsim_rfgr_shim(sp['M0'], rf, gr, sp['loc'], sh, m, **kw)
        return (Mo * w).sum()

    def b(rf, gr, sh):
        last['b'] = Mo = fused.blochsim_rfgr(sp['M0'], rf, gr, sp['loc'], **kw)
        return (Mo * w).sum()

    def c(rf, gr, sh):
        beff = beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], b1Map=b1, γ=γ, lazy=False)
        beff = beff + torch.nn.functional.pad(fused._shim_bz(sh, m).unsqueeze(-1), (2, 0))
        last['c'] = Mo = sims.blochsim(sp['M0'], beff, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
        return (Mo * w).sum()

    return {'a': a, 'b': b, 'c': c}, last


def timed(name, run, ops, grad):
    r"""Milliseconds of one call between two HIP events; the gradients w.r.t. rf, gr (and sh, where the call has it)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if grad:
        ops = [x.detach().requires_grad_(True) for x in ops]
        t0.record()
        g = torch.autograd.grad(run(*ops), ops[:2] if name == 'b' else ops)
        t1.record()
    else:
        with torch.no_grad():
            t0.record()
            run(*ops)
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
    ap.add_argument('--channels', type=int, nargs='+', default=[2, 4, 8])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shim_timing.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/shim_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'beff_bytes': 12 * args.n ** 3 * args.nT, 'channels': {}}
    for nS in args.channels:
        sp, p, b1, sh, m, w = problem(args.n, args.nT, nS, dev)
        ops = (p['rf'], p['gr'], sh)
        per = res['channels'][str(nS)] = {'predicted_a_over_b': dict(zip(('forward', 'forward+backward'),
                                                                       PREDICTED.get(nS, (None, None)))), 'modes': {}}
        for mode in ('precise', 'fast'):
            with mrphy_amd.precision(mode):
                runs, last = contenders(sp, p, b1, m, w)
                out = per['modes'][mode] = {}
                for grad in (False, True):
                    times = {k: [] for k in runs}
                    grads = {}
                    for r in range(3 + args.reps):                       # three warm-up rounds, then alternate
                        for k, run in runs.items():
                            ms, g = timed(k, run, ops, grad)
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
                        dist.update({f'grad_{n}.a_from_c': rel_l2(grads['a'][i], grads['c'][i])
                                     for i, n in enumerate(('rf', 'gr', 'sh'))})
                    grads.clear()
                    last.clear()
                    for k in runs:                                        # the allocator's peak over one call
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        timed(k, runs[k], ops, grad)
                        last.clear()
                        what[k]['peak_bytes'] = torch.cuda.max_memory_allocated() - base
                    what['distance'] = dist
                    what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
                    what['c_over_a'] = what['c']['median_ms'] / what['a']['median_ms']
                    what['a_range_wholly_below_c_range'] = what['a']['max_ms'] < what['c']['min_ms']
                    print(nS, mode, 'fwd+bwd' if grad else 'fwd',
                          {k: f"{v['median_ms']:.3f} ({v['min_ms']:.3f} - {v['max_ms']:.3f})" for k, v in what.items()
                           if isinstance(v, dict) and 'median_ms' in v},
                          'a/b', round(what['a_over_b'], 3), 'c/a', round(what['c_over_a'], 2),
                          'a below c:', what['a_range_wholly_below_c_range'], flush=True)
        del sp, p, b1, sh, m, w
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
