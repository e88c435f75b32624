r"""What ``fused.ab_rfgr`` costs next to the two ways the same ``A, B`` were available before it.

    python tools/ab_rfgr_timing.py [--n 64] [--nT 1024] [--reps 10] [--wrt pulse|maps|consts|all] [--coils 1]
                                   [--out FILE.json]

Shape: n^3 spins x nT steps, fp32, one transmit coil with a ``b1Map`` and per-spin ``T1 / T2`` (the synthetic cube and
pulse of ``mrphy_amd.synth``), in ``precision('precise')`` and ``('fast')``, the forward alone (``torch.no_grad``) and
forward + backward of ``(A wA).sum() + (B wB).sum()`` w.r.t. ``rf`` and ``gr``.  Contenders:

  (a) ``fused.ab_rfgr``;
  (b) the four-column emulation: ONE ``fused.blochsim_rfgr`` call at batch 4 -- ``Mi = e_x, e_y, e_z`` with a zero offset
      ``E1 - 1`` and ``Mi = 0`` with the real one, through ``consts=`` -- which forms the field and the rotation four
      times per step: K2 / K2b, the kernels this tree had before (a);
  (c) ``beffective.rfgr2beff`` + ``beffective.beff2ab``: ``Beff`` and, with gradients, the columns' history in memory.

HIP events around each call (the loss and its backward included, the same few small torch kernels for all three), three
warm-up rounds, then ``--reps`` rounds that alternate the contenders in one process; reported per contender: median,
min, max and the quartiles of the rounds (the run-to-run spread), the allocator's peak over one call, and the relative
L2 distance of (a)'s ``A, B`` and gradients from (b)'s and (c)'s.  Needs the GPU; there is no other path.

``--wrt`` (default ``pulse``: everything above, the output keys unchanged, ``profiles/ab_rfgr_timing.json``) adds leaves to
forward + backward: ``maps`` -- ``loc, Δf, b1Map``; ``consts`` -- ``T1, T2``; ``all`` -- both (K2abb's MAPS / CONSTS builds
in (a); K2b's in (b), whose constants are then formed from ``T1, T2`` by differentiable torch ops and handed over as
``consts=``; ``beff2ab``'s own constant gradients in (c), the route ``ab_rfgr`` took for these gradients before it had the
builds).  The default output is then ``profiles/ab_rfgr_spin_grads_timing.json``, which also says whether (a)'s median lies
below (c)'s by more than the rounds' min - max spread (the larger of the two): the condition for (a) to replace (c).
These runs form the step constants with torch's own ``exp`` on the device (``constants_on('native')``), all three alike.

``--coils N`` (default 1: everything above) is the default run under parallel transmit: ``rf`` `(1, xy, nT, N)` with a
``b1Map`` `(1, nM, xy, N)`, gradients w.r.t. the pulse.  (a) is then K2ab-mc / K2abb-mc up to the coil capacity, (b) K2 / K2b's
parallel-transmit builds at batch 4, (c) the composed route ``ab_rfgr`` took under parallel transmit before (a) had
those kernels.  The default output is ``profiles/ab_rfgr_ptx_timing.json``, one entry ``coils<N>`` per coil count measured.
"""
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


def problem(n, nT, dev, coils=1):
    sp = synth.cube_spins(n, dtype=torch.float32, device=dev)
    p = synth.pulse(nT, dtype=torch.float32, device=dev)
    nM = n ** 3
    gen = torch.Generator().manual_seed(5)
    b1 = (torch.rand((1, nM, 2), generator=gen, dtype=torch.float64) * 0.4 + 0.8).float().to(dev)
    if coils > 1:
        # parallel transmit: every coil plays the synthetic waveform at a weight of its own (they add up to about one
        # coil's), through a map of its own
        wc = ((torch.rand(coils, generator=gen, dtype=torch.float64) * 0.5 + 0.75) / coils).float().to(dev)
        p = dict(p, rf=(p['rf'][..., None] * wc).contiguous())
        b1 = (torch.rand((1, nM, 2, coils), generator=gen, dtype=torch.float64) * 0.4 + 0.8).float().to(dev)
    idx = lambda m: torch.arange(m, dtype=torch.float64)  # noqa: E731
    wA = torch.sin(idx(nM * 9) * 0.61 + 1).reshape(1, nM, 3, 3).float().to(dev)
    wB = torch.sin(idx(nM * 3) * 0.37 + 0.3).reshape(1, nM, 3).float().to(dev)
    return sp, p, b1, wA, wB


WRT = {'pulse': ('rf', 'gr'), 'maps': ('rf', 'gr', 'loc', 'Δf', 'b1'), 'consts': ('rf', 'gr', 'T1', 'T2'),
       'all': ('rf', 'gr', 'loc', 'Δf', 'b1', 'T1', 'T2')}


def contenders_wrt(sp, p, wA, wB, loss=None):
    r"""``{name: run(L) -> loss}`` for ``--wrt maps | consts | all``: ``L`` holds ``rf, gr, loc, Δf, b1, T1, T2``, leaves
    where the gradient is wanted; each run also leaves its ``A, B`` in ``last[name]``.  ``loss(A, B, L)``: another scalar
    than ``(A wA).sum() + (B wB).sum()`` (``tools/steadystate_timing.py``: the steady state's)."""
    fin = loss or (lambda A, B, L: (A * wA).sum() + (B * wB).sum())
    γ, dt = sp['γ'], p['dt']
    nM = wB.shape[1]
    last = {}

    def factors(L):                     # differentiable when T1, T2 are leaves: the constants of (b) and (c)
        return torch.exp(-dt / L['T1']).reshape(1, nM), torch.exp(-dt / L['T2']).reshape(1, nM)

    def a(L):
        A, B = fused.ab_rfgr(L['rf'], L['gr'], L['loc'], Δf=L['Δf'], b1Map=L['b1'], γ_beff=γ, T1=L['T1'], T2=L['T2'],
                             γ=γ, dt=dt)
        last['a'] = (A, B)
        return fin(A, B, L)

    Mi4 = torch.zeros((4, nM, 3), dtype=torch.float32, device=wB.device)
    for j in range(3):
        Mi4[j, :, j] = 1
    w4 = torch.cat((wA[0].permute(2, 0, 1), wB), dim=0).contiguous()
    γ2πdt = sims.relax_constants(None, None, γ, dt, 4, wB.device)[0]

    def b(L):
        E1, E2 = factors(L)
        e = lambda x: x.expand((4,) + tuple(x.shape[1:]))  # noqa: E731
        off4 = torch.cat((torch.zeros_like(E1).expand(3, nM), E1 - 1), dim=0)
        Mo = fused.blochsim_rfgr(Mi4, L['rf'], L['gr'], e(L['loc']), Δf=e(L['Δf']), b1Map=e(L['b1']), γ_beff=γ,
                                 consts=dict(γ2πdt=γ2πdt, E1=e(E1), E2=e(E2), E1_1=off4))
        last['b'] = (Mo[:3].permute(1, 2, 0)[None], Mo[3][None])
        return (Mo * w4).sum() if loss is None else loss(*last['b'], L)

    def c(L):
        E1, E2 = factors(L)
        beff = beffective.rfgr2beff(L['rf'], L['gr'], L['loc'], Δf=L['Δf'], b1Map=L['b1'], γ=γ)
        A, B = beffective.beff2ab(beff, E1=E1, E2=E2, γ=γ, dt=dt)
        last['c'] = (A, B)
        return fin(A, B, L)

    return {'a': a, 'b': b, 'c': c}, last


def timed_wrt(run, L0, wrt):
    r"""Milliseconds of forward + backward of ``run`` w.r.t. the operands named in ``wrt``, between two HIP events; the
    gradients by name."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    L = {k: (x.detach().requires_grad_(True) if k in wrt else x) for k, x in L0.items()}
    t0.record()
    g = torch.autograd.grad(run(L), [L[k] for k in wrt])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), dict(zip(wrt, g))


def main_wrt(args, dev, loss=None):
    r"""``--wrt maps | consts | all``: forward + backward only, the layout of the default run's entries.  ``loss(A, B, L, w)``
    with ``w`` `(1, nM, 3)`: see :func:`contenders_wrt`."""
    sp, p, b1, wA, wB = problem(args.n, args.nT, dev)
    wrt = WRT[args.wrt]
    L0 = dict(rf=p['rf'], gr=p['gr'], loc=sp['loc'], Δf=sp['Δf'], b1=b1, T1=sp['T1'], T2=sp['T2'])
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'wrt': list(wrt), 'beff_bytes': 12 * args.n ** 3 * args.nT, 'modes': {}}
    for mode in ('precise', 'fast'):
        # (b) and (c) are handed E1, E2 formed by torch's exp on the device: (a) forms its own the same way here, so that
        # the distances below compare kernels and not two roundings of E1 - 1
        with mrphy_amd.precision(mode), mrphy_amd.constants_on('native'):
            runs, last = contenders_wrt(sp, p, wA, wB, None if loss is None else (lambda A, B, L: loss(A, B, L, wB)))
            times, grads, failed = {k: [] for k in runs}, {}, {}
            for r in range(3 + args.reps):                           # three warm-up rounds, then alternate
                for k, run in list(runs.items()):
                    try:
                        ms, grads[k] = timed_wrt(run, L0, wrt)
                    except (RuntimeError, AssertionError, TypeError) as e:   # a contender that does not serve these
                        if k == 'a' or r > 0 or 'HIP' in str(e) or 'memory access' in str(e):   # gradients is left
                            raise                                            # out and named; a device error ends the run
                        failed[k] = f'{type(e).__name__}: {e}'[:300]
                        del runs[k], times[k]
                        continue
                    if r >= 3:
                        times[k].append(ms)
            what = {}
            for k, ts in times.items():
                q = statistics.quantiles(ts, n=4)
                what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0],
                           'q3_ms': q[2]}
            for k in runs:                                            # the allocator's peak over one call
                grads[k] = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                _, grads[k] = timed_wrt(runs[k], L0, wrt)
                what[k]['peak_bytes'] = torch.cuda.max_memory_allocated() - base
            dist = {f'{x}.from_{k}': rel_l2(u, w) for k in ('b', 'c') if k in runs for x, u, w in (
                [('A', last['a'][0], last[k][0]), ('B', last['a'][1], last[k][1])]
                + [('grad_' + n, grads['a'][n], grads[k][n]) for n in wrt])}
            if 'b' in runs:
                what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
            if 'c' in runs:
                spread = max(what[k]['max_ms'] - what[k]['min_ms'] for k in ('a', 'c'))
                what['a_over_c'] = what['a']['median_ms'] / what['c']['median_ms']
                what['a_below_c_by_more_than_the_spread'] = what['a']['median_ms'] < what['c']['median_ms'] - spread
            res['modes'][mode] = {'forward+backward': what, 'distance_of_a': dist, 'left_out': failed}
            print(mode, 'fwd+bwd wrt', args.wrt, {k: round(v['median_ms'], 3) for k, v in what.items()
                                                  if isinstance(v, dict)}, flush=True)
    return res


def contenders(sp, p, b1, wA, wB):
    r"""``{name: run(rf, gr) -> loss}`` -- each also leaves its ``A, B`` in ``last[name]``."""
    dev, nM = b1.device, b1.shape[1]
    γ, dt = sp['γ'], p['dt']
    γ2πdt, E1, E2, E1_1 = sims.relax_constants(sp['T1'], sp['T2'], γ, dt, 4, dev)
    # (b): batch 4 -- the columns e_x, e_y, e_z with a zero offset, the zero column with the real one
    Mi4 = torch.zeros((4, nM, 3), dtype=torch.float32, device=dev)
    for j in range(3):
        Mi4[j, :, j] = 1
    rep = lambda x: x.expand((4,) + tuple(x.shape[1:])).contiguous()  # noqa: E731
    loc4, df4, b14 = rep(sp['loc']), rep(sp['Δf']), rep(b1)
    e = lambda x: x.reshape(1, nM).expand(4, nM).contiguous()  # noqa: E731
    off4 = e(E1_1).clone()
    off4[:3] = 0
    consts4 = dict(γ2πdt=γ2πdt, E1=e(E1), E2=e(E2), E1_1=off4)
    w4 = torch.cat((wA[0].permute(2, 0, 1), wB), dim=0).contiguous()        # (4, nM, 3): column j of wA, then wB
    last = {}

    def a(rf, gr):
        A, B = fused.ab_rfgr(rf, gr, sp['loc'], Δf=sp['Δf'], b1Map=b1, γ_beff=γ, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
        last['a'] = (A, B)
        return (A * wA).sum() + (B * wB).sum()

    def b(rf, gr):
        Mo = fused.blochsim_rfgr(Mi4, rf, gr, loc4, Δf=df4, b1Map=b14, γ_beff=γ, consts=consts4)
        last['b'] = (Mo[:3].permute(1, 2, 0)[None], Mo[3][None])
        return (Mo * w4).sum()

    def c(rf, gr):
        beff = beffective.rfgr2beff(rf, gr, sp['loc'], Δf=sp['Δf'], b1Map=b1, γ=γ)
        A, B = beffective.beff2ab(beff, E1=E1.reshape(1, nM), E2=E2.reshape(1, nM), γ=γ, dt=dt)
        last['c'] = (A, B)
        return (A * wA).sum() + (B * wB).sum()

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
    ap.add_argument('--wrt', choices=sorted(WRT), default='pulse')
    ap.add_argument('--coils', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.coils >= 1 and (args.coils == 1 or args.wrt == 'pulse'), \
        'parallel transmit: gradients w.r.t. the pulse only (the others compose in (a) as well)'
    args.out = args.out or os.path.join(ROOT, 'profiles', 'ab_rfgr_ptx_timing.json' if args.coils > 1 else
                                        'ab_rfgr_timing.json' if args.wrt == 'pulse' else 'ab_rfgr_spin_grads_timing.json')
    assert torch.cuda.is_available(), 'tools/ab_rfgr_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    if args.wrt != 'pulse':
        res = main_wrt(args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
        print('wrote', args.out)
        return
    sp, p, b1, wA, wB = problem(args.n, args.nT, dev, args.coils)
    rf, gr = p['rf'], p['gr']
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'beff_bytes': 12 * args.n ** 3 * args.nT, 'modes': {}}
    if args.coils > 1:
        res['coils'] = args.coils
    for mode in ('precise', 'fast'):
        with mrphy_amd.precision(mode):
            runs, last = contenders(sp, p, b1, wA, wB)
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
                for k in runs:                                        # the allocator's peak over one call
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    timed(runs[k], rf, gr, grad)
                    what[k]['peak_bytes'] = torch.cuda.max_memory_allocated() - base
                if grad:
                    out['distance_of_a'] = {
                        f'{x}.from_{k}': d for k in ('b', 'c') for x, d in (
                            ('A', rel_l2(last['a'][0], last[k][0])), ('B', rel_l2(last['a'][1], last[k][1])),
                            ('grad_rf', rel_l2(grads['a'][0], grads[k][0])),
                            ('grad_gr', rel_l2(grads['a'][1], grads[k][1])))}
                b_ = what['b']
                what['a_over_b'] = what['a']['median_ms'] / b_['median_ms']
                what['a_not_slower_than_b_beyond_its_spread'] = \
                    what['a']['median_ms'] <= b_['median_ms'] + (b_['max_ms'] - b_['min_ms'])
                print(mode, 'fwd+bwd' if grad else 'fwd', {k: round(v['median_ms'], 3) for k, v in what.items()
                                                           if isinstance(v, dict)}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.coils > 1:
        # one file for every coil count measured: {'coils4': ..., 'coils8': ...}
        try:
            with open(args.out) as f:
                res = dict(json.load(f), **{f'coils{args.coils}': res})
        except (OSError, ValueError):
            res = {f'coils{args.coils}': res}
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
