r"""What ``fused.steadystate_rfgr`` costs next to the same composition with the rest period and the solve in plain torch.

    python tools/steadystate_timing.py [--n 64] [--nT 1024] [--reps 10] [--wrt pulse|maps|consts|all] [--out FILE.json]

Shape: n^3 spins x nT steps, fp32, one transmit coil with a ``b1Map`` and per-spin ``T1 / T2`` (the problem of
``tools/ab_rfgr_timing.py``), a rest of 5 ms, in ``precision('precise')`` and ``('fast')``, the forward alone
(``torch.no_grad``) and forward + backward of ``(Mss w).sum()`` w.r.t. ``rf`` and ``gr``.  Contenders:

  (a) ``fused.steadystate_rfgr``: ``fused.ab_rfgr`` (K2ab / K2abb), then Kss / Kssb;
  (b) ``fused.ab_rfgr``, then ``F, f`` of the rest period by elementwise torch ops and ``torch.linalg.solve`` of
      ``(I - A F) Mss = A f + B`` on the device, autograd through all of it;

and, on a fixed ``A, B`` with gradients w.r.t. both, the part that differs alone:

  (ta) ``fused.ab_steadystate``;   (tb) the torch rest period and solve of (b).

HIP events around each call (the loss and its backward included), three warm-up rounds, then ``--reps`` rounds that
alternate the contenders in one process; reported per contender: median, min, max and the quartiles of the rounds, and
the relative L2 distance of (a)'s ``Mss`` and gradients from (b)'s.  Nothing is asserted: the file records what comes
out.  Needs the GPU; there is no other path.

``--wrt maps | consts | all`` (default ``pulse``: everything above, the output keys unchanged): forward + backward of
``(Mss w).sum()`` with ``loc, Δf, b1Map`` and / or ``T1, T2`` requiring grad as well, Kss / Kssb on the ``A, B`` of the three
contenders of ``tools/ab_rfgr_timing.py --wrt`` -- ``ab_rfgr``, the batch-4 emulation through ``blochsim_rfgr``, and
``rfgr2beff`` + ``beff2ab`` --, ``T1, T2, Δf`` shared by the pulse and the rest; default output
``profiles/steadystate_spin_grads_timing.json``.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrphy_amd  # noqa: E402
from mrphy_amd import fused  # noqa: E402
from ab_rfgr_timing import WRT, main_wrt, problem, rel_l2  # noqa: E402

REST = 5e-3


def torch_tail(A, B, rest, T1, T2, df):
    r"""``Mss`` from ``A, B`` with the rest period and the solve as plain torch ops (``T1, T2, df`` `(1, nM)`)."""
    φ = -2 * π * df * rest
    E1r, E2r, c, s = torch.exp(-rest / T1), torch.exp(-rest / T2), torch.cos(φ), torch.sin(φ)
    o = torch.zeros_like(c)
    F = torch.stack((torch.stack((E2r * c, -E2r * s, o), -1), torch.stack((E2r * s, E2r * c, o), -1),
                     torch.stack((o, o, E1r), -1)), -2)
    f = torch.stack((o, o, -torch.expm1(-rest / T1)), -1)
    C = torch.eye(3, dtype=A.dtype, device=A.device) - A @ F
    return torch.linalg.solve(C, (A @ f[..., None])[..., 0] + B)


def contenders(sp, p, b1, w):
    r"""``{name: run(rf, gr) -> loss}`` for the whole composition, ``{name: run(A, B) -> loss}`` for the tail alone; each
    leaves its ``Mss`` in ``last[name]``."""
    γ, dt = sp['γ'], p['dt']
    rest = torch.tensor(REST, dtype=torch.float32, device=b1.device)
    kw = dict(Δf=sp['Δf'], b1Map=b1, γ_beff=γ, T1=sp['T1'], T2=sp['T2'], γ=γ, dt=dt)
    last = {}

    def a(rf, gr):
        last['a'] = Mss = fused.steadystate_rfgr(rf, gr, sp['loc'], rest=rest, **kw)
        return (Mss * w).sum()

    def b(rf, gr):
        A, B = fused.ab_rfgr(rf, gr, sp['loc'], **kw)
        last['b'] = Mss = torch_tail(A, B, rest, sp['T1'], sp['T2'], sp['Δf'])
        return (Mss * w).sum()

    def ta(A, B):
        last['ta'] = Mss = fused.ab_steadystate(A, B, rest=rest, T1=sp['T1'], T2=sp['T2'], Δf=sp['Δf'])
        return (Mss * w).sum()

    def tb(A, B):
        last['tb'] = Mss = torch_tail(A, B, rest, sp['T1'], sp['T2'], sp['Δf'])
        return (Mss * w).sum()

    return {'a': a, 'b': b}, {'ta': ta, 'tb': tb}, last, kw


def timed(run, x, y, grad):
    r"""Milliseconds of one call between two HIP events; the gradients w.r.t. ``x, y`` (or None)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if grad:
        x, y = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        t0.record()
        g = torch.autograd.grad(run(x, y), (x, y))
        t1.record()
    else:
        with torch.no_grad():
            t0.record()
            run(x, y)
            t1.record()
        g = None
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), g


def rounds(runs, x, y, grad, reps):
    times, grads = {k: [] for k in runs}, {}
    for r in range(3 + reps):                                   # three warm-up rounds, then alternate
        for k, run in runs.items():
            ms, grads[k] = timed(run, x, y, grad)
            if r >= 3:
                times[k].append(ms)
    what = {}
    for k, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        what[k] = {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'q1_ms': q[0], 'q3_ms': q[2]}
    return what, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--wrt', choices=sorted(WRT), default='pulse')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, 'profiles', 'steadystate_timing.json' if args.wrt == 'pulse'
                                        else 'steadystate_spin_grads_timing.json')
    assert torch.cuda.is_available(), 'tools/steadystate_timing.py measures on the GPU'
    assert args.reps >= 10, 'the median of at least ten rounds'
    dev = torch.device('cuda:0')
    if args.wrt != 'pulse':
        rest = torch.tensor(REST, dtype=torch.float32, device=dev)
        res = main_wrt(args, dev, lambda A, B, L, w: (fused.ab_steadystate(
            A, B, rest=rest, T1=L['T1'], T2=L['T2'], Δf=L['Δf']) * w).sum())
        res['rest_s'] = REST
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
        print('wrote', args.out)
        return
    sp, p, b1, _, w = problem(args.n, args.nT, dev)
    rf, gr = p['rf'], p['gr']
    res = {'device': torch.cuda.get_device_name(0), 'n': args.n, 'nT': args.nT, 'dtype': 'float32', 'reps': args.reps,
           'rest_s': REST, 'modes': {}}
    for mode in ('precise', 'fast'):
        with mrphy_amd.precision(mode):
            whole, tail, last, kw = contenders(sp, p, b1, w)
            with torch.no_grad():
                A, B = fused.ab_rfgr(rf, gr, sp['loc'], **kw)
            out = res['modes'][mode] = {}
            for grad in (False, True):
                what, grads = rounds(whole, rf, gr, grad, args.reps)
                tw, tgrads = rounds(tail, A, B, grad, args.reps)
                what.update(tw)
                what['a_over_b'] = what['a']['median_ms'] / what['b']['median_ms']
                what['ta_over_tb'] = what['ta']['median_ms'] / what['tb']['median_ms']
                out['forward+backward' if grad else 'forward'] = what
                if grad:
                    out['distance_of_a_from_b'] = {'Mss': rel_l2(last['a'], last['b']), 'grad_rf': rel_l2(grads['a'][0], grads['b'][0]),
                                                   'grad_gr': rel_l2(grads['a'][1], grads['b'][1])}
                    out['distance_of_ta_from_tb'] = {'Mss': rel_l2(last['ta'], last['tb']),
                                                     'grad_A': rel_l2(tgrads['ta'][0], tgrads['tb'][0]),
                                                     'grad_B': rel_l2(tgrads['ta'][1], tgrads['tb'][1])}
                print(mode, 'fwd+bwd' if grad else 'fwd', {k: round(v['median_ms'], 3) for k, v in what.items()
                                                           if isinstance(v, dict)}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
