r"""The MAPS builds of K2b / K2bt (gradients w.r.t. ``loc``, ``Δf``, ``b1Map`` out of the fused adjoint's sweep) next to
the plain K2b / K2bt of the same library and to the two-kernel route that forms the same gradients, each configuration
in a fresh process, timed with HIP events:

    python tools/maps_grad_stats.py [--n 64] [--nT 2048] [--every 16] [--reps 10] [--out profiles/r11_maps_grad.json]

Configurations (fp32, the default precise mode, the synthetic cube and pulse, a smooth synthetic b1 map):
``k2b`` -- ``blochsim_rfgr``'s adjoint for ``rf, gr`` (the plain kernel); ``k2b_maps`` -- the same call with ``loc``,
``Δf``, ``b1Map`` requiring gradients too (mode 0 of the MAPS builds); ``k2bt`` / ``k2bt_maps`` -- the trajectory's
adjoint at the stride ``--every``, without and with the maps; ``composed`` -- ``rfgr2beff`` + ``blochsim`` for the
gradients of ``k2b_maps`` (K0, K1h, K3, K0's adjoint and the torch reductions of ``grad_Beff``).  The adjoint is timed
around ``torch.autograd.grad`` (kernel + second pass + folds).  ``k2b_maps`` and ``composed`` also report the rise of the
allocator's peak over forward + backward and the relative L2 of each map gradient against ``ref64``: the fp64 run of the
same problem through the fused route, whose gradients the child leaves in a scratch file.
Each line printed is one JSON record; ``--out`` writes them all with the derived ratios."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
MAPS = ('loc', 'Δf', 'b1Map')


def child(cfg, n, nT, every, reps, ref):
    sys.path.insert(0, ROOT)
    import torch
    import mrphy_amd
    from mrphy_amd import synth, fused, beffective, sims
    dev = torch.device('cuda:0')
    dtype = torch.float64 if cfg == 'ref64' else torch.float32
    # the fp32 problem, widened for the fp64 run: the same inputs bit for bit
    sp = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in synth.cube_spins(n, device=dev).items()}
    p = {k: v.to(dtype) for k, v in synth.pulse(nT, device=dev).items()}
    loc = sp['loc'].clone()
    r2 = (loc ** 2).sum(-1, keepdim=True)
    b1 = torch.cat((1 - 0.2 * r2 / r2.max(), 0.1 * loc[..., :1] / loc.abs().max()), dim=-1)   # (N, *Nd, xy): smooth, |b1| <= 1
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    with_maps = cfg in ('k2b_maps', 'k2bt_maps', 'composed', 'ref64')
    df = sp['Δf'].clone()
    for x in (loc, df, b1):
        x.requires_grad_(with_maps)
    wrt = (rf, gr) + ((loc, df, b1) if with_maps else ())
    kw = dict(Δf=df, b1Map=b1, γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    traj = cfg in ('k2bt', 'k2bt_maps')

    def forward():
        if traj:
            return fused.blochsim_rfgr_traj(sp['M0'], rf, gr, loc, every=every, **kw)
        if cfg == 'composed':
            beff = beffective.rfgr2beff(rf, gr, loc, Δf=df, b1Map=b1, γ=sp['γ'])
            return sims.blochsim(sp['M0'], beff, T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
        return fused.blochsim_rfgr(sp['M0'], rf, gr, loc, **kw)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = forward()                                   # warm-up: library load, allocator -- and the memory figure
    g_out = torch.ones_like(out.movedim(-2, 0) if traj else out)
    if traj:
        g_out = g_out.movedim(0, -2)                  # a view of time-major storage, as the loss would give it
    grads = torch.autograd.grad(out, wrt, g_out)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    nM = n ** 3
    rec = dict(cfg=cfg, every=every if traj else None, n=n, nT=nT, spins=nM, reps=reps,
               precision=mrphy_amd.precision.get(), peak_rise_bytes=peak, beff_bytes=nM * nT * 12)
    if cfg == 'ref64':
        torch.save({k: g.cpu() for k, g in zip(MAPS, grads[2:])}, ref)
        print(json.dumps(rec), flush=True)
        return
    if with_maps and not traj and ref and os.path.exists(ref):
        want = torch.load(ref)
        rec['rel_l2_vs_fp64'] = {k: float((g.double().cpu() - want[k]).norm() / want[k].norm())
                                 for k, g in zip(MAPS, grads[2:])}
    del grads
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        out = forward()
        a.record()
        torch.autograd.grad(out, wrt, g_out)
        b.record()
        del out
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) for a, b in ev)
    rec.update(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=2048)
    ap.add_argument('--every', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out')
    ap.add_argument('--child', metavar='CFG')
    ap.add_argument('--ref', metavar='FILE')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, a.nT, a.every, a.reps, a.ref)
    recs = []
    with tempfile.TemporaryDirectory(prefix='maps_grad_') as d:
        ref = os.path.join(d, 'ref64.pt')
        for cfg in ('ref64', 'k2b', 'k2b_maps', 'k2bt', 'k2bt_maps', 'composed'):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', cfg, '--ref', ref, '--n', str(a.n),
                   '--nT', str(a.nT), '--every', str(a.every), '--reps', str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f'{cfg}: exit {r.returncode}')
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    by = {r['cfg']: r for r in recs}
    by['k2b_maps']['ratio_to_k2b'] = by['k2b_maps']['median_ms'] / by['k2b']['median_ms']
    by['k2bt_maps']['ratio_to_k2bt'] = by['k2bt_maps']['median_ms'] / by['k2bt']['median_ms']
    by['composed']['ratio_to_k2b_maps'] = by['composed']['median_ms'] / by['k2b_maps']['median_ms']
    by['composed']['peak_ratio_to_k2b_maps'] = by['composed']['peak_rise_bytes'] / by['k2b_maps']['peak_rise_bytes']
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/maps_grad_stats.py', timing='HIP events around torch.autograd.grad, median of '
                           'reps, fresh process per config', records=recs), f, indent=1)


if __name__ == '__main__':
    main()
