r"""K2t / K2bt (the trajectory kernels of ``fused.blochsim_rfgr_traj``) next to the shipped K2 with checkpoints and K2b,
each configuration in a fresh process, timed with HIP events:

    python tools/traj_stats.py [--n 64] [--nT 2048] [--every 1,16,2048] [--reps 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/traj_stats.py ...
    python tools/traj_stats.py --rocprof DIR [--every ...] [--out FILE.json]     # the kernel rows of that run

Configurations: ``k2ck`` (K2 writing checkpoints: what ``blochsim_rfgr`` runs when a gradient is wanted), ``k2b`` (its
adjoint), and per stride ``k2t`` (K2t with checkpoints) and ``k2bt`` (its adjoint, ``grad_Mt`` time-major).  fp32, the
default (precise) mode, the synthetic cube and pulse.  The forward is timed around the autograd Function's forward, the
adjoint around ``torch.autograd.grad`` (kernel + the fixed-order second pass + the pulse-gradient fold: the same for
both routes).  Under ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/traj_stats.py ...`` the children are
traced too, one directory per process; ``--rocprof DIR`` pairs the processes with the configurations in start order
and reports the kernel-only medians of K2 / K2t and of K2b / K2bt (+ their second pass).
Each line printed is one JSON record; ``--out`` writes them all with the derived ratios."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')


def child(cfg, n, nT, every, reps):
    sys.path.insert(0, ROOT)
    import torch
    import mrphy_amd
    from mrphy_amd import synth, fused
    dev = torch.device('cuda:0')
    sp = synth.cube_spins(n, device=dev)
    p = synth.pulse(nT, device=dev)
    rf = (0.05 * p['rf']).clone().requires_grad_(True)
    gr = p['gr'].clone().requires_grad_(True)
    kw = dict(Δf=sp['Δf'], γ_beff=sp['γ'], T1=sp['T1'], T2=sp['T2'], γ=sp['γ'], dt=p['dt'])
    traj = cfg in ('k2t', 'k2bt')

    def forward():
        if traj:
            return fused.blochsim_rfgr_traj(sp['M0'], rf, gr, sp['loc'], every=every, **kw)
        return fused.blochsim_rfgr(sp['M0'], rf, gr, sp['loc'], **kw)

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    times = []
    out = forward()                                   # warm-up: library load, allocator
    g_out = torch.ones_like(out.movedim(-2, 0) if traj else out)
    if traj:
        g_out = g_out.movedim(0, -2)                  # a view of time-major storage, as the loss would give it
    torch.autograd.grad(out, (rf, gr), g_out)
    torch.cuda.synchronize()
    for a, b in ev:
        if cfg in ('k2ck', 'k2t'):
            a.record()
            out = forward()
            b.record()
        else:
            out = forward()
            a.record()
            torch.autograd.grad(out, (rf, gr), g_out)
            b.record()
        del out
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) for a, b in ev)
    nM = n ** 3
    rec = dict(cfg=cfg, every=every if traj else None, n=n, nT=nT, spins=nM, reps=reps,
               median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1],
               mt_bytes=(-(-nT // every)) * nM * 12 if traj else 0, precision=mrphy_amd.precision.get())
    print(json.dumps(rec), flush=True)


def summarize(d, plan):
    r"""Kernel rows of a rocprofv3 csv run of this tool: per child process (in start order = plan order) the median
    duration of each of our kernels (``k_bloch_rfgr_*``)."""
    import csv
    import glob
    import statistics
    procs = []
    for f in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        rows = list(csv.DictReader(open(f)))
        ours = [r for r in rows if 'k_bloch_rfgr' in r['Kernel_Name']]
        if ours:
            procs.append((min(int(r['Start_Timestamp']) for r in rows), ours))
    procs.sort(key=lambda x: x[0])
    if len(procs) != len(plan):
        raise SystemExit(f'{len(procs)} traced processes with our kernels, {len(plan)} configurations')
    out = []
    for (cfg, e), (_, ours) in zip(plan, procs):
        by = {}
        for r in ours:
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            by.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6)
        ks = {k: dict(calls=len(v), median_ms=statistics.median(v), min_ms=min(v)) for k, v in by.items()}
        main_k = [k for k in ks if ('_fwd' in k) == (cfg in ('k2ck', 'k2t')) and '_p2' not in k]
        rec = dict(cfg=cfg, every=e or None, kernels=ks,
                   main_ms=sum(ks[k]['median_ms'] for k in main_k),
                   with_p2_ms=sum(ks[k]['median_ms'] for k in ks if ('_fwd' in k) == (cfg in ('k2ck', 'k2t'))))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    base = {r['cfg']: r['main_ms'] for r in out if r['every'] is None}
    for r in out:
        if r['cfg'] == 'k2t':
            r['ratio_to_k2ck'] = r['main_ms'] / base['k2ck']
        elif r['cfg'] == 'k2bt':
            r['ratio_to_k2b'] = r['main_ms'] / base['k2b']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=2048)
    ap.add_argument('--every', default='1,16,2048')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out')
    ap.add_argument('--child', nargs=2, metavar=('CFG', 'EVERY'))
    ap.add_argument('--rocprof', metavar='DIR')
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.n, a.nT, int(a.child[1]), a.reps)
    plan = [('k2ck', 0), ('k2b', 0)]
    for e in (int(x) for x in a.every.split(',')):
        plan += [('k2t', e), ('k2bt', e)]
    if a.rocprof:
        recs = summarize(a.rocprof, plan)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(dict(tool='tools/traj_stats.py --rocprof', timing='rocprofv3 --kernel-trace, kernel-only '
                               'medians per fresh process', records=recs), f, indent=1)
        return
    recs = []
    for cfg, e in plan:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', cfg, str(e), '--n', str(a.n), '--nT', str(a.nT),
               '--reps', str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f'{cfg} every={e}: exit {r.returncode}')
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    base = {r['cfg']: r['median_ms'] for r in recs if r['every'] is None}
    for r in recs:
        if r['cfg'] == 'k2t':
            r['ratio_to_k2ck'] = r['median_ms'] / base['k2ck']
            # the every = 1 store-bound figure: Mt bytes over the time, against the 8 TB/s peak
            r['mt_TBps'] = r['mt_bytes'] / (r['median_ms'] * 1e-3) / 1e12
        elif r['cfg'] == 'k2bt':
            r['ratio_to_k2b'] = r['median_ms'] / base['k2b']
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/traj_stats.py', timing='HIP events, median of reps, fresh process per config',
                           records=recs), f, indent=1)


if __name__ == '__main__':
    main()
