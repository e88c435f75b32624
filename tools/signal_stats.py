r"""K2s / K2bs (the signal kernels of ``fused.signal_rfgr``) next to the shipped K2 with checkpoints, K2b, the trajectory
kernels K2t / K2bt and the composed route (trajectory + the torch reduction over the spins), each configuration in a
fresh process, timed with HIP events:

    python tools/signal_stats.py [--n 64] [--nT 2048] [--every 1,16,2048] [--nrx R] [--reps 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/signal_stats.py ...
    python tools/signal_stats.py --rocprof DIR [--every ...] [--out FILE.json]     # the kernel rows of that run

Configurations: ``k2ck`` (K2 writing checkpoints) and ``k2b`` (its adjoint), and per stride ``k2t`` / ``k2bt`` (the
trajectory kernels), ``sig`` / ``sigb`` (the signal forward with checkpoints and its adjoint, cotangents on both outputs)
and ``comp`` / ``compb`` (``fused._signal_composed``: forward, and forward + backward end to end).  fp32, the default
(precise) mode, the synthetic cube and pulse, one receive map -- with ``--nrx R`` a receive array of ``R`` coils (``rx`` gets
a coil axis; nothing else changes, so the same file times a checkout that runs one launch per coil).  The forward is timed around the call, the adjoint around
``torch.autograd.grad`` (``compb`` around both).  ``--rocprof DIR`` pairs the traced processes with the configurations
in start order and reports the kernel-only medians of the main kernel (and with its second pass).
Each line printed is one JSON record; ``--out`` writes them all with the derived ratios."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
FWD = ('k2ck', 'k2t', 'sig', 'comp')


def child(cfg, n, nT, every, reps, nrx=0):
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
    gen = torch.Generator().manual_seed(1)
    rx = (torch.rand(tuple(sp['M0'].shape[:-1]) + (2,) + ((nrx,) if nrx else ()), generator=gen) * 2 - 1).to(dev)
    args = (sp['M0'], rf, gr, sp['loc'])

    def forward():
        if cfg in ('k2t', 'k2bt'):
            return (fused.blochsim_rfgr_traj(*args, every=every, **kw).movedim(-2, 0),)
        if cfg in ('sig', 'sigb'):
            return fused.signal_rfgr(*args, every=every, rx=rx, return_Mo=True, **kw)
        if cfg in ('comp', 'compb'):
            return fused._signal_composed(*args, every, rx, kw)
        return (fused.blochsim_rfgr(*args, **kw),)

    out = forward()                                   # warm-up: library load, allocator
    g_out = tuple(torch.ones_like(o) for o in out)
    torch.autograd.grad(out, (rf, gr), g_out)
    del out
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if cfg in FWD:
            a.record()
            out = forward()
            b.record()
        elif cfg == 'compb':
            a.record()
            out = forward()
            torch.autograd.grad(out, (rf, gr), g_out)
            b.record()
        else:
            out = forward()
            a.record()
            torch.autograd.grad(out, (rf, gr), g_out)
            b.record()
        del out
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) for a, b in ev)
    rec = dict(cfg=cfg, every=every or None, n=n, nT=nT, spins=n ** 3, reps=reps, nrx=nrx or None,
               median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1],
               peak_bytes=torch.cuda.max_memory_allocated(), precision=mrphy_amd.precision.get())
    print(json.dumps(rec), flush=True)


def ratios(recs, key):
    base = {r['cfg']: r[key] for r in recs if r['every'] is None}
    by = {(r['cfg'], r['every']): r[key] for r in recs}
    for r in recs:
        e = r['every']
        if r['cfg'] in ('k2t', 'sig'):
            r['ratio_to_k2ck'] = r[key] / base['k2ck']
        elif r['cfg'] in ('k2bt', 'sigb'):
            r['ratio_to_k2b'] = r[key] / base['k2b']
        if r['cfg'] == 'sig' and ('k2t', e) in by:
            r['ratio_to_k2t'] = r[key] / by['k2t', e]
        if r['cfg'] == 'sigb' and ('k2bt', e) in by:
            r['ratio_to_k2bt'] = r[key] / by['k2bt', e]


def summarize(d, plan):
    r"""Kernel rows of a rocprofv3 csv run of this tool: per child process (in start order = plan order) the median
    duration of each of our kernels (``k_bloch_rfgr_*``, ``k_signal_*``); ``main_ms`` is the simulation kernel of the
    configuration's direction, ``with_p2_ms`` adds its second pass.  The composed route is reported by HIP events only."""
    import csv
    import glob
    import statistics
    ours_of = lambda rows: [r for r in rows if 'k_bloch_rfgr' in r['Kernel_Name'] or 'k_signal' in r['Kernel_Name']]  # noqa: E731
    procs = []
    for f in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        rows = list(csv.DictReader(open(f)))
        if ours_of(rows):
            procs.append((min(int(r['Start_Timestamp']) for r in rows), ours_of(rows)))
    procs.sort(key=lambda x: x[0])
    if len(procs) != len(plan):
        raise SystemExit(f'{len(procs)} traced processes with our kernels, {len(plan)} configurations')
    out = []
    for (cfg, e), (_, ours) in zip(plan, procs):
        if cfg in ('comp', 'compb'):
            continue
        # both directions end in the same second pass (k_bloch_rfgr_p2): a launch of it belongs to the main kernel that
        # ran before it, and is listed under that kernel's direction
        by, after = {}, ''
        fwd = lambda k: '_fwd' in k  # noqa: E731
        for r in sorted(ours, key=lambda r: int(r['Start_Timestamp'])):
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            if '_p2' in name:
                name += after
            else:
                after = ' after_fwd' if fwd(name) else ' after_bwd'
            by.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6)
        ks = {k: dict(calls=len(v), median_ms=statistics.median(v), min_ms=min(v)) for k, v in by.items()}
        mine = [k for k in ks if fwd(k) == (cfg in FWD)]
        rec = dict(cfg=cfg, every=e or None, kernels=ks,
                   main_ms=sum(ks[k]['median_ms'] for k in mine if '_p2' not in k),
                   with_p2_ms=sum(ks[k]['median_ms'] for k in mine))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ratios(out, 'main_ms')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nT', type=int, default=2048)
    ap.add_argument('--every', default='1,16,2048')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--nrx', type=int, default=0, help='receive coils: rx gets a coil axis of this length (0: none)')
    ap.add_argument('--skip', default='', help='comma-separated configurations to leave out (e.g. comp,compb)')
    ap.add_argument('--out')
    ap.add_argument('--child', nargs=2, metavar=('CFG', 'EVERY'))
    ap.add_argument('--rocprof', metavar='DIR')
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.n, a.nT, int(a.child[1]), a.reps, a.nrx)
    skip = set(a.skip.split(','))
    plan = [('k2ck', 0), ('k2b', 0)]
    for e in (int(x) for x in a.every.split(',')):
        plan += [(c, e) for c in ('k2t', 'k2bt', 'sig', 'sigb', 'comp', 'compb') if c not in skip]
    if a.rocprof:
        recs = summarize(a.rocprof, plan)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(dict(tool='tools/signal_stats.py --rocprof', timing='rocprofv3 --kernel-trace, kernel-only '
                               'medians per fresh process', records=recs), f, indent=1)
        return
    recs = []
    for cfg, e in plan:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', cfg, str(e), '--n', str(a.n), '--nT', str(a.nT),
               '--reps', str(a.reps), '--nrx', str(a.nrx)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f'{cfg} every={e}: exit {r.returncode}')
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    ratios(recs, 'median_ms')
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/signal_stats.py', timing='HIP events, median of reps, fresh process per config',
                           records=recs), f, indent=1)


if __name__ == '__main__':
    main()
