"""Same-bits evidence for `fused.blochsim_rfgr_moving` and `fused.blochsim_rfgr_shim` between two trees of this repository,
on one GPU:

    python tools/moving_shim_bits.py TREE_A TREE_B [--limit SECONDS]

`tools/ab_family_bits.py`'s parent half (one fresh child per tree, its own time limit, the outputs compared line by line)
around this file's own child:

    python tools/moving_shim_bits.py --child

imports `mrphy_amd` from the tree it is STARTED IN, runs a seeded program on `cuda:0` and prints one line per tensor, its
name and its integer-view sum.  Public functions only, so a tree from before a host-side change runs it unchanged.  fp32
in `precision('precise')` and `('fast')`, and fp64; the shapes `(N, nM, nT)` = (1, 1, 16), (2, 100, 16), (2, 65, 48),
(1, 257, 32), (2, 100, 40) (the split route), (2, 100, 5) (forward only: a gradient there is composed) and, fp32 only,
(1, 131172, 16): more tiles than persistent waves; every kernel build of the axes b1Map x relaxation, with Δf where there
is a map or none of the two; the moving call at `step0` 0 and 32 with `vel` `(1, ...)` and `(N, ...)`; the shim call at
`nS` in {1, 2, 3, 4, 5, 8, capacity + 1} with `sh` shared and per batch entry; every output, and every gradient w.r.t.
`Mi`, `rf`, `gr` (and `sh`).  Nothing outside the two trees is read.  Not a test: pytest does not collect it.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ab_family_bits  # noqa: E402

SHAPES = ((1, 1, 16), (2, 100, 16), (2, 65, 48), (1, 257, 32), (2, 100, 40), (2, 100, 5), (1, 131172, 16))
FIELDS = ((False, False, False), (True, True, True), (True, True, False), (False, False, True))   # b1Map, Δf, relaxation


def child():
    root = os.getcwd()
    sys.path.insert(0, root)
    import torch
    import mrphy_amd
    from mrphy_amd import fused
    assert os.path.realpath(os.path.dirname(os.path.dirname(mrphy_amd.__file__))) == os.path.realpath(root), mrphy_amd.__file__
    lib = mrphy_amd.require_library()
    dev = torch.device('cuda', 0)

    def bits(x):
        return int(x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64).to(torch.int64).sum())

    def run(label, fn, operands, leaves, grad):
        r"""``fn(**operands)``; with ``grad`` the operands named in ``leaves`` require grad and the loss weights every element."""
        if not grad:
            with torch.no_grad():
                print(f'{label} Mo {bits(fn(**operands))}')
            return
        ops = {k: (v.clone().requires_grad_(True) if k in leaves else v) for k, v in operands.items()}
        Mo = fn(**ops)
        print(f'{label} Mo {bits(Mo.detach())}')
        (Mo * torch.sin(torch.arange(Mo.numel(), device=dev) * 0.61 + 1).to(Mo.dtype).reshape(Mo.shape)).sum().backward()
        for k in leaves:
            print(f'{label} grad_{k} {"none" if ops[k].grad is None else bits(ops[k].grad)}')

    for dt, mode in ((torch.float32, 'precise'), (torch.float32, 'fast'), (torch.float64, 'precise')):
        cap = int(lib.mrphy_blochsim_rfgr_shim_max_channels(0 if dt == torch.float32 else 1))
        for N, nM, nT in SHAPES:
            if nM > 100000 and dt == torch.float64:
                continue
            grad = nT >= 16
            for b1, df, relax in FIELDS:
                g = torch.Generator(device='cpu').manual_seed(1000 * N + nM + 7 * nT + 4 * b1 + 2 * df + relax)
                rnd = lambda *sh: torch.rand(sh, generator=g, dtype=torch.float64)  # noqa: E731
                on = lambda x: x.to(dt).to(dev)  # noqa: E731
                base = dict(Mi=on(rnd(N, nM, 3)), rf=on(0.2 * rnd(N, 2, nT) - 0.1), gr=on(2 * rnd(N, 3, nT) - 1),
                            loc=on(10 * rnd(N, nM, 3) - 5))
                kw = dict(Δf=on(100 * rnd(N, nM) - 50) if df else None, b1Map=on(0.8 + 0.4 * rnd(N, nM, 2)) if b1 else None,
                          T1=on(0.5 + rnd(N, nM)) if relax else None, T2=on(0.05 + 0.1 * rnd(N, nM)) if relax else None)
                vels = {'(1,)': on(20 * rnd(1, nM, 3) - 10), '(N,)': on(20 * rnd(N, nM, 3) - 10)}
                tag = f'{str(dt)[6:]} {mode} ({N},{nM},{nT}) b1={int(b1)} df={int(df)} relax={int(relax)}'
                with mrphy_amd.precision(mode):
                    for step0 in (0, 32):
                        for name, vel in vels.items():
                            run(f'{tag} moving step0={step0} vel={name}', fused.blochsim_rfgr_moving,
                                dict(base, vel=vel, step0=step0, **kw), ('Mi', 'rf', 'gr'), grad)
                    for nS in (1, 2, 3, 4, 5, 8, cap + 1):
                        shMap = on(0.1 * rnd(N, nM, nS) - 0.05)
                        for name, n1 in (('shared', 1), ('per-batch', N)):
                            run(f'{tag} shim nS={nS} sh={name}', fused.blochsim_rfgr_shim,
                                dict(base, sh=on(2 * rnd(n1, nS, nT) - 1), shMap=shMap, **kw), ('Mi', 'rf', 'gr', 'sh'), grad)
    torch.cuda.synchronize()


if __name__ == '__main__':
    ab_family_bits.main(__doc__, child, __file__)
