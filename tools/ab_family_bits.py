"""Same-bits evidence for the A, B-level family between two trees of this repository, on one GPU:

    python tools/ab_family_bits.py TREE_A TREE_B [--limit SECONDS]

starts one fresh child process in each tree root (`--child`, its own time limit, default 300 s; a child that fails or runs
out of time ends the run and nothing more is started) and compares what they print, line by line: the number of tensors
compared and of lines that differ; the exit code is 0 when none differs.

    python tools/ab_family_bits.py --child

is the child: it imports `mrphy_amd` from the tree it is STARTED IN (the working directory, whichever tree holds this
file), runs a seeded program on `cuda:0` and prints one line per tensor, its name and its integer-view sum.  The program
uses public functions only, so a tree from before a host-side change runs it unchanged: `fused.ab_steadystate`,
`ab_train`, `train_signal`, `ab_sequence`, `sequence_signal` and `sequence_steadystate`; fp32 and fp64; the shapes
`(N, nM, K)` = (1, 1, 1), (2, 100, 2), (2, 100, 7), (2, 65, S + 3), (1, 257, S + 3), (2, 200, 40), (1, 300, 3), (2, 65, 1)
with S = `mrphy_train_signal_ck_every()`, with per-spin and with shared operands; the sequences on a bank of 3 with runs,
changes and an entry never played; `rest` as `()`, `(N,)` and -- the sequences -- `(1, K)` with a repeat and a zero; the
signals with no map, 1, 3, 8 and capacity + 1 receive coils, with `demod`, with both cotangents and with each alone;
every output and every gradient.  Nothing outside the two trees is read.  Not a test: pytest does not collect it.
"""
import os
import subprocess
import sys

SHAPES = ((1, 1, 1), (2, 100, 2), (2, 100, 7), (2, 65, 'S+3'), (1, 257, 'S+3'), (2, 200, 40), (1, 300, 3), (2, 65, 1))


def parent(trees, limit, script=__file__):
    r"""``script --child`` in each tree; ``tools/moving_shim_bits.py`` runs its own child through this."""
    outs = []
    for tree in trees:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(script), '--child'], cwd=tree, capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f'{tree}: the child did not finish in {limit} s; nothing more is started')
        if r.returncode != 0:
            sys.exit(f'{tree}: the child ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}')
        outs.append(r.stdout.splitlines())
        print(f'{tree}: {len(outs[-1])} tensors', flush=True)
    a, b = outs
    differ = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in differ[:40]:
        print(f'- {x}\n+ {y}')
    if len(a) != len(b):
        print(f'the trees printed {len(a)} and {len(b)} lines')
    print(f'{min(len(a), len(b))} tensors compared, {len(differ)} lines differ')
    sys.exit(0 if not differ and len(a) == len(b) and a else 1)


def child():
    root = os.getcwd()
    sys.path.insert(0, root)
    import torch
    import mrphy_amd
    from mrphy_amd import fused
    assert os.path.realpath(os.path.dirname(os.path.dirname(mrphy_amd.__file__))) == os.path.realpath(root), mrphy_amd.__file__
    lib = mrphy_amd.require_library()
    dev = torch.device('cuda', 0)
    S = int(lib.mrphy_train_signal_ck_every())

    def bits(x):
        return int(x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64).to(torch.int64).sum())

    def weighted(o):          # a cotangent that differs from element to element
        return (o * torch.sin(torch.arange(o.numel(), device=dev) * 0.61 + 1).to(o.dtype).reshape(o.shape)).sum()

    def run(label, fn, operands, outputs=None):
        r"""``fn(**operands)`` with every tensor operand requiring grad; ``outputs``: which of the results carry a cotangent."""
        leaves = {k: v.clone().requires_grad_(True) for k, v in operands.items() if isinstance(v, torch.Tensor) and
                  v.dtype.is_floating_point}
        out = fn(**{**operands, **leaves})
        out = out if isinstance(out, tuple) else (out,)
        for i, o in enumerate(out):
            print(f'{label} out{i} {bits(o.detach())}')
        sum(weighted(o) for i, o in enumerate(out) if outputs is None or i in outputs).backward()
        for k, v in leaves.items():
            print(f'{label} grad_{k} {"none" if v.grad is None else bits(v.grad)}')

    for dt in (torch.float32, torch.float64):
        cap = int(lib.mrphy_train_signal_max_rx(0 if dt == torch.float32 else 1))
        for N, nM, K in SHAPES:
            K = S + 3 if K == 'S+3' else K
            for shared in (False, True):
                g = torch.Generator(device='cpu').manual_seed(1000 * N + nM + 7 * K + shared)
                rnd = lambda *sh: torch.rand(sh, generator=g, dtype=torch.float64)  # noqa: E731
                on = lambda x: x.to(dt).to(dev)  # noqa: E731
                P = 3
                A = on(0.4 * torch.eye(3, dtype=torch.float64) + 0.3 * rnd(P, N, nM, 3, 3) - 0.15)
                B = on(0.2 * rnd(P, N, nM, 3))
                n1, m1 = (1, 1) if shared else (N, nM)
                Mi, phase = on(rnd(n1, m1, 3)), on(6 * rnd(n1, K) - 3)
                T1, T2, df = on(0.5 + rnd(n1, m1)), on(0.05 + 0.1 * rnd(n1, m1)), on(100 * rnd(n1, m1) - 50)
                table = 4e-3 + 2e-3 * rnd(1, K)
                table[:, K // 2] = 0                            # no rest before this pulse
                if K > 2:
                    table[:, 1] = table[:, 0]                   # a repeat: no refresh of the constants
                rests = {'()': on(torch.tensor(5e-3, dtype=torch.float64)), '(N,)': on(4e-3 + 2e-3 * rnd(N)), '(1,K)': on(table)}
                pulse = [(0, 0, 2, 2, 0, 2, 0)[k % 7] for k in range(K)]        # entry 1 is never played
                coils = {0: None, **{c: on(2 * rnd(n1, nM, 2, c) - 1) for c in (3, 8, cap + 1)}, 1: on(2 * rnd(n1, nM, 2) - 1)}
                tag = f'{str(dt)[6:]} ({N},{nM},{K}) {"shared" if shared else "per-spin"}'
                common = dict(T1=T1, T2=T2, Δf=df)
                for name, rest in rests.items():
                    one = name != '(1,K)'
                    if one:
                        run(f'{tag} ab_steadystate rest={name}', fused.ab_steadystate, dict(A=A[0], B=B[0], rest=rest, **common))
                        run(f'{tag} ab_train rest={name}', fused.ab_train,
                            dict(A=A[0], B=B[0], Mi=Mi, phase=phase, rest=rest, **common))
                    seq = dict(A=A, B=B, pulse=pulse, phase=phase, rest=rest, **common)
                    run(f'{tag} ab_sequence rest={name}', fused.ab_sequence, dict(Mi=Mi, **seq))
                    run(f'{tag} sequence_steadystate rest={name}', fused.sequence_steadystate, seq)
                    for c, rx in coils.items():
                        # each cotangent alone and the demodulated signal at 3 coils, both cotangents at every count
                        forms = (('both', None, False), ('sig', (0,), False), ('Mlast', (1,), False), ('demod', None, True)) \
                            if c == 3 else (('both', None, False),)
                        for what, outputs, demod in forms:
                            sig = dict(Mi=Mi, rx=rx, demod=demod, return_last=True)
                            if one:
                                run(f'{tag} train_signal rest={name} coils={c} {what}', fused.train_signal,
                                    dict(A=A[0], B=B[0], phase=phase, rest=rest, **common, **sig), outputs)
                            run(f'{tag} sequence_signal rest={name} coils={c} {what}', fused.sequence_signal,
                                dict(**seq, **sig), outputs)
    torch.cuda.synchronize()


def main(doc, child, script):
    if sys.argv[1:] == ['--child']:
        child()
    else:
        args, limit = sys.argv[1:], 300
        if '--limit' in args:
            i = args.index('--limit')
            limit = float(args[i + 1])
            del args[i:i + 2]
        if len(args) != 2:
            sys.exit(doc)
        parent(args, limit, script)


if __name__ == '__main__':
    main(__doc__, child, __file__)
