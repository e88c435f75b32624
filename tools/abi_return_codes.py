"""What entry points of two builds of the library answer BEFORE any launch, compared call by call, without a GPU:

    python tools/abi_return_codes.py LIB_A LIB_B NAME [NAME ...]

starts one fresh child process per library (`--child LIB NAME ...`), which loads that `libmrphy_hip.so` with ctypes, binds
the named entry points by `mrphy_amd._lib.PROTOTYPES` of THIS tree, makes the calls of the sweep below with fake addresses
and prints one line per call: the name, the arguments, the value returned.  The parent compares the two outputs line by
line and prints the number of calls and of mismatches per name; the exit code is 0 when nothing differs.

Nothing can launch: in EVERY call `loc` or `g` -- required by every launching entry point of the fused family, at any
size (csrc/abi.hip: check_ops) -- is null, which the child asserts before it calls.  So the answers seen are 0 (an empty
problem) and MRPHY_EINVAL from the checks in front of the operands' -- dtype and sizes, the mode arguments, the empty
problem, the entry point's own pointers -- and MRPHY_EINVAL from the operands' check where those pass; a change in the
order of the checks shows as 0 against MRPHY_EINVAL.  The size queries are called over their whole grid.

The sweep knows the entry points of the Bz-extended family (moving, shim): what each 64-bit integer after the operands
means is written down in ROLES and checked against the prototype's integer count.  Per launching entry point:
  * the product of the dtype codes -1 .. 5, N, nM, nT in {-1, 0, 1, 16, 17, 65536}, nS in {0, 1, 4, 8, 9}, step0 in
    {-1, 0, 2^23 - 16, 2^23}, nC in {0, 1, 2}, ck_every in {0, 4, 8, 12, 16}, the workspace exact (by the library's own
    query) and one byte short -- each with `g` null and with `loc` null;
  * on six bases (a whole problem in fp32 and fp64, a ragged nT, nT = 0, N = 0, nM = 0): each pointer alone, and each pair
    of pointers, null or misaligned (an odd address), in all combinations.
"""
import ctypes
import itertools
import os
import subprocess
import sys

FAKE = 4096
SIZES = (-1, 0, 1, 16, 17, 65536)
VALUES = {'dtype': tuple(range(-1, 6)), 'N': SIZES, 'nM': SIZES, 'nT': SIZES, 'nS': (0, 1, 4, 8, 9),
          'step0': (-1, 0, (1 << 23) - 16, 1 << 23), 'nC': (0, 1, 2), 'ck_every': (0, 4, 8, 12, 16), 'sh_sn': (0,)}
BASE = dict(dtype=0, N=1, nM=16, nT=16, nS=4, step0=0, nC=1, ck_every=16, sh_sn=0)
BASES = (BASE, dict(BASE, dtype=1), dict(BASE, nT=17), dict(BASE, nT=0), dict(BASE, N=0), dict(BASE, nM=0))
# what the 64-bit integers after the fused family's operands are, in order; the queries: after the dtype code
ROLES = {
    'mrphy_blochsim_rfgr_moving_fwd': ('step0', 'ck_every', 'N', 'nM', 'nT', 'nC'),
    'mrphy_blochsim_rfgr_moving_bwd': ('step0', 'N', 'nM', 'nT'),
    'mrphy_blochsim_rfgr_shim_fwd': ('sh_sn', 'nS', 'ck_every', 'N', 'nM', 'nT', 'nC'),
    'mrphy_blochsim_rfgr_shim_bwd': ('sh_sn', 'nS', 'N', 'nM', 'nT'),
    'mrphy_blochsim_rfgr_shim_max_channels': (),
    'mrphy_blochsim_rfgr_shim_bwd_workspace': ('N', 'nM', 'nT', 'nS'),
}
WORKSPACE = {'mrphy_blochsim_rfgr_moving_bwd': ('mrphy_blochsim_rfgr_bwd_workspace', ('N', 'nM', 'nT')),
             'mrphy_blochsim_rfgr_shim_bwd': ('mrphy_blochsim_rfgr_shim_bwd_workspace', ('N', 'nM', 'nT', 'nS'))}


def child(path, names):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
    from mrphy_amd import _lib
    vp, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    lib = ctypes.CDLL(path)

    def bind(name):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
        return fn

    n_ops = len(_lib._FUSED)                    # dtype, Mi / Mck, the operands rf .. E1m1
    loc_at, g_at = 2 + 4, 2 + 12                # (tests/util.py: FUSED_OP_AT, behind dtype and Mi / Mck)
    for name in names:
        fn, (_, argtypes) = bind(name), _lib.PROTOTYPES[name]
        roles = ROLES[name]
        if argtypes[-1] is not vp:              # a query: dtype, then its integers -- the whole grid
            assert argtypes == [ctypes.c_int] + [i64] * len(roles), name
            for v in itertools.product(VALUES['dtype'], *(VALUES[r] for r in roles)):
                print(name, *v, '->', fn(*v))
            continue
        assert argtypes[:n_ops] == _lib._FUSED and argtypes[loc_at] is vp and argtypes[g_at] is vp, name
        ints = [i for i in range(n_ops, len(argtypes)) if argtypes[i] is i64]
        assert len(ints) == len(roles), (name, len(ints), roles)
        ptrs = [i for i in range(1, len(argtypes) - 1) if argtypes[i] is vp]      # every pointer but the stream
        work_at = [i for i, t in enumerate(argtypes) if t is sz]
        query = WORKSPACE.get(name)
        wfn = bind(query[0]) if query else None

        def call(scalars, short, pointers):
            r"""``scalars``: by role; ``short``: bytes short of the query's workspace; ``pointers``: position -> address."""
            a = [None if t is vp else 0 for t in argtypes]
            a[0] = scalars['dtype']
            for i, r in zip(ints, roles):
                a[i] = scalars[r]
            for i in ptrs:
                a[i] = pointers.get(i, FAKE)
            if work_at:
                a[work_at[0]] = max(int(wfn(scalars['dtype'], *(scalars[r] for r in query[1]))) - short, 0)
            assert (a[loc_at] is None or a[g_at] is None) and a[-1] is None, 'a call that could launch'
            print(name, *a[:-1], '->', fn(*a))

        swept = ('dtype',) + tuple(r for r in roles if len(VALUES[r]) > 1)
        for v in itertools.product(*(VALUES[r] for r in swept)):
            for short in ((0, 1) if work_at else (0,)):
                for null in (g_at, loc_at):
                    call(dict(BASE, **dict(zip(swept, v))), short, {null: None})
        states = (None, FAKE + 1)               # null; misaligned
        for base in BASES:
            for k in (1, 2):
                for at in itertools.combinations(ptrs, k):
                    for st in itertools.product(states, repeat=k):
                        p = dict(zip(at, st))
                        if p.get(loc_at, FAKE) is not None:
                            p[g_at] = None      # (replaces a misaligned g: that state is then seen with loc null only)
                        call(base, 0, p)


def parent(lib_a, lib_b, names):
    outs = []
    for path in (lib_a, lib_b):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', os.path.abspath(path), *names],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f'{path}: the child ended with status {r.returncode}\n{r.stderr[-2000:]}')
        outs.append(r.stdout.splitlines())
    a, b = outs
    if len(a) != len(b):
        sys.exit(f'the libraries were asked {len(a)} and {len(b)} calls')
    differ = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in differ[:40]:
        print(f'- {x}\n+ {y}')
    for name in names:
        answers = {}
        for x in a:
            if x.startswith(name + ' '):
                v = x.rsplit(' ', 1)[1]
                answers[v] = answers.get(v, 0) + 1
        bad = sum(1 for x, _ in differ if x.startswith(name + ' '))
        seen = f'; answers of A: {dict(sorted(answers.items()))}' if len(answers) < 8 else ''      # (a size query has many)
        print(f'{name}: {sum(answers.values())} calls, {bad} mismatches{seen}')
    print(f'{len(a)} calls compared, {len(differ)} mismatches')
    sys.exit(1 if differ or not a else 0)


if __name__ == '__main__':
    if sys.argv[1:2] == ['--child']:
        child(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) < 4 or any(n not in ROLES for n in sys.argv[3:]):
        sys.exit(__doc__)
    else:
        parent(sys.argv[1], sys.argv[2], sys.argv[3:])
