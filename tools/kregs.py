"""Register / LDS / scratch use of every kernel of the library, read from the code-object metadata of the
unit objects `mrphy_amd.build()` leaves under mrphy.py_amd/build/ (no recompilation):

    python tools/kregs.py [filter] [--scratch] [--objdir DIR]
    python tools/kregs.py [filter] --diff DIR_A DIR_B

The filter is looked for in the kernel's demangled name and in its unit object's name (`maps`: the kernels of
tu_fused_maps_bwd.hip).  `--scratch` lists only kernels with a private segment (spills); the exit code is then the number found.
`--objdir DIR` reads the unit objects of another build instead.
`--diff` compares two builds kernel by kernel (by unit object and kernel name): the register / LDS / scratch figures
and the count of every opcode of the disassembly; it names each kernel that differs with the opcodes and counts, and
the kernels only one build has.  The exit code is the number of kernels whose figures differ.
"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')


def kernels(objdir, flt=None):
    r"""[(object, demangled kernel name, {metadata})] for every kernel of every unit object in `objdir`.  With a
    filter `flt` on the demangled name the metadata also holds the kernel's instructions ('text': the lines of the
    disassembly) and their opcode counts ('ops')."""
    out, asm = [], {}
    with tempfile.TemporaryDirectory(prefix='kregs_') as d:
        for obj in sorted(glob.glob(os.path.join(objdir, '*.o'))):
            b = os.path.basename(obj)
            os.symlink(os.path.abspath(obj), os.path.join(d, b))
            subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', b], cwd=d, check=True,
                           capture_output=True)
            for co in glob.glob(os.path.join(d, b + '.*gfx950')):
                txt = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True,
                                     capture_output=True, text=True).stdout
                for blk in re.split(r'\n\s+- \.agpr_count:', txt)[1:]:
                    g = lambda k: re.search(r'\.' + k + r':\s+(\S+)', blk).group(1)  # noqa: E731
                    out.append((b, g('name'), {k: int(g(k)) for k in (
                        'vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size',
                        'vgpr_spill_count')}))
                if flt is not None:
                    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn',
                                          '--no-leading-addr', co], check=True, capture_output=True, text=True).stdout
                    for blk in re.split(r'\n(?=\S* ?<[^>]+>:\n)', dis)[1:]:
                        head, *lines = blk.splitlines()
                        asm[(b, re.search(r'<([^>]+)>', head).group(1))] = [
                            ln.split('//')[0].strip() for ln in lines
                            if ln.startswith(('\t', ' ')) and ln.strip() and ln.strip() != '...']   # '...': padding
    names = subprocess.run(['c++filt'] + [k[1] for k in out], capture_output=True, text=True).stdout.splitlines()
    res = []
    for (o, mangled, m), n in zip(out, names):
        n = n.replace('(anonymous namespace)::', '').replace('mrphy::', '').replace('void ', '').split('(')[0]
        if flt is not None and flt in n:
            m['text'] = asm[(o, mangled)]
            m['ops'] = collections.Counter(ln.split()[0] for ln in m['text'])
        res.append((o, n, m))
    return res


FIGURES = ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')


def diff(dir_a, dir_b, flt):
    r"""Compare the kernels of two builds whose name holds `flt`; returns how many differ in a register figure."""
    a, b = ({(o, n): m for o, n, m in kernels(d, flt) if flt in n} for d in (dir_a, dir_b))
    both = sorted(set(a) & set(b))
    same_text = [k for k in both if a[k]['text'] == b[k]['text']]
    same_ops = [k for k in both if a[k]['ops'] == b[k]['ops']]
    bad = 0
    for k in both:
        fa, fb = ([m[k][f] for f in FIGURES] for m in (a, b))
        if fa != fb:
            bad += 1
            print(f'FIGURES {k[1]} [{k[0]}]: vgpr/sgpr/lds/scratch {fa} -> {fb}')
        if a[k]['ops'] != b[k]['ops']:
            d = {op: (a[k]['ops'][op], b[k]['ops'][op]) for op in sorted(set(a[k]['ops']) | set(b[k]['ops']))
                 if a[k]['ops'][op] != b[k]['ops'][op]}
            print(f'OPCODES {k[1]} [{k[0]}]: ' + ', '.join(f'{op} {x} -> {y}' for op, (x, y) in d.items()))
    for tag, only in (('only in A', sorted(set(a) - set(b))), ('only in B', sorted(set(b) - set(a)))):
        for k in only:
            m = (a if k in a else b)[k]
            print(f'{tag}: {k[1]} [{k[0]}] vgpr/sgpr/lds/scratch {[m[f] for f in FIGURES]} '
                  f'{sum(m["ops"].values())} instructions')
    print(f'{len(both)} kernels compared: {len(same_text)} with identical text, {len(same_ops)} with an identical '
          f'opcode histogram, {bad} with other register / LDS / scratch figures; scratch > 0 in B: '
          f'{sum(1 for m in b.values() if m["private_segment_fixed_size"])}')
    return bad


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if '--diff' in sys.argv:
        i = sys.argv.index('--diff')
        dirs = sys.argv[i + 1:i + 3]
        sys.exit(diff(dirs[0], dirs[1], ([a for a in args if a not in dirs] or [''])[0]))
    objdir = os.path.join(ROOT, 'mrphy.py_amd', 'build')
    if '--objdir' in sys.argv:
        objdir = sys.argv[sys.argv.index('--objdir') + 1]
        args = [a for a in args if a != objdir]
    flt = args[0] if args else ''
    only_scratch = '--scratch' in sys.argv
    n = 0
    ks = kernels(objdir)
    for obj, name, m in ks:
        if (flt not in name and flt not in obj) or (only_scratch and not m['private_segment_fixed_size']):
            continue
        n += 1
        vg = m['vgpr_count']
        waves = min(8, 512 // (-(-vg // 8) * 8)) if vg else 8        # VGPRs are allocated in blocks of 8
        if '--brief' in sys.argv:
            print(f'{name[:70]:70s} v{vg:4d} lds{m["group_segment_fixed_size"]:6d} scr{m["private_segment_fixed_size"]:5d} spill{m["vgpr_spill_count"]:4d}')
            continue
        print(f'{name[:100]:100s} vgpr {vg:4d} sgpr {m["sgpr_count"]:4d} lds {m["group_segment_fixed_size"]:6d} '
              f'scratch {m["private_segment_fixed_size"]:5d} spilled {m["vgpr_spill_count"]:4d}  waves/SIMD<= {waves}  [{obj}]')
    print(f'{n} of {len(ks)} kernels listed')
    sys.exit(n if only_scratch else 0)
