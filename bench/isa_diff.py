"""Per-kernel comparison of two gfx950 assembly listings of the same source file, for changes
that must not change the generated code.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -Icsrc \
          --offload-device-only -S csrc/igemm.hip -o new/igemm.s      (and the old tree's)
    python bench/isa_diff.py old/igemm.s new/igemm.s [--hunks] [OLDNAME=NEWNAME ...]

Per kernel symbol: the resource metadata (registers, spills, scratch, LDS) must be equal, and the
instruction sequence with register numbers and block labels masked must be equal.  Prints one
line per kernel that differs (with --hunks, the differing instructions too) and per symbol that
only one listing has, and exits 1 if there is any.  A renamed or merged kernel is compared under
OLDNAME=NEWNAME, which renames the old listing's symbols (names of equal length, as the mangled
symbol carries it): ``pg_coef_kernel=bn_coef_kernel``.
"""
import difflib
import re
import sys

from isa_loop_count import functions

META = ('.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count',
        '.private_segment_fixed_size', '.group_segment_fixed_size')
MASK = re.compile(r'\b[vsa]\d+\b|\b[vsa]\[\d+:\d+\]|\.LBB\d+_\d+')
INSN = re.compile(r'^\s+[a-z]\w+')


def metadata(lines):
    """{symbol: {key: value}} from the amdhsa.kernels entries at the end of the listing"""
    out, cur = {}, None
    for ln in lines[lines.index('amdhsa.kernels:') + 1:]:
        if not ln.startswith('  '):
            break
        if ln.startswith('  - '):
            cur = {}
        m = re.match(r'^\s+(?:- )?(\.\w+):\s+(\S+)$', ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == '.name':
                out[m.group(2)] = cur
    return out


def insns(lines, span):
    """masked instructions of one function: no comments, directives or labels"""
    return [MASK.sub('#', ln.split(';')[0].strip()) for ln in lines[span[0]:span[1]]
            if INSN.match(ln)]


def main():
    args = [a for a in sys.argv[1:] if a != '--hunks' and '=' not in a]
    hunks = '--hunks' in sys.argv
    old, new = (open(p).read() for p in args)
    for a in sys.argv[1:]:
        if '=' in a:
            old = old.replace(*a.split('='))
    old, new = old.splitlines(), new.splitlines()
    fo, fn = functions(old), functions(new)
    mo, mn = metadata(old), metadata(new)
    for k in sorted(set(fo) ^ set(fn)):
        print('only in %s: %s' % (args[0] if k in fo else args[1], k))
    bad = len(set(fo) ^ set(fn))
    for k in sorted(set(fo) & set(fn)):
        x, y = mo.get(k, {}), mn.get(k, {})
        dm = [(f, x.get(f), y.get(f)) for f in META if x.get(f) != y.get(f)]
        a, b = insns(old, fo[k]), insns(new, fn[k])
        if not dm and a == b:
            continue
        bad += 1
        same_ops = [x.split()[0] for x in a] == [x.split()[0] for x in b]
        print('DIFFERS %s: metadata %s; %d -> %d instructions%s' %
              (k, dm or 'equal', len(a), len(b),
               ' (same mnemonics, operands differ)' if same_ops else ''))
        if hunks:
            print('\n'.join(difflib.unified_diff(a, b, 'old', 'new', lineterm='', n=2)))
    print('%d kernels compared, %d differ or are unmatched' % (len(set(fo) & set(fn)), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
