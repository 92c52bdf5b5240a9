"""Wait structure of the MFMA loops of chosen kernels in a gfx950 assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -Icsrc \
          --offload-device-only -S csrc/igemm.hip -o igemm.s
    python bench/isa_wait_seq.py igemm.s 'bwd_pair_kernel<64, 64, 64, 64>' ...

For every depth-1 loop that holds MFMAs (found as bench/isa_loop_count.py finds them) it prints
the loop's blocks in listing order as one line of tokens:

    vmcnt(n)   an ``s_waitcnt`` with a vmcnt field (the lgkmcnt / expcnt fields are not shown)
    ldN        a run of N vector-memory loads
    dswN       a run of N LDS writes
    mfmaN      a run of N MFMAs
    BAR        s_barrier

Everything else (address VALU, SALU, LDS reads, lgkmcnt-only waits, branches) is skipped and does
not break a run.  A register-staged loop that keeps its loads in flight shows vmcnt waits only
directly in front of the ``dsw`` run that stores the set they count down to; a wait between the
loop header and the first MFMAs means the loads issued late in the previous trip were drained.
``--summary`` adds, per loop, the waits that are not followed by an LDS write before the next
MFMA, load or barrier ("uncounted" waits), and per kernel the VGPR / AGPR / LDS / scratch /
spill figures of its ``.amdhsa`` and metadata lines.
"""
import re
import sys

from isa_loop_count import INSN, functions, mangled, mfma_loops

VMCNT = re.compile(r'vmcnt\((\d+)\)')


def tokens(lines):
    """[(kind, n)]: kind in 'vmcnt' (n = the count), 'ld', 'dsw', 'mfma' (n = run length), 'BAR'"""
    out = []

    def run(kind):
        if out and out[-1][0] == kind:
            out[-1] = (kind, out[-1][1] + 1)
        else:
            out.append((kind, 1))

    for ln in lines:
        m = INSN.match(ln)
        if not m:
            continue
        op = m.group(1)
        if op.startswith('v_mfma'):
            run('mfma')
        elif op.startswith(('buffer_load', 'global_load', 'flat_load', 'scratch_load')):
            run('ld')
        elif op.startswith('ds_write'):
            run('dsw')
        elif op == 's_barrier':
            out.append(('BAR', 0))
        elif op == 's_waitcnt':
            v = VMCNT.search(ln)
            if v:
                out.append(('vmcnt', int(v.group(1))))
    return out


def show(toks):
    """one line; a counted store -- vmcnt(a) dsw1 vmcnt(a-1) dsw1 ... vmcnt(b) dsw1 -- is folded
    to ``vmcnt(a..b)+dswN``"""
    out, i = [], 0
    while i < len(toks):
        k, n = toks[i]
        j = i
        while (j + 1 < len(toks) and toks[j][0] == 'vmcnt' and toks[j + 1] == ('dsw', 1) and
               (j == i or toks[j][1] == toks[j - 2][1] - 1)):
            j += 2
        if j - i >= 4:
            out.append('vmcnt(%d..%d)+dsw%d' % (n, toks[j - 2][1], (j - i) // 2))
            i = j
            continue
        out.append('BAR' if k == 'BAR' else 'vmcnt(%d)' % n if k == 'vmcnt' else '%s%d' % (k, n))
        i += 1
    return ' '.join(out)


def uncounted(toks):
    """the vmcnt waits that no LDS write follows before the next MFMA run, load run or barrier
    (circularly: the loop's last tokens are followed by its first)"""
    bad = []
    n = len(toks)
    for i, (k, v) in enumerate(toks):
        if k != 'vmcnt':
            continue
        for j in range(1, n):
            kk = toks[(i + j) % n][0]
            if kk == 'vmcnt':
                continue
            if kk != 'dsw':
                bad.append(v)
            break
    return bad


META = re.compile(r'^\s+\.(amdhsa_next_free_vgpr|amdhsa_accum_offset|amdhsa_group_segment_fixed_size'
                  r'|amdhsa_private_segment_fixed_size)\s+(\d+)')
NOTE = re.compile(r'^\s+\.(vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count'
                  r'|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)')


def metadata(lines, sym):
    """the kernel's figures from its .amdhsa_kernel block and its amdhsa.kernels entry"""
    out = {}
    inside = False
    for ln in lines:
        if ln.startswith('.amdhsa_kernel ' + sym):
            inside = True
        elif inside and ln.startswith('.end_amdhsa_kernel'):
            inside = False
        elif inside:
            m = META.match(ln)
            if m:
                out[m.group(1).replace('amdhsa_', '')] = int(m.group(2))
    # metadata entries list .name after some of the fields: collect per entry, keyed by .name
    entry, name = {}, None
    for ln in lines:
        s = ln.strip()
        if s.startswith('- .'):
            if name == sym:
                out.update(entry)
            entry, name = {}, None
            s = s[2:]
            ln = '    ' + s
        m = NOTE.match(ln)
        if m:
            entry[m.group(1)] = int(m.group(2))
        elif s.startswith('.name:'):
            name = s.split(':', 1)[1].strip()
    if name == sym:
        out.update(entry)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != '--summary']
    summary = '--summary' in sys.argv[1:]
    path, wanted = args[0], args[1:]
    lines = open(path).read().splitlines()
    spans = functions(lines)
    for want in wanted:
        for k in [k for k in spans if mangled(want) in k]:
            lo, hi = spans[k]
            print('## %s' % want)
            for head, body in mfma_loops(lines, lo, hi).items():
                toks = tokens(body)
                print('  loop %-9s %s' % (head, show(toks)))
                if summary:
                    bad = uncounted(toks)
                    print('       uncounted vmcnt waits: %s' %
                          (' '.join('vmcnt(%d)' % v for v in bad) if bad else 'none'))
            if summary:
                md = metadata(lines, k)
                print('       ' + '  '.join('%s %d' % kv for kv in sorted(md.items())))


if __name__ == '__main__':
    main()
