"""Instruction mix of the MFMA loops of chosen kernels in a gfx950 assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -Icsrc \
          --offload-device-only -S csrc/igemm.hip -o igemm.s
    python bench/isa_loop_count.py igemm.s 'bwd_pair_kernel<64, 64, 64, 64>' ...

A loop is the set of blocks the compiler annotates with one depth-1 loop header; those that hold
MFMAs are reported (a kernel made of several bodies, such as a dgrad + wgrad pair, has one per
body).  Per loop: MFMA, VALU (v_* other than MFMA), vector-memory loads, LDS ops, SALU, scratch
accesses and ``s_waitcnt vmcnt(0)``.  Static counts over the loop's blocks -- both arms of a
branch inside it are counted (the KCursor fast and slow paths, a PF = 2 loop's two stages).
"""
import re
import sys

FUNC = re.compile(r'^(_Z\w+):')
INSN = re.compile(r'^\s+([a-z]\w+)')


def mangled(want):
    """Itanium fragment of ``name<int | bool, ...>``: matched against the symbols themselves
    (demanglers stop at the bf16 pointer arguments)"""
    name, _, args = want.partition('<')
    frag = '%d%s' % (len(name), name)
    if args:
        frag += 'I'
        for a in args.rstrip('>').split(','):
            a = a.strip()
            frag += {'true': 'Lb1E', 'false': 'Lb0E'}.get(a) or 'Li%sE' % a
        frag += 'E'
    return frag


def functions(lines):
    """{mangled: (first, last)} line spans of the functions in the listing"""
    spans, cur, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = FUNC.match(ln)
        if m:
            cur, start = m.group(1), i
        elif cur and ln.startswith('.Lfunc_end'):
            spans[cur] = (start, i)
            cur = None
    return spans


def mix(lines):
    c = dict(mfma=0, valu=0, vmem_ld=0, vmem_st=0, lds=0, salu=0, scratch=0, vmcnt0=0, barrier=0)
    for ln in lines:
        m = INSN.match(ln)
        if not m:
            continue
        op = m.group(1)
        if op.startswith('v_mfma'):
            c['mfma'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
        elif op.startswith('scratch_'):
            c['scratch'] += 1
        elif op.startswith(('buffer_load', 'global_load', 'flat_load')):
            c['vmem_ld'] += 1
        elif op.startswith(('buffer_', 'global_', 'flat_')):
            c['vmem_st'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
        elif op == 's_barrier':
            c['barrier'] += 1
        elif op == 's_waitcnt':
            if re.search(r'vmcnt\(0\)', ln):
                c['vmcnt0'] += 1
        elif op.startswith('s_'):
            c['salu'] += 1
    return c


BLOCK = re.compile(r'^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)')
HEADER = re.compile(r'Loop Header: Depth=1')
MEMBER = re.compile(r'(?:in Loop: Header=|Parent Loop )(BB\d+_\d+) Depth=1')


def mfma_loops(lines, lo, hi):
    """{header label: [lines]} of the depth-1 loops that hold MFMAs, from the compiler's own
    block annotations (a loop's blocks need not be contiguous: a stage's LDS stores often sit
    behind the back edge)"""
    loops, cur = {}, None
    i = lo
    while i < hi:
        ln = lines[i]
        m = BLOCK.match(ln)
        if m:
            # the annotation may continue on the following comment-only lines
            note, j = ln, i + 1
            while j < hi and lines[j].startswith('   ') and lines[j].lstrip().startswith(';'):
                note += lines[j]
                j += 1
            mm = MEMBER.search(note)
            if HEADER.search(note) and m.group(1):
                cur = m.group(1).lstrip('.L')
            elif mm:
                cur = mm.group(1)
            else:
                cur = None
        if cur:
            loops.setdefault(cur, []).append(ln)
        i += 1
    return {k: v for k, v in loops.items() if any('v_mfma' in ln for ln in v)}


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    lines = open(path).read().splitlines()
    spans = functions(lines)
    for want in wanted:
        for k in [k for k in spans if mangled(want) in k]:
            lo, hi = spans[k]
            print('## %s' % want)
            for head, body in mfma_loops(lines, lo, hi).items():
                c = mix(body)
                print('  loop %-10s %4d lines  mfma %3d  valu %4d (%.2f / mfma)  vmem_ld %2d  '
                      'vmem_st %2d  lds %3d  salu %3d  barrier %d  scratch %d  vmcnt(0) %d' %
                      (head, len(body), c['mfma'], c['valu'],
                       c['valu'] / max(c['mfma'], 1), c['vmem_ld'], c['vmem_st'], c['lds'],
                       c['salu'], c['barrier'], c['scratch'], c['vmcnt0']))


if __name__ == '__main__':
    main()
