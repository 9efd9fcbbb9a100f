#!/usr/bin/env python
"""Static instruction counts of conv3x3_tile_kernel instantiations (gfx950 ISA out of hipcc -S): total, in front of the first MFMA, behind the
last MFMA (K-loop tail + epilogue), registers and scratch, and the register moves between each loop body's last MFMA and its closing barrier.  VERDICT r4 item 1 asks for <= 500 / <= 700 in the <1,1,*> instantiations.

    python tools/isa_count.py [--only NPL,MT,FMT,NPW[,PARTLO]] [--filter "1,1,"] [--src path/to/esr_conv.hip] [--keep out.s | --asm out.s]

--only compiles a scratch copy of the translation unit whose conv_kernel_exists() admits just that operand form (seconds instead of minutes); without
it every instantiation of the shipping file is compiled (about three minutes)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'explorable-super-resolution_amd', 'csrc')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='NPL,MT,FMT,NPW[,PARTLO] of the one operand form to compile')
    ap.add_argument('--filter', default='', help='prefix of the template argument list to print, e.g. "1,1,"')
    ap.add_argument('--src', default=os.path.join(CSRC, 'esr_conv.hip'))
    ap.add_argument('--keep', default=None, help='write the assembly here')
    ap.add_argument('--asm', default=None, help='count this assembly file (a --keep of an earlier run) instead of compiling')
    a = ap.parse_args()
    if a.asm:
        return report(open(a.asm).read(), a.filter)
    src = open(a.src).read()
    tmp = tempfile.mkdtemp()
    if a.only:
        npl, mt, fmt, npw, partlo = ([int(v) for v in a.only.split(',')] + [0])[:5]
        # restrict conv_kernel_exists() — the one list of instantiations — to the requested form
        head = 'constexpr bool conv_kernel_exists(int npl, int mt, int epi, int nst, int fmt, int npw, bool partlo, int tmode) {\n'
        assert head in src
        src = src.replace(head, head + '    if (!(npl == %d && mt == %d && fmt == %d && npw == %d && partlo == %s && tmode == 0)) return false;\n' % (npl, mt, fmt, npw, 'true' if partlo else 'false'))
    cp = os.path.join(tmp, 'esr_conv_isa.hip')
    open(cp, 'w').write(src.replace('#include "esr_common.h"', '#include "%s/esr_common.h"' % CSRC))
    out = a.keep or os.path.join(tmp, 'conv.s')
    subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-function', '-Wno-unused-command-line-argument',
                           '--cuda-device-only', '-S', cp, '-o', out])
    report(open(out).read(), a.filter)


def report(txt, prefix):
    rows = []
    for m in re.finditer(r'^(_Z[\w]*conv3x3_tile_kernel[\w]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        name, body = m.group(1), m.group(2)
        dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        t = re.search(r'conv3x3_tile_kernel<(.*?)>', dem).group(1).replace(' ', '')
        if prefix and not t.startswith(prefix.replace(' ', '')):
            continue
        ins = [l.strip() for l in body.split('\n') if l.startswith('\t') and not l.strip().startswith(('.', ';')) and l.strip()]
        mf = [i for i, l in enumerate(ins) if l.startswith('v_mfma')]
        meta = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(name), txt, re.S).group(1)
        vg = re.search(r'\.amdhsa_next_free_vgpr (\d+)', meta).group(1)
        sg = re.search(r'\.amdhsa_next_free_sgpr (\d+)', meta).group(1)
        scr = re.search(r'; ScratchSize: (\d+)', txt[m.end():m.end() + 3000])
        lanes = sum(1 for l in ins if l.startswith(('v_writelane', 'v_readlane')))
        # per loop body: the vector register moves between its last MFMA and the barrier that closes it — accumulators the allocator copies on
        # the workgroup's serial chain.  Two walks from the MFMA to the barrier, both following s_branch: "A..B" = A moves with every forward
        # conditional branch taken (the shortest way: what a chunk executes that skips every uniform `if`), B with none taken (through the
        # first arm of each).  An MFMA whose walk reaches another MFMA first is not the last of its body.
        lines = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith(';')]
        label = {m2.group(1): i for i, l in enumerate(lines) for m2 in [re.match(r'(\.LBB\d+_\d+):', l)] if m2}

        def walk(i, take):
            j, n, seen = i + 1, 0, set()
            while j < len(lines) and j not in seen and not lines[j].startswith(('v_mfma', 's_barrier', 's_endpgm')):
                seen.add(j)
                n += lines[j].startswith(('v_mov_', 'v_accvgpr_'))
                tgt = re.match(r's_(c?)branch\w* (\.LBB\d+_\d+)', lines[j])
                if tgt and (not tgt.group(1) or (take and label[tgt.group(2)] > j)):
                    j = label[tgt.group(2)]
                else:
                    j += 1
            return n if j < len(lines) and lines[j].startswith('s_barrier') else None

        movs = []
        for i, l in enumerate(lines):
            if l.startswith('v_mfma') and walk(i, False) is not None:
                lo, hi = walk(i, True), walk(i, False)
                movs.append(str(hi) if lo == hi or lo is None else '%d..%d' % (lo, hi))
        rows.append((t, len(ins), mf[0], len(ins) - 1 - mf[-1], len(mf), vg, sg, scr.group(1) if scr else '?', lanes, ' '.join(movs)))
    print('# conv3x3_tile_kernel<NPL, MT, EPI, NST, FMT, NPW, PARTLO, TMODE>: instructions total / before the first MFMA / after the last MFMA')
    print('# mov>bar: v_mov_* / v_accvgpr_* between the last MFMA of each loop body and the barrier behind it, one entry per body in text order;')
    print('#          A..B = with every forward conditional branch taken .. with none taken')
    print('%-34s %6s %7s %6s %5s %5s %5s %8s %10s  %s' % ('instantiation', 'total', 'before', 'after', 'mfma', 'vgpr', 'sgpr', 'scratch', 'sgpr-spill', 'mov>bar'))
    for r in sorted(rows):
        print('%-34s %6d %7d %6d %5d %5s %5s %8s %10d  %s' % r)


if __name__ == '__main__':
    main()
