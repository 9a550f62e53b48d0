#!/usr/bin/env python3
"""Per-basic-block instruction mix of ONE kernel of a gfx950 assembly file (hipcc -S / make asm output).

    python tools/isa_blocks.py FILE.s SYMBOL_SUBSTRING [--summary]

Prints one line per basic block (label, instruction count, VALU split by encoding, SALU, LDS, VMEM, branches) and marks the
blocks that branch back to themselves (the plant's sub-step loop: unrolled x10, two trips per env step).  --summary prints the
kernel's totals and the loop block's alone.  The counts are static; PMC (SQ_INSTS_*) gives the dynamic ones of a run.
`block_counts()` is what tests/test_step_lean_isa.py reads.
"""
import collections
import re
import sys

sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.abspath(__file__)))
from isa_count import classify  # noqa: E402


def kernel_lines(path, sym):
    """the instruction and label lines of the first kernel whose mangled name contains sym"""
    out, on = [], False
    for line in open(path):
        if not on:
            m = re.match(r'^(_Z\w+):', line)
            if m and sym in m.group(1):
                on = True
            continue
        t = line.split(';')[0].strip()
        if t.startswith('.Lfunc_end') or t.startswith('.end_amdhsa_kernel'):
            break
        if not t or (t.startswith('.') and not t.endswith(':')):
            continue
        out.append(t)
    if not on:
        raise KeyError('no kernel matching %r in %s' % (sym, path))
    return out


def is_vop3(t):
    """an 8-byte VALU encoding: _e64 forms, and the VOP3-only opcodes the assembler prints without a suffix"""
    op = t.split()[0]
    if op.endswith('_e64') or op.endswith('_e64_dpp'):
        return True
    if op.endswith('_e32') or op.endswith('_dpp') or op.endswith('_sdwa'):
        return False
    # fma / mad / 3-operand forms, 64-bit shifts, v_cmp writing an SGPR pair, v_cndmask with an SGPR mask
    return bool(re.match(r'v_(fma|mad|lshl_add|lshl_or|add3|and_or|or3|xad|med3|min3|max3|bfe|bfi|alignbit|perm|cvt_pk|ldexp|div_|'
                         r'cndmask_b32 .*s\[|cmp|mul_lo|mul_hi|readlane|writelane|lshlrev_b64|lshrrev_b64|ashrrev_i64|add_co|sub_co|addc|subb)', t))


def block_counts(path, sym):
    """[(label, Counter, loops_to_self)] in program order; the entry block is labelled '<entry>'"""
    blocks, label, c, jumps = [], '<entry>', collections.Counter(), []
    for t in kernel_lines(path, sym):
        if t.endswith(':'):
            if sum(c.values()):
                blocks.append((label, c, label in jumps))
            label, c, jumps = t[:-1], collections.Counter(), []
            continue
        op = t.split()[0]
        k = classify(op)
        if k == 'VALU':
            k = 'VOP3' if is_vop3(t) else 'VOP2'
        c[k] += 1
        if k == 'branch' and len(t.split()) > 1:
            jumps.append(t.split()[1])
        # 64-bit per-lane address arithmetic
        if re.match(r'v_(lshl_add_u64|mad_u64_u32|mad_i64_i32|cmp_\w+_[iu]64|lshlrev_b64|add_co_u32|addc_co_u32|ashrrev_i32)', op):
            c['addr64'] += 1
    if sum(c.values()):
        blocks.append((label, c, label in jumps))
    return blocks


def main():
    path, sym = sys.argv[1], sys.argv[2]
    blocks = block_counts(path, sym)
    keys = ['VOP2', 'VOP3', 'SALU', 'SMEM', 'LDS', 'VMEM', 'wait', 'branch', 'addr64']
    tot, loop = collections.Counter(), collections.Counter()
    for lab, c, self_loop in blocks:
        tot.update(c)
        if self_loop:
            loop.update(c)
        if '--summary' not in sys.argv:
            print('%-14s %5d %s%s' % (lab, sum(v for k, v in c.items() if k != 'addr64'), '  '.join('%s %d' % (k, c[k]) for k in keys if c[k]),
                                      '   <- loop' if self_loop else ''))
    fmt = lambda c: '%5d instr  %s' % (sum(v for k, v in c.items() if k != 'addr64'), '  '.join('%s %d' % (k, c[k]) for k in keys))
    print('total      ', fmt(tot))
    print('loop block ', fmt(loop))


if __name__ == '__main__':
    main()
