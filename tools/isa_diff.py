#!/usr/bin/env python3
"""Which kernels of two builds of the library are the same instruction stream?  Disassembles every code object of both (llvm-objdump), splits by
kernel symbol, strips addresses / encodings / the alignment fill behind the last instruction, and compares; a kernel of only one build is NEW or MISSING.  Usage: python tools/isa_diff.py OLD.so
NEW.so [substring ...]   (kernels whose demangled name contains every substring).  Used in round 5 to show that a feature compiled into the general per-env kernels left every default kernel alone."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa import device_disassembly


def kernels(lib):
    out = {}
    for _, txt in device_disassembly(lib).items():
        labels = {int(a, 16): n for a, n in re.findall(r'^([0-9a-f]{16}) <([^>]+)>:', txt, re.M)}
        for part in re.split(r'\n(?=[0-9a-f]{16} <)', txt):
            m = re.match(r'[0-9a-f]{16} <([^>]+)>:', part)
            if not m:
                continue
            body, pc = [], {}
            for ln in part.splitlines()[1:]:
                addr = re.search(r'//\s*([0-9A-Fa-f]+):', ln)
                ln = re.sub(r'//.*$', '', ln).strip()
                ln = re.sub(r'<[^>]*>', '', ln)             # branch targets carry symbol+offset
                ln = pc_relative(ln, addr, pc, labels)
                if ln and ln != '...':                      # '...': zero padding up to whatever the linker placed next
                    body.append(ln)
            # s_nop 0 behind the last instruction: the assembler's fill up to the next kernel of the same section (256-byte starts), which
            # the unit's last kernel does not have.  Like the linker's padding it is never executed and says where the kernel sits, not
            # what it is: a kernel that only moved to another unit, or whose neighbour left, would DIFFER.
            while body and body[-1] == 's_nop 0':
                body.pop()
            out[m.group(1)] = body
    return out


def pc_relative(ln, addr, pc, labels):
    """s_getpc_b64 s[a:a+1]; s_add_u32 sa, sa, lo; s_addc_u32 sa+1, sa+1, hi: the address of a function (a call to a non-inlined device
    function).  lo / hi depend on where the linker put the kernel and its callee, so a kernel that only moved would DIFFER: they are replaced
    by the callee's name.  An address that is no function's start keeps its literals."""
    g = re.match(r's_getpc_b64 s\[(\d+):\d+\]$', ln)
    if g and addr:
        pc[int(g.group(1))] = int(addr.group(1), 16) + 4      # s_getpc_b64 returns the address of the next instruction
        return ln
    a = re.match(r'(s_add_u32|s_addc_u32) s(\d+), s\d+, (\S+)$', ln)
    if not a:
        return ln
    op, reg, lit = a.group(1), int(a.group(2)), a.group(3)
    if op == 's_add_u32' and reg in pc:
        try:
            target = (pc.pop(reg) + int(lit, 0)) & 0xffffffff
        except ValueError:
            return ln
        name = next((n for base, n in labels.items() if base & 0xffffffff == target), None)
        if name:
            pc[('hi', reg + 1)] = name
            return '%s s%d, s%d, lo(%s)' % (op, reg, reg, name)
    elif op == 's_addc_u32' and ('hi', reg) in pc:
        return '%s s%d, s%d, hi(%s)' % (op, reg, reg, pc.pop(('hi', reg)))
    return ln


def demangle(names):
    try:
        return dict(zip(names, subprocess.run(['c++filt'] + names, check=True, capture_output=True, text=True).stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def main():
    old, new, want = kernels(sys.argv[1]), kernels(sys.argv[2]), sys.argv[3:]
    dem = demangle(sorted(set(old) | set(new)))
    same = diff = added = lost = 0
    for k in sorted(set(old) | set(new)):
        name = re.sub(r'\(dpenv::.*$', '', re.sub(r'^void ', '', dem[k]))
        if not all(w in name for w in want):
            continue
        if k not in new:
            lost += 1
            print('MISSING   %s (%d instructions)' % (name[:110], len(old[k])))
        elif k not in old:
            added += 1
            print('NEW       %s (%d instructions)' % (name[:110], len(new[k])))
        elif old[k] == new[k]:
            same += 1
            print('identical %s (%d instructions)' % (name[:110], len(new[k])))
        else:
            diff += 1
            print('DIFFERS   %s (%d -> %d instructions)' % (name[:110], len(old[k]), len(new[k])))
    print('%d identical, %d differ, %d new, %d missing' % (same, diff, added, lost))


if __name__ == '__main__':
    main()
