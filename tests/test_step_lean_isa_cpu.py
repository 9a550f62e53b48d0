"""The headline's lean step instantiation in the cross-compiled ISA (no GPU needed): its stream addresses are buffer offsets, not
64-bit per-lane addresses, and its sub-step loop block is no wider in 8-byte VALU encodings than it is today."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import isa_blocks  # noqa: E402

LEAN = '_ZN5dpenv11step_kernelILi4ELb1ELi0ELb0ELb1EEEvNS_8StepArgsE'       # step_kernel<MODE_FINAL_CONT, true, VES_ARGS, false, LEAN>
LOOP_VOP3_MAX = 154            # the unrolled x10 sub-step block: 14 VOP3 per sub-step (|x| modifiers, invariant addends) + the trip's own


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    csrc = os.path.join(ROOT, 'ml4ca_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1).split()
    out = str(tmp_path_factory.mktemp('isa') / 'k.s')
    subprocess.run([hipcc, '--offload-arch=gfx950'] + flags + ['-DDPENV_DEV_FAST', '--cuda-device-only', '-S', '-o', out,
                                                                os.path.join(csrc, 'dpenv_kernels.hip')], check=True, capture_output=True)
    return out


def test_lean_step_has_no_64bit_lane_addressing(asm):
    blocks = isa_blocks.block_counts(asm, LEAN)
    assert sum(c['addr64'] for _, c, _ in blocks) == 0
    ops = [t.split()[0] for t in isa_blocks.kernel_lines(asm, LEAN) if not t.endswith(':')]
    assert not [o for o in ops if o.startswith('global_') or o.startswith('flat_')], 'every stream of the lean step is a buffer access'
    assert sum(o.startswith('buffer_load') for o in ops) == 7 + 4 + 3 and sum(o.startswith('buffer_store') for o in ops) == 4 + 1 + 9 + 1


def test_lean_step_loop_block_vop3(asm):
    loops = [(lab, c) for lab, c, self_loop in isa_blocks.block_counts(asm, LEAN) if self_loop]
    assert loops, 'no sub-step loop block found'
    big = max(loops, key=lambda lc: sum(lc[1].values()))[1]
    assert big['VOP3'] <= LOOP_VOP3_MAX
