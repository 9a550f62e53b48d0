"""The headline's fixed step instantiation in the cross-compiled ISA (no GPU needed), set against the lean step's in the same
assembly: buffer accesses only, the leading arguments preloaded, every scalar load ahead of the first wait for a vector load, and
fewer scalar and vector instructions than the lean kernel it stands in for.  All counts are relative to the lean symbol."""
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
FIXED = '_ZN5dpenv17step_fixed_kernelILi4ELb1ELb1ELb0ELb0EEE'              # step_fixed_kernel<MODE_FINAL_CONT, ext, degrees, no end conditions, no setpoint>
SUBSTEPS_PER_TRIP = 10         # env_plant's `#pragma unroll 10`
LEAN_VOP3_PER_SUBSTEP = 14


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    csrc = os.path.join(ROOT, 'ml4ca_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1).split()
    unit = re.search(r'^KERNELS_FLAGS := (.*)$', mk, re.M).group(1).split()          # what dpenv_kernels.o alone is built with
    assert re.search(r'^\$\(OBJDIR\)/dpenv_kernels\.o: UNIT_FLAGS := \$\(KERNELS_FLAGS\)$', mk, re.M)
    assert any(f.startswith('-amdgpu-kernarg-preload-count=') for f in unit)
    out = str(tmp_path_factory.mktemp('isa') / 'k.s')
    subprocess.run([hipcc, '--offload-arch=gfx950'] + flags + unit + ['-DDPENV_DEV_FAST', '--cuda-device-only', '-S', '-o', out,
                                                                       os.path.join(csrc, 'dpenv_kernels.hip')], check=True, capture_output=True)
    return out


def _ops(asm, sym):
    return [t.split()[0] for t in isa_blocks.kernel_lines(asm, sym) if not t.endswith(':')]


def _totals(asm, sym):
    tot = {}
    for _, c, _ in isa_blocks.block_counts(asm, sym):
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    return tot


def _loop_block(asm, sym):
    loops = [c for _, c, self_loop in isa_blocks.block_counts(asm, sym) if self_loop]
    assert loops, 'no sub-step loop block found'
    return max(loops, key=lambda c: sum(c.values()))


def test_fixed_step_is_buffer_io_only(asm):
    assert _totals(asm, FIXED).get('addr64', 0) == 0
    ops = _ops(asm, FIXED)
    assert not [o for o in ops if o.startswith('global_') or o.startswith('flat_')], 'every stream of the fixed step is a buffer access'
    assert sum(o.startswith('buffer_load') for o in ops) == 7 + 4               # the action row, the four state streams
    assert sum(o.startswith('buffer_store') for o in ops) == 3 + 1 + 9 + 1      # state, done, the observation row, the reward
    assert not [o for o in ops if o.startswith('v_pk_') and o.endswith('_f32')], 'no packed fp32'


def test_fixed_step_arguments_are_preloaded_and_fetched_early(asm):
    txt = open(asm).read()
    sym = re.search(r'^(%s\w*):' % re.escape(FIXED), txt, re.M).group(1)
    desc = txt[txt.index('.amdhsa_kernel ' + sym):]
    desc = desc[:desc.index('.end_amdhsa_kernel')]
    assert int(re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)', desc).group(1)) > 0
    lines = isa_blocks.kernel_lines(asm, FIXED)
    first_wait = next(k for k, t in enumerate(lines) if t.startswith('s_waitcnt') and 'vmcnt' in t)
    assert any(t.startswith('s_load') for t in lines[:first_wait])
    assert not [t for t in lines[first_wait:] if t.startswith('s_load')], 'a scalar load behind the first wait for a vector load'


def test_fixed_step_issues_fewer_instructions_than_the_lean_step(asm):
    lean, fixed = _totals(asm, LEAN), _totals(asm, FIXED)
    print('lean  ', sorted(lean.items()))
    print('fixed ', sorted(fixed.items()))
    assert fixed['SALU'] < lean['SALU']
    assert fixed['VOP2'] + fixed['VOP3'] < lean['VOP2'] + lean['VOP3']


def test_fixed_step_sub_step_block_vop3(asm):
    # (the block runs on to the next label, so it holds the few instructions between the loop's branch and it as well: whole
    # 8-byte encodings per sub-step are what is compared)
    lean, fixed = _loop_block(asm, LEAN), _loop_block(asm, FIXED)
    assert lean['VOP3'] // SUBSTEPS_PER_TRIP == LEAN_VOP3_PER_SUBSTEP
    assert fixed['VOP3'] // SUBSTEPS_PER_TRIP <= lean['VOP3'] // SUBSTEPS_PER_TRIP
