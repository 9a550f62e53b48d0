"""CPU-side checks of the product boundary: libdpenv.so loads, exports every symbol that
include/dpenv.h declares, its structs have the layout the binding assumes, argument validation
works, and - with no GPU - it fails loudly instead of falling back to anything."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    txt = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(dpenv_[a-z_0-9]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    from ml4ca_amd import _lib
    lib = _lib.load()
    declared = _header_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), 'libdpenv.so does not export %s' % name
    # and nothing else: the internal launchers between the translation units stay out of the dynamic symbol table
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3 and f[1] == 'T' and f[2].startswith('dpenv_'))
    assert exported == declared, 'exported but not declared: %s; declared but not exported: %s' % (
        sorted(set(exported) - set(declared)), sorted(set(declared) - set(exported)))
    assert sorted(_lib.SYMBOLS) == declared, 'binding table and header drifted apart'
    assert lib.dpenv_abi_version() == _lib.ABI_VERSION


def test_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dpenv_config), sizeof(dpenv_step_io),'
                   ' offsetof(dpenv_config, seed), offsetof(dpenv_config, reset_fraction),'
                   ' offsetof(dpenv_config, hold_plant), offsetof(dpenv_step_io, final_obs),'
                   ' offsetof(dpenv_config, reset_acts), sizeof(dpenv_policy_desc), offsetof(dpenv_policy_desc, precision),'
                   ' offsetof(dpenv_policy_desc, device_pointers), sizeof(dpenv_policy_rollout_io), offsetof(dpenv_policy_rollout_io, sample),'
                   ' sizeof(dpenv_mlp), offsetof(dpenv_policy_rollout_io, reset_at_end));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.Config), C.sizeof(_lib.StepIO), _lib.Config.seed.offset, _lib.Config.reset_fraction.offset,
            _lib.Config.hold_plant.offset, _lib.StepIO.final_obs.offset, _lib.Config.reset_acts.offset, C.sizeof(_lib.PolicyDesc),
            _lib.PolicyDesc.precision.offset, _lib.PolicyDesc.device_pointers.offset, C.sizeof(_lib.PolicyRolloutIO),
            _lib.PolicyRolloutIO.sample.offset, C.sizeof(_lib.Mlp), _lib.PolicyRolloutIO.reset_at_end.offset]
    assert got == want


def test_defaults_match_reference_training_configuration():
    """train.py:47-54 (final, ext, cont_ang), customEnv.py:79-83 (20 x 0.01 s, T = 400)."""
    from ml4ca_amd import _lib
    lib = _lib.load()
    c = _lib.default_config()
    assert (c.variant, c.extended_state, c.cont_ang, c.n_substeps, c.max_ep_len) == (_lib.FINAL, 1, 1, 20, 400)
    assert abs(c.substep_dt - 0.01) < 1e-9 and abs(c.reset_fraction - 0.8) < 1e-7
    assert lib.dpenv_act_dim(C.byref(c)) == 7 and lib.dpenv_obs_dim(C.byref(c)) == 9
    for variant, cont, ad in [(_lib.FULL, 0, 6), (_lib.SIMPLE, 0, 3), (_lib.LIMITED, 0, 5), (_lib.FINAL, 0, 5)]:
        c.variant, c.cont_ang = variant, cont
        assert lib.dpenv_act_dim(C.byref(c)) == ad
    v = _lib.default_vessel()
    # thruster constants from the reference: qp_allocator.py:51-55,69-70 in env order bow, port, star
    assert np.allclose(v[12:18], [0.0009, 0.00205, 0.00205] * 2)
    assert np.allclose(v[18:24], [1.08, -1.12, -1.12, 0.0, -0.15, 0.15])
    # and they are the constants the oracle integrates with
    from oracle import oracle as O
    assert np.array_equal(v, O.Oracle(O.make_config(), np.float32).vessel)


def test_create_validates_and_fails_loudly_without_gpu():
    import torch
    from ml4ca_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    c = _lib.default_config()
    c.n_envs = 0
    assert lib.dpenv_create(C.byref(c), None, 1, C.byref(h)) == _lib.EINVAL
    assert b'n_envs' in lib.dpenv_last_error(None)
    c.n_envs = 16
    c.variant, c.cont_ang = _lib.SIMPLE, 0
    assert lib.dpenv_create(C.byref(c), None, 1, C.byref(h)) == _lib.EINVAL      # simple + extended
    assert b'customEnv.py:319' in lib.dpenv_last_error(None)
    c = _lib.default_config()
    c.n_envs = 16
    c.struct_size = 8
    assert lib.dpenv_create(C.byref(c), None, 1, C.byref(h)) == _lib.EINVAL
    if not torch.cuda.is_available():
        c = _lib.default_config()
        c.n_envs = 16
        assert lib.dpenv_create(C.byref(c), None, 1, C.byref(h)) == _lib.ENODEV
        assert b'no CPU fallback' in lib.dpenv_last_error(None)
        import ml4ca_amd
        with pytest.raises(RuntimeError):
            ml4ca_amd.BatchedRevoltEnv(4)
        with pytest.raises(RuntimeError):
            ml4ca_amd.RevoltFinal(None, extended_state=True, cont_ang=True)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: no file of the product package may reference it."""
    pkg = os.path.join(ROOT, 'ml4ca_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp', 'Makefile')):
                txt = open(os.path.join(root, f), errors='ignore').read()
                assert 'dpenv_oracle' not in txt and 'from oracle' not in txt and 'import oracle' not in txt, f
    code = 'import sys; import ml4ca_amd; assert not any(m == "oracle" or m.startswith("oracle.") for m in sys.modules)'
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_variant_constants_match_reference_fixtures():
    import ml4ca_amd
    G = os.path.join(ROOT, 'tests', 'golden')
    for mode, (variant, cont) in {'full': ('full', False), 'simple': ('simple', False), 'limited': ('limited', False),
                                  'final_wrap': ('final', False), 'final_cont': ('final', True)}.items():
        d = np.load(os.path.join(G, 'env_%s.npz' % mode))
        k = ml4ca_amd.variant_constants(variant, cont)
        assert np.allclose(k['real_ss_bounds'], d['real_ss_bounds'], rtol=0, atol=1e-15)
        assert np.allclose(k['real_action_bounds'], d['real_action_bounds'], rtol=0, atol=1e-15)
        assert np.allclose([k['default_actions'][i] for i in range(6)], d['default_actions'], rtol=0, atol=1e-15)
        assert list(k['valid_action_indices']) == list(d['valid_action_indices'])
        assert k['num_actions'] == int(d['meta'][3])


def test_no_packed_fp32_in_any_translation_unit():
    """MI355X hardware interaction (the record is profiles/r02_ws_hazard/):
    ``v_pk_fma_f32 ... op_sel:[0,1,0]`` / ``[0,0,1]`` - a packed fp32 FMA whose LOW result takes the HIGH register of src1 or
    src2, which is what the SLP vectoriser makes of ``acc += c * pair.hi`` - now and then returns src2.lo in lanes 48-63 while
    another wave on the same SIMD has VALU work in the shadow of its MFMAs.  It is between two waves, so no wait-state rule of
    the compiler covers it.  The library is therefore built without packed fp32 arithmetic at all (-fno-slp-vectorize): this
    compiles ALL translation units with the Makefile's flags and checks the ISA for (a) that exact operand form and
    (b) any packed fp32 arithmetic."""
    import re
    import shutil
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    csrc = os.path.join(ROOT, 'ml4ca_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1).split()
    assert '-fno-slp-vectorize' in flags
    units = re.search(r'^SRC := (.*)$', mk, re.M).group(1).split()
    assert sorted(units) == ['dpenv_api.hip', 'dpenv_api_free.hip', 'dpenv_control.hip', 'dpenv_kernels.hip', 'dpenv_label.hip', 'dpenv_policy.hip',
                             'dpenv_policy_ws.hip', 'dpenv_policy_x.hip', 'dpenv_policy_xws1.hip', 'dpenv_policy_xws2.hip']

    def isa(unit):
        # the policy units instantiate ~40 kernels each from ONE template (env variant x obs width x layer width x activation) and
        # take minutes apiece; the scan needs the code, not every copy of it: -DDPENV_DEV_FAST instantiates the shipped configuration
        # (final / continuous angles / extended state, 80-wide leaky-relu layers, both workgroup geometries) - the kernels the bench
        # runs.  The whole library, every instantiation, is scanned for packed fp32 by `make` itself (tools/check_isa.py on the
        # linked libdpenv.so: a hard build step).
        extra = ['-DDPENV_DEV_FAST'] if unit.startswith('dpenv_policy') else []
        return subprocess.run([hipcc, '--offload-arch=gfx950'] + flags + extra + ['--cuda-device-only', '-S', '-o', '-', os.path.join(csrc, unit)],
                              check=True, capture_output=True, text=True).stdout

    with ThreadPoolExecutor(4) as ex:
        asm = dict(zip(units, ex.map(isa, units)))
    assert 'v_mfma_f32_32x32x16_f16' in asm['dpenv_policy.hip'] and 'step_kernel' in asm['dpenv_kernels.hip']
    assert 'policy_rollout_ws_kernel' in asm['dpenv_policy_xws1.hip'] and 'policy_rollout_ws_kernel' in asm['dpenv_policy_ws.hip']
    # (a) the exact form: a packed f32 instruction whose op_sel (the LOW result's operand select) picks the high half of src1 / src2
    swz = re.compile(r'^\s*(v_pk_\w+_f32)\b.*\bop_sel:\[\d,(?:1(?:,\d)?|\d,1)\]', re.M)
    for unit, txt in asm.items():
        assert not swz.search(txt), (unit, swz.search(txt).group(0))
        # (b) no packed fp32 arithmetic at all; the f16 forms of the network's activation packing are fine
        packed = sorted(set(re.findall(r'\bv_pk_\w+', txt)))
        assert all(q.endswith('_f16') for q in packed), (unit, packed)
    # (c) inline asm vs the matrix pipe (tools/asm_mfma_waw_scan.py, dpenv_policy_dev.h HAZARD NOTE 2): the hazard recogniser does not
    # look inside asm statements, so no asm instruction may write a register inside the destination tile of an MFMA that can still be
    # running (round 2: dead rows 80..95 of an accumulator were handed to the activation / split asm as temporaries)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from asm_mfma_waw_scan import asm_reads_of_unlanded_mfma_dest, asm_writes_into_recent_mfma_dest
    for unit in ('dpenv_policy.hip', 'dpenv_policy_ws.hip', 'dpenv_policy_x.hip', 'dpenv_policy_xws1.hip', 'dpenv_policy_xws2.hip'):
        hits = asm_writes_into_recent_mfma_dest(asm[unit])
        assert not hits, (unit, len(hits), hits[:4])
        # (d) and the read side: no asm instruction reads an MFMA result that no compiler-visible VALU instruction has read
        # first (round 2: reading the accumulators from asm directly lost the last MFMA of the chain, a 2e-5 error)
        rhits = asm_reads_of_unlanded_mfma_dest(asm[unit])
        assert not rhits, (unit, len(rhits), rhits[:4])
    bad = """k:
\tv_mfma_f32_32x32x16_f16 v[32:47], v[76:79], v[92:95], 0
\t;;#ASMSTART
\tv_max_f32 v40, v58, v28
\t;;#ASMEND
"""
    assert asm_writes_into_recent_mfma_dest(bad)
    bad_read = bad.replace('v_max_f32 v40, v58, v28', 'v_max_f32 v100, v33, v28')          # reads v33 of the tile v[32:47] straight from asm
    assert asm_reads_of_unlanded_mfma_dest(bad_read) and not asm_writes_into_recent_mfma_dest(bad_read)
    assert not asm_reads_of_unlanded_mfma_dest(bad_read.replace('\t;;#ASMSTART', '\tv_mul_f32_e32 v1, s33, v33\n\t;;#ASMSTART'))
    assert not asm_writes_into_recent_mfma_dest(bad.replace('\t;;#ASMSTART', '\tv_mul_f32_e32 v1, s33, v33\n\t;;#ASMSTART'))   # a visible read first
    assert not asm_writes_into_recent_mfma_dest(bad.replace('v_max_f32 v40', 'v_max_f32 v48'))
    # the pattern itself must be what the check looks for: the reproducer's instruction text matches, the safe form does not
    assert swz.search('\tv_pk_fma_f32 v[46:47], v[124:125], v[38:39], v[46:47] op_sel:[0,1,0]')
    assert swz.search('\tv_pk_fma_f32 v[0:1], v[2:3], v[2:3], v[4:5] op_sel:[0,0,1]')
    assert not swz.search('\tv_pk_fma_f32 v[46:47], v[38:39], v[124:125], v[46:47] op_sel:[1,0,0]')
    assert not swz.search('\tv_pk_fma_f32 v[46:47], v[54:55], v[38:39], v[46:47] op_sel_hi:[1,0,1]')
