"""CPU checks of the deployed controller's integral action (include/dpenv.h dpenv_set_integral_action): the batched torch law
deploy.BatchedBodyFrameIntegrator against the node-pinned deploy.BodyFrameIntegrator (rl_allocator.py:252-273), its float32 operation
order against a NumPy restatement, and the C ABI of the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.25            # exact in binary: the node's clock (now = k * DT) and the step count decide the dwell the same way
D = 21               # the smallest D with D * 0.25 > 5.0


def _scripted_errors(K=90):
    """[K, n, 3] error sequences, one per env, that cross every branch of the law."""
    deg140 = float(np.deg2rad(140.0))
    e = np.zeros((K, 12, 3))
    e[:, 0] = (4.9, 4.9, 2.40)                                   # wind-up to every bound, just inside the box
    e[:, 1] = (-4.9, -4.9, -2.40)                                # ... and to the negative bounds
    e[:, 2] = (1.0, 0.5, 0.1)
    e[40, 2, 0] = 5.5                                            # leaves the box on x: I and the dwell clock reset
    e[:, 3] = (0.5, 1.0, -0.1)
    e[50, 3, 1] = -5.25                                          # ... on y
    e[:, 4] = (0.3, -0.2, 0.2)
    e[30, 4, 2] = deg140 + 0.01                                  # ... on yaw
    e[:, 5] = (5.0, -5.0, deg140)                                # exactly on the box: inside (strict >, as the node)
    e[:, 6] = (2.0, -3.0, 0.3) * np.where(np.arange(K) % 7 < 3, 1.0, -1.0)[:, None]    # sign reversals
    e[:, 7] = (0.7, 0.2, -0.05)
    e[:D + 1, 7] = (6.0, 0.0, 0.0)                               # arrives at k = D + 2: the dwell boundary later in the run
    e[:, 8] = (4.0, 4.0, 1.0)
    e[::11, 8, 0] = 5.0 + 1e-9                                   # knocked out of the box again and again: never dwells
    rng = np.random.RandomState(4)
    e[:, 9:] = rng.uniform(-6.0, 6.0, size=(K, 3, 3)) * (1.0, 1.0, 0.5)
    e[:, 9:, :] *= (rng.uniform(size=(K, 3, 1)) < 0.9) * 0.5 + 0.5
    return e


def _node_reference(e, step):
    from ml4ca_amd.deploy import BodyFrameIntegrator
    K, n, _ = e.shape
    out = np.zeros_like(e)
    for i in range(n):
        node = BodyFrameIntegrator(now=0.0)
        for k in range(K):
            out[k, i] = node.update(e[k, i], step, now=(k + 1) * DT)
    return out


def test_batched_law_equals_the_node_integrator_in_float64():
    import torch
    from ml4ca_amd.deploy import BatchedBodyFrameIntegrator, dwell_steps
    assert dwell_steps(5.0, DT) == D
    e = _scripted_errors()
    for step in (DT, 0.1):                                       # the node's control period, and another integration step
        ref = _node_reference(e, step)
        law = BatchedBodyFrameIntegrator(e.shape[1], dt=DT, step_s=step, dtype=torch.float64)
        got = np.stack([law.update(torch.from_numpy(e[k])).numpy() for k in range(e.shape[0])])
        assert np.abs(got - ref).max() < 1e-12
    # what the sequences exercised
    I = ref - e                                                  # (step 0.1)
    assert np.all(I[:D - 1] == 0.0)                              # k = D - 1: the dwell is not over (node: (D - 1) * dt = 5.0, not > 5)
    assert np.all(I[D - 1, :2] != 0.0) and np.all(I[D - 1, 5] != 0.0)   # k = D: integrating
    assert np.all(I[2 * D - 1, 7] == 0.0) and np.all(I[2 * D, 7] != 0.0)          # re-arrival at k = D + 2: dwell over D steps later
    ref = _node_reference(e, DT)
    I = ref - e
    bound = np.array([0.5, 1.0, np.pi / 32])
    assert np.allclose(I[-1, 0], bound, rtol=0, atol=1e-12) and np.allclose(I[-1, 1], -bound, rtol=0, atol=1e-12)   # wound up to every bound
    assert np.all(I[40, 2] == 0.0) and np.all(I[50, 3] == 0.0) and np.all(I[30, 4] == 0.0)                  # left the box: reset
    assert np.all(I[39, 2] != 0.0) and np.all(I[49, 3] != 0.0) and np.all(I[29, 4] != 0.0)
    assert np.all(I[-1, 8] == 0.0)
    assert np.any(np.diff(np.sign(I[:, 6, 0])) != 0)            # the sign reversals pulled I through zero


def test_batched_law_reset_zeroes_the_chosen_envs():
    import torch
    from ml4ca_amd.deploy import BatchedBodyFrameIntegrator
    law = BatchedBodyFrameIntegrator(4, dt=DT, dtype=torch.float64)
    e = torch.full((4, 3), 0.5, dtype=torch.float64)
    for _ in range(D + 3):
        law.update(e)
    assert bool((law.I != 0).all()) and bool((law.count == D).all())
    law.reset(torch.tensor([True, False, True, False]))
    assert bool((law.I[0::2] == 0).all()) and bool((law.count[0::2] == 0).all()) and bool((law.I[1::2] != 0).all())
    out = law.update(e)                                          # a reset env starts its dwell again
    assert torch.equal(out[0], e[0]) and bool((law.count[0::2] == 1).all())


def test_float32_form_follows_the_stated_operation_order():
    """In float32 the torch law is the kernels' f32 order: I_j = min(max(I_j + step_s * (gain_j * e_j), -bound_j), bound_j), compared
    bit for bit with a NumPy restatement (and the dwell count as int32)."""
    import torch
    from ml4ca_amd.deploy import BatchedBodyFrameIntegrator
    f = np.float32
    e = _scripted_errors().astype(f)
    dt = float(f(0.01) * f(20))                                  # the env's control period in f32 (0.2 s)
    gain, bound, box = (0.05, 0.07, 0.03), (0.5, 1.0, np.pi / 32), (5.0, 5.0, np.deg2rad(140.0))
    for step in (None, 0.1):
        law = BatchedBodyFrameIntegrator(e.shape[1], gain=gain, bound=bound, box=box, dt=dt, step_s=step)
        g, b, bx, s = f(gain), np.asarray(bound, f), np.asarray(box, f), f(dt if step is None else step)
        I = np.zeros((e.shape[1], 3), f)
        c = np.zeros(e.shape[1], np.int32)
        Dd = 26
        assert law.dwell == Dd
        for k in range(e.shape[0]):
            ek = e[k]
            outside = (np.abs(ek) > bx).any(1)
            c = np.where(outside, 0, np.minimum(c + 1, Dd)).astype(np.int32)
            new = np.minimum(np.maximum(I + s * (g * ek), -b), b)
            I = np.where(outside[:, None], f(0), np.where(((~outside) & (c >= Dd))[:, None], new, I)).astype(f)
            want = ek + I
            got = law.update(torch.from_numpy(ek)).numpy()
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
            assert np.array_equal(law.count.numpy(), c)
        assert np.any(I != 0)


def _header():
    return open(os.path.join(ROOT, 'include', 'dpenv.h')).read()


def test_integral_action_entry_points_are_declared_exported_and_versioned():
    from ml4ca_amd import _lib
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    new = ('dpenv_set_integral_action', 'dpenv_get_integral_state', 'dpenv_set_integral_state', 'dpenv_policy_rollout_integral')
    for name in new:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', _header()).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    # no handle: refused, not crashed (no GPU needed)
    ia = _lib.IntegralAction()
    ia.struct_size = C.sizeof(_lib.IntegralAction)
    assert lib.dpenv_set_integral_action(None, C.byref(ia), None) == _lib.EINVAL
    assert lib.dpenv_get_integral_state(None, None, None, None) == _lib.EINVAL
    assert lib.dpenv_policy_rollout_integral(None, None, None, None) == _lib.EINVAL


def test_integral_action_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    src = tmp_path / 'ia.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dpenv_integral_action), offsetof(dpenv_integral_action, gain),'
                   ' offsetof(dpenv_integral_action, bound), offsetof(dpenv_integral_action, box), offsetof(dpenv_integral_action, dwell_s),'
                   ' offsetof(dpenv_integral_action, step_s));return 0;}\n')
    exe = tmp_path / 'ia'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.IntegralAction
    assert got == [C.sizeof(S), S.gain.offset, S.bound.offset, S.box.offset, S.dwell_s.offset, S.step_s.offset]
