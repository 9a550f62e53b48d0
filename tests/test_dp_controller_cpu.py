"""CPU checks of the classical baseline (include/dpenv.h dpenv_set_dp_controller): the allocation matrix, the host law
deploy.BatchedDPController in float64 against the thruster force map, its float32 operation order against a line-by-line NumPy
restatement, the closed loop on the float64 oracle, and the C ABI of the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LX = (1.08, -1.12, -1.12)
LY = (0.0, -0.15, 0.15)


def _T(lx, ly):
    return np.array([[0, 1, 0, 1, 0], [1, 0, 1, 0, 1], [lx[0], -ly[1], lx[1], -ly[2], lx[2]]], np.float64)


def test_allocation_matrix_is_the_weighted_pseudo_inverse():
    from ml4ca_amd import _lib
    from ml4ca_amd.deploy import allocation_matrix
    G = allocation_matrix(LX, LY)
    assert G.shape == (5, 3) and G.dtype == np.float64
    assert np.abs(G - np.linalg.pinv(_T(LX, LY))).max() < 1e-12
    rng = np.random.RandomState(0)
    for _ in range(20):
        w = rng.uniform(0.1, 10.0, 5)
        lx = np.array(LX) + rng.uniform(-0.2, 0.2, 3)
        ly = np.array(LY) + rng.uniform(-0.05, 0.05, 3)
        G = allocation_matrix(lx, ly, w)
        assert np.abs(_T(lx, ly) @ G - np.eye(3)).max() < 1e-12
        Wi = np.diag(1.0 / w)
        T = _T(lx, ly)
        assert np.abs(G - Wi @ T.T @ np.linalg.inv(T @ Wi @ T.T)).max() < 1e-12
    # the C function: f64 inside, rounded once to f32
    lib = _lib.load()
    f3, f5 = C.c_float * 3, C.c_float * 5
    for w in ((1, 1, 1, 1, 1), (2.0, 0.5, 1.5, 0.25, 3.0)):
        lx32, ly32, w32 = np.float32(LX), np.float32(LY), np.float32(w)
        out = (C.c_float * 3 * 5)()
        assert lib.dpenv_dp_allocation_matrix(f3(*lx32), f3(*ly32), f5(*w32), C.byref(out)) == _lib.OK
        want = allocation_matrix(lx32.astype(np.float64), ly32.astype(np.float64), w32.astype(np.float64)).astype(np.float32)
        assert np.array_equal(np.array(out, np.float32).reshape(5, 3).view(np.uint32), want.view(np.uint32))
    out = (C.c_float * 3 * 5)()
    assert lib.dpenv_dp_allocation_matrix(f3(*LX), f3(*LY), f5(1, 1, 0, 1, 1), C.byref(out)) == _lib.EINVAL
    assert lib.dpenv_dp_allocation_matrix(None, f3(*LY), f5(1, 1, 1, 1, 1), C.byref(out)) == _lib.EINVAL


def _decode(act, p):
    """tau [n, 3] that the action's commands produce: B(alpha) K n|n| in env order (bow, port, star)."""
    from ml4ca_amd import allocation
    n_pct = act[:, 0:3] * 100.0
    alpha = np.stack([np.full(len(act), np.pi / 2), np.arctan2(act[:, 3], act[:, 4]), np.arctan2(act[:, 5], act[:, 6])], 1)
    K = np.stack([np.where(n_pct[:, 0] >= 0, p['kf'][0], p['kr_bow']), np.full(len(act), p['kf'][1]), np.full(len(act), p['kf'][2])], 1)
    F = K * n_pct * np.abs(n_pct)
    return np.stack([allocation.effectiveness(alpha[i], np.asarray(p['lx']), np.asarray(p['ly'])) @ F[i] for i in range(len(act))])


def test_host_law_in_float64_reproduces_the_wrench():
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_defaults
    p = dp_controller_defaults()
    rng = np.random.RandomState(1)
    tau = rng.uniform(-1.0, 1.0, (2000, 3)) * (15.0, 6.0, 6.0)
    ctrl = BatchedDPController(len(tau), p, dtype=np.float64)
    act = ctrl.allocate(tau)
    assert act.dtype == np.float64 and act.shape == (2000, 7)
    inside = (np.abs(act[:, 0]) < 1.0) & (act[:, 1] < 1.0) & (act[:, 2] < 1.0)
    assert inside.sum() > 1000
    assert np.abs(_decode(act[inside], p) - tau[inside]).max() < 1e-9
    assert np.abs(np.hypot(act[:, 3], act[:, 4]) - 1.0).max() < 1e-12 and np.all(act[:, 1:3] >= 0.0)
    # saturation clips, and is not redistributed
    big = ctrl.allocate(np.array([[400.0, 0.0, 0.0], [0.0, -300.0, 0.0], [0.0, 300.0, 0.0]]))
    assert np.all(big[0, 1:3] == 1.0) and big[1, 0] == -1.0 and big[2, 0] == 1.0
    # a stern force at or below f_eps keeps the direction (0, 1)
    zero = ctrl.allocate(np.zeros((1, 3)))
    assert np.array_equal(zero[0], [0, 0, 0, 0, 1, 0, 1])
    tiny = ctrl.allocate(np.array([[1e-7, 0.0, 0.0]]))
    assert np.array_equal(tiny[0, 3:], [0, 1, 0, 1]) and tiny[0, 1] > 0.0
    # the PID part: z integrates and clips at its bound, tau clips at tau_max
    c2 = BatchedDPController(1, p, dtype=np.float64)
    o = np.zeros((1, 9))
    o[0, 0] = 4.0
    for _ in range(20):
        t = c2.wrench(o)
    assert c2.z[0, 0] == 10.0 and t[0, 0] == -p['tau_max'][0] and t[0, 1] == 0.0
    c2.reset()
    assert np.all(c2.z == 0.0)
    o[0, 0] = 0.01
    t = c2.wrench(o)
    assert abs(t[0, 0] + (p['kp'][0] * 0.01 + p['ki'][0] * (0.2 * 0.01))) < 1e-6      # dt is the f32 control period
    # the defaults: pole placement on the default hull
    w = np.array([0.619, 0.619, 1.51])
    m, d = np.array([263.93, 300.9, 300.0]), np.array([3.0, 19.8, 77.8])
    assert np.allclose(p['kp'], m * w * w, rtol=1e-6) and np.allclose(p['kd'], 2 * w * m - d, rtol=1e-6)
    assert np.allclose(p['ki'], p['kp'] * w / 10, rtol=1e-12)
    assert tuple(p['z_bound']) == (10.0, 10.0, 2.0) and tuple(p['tau_max']) == (69.0, 30.0, 80.0) and p['f_eps'] == 1e-6


def _law_f32(p, dt, z, o):
    """The law of include/dpenv.h line by line in NumPy float32; z [n, 3] is updated in place."""
    f = np.float32
    kp, kd, ki, zb, tmax = (np.asarray(p[k], np.float64).astype(f) for k in ('kp', 'kd', 'ki', 'z_bound', 'tau_max'))
    G, kf, kr, eps = np.asarray(p['G'], np.float64).astype(f), np.asarray(p['kf'], np.float64).astype(f), f(p['kr_bow']), f(p['f_eps'])
    dt = f(dt)
    tau = np.zeros((len(o), 3), f)
    for j in range(3):
        z[:, j] = np.minimum(np.maximum(z[:, j] + dt * o[:, j], -zb[j]), zb[j])
        t = -((kp[j] * o[:, j] + kd[j] * o[:, 3 + j]) + ki[j] * z[:, j])
        tau[:, j] = np.minimum(np.maximum(t, -tmax[j]), tmax[j])
    fm = [(G[m, 0] * tau[:, 0] + G[m, 1] * tau[:, 1]) + G[m, 2] * tau[:, 2] for m in range(5)]
    act = np.zeros((len(o), 7), f)
    kb = np.where(fm[0] >= f(0), kf[0], kr).astype(f)
    nb = np.copysign(np.sqrt(np.abs(fm[0]) / kb), fm[0])
    act[:, 0] = np.minimum(np.maximum(nb / f(100), f(-1)), f(1))
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(2):
            Fx, Fy = fm[1 + 2 * i], fm[2 + 2 * i]
            F = np.sqrt(Fx * Fx + Fy * Fy)
            ns = np.sqrt(F / kf[1 + i])
            act[:, 1 + i] = np.minimum(ns / f(100), f(1))
            act[:, 3 + 2 * i] = np.where(F > eps, Fy / F, f(0))
            act[:, 4 + 2 * i] = np.where(F > eps, Fx / F, f(1))
    assert all(x.dtype == f for x in fm + [tau, nb, F, ns])
    return act, tau


def test_float32_form_follows_the_stated_operation_order():
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_defaults
    p = dp_controller_defaults()
    dt = float(np.float32(0.01) * np.float32(20))
    n = 10000
    rng = np.random.RandomState(2)
    ctrl = BatchedDPController(n, p, dt=dt)
    z = np.zeros((n, 3), np.float32)
    hit_z = hit_tau = 0
    for k in range(4):
        o = (rng.uniform(-1.0, 1.0, (n, 9)) * (6, 6, 1.5, 1, 0.5, 0.4, 1, 1, 1)).astype(np.float32)
        o[: n // 4, 0:3] *= np.float32(0.02)                       # near the setpoint: unsaturated wrenches
        o[: n // 4, 3:6] *= np.float32(0.02)
        o[n // 4: n // 2, 0:3] = np.abs(o[n // 4: n // 2, 0:3]) + np.float32(3.0)   # one-sided: z winds up to its bound
        if k == 3:
            o[-8:] = 0.0                                           # e = nu = 0 ...
            z[-8:] = 0.0                                           # ... at z = 0: tau = 0, the direction stays (0, 1)
            ctrl.z[-8:] = 0.0
        want, tau = _law_f32(p, dt, z, o)
        got = ctrl.act(o)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(ctrl.z.view(np.uint32), z.view(np.uint32))
        hit_z += int((np.abs(z) == np.float32(p['z_bound'])).any(1).sum())
        hit_tau += int((np.abs(tau) == np.float32(p['tau_max'])).any(1).sum())
    assert hit_z > 100 and hit_tau > 100
    assert np.array_equal(got[-8:], np.tile(np.float32([0, 0, 0, 0, 1, 0, 1]), (8, 1)))
    assert (np.abs(got[:, 0]) < 1).any() and (got[:, 1] < 1).any() and (got[:, 1] == 1).any() and (np.abs(got[:, 0]) == 1).any()


def _oracle_box_test(current=None):
    """The 1 250-step box test flown by the float64 host law on the float64 oracle, 16 envs: (e [T, n, 3], iae [n])."""
    import torch
    from ml4ca_amd import evaluate
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_defaults
    from oracle import oracle as O
    n, T = 16, 1250
    orc = O.Oracle(O.make_config(terminate=0, current_enabled=0 if current is None else 1), np.float64)
    state, ctr = orc.new_state(n)
    obs = orc.reset(state, ctr, init=np.zeros((6, n)), ref=np.zeros((3, n)))
    steps, refs = evaluate.box_schedule(torch.zeros((3, n), dtype=torch.float64), dt=0.2)
    refs = refs.numpy()
    ctrl = BatchedDPController(n, dp_controller_defaults(), dt=0.2, dtype=np.float64)
    rows = np.zeros((T, n, 9))
    for t in range(T):
        rows[t] = obs
        a = ctrl.act(obs)
        obs, _, _ = orc.step(state, ctr, a, new_ref=refs[steps.index(t)] if t in steps else None, current=current)
    assert np.isfinite(rows).all() and np.isfinite(state).all()
    tot, _ = evaluate.iae(torch.from_numpy(rows), dt=0.2)
    return rows[..., :3], tot.numpy()


def test_closed_loop_on_the_oracle_settles_the_box_test():
    """Calm water, default gains: the loop stays finite and over the last 10 s every env is within 0.25 m, 0.25 m, 0.05 rad of the last
    setpoint - 2.5 x the worst axis measured when the law was fixed (0.016 m, 0.093 m, under 0.001 rad; IAE 58.8).  In a 0.2 m/s
    current from 16 directions the flight stays finite; its IAE is recorded only (measured: mean 64.3, max 76.8)."""
    e, tot = _oracle_box_test()
    tail = np.abs(e[-50:]).max(axis=(0, 1))
    print('calm: tail |e| = %s, IAE mean %.1f max %.1f' % (tail, tot.mean(), tot.max()))
    assert tail[0] < 0.25 and tail[1] < 0.25 and tail[2] < 0.05
    n = 16
    cur = np.ascontiguousarray(np.stack([np.full(n, 0.2), 2 * np.pi * np.arange(n) / n]))
    e, tot = _oracle_box_test(cur)
    print('0.2 m/s from 16 directions: tail |e| = %s, IAE mean %.1f max %.1f' % (np.abs(e[-50:]).max(axis=(0, 1)), tot.mean(), tot.max()))
    assert np.isfinite(tot).all()


def _header():
    return open(os.path.join(ROOT, 'include', 'dpenv.h')).read()


def test_dp_controller_entry_points_are_declared_exported_and_bound():
    from ml4ca_amd import _lib
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    new = ('dpenv_dp_allocation_matrix', 'dpenv_set_dp_controller', 'dpenv_get_dp_controller_state', 'dpenv_set_dp_controller_state',
           'dpenv_controller_rollout', 'dpenv_thrust_alloc')
    for name in new:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', _header()).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    # no handle / bad arguments: refused, not crashed (no GPU needed)
    c = _lib.DPController()
    c.struct_size = C.sizeof(_lib.DPController)
    assert lib.dpenv_set_dp_controller(None, C.byref(c), None) == _lib.EINVAL
    assert lib.dpenv_get_dp_controller_state(None, None, None) == _lib.EINVAL
    assert lib.dpenv_set_dp_controller_state(None, None, None) == _lib.EINVAL
    assert lib.dpenv_controller_rollout(None, None, None) == _lib.EINVAL
    assert lib.dpenv_thrust_alloc(None, None, None, 4, None) == _lib.EINVAL
    assert lib.dpenv_thrust_alloc(C.byref(c), C.c_void_p(16), C.c_void_p(16), 4, None) == _lib.EINVAL      # kf = 0: refused on the host
    assert b'kf' in lib.dpenv_last_error(None)
    from ml4ca_amd import env, evaluate, policy
    for mod, names in ((env.BatchedRevoltEnv, ('set_dp_controller', 'get_dp_controller_state', 'set_dp_controller_state')),
                       (policy, ('controller_rollout',)), (evaluate, ('baseline_box_test', 'baseline_box_test_streamed'))):
        for name in names:
            assert callable(getattr(mod, name)), name


def test_dp_controller_struct_layouts_match_header(tmp_path):
    from ml4ca_amd import _lib
    src = tmp_path / 'dp.c'
    S, R = 'dpenv_dp_controller', 'dpenv_controller_rollout_io'
    fs = ('kp', 'kd', 'ki', 'z_bound', 'tau_max', 'G', 'kf', 'kr_bow', 'f_eps')
    fr = ('T', 'obs', 'act', 'reward', 'done', 'last_obs', 'ref_out', 'n_switch', 'switch_step', 'refs')
    items = ['sizeof(%s)' % S] + ['offsetof(%s, %s)' % (S, f) for f in fs] + ['sizeof(%s)' % R] + ['offsetof(%s, %s)' % (R, f) for f in fr]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (
        ' '.join(['%zu'] * len(items)), ', '.join('(size_t)' + it for it in items)))
    exe = tmp_path / 'dp'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A, B = _lib.DPController, _lib.ControllerRolloutIO
    want = [C.sizeof(A)] + [getattr(A, f).offset for f in fs] + [C.sizeof(B)] + [getattr(B, f).offset for f in fr]
    assert got == want
    assert C.sizeof(A) == 4 * (1 + 15 + 15 + 3 + 2)
