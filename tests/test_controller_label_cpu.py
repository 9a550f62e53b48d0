"""The labelling entry point without a GPU: dpenv_controller_label is declared, exported and bound with the header's struct layout; and
deploy.label_rows, its host statement, against the three-line law written out per env, in pieces, with a per-env table of equal rows,
and on the rows of a closed loop flown on the float64 oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = float(np.float32(0.01) * np.float32(20))


def test_entry_point_is_declared_exported_and_bound():
    from ml4ca_amd import _lib, deploy, policy
    from ml4ca_amd.train import PPOUpdater
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dpenv_controller_label\s*\(', txt)
    assert hasattr(lib, 'dpenv_controller_label') and 'dpenv_controller_label' in _lib.SYMBOLS
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = [f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3]
    assert 'dpenv_controller_label' in exported
    assert not [s for s in exported if 'launch_controller_label' in s], 'the cross-unit launcher stays out of the dynamic symbol table'
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    assert lib.dpenv_controller_label(None, None, None) == _lib.EINVAL                 # no handle: refused, not crashed
    assert callable(policy.controller_label) and callable(deploy.label_rows) and callable(PPOUpdater.dagger)


def test_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    S = 'dpenv_controller_label_io'
    fs = ('struct_size', 'T', 'obs', 'obs_dtype', 'done', 'z_in', 'z_out', 'act')
    items = ['sizeof(%s)' % S] + ['offsetof(%s, %s)' % (S, f) for f in fs]
    src = tmp_path / 'lab.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (
        ' '.join(['%zu'] * len(items)), ', '.join('(size_t)' + it for it in items)))
    exe = tmp_path / 'lab'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A = _lib.ControllerLabelIO
    assert [name for name, _ in A._fields_] == list(fs)
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fs]


def _law_one_env(p, dt, z, o):
    """One control step of include/dpenv.h for ONE env in NumPy float32 scalars: z [3] is advanced in place; returns the action [7]."""
    f = np.float32
    g = lambda k: np.asarray(p[k], np.float64).astype(f)
    kp, kd, ki, zb, tmax, G, kf = g('kp'), g('kd'), g('ki'), g('z_bound'), g('tau_max'), g('G'), g('kf')
    kr, eps, dt = f(p['kr_bow']), f(p['f_eps']), f(dt)
    tau = np.zeros(3, f)
    for j in range(3):
        z[j] = min(max(f(z[j] + f(dt * o[j])), -zb[j]), zb[j])
        t = -f(f(f(kp[j] * o[j]) + f(kd[j] * o[3 + j])) + f(ki[j] * z[j]))
        tau[j] = min(max(t, -tmax[j]), tmax[j])
    fm = [f(f(f(G[m, 0] * tau[0]) + f(G[m, 1] * tau[1])) + f(G[m, 2] * tau[2])) for m in range(5)]
    act = np.zeros(7, f)
    kb = kf[0] if fm[0] >= 0 else kr
    nb = np.copysign(np.sqrt(f(abs(fm[0]) / kb)), fm[0])
    act[0] = min(max(f(nb / f(100)), f(-1)), f(1))
    for i in range(2):
        Fx, Fy = fm[1 + 2 * i], fm[2 + 2 * i]
        F = np.sqrt(f(f(Fx * Fx) + f(Fy * Fy)))
        ns = np.sqrt(f(F / kf[1 + i]))
        act[1 + i] = min(f(ns / f(100)), f(1))
        if F > eps:
            act[3 + 2 * i], act[4 + 2 * i] = f(Fy / F), f(Fx / F)
        else:
            act[3 + 2 * i], act[4 + 2 * i] = f(0), f(1)
    return act


def _block(seed=4, n=5, T=9):
    """Synthetic rows: errors large enough to wind z up to its bound and to saturate the wrench in some envs, small in others; done bytes
    placed by hand, one at row 0 and one at the last row among them."""
    rng = np.random.RandomState(seed)
    obs = (rng.uniform(-1.0, 1.0, (T, n, 9)) * (6, 6, 1.5, 1, 0.5, 0.4, 1, 1, 1)).astype(np.float32)
    obs[:, 1, 0:6] *= np.float32(0.02)                                                 # near the setpoint: unsaturated
    obs[:, 2, 0:3] = np.abs(obs[:, 2, 0:3]) + np.float32(3.0)                          # one-sided: z runs into its bound
    done = np.zeros((T, n), np.uint8)
    done[0, 0] = 1
    done[T - 1, 1] = 2
    done[3, 2] = 1
    done[4, 2] = 3                                                                     # two in a row
    done[6, 4] = 4
    z0 = rng.uniform(-0.5, 0.5, (3, n)).astype(np.float32)
    return obs, done, z0


def test_label_rows_is_the_three_line_law_per_env():
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows
    p = dp_controller_defaults()
    obs, done, z0 = _block()
    T, n = done.shape
    act, z = label_rows(p, obs, done, z0, dt=DT)
    assert act.dtype == np.float32 and act.shape == (T, n, 7) and z.dtype == np.float32 and z.shape == (3, n)
    want, wz = np.zeros((T, n, 7), np.float32), np.zeros((3, n), np.float32)
    carried = zeroed = 0
    for i in range(n):
        zi = z0[:, i].copy()
        for t in range(T):
            before = zi.copy()
            want[t, i] = _law_one_env(p, DT, zi, obs[t, i])                            # o = obs[t][i]; act = dp_control(c, o, z)
            carried += int((zi != before).any())
            if done[t, i] != 0:                                                        # the next row is a new episode's first
                zi[:] = 0
                zeroed += 1
        wz[:, i] = zi
    assert np.array_equal(act.view(np.uint32), want.view(np.uint32)), int((act != want).sum())
    assert np.array_equal(z.view(np.uint32), wz.view(np.uint32))
    assert zeroed == 5 and carried > 30
    assert (z[:, 1] == 0).all() and (z[:, 0] != 0).any()                               # done at the last row: z leaves as 0; at row 0: rebuilt since
    # z after a done row is zero: the next row's label is the law at z = 0 on that row alone
    t, i = 1, 0
    alone, _ = label_rows(p, obs[t:t + 1, i:i + 1], None, None, dt=DT)
    assert np.array_equal(alone[0, 0].view(np.uint32), act[t, i].view(np.uint32))
    # ... and carried otherwise: the same row from z = 0 differs
    alone, _ = label_rows(p, obs[2:3, 1:2], None, None, dt=DT)                         # (env 1: near the setpoint, the wrench unsaturated)
    assert not np.array_equal(alone[0, 0], act[2, 1])
    # the clips were exercised: the integral's bound and a saturated bow command; and unsaturated rows
    assert (np.abs(z) == np.float32(p['z_bound'])[:, None]).any() and (np.abs(act[..., 0]) == 1).any() and (np.abs(act[..., 0]) < 1).any()
    # done=None is a block of zero done bytes; z=None is zero
    a, za = label_rows(p, obs, None, z0, dt=DT)
    b, zb = label_rows(p, obs, np.zeros_like(done), z0, dt=DT)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(za.view(np.uint32), zb.view(np.uint32))
    assert not np.array_equal(a, act)
    a, _ = label_rows(p, obs, done, None, dt=DT)
    b, _ = label_rows(p, obs, done, np.zeros_like(z0), dt=DT)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_label_rows_in_pieces_equals_one_call():
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows
    p = dp_controller_defaults()
    obs, done, z0 = _block(seed=6)
    one, z_one = label_rows(p, obs, done, z0, dt=DT)
    a1, z = label_rows(p, obs[0:4], done[0:4], z0, dt=DT)
    a2, z = label_rows(p, obs[4:9], done[4:9], z, dt=DT)
    got = np.concatenate([a1, a2])
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32)) and np.array_equal(z.view(np.uint32), z_one.view(np.uint32))


def test_label_rows_with_a_table_of_equal_rows_gives_the_scalar_forms_bits():
    from ml4ca_amd.deploy import dp_controller_defaults, dp_controller_table, label_rows
    p = dp_controller_defaults()
    obs, done, z0 = _block(seed=8)
    n = done.shape[1]
    a, za = label_rows(p, obs, done, z0, dt=DT)
    b, zb = label_rows(dp_controller_table(n, p), obs, done, z0, dt=DT)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(za.view(np.uint32), zb.view(np.uint32))
    # ... and a table of distinct rows does not
    kp = np.asarray(p['kp'])[None] * np.linspace(0.5, 2.0, n)[:, None]
    c, _ = label_rows(dp_controller_table(n, p, kp=kp), obs, done, z0, dt=DT)
    assert not np.array_equal(c, a)


def test_label_rows_reproduces_a_closed_loop_on_the_float64_oracle():
    """The float32 host law flies the float64 oracle with auto-reset the way the closed-loop launch does - z zeroed for the envs that end
    an episode - and label_rows on the recorded obs and done rows gives the recorded actions bit for bit."""
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_defaults, label_rows
    from oracle import oracle as O
    n, T = 16, 60
    orc = O.Oracle(O.make_config(terminate=1, auto_reset=1, max_ep_len=25, seed=9), np.float64)
    state, ctr = orc.new_state(n)
    obs = orc.reset(state, ctr)
    p = dp_controller_defaults()
    ctrl = BatchedDPController(n, p, dt=DT)
    rows, acts, dones = np.zeros((T, n, 9), np.float32), np.zeros((T, n, 7), np.float32), np.zeros((T, n), np.uint8)
    for t in range(T):
        rows[t] = np.asarray(obs, np.float32)                                          # the rows a float32 block would hold
        a = ctrl.act(rows[t])
        acts[t] = a
        obs, _, d = orc.step(state, ctr, a.astype(np.float64))
        dones[t] = d
        ctrl.reset(d != 0)
    assert (dones[1:T - 1] != 0).any(0).all() and np.isfinite(acts).all()
    got, z = label_rows(p, rows, dones, None, dt=DT)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), acts.view(np.uint32)), int((got != acts).sum())
    assert np.array_equal(z.view(np.uint32), np.ascontiguousarray(ctrl.z.T).view(np.uint32))
