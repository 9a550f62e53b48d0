"""The QP labelling entry point without a GPU: dpenv_controller_label_qp is declared, exported and bound with the header's struct layout;
and deploy.label_rows_qp, its host statement, against the composition written out per row - wrench, allocate, the two resets - in
float32 and float64, in pieces, with a per-env table of equal rows, and on the rows of a QP closed loop flown on the float64 oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = float(np.float32(0.01) * np.float32(20))
K = 8


def _qp(iters=K):
    from ml4ca_amd.deploy import qp_allocator_defaults
    p = qp_allocator_defaults()
    p['iterations'] = iters
    return p


def test_entry_point_is_declared_exported_and_bound():
    from ml4ca_amd import _lib, deploy, policy
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dpenv_controller_label_qp\s*\(', txt)
    assert hasattr(lib, 'dpenv_controller_label_qp') and 'dpenv_controller_label_qp' in _lib.SYMBOLS
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = [f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3]
    assert 'dpenv_controller_label_qp' in exported
    assert not [s for s in exported if 'launch_controller_label_qp' in s], 'the cross-unit launcher stays out of the dynamic symbol table'
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    assert lib.dpenv_controller_label_qp(None, None, None) == _lib.EINVAL              # no handle: refused, not crashed
    assert callable(policy.controller_label_qp) and callable(deploy.label_rows_qp)


def test_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    S = 'dpenv_controller_label_qp_io'
    fs = ('struct_size', 'T', 'obs', 'obs_dtype', 'done', 'z_in', 'z_out', 'x_in', 'x_out', 'act', 'cost', 'q')
    items = ['sizeof(%s)' % S] + ['offsetof(%s, %s)' % (S, f) for f in fs]
    src = tmp_path / 'labqp.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (
        ' '.join(['%zu'] * len(items)), ', '.join('(size_t)' + it for it in items)))
    exe = tmp_path / 'labqp'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A = _lib.ControllerLabelQpIO
    assert [name for name, _ in A._fields_] == list(fs)
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fs]
    # the pseudo-inverse call's struct is what it was
    assert [name for name, _ in _lib.ControllerLabelIO._fields_] == ['struct_size', 'T', 'obs', 'obs_dtype', 'done', 'z_in', 'z_out', 'act']


def test_example_refuses_the_qp_warm_start_on_randomised_hulls_and_names_the_way():
    """--expert qp --randomise R --warm-start N would have to FLY the QP on per-env hulls: an argparse error, before any device is touched,
    that names --dagger without --warm-start."""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_ppo.py'), '--update', 'fused', '--expert', 'qp', '--randomise', '0.15',
                        '--warm-start', '10'], capture_output=True, text=True)
    assert r.returncode == 2 and '--dagger without --warm-start' in r.stderr, r.stderr[-400:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_ppo.py'), '--expert', 'slsqp'], capture_output=True, text=True)
    assert r.returncode == 2 and "'pinv', 'qp'" in r.stderr, r.stderr[-400:]


def _block(seed=4, n=5, T=9):
    """Synthetic rows: errors large enough to wind z up to its bound and to saturate the wrench in some envs, small in others; done bytes
    placed by hand: at row 0, at the last row and two in a row among them; a starting integral and a starting thruster state."""
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
    x0 = (rng.uniform(-1.0, 1.0, (5, n)) * np.array([4, 8, 8, 2, 2])[:, None]).astype(np.float32)
    return obs, done, z0, x0


def _by_hand(p, q, obs, done, z0, x0, dtype):
    """The composition of the header, row by row: wrench, allocate, then the two resets behind a done row."""
    from ml4ca_amd.deploy import BatchedDPController, BatchedQPAllocator
    T, n = obs.shape[:2]
    ctrl, qp = BatchedDPController(n, p, dt=DT, dtype=dtype), BatchedQPAllocator(n, q, dt=DT, dtype=dtype)
    if z0 is not None:
        ctrl.z = np.ascontiguousarray(z0.T).astype(dtype)
    if x0 is not None:
        qp.x = np.ascontiguousarray(x0.T).astype(dtype)
    act = np.zeros((T, n, 7), dtype)
    moved = zeroed = 0
    for t in range(T):
        tau = ctrl.wrench(obs[t])                                                      # z advanced first, the wrench clipped
        before = qp.x.copy()
        act[t] = qp.allocate(tau)                                                      # x advanced in place
        moved += int((qp.x != before).any(1).sum())
        if done is not None:
            m = done[t] != 0
            ctrl.reset(m)
            qp.reset(m)
            zeroed += int(m.sum())
    return act, np.ascontiguousarray(ctrl.z.T), np.ascontiguousarray(qp.x.T), moved, zeroed


def _same(a, b):
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_label_rows_qp_is_the_composition_row_by_row(dtype):
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_qp
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block()
    T, n = done.shape
    act, z, x = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype)
    assert act.dtype == dtype and act.shape == (T, n, 7) and z.dtype == dtype and z.shape == (3, n) and x.dtype == dtype and x.shape == (5, n)
    want, wz, wx, moved, zeroed = _by_hand(p, q, obs, done, z0, x0, dtype)
    assert _same(act, want), int((act != want).sum())
    assert _same(z, wz) and _same(x, wx)
    assert zeroed == 5 and moved > 30 and np.isfinite(act).all()
    assert (z[:, 1] == 0).all() and (x[:, 1] == 0).all() and (x[:, 0] != 0).any()      # done at the last row: both leave as 0; at row 0: rebuilt since
    # behind a done row the next label is the chain from z = 0 and thrusters at rest on that row alone
    alone, _, _ = label_rows_qp(p, q, obs[1:2, 0:1], None, None, None, dt=DT, dtype=dtype)
    assert _same(alone[0, 0], act[1, 0])
    # ... and carried otherwise: the same row from rest differs
    alone, _, _ = label_rows_qp(p, q, obs[2:3, 3:4], None, None, None, dt=DT, dtype=dtype)
    assert not np.array_equal(alone[0, 0], act[2, 3])
    # done=None is a block of zero done bytes; z=None and x=None are zeros
    a = label_rows_qp(p, q, obs, None, z0, x0, dt=DT, dtype=dtype)
    b = label_rows_qp(p, q, obs, np.zeros_like(done), z0, x0, dt=DT, dtype=dtype)
    assert all(_same(u, v) for u, v in zip(a, b)) and not np.array_equal(a[0], act)
    a = label_rows_qp(p, q, obs, done, None, None, dt=DT, dtype=dtype)
    b = label_rows_qp(p, q, obs, done, np.zeros_like(z0), np.zeros_like(x0), dt=DT, dtype=dtype)
    assert all(_same(u, v) for u, v in zip(a, b)) and not np.array_equal(a[0], act)
    c = label_rows_qp(p, q, obs, done, z0, None, dt=DT, dtype=dtype)
    assert not np.array_equal(c[0], act) and not np.array_equal(c[0], a[0])            # z and x each matter
    # the iteration count is live
    d = label_rows_qp(p, _qp(2), obs, done, z0, x0, dt=DT, dtype=dtype)
    assert not np.array_equal(d[0], act)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_label_rows_qp_in_pieces_equals_one_call(dtype):
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_qp
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block(seed=6)
    one, z_one, x_one = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype)
    a1, z, x = label_rows_qp(p, q, obs[0:4], done[0:4], z0, x0, dt=DT, dtype=dtype)
    a2, z, x = label_rows_qp(p, q, obs[4:9], done[4:9], z, x, dt=DT, dtype=dtype)
    assert _same(np.concatenate([a1, a2]), one) and _same(z, z_one) and _same(x, x_one)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_label_rows_qp_with_a_table_of_equal_rows_gives_the_scalar_forms_bits(dtype):
    from ml4ca_amd.deploy import dp_controller_defaults, dp_controller_table, label_rows_qp
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block(seed=8)
    n = done.shape[1]
    a = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype)
    if dtype == np.float32:                                                            # (the public table is float32: its rows are the scalar numbers rounded)
        b = label_rows_qp(dp_controller_table(n, p), q, obs, done, z0, x0, dt=DT, dtype=dtype)
        assert all(_same(u, v) for u, v in zip(a, b))
    else:
        per = dict(p, kp=np.repeat(np.asarray(p['kp'])[None], n, 0), ki=np.repeat(np.asarray(p['ki'])[None], n, 0))
        b = label_rows_qp(per, q, obs, done, z0, x0, dt=DT, dtype=dtype)
        assert all(_same(u, v) for u, v in zip(a, b))
    # ... and a table of distinct rows does not
    kp = np.asarray(p['kp'])[None] * np.linspace(0.5, 2.0, n)[:, None]
    c = label_rows_qp(dp_controller_table(n, p, kp=kp), q, obs, done, z0, x0, dt=DT, dtype=dtype)
    assert not np.array_equal(c[0], a[0])


def test_label_rows_qp_reproduces_a_qp_closed_loop_on_the_float64_oracle():
    """The float32 host chain flies the float64 oracle with auto-reset the way the closed-loop launch does - z and the thruster state
    zeroed for the envs that end an episode - and label_rows_qp on the recorded obs and done rows gives the recorded actions bit for bit."""
    from ml4ca_amd.deploy import BatchedDPController, BatchedQPAllocator, dp_controller_defaults, label_rows_qp
    from oracle import oracle as O
    n, T = 16, 60
    orc = O.Oracle(O.make_config(terminate=1, auto_reset=1, max_ep_len=25, seed=9), np.float64)
    state, ctr = orc.new_state(n)
    obs = orc.reset(state, ctr)
    p, q = dp_controller_defaults(), _qp()
    ctrl, qp = BatchedDPController(n, p, dt=DT), BatchedQPAllocator(n, q, dt=DT)
    rows, acts, dones = np.zeros((T, n, 9), np.float32), np.zeros((T, n, 7), np.float32), np.zeros((T, n), np.uint8)
    for t in range(T):
        rows[t] = np.asarray(obs, np.float32)                                          # the rows a float32 block would hold
        a = qp.allocate(ctrl.wrench(rows[t]))
        acts[t] = a
        obs, _, d = orc.step(state, ctr, a.astype(np.float64))
        dones[t] = d
        ctrl.reset(d != 0)
        qp.reset(d != 0)
    assert (dones[1:T - 1] != 0).any(0).all(), 'every env ends an episode in an interior row'
    assert np.isfinite(acts).all()
    got, z, x = label_rows_qp(p, q, rows, dones, None, None, dt=DT)
    assert got.dtype == np.float32 and _same(got, acts), int((got != acts).sum())
    assert _same(z, np.ascontiguousarray(ctrl.z.T)) and _same(x, np.ascontiguousarray(qp.x.T))
    assert (x != 0).any()
