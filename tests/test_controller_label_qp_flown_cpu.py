"""The flown-state / per-env form of the QP labelling scan without a GPU: dpenv_controller_label_qp_ex is declared, exported and bound with
the header's struct layout; deploy.qp_state_from_action, the host statement of S (the thruster state an executed action row leaves), on
round trips and at its edges; and deploy.label_rows_qp(flown=..., a QP table) against the composition written out per row, in pieces,
behind done rows, with refused rows, and on the rows of a QP closed loop flown on the float64 oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_controller_label_qp_cpu import DT, _block, _by_hand, _qp, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_FIELDS = ('struct_size', 'T', 'obs', 'obs_dtype', 'done', 'z_in', 'z_out', 'x_in', 'x_out', 'act', 'cost', 'q')
NEW_FIELDS = ('flown', 'qp_table', 'iterations', 'refused_out')


def test_entry_point_is_declared_exported_and_bound():
    from ml4ca_amd import _lib, deploy, evaluate, policy
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dpenv_controller_label_qp_ex\s*\(', txt)
    assert hasattr(lib, 'dpenv_controller_label_qp_ex') and 'dpenv_controller_label_qp_ex' in _lib.SYMBOLS
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = [f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3]
    assert 'dpenv_controller_label_qp_ex' in exported and 'dpenv_controller_label_qp' in exported
    assert not [s for s in exported if 'launch_controller_label_qp' in s], 'the cross-unit launchers stay out of the dynamic symbol table'
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    assert lib.dpenv_controller_label_qp_ex(None, None, None) == _lib.EINVAL           # no handle: refused, not crashed
    assert callable(deploy.qp_state_from_action) and callable(deploy.qp_table_refused) and callable(evaluate.qp_label_sweep)
    import inspect
    for fn, names in ((policy.controller_label_qp, ('flown', 'table', 'iterations', 'refused')), (deploy.label_rows_qp, ('flown',))):
        sig = inspect.signature(fn).parameters
        assert all(k in sig and sig[k].default is None for k in names), fn
    from ml4ca_amd.train import PPOUpdater
    sig = inspect.signature(PPOUpdater.dagger).parameters
    assert sig['thruster_state'].default == 'own' and sig['qp_table'].default is None


def test_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    S = 'dpenv_controller_label_qp_ex_io'
    fs = OLD_FIELDS + NEW_FIELDS
    items = ['sizeof(%s)' % S] + ['offsetof(%s, %s)' % (S, f) for f in fs]
    items += ['offsetof(dpenv_controller_label_qp_io, %s)' % f for f in OLD_FIELDS] + ['sizeof(dpenv_controller_label_qp_io)']
    src = tmp_path / 'labqpex.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (
        ' '.join(['%zu'] * len(items)), ', '.join('(size_t)' + it for it in items)))
    exe = tmp_path / 'labqpex'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A, B = _lib.ControllerLabelQpExIO, _lib.ControllerLabelQpIO
    assert [name for name, _ in A._fields_] == list(fs)
    k = 1 + len(fs)
    assert got[:k] == [C.sizeof(A)] + [getattr(A, f).offset for f in fs]
    # every field of the old struct, in that order, at the same place; and the old struct is what it was
    assert [name for name, _ in B._fields_] == list(OLD_FIELDS)
    assert got[k:] == [getattr(B, f).offset for f in OLD_FIELDS] + [C.sizeof(B)]
    assert got[1:1 + len(OLD_FIELDS)] == got[k:-1]


def test_example_takes_the_expert_state_and_refuses_it_without_the_qp():
    import sys
    ex = os.path.join(ROOT, 'examples', 'train_ppo.py')
    r = subprocess.run([sys.executable, ex, '--expert-state', 'theirs'], capture_output=True, text=True)
    assert r.returncode == 2 and "'own', 'flown'" in r.stderr, r.stderr[-400:]
    r = subprocess.run([sys.executable, ex, '--update', 'fused', '--dagger', '1', '--expert-state', 'flown'], capture_output=True, text=True)
    assert r.returncode == 2 and '--expert qp' in r.stderr, r.stderr[-400:]


# ---- S, the thruster state an executed action row leaves ----

def _action_of(qp, x):
    """The action the law commands for the state x [n, 5] (BatchedQPAllocator.allocate's last lines)."""
    s, c = np.sin(x[:, 3:5]).astype(qp.dtype), np.cos(x[:, 3:5]).astype(qp.dtype)
    return np.concatenate([qp.thrust_columns(x[:, 0:3]), np.stack([s[:, 0], c[:, 0], s[:, 1], c[:, 1]], 1)], 1)


def _circle(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_state_from_action_round_trip(dtype):
    """x inside the box |F| <= f_max and inside K * 100^2: S(action_of(x)) = x.  Bounds: F within 4 ulp in float32 (six roundings lie between
    F and its return: /, sqrt, / 100, * 100 and the two products; measured on these 4096 states 4.0 ulp at the worst, 3.8e-6 N on forces up
    to 20.5 N), 1e-12 in float64 (measured 7.1e-15); angles within 1e-6 rad on the circle (measured 2.4e-7), 1e-12 in float64."""
    from ml4ca_amd.deploy import BatchedQPAllocator, qp_state_from_action
    n = 4096
    q = _qp()
    qp = BatchedQPAllocator(n, q, dt=DT, dtype=dtype)
    rng = np.random.RandomState(3)
    cap = np.minimum(np.asarray(q['f_max']), np.minimum(np.asarray(q['kf']), np.asarray(q['kr'])) * 1e4)
    F = rng.uniform(-1.0, 1.0, (n, 3)) * cap * 0.999
    F[np.abs(F) < 1e-3] = 0.5
    al = rng.uniform(-np.pi, np.pi, (n, 2)) * 0.9999
    x = np.concatenate([F, al], 1).astype(dtype)
    got = qp_state_from_action(q, _action_of(qp, x), dtype=dtype)
    assert got.dtype == dtype and got.shape == (n, 5)
    dF, da = np.abs(got[:, 0:3].astype(np.float64) - x[:, 0:3]), _circle(got[:, 3:5], x[:, 3:5])
    print('round trip %s: worst |dF| %.3g N (%.2f ulp), worst angle %.3g rad' % (np.dtype(dtype).name, dF.max(), (dF / np.spacing(np.abs(x[:, 0:3]))).max(), da.max()))
    if dtype == np.float32:
        assert (dF <= 4 * np.spacing(np.abs(x[:, 0:3]))).all() and da.max() <= 1e-6
    else:
        assert dF.max() <= 1e-12 and da.max() <= 1e-12
    assert (got[:, 3:5] >= -np.pi - 1e-6).all() and (got[:, 3:5] < np.pi + 1e-6).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_state_from_action_at_the_edges(dtype):
    from ml4ca_amd.deploy import qp_allocator_table, qp_state_from_action
    q = _qp()
    t = np.dtype(dtype).type
    kf, kr, fmax = (np.asarray(q[k], np.float64).astype(dtype) for k in ('kf', 'kr', 'f_max'))
    base = np.array([[0.25, -0.5, 0.75, 0.6, 0.8, -0.8, 0.6]], dtype)
    # thrust columns past the command range saturate: +-min(K * 1e4, f_max), also where f_max is the smaller
    for fm in (fmax, (fmax * t(0.5)).astype(dtype)):
        for sign, K in ((1.0, kf), (-1.0, kr)):
            a = base.copy()
            a[0, 0:3] = sign * 1.5
            x = qp_state_from_action(dict(q, f_max=fm), a, dtype=dtype)
            assert _same(x[0, 0:3], (t(sign) * np.minimum((K * t(100.0)) * t(100.0), fm)).astype(dtype))
    # in range the thrust law: (K n) |n| with n = 100 a, K by the sign
    x = qp_state_from_action(q, base, dtype=dtype)
    n3 = base[0, 0:3] * t(100.0)
    assert _same(x[0, 0:3], ((np.where(n3 >= 0, kf, kr) * n3) * np.abs(n3)).astype(dtype))
    assert _circle(x[0, 3:5], np.arctan2([0.6, -0.8], [0.8, 0.6])).max() <= (1e-6 if dtype == np.float32 else 1e-12)
    # heads are not normalised by the env and need not be here
    x2 = qp_state_from_action(q, base * np.array([1, 1, 1, 3, 3, 0.25, 0.25], dtype), dtype=dtype)
    assert _circle(x2[0, 3:5], x[0, 3:5]).max() <= (1e-6 if dtype == np.float32 else 1e-12) and _same(x2[0, 0:3], x[0, 0:3])
    # an entry that is not finite: its component is 0, the others are what they were
    for bad in (np.nan, np.inf, -np.inf):
        for col, comp in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (6, 4)):
            a = base.copy()
            a[0, col] = bad
            y = qp_state_from_action(q, a, dtype=dtype)
            keep = [k for k in range(5) if k != comp]
            assert y[0, comp] == 0 and np.isfinite(y).all() and _same(y[0, keep], x[0, keep]), (bad, col)
    a = np.full((1, 7), np.nan, dtype)
    assert (qp_state_from_action(q, a, dtype=dtype) == 0).all()
    # signed-zero head pairs follow np.arctan2: (+-0, +0) -> +-0, (+-0, -0) -> +-pi, which the wrap takes to the same point of the circle
    for s in (0.0, -0.0):
        for c in (0.0, -0.0):
            a = base.copy()
            a[0, 3], a[0, 4] = s, c
            y = qp_state_from_action(q, a, dtype=dtype)
            assert _circle(y[0, 3], np.arctan2(s, c)) <= (1e-6 if dtype == np.float32 else 1e-12) and -np.pi - 1e-6 <= y[0, 3] <= np.pi + 1e-6
            assert y[0, 3] == 0 if not np.signbit(c) else abs(abs(float(y[0, 3])) - np.pi) <= 1e-6
    # a table: row i's numbers on row i
    n = 3
    tab = qp_allocator_table(n, q, f_max=np.asarray(q['f_max'])[None] * np.array([1.0, 0.5, 0.25])[:, None])
    a = np.repeat(base, n, 0)
    a[:, 0:3] = 1.5
    y = qp_state_from_action(tab, a, dtype=dtype)
    for i in range(n):
        assert _same(y[i], qp_state_from_action(dict(q, f_max=tab[6:9, i].astype(np.float64)), a[i:i + 1], dtype=dtype)[0])
    assert not np.array_equal(y[0], y[1])
    with pytest.raises(ValueError):
        qp_state_from_action(q, base[0], dtype=dtype)


# ---- the scan ----

def _flown(seed, T, n):
    """Action rows nobody's law wrote: thrust columns partly past the command range, heads of any length, some entries not finite."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.2, 1.2, (T, n, 7)).astype(np.float32)
    a[2, 1, 0] = np.nan
    a[3, 3, 4] = np.inf
    return a


def _by_hand_flown(p, q, obs, done, z0, x0, flown, dtype):
    """The composition of the header, row by row: wrench, allocate from the state in force, the state the executed row leaves, the resets."""
    from ml4ca_amd.deploy import BatchedDPController, BatchedQPAllocator, qp_state_from_action
    T, n = obs.shape[:2]
    ctrl, qp = BatchedDPController(n, p, dt=DT, dtype=dtype), BatchedQPAllocator(n, q, dt=DT, dtype=dtype)
    ctrl.z = np.ascontiguousarray(z0.T).astype(dtype)
    qp.x = np.ascontiguousarray(x0.T).astype(dtype)
    act = np.zeros((T, n, 7), dtype)
    for t in range(T):
        act[t] = qp.allocate(ctrl.wrench(obs[t]))
        qp.x = qp_state_from_action(q, flown[t], dtype=dtype)
        if done is not None:
            ctrl.reset(done[t] != 0)
            qp.reset(done[t] != 0)
    return act, np.ascontiguousarray(ctrl.z.T), np.ascontiguousarray(qp.x.T)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_label_rows_qp_without_flown_rows_is_unchanged_in_bits(dtype):
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_qp
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block()
    want = _by_hand(p, q, obs, done, z0, x0, dtype)[:3]
    for got in (label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype), label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype, flown=None)):
        assert all(_same(u, v) for u, v in zip(got, want))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_label_rows_qp_flown_is_the_composition_row_by_row(dtype):
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_qp, qp_state_from_action
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block()
    T, n = done.shape
    fl = _flown(1, T, n)
    act, z, x = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype, flown=fl)
    want = _by_hand_flown(p, q, obs, done, z0, x0, fl, dtype)
    assert all(_same(u, v) for u, v in zip((act, z, x), want)) and np.isfinite(act).all()
    own, z_own, _ = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype)
    assert _same(own[0], act[0]) and not np.array_equal(own[1:], act[1:]) and _same(z, z_own)    # row 0 is solved from x_in either way; z does not see x
    # x out is the state the last executed row left, zero behind a done row in the last row
    last = qp_state_from_action(q, fl[T - 1], dtype=dtype)
    last[done[T - 1] != 0] = 0
    assert _same(x, np.ascontiguousarray(last.T)) and (x[:, 1] == 0).all() and (x[:, 0] != 0).any()
    # pieces with z and x handed over equal one call
    a1, z1, x1 = label_rows_qp(p, q, obs[0:4], done[0:4], z0, x0, dt=DT, dtype=dtype, flown=fl[0:4])
    a2, z2, x2 = label_rows_qp(p, q, obs[4:], done[4:], z1, x1, dt=DT, dtype=dtype, flown=fl[4:])
    assert _same(np.concatenate([a1, a2]), act) and _same(z2, z) and _same(x2, x)
    # behind a done row the label is the row alone from z = 0 and thrusters at rest, whatever was flown
    alone, _, _ = label_rows_qp(p, q, obs[1:2, 0:1], None, None, None, dt=DT, dtype=dtype)
    assert _same(alone[0, 0], act[1, 0])
    # row t ignores flown[t:] and depends on flown[t - 1]
    t = 5
    other = fl.copy()
    other[t:] = _flown(2, T, n)[t:]
    b, _, xb = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype, flown=other)
    assert _same(b[:t + 1], act[:t + 1]) and not np.array_equal(b[t + 1], act[t + 1]) and not np.array_equal(xb, x)
    other = fl.copy()
    other[t - 1, 3] = fl[t - 1, 3] * np.float32(0.5)                                    # env 3: no done row near
    c, _, _ = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype, flown=other)
    assert _same(c[:t], act[:t]) and not np.array_equal(c[t, 3], act[t, 3])
    keep = [i for i in range(n) if i != 3]
    assert _same(c[:, keep], act[:, keep])
    with pytest.raises(ValueError):
        label_rows_qp(p, q, obs, done, z0, x0, dt=DT, dtype=dtype, flown=fl[:-1])


@pytest.mark.parametrize('flown', [False, True])
def test_a_qp_table_of_equal_rows_gives_the_scalar_forms_bits_and_refused_rows_rest(flown):
    from ml4ca_amd.deploy import QP_SLOTS, dp_controller_defaults, label_rows_qp, qp_allocator_table, qp_table_refused
    p, q = dp_controller_defaults(), _qp()
    obs, done, z0, x0 = _block(seed=8)
    T, n = done.shape
    fl = _flown(4, T, n) if flown else None
    a = label_rows_qp(p, q, obs, done, z0, x0, dt=DT, flown=fl)
    tab = qp_allocator_table(n, q)
    assert not qp_table_refused(tab, DT).any()
    b = label_rows_qp(p, tab, obs, done, z0, x0, dt=DT, flown=fl, iterations=q['iterations'])
    assert all(_same(u, v) for u, v in zip(a, b))
    c = label_rows_qp(p, tab, obs, done, z0, x0, dt=DT, flown=fl)                      # 16 iterations: another law
    assert not np.array_equal(c[0], a[0])
    with pytest.raises(ValueError):
        label_rows_qp(p, q, obs, done, z0, x0, dt=DT, flown=fl, iterations=4)
    # distinct rows: lane i is the scalar form with row i's numbers
    wp = np.asarray(q['w_power']) * np.linspace(0.25, 4.0, n)
    fm = np.asarray(q['f_max'])[None] * np.linspace(0.5, 1.0, n)[:, None]
    tab2 = qp_allocator_table(n, q, w_power=wp, f_max=fm)
    d = label_rows_qp(p, tab2, obs, done, z0, x0, dt=DT, flown=fl, iterations=q['iterations'])
    for i in (0, 2, n - 1):
        qi = dict(q, w_power=float(np.float32(wp[i])), f_max=tab2[6:9, i].astype(np.float64))
        e = label_rows_qp(p, qi, obs[:, i:i + 1], done[:, i:i + 1], z0[:, i:i + 1], x0[:, i:i + 1], dt=DT, flown=None if fl is None else fl[:, i:i + 1])
        assert _same(d[0][:, i:i + 1], e[0]) and _same(d[2][:, i:i + 1], e[2])
    # refused rows: the mask, and the rest allocator - zero thrust, azimuths held, every output finite; the others are not affected
    bad = tab.copy()
    bad[QP_SLOTS['w_dalpha'][0], 1] = 0.0
    bad[QP_SLOTS['kf'][0] + 2, 3] = np.nan
    bad[QP_SLOTS['force_rate'][0], 4] = 3e38                                           # finite, its product with dt is not
    bad[30, 0] = np.nan                                                                # a reserved slot: not read
    assert qp_table_refused(bad, DT).tolist() == [False, True, False, True, False] and qp_table_refused(bad, 20.0).tolist() == [False, True, False, True, True]
    x00 = x0.copy()
    x00[0:3] = 0                                                                       # forces at rest: the rest allocator's precondition
    g = label_rows_qp(p, bad, obs, done, z0, x00, dt=DT, iterations=q['iterations'])   # own recursion: the azimuths are held along the rows
    ref = label_rows_qp(p, tab, obs, done, z0, x00, dt=DT, iterations=q['iterations'])
    ok = [0, 2]                                                                        # (env 4 is accepted at this dt, with another force rate)
    assert _same(g[0][:, ok], ref[0][:, ok]) and _same(g[2][:, ok], ref[2][:, ok]) and _same(g[1], ref[1])
    assert np.isfinite(g[0]).all() and (g[0][:, [1, 3], 0:3] == 0).all() and (g[2][0:3][:, [1, 3]] == 0).all()
    assert np.allclose(g[0][0, 3, 3:7], [np.sin(x00[3, 3]), np.cos(x00[3, 3]), np.sin(x00[4, 3]), np.cos(x00[4, 3])], atol=1e-6)
    assert _same(g[0][1, 3, 3:7], g[0][0, 3, 3:7])                                     # ... held: env 3 has no done row before row 6
    if flown:
        h = label_rows_qp(p, bad, obs, done, z0, x00, dt=DT, iterations=q['iterations'], flown=fl)
        assert np.isfinite(h[0]).all() and (h[0][:, [1, 3], 0:3] == 0).all() and (h[2][0:3][:, [1, 3]] == 0).all()    # f_max = 0: S leaves no force


def test_flown_labels_on_a_qp_closed_loop_of_the_float64_oracle_agree_with_its_rows():
    """The float64 host chain (K = 16) flies the float64 oracle with auto-reset; label_rows_qp on the recorded rows with flown = the
    flight's own act rows, in float64, agrees with those rows: the state read back from an action row differs from the carried one by
    rounding alone (3.6e-15), and the float64 solver does not amplify it past 1e-6.  Measured on this flight (n = 16, T = 60, K = 16):
    worst |label - flown row| 3.01e-08 in float64.  The bound is 10 x that.  The float32 figure on the same flight, recorded and not
    asserted: 2.2e-03 (the accept / reject turns amplify a 2-ulp change of the state; a synthetic 256 x 40 block gave 2.4e-2)."""
    from ml4ca_amd.deploy import BatchedDPController, BatchedQPAllocator, dp_controller_defaults, label_rows_qp
    from oracle import oracle as O
    n, T = 16, 60
    p, q = dp_controller_defaults(), _qp(16)
    worst = {}
    for dtype in (np.float64, np.float32):
        orc = O.Oracle(O.make_config(terminate=1, auto_reset=1, max_ep_len=25, seed=9), np.float64)
        state, ctr = orc.new_state(n)
        obs = orc.reset(state, ctr)
        ctrl, qp = BatchedDPController(n, p, dt=DT, dtype=dtype), BatchedQPAllocator(n, q, dt=DT, dtype=dtype)
        rows, acts, dones = np.zeros((T, n, 9), dtype), np.zeros((T, n, 7), dtype), np.zeros((T, n), np.uint8)
        for t in range(T):
            rows[t] = np.asarray(obs, dtype)
            a = qp.allocate(ctrl.wrench(rows[t]))
            acts[t] = a
            obs, _, d = orc.step(state, ctr, a.astype(np.float64))
            dones[t] = d
            ctrl.reset(d != 0)
            qp.reset(d != 0)
        assert (dones[1:T - 1] != 0).any(0).all() and np.isfinite(acts).all()
        own, _, _ = label_rows_qp(p, q, rows, dones, None, None, dt=DT, dtype=dtype)
        assert _same(own, acts)                                                        # the own recursion IS the flight
        got, _, x = label_rows_qp(p, q, rows, dones, None, None, dt=DT, dtype=dtype, flown=acts)
        worst[dtype] = float(np.abs(got - acts).max())
        assert (x != 0).any()
    print('flown labels vs the flight: float64 %.3g, float32 %.3g' % (worst[np.float64], worst[np.float32]))
    assert worst[np.float64] <= 10 * 3.01e-08
