"""The step kernels at the edges of their inputs (-m gpu): the tables of tests/step_edges.py through every single-step kernel that holds
its own copy of the step (the general step_kernel - asked for the reward parts -, the lean kernel - another sub-step count -, the fixed
kernel - the shipped 20 sub-steps) against the FLOAT64 oracle on the float32 inputs, with the comparison of test_gpu_parity.compare and
the floors of tests/tolerances.py (step_edges.judge: a row on a jump of the reference law may take either side, with everything it has).
tests/test_step_edges_cpu.py shows that the float32 oracle holds every one of these rows within half the tolerance.

Which kernel serves a launch is dev::launch_step's rule (reward parts -> general; else 20 sub-steps and a live plant -> fixed; else lean):
the library has no query for it, so each path is pinned by the inputs of that rule, which tests/test_gpu_step_fixed.py and
tests/test_gpu_step_lean.py hold bit for bit against the general body.

Per-quantity worst ratios error / tolerance are printed, and appended to the file the environment variable STEP_EDGES_RECORD names, if it is
set (profiles/step_edges_parity.txt is such a record).
"""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import step_edges as SE
from tests import tolerances as TOL

pytestmark = pytest.mark.gpu
RECORD = os.environ.get('STEP_EDGES_RECORD')
PATHS = {'general': dict(parts=True, n_steps=None), 'lean': dict(parts=False, n_steps=7), 'fixed': dict(parts=False, n_steps=None)}
LEAN_SUBSTEPS = 7
_truth = {}


def torch_():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def make_env(t, path):
    kw = dict(t.kw)
    if PATHS[path]['n_steps']:
        kw['n_steps'] = PATHS[path]['n_steps']
    env, _ = H.make_pair(t.mode, t.n, ext=t.ext, **kw)
    # the inputs of dev::launch_step's rule that the handle decides (the reward parts are gpu_step's)
    assert env.layout == 'aos' and env.n_steps == (LEAN_SUBSTEPS if path == 'lean' else 20) and not env.auto_reset
    assert env.obs_torch_dtype == torch_().float32 and not kw.get('current') and not kw.get('vessel_params') and not kw.get('hold_plant')
    return env


def gpu_step(env, t, path, st=None, act=None):
    torch = torch_()
    env.set_state(H.to_dev(t.st if st is None else st), H.to_dev(t.ctr))
    parts = torch.zeros((4, t.n), device=env.device) if PATHS[path]['parts'] else None
    obs, rew, done, _ = env.step(H.to_dev(t.act if act is None else act), reward_parts=parts)
    st2, ctr2 = env.get_state()
    torch.cuda.synchronize()
    g = dict(obs=obs.cpu().numpy(), rew=rew.cpu().numpy(), done=done.cpu().numpy(), st=st2.cpu().numpy(), ctr=ctr2.cpu().numpy())
    if parts is not None:
        g['parts'] = parts.cpu().numpy().T
    return g


def truth(key, t, n_substeps, steps=1):
    """float64 truth (and its neighbour variants) of a table: computed once, shared, never written to"""
    k = (key, n_substeps, steps)
    if k not in _truth:
        _truth[k] = SE.truth_variants(SE.make_oracle(t.mode, t.ext, np.float64, t.kw, n_substeps), t, steps)
    return _truth[k]


def check_parity(g_steps, variants, t, od, title):
    rows = SE.parity_rows(t)
    report, bad = SE.judge(g_steps, variants, t, od, rows)
    print(title, sorted(report.items()))
    SE.record(RECORD, 'HIP kernel / float64 oracle: ' + title, report)
    assert bad.size == 0, '%s: %d rows outside the tolerance: %s' % (title, bad.size, '; '.join(
        SE.describe(t, i) + ' got obs %r reward %r state %r want obs %r reward %r state %r' % (
            g_steps[-1]['obs'][i].tolist(), float(g_steps[-1]['rew'][i]), g_steps[-1]['st'][:, i].tolist(),
            variants[0][-1]['obs'][i].tolist(), float(variants[0][-1]['rew'][i]), variants[0][-1]['st'][:, i].tolist()) for i in bad[:3]))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_fold_rows(g, o, t, pre_st):
    """|psi| > 30000, beyond what sincos_lean promises accuracy for: finite, a rotation that keeps lengths (4 float32 ulp), and - the
    plant integrating body velocities through that rotation - a displacement of the oracle's length"""
    far = ~SE.parity_rows(t)
    if not far.any():
        return
    for k in ('obs', 'rew', 'st'):
        assert np.isfinite(g[k][far] if k != 'st' else g[k][:, far]).all(), k
    assert (g['done'][far] == 0).all()
    st = g['st'][:, far]
    dN, dE = (st[0] - st[6]).astype(np.float64), (st[1] - st[7]).astype(np.float64)          # float32 differences, as the kernel forms them
    x, y = g['obs'][far, 0].astype(np.float64), g['obs'][far, 1].astype(np.float64)
    lhs, rhs = x * x + y * y, dN * dN + dE * dE
    assert (np.abs(lhs - rhs) <= 4 * ulp32(np.maximum(lhs, rhs))).all(), (lhs, rhs)
    moved = np.hypot(st[0].astype(np.float64) - pre_st[0, far], st[1].astype(np.float64) - pre_st[1, far])
    want = np.hypot(o['st'][0, far] - pre_st[0, far], o['st'][1, far] - pre_st[1, far])
    # each of N, E within its parity tolerance (1e-5 * ETA_FLOOR) and the rotation's 4 ulp on a displacement of ~0.1 m
    assert (np.abs(moved - want) <= 2 * TOL.RTOL_F32 * TOL.ETA_FLOOR[0]).all(), (moved, want)


# ------------------------------------------------------------------------------------------------------------------------------
# A. action decode
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('mode,ext', SE.ALL_CASES)
def test_action_decode_edges(mode, ext, path):
    t = SE.padded(SE.table_a(mode, ext), SE.moving_state(mode), SE.mid_action(mode))
    env = make_env(t, path)
    g = gpu_step(env, t, path)
    check_parity([g], truth(('A', mode, ext), t, env.n_steps), t, 9 if ext else 6, 'A %s ext=%d %s' % (mode, ext, path))


@pytest.mark.parametrize('path', sorted(PATHS))
def test_zero_heads_push_where_the_reference_pushes(path):
    """full port thrust from rest: the surge after one step has the sign of the cos head's zero, the azimuth is arctan2's"""
    t = SE.zero_head_fact_rows()
    g = gpu_step(make_env(t, path), t, path)
    u, az = g['st'][3, :4], g['st'][13, :4]
    scale = LEAN_SUBSTEPS / 20.0 if path == 'lean' else 1.0
    assert (np.sign(u) == [1, -1, -1, 1]).all() and (np.abs(np.abs(u) - 0.01552 * scale) < 1e-4).all(), u
    assert az[0] == 0 and az[3] == 0 and abs(az[1] - np.pi) < 1e-6 and abs(az[2] + np.pi) < 1e-6, az


@pytest.mark.parametrize('path', sorted(PATHS))
def test_heads_outside_the_supported_range_stay_finite(path):
    """include/dpenv.h: max(|s|, |c|) at 2^-70 and 2^70 - finite outputs, no fault bit, nothing more"""
    t = SE.padded(SE.table_a_out_of_range(), SE.moving_state('final_cont'), SE.mid_action('final_cont'), total=1024 + 37)
    g = gpu_step(make_env(t, path), t, path)
    for k in ('obs', 'rew', 'st'):
        assert np.isfinite(g[k]).all(), k
    assert (g['done'] == 0).all()
    # the ordinary rows between them are the ordinary rows of table A
    pad = t.tag == 'pad'
    for k in ('obs', 'rew'):
        assert (g[k][pad] == g[k][pad][0]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# B. heading and wrap
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('wrap_mode', ['reference', 'radians'])
def test_heading_and_wrap_edges(wrap_mode, path):
    t = SE.padded(SE.table_b(wrap_mode), SE.moving_state('final_cont'), SE.mid_action('final_cont'))
    env = make_env(t, path)
    g = gpu_step(env, t, path)
    v = truth(('B', wrap_mode), t, env.n_steps)
    check_parity([g], v, t, 9, 'B %s %s' % (wrap_mode, path))
    check_fold_rows(g, v[0][0], t, t.st.astype(np.float64))


@pytest.mark.parametrize('wrap_mode', ['reference', 'radians'])
def test_heading_and_wrap_edges_through_the_fused_rollout(wrap_mode):
    """three steps of dpenv_rollout from the edge states against three oracle steps: the carried sin / cos goes through the re-evaluation
    behind a fired wrap inside a fused kernel.  Every step is held to the single-step tolerance."""
    torch = torch_()
    t = SE.padded(SE.table_b(wrap_mode), SE.moving_state('final_cont'), SE.mid_action('final_cont'))
    env = make_env(t, 'fixed')
    env.set_state(H.to_dev(t.st), H.to_dev(t.ctr))
    acts = H.to_dev(np.ascontiguousarray(np.broadcast_to(t.act, (3,) + t.act.shape)))
    obs, rew, done = env.rollout(acts)
    st2, ctr2 = env.get_state()
    torch.cuda.synchronize()
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    g = [dict(obs=obs[k], rew=rew[k], done=done[k], st=st2.cpu().numpy(), ctr=ctr2.cpu().numpy()) for k in range(3)]
    v = truth(('B', wrap_mode), t, 20, steps=3)
    check_parity(g, v, t, 9, 'B %s fused rollout, 3 steps' % wrap_mode)
    far = ~SE.parity_rows(t)
    assert np.isfinite(obs[:, far]).all() and np.isfinite(rew[:, far]).all() and np.isfinite(g[-1]['st'][:, far]).all() and (done[:, far] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# C. termination bounds
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['general', 'lean'])
@pytest.mark.parametrize('mode,ext', SE.ALL_CASES)
def test_termination_bounds(mode, ext, path):
    """plant held, psi = 0 (or no position error), setpoint 0: the observation is the state bit for bit, and the done bits are the float32
    oracle's on the same pose - at every bound, one ulp above, one below, both signs"""
    t = SE.table_c(mode, ext)
    kw = dict(t.kw)
    env, _ = H.make_pair(mode, t.n, ext=ext, **kw)
    assert env.n_steps == 20
    g = gpu_step(env, t, path)
    o = SE.oracle_steps(SE.make_oracle(mode, ext, np.float32, t.kw), t)[0]
    assert np.array_equal(g['done'], o['done']), (g['done'], o['done'])
    at, above, below = (o['done'][t.tag == k] for k in ('at_bound', 'above_bound', 'below_bound'))
    assert (above == 1).all() and (at == 0).all() and (below == 0).all() and o['done'][0] == 0      # strict >: the table really straddles every bound
    want = np.ascontiguousarray(t.st[0:6].T)
    level = t.st[2] == 0                   # sincos_lean(0) is exactly (0, 1): bit for bit; a heading AT its bound rotates a zero position error, whose zero may come out signed
    assert g['obs'][level, :6].tobytes() == want[level].tobytes() and np.array_equal(g['obs'][:, :6], want), 'observation is not the state'
    assert g['st'][0:6].tobytes() == t.st[0:6].tobytes(), 'a held plant moved'


# ------------------------------------------------------------------------------------------------------------------------------
# D. force map
# ------------------------------------------------------------------------------------------------------------------------------
def test_force_map_edges():
    """ml4ca_amd.thrust_map, one thruster at a time at +-100 %.  |alpha| <= 30000: |tau_x - F cos alpha|, |tau_y - F sin alpha| <= F * 9.2e-8
    (the bound dpenv_env_dev.h states for sincos_lean, from tools/lean_math_check.py) plus two roundings of F; beyond: finite, and
    tau_x^2 + tau_y^2 = F^2 within 4 float32 ulp."""
    import ml4ca_amd
    torch_()
    n_pct, alpha, which = SE.table_d()
    tau = ml4ca_amd.thrust_map(H.to_dev(n_pct), H.to_dev(alpha)).cpu().numpy().astype(np.float64)
    assert np.isfinite(tau).all()
    v = np.asarray(ml4ca_amd.default_vessel(), np.float32)
    cols = np.arange(n_pct.shape[1])
    n = n_pct[which, cols]
    a = alpha[which, cols].astype(np.float64)
    K = np.where(n >= 0, v[12:15][which], v[15:18][which]).astype(np.float32)
    F = ((K * np.abs(n)) * n).astype(np.float64)              # float32 products in the kernel's order: F itself carries no error
    lx, ly = v[18:21][which].astype(np.float64), v[21:24][which].astype(np.float64)
    near = np.abs(a) <= SE.FOLD
    tol = np.abs(F) * 9.2e-8 + 2 * 0.5 * ulp32(F)
    ex, ey = np.abs(tau[0] - F * np.cos(a)), np.abs(tau[1] - F * np.sin(a))
    worst = max(float((ex / tol)[near].max()), float((ey / tol)[near].max()))
    print('force map: worst |error| / (F 9.2e-8 + 2 roundings) =', worst, 'worst |error| / F =', float((np.maximum(ex, ey) / np.abs(F))[near].max()))
    SE.record(RECORD, 'HIP thrust_map / float64, |alpha| <= 30000', {'tau_x, tau_y error / (F 9.2e-8 + 2 roundings of F)': worst})
    assert ((ex <= tol) | ~near).all() and ((ey <= tol) | ~near).all(), (alpha[which, cols][near & ((ex > tol) | (ey > tol))], worst)
    # the moment: (lx sin - ly cos) F, the same two errors weighted by the lever arms, and three more roundings
    en = np.abs(tau[2] - (lx * np.sin(a) - ly * np.cos(a)) * F)
    assert ((en <= (np.abs(lx) + np.abs(ly)) * tol + 3 * ulp32((np.abs(lx) + np.abs(ly)) * F)) | ~near).all()
    lhs, rhs = tau[0] ** 2 + tau[1] ** 2, F * F
    assert (np.abs(lhs - rhs) <= 4 * ulp32(np.maximum(lhs, rhs)))[~near].all(), (lhs[~near], rhs[~near])


# ------------------------------------------------------------------------------------------------------------------------------
# non-finite rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,ext', SE.ALL_CASES)
def test_non_finite_rows_fault_alone(mode, ext):
    """NaN, +Inf, -Inf in each action component and each pose / velocity component, one row each: those rows carry DONE_FAULT | DONE_TERMINAL,
    and every other row of the launch - their neighbours in the same wave - is what it is without them, bit for bit.  All three kernels."""
    clean, bad, idx = SE.poisoned(mode, ext)
    ok = np.ones(clean.n, bool)
    ok[idx] = False
    for path in sorted(PATHS):
        env = make_env(clean, path)
        want = gpu_step(env, clean, path)
        got = gpu_step(env, bad, path)
        fault = SE.DONE_FAULT | SE.DONE_TERMINAL
        assert (got['done'][idx] & fault == fault).all(), (path, got['done'][idx])
        assert not (got['done'][ok] & SE.DONE_FAULT).any()
        for k in sorted(want):
            a, b = (got[k][:, ok], want[k][:, ok]) if k in ('st', 'ctr') else (got[k][ok], want[k][ok])
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (path, k)
