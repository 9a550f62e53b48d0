"""The in-kernel actor-critic at the edges of its inputs (-m gpu): dpenv_policy_forward and dpenv_policy_rollout on the cases of
tests/policy_edges.py against the FLOAT64 evaluation of the float32 parameters (oracle/policy_ref.py).

THE BOUNDS.  Per output tensor, S = max |float64| of that tensor:
  range / small batches   |kernel - float64| <= max(2 |split_model - float64|_max, K 2^-24 max(S, 1)), K = (16 + 1) + 3 (80 + 1) the fma
                          chain to an output as tests/test_gpu_ppo_update.py counts it, 2 its allowance for another summation order:
                          the kernel is pinned to the arithmetic include/dpenv.h states, whatever the case; and inside the header's
                          domain (policy_edges.domain) also <= C max(S, 1), C = 1e-5 (F32) / 2e-3 (F16).
  log_std ends            max(8 |torch-float32 - float64|, K' 2^-24 S'), the yardstick of tests/test_gpu_ppo_update.py; for logp
                          K' = K + 14 and S' = max_i sum_k (z_k^2 / 2 + |logp_const_k|), the sizes of the summed terms.
  isolation / shards      bit for bit.
tests/test_policy_edges_cpu.py holds what these lean on.  Every measured figure is printed, and appended to the file the environment
variable POLICY_EDGES_RECORD names, if it is set (DESIGN.md holds such a record)."""
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import policy_edges as PE

pytestmark = pytest.mark.gpu
RECORD = os.environ.get('POLICY_EDGES_RECORD', '')
DEV = 'cuda:0'
PE_CLIP = 0.2
BLOCKS = ('obs', 'act', 'rew', 'val', 'logp', 'done', 'boot', 'last_obs', 'last_val')


def torch_():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def forward(env, ac, obs, precision):
    from ml4ca_amd.policy import policy_forward
    ac.upload(env, precision=precision)
    mu, v = policy_forward(env, obs)
    return host(mu), host(v)


def check_forward(tag, ev, got, case, activation, precision):
    """the range bound (and, in the domain, the header's constant) for mu and v of one launch; every figure recorded before any assertion"""
    fails = []
    for j, name in enumerate(('mu', 'v')):
        tp = PE.tensor_precision(precision, j)
        ref = ev['ref'][j]
        S = PE.scale_of(ref)
        e, m, y = PE.err(got[j], ref), PE.err(ev['model'][tp][j], ref), PE.err(ev['y32'][j], ref)
        bound = PE.range_bound(ev, tp, j)
        inside = PE.domain(case, activation, tp)
        PE.record(RECORD, '%s %-9s %-5s %-9s %-2s kernel %.3e  model %.3e  y32 %.3e  bound %.3e  C*S %s' % (
            tag, case, activation, precision, name, e, m, y, bound, ('%.3e' % (PE.C[tp] * S)) if inside else 'outside'))
        if not e <= bound:
            fails.append((name, 'bound', e, bound))
        if inside and not e <= PE.C[tp] * S:
            fails.append((name, 'C', e, PE.C[tp] * S))
    assert not fails, (tag, case, activation, precision, fails)


# ------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize('activation', PE.ACTIVATIONS)
@pytest.mark.parametrize('case', PE.RANGE_CASES)
def test_forward_over_the_range_of_observations_and_weights(case, activation):
    """dpenv_policy_forward in F16, F32 and F32_ACTOR on 97 rows of every case below the overflow.  F32_ACTOR: mu is F32's bit for bit,
    v is F16's bit for bit."""
    ev = PE.evaluate(case, activation)
    env, _ = H.make_pair('final_cont', PE.N_ROWS, terminate=False)
    ac = PE.make_ac(activation, PE.CASES[case][1], device=DEV)
    obs = dev(ev['obs'])
    got = {p: forward(env, ac, obs, p) for p in PE.PRECISIONS}
    for p in PE.PRECISIONS:
        check_forward('range ', ev, got[p], case, activation, p)
    assert got['f32_actor'][0].tobytes() == got['f32'][0].tobytes()
    assert got['f32_actor'][1].tobytes() == got['f16'][1].tobytes()
    assert got['f32'][0].tobytes() != got['f16'][0].tobytes()


# ------------------------------------------------------------------------------------------------ the log_std clamp ends
def _rollout_rows(form, precision, T=3):
    from ml4ca_amd.policy import policy_rollout, policy_launch_form
    n = PE.N_ROWS
    env, _ = H.make_pair('final_cont', n, terminate=False, seed=5)
    ac = PE.make_ac('leaky', 1.0, device=DEV, log_std=PE.LOG_STD_ENDS).upload(env, precision=precision, launch_form=form)
    assert policy_launch_form(env)[0] == form
    env.reset()
    xi = PE.ends_noise(T, n)
    out = policy_rollout(env, T, noise=dev(xi))
    rows = {k: host(out[k]) for k in ('obs', 'act', 'val', 'logp')}
    return ac, xi.reshape(T * n, 7), rows['obs'].reshape(T * n, 9), rows['act'].reshape(T * n, 7), rows['val'].reshape(-1), rows['logp'].reshape(-1)


def _ends_figures(tag, ac, xi, obs, act, val, logp, precision):
    """(figure, bound) of act, val, logp of a launch on its own obs rows, and of the update statistics of dpenv_ppo_actor_grad on the same
    rows with the same parameters: [(name, figure, bound)]"""
    import torch
    from ml4ca_amd import train as TR
    p = PE.params('leaky')
    p = dict(p, **{'pi/log_std': np.asarray(PE.LOG_STD_ENDS, np.float32)})
    ls = p['pi/log_std'].astype(np.float64)
    mu64, v64 = PE.ref64(p, obs, 'leaky')
    mu32, v32 = PE.y32(p, obs, 'leaky')
    act64 = mu64 + np.exp(ls) * xi.astype(np.float64)
    with torch.no_grad():
        act32 = (torch.from_numpy(mu32).float() + torch.exp(torch.from_numpy(p['pi/log_std'])) * torch.from_numpy(xi)).double().numpy()
    lp64, lp32 = PE.logp64(p, obs, act, 'leaky'), PE.logp32(p, obs, act, 'leaky')
    floor = PE.K_FORWARD * 2.0 ** -24
    figs = [('act', PE.err(act, act64), max(8.0 * PE.err(act32, act64), floor * PE.scale_of(act64)))]
    if PE.tensor_precision(precision, 1) == 'f32':
        figs.append(('val', PE.err(val, v64), max(8.0 * PE.err(v32, v64), floor * PE.scale_of(v64))))
    else:
        vm = PE.split_model(p, obs, 'leaky', PE.LEAK['leaky'], 'f16')[1]
        figs.append(('val', PE.err(val, v64), max(2.0 * PE.err(vm, v64), floor * PE.scale_of(v64))))
    figs.append(('logp', PE.err(logp, lp64), max(8.0 * PE.err(lp32, lp64), PE.K_LOGP * 2.0 ** -24 * PE.logp_scale(act, mu64, ls))))
    # the first gradient step of an update on these rows: the ratio exp(logp_new - logp_old) starts at 1
    theta = TR.flatten([w for w in ac.pi_W], [b for b in ac.pi_b], ac.log_std).contiguous()
    adv = np.random.RandomState(7).standard_normal(obs.shape[0]).astype(np.float32)
    out = TR.ppo_actor_grad(theta, dev(obs), dev(act), dev(adv), dev(logp), PE_CLIP, leak=PE.LEAK['leaky'])
    pi_loss, kl, clip_frac, mean_ratio = (float(x) for x in host(out[-4:]))
    yard = 8.0 * float(np.abs(np.expm1(lp32 - lp64)).max())
    # the float64 law of the update (train.ppo_actor_grad_ref) on its own log-likelihood of these actions: the reference ratio is exactly 1
    lk = float(np.float32(PE.LEAK['leaky']))
    _, _, ls_r, _, _, mu_r = TR._forward64(host(theta), obs, PE.OBS_DIM, PE.ACT_DIM, True, lk)
    q = (act.astype(np.float64) - mu_r) / (np.exp(ls_r) + 1e-8)
    lp_r = (-0.5 * ((q * q + 2.0 * ls_r) + math.log(2.0 * math.pi))).sum(1)
    _, stats_r, _, ratio = TR.ppo_actor_grad_ref(host(theta), obs, act, adv, lp_r, PE_CLIP, leak=lk, hidden_z=True)
    assert (ratio == 1.0).all() and stats_r[2] == 0.0 and stats_r[3] == 1.0
    assert PE.err(lp_r, lp64) <= 1e-6 * PE.logp_scale(act, mu64, ls)      # the two float64 statements differ in float32(1e-8) against 1e-8 only
    figs += [('clip_frac', clip_frac, 0.0), ('mean_ratio-1', abs(mean_ratio - 1.0), yard), ('approx_kl', abs(kl), yard)]
    for name, f, b in figs:
        PE.record(RECORD, '%s %-9s %-12s kernel %.3e  bound %.3e' % (tag, precision, name, f, b))
    return figs


@pytest.mark.parametrize('precision', ['f32', 'f32_actor'])
@pytest.mark.parametrize('form', ['one_wave', 'two_wave'])
def test_rollout_rows_at_the_log_std_clamp_ends_start_the_ppo_ratio_at_one(form, precision):
    """log_std = (-4, -4, -2, 0, 1, 1, -0.5), the ends of the clamp of examples/train_ppo.py, noise with xi = 0 exactly, xi = +-5 and ordinary
    draws, T = 3: act, val and logp of the launch against float64 on its own obs rows (at std = e^-4 an error of mu is 55 x as large in z),
    then the same rows through dpenv_ppo_actor_grad with the same parameters: no row is clipped, mean_ratio - 1 and approx_kl are within
    8 x the largest |exp(logp32 - logp64) - 1| of a torch float32 evaluation of the same actions."""
    figs = _ends_figures('logstd %s' % form, *_rollout_rows(form, precision), precision=precision)
    bad = [(name, f, b) for name, f, b in figs if not f <= b]
    assert not bad, (form, precision, bad)


@pytest.mark.parametrize('form', ['one_wave', 'two_wave'])
def test_f16_rows_at_the_log_std_clamp_ends_are_recorded(form):
    """The same in F16: RECORDED, not asserted - its ratio is known to be off at small std, which is why F32_ACTOR exists.  Only the launch's
    own consistency is required: finite rows."""
    figs = _ends_figures('logstd %s' % form, *_rollout_rows(form, 'f16'), precision='f16')
    assert all(np.isfinite(f) for _, f, _ in figs)


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize('activation', PE.ACTIVATIONS)
def test_forward_rows_past_the_f16_range_are_non_finite_alone(activation):
    """`overflow` (rows 0, 31, 32, 63, 64, 96 x 2^14: an input past f16's range in each) against the same batch with those rows zeroed:
    every clean row is the same bit for bit in all three precisions - the other 31 columns of the MFMA tile are untouched - and the
    poisoned rows are non-finite exactly where the documented arithmetic is."""
    ev = PE.evaluate('overflow', activation)
    bad = list(PE.POISONED)
    clean = np.setdiff1d(np.arange(PE.N_ROWS), bad)
    zeroed = ev['obs'].copy()
    zeroed[bad] = 0.0
    env, _ = H.make_pair('final_cont', PE.N_ROWS, terminate=False)
    ac = PE.make_ac(activation, 1.0, device=DEV)
    for p in PE.PRECISIONS:
        mu, v = forward(env, ac, dev(ev['obs']), p)
        mu0, v0 = forward(env, ac, dev(zeroed), p)
        mm, vm = ev['model'][p]
        PE.record(RECORD, 'overflow %-5s %-9s poisoned rows finite: mu kernel %d model %d of 42, v kernel %d model %d of 6' % (
            activation, p, int(np.isfinite(mu[bad]).sum()), int(np.isfinite(mm[bad]).sum()), int(np.isfinite(v[bad]).sum()),
            int(np.isfinite(vm[bad]).sum())))
        assert mu[clean].tobytes() == mu0[clean].tobytes() and v[clean].tobytes() == v0[clean].tobytes(), (activation, p)
        assert np.isfinite(mu0).all() and np.isfinite(v0).all()
        assert np.array_equal(np.isfinite(mu[bad]), np.isfinite(mm[bad])), (activation, p, mu[bad], mm[bad])
        assert np.array_equal(np.isfinite(v[bad]), np.isfinite(vm[bad])), (activation, p, v[bad], vm[bad])


def _launch(env, st, ctr, T):
    from ml4ca_amd.policy import policy_rollout
    env.set_state(st.clone(), ctr.clone())
    out = policy_rollout(env, T)
    st2, ctr2 = env.get_state()
    g = {k: host(out[k]) for k in BLOCKS}
    g['st'], g['ctr'] = host(st2), host(ctr2)
    return g


@pytest.mark.parametrize('precision', ['f16', 'f32'])
@pytest.mark.parametrize('form', ['one_wave', 'two_wave'])
@pytest.mark.parametrize('n', [97, 257])
def test_rollout_env_a_thousand_kilometres_off_is_alone_with_it(n, form, precision):
    """One env at a time - lanes 0, 31, 32, 63, 64 and n - 1 - is put 2^20 m north of its setpoint (dpenv_set_state; terminate = False, the
    headline configuration): its observation leaves f16's range and its rows are what they are.  Every block of every OTHER env (obs, act,
    rew, val, logp, done, boot, last_obs, last_val) and its final state equal the clean launch bit for bit: neither the other columns of
    its MFMA tile, nor the other tile of its wave, nor - in the two-wave form - the partner wave."""
    from ml4ca_amd.policy import policy_launch_form
    from ml4ca_amd import _lib
    T = 3
    env, _ = H.make_pair('final_cont', n, terminate=False, seed=9)
    PE.make_ac('leaky', 1.0, device=DEV).upload(env, precision=precision, launch_form=form)
    assert policy_launch_form(env)[0] == form
    env.reset()
    st0, ctr0 = env.get_state()
    st0, ctr0 = st0.clone(), ctr0.clone()
    want = _launch(env, st0, ctr0, T)
    assert all(np.isfinite(want[k]).all() for k in BLOCKS if k != 'done')
    for lane in (0, 31, 32, 63, 64, n - 1):
        st = st0.clone()
        st[_lib.S['N'], lane] = st[_lib.S['REF_N'], lane] + 2.0 ** 20
        got = _launch(env, st, ctr0, T)
        others = np.arange(n) != lane
        assert not np.isfinite(got['act'][:, lane]).all(), lane          # the env itself did leave the range
        for k in sorted(want):
            ax = 0 if k in ('last_obs', 'last_val') else 1               # the env axis of the block
            a, b = np.compress(others, got[k], axis=ax), np.compress(others, want[k], axis=ax)
            assert a.tobytes() == b.tobytes(), (n, form, precision, lane, k)


# ------------------------------------------------------------------------------------------------ small batches
@pytest.mark.parametrize('activation', PE.ACTIVATIONS)
@pytest.mark.parametrize('n', [1, 31, 33, 65])
def test_forward_small_batches(n, activation):
    """n = 1, one lane short of a tile, one lane into the second tile, one lane into the second wave: `nominal` with the range test's bounds"""
    ev = PE.evaluate('nominal', activation, n)
    env, _ = H.make_pair('final_cont', n, terminate=False)
    ac = PE.make_ac(activation, 1.0, device=DEV)
    for p in PE.PRECISIONS:
        got = forward(env, ac, dev(ev['obs']), p)
        assert got[0].shape == (n, 7) and got[1].shape == (n,)
        check_forward('small %2d' % n, ev, got, 'nominal', activation, p)


@pytest.mark.parametrize('n', [1, 31, 33, 65])
def test_rollout_small_batches(n):
    """dpenv_policy_rollout of n envs, T = 1 and T = 2, both launch forms, F16 and F32, deterministic: act = mu, val and last_val against
    float64 on the launch's own obs rows with the range test's bounds (the documented arithmetic evaluated on those rows), logp the
    constant sum within K' 2^-24 S'."""
    from ml4ca_amd.policy import policy_rollout, policy_launch_form
    p = PE.params('leaky')
    ls = p['pi/log_std'].astype(np.float64)
    fails = []
    for form in ('one_wave', 'two_wave'):
        for prec in ('f16', 'f32'):
            env, _ = H.make_pair('final_cont', n, terminate=False, seed=13)
            PE.make_ac('leaky', 1.0, device=DEV).upload(env, precision=prec, launch_form=form)
            assert policy_launch_form(env)[0] == form
            for T in (1, 2):
                env.reset()
                out = {k: host(v) for k, v in policy_rollout(env, T).items()}
                assert out['obs'].shape == (T, n, 9) and out['last_obs'].shape == (n, 9)
                obs = np.concatenate([out['obs'].reshape(T * n, 9), out['last_obs']])
                act, val = out['act'].reshape(T * n, 7), np.concatenate([out['val'].reshape(-1), out['last_val']])
                mu64, v64 = PE.ref64(p, obs, 'leaky')
                mm, vm = PE.split_model(p, obs, 'leaky', PE.LEAK['leaky'], prec)
                floor = PE.K_FORWARD * 2.0 ** -24
                lp64 = PE.logp64(p, obs[:T * n], act, 'leaky')
                figs = [('act', PE.err(act, mu64[:T * n]), max(2.0 * PE.err(mm, mu64), floor * PE.scale_of(mu64)), PE.C[prec] * PE.scale_of(mu64)),
                        ('val', PE.err(val, v64), max(2.0 * PE.err(vm, v64), floor * PE.scale_of(v64)), PE.C[prec] * PE.scale_of(v64))]
                if prec == 'f32':
                    b = PE.K_LOGP * 2.0 ** -24 * PE.logp_scale(act, mu64[:T * n], ls)
                    figs.append(('logp', PE.err(out['logp'].reshape(-1), lp64), b, b))
                for name, e, b, c in figs:
                    PE.record(RECORD, 'small %2d rollout T=%d %-8s %-3s %-4s kernel %.3e  bound %.3e  C*S %.3e' % (n, T, form, prec, name, e, b, c))
                    if not (e <= b and e <= c):
                        fails.append((form, prec, T, name, e, b, c))
    assert not fails, fails


@pytest.mark.parametrize('precision', ['f16', 'f32'])
@pytest.mark.parametrize('form', ['one_wave', 'two_wave'])
def test_rollout_of_97_envs_equals_its_shards_of_64_and_33(form, precision):
    """One launch of 97 envs (in-kernel noise, auto-reset) against two launches of its first 64 and its last 33 envs with env_id_base moved:
    every row is the same bit for bit - what an env computes does not depend on which lane, tile or wave it sits in."""
    from ml4ca_amd.policy import policy_rollout
    T = 3
    kw = dict(seed=21, auto_reset=True, max_ep_len=12, terminate=False)

    def run(base, cnt):
        env, _ = H.make_pair('final_cont', cnt, env_id_base=base, **kw)
        PE.make_ac('leaky', 1.0, device=DEV).upload(env, precision=precision, launch_form=form)
        env.reset()
        return {k: host(v) for k, v in policy_rollout(env, T, sample=True).items()}

    whole, parts = run(0, 97), [run(0, 64), run(64, 33)]
    assert np.abs(whole['act']).max() > 0 and np.isfinite(whole['logp']).all()
    for k in BLOCKS:
        ax = 0 if k in ('last_obs', 'last_val') else 1
        joined = np.concatenate([parts[0][k], parts[1][k]], axis=ax)
        assert joined.tobytes() == whole[k].tobytes(), (form, precision, k)
