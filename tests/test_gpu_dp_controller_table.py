"""Per-env numbers for the baseline in the closed loop (include/dpenv.h dpenv_set_dp_controller_table): every env flies its own row of
a controller table.  What is tested is kernel = host law per env, bit for bit - deploy.BatchedDPController with per-env parameters on
the launch's own observation rows, which is also the test that the packing kernel's f64 allocation matrix is the host's - equal rows
against the scalar controller, lanes that do not mix, launches in pieces, the vessel sources, graph capture, the refusals and the
zero controller, and the scored gain sweep against one scalar flight per gain set."""
import math

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, T = 200, 40                       # three full waves and a tail
ROWS = ('obs', 'act', 'rew', 'done', 'last_obs')
ZERO_ACTION = np.float32([0, 0, 0, 0, 1, 0, 1])


def torch_():
    import torch
    return torch


def _env(n=N, **kw):
    kw.setdefault('current', True)
    kw.setdefault('seed', 5)
    return H.make_pair('final_cont', n, **kw)[0]


def _current(env, vc=0.2):
    """0.2 m/s from 16 directions."""
    torch = torch_()
    n = env.n_envs
    beta = (2 * math.pi / 16) * (torch.arange(n, device=env.device) % 16).float()
    env.set_current(torch.full((n,), vc, device=env.device), beta.contiguous())


def _start(env, table=None, check=True):
    """The controller on (defaults), the table in force if given, every env from the training sampler in the 0.2 m/s current."""
    if env.cfg.current_enabled:
        _current(env)
    env.set_dp_controller()
    if table is not None:
        env.set_dp_controller_table(table, check=check)
    return env.reset().clone()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b, keys=ROWS, what=''):
    torch = torch_()
    for k in keys:
        assert torch.equal(a[k], b[k]), '%s %s: %d elements differ' % (what, k, int((a[k] != b[k]).sum()))


def _same_state(a, b):
    torch = torch_()
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.get_dp_controller_state(), b.get_dp_controller_state())
    assert torch.equal(a.get_obs_thrust(), b.get_obs_thrust())


def _distinct_table(n, seed=7, hulls=None):
    """[32, n] float32, every row its own: factors in [0.25, 4] on kp / kd / ki, in [0.5, 2] on z_bound / tau_max, the weights and kf,
    lever arms +- 10 % (or each env's own hull's lever arms and thrust constants)."""
    from ml4ca_amd import _lib
    from ml4ca_amd.deploy import dp_controller_defaults, dp_controller_table
    rng = np.random.RandomState(seed)
    p = dp_controller_defaults()
    f = lambda lo, hi, k: np.exp(rng.uniform(np.log(lo), np.log(hi), (n, k)))
    per = dict(kp=p['kp'] * f(0.25, 4, 3), kd=p['kd'] * f(0.25, 4, 3), ki=p['ki'] * f(0.25, 4, 3), z_bound=p['z_bound'] * f(0.5, 2, 3),
               tau_max=p['tau_max'] * f(0.5, 2, 3), weight=f(0.5, 2, 5))
    if hulls is None:
        per.update(kf=p['kf'] * f(0.5, 2, 3), lx=p['lx'] * (1 + 0.1 * rng.uniform(-1, 1, (n, 3))), ly=p['ly'] * (1 + 0.1 * rng.uniform(-1, 1, (n, 3))))
    else:
        P = _lib.P
        per.update(kf=hulls[P['KF_BOW']:P['KF_BOW'] + 3].T, kr_bow=hulls[P['KR_BOW']], lx=hulls[P['LX_BOW']:P['LX_BOW'] + 3].T,
                   ly=hulls[P['LY_BOW']:P['LY_BOW'] + 3].T)
    return dp_controller_table(n, p, **per)


def _host_actions(env, out, table):
    """The NumPy-f32 per-env host law on the launch's own obs rows in order, z reset where done[t - 1] != 0: (act [T, n, 7], ctrl, hits)."""
    from ml4ca_amd.deploy import BatchedDPController
    ctrl = BatchedDPController(env.n_envs, table, dt=env.control_period)
    obs, done = _np(out['obs']), _np(out['done'])
    acts, hits = [], dict(z=0, tau=0)
    for t in range(obs.shape[0]):
        if t > 0:
            ctrl.reset(done[t - 1] != 0)
        tau = ctrl.wrench(obs[t])
        acts.append(ctrl.allocate(tau))
        hits['z'] += int((np.abs(ctrl.z) == ctrl.zb).any(1).sum())
        hits['tau'] += int((np.abs(tau) == ctrl.tmax).any(1).sum())
    return np.stack(acts), ctrl, hits


def _assert_host_law(env, out, table):
    want, ctrl, hits = _host_actions(env, out, table)
    got = _np(out['act'])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    z = np.ascontiguousarray(_np(env.get_dp_controller_state()).T)
    ctrl.reset(_np(out['done'])[-1] != 0)
    assert np.array_equal(z.view(np.uint32), ctrl.z.view(np.uint32))
    return got, hits


@pytest.mark.parametrize('n', [N, 65])                                                # 65: a full wave plus one lane
def test_equal_rows_write_the_rows_of_the_scalar_controller(n):
    from ml4ca_amd.deploy import dp_controller_table
    from ml4ca_amd.policy import controller_rollout
    a, b = (_env(n, auto_reset=True, terminate=False, max_ep_len=70) for _ in range(2))
    tab = H.to_dev(dp_controller_table(n), b.device)
    _start(a)
    _start(b, tab)
    assert a.dp_controller_table is None and b.dp_controller_table is tab
    _same(controller_rollout(a, T), controller_rollout(b, T), what='equal rows')
    _same_state(a, b)
    assert bool((a.get_dp_controller_state() != 0).any())


def test_distinct_rows_equal_the_per_env_host_law_bit_for_bit():
    from ml4ca_amd.policy import controller_rollout
    env = _env(auto_reset=True, terminate=False, max_ep_len=70)                        # every env is cut (and re-drawn) at step 35
    tab = _distinct_table(N)
    _start(env, H.to_dev(tab, env.device))
    out = controller_rollout(env, T)
    got, hits = _assert_host_law(env, out, tab)
    done = _np(out['done'])
    print('clips: z %d, tau %d, bow %d, stern %d; resets %d' % (hits['z'], hits['tau'], int((np.abs(got[..., 0]) == 1).sum()),
                                                               int((got[..., 1:3] == 1).sum()), int((done != 0).sum())))
    # every clip of the law was exercised: the integral's bound, tau_max, the bow and the stern thrust limits; and the re-draw
    assert hits['z'] > 0 and hits['tau'] > 0 and (np.abs(got[..., 0]) == 1).any() and (got[..., 1:3] == 1).any()
    assert (np.abs(got[..., 0]) < 1).any() and (got[..., 1:3] < 1).any() and (done != 0).any()
    # ... and the rows are not the scalar controller's
    b = _env(auto_reset=True, terminate=False, max_ep_len=70)
    _start(b)
    assert not torch_().equal(controller_rollout(b, T)['act'], out['act'])


def test_rows_do_not_mix_between_lanes():
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    rng = np.random.RandomState(9)
    tab = _distinct_table(N, seed=8)
    init = np.zeros((6, N), np.float32)
    init[0:2] = rng.uniform(-6, 6, (2, N))
    init[2] = rng.uniform(-2.5, 2.5, N)
    init[3:6] = rng.uniform(-0.3, 0.3, (3, N))
    ref = (rng.uniform(-3, 3, (3, N)) * np.array([[1.0], [1.0], [0.3]])).astype(np.float32)
    vc, beta = rng.uniform(0.05, 0.3, N).astype(np.float32), rng.uniform(-math.pi, math.pi, N).astype(np.float32)
    outs = []
    for flip in (False, True):
        env = _env(auto_reset=False, terminate=False)
        r = (lambda x: np.ascontiguousarray(x[..., ::-1])) if flip else (lambda x: x)
        env.set_current(H.to_dev(r(vc), env.device), H.to_dev(r(beta), env.device))
        env.set_dp_controller()
        env.set_dp_controller_table(H.to_dev(r(tab), env.device))
        env.reset(init=H.to_dev(r(init), env.device), new_ref=H.to_dev(r(ref), env.device))
        out = controller_rollout(env, T)
        out['z'] = env.get_dp_controller_state()
        out['state'] = env.get_state()[0]
        outs.append(out)
    a, b = outs
    for k in ('obs', 'act', 'rew', 'done'):
        assert torch.equal(a[k], b[k].flip(1)), k
    assert torch.equal(a['last_obs'], b['last_obs'].flip(0))
    assert torch.equal(a['z'], b['z'].flip(1)) and torch.equal(a['state'], b['state'].flip(1))
    assert len({_np(a['act'])[-1, i].tobytes() for i in range(N)}) == N


@pytest.mark.parametrize('filt', [False, True])
def test_two_launches_of_half_write_the_rows_of_one(filt):
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    a, b = (_env(auto_reset=True, terminate=True, max_ep_len=24) for _ in range(2))
    tab = H.to_dev(_distinct_table(N, seed=10), a.device)
    for e in (a, b):
        if filt:
            e.set_reference_filter()
        _start(e, tab)
    refs = torch.zeros((2, 3, N), device=a.device)
    refs[0, 0], refs[0, 1], refs[0, 2] = 3.0, -2.0, math.radians(-45.0)
    refs[1, 0], refs[1, 1], refs[1, 2] = 1.0, 2.0, math.radians(170.0)
    one = controller_rollout(a, T, switch_steps=(3, 25), refs=refs)
    h1 = controller_rollout(b, T // 2, switch_steps=(3,), refs=refs[0:1].contiguous())
    h1 = {k: v.clone() for k, v in h1.items()}
    z = b.get_dp_controller_state().clone()
    b.set_dp_controller_table(tab)                                                     # the same table again: z is left alone
    assert torch.equal(b.get_dp_controller_state(), z) and bool((z != 0).any())
    h2 = controller_rollout(b, T // 2, switch_steps=(5,), refs=refs[1:2].contiguous())
    keys = ('obs', 'act', 'rew', 'done') + (('ref',) if filt else ())
    for k in keys:
        assert torch.equal(one[k][:T // 2], h1[k]) and torch.equal(one[k][T // 2:], h2[k]), k
    assert torch.equal(one['obs'][T // 2], h1['last_obs']) and torch.equal(one['last_obs'], h2['last_obs'])
    _same_state(a, b)
    if filt:
        for x, y in zip(a.get_reference_filter_state(), b.get_reference_filter_state()):
            assert torch.equal(x, y)
    assert bool((one['done'] != 0).any())


def _replay_through_rollout(env, table, randomised=False):
    """Fly the table, restore the pre-launch state, feed its act block to dpenv_rollout: the same rows and the same final state."""
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    _start(env, H.to_dev(table, env.device))
    st, ctr = env.get_state()
    hull = env.get_vessel_params().clone() if randomised else None
    out = controller_rollout(env, T)
    st1, ctr1 = env.get_state()
    env.set_state(st, ctr)
    if randomised:
        env.set_vessel_params(hull, keep_randomisation=True)
    obs, rew, done = env.rollout(out['act'])
    assert torch.equal(obs[:-1], out['obs'][1:]) and torch.equal(obs[-1], out['last_obs'])
    assert torch.equal(rew, out['rew']) and torch.equal(done, out['done'])
    st2, ctr2 = env.get_state()
    assert torch.equal(st1, st2) and torch.equal(ctr1, ctr2)
    return out


def test_vessel_sources():
    import ml4ca_amd
    n = 130
    kw = dict(auto_reset=True, terminate=True, max_ep_len=24, step_one_wave=True)
    tab = _distinct_table(n, seed=12)
    # the shared hull
    a = _env(n, **kw)
    out = _replay_through_rollout(a, tab)
    _assert_host_law(a, out, tab)
    assert bool((out['done'] != 0).any())
    # the thrust-loss preset as the one class
    b = _env(n, vessel_params=ml4ca_amd.default_vessel('thrust_loss'), **kw)
    out_b = _replay_through_rollout(b, tab)
    _assert_host_law(b, out_b, tab)
    assert not torch_().equal(out_b['obs'], out['obs'])                                # the loss acts
    # per-env hulls, flown by controllers that KNOW them: lever arms and thrust constants from each env's own hull
    hulls = H.random_hulls(np.random.RandomState(13), n)
    c = _env(n, **kw)
    c.set_vessel_params(H.to_dev(hulls, c.device))
    own = _distinct_table(n, seed=12, hulls=hulls)
    out_c = _replay_through_rollout(c, own)
    _assert_host_law(c, out_c, own)
    nominal = _env(n, **kw)                                                            # ... which is not the nominal lever arms' flight
    nominal.set_vessel_params(H.to_dev(hulls, nominal.device))
    from ml4ca_amd.policy import controller_rollout
    _start(nominal, H.to_dev(tab, nominal.device))
    assert not torch_().equal(controller_rollout(nominal, T)['act'], out_c['act'])
    # hulls re-drawn per episode
    d = _env(n, **kw)
    d.set_vessel_randomisation(0.1)
    out_d = _replay_through_rollout(d, tab, randomised=True)
    _assert_host_law(d, out_d, tab)
    assert bool((out_d['done'] != 0).any())


def test_captured_setter_and_launch_replay_like_eager_calls():
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    a, b, c = (_env(auto_reset=True, terminate=True, max_ep_len=24) for _ in range(3))
    tabs = [H.to_dev(_distinct_table(N, seed=14), e.device) for e in (a, b, c)]
    for e, tb in zip((a, b, c), tabs):
        _start(e, tb, check=False)                                                     # (the first call allocates the packed block)
        assert e.dp_controller_table is tb
    out = controller_rollout(a, 8)                                                     # warm-up: the buffers the graph writes
    controller_rollout(b, 8)
    controller_rollout(c, 8)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.set_dp_controller_table(tabs[0], check=False)
        controller_rollout(a, 8, out=out)
    for k in range(2):
        g.replay()
        eager = controller_rollout(b, 8)
        controller_rollout(c, 8)
        torch.cuda.synchronize()
        _same(out, eager, what='replay %d' % k)
    # the table's contents changed in place: the replay packs and flies the new gains
    for tb in tabs[:2]:
        tb[0:9] *= 0.5
    b.set_dp_controller_table(tabs[1], check=False)
    g.replay()
    eager = controller_rollout(b, 8)
    old = controller_rollout(c, 8)
    torch.cuda.synchronize()
    _same(out, eager, what='replay with new gains')
    assert not torch.equal(out['act'], old['act'])
    _same_state(a, b)


def test_refused_rows_fly_the_zero_controller():
    from ml4ca_amd import DpenvError, _lib
    from ml4ca_amd.deploy import allocation_matrix, dp_controller_table
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    good = _distinct_table(N, seed=15)
    bad = good.copy()
    rows = {3: 'a NaN gain', 64: 'a negative bound', 65: 'kf = 0', 130: 'a zero weight', 199: 'singular lever arms'}
    bad[1, 3] = np.nan                                                                 # kp[1]
    bad[9, 64] = -1.0                                                                  # z_bound[0]
    bad[28, 65] = 0.0                                                                  # kf[2]
    bad[17, 130] = 0.0                                                                 # weight[2]
    bad[20:23, 199] = 1.0                                                              # lx all equal and ly port = star: T has rank 2, and with
    bad[24:26, 199] = 0.5                                                              # these values and unit weights every product and sum of
    bad[15:20, 199] = 1.0                                                              # the recipe is exact in f64 - det is exactly 0
    with pytest.raises(ValueError, match='singular'):
        allocation_matrix(bad[20:23, 199], bad[23:26, 199], bad[15:20, 199])
    kw = dict(auto_reset=True, terminate=True, max_ep_len=24)
    a, b, c, d = (_env(**kw) for _ in range(4))
    # the library marks exactly those envs, and they fly the zero controller; every other env flies as without them
    _current(a)
    a.set_dp_controller()
    mask = torch.full((N,), 7, dtype=torch.uint8, device=a.device)
    tb = H.to_dev(bad, a.device)
    _lib.check(a.lib.dpenv_set_dp_controller_table(a._h, a._ptr(tb), a._ptr(mask), a._stream()), a._h)
    a.reset()
    want_mask = np.zeros(N, np.uint8)
    want_mask[list(rows)] = 1
    assert np.array_equal(_np(mask), want_mask)
    out = controller_rollout(a, T)
    _start(b, H.to_dev(good, b.device))
    ref = controller_rollout(b, T)
    ok = torch.from_numpy(want_mask == 0).to(a.device)
    for k in ('obs', 'act', 'rew', 'done'):
        assert torch.equal(out[k][:, ok], ref[k][:, ok]), k
    assert torch.equal(out['last_obs'][ok], ref['last_obs'][ok])
    act = _np(out['act'])
    for i, what in rows.items():
        assert np.array_equal(act[:, i], np.tile(ZERO_ACTION, (T, 1))), what
    assert bool((a.get_dp_controller_state()[:, ~ok] == 0).all())
    # check=True raises and leaves the scalar law in force (c and d from here on in lock step: d never sees a table)
    _current(c)
    c.set_dp_controller()
    with pytest.raises(ValueError, match=r'5 row\(s\) refused \(envs \[3, 64, 65, 130, 199\]'):
        c.set_dp_controller_table(tb)
    assert c.dp_controller_table is None
    c.reset()
    _start(d)
    _same(controller_rollout(c, T), controller_rollout(d, T), what='after a refused table')
    # a table while the controller is off, and a NULL handle: DPENV_EINVAL, the handle works afterwards
    c.set_dp_controller(off=True)
    with pytest.raises(DpenvError, match='is off'):
        c.set_dp_controller_table(H.to_dev(good, c.device))
    assert c.dp_controller_table is None
    assert c.lib.dpenv_set_dp_controller_table(None, c._ptr(tb), None, c._stream()) == _lib.EINVAL
    # set_dp_controller(params) after a table drops the table
    c.set_dp_controller()
    c.set_dp_controller_table(H.to_dev(good, c.device))
    c.set_dp_controller()
    assert c.dp_controller_table is None
    d.set_dp_controller()
    _same(controller_rollout(c, T), controller_rollout(d, T), what='after set_dp_controller')
    _same_state(c, d)
    # None returns to the scalar numbers without touching z
    c.set_dp_controller_table(H.to_dev(dp_controller_table(N), c.device))
    z = c.get_dp_controller_state().clone()
    c.set_dp_controller_table(None)
    assert c.dp_controller_table is None and torch.equal(c.get_dp_controller_state(), z) and bool((z != 0).any())
    _same(controller_rollout(c, 4), controller_rollout(d, 4), what='after None')


def test_gain_sweep_equals_one_scalar_flight_per_gain_set():
    from ml4ca_amd import evaluate
    from ml4ca_amd.deploy import dp_controller_defaults, gain_population
    torch = torch_()
    K, D, T_ = 3, 16, 100                                                              # one switch (step 50), four chunks of 25
    base = dp_controller_defaults()
    pop = gain_population(K, base, seed=1)
    env = _env(K * D, terminate=False, auto_reset=False)
    res = evaluate.baseline_gain_sweep(env, pop, directions=D, vc=0.2, reference_filter=True, T=T_, chunk=25)
    assert res['iae'].shape == (K, D) and res['work'].shape == (K, D, 3) and res['iae'].dtype == torch.float64
    assert env.dp_controller_table is res['table'] and res['table'].shape == (32, K * D)
    for k in range(K):                                                                 # gain set k as the scalar controller, the same currents
        one = _env(D, terminate=False, auto_reset=False)
        _current(one)
        one.set_dp_controller(dict(base, kp=pop['kp'][k], kd=pop['kd'][k], ki=pop['ki'][k]))
        st = evaluate.baseline_box_test_streamed(one, T=T_, reference_filter=True, chunk=25)
        assert torch.equal(res['iae'][k], st['iae']) and torch.equal(res['work'][k], st['work']), k
    assert not torch.equal(res['iae'][0], res['iae'][1])
    # the one-piece flight's scores, within what test_gpu_score.py allows between the streamed and the host sums
    whole = evaluate.baseline_box_test(env, T=T_, reference_filter=True)
    iae1, w1 = whole['iae'].double().reshape(K, D), whole['work'].double().reshape(K, D, 3)
    assert float(((res['iae'] - iae1).abs() / iae1.abs().clamp_min(1e-30)).max()) < 1e-6
    assert float(((res['work'] - w1).abs() / w1.abs().clamp_min(1e-30)).max()) < 1e-6
    assert torch.equal(res['mean_iae'], res['iae'].mean(1)) and torch.equal(res['mean_work'], res['work'].mean(1))
    want = evaluate.pareto_front(_np(res['mean_iae']), _np(res['mean_work'].sum(1)))
    assert np.array_equal(res['front'], want) and 1 <= len(want) <= K
    with pytest.raises(ValueError, match='need an env of'):
        evaluate.baseline_gain_sweep(env, gain_population(K + 1, base), directions=D, T=T_, chunk=25)
