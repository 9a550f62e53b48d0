"""The classical baseline in the closed loop (include/dpenv.h dpenv_set_dp_controller / dpenv_controller_rollout): the PID +
pseudo-inverse law evaluated inside a T-step launch.  What is tested is kernel = host law, bit for bit: deploy.BatchedDPController in
NumPy float32 on the launch's own observation rows, dpenv_rollout on its action rows, the eager composition with the reference filter,
launches in pieces, the reset paths, the vessel sources, graph capture, the refusals, the stateless allocation and the score card."""
import math

import numpy as np
import pytest

from tests import helpers as H
from tests import tolerances as TOL

pytestmark = pytest.mark.gpu

N, T = 200, 40                       # three full waves and a tail
ROWS = ('obs', 'act', 'rew', 'done', 'last_obs')


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


def _start(env):
    """The controller on (defaults), every env from the training sampler in the 0.2 m/s current."""
    if env.cfg.current_enabled:
        _current(env)
    env.set_dp_controller()
    return env.reset().clone()


def _host(env):
    from ml4ca_amd.deploy import BatchedDPController
    return BatchedDPController(env.n_envs, env.dp_controller, dt=env.control_period)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b, keys=ROWS, what=''):
    torch = torch_()
    for k in keys:
        assert torch.equal(a[k], b[k]), '%s %s: %d elements differ' % (what, k, int((a[k] != b[k]).sum()))


def _host_actions(env, out, ctrl=None):
    """The NumPy-f32 host law on the launch's own obs rows in order, z reset where done[t - 1] != 0: (act [T, n, 7], ctrl, stats)."""
    ctrl = ctrl or _host(env)
    obs, done = _np(out['obs']), _np(out['done'])
    zb, tm = np.float32(env.dp_controller['z_bound']), np.float32(env.dp_controller['tau_max'])
    acts, hits = [], dict(z=0, tau=0)
    for t in range(obs.shape[0]):
        if t > 0:
            ctrl.reset(done[t - 1] != 0)
        tau = ctrl.wrench(obs[t])
        acts.append(ctrl.allocate(tau))
        hits['z'] += int((np.abs(ctrl.z) == zb).any(1).sum())
        hits['tau'] += int((np.abs(tau) == tm).any(1).sum())
    return np.stack(acts), ctrl, hits


def test_law_actions_equal_the_host_law_bit_for_bit():
    from ml4ca_amd.policy import controller_rollout
    env = _env(auto_reset=True, terminate=False, max_ep_len=70)       # every env is cut (and re-drawn) at step 35
    _start(env)
    out = controller_rollout(env, T)
    want, ctrl, hits = _host_actions(env, out)
    got = _np(out['act'])
    print('clips: z %d, tau %d, bow %d, stern %d; resets %d' % (hits['z'], hits['tau'], int((np.abs(got[..., 0]) == 1).sum()),
                                                               int((got[..., 1:3] == 1).sum()), int((_np(out['done']) != 0).sum())))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    z = _np(env.get_dp_controller_state()).T
    ctrl.reset(_np(out['done'])[-1] != 0)
    assert np.array_equal(z.view(np.uint32), ctrl.z.view(np.uint32))
    # every clip of the law was exercised: the integral's bound, tau_max, the bow and the stern thrust limits; and the re-draw
    assert hits['z'] > 0 and hits['tau'] > 0 and (np.abs(got[..., 0]) == 1).any() and (got[..., 1:3] == 1).any()
    assert (np.abs(got[..., 0]) < 1).any() and (got[..., 1:3] < 1).any() and (_np(out['done']) != 0).any()


def _replay_through_rollout(env, randomised=False):
    """Fly the controller, restore the pre-launch state, feed its act block to dpenv_rollout: the same rows and the same final state."""
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    _start(env)
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


def test_env_rows_replay_through_dpenv_rollout():
    out = _replay_through_rollout(_env(auto_reset=True, terminate=True, max_ep_len=24, step_one_wave=True))
    assert bool((out['done'] != 0).any())
    _replay_through_rollout(_env(auto_reset=False, terminate=False))                  # (the two-wave rollout kernel)


@pytest.mark.parametrize('filt', [False, True])
def test_two_launches_of_half_write_the_rows_of_one(filt):
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    a, b = (_env(auto_reset=True, terminate=True, max_ep_len=24) for _ in range(2))
    for e in (a, b):
        if filt:
            e.set_reference_filter()
        _start(e)
    dev = a.device
    refs = torch.zeros((2, 3, N), device=dev)
    refs[0, 0], refs[0, 1], refs[0, 2] = 3.0, -2.0, math.radians(-45.0)
    refs[1, 0], refs[1, 1], refs[1, 2] = 1.0, 2.0, math.radians(170.0)
    one = controller_rollout(a, T, switch_steps=(3, 25), refs=refs)
    h1 = controller_rollout(b, T // 2, switch_steps=(3,), refs=refs[0:1].contiguous())
    h1 = {k: v.clone() for k, v in h1.items()}
    h2 = controller_rollout(b, T // 2, switch_steps=(5,), refs=refs[1:2].contiguous())
    keys = ('obs', 'act', 'rew', 'done') + (('ref',) if filt else ())
    for k in keys:
        assert torch.equal(one[k][:T // 2], h1[k]) and torch.equal(one[k][T // 2:], h2[k]), k
    assert torch.equal(one['obs'][T // 2], h1['last_obs']) and torch.equal(one['last_obs'], h2['last_obs'])
    assert bool((one['obs'][1:, :, 6:9] != 0).any())                                  # thrust columns
    assert torch.equal(a.get_dp_controller_state(), b.get_dp_controller_state())
    assert torch.equal(a.get_obs_thrust(), b.get_obs_thrust())
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    if filt:
        for x, y in zip(a.get_reference_filter_state(), b.get_reference_filter_state()):
            assert torch.equal(x, y)
    assert bool((one['done'] != 0).any())


def test_fused_launch_equals_the_eager_composition_with_the_filter():
    from ml4ca_amd.deploy import BatchedReferenceFilter
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    K = 20
    a, b = (_env(auto_reset=False, terminate=False) for _ in range(2))
    a.set_reference_filter()
    obs0 = [_start(e) for e in (a, b)][-1]
    dev = a.device
    ref0 = a.get_state()[0][6:9].clone().contiguous()
    refs = torch.zeros((1, 3, N), device=dev)
    refs[0, 0], refs[0, 1], refs[0, 2] = 3.0, -2.0, math.radians(-45.0)
    fused = controller_rollout(a, K, switch_steps=(3,), refs=refs)
    p = a.reference_filter
    F = BatchedReferenceFilter(N, omega=p['omega'], zeta=p['zeta'], dt=a.control_period, device=dev)
    F.reset(ref0)
    ctrl = _host(b)
    rows = {k: [] for k in ('obs', 'act', 'rew', 'done', 'ref')}
    o, eta, in_force = obs0.clone(), ref0.clone(), ref0.clone()
    for t in range(K):
        act = torch.from_numpy(ctrl.act(_np(o))).to(dev)
        rows['obs'].append(o.clone())
        rows['act'].append(act)
        rows['ref'].append(eta.T.clone())
        if t == 3:
            F.switch(refs[0])
        nr = F.advance()
        o, rew, done, _ = b.step(act, new_ref=nr)
        o = o.clone()
        rows['rew'].append(rew.clone())
        rows['done'].append(done.clone())
        eta, in_force = in_force, nr                                # o_t+1 was formed before new_ref applied
    eager = {k: torch.stack(v) for k, v in rows.items()}
    eager['last_obs'] = o
    _same(fused, eager, ROWS + ('ref',))
    assert torch.equal(a.get_dp_controller_state(), torch.from_numpy(ctrl.z.T.copy()).to(dev))


def test_resets_zero_the_integral():
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    env = _env(auto_reset=True, terminate=True, max_ep_len=24)                        # config.max_ep_len = 12
    assert env.cfg.max_ep_len == 12 and env.cfg.terminate == 1 and env.cfg.auto_reset == 1
    _start(env)
    out = controller_rollout(env, T)
    obs, act, done = _np(out['obs']), _np(out['act']), _np(out['done'])
    fresh = 0
    for t in range(1, T):
        m = done[t - 1] != 0
        if m.any():
            c0 = _host(env)                                                           # z = 0
            want = c0.act(obs[t])
            assert np.array_equal(act[t][m].view(np.uint32), want[m].view(np.uint32)), t
            fresh += int(m.sum())
    assert fresh >= N                                                                  # every env was cut at least once
    # a masked dpenv_reset zeroes z of the masked envs only
    z0 = env.get_dp_controller_state().clone()
    assert bool((z0 != 0).any(0).sum() > N // 2)
    mask = (torch.arange(N, device=env.device) % 2 == 0).to(torch.uint8)
    env.reset(mask=mask)
    z1 = env.get_dp_controller_state()
    assert bool((z1[:, 0::2] == 0).all()) and torch.equal(z1[:, 1::2], z0[:, 1::2])
    # ... and the state round-trips
    env.set_dp_controller_state(z0)
    assert torch.equal(env.get_dp_controller_state(), z0)


def test_vessel_sources():
    import ml4ca_amd
    from ml4ca_amd.policy import controller_rollout
    n = 130
    kw = dict(auto_reset=True, terminate=True, max_ep_len=24)
    # per-env blocks given the class's numbers = the shared hull
    a, b = _env(n, **kw), _env(n, **kw)
    b.set_vessel_params(ml4ca_amd.default_vessel())
    for e in (a, b):
        _start(e)
    _same(controller_rollout(a, T), controller_rollout(b, T), what='per-env blocks')
    # the thrust-loss preset as the shared form = the same hull as per-env blocks
    loss = ml4ca_amd.default_vessel('thrust_loss')
    a, b = _env(n, vessel_params=loss, **kw), _env(n, **kw)
    b.set_vessel_params(loss)
    for e in (a, b):
        _start(e)
    ra, rb = controller_rollout(a, T), controller_rollout(b, T)
    _same(ra, rb, what='thrust loss')
    c = _env(n, **kw)
    _start(c)
    assert not torch_().equal(controller_rollout(c, T)['obs'], ra['obs'])             # the loss acts
    # hull randomisation on: the rows replay through dpenv_rollout
    d = _env(n, step_one_wave=True, **kw)
    d.set_vessel_randomisation(0.1)
    out = _replay_through_rollout(d, randomised=True)
    assert bool((out['done'] != 0).any())
    want, _, _ = _host_actions(d, out)                                                # ... flown by a controller that does not know the hull
    assert np.array_equal(_np(out['act']).view(np.uint32), want.view(np.uint32))


def test_captured_launch_replays_like_eager_launches():
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    a, b = (_env(auto_reset=True, terminate=True, max_ep_len=24) for _ in range(2))
    for e in (a, b):
        _start(e)
    out = controller_rollout(a, 8)                                                    # warm-up: the buffers the graph writes
    controller_rollout(b, 8)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        controller_rollout(a, 8, out=out)
    for k in range(3):
        g.replay()
        eager = controller_rollout(b, 8)
        torch.cuda.synchronize()
        _same(out, eager, what='replay %d' % k)
    assert torch.equal(a.get_dp_controller_state(), b.get_dp_controller_state())


def _refused(fn, word):
    from ml4ca_amd import DpenvError
    with pytest.raises(DpenvError, match=word):
        fn()


def test_refusals_leave_the_handle_alone():
    import ml4ca_amd
    from ml4ca_amd.deploy import dp_controller_defaults
    from ml4ca_amd.policy import controller_rollout
    torch = torch_()
    n = 64
    rng = np.random.RandomState(0)
    # configurations outside the supported set: refused with the set named, later rows as a handle that never asked
    two = np.stack([ml4ca_amd.default_vessel(), ml4ca_amd.default_vessel() * np.float32(1.1)])        # two vessel classes
    for mode, kw in (('limited', {}), ('final_wrap', {}), ('final_cont', dict(ext=False)), ('final_cont', dict(vessel_params=two))):
        a, b = (H.make_pair(mode, n, seed=2, **kw)[0] for _ in range(2))
        acts = H.to_dev(np.stack([H.random_actions(rng, n, a.num_actions) for _ in range(4)]), a.device)
        for e in (a, b):
            if 'vessel_params' in kw:
                e.set_vessel_class((torch.arange(n, device=e.device) % 2).to(torch.int32))
            e.reset()
        _refused(a.set_dp_controller, 'final variant')
        assert a.dp_controller is None
        for x, y in zip(a.rollout(acts), b.rollout(acts)):
            assert torch.equal(x, y), mode
    # the integral action on
    a, b = _env(n), _env(n)
    a.set_integral_action()
    _refused(a.set_dp_controller, 'integral action')
    a.set_integral_action(None)
    # launch while the controller is off
    _refused(lambda: controller_rollout(a, 4), 'is off')
    for e in (a, b):
        _start(e)
    _same(controller_rollout(a, 4), controller_rollout(b, 4), what='after refusals')
    # a NaN gain (and the other bad numbers): refused before any state changes - z and the numbers in force stay
    good = dp_controller_defaults()
    for key, idx, val, word in (('kp', 1, float('nan'), 'finite'), ('z_bound', 0, -1.0, 'z_bound'), ('kf', 2, 0.0, 'kf'),
                                ('tau_max', 2, float('nan'), 'tau_max')):
        bad = {k: np.array(v, np.float64, copy=True) for k, v in good.items()}
        bad[key][idx] = val
        _refused(lambda: a.set_dp_controller(bad), word)
    assert bool((a.get_dp_controller_state() != 0).any())
    _same(controller_rollout(a, 4), controller_rollout(b, 4), what='after a NaN gain')
    # the integral action turned on behind the controller's back: the launch is refused
    a.set_integral_action()
    _refused(lambda: controller_rollout(a, 4), 'integral action')
    a.set_integral_action(None)
    _same(controller_rollout(a, 4), controller_rollout(b, 4), what='after the integral action')
    # ref_out needs the filter; the other launches keep working while the controller is on
    acts = H.to_dev(np.stack([H.random_actions(rng, n, 7) for _ in range(4)]), a.device)
    for x, y in zip(a.rollout(acts), b.rollout(acts)):
        assert torch.equal(x, y)
    assert torch.equal(a.get_dp_controller_state(), b.get_dp_controller_state())


def test_thrust_alloc_equals_the_host_allocation():
    import ml4ca_amd
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_defaults
    torch = torch_()
    n = 1000
    rng = np.random.RandomState(3)
    tau = (rng.uniform(-1.0, 1.0, (n, 3)) * (40.0, 12.0, 12.0)).astype(np.float32)
    tau[:8] = 0.0
    tau[8:16] *= np.float32(1e-8)
    p = dp_controller_defaults()
    want = BatchedDPController(n, p).allocate(tau)
    t_dev = H.to_dev(tau.T.copy())
    got = ml4ca_amd.thrust_alloc(t_dev, p)
    g = _np(got)
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), int((g != want).sum())
    assert np.array_equal(g[:8], np.tile(np.float32([0, 0, 0, 0, 1, 0, 1]), (8, 1)))
    # decoded through the force map, unsaturated rows reproduce tau
    n_pct = (got[:, 0:3] * 100.0).T.contiguous()
    alpha = torch.stack([torch.full((n,), math.pi / 2, device=got.device), torch.atan2(got[:, 3], got[:, 4]),
                         torch.atan2(got[:, 5], got[:, 6])]).contiguous()
    back = _np(ml4ca_amd.thrust_map(n_pct, alpha)).T
    inside = (np.abs(g[:, 0]) < 1) & (g[:, 1] < 1) & (g[:, 2] < 1)
    assert 300 < inside.sum() < n
    err = np.abs(back[inside].astype(np.float64) - tau[inside])
    print('tau round trip: max abs err %.3e, max err / tol %.3f' % (
        err.max(), (err / (TOL.RTOL_F32 * np.maximum(np.abs(tau[inside]), TOL.TAU_FLOOR))).max()))
    TOL.assert_close(back[inside], tau[inside], TOL.TAU_FLOOR, what='tau')
    assert (np.abs(back[~inside] - tau[~inside]) > 0.1).any()                       # a saturated command is not redistributed


def test_streamed_box_test_equals_the_one_piece_flight():
    from ml4ca_amd import evaluate
    torch = torch_()
    n = 256
    env = _env(n, terminate=False, auto_reset=False)
    _current(env, 0.0)
    T_ = 320                                                                           # two switches (steps 50, 300), seven chunks
    one = evaluate.baseline_box_test(env, T=T_, reference_filter=True)
    assert set(one) == {'iae', 'work', 'e', 'integ', 'ref', 'out'} and one['e'].shape == (T_, n, 3)
    st = evaluate.baseline_box_test_streamed(env, T=T_, reference_filter=True, chunk=50)
    assert set(st) == {'iae', 'work', 'ret', 'score'}
    iae1, w1 = one['iae'].double(), one['work'].double()
    assert float(((st['iae'] - iae1).abs() / iae1.abs().clamp_min(1e-30)).max()) < 1e-6
    assert float(((st['work'] - w1).abs() / w1.abs().clamp_min(1e-30)).max()) < 1e-6
    assert float(iae1.min()) > 0.0
    # in a 0.2 m/s current from 16 directions the flight stays finite
    _current(env)
    cur = evaluate.baseline_box_test_streamed(env, T=T_, reference_filter=True, chunk=50)
    assert bool(torch.isfinite(cur['iae']).all()) and bool(torch.isfinite(cur['work']).all())
    assert not torch.equal(cur['iae'], st['iae'])
    print('box test, first %d steps, filter on: IAE calm %.2f, in current mean %.2f max %.2f' % (
        T_, float(st['iae'].mean()), float(cur['iae'].mean()), float(cur['iae'].max())))
