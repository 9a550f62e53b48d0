"""The deployed controller in the closed loop: the trained actor plus the RL node's body-frame integral action (rl_allocator.py:252-273),
applied inside the fused launch while dpenv_set_integral_action is on (include/dpenv.h).  The reference for every row is the eager
deployment path on a second handle with the action off: dpenv_step -> deploy.BatchedBodyFrameIntegrator (float32) ->
dpenv_policy_forward -> dpenv_step(mu), bit for bit."""
import math
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

ROWS = ('obs', 'act', 'val', 'logp', 'rew', 'done', 'boot', 'integ', 'last_obs', 'last_val')
# parameters that make every branch of the law happen within a short launch: a one-second dwell (D = 6) and bounds small enough to wind up
FAST = dict(gain=(0.05, 0.05, 0.05), bound=(0.02, 0.03, 0.004), box=(5.0, 5.0, float(np.deg2rad(140.0))), dwell_s=1.0)


def torch_():
    import torch
    return torch


def _make(mode, n, precision, form, seed=3, hidden=(80, 80, 80), **kw):
    """Two identically configured handles with the same actor-critic: A flies the fused launch, B is the eager reference."""
    from ml4ca_amd.policy import ActorCritic
    kw.setdefault('auto_reset', True)
    kw.setdefault('max_ep_len', 50)                              # 25 control steps: every env is cut (and re-drawn) once per 40-step launch
    envs = [H.make_pair(mode, n, seed=seed, **kw)[0] for _ in range(2)]
    ac = ActorCritic(envs[0].num_states, envs[0].num_actions, hidden, seed=seed + 7, device=envs[0].device)
    ac.upload(envs[0], precision=precision, launch_form=form)
    ac.upload(envs[1], precision=precision, launch_form='one_wave')
    return envs[0], envs[1]


def _start(envs, n, seed, kick=6.0, T=40):
    """Both handles at the same pose, 0.5-2 m / a few degrees off the setpoint (inside the box), and a setpoint schedule: at step 12 half
    the envs are kicked `kick` m north (outside the box: I and the dwell clock reset), the rest 1 m; at step 30 a small move."""
    torch = torch_()
    dev = envs[0].device
    g = torch.Generator(device='cpu').manual_seed(seed)
    init = torch.zeros((6, n))
    init[0:2] = (torch.rand((2, n), generator=g) * 1.5 + 0.5) * torch.where(torch.rand((2, n), generator=g) < 0.5, -1.0, 1.0)
    init[2] = (torch.rand(n, generator=g) - 0.5) * 0.2
    init = init.to(dev)
    ref0 = torch.zeros((3, n), device=dev)
    obs0 = [e.reset(init=init, new_ref=ref0).clone() for e in envs]
    k1 = torch.zeros((3, n))
    k1[0] = torch.where(torch.arange(n) % 2 == 0, kick, 1.0)
    k2 = k1.clone()
    k2[1] = 0.5
    k2[2] = 0.05
    steps = (12, 30) if T > 30 else (T // 3,)
    refs = torch.stack([k1, k2][:len(steps)]).to(dev).contiguous()
    return steps, refs, obs0[-1]


def _law(env, **ia):
    from ml4ca_amd.deploy import BatchedBodyFrameIntegrator
    p = env.integral_action
    dt64 = float(np.float64(np.float32(env.cfg.substep_dt)) * env.cfg.n_substeps)      # D in f64, as the library computes it
    law = BatchedBodyFrameIntegrator(env.n_envs, gain=p['gain'], bound=p['bound'], box=p['box'], dwell_s=p['dwell_s'], dt=dt64,
                                     step_s=p['step_s'], device=env.device)
    return law


def replay(envB, law, T, steps=(), refs=None, reset_at_end=False, obs0=None):
    """The eager deployment path: T control steps of dpenv_step + the torch law + dpenv_policy_forward on handle B (action off),
    returning the rows a closed-loop launch writes.  obs0: B's true observation now (the launch's first input is rebuilt from it and
    the stored I with no update)."""
    from ml4ca_amd.policy import policy_forward
    torch = torch_()
    n = envB.n_envs
    rows = {k: [] for k in ('obs', 'act', 'val', 'rew', 'done', 'boot', 'integ')}
    p = obs0.clone()
    p[:, :3] = obs0[:, :3] + law.I
    mu, v = policy_forward(envB, p)
    sw = dict(zip(steps, range(len(steps))))
    fo = torch.empty_like(obs0)
    for t in range(T):
        rows['obs'].append(p.clone())
        rows['integ'].append(law.I.clone())
        rows['act'].append(mu.clone())
        rows['val'].append(v.clone())
        nr = refs[sw[t]].contiguous() if t in sw else None
        obs, rew, done, _ = envB.step(mu.contiguous(), new_ref=nr, final_obs=fo)
        obs, rew, done = obs.clone(), rew.clone(), done.clone()
        rows['rew'].append(rew)
        rows['done'].append(done)
        reset = (done != 0) if envB.auto_reset else torch.zeros(n, dtype=torch.bool, device=obs.device)
        pre = torch.where(reset[:, None], fo, obs)                  # the step's observation before an auto-reset
        if reset_at_end and t == T - 1:
            cont = ~reset
            o_new = envB.reset(mask=cont.to(torch.uint8)).clone()
            obs = torch.where(cont[:, None], o_new, obs)
            reset = torch.ones_like(reset)
        p_pre = pre.clone()
        p_pre[:, :3] = law.update(pre)                              # the step's update (a cut episode's last input carries it)
        law.reset(reset)                                            # a new episode starts with I = 0
        p = obs.clone()
        p[:, :3] = obs[:, :3] + law.I
        mu, v = policy_forward(envB, p)
        _, v_pre = policy_forward(envB, p_pre)
        ended = (done != 0) | (t == T - 1)
        terminal = (done & 1) != 0
        rows['boot'].append(torch.where(ended & ~terminal, torch.where(reset, v_pre, v), torch.zeros_like(v)))
    out = {k: torch.stack(x) for k, x in rows.items()}
    out['last_obs'], out['last_val'] = p, v
    return out


def _logp_rows(envB, T):
    """The deterministic policy's logp (a = mu: a constant of log_std) as a closed loop writes it, from one launch of handle B."""
    from ml4ca_amd.policy import policy_rollout
    return policy_rollout(envB, 1, sample=False)['logp'][0].expand(T, -1)


def _assert_rows(a, b, T, envB):
    torch = torch_()
    b = dict(b, logp=_logp_rows(envB, T))
    for k in ROWS:
        assert torch.equal(a[k], b[k]), k


def _fly(mode, n, precision, form, T=40, reset_at_end=False, seed=3, ia=FAST, setup=None, **kw):
    from ml4ca_amd.policy import policy_rollout
    envA, envB = _make(mode, n, precision, form, seed=seed, **kw)
    if setup is not None:
        setup(envA)
        setup(envB)
    envA.set_integral_action(**ia)
    steps, refs, obs0 = _start((envA, envB), n, seed, T=T)
    a = policy_rollout(envA, T, sample=False, switch_steps=steps, refs=refs, reset_at_end=reset_at_end)
    law = _law(envA)
    b = replay(envB, law, T, steps, refs, reset_at_end=reset_at_end, obs0=obs0)
    _assert_rows(a, b, T, envB)
    return a, b, envA, envB, law


def _law_events(a, ia):
    """(wound up to a bound, reset by a kick, crossed the dwell boundary) in the rows of a launch."""
    torch = torch_()
    I = a['integ']
    bound = torch.tensor(ia['bound'], device=I.device, dtype=I.dtype)
    wound = bool((I.abs() == bound).any())
    nz = (I != 0).any(-1)                                           # [T, n]
    reset = bool((nz[:-1] & ~nz[1:]).any())                        # an env's I went back to zero
    first = nz.float().argmax(0)
    crossed = bool(((first > 0) & nz.any(0)).any())                # zero for the first D steps, then integrating
    return wound, reset, crossed


@pytest.mark.parametrize('precision,form,n', [
    ('f16', 'two_wave', 1000), ('f16', 'one_wave', 1000), ('f32', 'two_wave', 1000), ('f32', 'one_wave', 1000),
    ('f32_actor', 'two_wave', 1000), ('f32_actor', 'one_wave', 1000), ('f16', 'two_wave', 65536), ('f32', 'two_wave', 65536)])
@pytest.mark.parametrize('reset_at_end', [False, True])
def test_closed_loop_replays_through_single_steps(precision, form, n, reset_at_end):
    """Box-like switch schedule, cuts (time limit) + auto-reset, optionally reset_at_end: every row of the fused launch equals the eager
    composition, bit for bit; the schedule winds the integrator up to a bound, resets it with a kick out of the box and crosses the dwell."""
    a, b, envA, envB, law = _fly('final_cont', n, precision, form, reset_at_end=reset_at_end)
    assert all(_law_events(a, FAST)), _law_events(a, FAST)
    assert int((a['done'] != 0).sum()) >= n // 2                   # the auto-reset path ran
    torch = torch_()
    I, c = envA.get_integral_state()
    assert torch.equal(I.T, law.I) and torch.equal(c, law.count)
    if reset_at_end:
        assert bool((I == 0).all()) and bool((c == 0).all())


@pytest.mark.parametrize('precision,form', [('f16', 'two_wave'), ('f32', 'one_wave'), ('f32_actor', 'two_wave')])
def test_zero_gain_and_bounds_give_the_plain_launch(precision, form):
    """gain 0 and bounds 0: the launch writes the rows of the action-off launch, and integ is all zero."""
    from ml4ca_amd.policy import ActorCritic, policy_rollout
    torch = torch_()
    n, T = 1000, 30
    envA, envB = _make('final_cont', n, precision, form)
    ac = ActorCritic(9, 7, (80, 80, 80), seed=10, device=envA.device)
    for e in (envA, envB):
        ac.upload(e, precision=precision, launch_form=form)
    envA.set_integral_action(gain=(0, 0, 0), bound=(0, 0, 0))
    steps, refs, _ = _start((envA, envB), n, 5, T=T)
    a = policy_rollout(envA, T, sample=True, switch_steps=steps, refs=refs)
    b = policy_rollout(envB, T, sample=True, switch_steps=steps, refs=refs)
    for k in ('obs', 'act', 'val', 'logp', 'rew', 'done', 'boot', 'last_obs', 'last_val'):
        assert torch.equal(a[k], b[k]), k
    assert bool((a['integ'] == 0).all())


def test_pieces_of_one_episode_and_checkpoint_restore():
    """Two launches of T/2 write the rows of one launch of T; a checkpoint (state, RNG counters, present current, thrust columns and
    the integral state) restored into the handle continues bit for bit - per-env randomised hulls, a re-drawn drifting current, sampled."""
    from ml4ca_amd.policy import ActorCritic, policy_rollout
    torch = torch_()
    n, T = 1000, 40
    kw = dict(auto_reset=True, max_ep_len=2000, terminate=False, current=True, current_drift=True)
    envs = [H.make_pair('final_cont', n, seed=9, **kw)[0] for _ in range(2)]
    ac = ActorCritic(9, 7, (80, 80, 80), seed=4, device=envs[0].device)
    for e in envs:
        ac.upload(e, precision='f16', launch_form='two_wave')
        e.set_current(torch.full((n,), 0.2, device=e.device), torch.full((n,), 1.0, device=e.device))
        e.set_current_randomisation(0.1, 0.8)
        e.set_vessel_randomisation(0.15)
        e.set_integral_action(**FAST)
        e.reset()
    one = policy_rollout(envs[0], T, sample=True)
    h1 = policy_rollout(envs[1], T // 2, sample=True)
    ck = (envs[1].get_state(), envs[1].get_rng_counters(), envs[1].get_current(), envs[1].get_obs_thrust(), envs[1].get_integral_state())
    ck = tuple(tuple(x.clone() for x in c) if isinstance(c, tuple) else c.clone() for c in ck)
    h2 = policy_rollout(envs[1], T // 2, sample=True)
    for k in ('obs', 'act', 'val', 'logp', 'rew', 'done', 'integ'):
        assert torch.equal(one[k], torch.cat([h1[k], h2[k]])), k
    assert torch.equal(one['boot'][T // 2:], h2['boot']) and torch.equal(one['boot'][:T // 2 - 1], h1['boot'][:T // 2 - 1])
    assert torch.equal(one['last_obs'], h2['last_obs']) and bool((one['integ'] != 0).any())
    # restore the mid-point and fly the second half again
    (st, ctr), (nc, dc), (vc, beta), thr, (I, c) = ck
    envs[1].set_state(st, ctr)
    envs[1].set_rng_counters(nc, dc)
    envs[1].set_current(vc, beta, present_only=True)
    envs[1].set_obs_thrust(thr)
    envs[1].set_integral_state(I, c)
    h3 = policy_rollout(envs[1], T // 2, sample=True)
    for k in ROWS:
        assert torch.equal(h2[k], h3[k]), k


def _hulls(env, rng, loss=0.0):
    env.set_vessel_params(H.to_dev(H.random_hulls(rng, env.n_envs, loss=loss)))


ROBUST = {
    'per_env_hulls': (dict(), lambda e: _hulls(e, np.random.RandomState(1))),
    'randomisation': (dict(), lambda e: e.set_vessel_randomisation(0.15)),
    'loss_shared': (dict(vessel_params='thrust_loss'), None),
    'loss_per_env': (dict(), lambda e: _hulls(e, np.random.RandomState(2), loss=0.05)),
    'current_rand_drift': (dict(current=True, current_drift=True),
                           lambda e: (e.set_current(torch_().full((e.n_envs,), 0.2, device=e.device), torch_().full((e.n_envs,), 2.0, device=e.device)),
                                      e.set_current_randomisation(0.1, 0.8))),
}


@pytest.mark.parametrize('case,form,n', [(c, f, 1000) for c in sorted(ROBUST) for f in ('two_wave', 'one_wave')] +
                         [('randomisation', 'two_wave', 65536), ('loss_shared', 'two_wave', 65536)])
def test_robustness_matrix_replays_through_single_steps(case, form, n):
    """Per-env hulls, hull randomisation, the thrust-loss preset (shared and per env), a re-drawn drifting current: each route of the closed
    loop with the action on replays through single steps bit for bit (1 000 envs: 128-env workgroups; 65 536: 256-env workgroups)."""
    import ml4ca_amd
    kw, setup = ROBUST[case]
    kw = dict(kw)
    if kw.get('vessel_params') == 'thrust_loss':
        kw['vessel_params'] = np.asarray(ml4ca_amd.default_vessel('thrust_loss'), np.float32)
    a, _, _, _, _ = _fly('final_cont', n, 'f16', form, setup=setup, seed=11, **kw)
    assert bool((a['integ'] != 0).any())


@pytest.mark.parametrize('precision', ['f16', 'f32'])
@pytest.mark.parametrize('mode', ['limited', 'full'])
def test_limited_and_full_variants_replay_through_single_steps(mode, precision):
    a, _, _, _, _ = _fly(mode, 1000, precision, 'auto')
    assert all(_law_events(a, FAST))


def test_refusals_leave_the_handle_working():
    from ml4ca_amd import DpenvError, _lib
    from ml4ca_amd.policy import ActorCritic, policy_rollout
    import ctypes as C
    torch = torch_()
    n, T = 640, 8
    env, ref = _make('final_cont', n, 'f16', 'auto', seed=21)
    senv, _ = H.make_pair('simple', 64, ext=False)
    with pytest.raises(DpenvError, match='simple'):
        senv.set_integral_action()
    for bad in (dict(gain=(float('nan'), 0.05, 0.05)), dict(bound=(-0.5, 1.0, 0.1)), dict(box=(5.0, float('nan'), 1.0)), dict(dwell_s=-1.0)):
        with pytest.raises(DpenvError):
            env.set_integral_action(**bad)
    with pytest.raises(DpenvError, match='off'):
        env.get_integral_state()
    for e in (env, ref):
        e.reset()
    policy_rollout(ref, T, sample=True)                             # the lagged thrust columns of both handles are valid from here
    env.set_integral_action()
    act = torch.zeros((n, 7), device=env.device)
    with pytest.raises(ValueError, match='integral action'):
        env.step(act)
    with pytest.raises(ValueError, match='integral action'):
        env.rollout(torch.zeros((2, n, 7), device=env.device))
    o = torch.empty((n, 9), device=env.device)
    r = torch.empty(n, device=env.device)
    d = torch.empty(n, dtype=torch.uint8, device=env.device)
    rc = env.lib.dpenv_step(env._h, C.c_void_p(act.data_ptr()), None, C.c_void_p(o.data_ptr()), C.c_void_p(r.data_ptr()),
                            C.c_void_p(d.data_ptr()), env._stream())
    assert rc == _lib.EINVAL and b'integral action' in env.lib.dpenv_last_error(env._h)
    # unsupported shapes: refused with the supported set named
    for hidden, activation in (((96, 96), 'leaky'), ((64, 64), 'tanh')):
        ActorCritic(9, 7, hidden, seed=1, device=env.device, activation=activation).upload(env, precision='f16')
        with pytest.raises(DpenvError, match='width <= 80'):
            policy_rollout(env, T, sample=True)
    wenv, _ = H.make_pair('final_wrap', 64)
    ActorCritic(wenv.num_states, wenv.num_actions, (80, 80, 80), seed=1, device=wenv.device).upload(wenv)
    wenv.set_integral_action()
    wenv.reset()
    with pytest.raises(DpenvError, match='continuous angles'):
        policy_rollout(wenv, T, sample=True)
    # the handle still works: on, then off again -> the original kernels' rows exactly (from the same state as a handle never switched)
    ac = ActorCritic(9, 7, (80, 80, 80), seed=5, device=env.device)
    for e in (env, ref):
        ac.upload(e, precision='f16', launch_form='auto')
    on = policy_rollout(env, T, sample=True)
    assert bool(torch.isfinite(on['val']).all()) and 'integ' in on
    env.set_integral_action(None)
    with pytest.raises(DpenvError):
        env.get_integral_state()
    st, ctr = ref.get_state()
    env.set_state(st.clone(), ctr.clone())
    env.set_rng_counters(*[x.clone() for x in ref.get_rng_counters()])
    env.set_obs_thrust(ref.get_obs_thrust().clone())
    env_rows = policy_rollout(env, T, sample=True)
    ref_rows = policy_rollout(ref, T, sample=True)
    assert 'integ' not in env_rows
    for k in ('obs', 'act', 'val', 'logp', 'rew', 'done', 'boot', 'last_obs', 'last_val'):
        assert torch.equal(env_rows[k], ref_rows[k]), k


def test_thesis_checkpoint_flies_the_current_box_test_with_integral_action():
    """final_policy.npz (the thesis' trained actor) flies evaluate.deployment_box_test in a 0.2 m/s current from 16 directions, with
    and without the node's integral action.  Rows finite, |I| within the bounds, the integrator working at the corners.  IAE and work
    are printed, not asserted: the plant is build-owned and unpinned, so the size of the effect is not known."""
    import ml4ca_amd
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.policy import ActorCritic
    torch = torch_()
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'final_policy.npz'))
    n = 16
    env = ml4ca_amd.BatchedRevoltEnv(n, terminate=False, time_limit=False, current=True, seed=2)
    ActorCritic.from_tensors({k.replace('.', '/'): d[k] for k in d.files if '.' in k}, device=env.device).upload(env)
    env.set_current(torch.full((n,), 0.2, device=env.device), torch.arange(n, device=env.device, dtype=torch.float32) * (2 * math.pi / n))
    res = {}
    for integral in (False, True):
        r = EV.deployment_box_test(env, integral=integral)
        for k in ('e', 'integ', 'iae', 'work'):
            assert bool(torch.isfinite(r[k]).all()), k
        assert bool(torch.isfinite(r['out']['obs']).all())
        res[integral] = r
    I = res[True]['integ']
    bound = torch.tensor([0.5, 1.0, math.pi / 32], device=I.device)
    assert bool((I.abs() <= bound).all())
    steps = [int(round(t / env.dt)) for t in EV.BOX_TIMES[1:]] + [I.shape[0]]
    for t in steps:                                                 # at the end of each corner's dwell the integrator is active
        assert float((I[t - 1].abs().sum(-1) > 0).float().mean()) > 0.5, t
    assert bool((res[False]['integ'] == 0).all())
    for integral in (False, True):
        r = res[integral]
        print('deployment box test, 0.2 m/s current from %d directions, integral action %-3s: IAE %.2f (min %.2f, max %.2f), '
              'work W* bow/port/star %s' % (n, 'on' if integral else 'off', float(r['iae'].mean()), float(r['iae'].min()),
                                            float(r['iae'].max()), [round(float(x), 1) for x in r['work'].mean(0)]))
