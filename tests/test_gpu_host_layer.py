"""The Python host layer's shared fronts on the device: the block checks policy_rollout shares with controller_rollout (env._blocks),
the setpoint schedule all three row-block launches share (env._schedule), and the per-env state accessors (env._get / env._set)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOO_MANY = 'at most 8 setpoint switches per rollout launch'


def torch_():
    import torch
    return torch


def _env(n, actor=True, **kw):
    import ml4ca_amd
    from ml4ca_amd.policy import ActorCritic
    env = ml4ca_amd.BatchedRevoltEnv(n, device='cuda:0', seed=3, **kw)
    if actor:
        ActorCritic(9, 7, (80, 80, 80), seed=1, device=env.device).upload(env)
    env.reset()
    return env


def _policy_blocks(env, T):
    torch = torch_()
    n, od, ad, dev, f32 = env.n_envs, env.num_states, env.num_actions, env.device, torch.float32
    e = lambda shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
    return dict(obs=e((T, n, od)), act=e((T, n, ad)), rew=e((T, n)), val=e((T, n)), logp=e((T, n)), boot=e((T, n)),
                done=e((T, n), torch.uint8), last_obs=e((n, od)), last_val=e((n,)))


def test_policy_rollout_refuses_a_wrong_block_and_launches_nothing():
    from ml4ca_amd.policy import policy_rollout
    torch = torch_()
    n, T = 64, 2
    a, b = _env(n), _env(n)
    for env in (a, b):
        env.set_reference_filter()
    dev = a.device
    bad = dict(act=torch.empty((T + 1, n, 7), device=dev),                               # T + 1 rows
               done=torch.empty((T, n), dtype=torch.float32, device=dev),                # float32, not uint8
               last_obs=torch.empty((9, n), device=dev).t(),                             # [n, 9], not contiguous
               ref=torch.empty((T, n, 4), device=dev))                                   # the filter is on: [T, n, 3] wanted
    assert not bad['last_obs'].is_contiguous() and tuple(bad['last_obs'].shape) == (n, 9)
    for key, block in bad.items():
        out = _policy_blocks(a, T)
        out[key] = block
        with pytest.raises(ValueError, match=re.escape("out['%s']" % key)):
            policy_rollout(a, T, out=out)
    got = policy_rollout(a, T, out=_policy_blocks(a, T))
    want = policy_rollout(b, T)
    assert set(got) == set(want) and 'ref' in got
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    for u, v in zip(a.get_state(), b.get_state()):
        assert torch.equal(u, v)
    torch.cuda.synchronize()


def _refs(env, k):
    torch = torch_()
    g = torch.Generator().manual_seed(9)
    r = (torch.rand((k, 3, env.n_envs), generator=g) * 2 - 1) * torch.tensor([1.0, 1.0, 0.2])[None, :, None]
    return r.to(env.device).contiguous()


@pytest.mark.parametrize('who', ['policy_rollout', 'controller_rollout'])
def test_nine_switches_are_refused_and_eight_fly_as_env_rollout_flies_them(who):
    from ml4ca_amd import policy
    torch = torch_()
    n, T = 64, 9
    env = _env(n, terminate=False)
    env.set_dp_controller()
    launch = getattr(policy, who)
    with pytest.raises(ValueError, match=TOO_MANY):
        launch(env, T, switch_steps=tuple(range(9)), refs=_refs(env, 9))
    with pytest.raises(ValueError, match=TOO_MANY):
        env.rollout(torch.zeros((T, n, 7), device=env.device), switch_steps=tuple(range(9)), refs=_refs(env, 9))
    steps, refs = tuple(range(8)), _refs(env, 8)
    st, ctr = env.get_state()
    out = launch(env, T, switch_steps=steps, refs=refs)
    st1, ctr1 = env.get_state()
    env.set_state(st, ctr)
    obs, rew, done = env.rollout(out['act'], switch_steps=steps, refs=refs)
    assert torch.equal(obs[:-1], out['obs'][1:]) and torch.equal(obs[-1], out['last_obs'])
    assert torch.equal(rew, out['rew']) and torch.equal(done, out['done'])
    st2, ctr2 = env.get_state()
    assert torch.equal(st1, st2) and torch.equal(ctr1, ctr2)
    assert not torch.equal(st[6:9], st2[6:9])                                            # the setpoints did move
    torch.cuda.synchronize()


def _values(shape, dtype, seed, scale):
    """Distinct, moderate values of that shape and dtype (a CPU tensor)."""
    torch = torch_()
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int32:
        return torch.randint(0, 1000, shape, generator=g, dtype=torch.int32)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _round_trip(env, name, get, set_, specs, scale=0.25, seed=0):
    """set distinct values, get them back bit for bit with shape and dtype; a wrong shape and a wrong dtype raise from the setter."""
    torch = torch_()
    vals = [_values(shape, dtype, seed + j, scale).to(env.device).contiguous() for j, (shape, dtype) in enumerate(specs)]
    set_(*vals)
    got = get()
    got = (got,) if isinstance(got, torch.Tensor) else got
    assert len(got) == len(vals), name
    for g, v in zip(got, vals):
        assert g.dtype == v.dtype and tuple(g.shape) == tuple(v.shape) and torch.equal(g, v), name
    for j, (shape, dtype) in enumerate(specs):
        wide = torch.zeros(tuple(shape[:-1]) + (shape[-1] + 1,), dtype=dtype, device=env.device)
        other = torch.zeros(shape, dtype=torch.float64 if dtype == torch.float32 else torch.int64, device=env.device)
        for wrong in (wide, other):
            args = list(vals)
            args[j] = wrong
            with pytest.raises(ValueError, match='must be a contiguous'):
                set_(*args)
    again = get()
    again = (again,) if isinstance(again, torch.Tensor) else again
    assert all(torch.equal(g, v) for g, v in zip(again, vals)), '%s: a refused set changed the state' % name
    return vals


def test_every_accessor_pair_round_trips_at_a_ragged_n():
    import ml4ca_amd
    torch = torch_()
    n = 65
    f32, i32 = torch.float32, torch.int32
    env = _env(n, current=True)
    env.set_integral_action()
    env.set_reference_filter()
    _round_trip(env, 'state', env.get_state, env.set_state, (((15, n), f32), ((2, n), i32)))
    _round_trip(env, 'integral_state', env.get_integral_state, env.set_integral_state, (((3, n), f32), ((n,), i32)), seed=10)
    _round_trip(env, 'reference_filter_state', env.get_reference_filter_state, env.set_reference_filter_state,
                (((9, n), f32), ((3, n), f32)), seed=20)
    _round_trip(env, 'rng_counters', env.get_rng_counters, env.set_rng_counters, (((n,), i32), ((n,), i32)), seed=30)
    _round_trip(env, 'obs_thrust', env.get_obs_thrust, env.set_obs_thrust, (((n, 4), f32),), seed=40)
    # the current: speeds are positive; set_current gives the present values and the means, present_only the present values alone
    vc =(_values((n,), f32, 50, 0.25).abs() + 0.05).to(env.device)
    beta = _values((n,), f32, 51, 3.0).to(env.device)
    _round_trip_current(env, vc, beta)
    # per-env hulls: the default hull, every parameter moved by up to 10 %
    hull = torch.as_tensor(np.asarray(ml4ca_amd.default_vessel(), np.float32))[:, None]
    hulls = (hull * (1.0 + _values((32, n), f32, 60, 0.1))).to(env.device).contiguous()
    env.set_vessel_params(hulls)
    got = env.get_vessel_params()
    assert got.dtype == f32 and tuple(got.shape) == (32, n) and torch.equal(got, hulls)
    for wrong in (hulls[:, :-1].contiguous(), hulls.double()):
        with pytest.raises(ValueError, match='must be a contiguous'):
            env.set_vessel_params(wrong)
    # the baseline's integral and the QP allocator's thruster state (shared hull)
    env2 = _env(n, actor=False)
    env2.set_dp_controller()
    env2.set_qp_allocator()
    _round_trip(env2, 'dp_controller_state', env2.get_dp_controller_state, env2.set_dp_controller_state, (((3, n), f32),), seed=70)
    _round_trip(env2, 'qp_allocator_state', env2.get_qp_allocator_state, env2.set_qp_allocator_state, (((5, n), f32),), seed=80)
    torch.cuda.synchronize()


def _round_trip_current(env, vc, beta):
    torch = torch_()
    n = env.n_envs
    env.set_current(vc, beta)
    for got in (env.get_current(), env.get_current_mean()):
        assert all(g.dtype == torch.float32 and tuple(g.shape) == (n,) for g in got)
        assert torch.equal(got[0], vc) and torch.equal(got[1], beta)
    vc2, beta2 = (vc * 0.5).contiguous(), (beta * 0.5).contiguous()
    env.set_current(vc2, beta2, present_only=True)
    got, mean = env.get_current(), env.get_current_mean()
    assert torch.equal(got[0], vc2) and torch.equal(got[1], beta2) and torch.equal(mean[0], vc) and torch.equal(mean[1], beta)
    for present_only in (False, True):
        for args in ((vc[:-1].contiguous(), beta), (vc, beta.double())):
            with pytest.raises(ValueError, match='must be a contiguous'):
                env.set_current(*args, present_only=present_only)
