#!/usr/bin/env python
"""One sha256 per named result of the Python host layer (env.py, policy.py, train.py, deploy.py, evaluate.py, rollout.py) on one fixed
small scenario: what a change of that layer alone must leave bit for bit.

    python tools/host_layer_bits.py [--package-dir DIR] [--lib PATH] [--time]

The package is imported from DIR (default: this checkout), the kernel library from PATH (default: the package's own lib/), so that two
versions of ml4ca_amd/*.py - say `git archive <parent> ml4ca_amd | tar -x -C DIR` - run against ONE built library in one session.  Run a
version twice first: a key whose hash differs between two runs of one version is not deterministic and says nothing.
--time: instead, microseconds per call of policy_rollout(env, 1, out=out) and controller_rollout(env, 1, out=out) at n = 64 over
2 000 calls with one synchronise at the end - host-bound at that size.  profiles/host_layer_bits.txt holds a listing of both."""
import argparse
import hashlib
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--package-dir', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--lib', default=None)
ap.add_argument('--time', action='store_true')
args = ap.parse_args()
if args.lib:
    os.environ['DPENV_LIB'] = os.path.abspath(args.lib)
sys.path.insert(0, os.path.abspath(args.package_dir))

import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import ml4ca_amd                                           # noqa: E402
from ml4ca_amd import deploy, evaluate, policy, rollout, train   # noqa: E402

assert os.path.abspath(os.path.dirname(ml4ca_amd.__file__)) == os.path.join(os.path.abspath(args.package_dir), 'ml4ca_amd')
N, T, DEV = 128, 8, 'cuda:0'


def digest(h, v):
    """Feed a result into the hash: tensors and arrays as dtype, shape and bytes; containers in order (dicts by sorted key)."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu()
        v = v.view(torch.int16).numpy() if v.dtype == torch.bfloat16 else v.numpy()
    if isinstance(v, np.ndarray):
        h.update(('%s%s' % (v.dtype, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            h.update(str(k).encode())
            digest(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b'[%d' % len(v))
        for x in v:
            digest(h, x)
    elif isinstance(v, evaluate.ScoreCard):
        digest(h, v.totals())
    else:
        h.update(repr(v).encode())


def show(name, value):
    h = hashlib.sha256()
    digest(h, value)
    print('%-44s %s' % (name, h.hexdigest()), flush=True)


def make_env(n=N, seed=3, **kw):
    env = ml4ca_amd.BatchedRevoltEnv(n, device=DEV, seed=seed, **kw)
    env.reset()
    return env


def actor(env, seed=1, precision='f32'):
    return policy.ActorCritic(9, 7, (80, 80, 80), seed=seed, device=env.device).upload(env, precision=precision)


def refs_for(env, k, seed=9):
    g = torch.Generator().manual_seed(seed)
    r = (torch.rand((k, 3, env.n_envs), generator=g) * 2 - 1) * torch.tensor([1.0, 1.0, 0.2])[None, :, None]
    return r.to(env.device).contiguous()


def rollouts():
    env = make_env(auto_reset=True, max_ep_len=5)
    actor(env)
    env.set_dp_controller()
    sw, refs = (2, 5), refs_for(env, 2)
    out = policy.policy_rollout(env, T, switch_steps=sw, refs=refs, sample=True)
    show('policy_rollout', out)
    show('policy_rollout state', env.get_state())
    show('env.rollout', env.rollout(out['act'].clone(), switch_steps=sw, refs=refs))
    show('controller_rollout', policy.controller_rollout(env, T, switch_steps=sw, refs=refs))
    env.set_reference_filter()
    env.set_integral_action()
    show('policy_rollout deployed', policy.policy_rollout(env, T, switch_steps=sw, refs=refs, reset_at_end=True))
    env.set_integral_action(None)
    show('controller_rollout filtered', policy.controller_rollout(env, T, switch_steps=sw, refs=refs))
    env.set_reference_filter(None)
    env.set_integral_action()
    show('policy_rollout integral', policy.policy_rollout(env, T))
    return out


def labels(block):
    env = make_env(seed=4)
    env.set_dp_controller()
    obs, done, flown = block['obs'], block['done'], block['act']
    z = 0.1 * refs_for(env, 1, seed=2)[0]
    x = 0.5 * torch.cat([refs_for(env, 1, seed=5)[0], refs_for(env, 1, seed=6)[0][:2]]).contiguous()
    qp = deploy.qp_allocator_defaults()
    table = torch.as_tensor(deploy.qp_allocator_table(N, qp)).to(env.device)
    net = policy.nn_net_to(train_net(), env.device)
    show('controller_label', policy.controller_label(env, obs, done, z=z))
    show('controller_label_qp', policy.controller_label_qp(env, obs, done, z=z, x=x, params=qp, cost=True))
    show('controller_label_qp flown + table', policy.controller_label_qp(env, obs, done, z=z, x=x, flown=flown, table=table, iterations=8,
                                                                         refused=torch.zeros(N, dtype=torch.uint8, device=env.device)))
    show('controller_label_nn', policy.controller_label_nn(env, obs, done, z=z, net=net, raw=True, tau=True))
    show('controller_label_nn wrench only', policy.controller_label_nn(env, obs, done, z=z, act=False, tau=True))
    host = [a.cpu().numpy() for a in (obs[:4, :8], done[:4, :8], z[:, :8], x[:, :8])]
    show('deploy.label_rows', deploy.label_rows(None, host[0], host[1], host[2], dt=env.control_period))
    show('deploy.label_rows_qp', deploy.label_rows_qp(None, qp, *host, dt=env.control_period))
    show('deploy.label_rows_nn', deploy.label_rows_nn(None, {k: ([t.cpu().numpy() for t in v] if k in 'Wb' else v) for k, v in net.items()},
                                                      host[0], host[1], host[2], dt=env.control_period))


def train_net():
    th = train.nn_allocator_init(9, 5)
    W, b, _ = train.unflatten(th, 9, 6, True)
    return dict(W=list(W), b=list(b), leak=0.2)


def accessors():
    env = make_env(seed=6, current=True, current_drift=True)
    actor(env)
    env.set_integral_action()
    env.set_reference_filter()
    policy.policy_rollout(env, T, switch_steps=(1,), refs=refs_for(env, 1), sample=True)
    pairs = (('state', env.get_state, env.set_state), ('integral_state', env.get_integral_state, env.set_integral_state),
             ('reference_filter_state', env.get_reference_filter_state, env.set_reference_filter_state),
             ('rng_counters', env.get_rng_counters, env.set_rng_counters), ('current', env.get_current, env.set_current))
    for name, get, set_ in pairs:
        v = get()
        show('get_' + name, v)
        set_(*[t.flip(-1).contiguous() for t in v])
        show('set_%s, get' % name, get())
    show('get_current_mean', env.get_current_mean())
    t = env.get_obs_thrust()
    show('get_obs_thrust', t)
    env.set_obs_thrust(t.flip(0).contiguous())
    show('set_obs_thrust, get', env.get_obs_thrust())
    show('get_vessel_params', env.get_vessel_params())
    env2 = make_env(seed=7)
    env2.set_dp_controller()
    env2.set_qp_allocator()
    policy.controller_rollout(env2, T)
    for name, get, set_ in (('dp_controller_state', env2.get_dp_controller_state, env2.set_dp_controller_state),
                            ('qp_allocator_state', env2.get_qp_allocator_state, env2.set_qp_allocator_state)):
        v = get()
        show('get_' + name, v)
        set_(v.flip(-1).contiguous())
        show('set_%s, get' % name, get())


def updates(block):
    env = make_env(seed=8, auto_reset=True)
    ac = policy.ActorCritic(9, 7, (80, 80, 80), seed=2, device=env.device)
    up = train.PPOUpdater(ac)
    adv, ret = rollout.gae(block['rew'], block['val'], end=block['done'], boot=block['boot'])
    flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:])).contiguous()
    obs, act, adv, ret, logp = (flat(t) for t in (block['obs'], block['act'], adv, ret, block['logp']))
    torch.manual_seed(11)
    show('PPOUpdater.update', (up.update(obs, act, adv, ret, logp, iters=3, minibatch=32), up.pi_theta, up.v_theta, up.pi_m, up.v_v))
    show('PPOUpdater.update, every row', (up.update(obs, act, adv, ret, logp, iters=2), up.pi_theta, up.v_theta))
    show('PPOUpdater.pretrain', (up.pretrain(obs, act, 3, minibatch=32), up.pi_theta, up.pi_m, up.pi_steps, up._pi_steps_host))
    show('PPOUpdater.pretrain kept', (up.pretrain(obs, act, 2, loss='nll', keep_optimizer_state=True), up.pi_theta, up.pi_steps,
                                      up._pi_steps_host))
    show('PPOUpdater.pretrain_critic', (up.pretrain_critic(obs, ret, 3, minibatch=32), up.v_theta, up.v_m, up.v_steps))
    env.set_dp_controller()
    table = torch.as_tensor(deploy.qp_allocator_table(N)).to(env.device)
    for name, kw in (('pinv', {}), ('qp', dict(expert='qp', thruster_state='flown', qp_table=table)),
                     ('nn', dict(expert='nn', nn_net=policy.nn_net_to(train_net(), env.device)))):
        env.reset()
        rec = up.dagger(env, 3, 4, 2, minibatch=64, keep=2, upload=dict(precision='f32'), reset_at_end=(name == 'qp'), **kw)
        show('PPOUpdater.dagger ' + name, (rec, up.pi_theta, up.dagger_data))


def fits():
    ds = deploy.nn_allocator_dataset(512, 3)
    for loss in ('mse', 'wrench'):
        fit = train.fit_nn_allocator(ds, iters=3, minibatch=64, seed=1, device=DEV, loss=loss)
        show('fit_nn_allocator ' + loss, fit)
    env = make_env(seed=9)
    env.set_dp_controller()
    show('fit_nn_allocator_on_policy', train.fit_nn_allocator_on_policy(env, 2, 4, 2, base=ds, keep=1, minibatch=64))
    return fit


def box_tests(net):
    for wear in (False, True):
        for filt in (False, True):
            tag = '%s%s' % (' filtered' if filt else '', ' wear' if wear else '')
            env = make_env(seed=10, current=True)
            actor(env)
            res = evaluate.deployment_box_test(env, T=30, reference_filter=filt, wear=wear)
            show('deployment_box_test' + tag, res)
            res = evaluate.deployment_box_test_streamed(env, T=30, chunk=7, reference_filter=filt, wear=wear)
            show('deployment_box_test_streamed' + tag, res)
            for alloc in ('pinv', 'qp', 'nn'):
                kw = dict(allocator=alloc, net=net if alloc == 'nn' else None)
                show('baseline_box_test %s%s' % (alloc, tag), evaluate.baseline_box_test(env, T=30, reference_filter=filt, wear=wear, **kw))
                show('baseline_box_test_streamed %s%s' % (alloc, tag),
                     evaluate.baseline_box_test_streamed(env, T=30, chunk=7, reference_filter=filt, wear=wear, **kw))


def timing():
    env = make_env(64)
    actor(env, precision='f16')
    env.set_dp_controller()
    for name, launch in (('policy_rollout', policy.policy_rollout), ('controller_rollout', policy.controller_rollout)):
        out = launch(env, 1)
        for _ in range(200):
            launch(env, 1, out=out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2000):
            launch(env, 1, out=out)
        torch.cuda.synchronize()
        print('%-44s %.3f us per call' % (name + '(env, 1, out=out), n = 64', (time.perf_counter() - t0) / 2000 * 1e6), flush=True)


if args.time:
    timing()
else:
    torch.manual_seed(0)
    np.random.seed(0)
    blk = rollouts()
    labels(blk)
    accessors()
    updates(blk)
    box_tests(fits())
torch.cuda.synchronize()
