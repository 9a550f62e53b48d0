#!/usr/bin/env python3
"""Times the PPO update both ways on one GPU: torch autograd + torch.optim.Adam (the loop of examples/train_ppo.py, the baseline) against
the fused kernels (ml4ca_amd/train.py).  One process, device events, the two arms alternating, medians of 20.

    python tools/time_ppo_update.py [--envs 4096] [--steps 400] [--out profiles/ppo_update_timing.txt]

Measured: one actor step and one critic step (gradient + Adam) on a 2^18-row minibatch and on the full batch, and a whole 80 + 80
update with the KL gate open.  The rows are synthetic (normal observations, actions drawn from the policy, |log ratio| small): the
time of a step does not depend on the values."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ml4ca_amd import train as TR
from ml4ca_amd.policy import ActorCritic


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, reps=20):
    """{name: median ms} of the arms run in turn, `reps` times each after one warm-up round."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ts[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--minibatch', type=int, default=1 << 18)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--update-reps', type=int, default=3)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    spec = importlib.util.spec_from_file_location('train_ppo_example', os.path.join(ROOT, 'examples', 'train_ppo.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    N = args.envs * args.steps
    ac_t = ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=0, device=dev)
    ac_f = ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=0, device=dev)
    obs = torch.randn(N, 9, device=dev)
    with torch.no_grad():
        mu, _ = ac_t.forward_ref(obs)
        act = mu + torch.exp(ac_t.log_std) * torch.randn(N, 7, device=dev)
        logp_old = ac_t.logp_ref(act, mu) + 0.001 * torch.randn(N, device=dev)
    adv, ret = torch.randn(N, device=dev), torch.randn(N, device=dev)
    for p in ac_t.parameters():
        p.requires_grad_(True)
    pi_params, v_params = ac_t.pi_W + ac_t.pi_b + [ac_t.log_std], ac_t.v_W + ac_t.v_b
    pi_opt, v_opt = torch.optim.Adam(pi_params, lr=3e-4), torch.optim.Adam(v_params, lr=1e-3)
    upd = TR.PPOUpdater(ac_f, target_kl=1e9)                     # the gate stays open: every step is taken in both arms
    lines = ['PPO update, %d envs x %d steps = %d rows; medians of %d, arms alternating; ms' % (args.envs, args.steps, N, args.reps)]

    def torch_actor(idx):
        mu = ac_t._mlp(obs[idx], ac_t.pi_W, ac_t.pi_b)
        logp = ac_t.logp_ref(act[idx], mu)
        ratio = torch.exp(logp - logp_old[idx])
        a = adv[idx]
        loss = -torch.min(ratio * a, torch.clamp(ratio, 0.8, 1.2) * a).mean()
        pi_opt.zero_grad()
        loss.backward()
        pi_opt.step()

    def torch_critic(idx):
        v = ac_t._mlp(obs[idx], ac_t.v_W, ac_t.v_b)[:, 0]
        loss = ((ret[idx] - v) ** 2).mean()
        v_opt.zero_grad()
        loss.backward()
        v_opt.step()

    b1, b2 = upd.betas
    for mb in (min(args.minibatch, N), N):
        idx64 = torch.randint(0, N, (mb,), device=dev) if mb < N else slice(None)
        idx32 = idx64.to(torch.int32) if mb < N else None
        ws = upd._workspace(mb)

        def fused_actor():
            TR.ppo_actor_grad(upd.pi_theta, obs, act, adv, logp_old, 0.2, idx=idx32, out=upd.pi_grad, workspace=ws, leak=0.2, stop_flag=upd.stop, count=mb)
            TR.adam_step(upd.pi_theta, upd.pi_grad, upd.pi_m, upd.pi_v, upd.pi_steps, 3e-4, b1, b2, 1e-8, gate_kl=upd.pi_grad[14335:14336], kl_limit=1e9,
                         stop_flag=upd.stop)

        def fused_critic():
            TR.value_grad(upd.v_theta, obs, ret, idx=idx32, out=upd.v_grad, workspace=ws, leak=0.2, count=mb)
            TR.adam_step(upd.v_theta, upd.v_grad, upd.v_m, upd.v_v, upd.v_steps, 1e-3, b1, b2, 1e-8)

        for name, arms in (('actor step', {'torch': lambda: torch_actor(idx64), 'fused': fused_actor}),
                           ('critic step', {'torch': lambda: torch_critic(idx64), 'fused': fused_critic})):
            t = alternate(arms, args.reps)
            lines.append('%-12s %8d rows  torch %8.3f  fused %8.3f  ratio %.2f' % (name, mb, t['torch'], t['fused'], t['torch'] / t['fused']))
            print(lines[-1], flush=True)
    mb = min(args.minibatch, N)
    arms = {'torch': lambda: ex.torch_update(ac_t, pi_opt, v_opt, pi_params, v_params, obs, act, adv, ret, logp_old, mb, 0.2, 1e9, False),
            'fused': lambda: upd.update(obs, act, adv, ret, logp_old, iters=80, minibatch=mb)}
    t = alternate(arms, args.update_reps)
    lines.append('%-12s %8d rows  torch %8.1f  fused %8.1f  ratio %.2f   (80 + 80 steps, index draws and the final read included; median of %d)' % (
        'whole update', mb, t['torch'], t['fused'], t['torch'] / t['fused'], args.update_reps))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
