#!/usr/bin/env python3
"""Times one imitation step (gradient + Adam) of both losses on one GPU against the PPO actor step on the same rows, and against torch
autograd + torch.optim.Adam of the same losses.  One process, device events, the arms alternating, medians of 20.

    python tools/time_imitation.py [--envs 4096] [--steps 400] [--out profiles/imitation_timing.txt]

The yardstick is the existing dpenv_ppo_actor_grad step measured beside the new ones in the same call: the imitation kernels share
everything with it but the per-row output stage, which does less.  The rows are synthetic (normal observations, actions drawn from the
policy): the time of a step does not depend on the values."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ml4ca_amd import train as TR
from ml4ca_amd.policy import ActorCritic
from time_ppo_update import alternate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--minibatch', type=int, default=1 << 18)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    N = args.envs * args.steps
    ac_t = ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=0, device=dev)
    ac_f = ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=0, device=dev)
    obs = torch.randn(N, 9, device=dev)
    with torch.no_grad():
        mu, _ = ac_t.forward_ref(obs)
        act = mu + torch.exp(ac_t.log_std) * torch.randn(N, 7, device=dev)
        logp_old = ac_t.logp_ref(act, mu) + 0.001 * torch.randn(N, device=dev)
    adv, weight = torch.randn(N, device=dev), 2.0 * torch.rand(N, device=dev)
    for p in ac_t.parameters():
        p.requires_grad_(True)
    pi_params = ac_t.pi_W + ac_t.pi_b + [ac_t.log_std]
    pi_opt = torch.optim.Adam(pi_params, lr=3e-4)
    upd = TR.PPOUpdater(ac_f, target_kl=1e9)
    b1, b2 = upd.betas
    mb = min(args.minibatch, N)
    idx64 = torch.randint(0, N, (mb,), device=dev) if mb < N else slice(None)
    idx32 = idx64.to(torch.int32) if mb < N else None
    ws = upd._workspace(mb)

    def adam():
        TR.adam_step(upd.pi_theta, upd.pi_grad, upd.pi_m, upd.pi_v, upd.pi_steps, 3e-4, b1, b2, 1e-8)

    def fused_ppo():
        TR.ppo_actor_grad(upd.pi_theta, obs, act, adv, logp_old, 0.2, idx=idx32, out=upd.pi_grad, workspace=ws, leak=0.2, count=mb)
        adam()

    def fused(loss, w):
        def run():
            TR.imitation_grad(upd.pi_theta, obs, act, loss=loss, weight=w, idx=idx32, out=upd.pi_grad, workspace=ws, leak=0.2, count=mb)
            adam()
        return run

    def torch_arm(loss):
        def run():
            mu = ac_t._mlp(obs[idx64], ac_t.pi_W, ac_t.pi_b)
            w = weight[idx64]
            L = (w * ((mu - act[idx64]) ** 2).sum(dim=1)).mean() if loss == 'mse' else -(w * ac_t.logp_ref(act[idx64], mu)).mean()
            pi_opt.zero_grad()
            L.backward()
            pi_opt.step()
        return run

    arms = {'ppo actor step (fused, the yardstick)': fused_ppo,
            'imitation nll, weighted (fused)': fused('nll', weight), 'imitation mse, weighted (fused)': fused('mse', weight),
            'imitation nll, no weights (fused)': fused('nll', None), 'imitation mse, no weights (fused)': fused('mse', None),
            'imitation nll, weighted (torch)': torch_arm('nll'), 'imitation mse, weighted (torch)': torch_arm('mse')}
    t = alternate(arms, args.reps)
    base = t['ppo actor step (fused, the yardstick)']
    lines = ['imitation step (gradient + Adam), %d envs x %d steps = %d rows, minibatch %d rows; medians of %d, arms alternating; ms' % (
        args.envs, args.steps, N, mb, args.reps)]
    for k, v in t.items():
        lines.append('%-40s %8.3f   x %.3f of the PPO actor step' % (k, v, v / base))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
