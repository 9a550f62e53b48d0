#!/usr/bin/env python3
"""Cost of the neural thrust allocation, alone (dpenv_thrust_alloc_nn / policy.thrust_alloc_nn) and as the allocation stage of the fused
closed loop (dpenv_set_nn_allocator + dpenv_controller_rollout), beside the pseudo-inverse and the 16-iteration QP in the same process:
device events, warmed-up shapes, launch spacing over batches of 20 back-to-back launches, arms alternating batch by batch, medians of 7
batches (tools/time_qp_alloc.py's scheme).  Workload: 65 536 envs; launches of T = 50 steps with auto-reset on.

  A  thrust_alloc_nn, the reference's 9-20-20-20-20-6 relu shape and the fitted 9-80-80-80-6 leaky shape (weights read in place).
  B  thrust_alloc, the stateless pseudo-inverse allocation, on the same wrenches.
  C  controller_rollout with the pseudo-inverse, T = 50: the yardstick of the closed loop.
  D  controller_rollout with the QP allocation at K = 16.
  E  controller_rollout with the neural allocation, both shapes.
  F  env.set_nn_allocator with device tensors: the packing launch, per call.
  G  train.fit_nn_allocator on 4 096 dataset rows, per count of --fit Adam steps: the loss before and after, and the fitted network on the calm
     250 s box test (64 envs) beside the pseudo-inverse and the QP.

  --population K [K ...]: instead of the legs above, the closed loop with a POPULATION of K networks (dpenv_set_nn_allocator_population,
     one network per 64 envs, distinct random weights) per K and shape beside the one-network launch of the same build, the handle-free
     map with K stacked networks, and the K-network packing launch (env.set_nn_allocator_population from device tensors); written to
     profiles/nn_population_timing.txt unless --out says otherwise.

Usage: python tools/time_nn_alloc.py [--out profiles/nn_alloc_timing.txt] [--envs 65536] [--fit 200 5000] [--population 1 16 256 1024]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import ml4ca_amd
from ml4ca_amd import evaluate
from ml4ca_amd.deploy import nn_allocator_dataset, qp_allocator_defaults
from ml4ca_amd.policy import controller_rollout, nn_net_to, nn_population_to, thrust_alloc_nn, thrust_alloc_nn_population
from ml4ca_amd.train import fit_nn_allocator
from tools.time_qp_alloc import spacing_us

SHAPES = (((9, 20, 20, 20, 20, 6), 0.0), ((9, 80, 80, 80, 6), 0.2))


def glorot(sizes, leak, dev, seed=0):
    rng = np.random.RandomState(seed)
    W = [rng.uniform(-1, 1, size=(a, b)).astype(np.float32) * np.float32(np.sqrt(6.0 / (a + b))) for a, b in zip(sizes[:-1], sizes[1:])]
    return nn_net_to(dict(W=W, b=[np.zeros(b, np.float32) for b in sizes[1:]], leak=leak), dev)


def population_leg(args, dev, out):
    n, T = args.envs, 50
    rng = np.random.default_rng(0)
    tau = torch.from_numpy((rng.normal(0.0, 1.0, (3, n)) * np.array([[20.0], [10.0], [15.0]])).astype(np.float32)).to(dev)
    act = torch.empty((n, 7), device=dev)
    out('%d envs (%d waves), envs_per_net = 64, T = %d, launch spacing over 20 back-to-back launches, medians of 7 batches, arms alternating:'
        % (n, (n + 63) // 64, T))
    for sizes, leak in SHAPES:
        name = '-'.join(map(str, sizes))
        one = glorot(sizes, leak, dev)
        pops = [nn_population_to([glorot(sizes, leak, 'cpu', seed=k) for k in range(K)], dev) for K in args.population]
        fly, envs = None, []
        for st in [None] + pops:
            env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5)
            env.set_dp_controller()
            if st is None:
                env.set_nn_allocator(one)
            else:
                env.set_nn_allocator_population(st)
            env.reset()
            if fly is None:
                fly = {k: torch.empty_like(v) for k, v in controller_rollout(env, T).items()}
            envs.append(env)
        arms = [lambda env=env: controller_rollout(env, T, out=fly) for env in envs]
        arms.append(lambda: thrust_alloc_nn(tau, one, out=act))
        arms += [lambda st=st: thrust_alloc_nn_population(tau, st, out=act) for st in pops]
        arms.append(lambda: envs[0].set_nn_allocator(one))
        arms += [lambda env=env, st=st: env.set_nn_allocator_population(st) for env, st in zip(envs[1:], pops)]
        us = spacing_us(arms)
        m = len(pops)
        floats = sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:]))
        out('  network %s, leak %.1f (%d weights = %.1f KB per network)' % (name, leak, floats, floats * 4 / 1024.0))
        out('    controller_rollout, one network                 %9.1f us per launch = %.2f us per step' % (us[0], us[0] / T))
        for K, u in zip(args.population, us[1:1 + m]):
            out('    controller_rollout, population K = %-5d        %9.1f us per launch = %.2f us per step  x %.3f of one network'
                % (K, u, u / T, u / us[0]))
        out('    thrust_alloc_nn, one network                    %9.1f us per call' % us[1 + m])
        for K, u in zip(args.population, us[2 + m:2 + 2 * m]):
            out('    thrust_alloc_nn_population, K = %-5d           %9.1f us per call  x %.3f of one network' % (K, u, u / us[1 + m]))
        out('    set_nn_allocator from device tensors            %9.1f us per call (one packing launch)' % us[2 + 2 * m])
        for K, u in zip(args.population, us[3 + 2 * m:]):
            out('    set_nn_allocator_population, K = %-5d          %9.1f us per call (one packing launch, %.1f MB image)'
                % (K, u, K * sum(a * ((b + 15) // 16 * 16) + (b + 15) // 16 * 16 for a, b in zip(sizes[:-1], sizes[1:])) * 4 / 1e6))
        del envs, arms, pops
        torch.cuda.empty_cache()


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--population', type=int, nargs='+', default=None, help='time populations of K networks instead of the legs A..G')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--fit', type=int, nargs='*', default=[200], help='Adam steps of the fit(s) in leg G (none = skip the leg)')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(here, 'profiles', 'nn_population_timing.txt' if args.population else 'nn_alloc_timing.txt')
    dev = torch.device('cuda', 0)
    n, T = args.envs, 50
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_nn_alloc.py on %s' % torch.cuda.get_device_name(dev))
    if args.population:
        population_leg(args, dev, out)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    rng = np.random.default_rng(0)
    tau = torch.from_numpy((rng.normal(0.0, 1.0, (3, n)) * np.array([[20.0], [10.0], [15.0]])).astype(np.float32)).to(dev)
    nets = [glorot(s, leak, dev) for s, leak in SHAPES]
    act = torch.empty((n, 7), device=dev)
    arms = [lambda net=net: thrust_alloc_nn(tau, net, out=act) for net in nets]
    arms.append(lambda: ml4ca_amd.thrust_alloc(tau))
    fly, envs = None, []
    for kind in ('pinv', 'qp', 0, 1):
        env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5)
        env.set_dp_controller()
        if kind == 'qp':
            env.set_qp_allocator(dict(qp_allocator_defaults(), iterations=16))
        elif kind != 'pinv':
            env.set_nn_allocator(nets[kind])
        env.reset()
        if fly is None:
            fly = {k: torch.empty_like(v) for k, v in controller_rollout(env, T).items()}
        envs.append(env)
        arms.append(lambda env=env: controller_rollout(env, T, out=fly))
    arms.append(lambda: envs[3].set_nn_allocator(nets[1]))
    us = spacing_us(arms)
    step = [u / T for u in us[3:7]]
    out('%d envs, launch spacing over 20 back-to-back launches, medians of 7 batches, arms alternating:' % n)
    for (s, leak), u in zip(SHAPES, us[0:2]):
        out('  A thrust_alloc_nn %-22s leak %.1f   %8.1f us per control step  x %.1f of B  x %.2f of a C step' % (
            '-'.join(map(str, s)), leak, u, u / us[2], u / step[0]))
    out('  B thrust_alloc (pseudo-inverse, stateless)          %8.1f us per call' % us[2])
    out('  C controller_rollout, pseudo-inverse, T = %d        %8.1f us per launch = %.2f us per step' % (T, us[3], step[0]))
    out('  D controller_rollout, QP allocation K = 16, T = %d  %8.1f us per launch = %.2f us per step  x %.2f of C' % (T, us[4], step[1], step[1] / step[0]))
    for (s, leak), u, st in zip(SHAPES, us[5:7], step[2:4]):
        fma = sum(a * b for a, b in zip(s[:-1], s[1:]))
        out('  E controller_rollout, network %-22s T = %d  %8.1f us per launch = %.2f us per step  x %.2f of C  x %.2f of D  (%d fmaf per env-step)'
            % ('-'.join(map(str, s)), T, u, st, st / step[0], st / step[1], fma))
    out('  F set_nn_allocator, 9-80-80-80-6 from device tensors %7.1f us per call (one packing launch)' % us[7])
    for iters in args.fit:
        data = nn_allocator_dataset(4096, seed=1)
        net = fit_nn_allocator(data, in_dim=9, iters=iters, lr=1e-3, minibatch=256)
        out('  G fit_nn_allocator, 4 096 rows, %d Adam steps of 256 rows: MSE %.4g -> %.4g (ratio %.3g)'
            % (iters, net['mse_initial'], net['mse_final'], net['mse_final'] / net['mse_initial']))
        env = ml4ca_amd.BatchedRevoltEnv(64, device=dev, terminate=False, seed=3)
        for name, kw in (('fitted network', dict(allocator='nn', net=net)), ('pseudo-inverse', dict(allocator='pinv')), ('QP, K = 16', dict(allocator='qp'))):
            r = evaluate.baseline_box_test(env, **kw)
            out('    calm box test, 64 envs, %-15s IAE %9.2f   work bow / port / star %s' % (
                name + ':', float(r['iae'].mean()), ' / '.join('%.1f' % w for w in r['work'].mean(0).tolist())))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
