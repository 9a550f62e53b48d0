#!/usr/bin/env python3
"""Cost of the QP thrust allocation, alone (dpenv_thrust_alloc_qp / policy.thrust_alloc_qp) and as the allocation stage of the fused closed
loop (dpenv_set_qp_allocator + dpenv_controller_rollout): one process, device events, warmed-up shapes, launch spacing over batches of 20
back-to-back launches, arms alternating batch by batch, medians of 7 batches.  Workload: 65 536 envs; launches of T = 50 steps with auto-reset on.

  A  thrust_alloc_qp at K = 8, 16 and 32 iterations (state in place, no objective read-out, wrenches of a normal draw).
  B  thrust_alloc, the stateless pseudo-inverse allocation, on the same wrenches: the existing allocation call.
  C  controller_rollout with the pseudo-inverse, T = 50: the yardstick of the closed loop.
  D  controller_rollout with the QP allocation at K = 8 and K = 16, T = 50, in the same call.

Usage: python tools/time_qp_alloc.py [--out profiles/qp_alloc_timing.txt] [--envs 65536]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import ml4ca_amd
from ml4ca_amd.deploy import qp_allocator_defaults
from ml4ca_amd.policy import controller_rollout, thrust_alloc_qp


def spacing_us(arms, launches=20, reps=7, warm=3):
    """arms: callables.  Launch spacing: per repetition and arm one event pair around `launches` back-to-back calls, the arms alternating
    batch by batch; behind a ~1 ms spin kernel, so that the host (the Python binding builds its argument struct on every call) has queued
    the batch before the device starts it and the pair times the device alone.  Median over the repetitions of time / launches, in us."""
    for _ in range(warm):
        for f in arms:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in arms]
    for r in range(reps):
        for k, f in enumerate(arms):
            torch.cuda._sleep(2500000)
            ev[k][r][0].record()
            for _ in range(launches):
                f()
            ev[k][r][1].record()
        torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 / launches for a, b in e) for e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'qp_alloc_timing.txt'))
    ap.add_argument('--envs', type=int, default=65536)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, T = args.envs, 50
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_qp_alloc.py on %s' % torch.cuda.get_device_name(dev))
    rng = np.random.default_rng(0)
    tau = torch.from_numpy((rng.normal(0.0, 1.0, (3, n)) * np.array([[20.0], [10.0], [15.0]])).astype(np.float32)).to(dev)
    arms, Ks = [], (8, 16, 32)
    for K in Ks:
        p = qp_allocator_defaults()
        p['iterations'] = K
        S = torch.zeros((5, n), device=dev)
        buf = (torch.empty((n, 7), device=dev), S)
        for _ in range(10):                                  # a state in flight, not the rest state
            thrust_alloc_qp(tau, S, p, out=buf)
        arms.append(lambda p=p, S=S, buf=buf: thrust_alloc_qp(tau, S, p, out=buf))
    arms.append(lambda: ml4ca_amd.thrust_alloc(tau))
    fly = None
    for K in (None, 8, 16):
        env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5)
        env.set_dp_controller()
        if K:
            p = qp_allocator_defaults()
            p['iterations'] = K
            env.set_qp_allocator(p)
        env.reset()
        if fly is None:
            fly = {k: torch.empty_like(v) for k, v in controller_rollout(env, T).items()}
        arms.append(lambda env=env: controller_rollout(env, T, out=fly))
    us = spacing_us(arms)
    out('%d envs, launch spacing over 20 back-to-back launches, medians of 7 batches, arms alternating:' % n)
    for K, u in zip(Ks, us[:3]):
        out('  A thrust_alloc_qp, K = %-2d                          %8.1f us per control step  (%.2f us per iteration)  x %.1f of B  x %.2f of a C step'
            % (K, u, u / K, u / us[3], u / (us[4] / T)))
    out('  B thrust_alloc (pseudo-inverse, stateless)          %8.1f us per call' % us[3])
    out('  C controller_rollout, pseudo-inverse, T = %d        %8.1f us per launch = %.2f us per step' % (T, us[4], us[4] / T))
    for K, u in zip((8, 16), us[5:7]):
        out('  D controller_rollout, QP allocation K = %-2d, T = %d  %8.1f us per launch = %.2f us per step  x %.2f of C' % (K, T, u, u / T, u / us[4]))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
