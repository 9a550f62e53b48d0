#!/usr/bin/env python3
"""Cost of the QP thrust allocation, alone (dpenv_thrust_alloc_qp / policy.thrust_alloc_qp) and as the allocation stage of the fused closed
loop (dpenv_set_qp_allocator + dpenv_controller_rollout): one process, device events, warmed-up shapes, launch spacing over batches of 20
back-to-back launches, arms alternating batch by batch, medians of 7 batches.  Workload: 65 536 envs; launches of T = 50 steps with auto-reset on.

  A  thrust_alloc_qp at K = 8, 16 and 32 iterations (state in place, no objective read-out, wrenches of a normal draw).
  B  thrust_alloc, the stateless pseudo-inverse allocation, on the same wrenches: the existing allocation call.
  C  controller_rollout with the pseudo-inverse, T = 50: the yardstick of the closed loop.
  D  controller_rollout with the QP allocation at K = 8 and K = 16, T = 50, in the same call.

--table times the per-env table forms (dpenv_set_qp_allocator_table, dpenv_thrust_alloc_qp_table) against the scalar forms IN THE SAME CALL
(the scalar kernels are instruction for instruction what they were before the table existed, so they are the yardstick), the same way:

  E  controller_rollout, T = 50, K = 16 and K = 8: the scalar QP against a table of equal rows.
  F  env.set_qp_allocator_table(check=False): the packing kernel and the zeroing of the thruster state, per call.
  G  thrust_alloc_qp at K = 16: params against table.
  H  evaluate.qp_weight_sweep, --sweep K sets x 16 directions (the default population, the whole 250 s box test, reference filter on):
     wall time of the call after one warm-up call, and the front's points.

Usage: python tools/time_qp_alloc.py [--out profiles/qp_alloc_timing.txt] [--envs 65536]
       python tools/time_qp_alloc.py --table [--sweep 32] [--out profiles/qp_alloc_table_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import ml4ca_amd
from ml4ca_amd.deploy import qp_allocator_defaults, qp_allocator_table, qp_weight_population
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


def table_leg(args, dev, out):
    from ml4ca_amd import evaluate
    n, T = args.envs, 50
    tab = torch.from_numpy(qp_allocator_table(n)).to(dev)
    arms, fly = [], None
    for K in (16, 8):
        for tabbed in (False, True):
            env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5)
            env.set_dp_controller()
            if tabbed:
                env.set_qp_allocator_table(tab, iterations=K)
            else:
                env.set_qp_allocator(dict(qp_allocator_defaults(), iterations=K))
            env.reset()
            if fly is None:
                fly = {k: torch.empty_like(v) for k, v in controller_rollout(env, T).items()}
            arms.append(lambda env=env: controller_rollout(env, T, out=fly))
    packer = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5)
    packer.set_dp_controller()
    packer.set_qp_allocator_table(tab)
    arms.append(lambda: packer.set_qp_allocator_table(tab, check=False))
    rng = np.random.default_rng(0)
    tau = torch.from_numpy((rng.normal(0.0, 1.0, (3, n)) * np.array([[20.0], [10.0], [15.0]])).astype(np.float32)).to(dev)
    p = qp_allocator_defaults()
    for tabbed in (False, True):
        S = torch.zeros((5, n), device=dev)
        buf = (torch.empty((n, 7), device=dev), S)
        kw = dict(table=tab, iterations=16) if tabbed else dict(params=p)
        for _ in range(10):                                  # a state in flight, not the rest state
            thrust_alloc_qp(tau, S, out=buf, **kw)
        arms.append(lambda S=S, buf=buf, kw=kw: thrust_alloc_qp(tau, S, out=buf, **kw))
    us = spacing_us(arms)
    out('%d envs, launch spacing over 20 back-to-back launches, medians of 7 batches, arms alternating:' % n)
    for k, K in enumerate((16, 8)):
        a, b = us[2 * k], us[2 * k + 1]
        out('  E controller_rollout, T = %d, K = %-2d: scalar QP %8.1f us per launch, per-env table %8.1f us  x %.3f' % (T, K, a, b, b / a))
    out('  F set_qp_allocator_table (pack %d rows + zero the thruster state)  %8.1f us per call' % (n, us[4]))
    out('  G thrust_alloc_qp, K = 16: params %8.1f us per call, table %8.1f us  x %.3f' % (us[5], us[6], us[6] / us[5]))
    if args.sweep:
        K, D = args.sweep, 16
        env = ml4ca_amd.BatchedRevoltEnv(K * D, device=dev, terminate=False, time_limit=False, current=True, seed=5)
        pop = qp_weight_population(K)
        evaluate.qp_weight_sweep(env, pop, directions=D)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate.qp_weight_sweep(env, pop, directions=D)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out('  H qp_weight_sweep, %d sets x %d directions = %d envs, 1250 steps, filter on: %.3f s wall per sweep' % (K, D, K * D, dt))
        mi, mw = res['mean_iae'].cpu().numpy(), res['mean_work'].sum(1).cpu().numpy()
        out('    set 0 (the defaults): mean IAE %.2f, mean work %.4g' % (mi[0], mw[0]))
        out('    front (set: mean IAE, mean work, w_power, w_dalpha, w_dforce):')
        for k in res['front']:
            out('      %3d: %8.2f %10.4g   %.3g %.3g %.3g' % (k, mi[k], mw[k], pop['w_power'][k], pop['w_dalpha'][k], pop['w_dforce'][k]))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--table', action='store_true', help='the per-env table forms against the scalar forms')
    ap.add_argument('--sweep', type=int, default=0, help='with --table: time qp_weight_sweep with this many weight sets')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(here, 'profiles', 'qp_alloc_table_timing.txt' if args.table else 'qp_alloc_timing.txt')
    dev = torch.device('cuda', 0)
    n, T = args.envs, 50
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_qp_alloc.py%s on %s' % (' --table' if args.table else '', torch.cuda.get_device_name(dev)))
    if args.table:
        table_leg(args, dev, out)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
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
