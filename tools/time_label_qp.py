#!/usr/bin/env python3
"""Cost of the QP labelling scan (dpenv_controller_label_qp / policy.controller_label_qp), one process, device events, warmed-up shapes,
arms alternating launch by launch, medians of 20.  Workload: 65 536 envs x 50 rows, at K = 16 and K = 8 LM iterations.

  A  controller_label_qp on a resident block: the scalar controller with f32 rows, a per-env table with f32 rows, the scalar
     controller with bf16 rows.
  C  controller_rollout with the QP set, the same n, T and K: the yardstick.  It does the scan's allocation work and the plant besides,
     so the scan should not be slower; the bar is 1.05 x C (the margin is this pool's several-per-cent spread).  It runs between every
     two A arms, so each of them starts from the same cache state (its rows displace the block).

The kernel is bound by VALU issue (about 620 instructions per LM iteration against 7 loads per row): the time is K x rows x waves per
SIMD.  The scan is serial in T per env, so at small n its cost is the closed loop's latency per row; nothing here works around that.

Usage: python tools/time_label_qp.py [--out profiles/controller_label_qp_timing.txt] [--envs 65536] [--rows 50]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import ml4ca_amd
from ml4ca_amd.deploy import dp_controller_table, qp_allocator_defaults
from ml4ca_amd.policy import controller_label_qp, controller_rollout

from time_label import median_us

BAR = 1.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'controller_label_qp_timing.txt'))
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, T = args.envs, args.rows
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_label_qp.py on %s' % torch.cuda.get_device_name(dev))
    scalar, table = (ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5, max_ep_len=40) for _ in range(2))
    for e in (scalar, table):
        e.set_dp_controller()
        e.reset()
    table.set_dp_controller_table(torch.from_numpy(dp_controller_table(n)).to(dev))
    z, x = torch.zeros((3, n), device=dev), torch.zeros((5, n), device=dev)
    lab = (torch.empty((T, n, 7), device=dev), torch.empty((3, n), device=dev), torch.empty((5, n), device=dev))
    out('%d envs x %d rows, medians of 20, arms alternating; the bar: A <= %.2f x C' % (n, T, BAR))
    worst = 0.0
    for K in (16, 8):
        q = dict(qp_allocator_defaults(), iterations=K)
        # the block: the QP chain's own flight with auto-reset (done bytes of real episodes), then held resident
        flyer = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5, max_ep_len=40)
        flyer.set_dp_controller()
        flyer.set_qp_allocator(q)
        flyer.reset()
        blk = {k: v.clone() for k, v in controller_rollout(flyer, T).items()}
        obs16 = blk['obs'].to(torch.bfloat16)
        fly = {k: torch.empty_like(v) for k, v in blk.items()}
        got, _, _ = controller_label_qp(scalar, blk['obs'], blk['done'], z=z, x=x, params=q)
        assert torch.equal(got, blk['act']), 'the labels of the QP chain\'s own f32 rows are its act rows'
        fly_c = lambda: controller_rollout(flyer, T, out=fly)
        arms = [lambda: controller_label_qp(scalar, blk['obs'], blk['done'], z=z, x=x, params=q, out=lab), fly_c,
                lambda: controller_label_qp(table, blk['obs'], blk['done'], z=z, x=x, params=q, out=lab), fly_c,
                lambda: controller_label_qp(scalar, obs16, blk['done'], z=z, x=x, params=q, out=lab), fly_c]
        us = median_us(arms)
        c = statistics.median(us[1::2])
        out('K = %d:' % K)
        for name, t in zip(('A controller_label_qp, scalar controller, f32 rows', 'A controller_label_qp, per-env table, f32 rows',
                            'A controller_label_qp, scalar controller, bf16 rows'), us[0::2]):
            out('  %-52s %9.1f us  %6.2f ns per env-row  %5.2f ns per env-row and iteration  x %.3f of arm C' % (
                name, t, t * 1e3 / (n * T), t * 1e3 / (n * T * K), t / c))
            worst = max(worst, t / c)
        out('  %-52s %9.1f us  %6.2f ns per env-step' % ('C controller_rollout with the QP set, the same shape', c, c * 1e3 / (n * T)))
        del flyer, blk, obs16, fly
    out('worst A / C ratio %.3f: %s the bar of %.2f' % (worst, 'within' if worst <= BAR else 'OVER', BAR))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
