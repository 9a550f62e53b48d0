#!/usr/bin/env python3
"""Cost of the labelling scan (dpenv_controller_label / policy.controller_label), one process, device events, warmed-up shapes, arms
alternating launch by launch, medians of 20.  Workload: 65 536 envs x 50 rows.

  A  controller_label on a resident block: the scalar controller and a per-env table, f32 and bf16 obs rows.
  B  evaluate.ScoreCard.add on the same block (obs, act, integ, rew, done): the existing row scan, the yardstick - time per byte moved.
  C  controller_rollout of the same shape: the existing way to obtain expert rows (it flies the expert's own states, not the block's).
     It runs between every two other arms, so each of them starts from the same cache state (its rows displace the block).

Usage: python tools/time_label.py [--out profiles/controller_label_timing.txt] [--envs 65536] [--rows 50]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import ml4ca_amd
from ml4ca_amd import evaluate as EV
from ml4ca_amd.deploy import dp_controller_table
from ml4ca_amd.policy import controller_label, controller_rollout

LABEL_BYTES = {'f32': 36 + 1 + 28, 'bf16': 18 + 1 + 28}      # whole obs row + done byte in, action row out
SCORE_BYTES = 36 + 28 + 12 + 4 + 1                           # tools/time_score.py ROW_BYTES
HBM = 8.0e12


def median_us(arms, reps=20, warm=3):
    """arms: callables; alternate them launch by launch; median device time of each in us."""
    for _ in range(warm):
        for f in arms:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in arms]
    for r in range(reps):
        for k, f in enumerate(arms):
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in e) for e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'controller_label_timing.txt'))
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, T = args.envs, args.rows
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_label.py on %s' % torch.cuda.get_device_name(dev))
    # the block: the baseline's own flight with auto-reset (done bytes of real episodes), then held resident
    scalar, table, flyer = (ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5, max_ep_len=40) for _ in range(3))
    for e in (scalar, table, flyer):
        e.set_dp_controller()
        e.reset()
    table.set_dp_controller_table(torch.from_numpy(dp_controller_table(n)).to(dev))
    blk = {k: v.clone() for k, v in controller_rollout(flyer, T).items()}
    blk['integ'] = torch.zeros((T, n, 3), device=dev)
    obs16 = blk['obs'].to(torch.bfloat16)
    z = torch.zeros((3, n), device=dev)
    lab = (torch.empty((T, n, 7), device=dev), torch.empty((3, n), device=dev))
    fly = {k: torch.empty_like(v) for k, v in blk.items() if k != 'integ'}
    sc = EV.ScoreCard(n, dev)
    got, _ = controller_label(scalar, blk['obs'], blk['done'], z=z)
    assert torch.equal(got, blk['act']), 'the labels of the baseline\'s own f32 rows are its act rows'

    # Arm C flies between every two other arms: a 50-step flight writes 226 MB of rows of its own, so every A and B arm starts from the
    # same cache state - the block pushed out of the 256 MB last-level cache, as it is when a flight has just written it.  (Without it an
    # arm that follows another reader of the same block finds its rows there: the first record of this tool read the table form 17 %
    # faster than the scalar form for that reason alone.)
    fly_c = lambda: controller_rollout(flyer, T, out=fly)
    arms = [lambda: controller_label(scalar, blk['obs'], blk['done'], z=z, out=lab), fly_c,
            lambda: controller_label(table, blk['obs'], blk['done'], z=z, out=lab), fly_c,
            lambda: controller_label(scalar, obs16, blk['done'], z=z, out=lab), fly_c,
            lambda: controller_label(table, obs16, blk['done'], z=z, out=lab), fly_c,
            lambda: sc.add(blk), fly_c]
    us = median_us(arms)
    a_s, a_t, a_s16, a_t16, b = us[0::2]
    c = statistics.median(us[1::2])
    rows = n * T
    per_byte = lambda us, nbytes: us * 1e-6 / (rows * nbytes)
    score_pb = per_byte(b, SCORE_BYTES)
    out('%d envs x %d rows, medians of 20, arms alternating:' % (n, T))
    for name, us, kind in (('A controller_label, scalar controller, f32 rows', a_s, 'f32'), ('A controller_label, per-env table, f32 rows', a_t, 'f32'),
                           ('A controller_label, scalar controller, bf16 rows', a_s16, 'bf16'), ('A controller_label, per-env table, bf16 rows', a_t16, 'bf16')):
        nb = LABEL_BYTES[kind]
        out('  %-50s %8.1f us  %7.1f GB/s at %d B per env-row = %.3f of 8 TB/s  time per byte x %.2f of ScoreCard.add\'s  x %.3f of arm C' % (
            name, us, rows * nb / us / 1e3, nb, rows * nb / (us * 1e-6) / HBM, per_byte(us, nb) / score_pb, us / c))
    out('  %-50s %8.1f us  %7.1f GB/s at %d B per env-row = %.3f of 8 TB/s' % (
        'B ScoreCard.add (obs, act, integ, rew, done)', b, rows * SCORE_BYTES / b / 1e3, SCORE_BYTES, rows * SCORE_BYTES / (b * 1e-6) / HBM))
    out('  %-50s %8.1f us' % ('C controller_rollout, the same shape', c))
    out('expectation written before the first measurement: A\'s time per byte within 1.5 x of B\'s; the condition: A faster than C')
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
