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

--flown / --qp-table: the arms of dpenv_controller_label_qp_ex instead (the thruster state from the FLOWN action rows; one QP allocator per
env read from the public table by the lanes; with both flags also the two together).  Same protocol; the yardstick is the scalar
own-recursion arm A in the same process (the kernel above, unchanged), C still runs between every two arms.  Bar: 1.05 x (1 + the share
of the new per-row instructions in a row's instruction count read from the ISA): the flown decode is 161 instructions, the table adds
none per row, a row is about 800 + 620 K.  Above 1.25 means scratch or VGPR-indexed moves: look at the ISA first.

Usage: python tools/time_label_qp.py [--flown] [--qp-table] [--out profiles/controller_label_qp_timing.txt] [--envs 65536] [--rows 50]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import ml4ca_amd
from ml4ca_amd.deploy import dp_controller_table, qp_allocator_defaults, qp_allocator_table
from ml4ca_amd.policy import controller_label_qp, controller_rollout

from time_label import median_us

BAR = 1.05
DECODE_INSTRUCTIONS, ROW_INSTRUCTIONS, ITERATION_INSTRUCTIONS = 161, 800, 620      # read from the ISA of the label unit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--flown', action='store_true', help='time the flown-state arm of dpenv_controller_label_qp_ex against the own-recursion arm')
    ap.add_argument('--qp-table', action='store_true', help='time the per-env QP table arm of dpenv_controller_label_qp_ex against the own-recursion arm')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=50)
    args = ap.parse_args()
    ex = args.flown or args.qp_table
    if not args.out:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'controller_label_qp_flown_timing.txt' if ex else 'controller_label_qp_timing.txt')
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
    if ex:
        out('%d envs x %d rows, medians of 20, arms alternating; the bar: an arm <= %.2f x (1 + its new instructions per row / a row\'s) x the '
            'scalar own-recursion arm' % (n, T, BAR))
    else:
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
        if ex:
            worst = max(worst, ex_arms(out, scalar, blk, z, x, q, K, lab, fly_c, args, n, T))
            del flyer, blk, obs16, fly
            continue
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
    if ex:
        out('worst ratio to its bar %.3f: %s' % (worst, 'within' if worst <= 1.0 else 'OVER'))
    else:
        out('worst A / C ratio %.3f: %s the bar of %.2f' % (worst, 'within' if worst <= BAR else 'OVER', BAR))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def ex_arms(out, env, blk, z, x, q, K, lab, fly_c, args, n, T):
    """The arms of dpenv_controller_label_qp_ex against the scalar own-recursion arm; returns the worst time / bar."""
    tab = torch.from_numpy(qp_allocator_table(n, q)).to(env.device)                   # equal rows: the same solves, lane by lane
    own = lambda: controller_label_qp(env, blk['obs'], blk['done'], z=z, x=x, params=q, out=lab)
    names, arms = ['A controller_label_qp, own recursion (the yardstick)'], [own, fly_c]
    share = []
    row = ROW_INSTRUCTIONS + ITERATION_INSTRUCTIONS * K
    if args.flown:
        names.append('F flown thruster state')
        share.append(DECODE_INSTRUCTIONS / row)
        arms += [lambda: controller_label_qp(env, blk['obs'], blk['done'], z=z, x=x, params=q, out=lab, flown=blk['act']), fly_c]
    if args.qp_table:
        names.append('Q per-env QP table, own recursion')
        share.append(0.0)
        arms += [lambda: controller_label_qp(env, blk['obs'], blk['done'], z=z, x=x, out=lab, table=tab, iterations=K), fly_c]
    if args.flown and args.qp_table:
        names.append('FQ flown thruster state and per-env QP table')
        share.append(DECODE_INSTRUCTIONS / row)
        arms += [lambda: controller_label_qp(env, blk['obs'], blk['done'], z=z, x=x, out=lab, table=tab, iterations=K, flown=blk['act']), fly_c]
    got = controller_label_qp(env, blk['obs'], blk['done'], z=z, x=x, table=tab, iterations=K)[0]
    assert torch.equal(got, blk['act']), 'a table of equal rows labels the QP chain\'s own rows with its act rows'
    us = median_us(arms)
    a, c = us[0], statistics.median(us[1::2])
    out('K = %d:' % K)
    worst = 0.0
    for name, t, sh in zip(names, us[0::2], [None] + share):
        tail = '' if sh is None else '  x %.3f of arm A (bar %.3f)' % (t / a, BAR * (1.0 + sh))
        out('  %-52s %9.1f us  %6.2f ns per env-row  %5.2f ns per env-row and iteration%s' % (name, t, t * 1e3 / (n * T), t * 1e3 / (n * T * K), tail))
        if sh is not None:
            worst = max(worst, t / a / (BAR * (1.0 + sh)))
    out('  %-52s %9.1f us  %6.2f ns per env-step' % ('C controller_rollout with the QP set, the same shape', c, c * 1e3 / (n * T)))
    return worst


if __name__ == '__main__':
    main()
