#!/usr/bin/env python3
"""Cost of the streaming score card (dpenv_score_* / evaluate.ScoreCard), one process, device events, warmed-up shapes, arms alternating
launch by launch, medians of 20.

  block   65 536 envs x 50-row blocks, resident (f32 obs 9, act 7, integ, rew, done): A = ScoreCard.add, B = the host-composed way to the
          same numbers from the same blocks: evaluate.iae(obs - integ) + evaluate.work(commanded_thrust(act)) + rew.sum(0); then the
          one-pass score + wear call (ScoreCard(wear=).add) for three variants beside A, and A on the act rows alone.
  flight  the 1 250-step box test at 16 384 envs (f16 actor, integral action + reference filter): streamed in 50-step launches against the
          one-piece deployment_box_test - wall time including the scoring, peak allocated memory, and the adds' share of the streamed flight;
          then the streamed flight alone at 65 536 envs (one piece there is the 8.6 GB of rows the card exists to avoid: not run).

Usage: python tools/time_score.py [--out profiles/score_card_timing.txt] [--envs 65536] [--flight-envs 16384] [--block-only]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import ml4ca_amd
from ml4ca_amd import evaluate as EV
from ml4ca_amd.policy import ActorCritic

ROW_BYTES = 36 + 28 + 12 + 4 + 1         # what the layout moves per env-step: whole obs and act rows
ALGO_BYTES = 12 + 12 + 12 + 4 + 1        # what the sums need: three columns of obs, act and integ, the reward, the done byte
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


def block_cost(n, T, dev, out):
    g = torch.Generator(device=dev).manual_seed(0)
    blk = dict(obs=torch.randn((T, n, 9), device=dev, generator=g), act=torch.rand((T, n, 7), device=dev, generator=g) * 2.6 - 1.3,
               integ=torch.randn((T, n, 3), device=dev, generator=g) * 0.01, rew=torch.rand((T, n), device=dev, generator=g),
               done=(torch.rand((T, n), device=dev, generator=g) < 0.01).to(torch.uint8))
    sc = EV.ScoreCard(n, dev)

    def arm_a():
        sc.add(blk)

    def arm_b():
        iae, _ = EV.iae(blk['obs'][..., :3] - blk['integ'])
        return iae, EV.work(EV.commanded_thrust(blk['act'])), blk['rew'].sum(0)

    a, b = median_us([arm_a, arm_b])
    rows = n * T
    out('block cost, %d envs x %d rows (f32 obs 9, act 7, integ, rew, done), medians of 20, arms alternating:' % (n, T))
    out('  A ScoreCard.add (score_kernel, plain strided row loads, 2 x %d rows ahead): %8.1f us  %7.1f GB/s at %d B per env-step = %.3f of 8 TB/s'
        '  (%.1f GB/s at the %d B the sums need)' % (2, a, rows * ROW_BYTES / a / 1e3, ROW_BYTES, rows * ROW_BYTES / (a * 1e-6) / HBM,
                                                     rows * ALGO_BYTES / a / 1e3, ALGO_BYTES))
    out('  B evaluate.iae(obs - integ) + evaluate.work(commanded_thrust(act)) + rew.sum(0):      %8.1f us  (A is %.1f x faster)' % (b, b / a))
    # the same kernel on other inputs: bf16 obs; obs alone
    blk_bf = dict(blk, obs=blk['obs'].to(torch.bfloat16))
    c, d = median_us([lambda: sc.add(blk_bf), lambda: sc.add(dict(obs=blk['obs'], rew=blk['rew']))])
    out('  A with bf16 obs rows: %.1f us;  A with obs and rew alone: %.1f us' % (c, d))
    # the one-pass call (dpenv_score_accumulate_wear: score + IADC, the act fetch widened to the variant's columns) beside A, from the same run
    wear_row = {'final cont_ang (7 columns)': ROW_BYTES + 16, 'final (5 columns)': ROW_BYTES + 8, 'simple (3 columns)': ROW_BYTES}
    cards = [EV.ScoreCard(n, dev, wear=w) for w in (dict(variant='final', cont_ang=True), dict(variant='final', cont_ang=False), dict(variant='simple'))]
    t = median_us([arm_a] + [lambda c=c: c.add(blk) for c in cards])
    out('  one pass, score + wear (score_wear_kernel; 64 B of wear state per env beside the 128 B), against A = %.1f us in the same alternation:' % t[0])
    for (name, rb), us in zip(wear_row.items(), t[1:]):
        out('    %-28s %8.1f us  x %.3f of A  %7.1f GB/s at %d B per env-step' % (name, us, us / t[0], rows * rb / us / 1e3, rb))
    # the alternative: A, then a second full pass over the act rows (here: A on the act rows alone, what a separate wear kernel would at least read)
    e, = median_us([lambda: sc.add(dict(act=blk['act']))])
    out('  A on the act rows alone (the least a separate wear pass would cost): %.1f us; A + that = %.1f us' % (e, t[0] + e))
    return a


def flight(n, dev, out, one_piece):
    env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=5)
    ActorCritic(9, 7, (80, 80, 80), seed=1, device=dev).upload(env, precision='f16')
    T, chunk = 1250, 50

    def run(f):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(dev) - base
        iae = float(r['iae'].double().mean())
        del r
        return dt, peak, iae

    streamed = lambda: EV.deployment_box_test_streamed(env, T=T, chunk=chunk, integral=True, reference_filter=True)
    whole = lambda: EV.deployment_box_test(env, T=T, integral=True, reference_filter=True)
    run(streamed)
    if one_piece:
        run(whole)
    s = [run(streamed) for _ in range(5)]
    ts = statistics.median(x[0] for x in s)
    out('box test, %d steps, %d envs, f16 actor, integral action + reference filter:' % (T, n))
    out('  streamed (%d launches of %d steps, a ScoreCard.add behind each): %8.2f ms per flight incl. scoring, peak allocated %8.1f MB above the env, mean IAE %.4f'
        % (T // chunk, chunk, ts * 1e3, s[0][1] / 1e6, s[0][2]))
    if one_piece:
        w = [run(whole) for _ in range(5)]
        tw = statistics.median(x[0] for x in w)
        out('  one piece (deployment_box_test: one launch, evaluate.iae / work over the rows):  %8.2f ms per flight incl. scoring, peak allocated %8.1f MB above the env, mean IAE %.4f'
            % (tw * 1e3, w[0][1] / 1e6, w[0][2]))
    # the adds' share: the same 25 adds on a resident block of this size, timed by events
    blk = dict(obs=torch.randn((chunk, n, 9), device=dev), act=torch.randn((chunk, n, 7), device=dev), integ=torch.zeros((chunk, n, 3), device=dev),
               rew=torch.zeros((chunk, n), device=dev), done=torch.zeros((chunk, n), dtype=torch.uint8, device=dev))
    sc = EV.ScoreCard(n, dev)

    def adds():
        for _ in range(T // chunk):
            sc.add(blk)

    a, = median_us([adds])
    out('  score_kernel over the flight (%d adds): %.1f us = %.2f %% of the streamed flight' % (T // chunk, a, 100.0 * a * 1e-6 / ts))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'score_card_timing.txt'))
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--flight-envs', type=int, default=16384)
    ap.add_argument('--block-only', action='store_true', help='the block costs alone, no flights')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_score.py on %s' % torch.cuda.get_device_name(dev))
    block_cost(args.envs, 50, dev, out)
    if not args.block_only:
        flight(args.flight_envs, dev, out, one_piece=True)
        flight(args.envs, dev, out, one_piece=False)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
