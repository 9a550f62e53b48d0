#!/usr/bin/env python3
"""Cost of the network's labelling scan (dpenv_controller_label_nn / policy.controller_label_nn), one process, device events, warmed-up
shapes, arms alternating launch by launch, medians of 20.  Workload: 65 536 envs x 50 rows, for the reference's 9-20-20-20-20-6 relu shape
and the fitted 9-80-80-80-6 leaky shape.

  A  the full scan on a resident block: the handle's padded image (a = NULL), the weights read in place (explicit net), the padded image
     with bf16 rows.
  C  controller_rollout with the same network set, the same n and T: the yardstick.  It does the scan's network work and the plant
     besides.  It runs between every two A arms, so each of them starts from the same cache state.
  W  the wrench-only scan (act=False, tau=True: 12 B out per env-row) beside L, controller_label (the pseudo-inverse, 28 B out).

No bar is fixed: the ratios are written down.  The full scan is bound by VALU issue (one v_fmac per weight and env),
the wrench-only scan by its row traffic.

Usage: python tools/time_label_nn.py [--out profiles/controller_label_nn_timing.txt] [--envs 65536] [--rows 50]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import ml4ca_amd
from ml4ca_amd.policy import controller_label, controller_label_nn, controller_rollout, nn_net_to

from time_label import median_us

SHAPES = (((9, 20, 20, 20, 20, 6), 0.0), ((9, 80, 80, 80, 6), 0.2))


def seeded_net(sizes, leak, seed=21, scale=3.0):
    rng = np.random.RandomState(seed)
    W, b = [], []
    for i in range(len(sizes) - 1):
        lim = scale * np.sqrt(6.0 / (sizes[i] + sizes[i + 1]))
        W.append(rng.uniform(-lim, lim, size=(sizes[i], sizes[i + 1])).astype(np.float32))
        b.append(rng.uniform(-0.1, 0.1, size=sizes[i + 1]).astype(np.float32))
    return dict(W=W, b=b, leak=leak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'controller_label_nn_timing.txt'))
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, T = args.envs, args.rows
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out('tools/time_label_nn.py on %s' % torch.cuda.get_device_name(dev))
    out('%d envs x %d rows, medians of 20, arms alternating' % (n, T))
    z = torch.zeros((3, n), device=dev)
    lab = (torch.empty((T, n, 7), device=dev), torch.empty((3, n), device=dev))
    blk = None
    for sizes, leak in SHAPES:
        # the block: the network chain's own flight with auto-reset (done bytes of real episodes), then held resident
        flyer = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5, max_ep_len=40)
        flyer.set_dp_controller()
        net = nn_net_to(seeded_net(sizes, leak), dev)
        flyer.set_nn_allocator(net)
        flyer.reset()
        blk = {k: v.clone() for k, v in controller_rollout(flyer, T).items()}
        obs16 = blk['obs'].to(torch.bfloat16)
        fly = {k: torch.empty_like(v) for k, v in blk.items()}
        got, _ = controller_label_nn(flyer, blk['obs'], blk['done'], z=z)
        assert torch.equal(got, blk['act']), 'the labels of the network chain\'s own f32 rows are its act rows'
        fly_c = lambda: controller_rollout(flyer, T, out=fly)
        arms = [lambda: controller_label_nn(flyer, blk['obs'], blk['done'], z=z, out=lab), fly_c,
                lambda: controller_label_nn(flyer, blk['obs'], blk['done'], z=z, net=net, out=lab), fly_c,
                lambda: controller_label_nn(flyer, obs16, blk['done'], z=z, out=lab), fly_c]
        us = median_us(arms)
        c = statistics.median(us[1::2])
        out('%s, leak %g:' % ('-'.join(str(s) for s in sizes), leak))
        for name, t in zip(('A controller_label_nn, padded image (a = NULL), f32 rows', 'A controller_label_nn, weights in place, f32 rows',
                            'A controller_label_nn, padded image, bf16 rows'), us[0::2]):
            out('  %-58s %9.1f us  %6.2f ns per env-row  x %.3f of arm C' % (name, t, t * 1e3 / (n * T), t / c))
        out('  %-58s %9.1f us  %6.2f ns per env-step' % ('C controller_rollout with the network set, the same shape', c, c * 1e3 / (n * T)))
        del flyer, fly
    # the wrench-only scan beside the pseudo-inverse scan, on a handle with no network set
    plain = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=5, max_ep_len=40)
    plain.set_dp_controller()
    plain.reset()
    tau = (None, torch.empty((3, n), device=dev), torch.empty((T, n, 3), device=dev))
    arms = [lambda: controller_label_nn(plain, blk['obs'], blk['done'], z=z, act=False, tau=True, out=tau),
            lambda: controller_label(plain, blk['obs'], blk['done'], z=z, out=lab),
            lambda: controller_label_nn(plain, obs16, blk['done'], z=z, act=False, tau=True, out=tau),
            lambda: controller_label(plain, obs16, blk['done'], z=z, out=lab)]
    us = median_us(arms)
    out('the wrench-only scan beside controller_label:')
    for name, t, ref in zip(('W controller_label_nn(act=False, tau=True), f32 rows', 'L controller_label, f32 rows',
                             'W controller_label_nn(act=False, tau=True), bf16 rows', 'L controller_label, bf16 rows'), us, (us[1], us[1], us[3], us[3])):
        out('  %-58s %9.1f us  %6.2f ns per env-row  x %.3f of arm L' % (name, t, t * 1e3 / (n * T), t / ref))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
