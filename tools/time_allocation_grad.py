#!/usr/bin/env python3
"""Times one allocation-loss step (gradient + Adam) on one GPU beside the imitation MSE step of the same network shape on the same rows.
One process, device events, the arms alternating, medians of 20.

    python tools/time_allocation_grad.py [--rows 262144] [--out profiles/allocation_grad_timing.txt]

The yardstick is dpenv_imitation_grad(MSE) measured in the same call: the allocation kernel shares everything with it but the per-row
output stage, which adds two sincos and some thirty VALU operations on 16 lanes per wave behind the matrix phases.  --score also fits
the network with the wrench loss at w_power 1, 0.05 and 0 (and with the MSE loss) and flies each through the calm box test beside the
pseudo-inverse and the QP: the score card of DESIGN.md section 7."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ml4ca_amd import deploy
from ml4ca_amd import train as TR
from time_ppo_update import alternate


def timing(args, dev):
    N = args.rows
    ds = deploy.nn_allocator_dataset(N, 0)
    x, y = torch.as_tensor(ds['x']).to(dev), torch.as_tensor(ds['y']).to(dev)
    tau = torch.zeros(N, 6, device=dev)
    tau[:, :3] = torch.as_tensor(ds['tau']).float().to(dev)
    weight = 2.0 * torch.rand(N, device=dev)
    theta = torch.as_tensor(TR.nn_allocator_init(9, 0)).to(dev)
    P = theta.numel()
    m, v, step = torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.empty(P + 4, device=dev)
    ws = torch.empty((TR.workspace_bytes(TR.make_shape(9, 6, True), N) + 3) // 4, device=dev)
    q0, q1 = TR.alloc_loss_params(), TR.alloc_loss_params(dict(azimuth_mode=1))

    def adam():
        TR.adam_step(theta, g, m, v, step, 1e-5)

    def mse(w):
        def run():
            TR.imitation_grad(theta, x, y, loss='mse', weight=w, out=g, workspace=ws, leak=0.2)
            adam()
        return run

    def alloc(q, w):
        def run():
            TR.allocation_grad(theta, x, tau, q, weight=w, out=g, workspace=ws, leak=0.2)
            adam()
        return run

    arms = {'imitation mse, no weights (the yardstick)': mse(None), 'imitation mse, weighted': mse(weight),
            'allocation loss, no weights': alloc(q0, None), 'allocation loss, weighted': alloc(q0, weight),
            'allocation loss, fixed azimuths (mode 1)': alloc(q1, None), 'adam step alone': adam}
    t = alternate(arms, args.reps)
    base = t['imitation mse, no weights (the yardstick)']
    lines = ['allocation step (gradient + Adam), 9-80-80-80-6, %d rows; medians of %d, arms alternating; ms' % (N, args.reps)]
    for k, val in t.items():
        lines.append('%-44s %8.3f   x %.3f of the imitation MSE step' % (k, val, val / base))
    return lines


def score(args, dev):
    import ml4ca_amd
    from ml4ca_amd import evaluate as EV
    nominal = ml4ca_amd.default_vessel('no_loss')
    nb, T = args.score_envs, 1250
    start = torch.zeros((3, nb), device=dev)
    lines = ['calm box test, nominal hull, %d envs x %d steps; network fits: %d Adam steps on 16 384 rows' % (nb, T, args.score_iters)]

    def fly(tag, allocator='pinv', net=None, note=''):
        env = ml4ca_amd.BatchedRevoltEnv(nb, device=dev, terminate=False, time_limit=False, seed=77, vessel_params=nominal)
        env.set_dp_controller(deploy.dp_controller_defaults(nominal))
        if allocator == 'qp':
            env.set_qp_allocator(deploy.qp_allocator_defaults(nominal))
        s = EV.baseline_box_test_streamed(env, T=T, start=start, chunk=50, allocator=allocator, net=net)
        w = [float(v) for v in s['work'].mean(0)]
        lines.append('%-34s IAE %7.2f (worst env %7.2f)  work bow/port/star %s  sum %.1f  %s' % (
            tag, float(s['iae'].mean()), float(s['iae'].max()), [round(v, 1) for v in w], sum(w), note))
        print(lines[-1], flush=True)

    fly('PID + pseudo-inverse')
    fly('PID + QP', allocator='qp')
    ds = deploy.nn_allocator_dataset(16384, 0, vessel=nominal)
    for loss, wp in (('mse', None), ('wrench', 1.0), ('wrench', 0.05), ('wrench', 0.0)):
        net = TR.fit_nn_allocator(ds, iters=args.score_iters, seed=0, device=dev, loss=loss, alloc_loss=None if wp is None else dict(w_power=wp))
        fly('PID + network, %s%s' % (loss, '' if wp is None else ' w_power %g' % wp), allocator='nn', net=net,
            note='fit: label MSE %.3g -> %.3g, mean Js %.1f -> %.2f N^2' % (net['mse_initial'], net['mse_final'], net['wrench_ms_initial'],
                                                                           net['wrench_ms_final']))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--score', action='store_true', help='also fit and fly the calm box test score card')
    ap.add_argument('--score-envs', type=int, default=1024)
    ap.add_argument('--score-iters', type=int, default=5000)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    lines = timing(args, dev)
    print('\n'.join(lines), flush=True)
    if args.score:
        lines += score(args, dev)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
