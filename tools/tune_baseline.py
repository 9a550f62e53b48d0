#!/usr/bin/env python3
"""The baseline's IAE / work trade-off curve beside the thesis actor: evaluate.baseline_gain_sweep at scale.  --sets gain sets around the
pole-placement defaults (deploy.gain_population; set 0 is the default baseline) x 16 directions of a 0.2 m/s current fly ONE scored
250 s box test behind the reference filter, every env on its own row of the per-env controller table; the thesis actor
(tests/golden/final_policy.npz), without and with the node's integral action, flies the same envs and currents.  Prints the wall time
per flight (scoring included, second flight of two), the peak device memory above the env, about ten points of the front, the lowest
IAE any set reaches, the lowest IAE at no more than the actor's work, and what the default spends against the best set of equal IAE.
    python tools/tune_baseline.py [--sets 4096] [--span 4] [--seed 0] [--box-steps 1250] [--out tune_baseline.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', type=int, default=4096)
    ap.add_argument('--directions', type=int, default=16)
    ap.add_argument('--vc', type=float, default=0.2)
    ap.add_argument('--span', type=float, default=4.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--box-steps', type=int, default=1250)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import numpy as np
    import torch
    import ml4ca_amd
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import gain_population
    from ml4ca_amd.policy import ActorCritic
    dev = torch.device('cuda', 0)
    K, D, T = args.sets, args.directions, args.box_steps
    n = K * D
    env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=2, current=True)
    pop = gain_population(K, span=args.span, seed=args.seed)
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sw = EV.baseline_gain_sweep(env, pop, directions=D, vc=args.vc, reference_filter=True, T=T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated(dev) - base_mem
    iae, work = sw['mean_iae'].cpu().numpy(), sw['mean_work'].cpu().numpy()
    tot = work.sum(1)
    print('%d gain sets x %d directions of %.1f m/s = %d envs, %d-step box test behind the reference filter, factors log-uniform in [1/%g, %g]' % (
        K, D, args.vc, n, T, args.span, args.span))
    print('flight + scoring, wall: first %.1f ms, second %.1f ms; peak device memory above the env %.1f MB' % (ms[0], ms[1], peak / 1e6), flush=True)

    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'final_policy.npz'))
    ActorCritic.from_tensors({k.replace('.', '/'): d[k] for k in d.files if '.' in k}, device=dev).upload(env)
    actors = {}
    for who, integral in (('actor', False), ('actor + integral action', True)):
        st = EV.deployment_box_test_streamed(env, T=T, chunk=50, integral=integral, reference_filter=True)   # (the sweep left the currents set)
        actors[who] = (float(st['iae'].mean()), st['work'].mean(0).cpu().numpy())
    fmt = lambda name, i, w: '%-34s IAE %7.2f   work bow/port/star %7.1f %7.1f %7.1f   total %8.1f' % (name, i, w[0], w[1], w[2], w.sum())
    gains = lambda k: '  kp x %s kd x %s ki x %s' % tuple([round(float(x), 2) for x in pop['factors'][g][k]] for g in ('kp', 'kd', 'ki'))
    for who, (i, w) in actors.items():
        print(fmt(who, i, w))
    print(fmt('default baseline (set 0)', iae[0], work[0]))
    front = [int(k) for k in sw['front']]
    print('front: %d of %d sets; about ten of them by IAE:' % (len(front), K))
    for k in [front[j] for j in sorted(set(np.linspace(0, len(front) - 1, 10).round().astype(int).tolist()))]:
        print(fmt('  set %d' % k, iae[k], work[k]) + gains(k))
    best = int(iae.argmin())
    print(fmt('lowest IAE: set %d' % best, iae[best], work[best]) + gains(best))
    res = {'sets': K, 'directions': D, 'envs': n, 'steps': T, 'ms': ms, 'peak_bytes': int(peak), 'front': front,
           'mean_iae': iae.tolist(), 'mean_work': work.tolist(), 'actors': {k: {'IAE': v[0], 'work': v[1].tolist()} for k, v in actors.items()}}
    for who, (a_iae, a_work) in actors.items():
        fair = np.flatnonzero(tot <= a_work.sum())
        if len(fair):
            k = int(fair[iae[fair].argmin()])
            print(fmt('lowest IAE at <= the work of the %s: set %d' % (who, k), iae[k], work[k]) + gains(k))
        else:
            k = int(tot.argmin())
            print('no set spends as little work as the %s (%.1f); the least: ' % (who, a_work.sum()) + fmt('set %d' % k, iae[k], work[k]) + gains(k))
    same = np.flatnonzero(iae <= iae[0])
    k = int(same[tot[same].argmin()])
    print('the default spends %.1f; the cheapest set with IAE <= the default\'s: ' % tot[0] + fmt('set %d' % k, iae[k], work[k]) + gains(k))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
