#!/usr/bin/env python3
"""The baseline DP controller's closed-loop launch (dpenv_controller_rollout) against its yardstick: dpenv_rollout with step_one_wave=1
on a pre-made action block - the same one-wave T-step loop minus the law, the parent's kernel.  One process, device events, the arms
alternating launch by launch, medians of --reps launches of --steps steps at --envs envs.  Also: the eager composition (env.step plus
the law in torch on the device), and a 1 250-step streamed box test with scoring, calm and in 0.2 m/s from 16 directions, with the IAE
and work it scores (beside the thesis actor's with --actor).  --table adds the per-env controller table's arm (every row the defaults:
the same flight through controller_rollout_tab_kernel), alternating with the scalar arm launch by launch, and the packing kernel's time.
    python tools/time_controller.py [--envs 65536] [--steps 50] [--reps 20] [--actor] [--table] [--no-box] [--out time_controller.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn):
    """Milliseconds of fn() on the current stream, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--eager-reps', type=int, default=5)
    ap.add_argument('--box-steps', type=int, default=1250)
    ap.add_argument('--actor', action='store_true', help='fly the thesis actor (tests/golden/final_policy.npz) through the same box tests')
    ap.add_argument('--table', action='store_true', help='also time the per-env controller table form and its packing kernel')
    ap.add_argument('--no-box', action='store_true', help='skip the eager composition and the box tests')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import numpy as np
    import torch
    import ml4ca_amd
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import BatchedDPController, dp_controller_table
    from ml4ca_amd.policy import controller_rollout
    dev = torch.device('cuda', 0)
    n, T = args.envs, args.steps
    res = {'envs': n, 'steps': T, 'reps': args.reps}

    # ---- the launch against its yardstick, the filter off and on ----
    env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=1, step_one_wave=True)
    env.set_dp_controller()
    env.reset()
    out = {False: controller_rollout(env, T)}
    actions = out[False]['act'].clone()
    yard = env.rollout(actions)
    env.set_reference_filter()
    out[True] = controller_rollout(env, T)
    env.set_reference_filter(None)
    ts = {'yardstick': [], False: [], True: []}
    for k in range(args.warm + args.reps):
        t = {'yardstick': timed(torch, lambda: env.rollout(actions, out=yard)),
             False: timed(torch, lambda: controller_rollout(env, T, out=out[False]))}
        env.set_reference_filter()
        t[True] = timed(torch, lambda: controller_rollout(env, T, out=out[True]))
        env.set_reference_filter(None)
        if k >= args.warm:
            for key, v in t.items():
                ts[key].append(v / T * 1e3)
    med = {k: median(v) for k, v in ts.items()}
    res['launch'] = {'yardstick_us_per_step': med['yardstick'], 'controller_us_per_step': med[False], 'controller_filter_us_per_step': med[True],
                     'ratio': med[False] / med['yardstick'], 'ratio_filter': med[True] / med['yardstick'],
                     'min_us_per_step': {str(k): min(v) for k, v in ts.items()}}
    print('%d envs, %d-step launches, medians of %d: yardstick (dpenv_rollout, one wave) %.2f us/step; controller %.2f (x %.3f); with the '
          'reference filter %.2f (x %.3f)' % (n, T, args.reps, med['yardstick'], med[False], med[False] / med['yardstick'], med[True],
                                              med[True] / med['yardstick']), flush=True)
    assert bool(torch.isfinite(out[False]['act']).all()) and bool(torch.isfinite(out[True]['ref']).all())

    # ---- the per-env table form against the scalar form: the same flight, operands per lane ----
    if args.table:
        table = torch.from_numpy(dp_controller_table(n, env.dp_controller)).to(dev)
        env.set_dp_controller_table(table)                          # (the first call allocates the packed block; rows checked once)
        tt = {('scalar', False): [], ('table', False): [], ('scalar', True): [], ('table', True): [], 'pack': []}
        for k in range(args.warm + args.reps):
            t = {}
            for filt in (False, True):
                if filt:
                    env.set_reference_filter()
                env.set_dp_controller_table(None)
                t[('scalar', filt)] = timed(torch, lambda: controller_rollout(env, T, out=out[filt])) / T * 1e3
                t['pack'] = timed(torch, lambda: env.set_dp_controller_table(table, check=False)) * 1e3
                t[('table', filt)] = timed(torch, lambda: controller_rollout(env, T, out=out[filt])) / T * 1e3
                if filt:
                    env.set_reference_filter(None)
            if k >= args.warm:
                for key, v in t.items():
                    tt[key].append(v)
        m = {key: median(v) for key, v in tt.items()}
        res['table'] = {'scalar_us_per_step': m[('scalar', False)], 'table_us_per_step': m[('table', False)],
                        'ratio': m[('table', False)] / m[('scalar', False)], 'scalar_filter_us_per_step': m[('scalar', True)],
                        'table_filter_us_per_step': m[('table', True)], 'ratio_filter': m[('table', True)] / m[('scalar', True)],
                        'pack_us': m['pack']}
        print('per-env table, %d envs, %d-step launches, arms alternating, medians of %d: scalar %.2f us/step, table %.2f (x %.3f); with the '
              'reference filter scalar %.2f, table %.2f (x %.3f); packing kernel (setter call, one launch) %.1f us' % (
                  n, T, args.reps, m[('scalar', False)], m[('table', False)], res['table']['ratio'], m[('scalar', True)], m[('table', True)],
                  res['table']['ratio_filter'], m['pack']), flush=True)
        env.set_dp_controller_table(None)
    if args.no_box:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(res, open(args.out, 'w'), indent=1)
        return

    # ---- the eager composition: env.step + the law in torch on the device ----
    ctrl = BatchedDPController(n, env.dp_controller, dt=env.control_period, device=dev)
    obs = env.reset().clone()

    def eager():
        o = obs
        for _ in range(T):
            o, _, done, _ = env.step(ctrl.act(o).contiguous())
            ctrl.reset(done != 0)

    te = [timed(torch, eager) / T * 1e3 for _ in range(1 + args.eager_reps)][1:]
    res['eager_us_per_step'] = median(te)
    res['eager_over_fused'] = median(te) / med[False]
    print('eager composition (env.step + the law in torch): %.1f us/step = %.1f x the fused launch' % (median(te), median(te) / med[False]), flush=True)
    del env

    # ---- the streamed box test with scoring, on the default hull ----
    box = ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=2, current=True)
    if args.actor:
        from ml4ca_amd.policy import ActorCritic
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'final_policy.npz'))
        ActorCritic.from_tensors({k.replace('.', '/'): d[k] for k in d.files if '.' in k}, device=dev).upload(box)
    beta = ((2 * math.pi / 16) * (torch.arange(n, device=dev) % 16).float()).contiguous()
    res['box'] = {}
    for name, vc in (('calm', 0.0), ('0.2 m/s from 16 directions', 0.2)):
        box.set_current(torch.full((n,), vc, device=dev), beta)
        for filt in (False, True):
            runs = [('baseline', lambda: EV.baseline_box_test_streamed(box, T=args.box_steps, reference_filter=filt))]
            if args.actor:
                runs.append(('actor', lambda: EV.deployment_box_test_streamed(box, T=args.box_steps, integral=False, reference_filter=filt)))
                runs.append(('actor + integral action', lambda: EV.deployment_box_test_streamed(box, T=args.box_steps, integral=True,
                                                                                               reference_filter=filt)))
            for who, fly in runs:
                if who.startswith('actor + integral') and not filt:
                    continue                                     # (chunk 50 needs no eager step, but the node flew behind its filter)
                st = {}
                ms = timed(torch, lambda: st.update(fly()))
                r = {'ms': ms, 'IAE_mean': float(st['iae'].mean()), 'IAE_max': float(st['iae'].max()), 'work_mean': [float(x) for x in st['work'].mean(0)]}
                res['box']['%s / %s / %s' % (name, 'filter' if filt else 'steps', who)] = r
                print('box test %4d steps, %-27s %-7s %-24s %7.1f ms  IAE mean %.2f max %.2f  work bow/port/star %s' % (
                    args.box_steps, name, 'filter' if filt else 'steps', who, ms, r['IAE_mean'], r['IAE_max'], [round(x, 1) for x in r['work_mean']]),
                    flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
