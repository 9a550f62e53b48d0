#!/usr/bin/env python3
"""Closed-loop launch forms side by side (same call, same box): us per env step of dpenv_policy_rollout for every arithmetic x launch
form at 65 536 envs (256-env workgroups: an env and a network wave per SIMD) and 32 768 envs (128-env workgroups: a SIMD per wave).
--integral times the integral action on against off; --reference-filter times the setpoint reference filter on against off (with the
integral action on in both arms if --integral is given too).
    python tools/time_closed_loop.py [--envs 65536,32768] [--steps 50] [--reps 8] [--out gpurun_out/closed_loop_forms.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='65536,32768')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warm', type=int, default=40, help='untimed launches first: the MFMA-heavy forms wobble by 10-30 %% for the first ~20 launches of a process (clock / power ramp)')
    ap.add_argument('--out', default='')
    ap.add_argument('--integral', action='store_true', help='time every form with the deployed node\'s integral action (dpenv_set_integral_action, '
                    'the node\'s parameters) off and on, alternating launch by launch in one process; prints the ratio on / off of the medians')
    ap.add_argument('--reference-filter', action='store_true', help='time every form with the setpoint reference filter (dpenv_set_reference_filter, '
                    'the recorded fit) off and on, alternating launch by launch in one process; with --integral the integral action is on in both')
    ap.add_argument('--forms', default='f16:two_wave,f16:one_wave,f32_actor:two_wave,f32_actor:one_wave,f32:two_wave,f32:one_wave')
    args = ap.parse_args()
    import torch
    import ml4ca_amd
    from ml4ca_amd import DpenvError
    from ml4ca_amd.policy import ActorCritic, policy_rollout
    dev = torch.device('cuda', 0)
    res = {}
    for n in [int(x) for x in args.envs.split(',')]:
        env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, auto_reset=True, seed=1)
        ac = ActorCritic(9, 7, (80, 80, 80), seed=0, device=dev)
        for spec in args.forms.split(','):
            prec, form = spec.split(':')
            try:
                ac.upload(env, precision=prec, launch_form=form)
            except DpenvError as e:
                res['%d/%s' % (n, spec)] = 'refused: %s' % e
                print('%7d %-22s refused (%s)' % (n, spec, str(e)[:60]), flush=True)
                continue
            env.reset()
            if args.reference_filter:
                res['%d/%s' % (n, spec)] = time_reference_filter(env, args, n, spec)
                continue
            if args.integral:
                res['%d/%s' % (n, spec)] = time_integral(env, args, n, spec)
                continue
            out = policy_rollout(env, args.steps, sample=True)
            for _ in range(args.warm):
                policy_rollout(env, args.steps, sample=True, out=out)
            torch.cuda.synchronize()
            best = 1e9
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                policy_rollout(env, args.steps, sample=True, out=out)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / args.steps * 1e6)
            ts.sort()
            res['%d/%s' % (n, spec)] = {'us_per_step_median': ts[len(ts) // 2], 'us_per_step_min': ts[0], 'env_steps_per_s': n / (ts[len(ts) // 2] * 1e-6)}
            print('%7d %-22s %7.2f us/step (min %6.2f)  %.3g env-steps/s' % (n, spec, ts[len(ts) // 2], ts[0], n / (ts[len(ts) // 2] * 1e-6)), flush=True)
            assert bool(torch.isfinite(out['logp']).all())
        del env
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, 'w'), indent=1)


def time_integral(env, args, n, spec):
    """us per env step with the integral action off and on, alternating launch by launch (same process, same state stream)."""
    import torch
    from ml4ca_amd.policy import policy_rollout
    outs, ts = {}, {False: [], True: []}
    for k in range(args.warm + args.reps):
        for on in (False, True):
            env.set_integral_action() if on else env.set_integral_action(None)
            outs[on] = policy_rollout(env, args.steps, sample=True, out=outs.get(on))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            policy_rollout(env, args.steps, sample=True, out=outs[on])
            torch.cuda.synchronize()
            if k >= args.warm:
                ts[on].append((time.perf_counter() - t0) / args.steps * 1e6)
    env.set_integral_action(None)
    med = {on: sorted(v)[len(v) // 2] for on, v in ts.items()}
    assert bool(torch.isfinite(outs[True]['integ']).all())
    print('%7d %-22s off %7.2f  on %7.2f us/step (min %6.2f / %6.2f)  on/off %.3f' % (n, spec, med[False], med[True], min(ts[False]),
                                                                                    min(ts[True]), med[True] / med[False]), flush=True)
    return {'us_per_step_median_off': med[False], 'us_per_step_median_on': med[True], 'us_per_step_min_off': min(ts[False]),
            'us_per_step_min_on': min(ts[True]), 'on_over_off': med[True] / med[False]}


def time_reference_filter(env, args, n, spec):
    """us per env step with the reference filter off and on, alternating launch by launch (same process, same state stream); the
    integral action on in both arms with --integral."""
    import torch
    from ml4ca_amd.policy import policy_rollout
    if args.integral:
        env.set_integral_action()
    outs, ts = {}, {False: [], True: []}
    for k in range(args.warm + args.reps):
        for on in (False, True):
            env.set_reference_filter() if on else env.set_reference_filter(None)
            outs[on] = policy_rollout(env, args.steps, sample=True, out=outs.get(on))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            policy_rollout(env, args.steps, sample=True, out=outs[on])
            torch.cuda.synchronize()
            if k >= args.warm:
                ts[on].append((time.perf_counter() - t0) / args.steps * 1e6)
    env.set_reference_filter(None)
    env.set_integral_action(None)
    med = {on: sorted(v)[len(v) // 2] for on, v in ts.items()}
    assert bool(torch.isfinite(outs[True]['ref']).all())
    print('%7d %-22s %s off %7.2f  on %7.2f us/step (min %6.2f / %6.2f)  on/off %.3f' % (
        n, spec, 'integ' if args.integral else '     ', med[False], med[True], min(ts[False]), min(ts[True]), med[True] / med[False]), flush=True)
    return {'integral': bool(args.integral), 'us_per_step_median_off': med[False], 'us_per_step_median_on': med[True],
            'us_per_step_min_off': min(ts[False]), 'us_per_step_min_on': min(ts[True]), 'on_over_off': med[True] / med[False]}


if __name__ == '__main__':
    main()
