#!/usr/bin/env python3
"""PPO-clip on the batched ReVolt DP environment with the rollout entirely inside one launch per epoch.

Host-side glue around the accelerated path.  The update runs either way: --update torch (the default) is autograd and
torch.optim.Adam, the form SURVEY section 2 row 9 scoped out of the hot path; --update fused runs the 80 + 80 gradient steps as the
library's kernels (ml4ca_amd/train.py: PPO-clip and MSE gradients on the matrix cores, Adam gated on the KL on the device), since
with the rollout at 3 ms the update is where an epoch's time goes.  The algorithm and hyper-parameters are the reference's (spinup/algos/tf1/ppo/ppo.py:109-347, train.py:29-55,
config.json of the shipped run): clip 0.2, pi_lr 3e-4, vf_lr 1e-3, <= 80 policy iterations with early stop at
KL > 1.5 * 0.01, 80 value iterations, gamma 0.99, lambda 0.97, hidden 3 x 80 leaky-relu, T = 400.
What differs is the rollout: N environments x T steps from ONE dpenv_policy_rollout launch (actor, sampling,
env.step, critic, trajectory rows), GAE by one scan kernel, advantage statistics by device reductions.

    python examples/train_ppo.py --envs 4096 --epochs 30
    python examples/train_ppo.py --envs 4096 --epochs 30 --update fused
    python examples/train_ppo.py --envs 4096 --epochs 30 --update fused --warm-start 300 --eval      clone the PID + pseudo-inverse baseline into the
                                                                                      actor first (PPOUpdater.pretrain on one controller_rollout), then PPO
    python examples/train_ppo.py --envs 4096 --epochs 30 --update fused --warm-start 300 --dagger 5 --eval      ... then DAgger: fly the clone, label ITS
                                                                                      states with the baseline (policy.controller_label), aggregate, refit
    python examples/train_ppo.py --envs 4096 --epochs 30 --update fused --warm-start 300 --dagger 5 --expert qp --eval      the same with the PID + QP
                                                                                      chain as the expert: it flies the demonstration and labels the rounds
    python examples/train_ppo.py --envs 4096 --epochs 30 --update fused --warm-start 300 --dagger 5 --expert qp --expert-state flown --eval      ... each
                                                                                      row labelled from the thruster state the ACTOR's last action left
    python examples/train_ppo.py --envs 4096 --epochs 40 --randomise 0.15 --eval      domain randomisation: every episode of every env
                                                                                      runs on its own hull, +-15 % on all 26 parameters, re-drawn by the reset path
                                                                                      inside the rollout launch; --eval: the reference's evaluation harness
                                                                                      (test_policy.py:97-186) and the box test (IAE, energy) on the NOMINAL hull
    python examples/train_ppo.py --envs 4096 --epochs 30 --eval --nn-allocator 5000   ... with the supervised neural allocator (src/sl) fitted and flown
                                                                                      behind the baseline's PID beside the pseudo-inverse and the QP
    python examples/train_ppo.py --envs 4096 --epochs 30 --eval --nn-allocator 5000 --nn-loss wrench --nn-w-power 0.05
                                                                                      ... the same network trained through the force map (the allocation loss)
    python examples/train_ppo.py --envs 4096 --epochs 1 --eval --tune-nn 8            the neural allocator's IAE / work front in ONE flight: 8 wrench-loss
                                                                                      fits (w_power 0, 0.01 .. 1), one network per 64 envs
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ml4ca_amd
from ml4ca_amd import dist as D
from ml4ca_amd import rollout
from ml4ca_amd.policy import ActorCritic


def iadc_text(s):
    """'  IADC total (rps part + angle part)' of a box-test result scored with wear=True: the thesis' wear axis, means over the envs."""
    return '  IADC %.2f (rps %.2f + angle %.2f)' % (float(s['iadc'].mean()), float(s['iadc_rps'].mean()), float(s['iadc_angle'].mean()))


def iadc_entries(s):
    return {'IADC': float(s['iadc'].mean()), 'IADC_rps': float(s['iadc_rps'].mean()), 'IADC_angle': float(s['iadc_angle'].mean())}


def evaluate_actor(ac, dev, preset, precision, seed, out=print, eval_envs=1024, only=None, nn_net=None):
    """The trained actor on the NOMINAL hull (and on a spread of hulls): the reference's run_RL_policy (spinup/utils/test_policy.py:97-186: six
    fixed starts, deterministic policy) and the thesis' 4-corner box test with its three metrics - IAE (results/all_plots/common.py:60-74),
    the energy-equivalent work of the thruster power model (box_test/plot_act.py:128-135,184-211) and IADC, the wear of the commands
    (box_test/plot_act.py:320-391), on every contender's line."""
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import dp_controller_defaults, qp_allocator_defaults
    from ml4ca_amd.policy import policy_rollout
    nominal = ml4ca_amd.default_vessel(preset)
    env6 = ml4ca_amd.BatchedRevoltEnv(6, device=dev, auto_reset=False, testing=True, vessel_params=nominal)
    ac.upload(env6, precision=precision)
    r = EV.run_RL_policy(env6, ac)
    out('eval  run_RL_policy on the nominal hull (six fixed starts, deterministic actor): EpRet %s  EpLen %s' % (
        [round(float(x), 1) for x in r['EpRet']], [int(x) for x in r['EpLen']]))
    res = {'EpRet_mean': float(r['EpRet'].mean()), 'EpLen_mean': float(r['EpLen'].float().mean())}
    T, nb = 1250, int(eval_envs)
    # (the last two rows: the thesis' current box test - 0.2 m/s towards 135 deg, results/all_plots/current_box_test/plot_pos.py:78 - and a spread
    # of currents around it: +-0.1 m/s, +-90 deg, one draw per env)
    for tag, spread, cur in (('nominal hull', 0.0, None), ('hulls +-15 %', 0.15, None), ('hulls +-30 %', 0.30, None), ('hulls +-50 %', 0.50, None),
                             ('current 0.2 m/s @ 135 deg', 0.0, (0.0, 0.0)), ('currents 0.2 +-0.1 m/s, 135 +-90 deg', 0.0, (0.1, 1.5708))):
        if only is not None and tag not in only:
            continue
        def make_env():
            env = ml4ca_amd.BatchedRevoltEnv(nb, device=dev, terminate=False, time_limit=False, seed=seed + 77, vessel_params=nominal, current=cur is not None)
            if spread > 0:
                env.set_vessel_randomisation(spread, nominal=nominal)      # one draw per env at the first reset; no resets after it
            if cur is not None:
                env.set_current(torch.full((nb,), 0.2, device=dev), torch.full((nb,), 2.35619, device=dev))
                if cur[0] > 0:
                    env.set_current_randomisation(cur[0], cur[1])          # one draw per env at the first reset
            return env

        def baseline():
            # the classical chain on the same envs, hulls and currents (a handle made the same way draws the same ones): PID + pseudo-inverse
            # with the pole-placement defaults of the NOMINAL hull (deploy.dp_controller_defaults), flown in 50-step launches
            envb = make_env()
            envb.set_dp_controller(dp_controller_defaults(nominal))
            sb = EV.baseline_box_test_streamed(envb, T=T, start=torch.zeros((3, nb), device=dev), chunk=50, wear=True)
            out('eval  box test (1250 steps, %d envs), %-13s: baseline PID + pseudo-inverse IAE %.2f (worst env %.2f)  work bow/port/star %s%s' % (
                nb, tag, float(sb['iae'].mean()), float(sb['iae'].max()), [round(float(x), 1) for x in sb['work'].mean(0)], iadc_text(sb)))
            rb = {'IAE': float(sb['iae'].mean()), 'IAE_worst': float(sb['iae'].max()), 'work': [float(x) for x in sb['work'].mean(0)], **iadc_entries(sb)}
            if nn_net is not None:
                # the supervised contender (--nn-allocator): the same PID with the fitted network in place of the pseudo-inverse; it touches
                # no hull, so it flies the spreads of hulls too - on a handle made the same way, which draws the same hulls and currents
                envn = make_env()
                envn.set_dp_controller(dp_controller_defaults(nominal))
                sn = EV.baseline_box_test_streamed(envn, T=T, start=torch.zeros((3, nb), device=dev), chunk=50, allocator='nn', net=nn_net, wear=True)
                out('eval  box test (1250 steps, %d envs), %-13s: baseline PID + neural allocation IAE %.2f (worst env %.2f)  work bow/port/star %s%s' % (
                    nb, tag, float(sn['iae'].mean()), float(sn['iae'].max()), [round(float(x), 1) for x in sn['work'].mean(0)], iadc_text(sn)))
                rb['nn'] = {'IAE': float(sn['iae'].mean()), 'IAE_worst': float(sn['iae'].max()), 'work': [float(x) for x in sn['work'].mean(0)],
                            **iadc_entries(sn)}
                del envn
            if spread > 0:
                return rb                                                  # (the QP allocation flies the shared hull only: no per-env hull blocks)
            # the thesis' third contender: the same PID with the rate-limited QP allocation in place of the pseudo-inverse
            envb.set_qp_allocator(qp_allocator_defaults(nominal))
            sq = EV.baseline_box_test_streamed(envb, T=T, start=torch.zeros((3, nb), device=dev), chunk=50, allocator='qp', wear=True)
            out('eval  box test (1250 steps, %d envs), %-13s: baseline PID + QP allocation IAE %.2f (worst env %.2f)  work bow/port/star %s%s' % (
                nb, tag, float(sq['iae'].mean()), float(sq['iae'].max()), [round(float(x), 1) for x in sq['work'].mean(0)], iadc_text(sq)))
            rb['qp'] = {'IAE': float(sq['iae'].mean()), 'IAE_worst': float(sq['iae'].max()), 'work': [float(x) for x in sq['work'].mean(0)],
                        **iadc_entries(sq)}
            return rb

        env = make_env()
        ac.upload(env, precision=precision)
        start = torch.zeros((3, nb), device=dev)
        if nb != 1024:
            # any other batch: the same flight in 50-step launches through one re-used set of row blocks, scored on the device as it flies
            # (evaluate.ScoreCard: O(n) memory - 65 536 envs fit); the corner errors need the rows and are not reported
            st = EV.deployment_box_test_streamed(env, T=T, chunk=50, integral=False, start=start, wear=True)
            iae_tot, w, rps = st['iae'], st['work'], float(st['ret'].mean()) / T
            out('eval  box test (1250 steps, %d envs, streamed), %-13s: IAE %.2f (worst env %.2f)  work bow/port/star %s%s  reward/step %.3f' % (
                nb, tag, float(iae_tot.mean()), float(iae_tot.max()), [round(float(x), 1) for x in w.mean(0)], iadc_text(st), rps))
            res[tag] = {'IAE': float(iae_tot.mean()), 'IAE_worst': float(iae_tot.max()), 'work': [float(x) for x in w.mean(0)], 'reward_per_step': rps,
                        **iadc_entries(st)}
            del env
            res[tag]['baseline'] = baseline()
            continue
        env.reset(init=torch.zeros((6, nb), device=dev), new_ref=start.clone())
        steps, refs = EV.box_schedule(start)
        o = policy_rollout(env, T, noise=None, switch_steps=steps, refs=refs)
        iae_tot, _ = EV.iae(o['obs'])
        w = EV.work(EV.commanded_thrust(o['act']))
        wear = EV.iadc(o['act'], env.variant, env.cont_ang)
        e = o['obs'][:, :, :3]
        k = [max(t - 1, 0) for t in list(steps)[1:] + [T - 1]]             # just before each switch: how close to the corner
        pos = torch.sqrt(e[k, :, 0] ** 2 + e[k, :, 1] ** 2)
        out('eval  box test (1250 steps, %d envs), %-13s: IAE %.2f (worst env %.2f)  work bow/port/star %s%s  corner error %.2f m / %.1f deg (worst %.2f m)  reward/step %.3f' % (
            nb, tag, float(iae_tot.mean()), float(iae_tot.max()), [round(float(x), 1) for x in w.mean(0)], iadc_text(wear), float(pos.mean()),
            float(torch.rad2deg(e[k, :, 2].abs().mean())), float(pos.max()), float(o['rew'].mean())))
        res[tag] = {'IAE': float(iae_tot.mean()), 'IAE_worst': float(iae_tot.max()), 'work': [float(x) for x in w.mean(0)],
                    'corner_error_m': float(pos.mean()), 'reward_per_step': float(o['rew'].mean()), **iadc_entries(wear)}
        del env
        res[tag]['baseline'] = baseline()
    return res


def tune_baseline(ac, dev, preset, precision, K, seed=0, out=print, directions=16, vc=0.2):
    """The baseline's trade-off curve beside the actor (evaluate.baseline_gain_sweep): K gain sets around the pole-placement defaults
    (deploy.gain_population; set 0 is the default baseline) x 16 current directions in ONE scored box test behind the reference filter,
    every env on its own row of the per-env controller table, and the actor (no integral action) flown in the same currents."""
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import dp_controller_defaults, gain_population
    nominal = ml4ca_amd.default_vessel(preset)
    n = K * directions
    env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=seed + 77, vessel_params=nominal, current=True)
    pop = gain_population(K, dp_controller_defaults(nominal), seed=seed)
    env.set_dp_controller(dp_controller_defaults(nominal))
    sw = EV.baseline_gain_sweep(env, pop, directions=directions, vc=vc, reference_filter=True, wear=True)
    iae, work, wear = sw['mean_iae'].cpu().numpy(), sw['mean_work'].cpu().numpy(), sw['mean_iadc'].cpu().numpy()
    tot = work.sum(1)
    ac.upload(env, precision=precision)
    sa = EV.deployment_box_test_streamed(env, chunk=50, integral=False, reference_filter=True, wear=True)       # (the sweep left the currents set)
    a_iae, a_work = float(sa['iae'].mean()), sa['work'].mean(0).cpu().numpy()
    row = lambda k: 'set %4d  IAE %.2f  work bow/port/star %s (total %.1f)  IADC %.2f  kp x %s  kd x %s  ki x %s' % (
        k, iae[k], [round(float(x), 1) for x in work[k]], tot[k], wear[k], *([round(float(x), 2) for x in pop['factors'][g][k]] for g in ('kp', 'kd', 'ki')))
    out('tune  %d gain sets x %d directions of %.1f m/s, 1250-step box test behind the reference filter' % (K, directions, vc))
    out('tune  actor (no integral action): IAE %.2f  work bow/port/star %s (total %.1f)%s' % (a_iae, [round(float(x), 1) for x in a_work], a_work.sum(), iadc_text(sa)))
    out('tune  default baseline : ' + row(0))
    out('tune  front (%d of %d sets, by IAE):' % (len(sw['front']), K))
    for k in sw['front']:
        out('tune      ' + row(int(k)))
    best = int(iae.argmin())
    out('tune  lowest IAE       : ' + row(best))
    fair = [int(k) for k in range(K) if tot[k] <= a_work.sum()]
    if fair:
        out('tune  lowest IAE at no more than the actor\'s work: ' + row(min(fair, key=lambda k: iae[k])))
    else:
        out('tune  no gain set spends as little work as the actor (the least: ' + row(int(tot.argmin())) + ')')
    out('tune  front on IAE, work and IADC: %d of %d sets' % (len(sw['front3']), K))
    return {'mean_iae': iae.tolist(), 'mean_work': work.tolist(), 'mean_iadc': wear.tolist(), 'front': [int(k) for k in sw['front']],
            'front3': [int(k) for k in sw['front3']], 'actor': {'IAE': a_iae, 'work': a_work.tolist(), **iadc_entries(sa)}}


def tune_qp(dev, preset, K, seed=0, out=print, directions=16, vc=0.2):
    """The QP allocator's trade-off curve beside tune_baseline's (evaluate.qp_weight_sweep): K weight sets around the reference's weights
    (deploy.qp_weight_population; set 0 is the default QP) x 16 current directions in ONE scored box test behind the reference filter,
    every env on its own row of the per-env QP table, the PID the hull's default controller."""
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import dp_controller_defaults, qp_allocator_defaults, qp_weight_population
    nominal = ml4ca_amd.default_vessel(preset)
    n = K * directions
    env = ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=seed + 77, vessel_params=nominal, current=True)
    pop = qp_weight_population(K, qp_allocator_defaults(nominal), seed=seed)
    env.set_dp_controller(dp_controller_defaults(nominal))
    sw = EV.qp_weight_sweep(env, pop, directions=directions, vc=vc, reference_filter=True, wear=True)
    iae, work, wear = sw['mean_iae'].cpu().numpy(), sw['mean_work'].cpu().numpy(), sw['mean_iadc'].cpu().numpy()
    tot = work.sum(1)
    names = ('w_power', 'w_dalpha', 'w_dforce')
    row = lambda k: 'set %4d  IAE %.2f  work bow/port/star %s (total %.1f)  IADC %.2f  %s' % (
        k, iae[k], [round(float(x), 1) for x in work[k]], tot[k], wear[k], '  '.join('%s x %.2f' % (g, float(pop['factors'][g][k])) for g in names))
    out('tuneqp  %d QP weight sets x %d directions of %.1f m/s, 1250-step box test behind the reference filter' % (K, directions, vc))
    out('tuneqp  default QP       : ' + row(0))
    out('tuneqp  front (%d of %d sets, by IAE):' % (len(sw['front']), K))
    for k in sw['front']:
        out('tuneqp      ' + row(int(k)))
    out('tuneqp  lowest IAE       : ' + row(int(iae.argmin())))
    out('tuneqp  least work       : ' + row(int(tot.argmin())))
    out('tuneqp  least wear       : ' + row(int(wear.argmin())))
    out('tuneqp  front on IAE, work and IADC: %d of %d sets' % (len(sw['front3']), K))
    return {'mean_iae': iae.tolist(), 'mean_work': work.tolist(), 'mean_iadc': wear.tolist(), 'front': [int(k) for k in sw['front']],
            'front3': [int(k) for k in sw['front3']]}


def nn_w_power_grid(K):
    """--tune-nn's power weights: 0 (no power term: the tracking end of the front), then K - 1 values spaced evenly in the logarithm from
    0.01 to 1 (the QP's own weight: the thrifty end); K = 1 is 0.05, the README's one-at-a-time pick."""
    import numpy as np
    if K == 1:
        return [0.05]
    return [0.0] + [float(w) for w in np.geomspace(0.01, 1.0, K - 1)]


def tune_nn(args, dev, preset, K, seed=0, out=print, directions=16, vc=0.2):
    """The neural allocator's trade-off curve beside tune_qp's (evaluate.nn_allocator_sweep): K wrench-loss fits, one per w_power of
    nn_w_power_grid(K) (train.fit_nn_allocator_population; --nn-allocator ITERS Adam steps each, 5000 if not given), flown as ONE
    population - network k on envs 64 k .. 64 k + 63, four envs per current direction - in one scored box test behind the reference
    filter; then the same K box tests one network at a time, for the clock and as a check (the per-env scores are equal)."""
    import math
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import dp_controller_defaults, nn_allocator_dataset
    from ml4ca_amd.train import alloc_loss_params, fit_nn_allocator_population
    nominal = ml4ca_amd.default_vessel(preset)
    grid = nn_w_power_grid(K)
    iters = args.nn_allocator or 5000
    t0 = time.perf_counter()
    nets = fit_nn_allocator_population(nn_allocator_dataset(16384, seed, vessel=nominal), grid, alloc_loss=alloc_loss_params(None, vessel=nominal),
                                       iters=iters, seed=seed, device=dev)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    mk = lambda n: ml4ca_amd.BatchedRevoltEnv(n, device=dev, terminate=False, time_limit=False, seed=seed + 77, vessel_params=nominal, current=True)
    env = mk(64 * K)
    env.set_dp_controller(dp_controller_defaults(nominal))
    t0 = time.perf_counter()
    sw = EV.nn_allocator_sweep(env, nets, directions=directions, vc=vc, reference_filter=True, wear=True)
    torch.cuda.synchronize()
    t_sweep = time.perf_counter() - t0
    one = mk(64)
    one.set_dp_controller(dp_controller_defaults(nominal))
    one.set_current(torch.full((64,), float(vc), device=dev), ((2.0 * math.pi / directions) * (torch.arange(64, device=dev) % directions).float()).contiguous())
    t0 = time.perf_counter()
    seq = [EV.baseline_box_test_streamed(one, reference_filter=True, chunk=50, allocator='nn', net=net) for net in nets]
    torch.cuda.synchronize()
    t_seq = time.perf_counter() - t0
    same = all(torch.equal(sw['env_iae'][64 * k:64 * k + 64], r['iae']) and torch.equal(sw['env_work'][64 * k:64 * k + 64], r['work'])
               for k, r in enumerate(seq))
    iae, work, wear = sw['mean_iae'].cpu().numpy(), sw['mean_work'].cpu().numpy(), sw['mean_iadc'].cpu().numpy()
    tot = work.sum(1)
    row = lambda k: 'net %4d  w_power %-8.4g IAE %.2f  work bow/port/star %s (total %.1f)  IADC %.2f  wrench residual Js %.4g N^2' % (
        k, grid[k], iae[k], [round(float(x), 1) for x in work[k]], tot[k], wear[k], nets[k]['wrench_ms_final'])
    out('tunenn  %d networks (9-80-80-80-6, wrench loss, %d Adam steps each: %.1f s) x %d directions of %.1f m/s x 4 envs, 1250-step box test behind '
        'the reference filter' % (K, iters, t_fit, directions, vc))
    out('tunenn  w_power grid: %s' % ', '.join('%.4g' % w for w in grid))
    out('tunenn  one flight of the population: %.2f s; the same %d box tests one network at a time: %.2f s (x %.1f); per-env scores %s'
        % (t_sweep, K, t_seq, t_seq / t_sweep, 'equal' if same else 'DIFFER'))
    for k in range(K):
        out('tunenn      ' + row(k))
    out('tunenn  front (%d of %d networks, by IAE):' % (len(sw['front']), K))
    for k in sw['front']:
        out('tunenn      ' + row(int(k)))
    out('tunenn  front on IAE, work and IADC: %d of %d networks' % (len(sw['front3']), K))
    return {'w_power': grid, 'mean_iae': iae.tolist(), 'mean_work': work.tolist(), 'mean_iadc': wear.tolist(), 'front': [int(k) for k in sw['front']],
            'front3': [int(k) for k in sw['front3']], 'seconds': {'fit': t_fit, 'sweep': t_sweep, 'sequential': t_seq}, 'same': same}


def warm_start(upd, env, args, out=print):
    """--warm-start: clone the classical baseline into the actor before epoch 0.  The baseline (PID + pseudo-inverse with the pole-placement
    defaults of the nominal hull) flies the training envs for --warm-start-steps steps in one launch; its obs / act rows are the
    demonstration PPOUpdater.pretrain fits the actor to, and their discounted returns what pretrain_critic fits the critic to.  The
    actor is memoryless: it sees o, not the PID's integral z, so in a current the clone holds station with an offset unless it is flown
    with env.set_integral_action().  --expert qp: the same PID with the rate-limited QP allocation flies the demonstration.
    Several ranks: every rank flies its own envs and draws its own minibatches, exactly as in the PPO epochs with --exchange gradients, and
    every step's gradient-and-statistics buffer is averaged across the ranks (dist.average_flat) before its Adam step, whatever --exchange
    says: the replicas take the same steps and enter PPO with the same parameters (checked once, dist.assert_params_in_step)."""
    from ml4ca_amd.deploy import dp_controller_defaults, qp_allocator_defaults
    from ml4ca_amd.policy import controller_rollout
    T = args.warm_start_steps or args.steps
    env.set_dp_controller(dp_controller_defaults(ml4ca_amd.default_vessel(args.preset)))
    if args.expert == 'qp':                                                       # the demonstration is the PID + QP chain's flight
        env.set_qp_allocator(qp_allocator_defaults(ml4ca_amd.default_vessel(args.preset)))
    env.reset()
    o = controller_rollout(env, T)
    _, ret = rollout.gae(o['rew'], torch.zeros_like(o['rew']), end=o['done'], gamma=0.99, lam=0.97)      # rewards-to-go (ppo.py:88)
    obs, act, ret = o['obs'].reshape(-1, 9).float().contiguous(), o['act'].reshape(-1, 7), ret.reshape(-1)
    mb = min(args.minibatch, obs.shape[0])
    t0 = time.perf_counter()
    h = upd.pretrain(obs, act, args.warm_start, minibatch=mb, loss=args.warm_start_loss, average=D.average_flat)      # (a no-op on one rank)
    hv = upd.pretrain_critic(obs, ret, args.warm_start, minibatch=mb, average=D.average_flat)
    torch.cuda.synchronize()
    D.assert_params_in_step(list(upd.ac.parameters()), what='warm-started parameters')
    if args.expert == 'qp':
        env.set_qp_allocator(off=True)
    env.set_dp_controller(off=True)
    out('warm start: %d rows of the baseline (reward/step %.3f), %d %s steps + as many critic steps in %.2f s: MSE %.4g -> %.4g  NLL %.4g -> %.4g  V-loss %.4g -> %.4g' % (
        obs.shape[0], float(o['rew'].mean()), args.warm_start, args.warm_start_loss, time.perf_counter() - t0,
        float(h[0, 2]), float(h[-1, 2]), float(h[0, 1]), float(h[-1, 1]), float(hv[0, 0]), float(hv[-1, 0])))
    return h, hv


def fit_allocator(args, dev, preset, out=print):
    """--nn-allocator ITERS: the neural allocator fitted for the preset's hull (train.fit_nn_allocator), with the line that says how."""
    from ml4ca_amd.deploy import nn_allocator_dataset
    from ml4ca_amd.train import alloc_loss_params, fit_nn_allocator
    hull = ml4ca_amd.default_vessel(preset)
    wrench = alloc_loss_params(None if args.nn_w_power is None else dict(w_power=args.nn_w_power), vessel=hull)
    base = nn_allocator_dataset(16384, args.seed, vessel=hull)
    nn_net = fit_nn_allocator(base, iters=args.nn_allocator, seed=args.seed, device=dev, loss=args.nn_loss, alloc_loss=wrench)
    out('eval  neural allocator fitted in %d Adam steps, loss %s%s: label MSE %.4g -> %.4g, mean wrench residual Js %.4g -> %.4g N^2' % (
        args.nn_allocator, args.nn_loss, ' (w_power %g)' % wrench['w_power'] if args.nn_loss == 'wrench' else '', nn_net['mse_initial'],
        nn_net['mse_final'], nn_net['wrench_ms_initial'], nn_net['wrench_ms_final']))
    return nn_net, base, wrench


def nn_score_card(nn_net, dev, preset, seed, nb, tag, out=print):
    """The score-card line of the PID + neural allocation on the nominal hull, calm and in the thesis' 0.2 m/s current."""
    from ml4ca_amd import evaluate as EV
    from ml4ca_amd.deploy import dp_controller_defaults
    nominal = ml4ca_amd.default_vessel(preset)
    for name, cur in (('calm', False), ('current 0.2 m/s @ 135 deg', True)):
        env = ml4ca_amd.BatchedRevoltEnv(nb, device=dev, terminate=False, time_limit=False, seed=seed + 77, vessel_params=nominal, current=cur)
        if cur:
            env.set_current(torch.full((nb,), 0.2, device=dev), torch.full((nb,), 2.35619, device=dev))
        env.set_dp_controller(dp_controller_defaults(nominal))
        sn = EV.baseline_box_test_streamed(env, T=1250, start=torch.zeros((3, nb), device=dev), chunk=50, allocator='nn', net=nn_net, wear=True)
        out('eval  box test (1250 steps, %d envs), %s, %s: baseline PID + neural allocation IAE %.2f (worst env %.2f)  work bow/port/star %s (total %.1f)%s' % (
            nb, tag, name, float(sn['iae'].mean()), float(sn['iae'].max()), [round(float(x), 1) for x in sn['work'].mean(0)], float(sn['work'].mean(0).sum()),
            iadc_text(sn)))
        del env


def nn_on_policy(args, dev, preset, base, wrench, out=print):
    """--nn-on-policy ROUNDS: refit the allocator on the wrenches its own closed loop asks of it (train.fit_nn_allocator_on_policy) - training
    envs with auto-reset in a 0.2 m/s current from 16 directions, one episode per round, the dataset's rows kept in the pool."""
    import math
    from ml4ca_amd.deploy import dp_controller_defaults
    from ml4ca_amd.train import fit_nn_allocator_on_policy
    nominal = ml4ca_amd.default_vessel(preset)
    n = args.eval_envs
    env = ml4ca_amd.BatchedRevoltEnv(n, auto_reset=True, seed=args.seed + 31, device=dev, current=True, vessel_params=nominal)
    env.set_current(torch.full((n,), 0.2, device=dev), ((2 * math.pi / 16) * (torch.arange(n, device=dev) % 16).float()).contiguous())
    env.set_dp_controller(dp_controller_defaults(nominal))
    env.reset()
    res = fit_nn_allocator_on_policy(env, args.nn_on_policy, args.steps, args.nn_allocator, base=base, seed=args.seed, alloc_loss=wrench)
    for r, x in enumerate(res['rounds']):
        out('eval  on-policy round %2d: %d rows (%d flown)  J %.4g -> %.4g  mean wrench residual Js %.4g -> %.4g N^2' % (
            r, x['rows'], x['rows'] - res['base']['rows'], x['J_initial'], x['J_final'], x['wrench_ms_initial'], x['wrench_ms_final']))
    return dict(W=res['W'], b=res['b'], leak=res['leak'])


def dagger(upd, env, args, out=print):
    """--dagger: after the warm start (if any) and before PPO, fly the ACTOR on the training envs, label the states it visits with the
    baseline (policy.controller_label: the PID + pseudo-inverse law scanned over the actor's rows in one launch), aggregate the rounds and
    refit (PPOUpdater.dagger).  A clone trained on the expert's states alone has no labels where its own errors take it; these rounds
    supply them.  The labels carry the PID's integral, which the memoryless actor cannot see: it can only fit their mean given o.
    --expert qp labels with the PID + rate-limited QP chain instead (policy.controller_label_qp), whose labels carry its thruster state
    as well.  --expert nn labels with the PID + the fitted neural allocator (policy.controller_label_nn; --nn-allocator ITERS fits it first)."""
    from ml4ca_amd.deploy import dp_controller_defaults, qp_allocator_defaults
    nn_net = fit_allocator(args, env.device, args.preset, out=out)[0] if args.expert == 'nn' else None
    T = args.dagger_steps or args.steps
    nominal = ml4ca_amd.default_vessel(args.preset)
    env.set_dp_controller(dp_controller_defaults(nominal))
    env.reset()
    mb = min(args.minibatch, T * env.n_envs)
    t0 = time.perf_counter()
    # --expert qp: the labels are the PID + QP chain's (policy.controller_label_qp), with the nominal hull's lever arms and thrust constants;
    # the scan touches no hull, so it labels the randomised-hull envs the QP closed loop cannot fly
    rec = upd.dagger(env, args.dagger, T, args.dagger_iters, minibatch=mb, loss=args.warm_start_loss, keep=args.dagger_keep or None,
                     average=D.average_flat, upload=dict(precision=args.precision), expert=args.expert,
                     qp_params=qp_allocator_defaults(nominal) if args.expert == 'qp' else None, thruster_state=args.expert_state,
                     **(dict(nn_net=nn_net) if nn_net is not None else {}))
    torch.cuda.synchronize()
    D.assert_params_in_step(list(upd.ac.parameters()), what='parameters after DAgger')
    env.set_dp_controller(off=True)
    for r, x in enumerate(rec):
        h = x['history']
        out('dagger round %2d: actor reward/step %.3f  |actor - baseline|^2 on its own states %.4g  %d rows  %d %s steps: MSE %.4g -> %.4g  NLL %.4g -> %.4g' % (
            r, x['reward_per_step'], x['label_msd'], x['rows'], h.shape[0], args.warm_start_loss, float(h[0, 2]), float(h[-1, 2]),
            float(h[0, 1]), float(h[-1, 1])))
    out('dagger: %d rounds of %d steps on %d envs in %.2f s' % (len(rec), T, env.n_envs, time.perf_counter() - t0))
    upd.pi_m.zero_()                                                             # PPO starts with a fresh actor optimiser, as after the warm start
    upd.pi_v.zero_()
    upd.pi_steps.zero_()
    upd._pi_steps_host = 0
    return rec


def torch_update(ac, pi_opt, v_opt, pi_params, v_params, obs, act, adv, ret, logp_old, mb, clip=0.2, target_kl=0.01, gather=False, iters=80):
    """The update of ppo.py:265-273 through torch autograd and torch.optim.Adam (--update torch): the baseline the fused update
    (ml4ca_amd.train.PPOUpdater, --update fused) is held to and timed against.  Returns (pi_iters, kl, v_loss)."""
    dev, N = obs.device, obs.shape[0]
    kl, pi_iters = 0.0, 0
    for i in range(iters):                                                  # ppo.py:265-271
        idx = torch.randint(0, N, (mb,), device=dev) if mb < N else slice(None)
        mu = ac._mlp(obs[idx], ac.pi_W, ac.pi_b)
        logp = ac.logp_ref(act[idx], mu)
        ratio = torch.exp(logp - logp_old[idx])
        a = adv[idx]
        pi_loss = -torch.min(ratio * a, torch.clamp(ratio, 1 - clip, 1 + clip) * a).mean()   # ppo.py:238-240
        kl_t = (logp_old[idx] - logp).mean().detach()
        kl = float(kl_t if gather else D.mean_across_ranks(kl_t))             # mpi_avg(kl), ppo.py:267 (identical on every rank when gathered)
        if kl > 1.5 * target_kl:                                            # ppo.py:267-270
            break
        pi_opt.zero_grad()
        pi_loss.backward()
        if not gather:
            D.average_gradients(pi_params)                                 # mpi_tf.py:59-62 (no-op on one rank)
        pi_opt.step()
        pi_iters += 1
    for i in range(iters):                                                  # ppo.py:272-273
        idx = torch.randint(0, N, (mb,), device=dev) if mb < N else slice(None)
        v = ac._mlp(obs[idx], ac.v_W, ac.v_b)[:, 0]
        v_loss = ((ret[idx] - v) ** 2).mean()                               # ppo.py:241
        v_opt.zero_grad()
        v_loss.backward()
        if not gather:
            D.average_gradients(v_params)
        v_opt.step()
    return pi_iters, kl, float(v_loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--steps', type=int, default=400, help='rollout length per epoch = max_ep_len (train.py:70-73)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--minibatch', type=int, default=1 << 18, help='samples per gradient step (full batch in the reference)')
    ap.add_argument('--activation', default='leaky', choices=('leaky', 'relu', 'tanh'), help='hidden activation (train.py:24,31)')
    ap.add_argument('--precision', default='f32', choices=('f16', 'f32', 'f32_actor'),
                    help="in-kernel network arithmetic: 'f32' (split-f16, within 1e-5 of the fp32 update's own evaluation: the PPO ratio starts at 1) or 'f16' (fast)")
    ap.add_argument('--update', default='torch', choices=('torch', 'fused'),
                    help="the 80 + 80 gradient steps: 'torch' = autograd + torch.optim.Adam (torch_update below); 'fused' = the library's gradient and "
                         'gated-Adam kernels (ml4ca_amd.train.PPOUpdater): the whole update queues without a host round trip, one read at the end')
    ap.add_argument('--warm-start', type=int, default=0, metavar='ITERS',
                    help='with --update fused: before epoch 0 fly the baseline DP controller (PID + pseudo-inverse) on the training envs, fit the actor to '
                         'its obs -> act rows for ITERS gradient steps (ml4ca_amd.train.PPOUpdater.pretrain) and the critic to their discounted returns, '
                         'reset Adam, and let PPO fine-tune from there.  The actor is memoryless: it sees o, not the PID\'s integral z, so in a current '
                         'the clone holds station with an offset unless it is flown with env.set_integral_action()')
    ap.add_argument('--warm-start-loss', default='mse', choices=('mse', 'nll'), help="the imitation loss: 'mse' on the mean action, or the Gaussian 'nll' "
                                                                                       '(which also fits log_std)')
    ap.add_argument('--warm-start-steps', type=int, default=0, metavar='T', help='steps of the demonstration flight (default: one episode, --steps)')
    ap.add_argument('--dagger', type=int, default=0, metavar='ROUNDS',
                    help='with --update fused, after --warm-start (if given) and before PPO: ROUNDS x (fly the actor, label the states it visits with the '
                         'baseline DP controller in one launch, aggregate, refit the actor: ml4ca_amd.train.PPOUpdater.dagger); one line per round')
    ap.add_argument('--dagger-iters', type=int, default=100, metavar='ITERS', help='gradient steps per DAgger round (loss: --warm-start-loss)')
    ap.add_argument('--dagger-steps', type=int, default=0, metavar='T', help='steps of each DAgger flight (default: one episode, --steps)')
    ap.add_argument('--dagger-keep', type=int, default=0, metavar='K', help='rounds kept in the aggregated dataset, a ring (default 0: all of them)')
    ap.add_argument('--expert', default='pinv', choices=('pinv', 'qp', 'nn'),
                    help="the expert of --warm-start and --dagger: 'pinv' = PID + pseudo-inverse; 'qp' = the same PID with the rate-limited QP allocation "
                         '(55 %% of the pseudo-inverse\'s thruster work on the box test): the warm-start flight flies it (env.set_qp_allocator), --dagger '
                         'labels with it (policy.controller_label_qp)')
    ap.add_argument('--expert-state', default='own', choices=('own', 'flown'),
                    help="--dagger --expert qp: the thruster state the QP labels a row from: 'own' = the expert's own recursion along the rows; 'flown' = "
                         'the state the ACTOR\'s executed action of the row before left (PPOUpdater.dagger thruster_state), whose thrust part the actor '
                         'sees in its lagged thrust columns')
    ap.add_argument('--exchange', default='gradients', choices=('gradients', 'rollout'),
                    help="multi-rank runs: 'gradients' = every rank updates on ITS OWN episode and the gradients are averaged, exactly the "
                         "reference (ppo.py:226, mpi_tf.py:29-62: no trajectory ever crosses); 'rollout' = BASELINE.json config 4: the ranks "
                         "all-gather the episode (dist.EpisodeExchange: obs | act | logp chunk by chunk under the next chunk's launch, adv | ret "
                         "after the local scan) and every rank runs the identical update on the global batch - no gradient all-reduce")
    ap.add_argument('--chunks', type=int, default=4, help="--exchange rollout: pieces the episode is rolled out and posted in")
    ap.add_argument('--reset-at-end', action='store_true', help='the reference\'s epoch boundary (ppo.py:305-322): every env is cut and re-drawn '
                                                                'after the last step of an epoch (matters when --steps < max_ep_len)')
    ap.add_argument('--randomise', type=float, default=0.0, help='R > 0: domain randomisation - every reset (also the ones inside the rollout launch) draws the '
                                                                  'new episode\'s hull: each of the 26 vessel parameters = nominal x (1 + R u), u ~ U[-1, 1), '
                                                                  'Philox keyed (seed; global env id, episode): independent of the rank count')
    ap.add_argument('--current', default='', help="'V,BETA_DEG': train in a current (e.g. '0.2,135': the reference's one operating point, "
                                                 'results/all_plots/current_box_test/plot_pos.py:78)')
    ap.add_argument('--randomise-current', default='', help="'RV,RB_DEG' with --current: every reset (also inside the rollout launch) draws the new episode's current, "
                                                           'V_c = max(0, V + RV u1), beta_c = BETA + RB u2 (dpenv_set_current_randomisation)')
    ap.add_argument('--preset', default='thrust_loss', choices=('no_loss', 'thrust_loss', 'dynpos_fit', 'dynpos_fit_thrust_loss'),
                    help="nominal hull (dpenv_default_vessel_ex); default (round 6): the thrust-loss preset - the steady speeds 'with thrust losses' are the velocity "
                         'bounds the reference trains with (customEnv.py:17,26), and the shared training form runs it at the cost of the default hull')
    ap.add_argument('--eval', action='store_true', help='after training: run_RL_policy + the box test (IAE, energy) on the nominal hull and on spreads of hulls')
    ap.add_argument('--tune-baseline', type=int, default=0, metavar='K', help='with --eval: a scored sweep of K baseline gain sets x 16 current directions in one '
                    'flight (per-env controller table): the default baseline, the IAE / work front, the best set, and the best at no more than the actor\'s work')
    ap.add_argument('--tune-qp', type=int, default=0, metavar='K', help='with --eval: a scored sweep of K QP weight sets (w_power, w_dalpha, w_dforce) x 16 current '
                    'directions in one flight (per-env QP table): the default QP and its IAE / work front, to read beside --tune-baseline\'s')
    ap.add_argument('--tune-nn', type=int, default=0, metavar='K', help='with --eval: K neural allocators fitted with the wrench loss, one per w_power of '
                    'nn_w_power_grid(K) (0, then K - 1 values log-spaced from 0.01 to 1), flown as one population (one network per 64 envs) in one scored '
                    'box test: every network\'s IAE / work and their front, to read beside --tune-qp\'s; --nn-allocator ITERS sets the Adam steps per fit')
    ap.add_argument('--nn-allocator', type=int, default=0, metavar='ITERS', help='with --eval: fit the supervised neural allocator (9-80-80-80-6, '
                    'train.fit_nn_allocator: ITERS Adam steps on 16 384 rows of deploy.nn_allocator_dataset for the preset\'s hull) and fly it behind the '
                    'baseline\'s PID on every box test, beside the pseudo-inverse and the QP')
    ap.add_argument('--nn-loss', choices=('mse', 'wrench'), default='mse', help="with --nn-allocator: 'mse' regresses the network on the dataset's (u, alpha) "
                    "labels (FFNN.py); 'wrench' trains it through the force map with the allocation loss (train.allocation_grad: the QP's objective at "
                    'the network\'s output, no labels)')
    ap.add_argument('--nn-w-power', type=float, default=None, metavar='X', help="with --nn-loss wrench: the loss's w_power (default: the QP's, 1)")
    ap.add_argument('--nn-on-policy', type=int, default=0, metavar='ROUNDS', help='with --nn-allocator ITERS --nn-loss wrench: after the fit, ROUNDS rounds of '
                    'train.fit_nn_allocator_on_policy (fly the PID + network chain, read the PID\'s wrench on every row with the labelling scan, refit '
                    'ITERS steps on the dataset plus the flown wrenches); the score-card line of the network is printed before and after')
    ap.add_argument('--eval-envs', type=int, default=1024, help='envs per --eval box test; 1024 (the default) scores the resident rows as before, any other '
                                                                'value flies the test in 50-step launches scored on the device (evaluate.ScoreCard), e.g. 65536')
    ap.add_argument('--eval-presets', default='', help="comma-separated presets to run --eval on (default: the training preset), e.g. 'no_loss,thrust_loss': "
                                                      'how an actor trained on one thrust regime fares on the other')
    ap.add_argument('--save', default='', help='write the trained parameters (reference variable names) to this .npz')
    ap.add_argument('--backend', default='nccl', help="'nccl' (RCCL, one GPU per rank) or 'gloo' (rehearsal)")
    ap.add_argument('--same-device', action='store_true', help='all ranks on cuda:0 (multi-rank rehearsal on a one-GPU box)')
    args = ap.parse_args()
    if args.warm_start > 0 and args.update != 'fused':
        ap.error('--warm-start needs --update fused (the imitation gradient is a kernel of the fused update)')
    if args.dagger > 0 and args.update != 'fused':
        ap.error('--dagger needs --update fused (the imitation gradient is a kernel of the fused update)')
    if args.expert_state == 'flown' and args.expert != 'qp':
        ap.error('--expert-state flown goes with --expert qp (the pseudo-inverse has no thruster state)')
    if args.expert == 'qp' and args.randomise > 0 and args.warm_start > 0:
        ap.error('--expert qp with --randomise cannot fly the warm-start demonstration: the QP closed loop runs on a shared hull, not on per-env '
                 'hulls.  Use --dagger without --warm-start: the labelling scan touches no hull')
    if args.expert == 'nn' and (args.warm_start > 0 or args.nn_allocator <= 0):
        ap.error("--expert nn labels --dagger rounds with the fitted network: it needs --nn-allocator ITERS, and --warm-start flies 'pinv' or 'qp'")
    if args.nn_on_policy > 0 and (args.nn_allocator <= 0 or args.nn_loss != 'wrench'):
        ap.error('--nn-on-policy goes with --nn-allocator ITERS --nn-loss wrench (the wrench loss needs no labels, only wrenches)')
    # one process per GPU under torch.distributed.run (backend nccl = RCCL); envs shard by global id, gradients average
    rank, world, local = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1)), int(os.environ.get('LOCAL_RANK', 0))
    dev = torch.device('cuda', 0 if args.same_device else local)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if args.backend == 'nccl':
            torch.distributed.init_process_group('nccl', device_id=dev)
        else:
            torch.distributed.init_process_group(args.backend)
    torch.manual_seed(args.seed + 1000 * rank)
    env = ml4ca_amd.BatchedRevoltEnv(args.envs, auto_reset=True, seed=args.seed, device=dev, env_id_base=rank * args.envs, current=bool(args.current),
                                     vessel_params=ml4ca_amd.default_vessel(args.preset) if args.preset != 'no_loss' else None)   # final / ext / cont_ang
    if args.randomise > 0:
        env.set_vessel_randomisation(args.randomise, nominal=ml4ca_amd.default_vessel(args.preset))
    if args.current:
        import math
        v_c, b_c = (float(x) for x in args.current.split(','))
        env.set_current(torch.full((args.envs,), v_c, device=dev), torch.full((args.envs,), math.radians(b_c), device=dev))
        if args.randomise_current:
            r_v, r_b = (float(x) for x in args.randomise_current.split(','))
            env.set_current_randomisation(r_v, math.radians(r_b))
    ac = ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=args.seed, device=dev, activation=args.activation)
    D.sync_params(ac.parameters())                                               # sync_all_params, ppo.py:255
    clip, target_kl, T, n = 0.2, 0.01, args.steps, args.envs
    upd = average = None
    if args.update == 'fused':
        from ml4ca_amd.train import PPOUpdater
        upd = PPOUpdater(ac, pi_lr=3e-4, v_lr=1e-3, clip=clip, target_kl=target_kl)      # ac's tensors are now views of its two flat vectors
        if world > 1 and args.exchange == 'gradients':
            average = D.average_flat                                             # gradient AND statistics (the KL of the gate) in one all-reduce
    else:
        for p in ac.parameters():
            p.requires_grad_(True)
    pi_params = ac.pi_W + ac.pi_b + [ac.log_std]
    v_params = ac.v_W + ac.v_b
    pi_opt = torch.optim.Adam(pi_params, lr=3e-4) if upd is None else None
    v_opt = torch.optim.Adam(v_params, lr=1e-3) if upd is None else None
    buf = rollout.RolloutBuffer(T, env, gamma=0.99, lam=0.97)
    if args.warm_start > 0:
        warm_start(upd, env, args, out=print if rank == 0 else (lambda *a: None))
        with torch.no_grad():
            ac.log_std.clamp_(-4.0, 1.0)
        if args.eval and rank == 0:
            print('eval of the cloned actor, before any PPO epoch')
            evaluate_actor(ac, dev, args.preset, 'f32', args.seed, eval_envs=args.eval_envs, only=('nominal hull',))
    if args.dagger > 0:
        dagger(upd, env, args, out=print if rank == 0 else (lambda *a: None))
        with torch.no_grad():
            ac.log_std.clamp_(-4.0, 1.0)
        if args.eval and rank == 0:
            print('eval of the actor after DAgger, before any PPO epoch')
            evaluate_actor(ac, dev, args.preset, 'f32', args.seed, eval_envs=args.eval_envs, only=('nominal hull',))
    ac.upload(env, precision=args.precision)          # device pointers: one packing kernel, no host copy
    env.reset()
    gather = world > 1 and args.exchange == 'rollout'
    ex = D.EpisodeExchange(buf.exchange_blocks(), n_chunks=args.chunks) if gather else None
    if gather:
        torch.manual_seed(args.seed)                  # identical minibatch draws on every rank: the updates stay identical without a broadcast
    if rank == 0:
        print('epoch  mean_reward/step(max 3.5)  terminated/1k-steps  pi_iters  KL      V-loss    rollout_ms  update_s')
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # exploration noise is drawn inside the kernel (core.py:85), keyed by seed / global env id / draw index: no [T, n, 7]
        # noise block, and the trajectories do not depend on how many ranks share the envs
        if gather:
            # on-policy and overlapped: a piece of the episode crosses xGMI while the next piece is being rolled out; the advantages
            # are scanned and normalised locally (24 bytes of statistics cross) and follow as 8 B per env-step
            for c in range(ex.C):
                blk = buf.collect(env, sample=True, rows=ex.rows(c), reset_at_end=args.reset_at_end)
                ex.post_steps(c)
            buf.finish()
            buf.get()
            ex.post_scan()
            ex.wait()
            obs, act, adv, ret, logp_old = (ex.flat(k) for k in ('obs', 'act', 'adv', 'ret', 'logp'))
            obs = obs.float()
        else:
            blk = buf.collect(env, sample=True, reset_at_end=args.reset_at_end)
            buf.finish()
            obs, act, adv, ret, logp_old = buf.get()
        torch.cuda.synchronize()
        t_roll = time.perf_counter() - t0
        obs, act = obs.reshape(-1, 9), act.reshape(-1, 7)
        adv, ret, logp_old = adv.reshape(-1), ret.reshape(-1), logp_old.reshape(-1)
        N = obs.shape[0]
        mb = min(args.minibatch, N)
        t1 = time.perf_counter()
        if upd is not None:
            pi_iters, kl, v_loss = upd.update(obs, act, adv, ret, logp_old, iters=80, minibatch=mb, average=average)
        else:
            pi_iters, kl, v_loss = torch_update(ac, pi_opt, v_opt, pi_params, v_params, obs, act, adv, ret, logp_old, mb, clip, target_kl, gather)
        with torch.no_grad():
            ac.log_std.clamp_(-4.0, 1.0)
        if gather:
            D.assert_params_in_step(ac.parameters())                            # replicated updates: no collective keeps them equal, so check
        ac.upload(env, precision=args.precision)
        torch.cuda.synchronize()
        t_upd = time.perf_counter() - t1
        done = blk['done']
        if rank == 0:
            print('%5d  %10.3f  %22.2f  %8d  %.4f  %8.1f  %9.1f  %8.2f' % (
                epoch, float(blk['rew'].mean()), 1000.0 * float((done & 1).float().mean()), pi_iters, kl,
                v_loss, t_roll * 1e3, t_upd))
    if rank == 0:
        print('env-steps collected: %d (%.1f M per epoch, %d rank(s))' % (args.epochs * T * n * world, T * n * world / 1e6, world))
        if args.randomise > 0:
            hp = env.get_vessel_params()[:4]
            print('hulls in force at the end: m11 %.1f .. %.1f (nominal %.1f), episodes per env so far %.1f' % (
                float(hp[0].min()), float(hp[0].max()), float(ml4ca_amd.default_vessel(args.preset)[0]), float(env.get_state()[1][1].float().mean())))
        for p in ac.parameters():
            p.requires_grad_(False)
        if args.save:
            import numpy as np
            np.savez(args.save, **{k.replace('/', '.'): v for k, v in ac.state_dict().items()})
        if args.eval:
            for pz in (args.eval_presets.split(',') if args.eval_presets else [args.preset]):
                print('eval on the %s preset (trained on %s%s)' % (pz, args.preset, ', hulls re-drawn +-%g %%' % (100 * args.randomise) if args.randomise > 0 else ''))
                nn_net = None
                if args.nn_allocator > 0:
                    nn_net, base, wrench = fit_allocator(args, dev, pz)
                    if args.nn_on_policy > 0:
                        nn_score_card(nn_net, dev, pz, args.seed, args.eval_envs, 'before the on-policy rounds')
                        nn_net = nn_on_policy(args, dev, pz, base, wrench)
                        nn_score_card(nn_net, dev, pz, args.seed, args.eval_envs, 'after %d on-policy rounds' % args.nn_on_policy)
                evaluate_actor(ac, dev, pz, 'f32', args.seed, eval_envs=args.eval_envs, nn_net=nn_net)
                if args.tune_baseline > 0:
                    tune_baseline(ac, dev, pz, 'f32', args.tune_baseline, seed=args.seed)
                if args.tune_qp > 0:
                    tune_qp(dev, pz, args.tune_qp, seed=args.seed)
                if args.tune_nn > 0:
                    tune_nn(args, dev, pz, args.tune_nn, seed=args.seed)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
