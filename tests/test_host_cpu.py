"""CPU tests of host logic: config 1 (pseudo-inverse allocation), reset samplers, sharding, and the
world_size-2 gloo rehearsal of the episode-boundary trajectory all-gather."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')


def test_config1_pseudoinverse_allocation():
    """BASELINE.json configs[0] as restated in SURVEY 8(d): B(alpha) K n|n| == tau to 1e-9 (float64)."""
    from ml4ca_amd import allocation as AL
    for alpha in ([0.0, 0.0, np.pi / 2], [0.3, -0.4, np.pi / 2]):
        for tau in ([10.0, 5.0, 3.0], [0.0, 0.0, 0.0], [20.0, -10.0, 15.0]):
            n, F = AL.pinv_allocate(tau, alpha)
            back = AL.effectiveness(alpha) @ AL.percent_to_force(n)
            assert np.allclose(back, tau, rtol=0, atol=1e-9)
            assert np.allclose(AL.percent_to_force(n), F, rtol=0, atol=1e-12)
    # the effectiveness matrix is the reference's (SupervisedTau.B fixture, reference order port, star, bow)
    d = np.load(os.path.join(G, 'forcemap.npz'))
    for i in range(0, len(d['alpha']), 17):
        assert np.allclose(AL.effectiveness(d['alpha'][i]), d['B'][i], rtol=0, atol=1e-14)
    assert np.allclose(AL.LX, d['lx']) and np.allclose(AL.LY, d['ly'])
    # and the env-order force map of the oracle agrees with it
    from oracle import oracle as O
    orc = O.Oracle(O.make_config())
    n, F = AL.pinv_allocate([10.0, 5.0, 3.0], [0.3, -0.4, np.pi / 2])
    tau = orc.thrust_map(n[AL.ROS_TO_ENV], np.array([0.3, -0.4, np.pi / 2])[AL.ROS_TO_ENV])
    assert np.allclose(tau, [10.0, 5.0, 3.0], atol=1e-9)
    # saturation clips forces at the simulator's limits (qp_allocator.py:52)
    n, F = AL.pinv_allocate([500.0, 0.0, 0.0], [0.0, 0.0, np.pi / 2], saturate=True)
    assert np.all(np.abs(F) <= AL.F_MAX + 1e-12) and np.all(np.abs(n) <= 100.0 + 1e-9)


def test_host_reset_samplers_match_reference_fixture():
    from ml4ca_amd import reset_samplers as simtools
    d = np.load(os.path.join(G, 'env_final_cont.npz'))
    got = np.array([simtools.get_fixed_pose_on_radius(n) for n in range(6)])
    assert np.allclose(got, d['fixed_pose_on_radius'], rtol=0, atol=1e-15)
    assert simtools.get_fixed_pose_on_radius(7) == simtools.get_fixed_pose_on_radius(1)   # wraps like the reference
    np.random.seed(3)
    rr = np.array([simtools.get_random_pose_on_radius() for _ in range(500)])
    assert np.allclose(np.hypot(rr[:, 0], rr[:, 1]), 5.0) and np.abs(rr[:, 2]).max() <= 5 * np.pi / 180
    b = d['real_ss_bounds']
    tr = np.array([list(simtools.get_pose_on_state_space(b[0:3], 0.8)) + list(simtools.get_vel_on_state_space(b[3:], 0.24))
                   for _ in range(3000)])
    lim = np.array([0.8, 0.8, 0.8, 0.24, 0.24, 0.24]) * b
    assert (np.abs(tr) <= lim).all() and np.allclose(tr.std(0), lim / np.sqrt(3), rtol=0.06)


def test_shard_covers_all_envs_once():
    from ml4ca_amd import dist as D
    for total, world in [(262144, 8), (65536, 1), (1000, 3), (7, 7)]:
        spans = [D.shard(total, r, world) for r in range(world)]
        assert sum(n for n, _ in spans) == total
        pos = 0
        for n, base in spans:
            assert base == pos
            pos += n
    assert D.shard(262144, 5, 8) == (32768, 5 * 32768)       # config 4: 8 x 32768
    with pytest.raises(ValueError):
        D.shard(4, 4, 4)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, total, T, q):
    """One rank: step its env shard with the CPU oracle (standing in for the GPU kernel, which cannot run
    here), pack the [T, n_local, 19] block, all-gather over gloo, reassemble in global env order."""
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch
    import torch.distributed as dist
    from ml4ca_amd import dist as D
    from oracle import oracle as O
    dist.init_process_group('gloo', rank=rank, world_size=world)
    n_local, base = D.shard(total, rank, world)
    orc = O.Oracle(O.make_config(max_ep_len=6, auto_reset=1, seed=99, env_id_base=base), np.float32)
    st, ctr = orc.new_state(n_local)
    obs = orc.reset(st, ctr)
    block = np.zeros((T, n_local, 19), np.float32)
    for t in range(T):
        rng = np.random.RandomState(1000 + t)                 # actions are a function of (t, global env id)
        act = rng.normal(0, 0.7, size=(total, 7)).astype(np.float32)[base:base + n_local]
        block[t, :, 0:9] = obs
        block[t, :, 9:16] = act
        obs, rew, done = orc.step(st, ctr, act)
        block[t, :, 16] = rew
        block[t, :, 17] = done
    g = D.gather_trajectories(torch.from_numpy(block))
    full = D.to_global_env_order(g).numpy()
    g2, work = D.gather_trajectories(torch.from_numpy(block), async_op=True)     # overlappable form
    work.wait()
    assert torch.equal(g, g2)
    # the same rollout as the five blocks the kernels write, gathered in place (no packed [T, n, 19] staging copy)
    blocks = {'obs': torch.from_numpy(block[..., 0:9].copy()), 'act': torch.from_numpy(block[..., 9:16].copy()),
              'rew': torch.from_numpy(block[..., 16].copy()), 'val': torch.from_numpy(block[..., 17].copy()),
              'logp': torch.from_numpy(block[..., 18].copy())}
    gr = D.gather_rollout(blocks)
    gr2, works = D.gather_rollout(blocks, async_op=True)
    for w_ in works:
        w_.wait()
    for k_, lo, hi in (('obs', 0, 9), ('act', 9, 16)):
        assert torch.equal(D.to_global_env_order(gr[k_]), torch.from_numpy(full[..., lo:hi])) and torch.equal(gr[k_], gr2[k_])
    assert torch.equal(D.to_global_env_order(gr['rew']), torch.from_numpy(full[..., 16]))
    # the compact, pipelined exchange (dist.EpisodeExchange): obs as bf16 rows | act | logp posted chunk by chunk (async), adv | ret
    # after the scan; chunk-major output = the one-piece gather of the same blocks, bit for bit
    xb = {'obs': blocks['obs'].to(torch.bfloat16), 'act': blocks['act'], 'logp': blocks['logp'], 'adv': blocks['rew'].clone(), 'ret': blocks['val'].clone()}
    whole = D.gather_rollout(xb)
    for C in (1, 3, 4):
        ex = D.EpisodeExchange(xb, n_chunks=C)
        for c in range(C):
            ex.post_steps(c)
        ex.post_scan()
        got = ex.wait()
        for k_ in xb:
            assert got[k_].shape[:3] == (C, world, T // C)
            assert torch.equal(ex.episode_order(k_), whole[k_]), (C, k_)
            assert ex.flat(k_).shape[0] == world * T * n_local
    assert D.EpisodeExchange.bytes_per_env_step(xb) == 9 * 2 + 7 * 4 + 4 + 4 + 4
    # scalar statistics the way mpi_statistics_scalar does them: two all-reduces
    acc = torch.tensor([block[..., 16].sum(dtype=np.float64), block[..., 16].size], dtype=torch.float64)
    dist.all_reduce(acc)
    # ... and the one-pass form of the advantage normalisation: (sum, sum of squares) in double + the count, ONE all-reduce
    # (rollout.combine_stats is what RolloutBuffer.get calls between the GAE kernel and the apply kernel)
    from ml4ca_amd import rollout as RO
    x = block[..., 16].astype(np.float64)
    local = torch.tensor([x.sum(), (x * x).sum()], dtype=torch.float64)
    gstats, gcount = RO.combine_stats(local, x.size)
    one_pass = [float(gstats[0]), float(gstats[1]), float(gcount), float(local[0]), float(local[1])]
    # data-parallel optimiser plumbing (mpi_tf.py:16-62): parameter broadcast, gradient averaging, mpi_avg
    torch.manual_seed(100 + rank)
    params = [torch.randn(9, 80, requires_grad=True), torch.randn(80, requires_grad=True), torch.randn(7, requires_grad=True)]
    D.sync_params(params, root=0)
    psum = float(sum(p.detach().sum() for p in params))
    for p in params:
        p.grad = torch.full_like(p, float(rank + 1))
    D.average_gradients(params)
    gmean = float(params[0].grad[0, 0])
    kl = float(D.mean_across_ranks(torch.tensor(0.01 * (rank + 1))))
    chk = torch.tensor([psum, gmean, kl], dtype=torch.float64)
    lst = [torch.zeros(3, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(lst, chk)
    if rank == 0:
        q.put((full, float(acc[0] / acc[1]), [x.tolist() for x in lst], one_pass))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_gather_matches_single_process_run():
    import torch.multiprocessing as mp
    from oracle import oracle as O
    total, T, world = 64, 12, 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, total, T, q)) for r in range(world)]
    for p in procs:
        p.start()
    full, mean_rew, dp, one_pass = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # single-process run of all 64 envs
    orc = O.Oracle(O.make_config(max_ep_len=6, auto_reset=1, seed=99, env_id_base=0), np.float32)
    st, ctr = orc.new_state(total)
    obs = orc.reset(st, ctr)
    ref = np.zeros((T, total, 19), np.float32)
    for t in range(T):
        act = np.random.RandomState(1000 + t).normal(0, 0.7, size=(total, 7)).astype(np.float32)
        ref[t, :, 0:9] = obs
        ref[t, :, 9:16] = act
        obs, rew, done = orc.step(st, ctr, act)
        ref[t, :, 16] = rew
        ref[t, :, 17] = done
    assert full.shape == ref.shape
    assert np.array_equal(full, ref), 'sharded + gathered rollout must equal the single-process rollout bit for bit'
    assert (ref[..., 17] != 0).sum() >= total        # episodes ended and were re-sampled (Philox keyed by global id)
    assert abs(mean_rew - ref[..., 16].mean(dtype=np.float64)) < 1e-9
    # one-pass normalisation statistics over two ranks = the two per-shard double sums added, bit for bit (a two-term sum does
    # not depend on the order), and they give the mean / population std of mpi_statistics_scalar (mpi_tools.py:71-92)
    xa, xb = ref[:, : total // 2, 16].astype(np.float64), ref[:, total // 2:, 16].astype(np.float64)
    assert one_pass[3] == xa.sum() and one_pass[4] == (xa * xa).sum()
    assert one_pass[0] == xa.sum() + xb.sum() and one_pass[1] == (xa * xa).sum() + (xb * xb).sum() and one_pass[2] == ref[..., 16].size
    mean = one_pass[0] / one_pass[2]
    std = np.sqrt(one_pass[1] / one_pass[2] - mean * mean)
    xall = ref[..., 16].astype(np.float64)
    assert abs(mean - xall.mean()) < 1e-14 and abs(std - np.sqrt(((xall - xall.mean()) ** 2).mean())) < 1e-12
    # after sync_params both ranks hold rank 0's parameters; averaged gradients = (1 + 2) / 2; mpi_avg of (0.01, 0.02)
    assert dp[0][0] == dp[1][0] and dp[0][1] == dp[1][1] == 1.5 and abs(dp[0][2] - 0.015) < 1e-9 and abs(dp[1][2] - 0.015) < 1e-9


def _params_in_step_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from ml4ca_amd import dist as D
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    g = torch.Generator().manual_seed(4)
    params = [torch.randn((9, 80), generator=g), torch.randn(80, generator=g), torch.full((7,), -0.5)]
    res = []
    D.assert_params_in_step(params)                                   # equal on both ranks: passes
    res.append('equal ok')
    params[0][3, 5] += (1e-7 if rank == 1 else 0.0)                   # one ulp-sized difference on ONE rank
    try:
        D.assert_params_in_step(params)
        res.append('missed')
    except RuntimeError as e:
        res.append('raised: ' + str(e)[:60])
    a, b = params[1][2].clone(), params[1][7].clone()                 # a swap of two unequal entries keeps the plain sum: the weights catch it
    if rank == 1:
        params[0][3, 5] -= 1e-7
        params[1][2], params[1][7] = b, a
    else:
        params[0][3, 5] += 0.0
    try:
        D.assert_params_in_step(params)
        res.append('missed swap')
    except RuntimeError:
        res.append('raised swap')
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_replicated_update_divergence_is_detected():
    """examples/train_ppo.py --exchange rollout keeps the ranks' policies equal by computing the same update everywhere;
    dist.assert_params_in_step is the per-epoch check that they still are (raises on EVERY rank, so nobody is left in a collective)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_params_in_step_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        assert got[r][0] == 'equal ok' and got[r][1].startswith('raised: parameters differ between ranks') and got[r][2] == 'raised swap', got


def test_current_drift_is_a_stationary_gauss_markov_process():
    """Config 5's slowly varying current (build-defined): mean reversion to the set value, stationary std sigma,
    correlation time tau - checked on the oracle (the GPU kernel is checked against the oracle in -m gpu)."""
    from oracle import oracle as O
    n, T = 4096, 600
    tau, sv, sb = 20.0, 0.03, 0.1
    orc = O.Oracle(O.make_config(terminate=0, current_enabled=1, current_drift=1, current_tau=tau, current_sigma_v=sv,
                                 current_sigma_beta=sb, seed=12), np.float32)
    st, ctr = orc.new_state(n)
    orc.reset(st, ctr, init=np.zeros((6, n), np.float32))
    mean = np.stack([np.full(n, 0.2, np.float32), np.full(n, np.deg2rad(135), np.float32)])
    cur = mean.copy()
    dctr = np.zeros(n, np.uint32)
    act = np.zeros((n, 7), np.float32)
    hist = []
    for t in range(T):
        orc.step(st, ctr, act, current=cur, current_mean=mean, drift_ctr=dctr)
        hist.append(cur.copy())
    hist = np.array(hist)                      # [T, 2, n]
    assert (dctr == T).all()
    tail = hist[300:]
    assert abs(tail[:, 0].mean() - 0.2) < 2e-3 and abs(tail[:, 1].mean() - np.deg2rad(135)) < 5e-3
    assert abs(tail[:, 0].std() - sv) < 0.1 * sv and abs(tail[:, 1].std() - sb) < 0.1 * sb
    # lag-k autocorrelation of an OU process sampled every dt: (1 - dt/tau)^k
    x = tail[:, 0] - 0.2
    k = 25
    rho = (x[:-k] * x[k:]).mean() / (x * x).mean()
    assert abs(rho - (1 - 0.2 / tau) ** k) < 0.05
    # different envs draw independent noise; the same (seed, env, draw) repeats exactly
    assert abs(np.corrcoef(hist[:, 0, 0], hist[:, 0, 1])[0, 1]) < 0.3
    cur2, dctr2 = mean.copy(), np.zeros(n, np.uint32)
    st2, ctr2 = orc.new_state(n)
    orc.reset(st2, ctr2, init=np.zeros((6, n), np.float32))
    orc.step(st2, ctr2, act, current=cur2, current_mean=mean, drift_ctr=dctr2)
    assert np.array_equal(cur2, hist[0])


def test_qp_allocator_restatement_matches_reference_fixture():
    """qp_allocator.py:108-320 (imported behind ROS stubs by tools/gen_golden.py qp): 30 wrenches through the SLSQP
    allocator - raw solution, success flag, published efforts / azimuths, carried state - incl. one infeasible jump
    after which the node keeps its previous state."""
    from ml4ca_amd.allocation import QPAllocator
    d = np.load(os.path.join(G, 'qp_allocator.npz'))
    qa = QPAllocator(simulation=bool(d['simulation_flag'][0]), retry=False)
    assert np.allclose(qa.max_force_rate, d['max_force_rate']) and np.allclose(qa.max_rotational_rate, d['max_rotational_rate'])
    n_fail = 0
    for k, tau in enumerate(d['tau']):
        x, ok = qa.solve(tau)
        assert ok == bool(d['success'][k]), k
        if ok:
            assert np.allclose(x, d['solution'][k], rtol=0, atol=2e-4), (k, x, d['solution'][k])
        n, ang, ok2 = qa.allocate(tau)
        assert np.allclose(n, d['published_effort'][k], rtol=0, atol=2e-2), (k, n, d['published_effort'][k])
        assert np.allclose(ang, d['published_angle_deg'][k], rtol=0, atol=2e-2)
        assert np.allclose(qa.previous_thruster_state, d['previous_state'][k], rtol=0, atol=2e-4)
        n_fail += (not ok)
    assert n_fail == 1
    # a successful allocation reproduces the wrench within its +-1 N slack (equality constraints :156-158)
    from ml4ca_amd import allocation as AL
    F = np.array(qa.previous_thruster_state[:3])
    a = np.array(qa.previous_thruster_state[3:])
    assert np.all(np.abs(AL.effectiveness(a) @ F - d['tau'][-1]) <= 1.0 + 1e-6)
    # with the retry loop the infeasible jump is followed as far as the rate limits allow
    qr = QPAllocator(retry=True)
    x, ok = qr.solve([60.0, -30.0, 40.0])
    assert ok and abs(x[0] - 5.0) < 1e-3 and np.abs(x[5:]).max() > 1.0


def test_default_hull_soft_pins_and_free_drift_record():
    """The BUILD-OWNED default hull (calibrated by tests/calibration/calibrate_plant.py; no parity claim) against what the reference
    records about its plant: steady full-thrust speeds (customEnv.py:13-14: +2.20 m/s, 0.60 rad/s) and the free-drift
    run in a 0.2 m/s / 135 deg current (results/all_plots/stationKeep135, fixture cybersea_free_drift.npz), incl. the
    swing towards broadside that the Munk moment produces."""
    from oracle import oracle as O
    orc = O.Oracle(O.make_config(terminate=0, current_enabled=1), np.float64)
    e, v = np.zeros(3), np.zeros(3)
    for _ in range(600):
        e, v = orc.plant(e, v, [0, 100, 100], [np.pi / 2, 0, 0])
    assert abs(v[0] - 2.20) < 0.05 and abs(v[1]) < 1e-9 and abs(v[2]) < 1e-9
    e, v = np.zeros(3), np.zeros(3)
    for _ in range(600):
        e, v = orc.plant(e, v, [100, 100, 100], [np.pi / 2, -np.pi / 2, -np.pi / 2])
    assert abs(v[2] - 0.60) < 0.03
    d = np.load(os.path.join(G, 'cybersea_free_drift.npz'))
    st, ctr = orc.new_state(1)
    orc.reset(st, ctr, init=np.zeros((6, 1)))
    cur = d['current'].reshape(2, 1).astype(np.float64)
    a = np.zeros((1, 7))
    a[0, 4] = a[0, 6] = 1.0
    traj = []
    for _ in range(len(d['t']) - 1):
        orc.step(st, ctr, a, current=cur)
        traj.append(st[0:3, 0].copy())
    err = np.array(traj) - d['pose'][1:]
    assert np.sqrt((err[:, :2] ** 2).sum(1).mean()) < 0.6          # measured 0.36 m over 60 s
    assert np.degrees(np.sqrt((err[:, 2] ** 2).mean())) < 12.0       # measured 8.1 deg
    assert np.degrees(np.array(traj)[:, 2].max()) > 30.0             # the hull does swing towards broadside (record: 49 deg)


def test_default_hull_open_loop_against_recorded_cybersea_commands():
    """Soft validation of the BUILD-OWNED plant (no parity claim): seven recorded Cybersea runs with the thruster commands
    that produced them (tests/golden/cybersea_replay.npz from results/all_plots/{box_test,large_setpoints,
    current_box_test}, tools/gen_golden.py replay).  392 windows of 10 s start from the recorded pose and are driven
    OPEN LOOP by the recorded commands: the prediction must beat the no-model predictors (stay put, constant velocity)
    at every horizon and stay inside the error band measured when the default hull was fixed."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'calibration'))
    import replay_cybersea as RC
    W = RC.load_windows()
    assert W['eta0'].shape[0] == 392 and len(W['names']) == 7
    pred = RC.replay_oracle(W)
    assert np.isfinite(pred).all()
    e = RC.errors(pred, W)
    cv = RC.errors(RC.constant_velocity(W), W)
    still = RC.errors(np.repeat(W['eta0'][None], W['truth'].shape[0], 0), W)
    band = {10: (0.07, 2.2), 25: (0.26, 7.5), 50: (0.65, 17.0)}        # measured 0.05/1.7, 0.21/6.6, 0.57/15.4
    for h in RC.HORIZONS:
        assert e[h][0] < band[h][0] and e[h][1] < band[h][1], (h, e[h])
        assert e[h][0] < 0.7 * cv[h][0] and e[h][1] < 0.7 * cv[h][1], (h, e[h], cv[h])
        assert e[h][0] < 0.35 * still[h][0] and e[h][1] < 0.8 * still[h][1], (h, e[h], still[h])
    # an independent NumPy statement of the model equations reproduces the C oracle's plant over all 392 x 50 steps
    assert np.abs(RC.replay_numpy(W) - pred).max() < 1e-9
    # the current run is predicted as well as the calm-water one: the relative-velocity current model is in the right place
    sel = W['run'] == W['names'].index('current_box_test_QP')
    assert RC.errors(pred, W, sel)[50][0] < 0.5


def test_bench_starts_its_own_ranks_when_no_launcher_is_around():
    """bench.py --gpus 2 without torch.distributed.run around it: the ranks are started as a CHILD process before anything touches a
    GPU (never os.exec), rank 0's single JSON line comes through, the exit code is the child's.  --rendezvous-only keeps it on the
    CPU (gloo): what is tested is the launch path the driver's N > 1 runs depend on."""
    import json
    import subprocess
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None); env.pop('RANK', None); env.pop('LOCAL_RANK', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--rendezvous-only'], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r['n_gpus'] == 2 and r['sum_of_rank_plus_1'] == 3.0
    assert r['group']['world_size'] == 2 and r['group']['backend'] == 'gloo' and len(r['group']['ranks']) == 2
    assert sorted(x['rank'] for x in r['group']['ranks']) == [0, 1] and len({x['pid'] for x in r['group']['ranks']}) == 2
    assert 'starting 2 ranks as a child process' in p.stderr
    # under a launcher with the wrong rank count it refuses instead of measuring something else
    env2 = dict(env, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    q = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--rendezvous-only'], env=env2, capture_output=True,
                       text=True, timeout=600)
    assert q.returncode != 0 and 'started 1 rank' in (q.stderr + q.stdout)


def test_bench_under_the_drivers_launcher_has_the_same_environment():
    """The driver's form for N > 1 (bench.py docstring): `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 2 ...` - WORLD_SIZE is set, so self_launch is skipped.  The ranks must give themselves the
    pool's environment (HSA_ENABLE_IPC_MODE_LEGACY=0: dmabuf IPC for RCCL) before torch initialises anything, exactly as the self-launched
    ranks get it, and the JSON line records it.  The variable is removed from the launcher's environment first: the
    driver's shell may not have it."""
    import json
    import socket
    import subprocess
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'HSA_ENABLE_IPC_MODE_LEGACY', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    sock = socket.socket(); sock.bind(('127.0.0.1', 0)); port = sock.getsockname()[1]; sock.close()
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--rendezvous-only'],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert 'starting 2 ranks as a child process' not in p.stderr                      # the launcher's ranks, not bench.py's own
    g = r['group']
    assert g['world_size'] == 2 and g['launcher'] == 'torch.distributed.run' and len(g['ranks']) == 2
    assert g['environment']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0' and g['environment']['MASTER_ADDR'] == '127.0.0.1'
    assert all(x['environment']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0' for x in g['ranks'])    # every rank's own os.environ
    assert g['init_timeout_s'] == 180.0
    # an operator's explicit choice wins over the default
    p2 = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--rendezvous-only'],
                        env=dict(env, HSA_ENABLE_IPC_MODE_LEGACY='1'), capture_output=True, text=True, timeout=600)
    assert p2.returncode == 0, p2.stderr[-2000:]
    r2 = json.loads([l for l in p2.stdout.splitlines() if l.startswith('{')][0])
    assert all(x['environment']['HSA_ENABLE_IPC_MODE_LEGACY'] == '1' for x in r2['group']['ranks'])


def test_bench_rank_that_cannot_reach_its_peers_exits_nonzero_with_one_line():
    """A rank whose peers never arrive must not hang until the driver's kill: init_process_group has a timeout, the failure is one
    line naming rank, device and error, and the exit code is non-zero.  One rank of a pretended 2-rank job, nobody else, 3 s."""
    import socket
    import subprocess
    import time as _t
    sock = socket.socket(); sock.bind(('127.0.0.1', 0)); port = sock.getsockname()[1]; sock.close()
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    t0 = _t.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--rendezvous-only', '--init-timeout', '3'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 5, (p.returncode, p.stderr[-1500:])
    msg = [l for l in p.stderr.splitlines() if l.startswith('bench.py: rank 0 of 2')]
    assert len(msg) == 1 and 'could not join the process group within 3 s' in msg[0], p.stderr[-1500:]
    assert p.stdout.strip() == ''
    assert _t.time() - t0 < 120


def test_bench_refuses_more_ranks_than_devices():
    """fewer devices than --gpus: non-zero exit with a message, nothing measured, no rank started"""
    import subprocess
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('this host has the devices')
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 3 and 'only' in p.stderr and 'device(s) visible' in p.stderr and p.stdout.strip() == ''


def test_episode_exchange_single_process_is_a_copy():
    """dist.EpisodeExchange without a process group (one rank): the 'gather' degenerates to copies into the chunk-major output; the views
    flat() / episode_order() address the same samples as the blocks themselves."""
    import torch
    from ml4ca_amd import dist as D
    T, n = 12, 5
    g = torch.Generator().manual_seed(0)
    blocks = {'obs': torch.randn((T, n, 9), generator=g).to(torch.bfloat16), 'act': torch.randn((T, n, 7), generator=g),
              'logp': torch.randn((T, n), generator=g), 'adv': torch.randn((T, n), generator=g), 'ret': torch.randn((T, n), generator=g)}
    for C in (1, 3, 4, 12):
        ex = D.EpisodeExchange(blocks, n_chunks=C)
        assert [ex.rows(c) for c in range(C)] == [(c * T // C, (c + 1) * T // C) for c in range(C)]
        for c in range(C):
            ex.post_steps(c)
        ex.post_scan()
        out = ex.wait()
        for k, b in blocks.items():
            assert out[k].shape[:3] == (C, 1, T // C)
            assert torch.equal(ex.episode_order(k)[0], b)
            assert torch.equal(ex.flat(k), b.reshape((T * n,) + tuple(b.shape[2:])))
    with pytest.raises(ValueError):
        D.EpisodeExchange(blocks, n_chunks=5)


def test_thrust_loss_preset_against_the_second_set_of_recorded_speeds():
    """dpenv_default_vessel_ex(DPENV_VESSEL_THRUST_LOSS): the calibrated hull with stern thrusters that give BOTH sets of steady speeds the
    reference records - without thrust losses -1.60 m/s astern (customEnv.py:14, through their reverse gain), with thrust losses +1.4 / -1.1 m/s
    (customEnv.py:17; the velocity bounds it trains with, customEnv.py:26; through an inflow loss F = K n|n| - Kl |n| u_a) - derived by
    tests/calibration/fit_thrust_loss_preset.py.  BUILD-OWNED like the plant itself: soft pins, no parity claim.  Yaw under losses is an
    outcome: 0.505 rad/s against the recorded 0.52 (a constant gain reduced to meet +1.4 m/s gave 0.35)."""
    from ml4ca_amd import _lib
    from oracle import oracle as O
    from tests.calibration import fit_thrust_loss_preset as F
    base, loss = _lib.default_vessel('no_loss').astype(np.float64), _lib.default_vessel('thrust_loss').astype(np.float64)
    assert np.array_equal(_lib.default_vessel(), _lib.default_vessel('no_loss'))
    P = _lib.P
    changed = np.nonzero(base != loss)[0]
    assert list(changed) == [P['KR_PORT'], P['KR_STAR'], P['KLF_PORT'], P['KLF_STAR'], P['KLR_PORT'], P['KLR_STAR']]    # stern thrusters only: same hull, same bow
    # the oracle holds the same vector (what its parity runs of the preset use)
    ov = np.zeros(O.NPARAM, np.float32)
    O.lib().dpo_thrust_loss_vessel_f32(ov.ctypes.data_as(O.C.POINTER(O.C.c_float)))
    assert np.array_equal(ov, _lib.default_vessel('thrust_loss'))
    m0, m1, m2 = F.manoeuvres(base), F.manoeuvres(F.no_loss_of(loss)), F.manoeuvres(loss)
    assert abs(m0['surge_ahead'] - 2.20) < 0.02 and abs(m0['yaw'] - 0.60) < 0.02 and abs(m0['sway'] - 0.35) < 0.07
    assert abs(m1['surge_ahead'] - 2.20) < 0.02 and abs(m1['surge_astern'] + 1.60) < 0.01                       # loss off: the first set, now astern too
    assert abs(m2['surge_ahead'] - 1.40) < 0.01 and abs(m2['surge_astern'] + 1.10) < 0.01
    assert abs(m2['sway'] - 0.30) < 0.02 and abs(m2['sway_to_port'] + 0.30) < 0.02
    assert abs(m2['yaw'] - 0.52) < 0.03
    # a fit from the default reproduces the shipped numbers
    fit = F.fit(base)
    assert np.allclose(fit[[16, 17, 27, 28, 30, 31]], loss[[16, 17, 27, 28, 30, 31]], rtol=2e-3)
    # the free drift (no thrust) is the same trajectory under both presets
    d = np.load(os.path.join(G, 'cybersea_free_drift.npz'))
    traj = []
    for vec in (base, loss):
        orc = O.Oracle(O.make_config(terminate=0, current_enabled=1), np.float64, vessel=vec)
        st, ctr = orc.new_state(1)
        orc.reset(st, ctr, init=np.zeros((6, 1)))
        a = np.zeros((1, 7))
        a[0, 4] = a[0, 6] = 1.0
        for _ in range(100):
            orc.step(st, ctr, a, current=d['current'].reshape(2, 1).astype(np.float64))
        traj.append(st[0:6, 0].copy())
    assert np.array_equal(traj[0], traj[1])


def test_dynpos_fit_preset_against_every_recorded_pin():
    """dpenv_default_vessel_ex(DPENV_VESSEL_DYNPOS_FIT) (round 6; BUILD-OWNED like the plant: soft pins, no parity claim): the sway-yaw part of the hull
    refitted jointly to the default's records, the reference's 32 recorded Cybersea station-keeping runs (results/all_plots/dyn_pos/) and the
    recorded steady sway speed (customEnv.py:14: 0.35 m/s, which the default hull misses at 0.29) - tests/calibration/fit_dynpos_preset.py.
    It is a FLAG: combined with the thrust-loss preset the stern thrusters' numbers are the same (a surge fit; the surge terms did not move)."""
    from ml4ca_amd import _lib
    from oracle import oracle as O
    from tests.calibration import fit_dynpos_preset as FD
    from tests.calibration import fit_thrust_loss_preset as F
    base, fitp = _lib.default_vessel('no_loss').astype(np.float64), _lib.default_vessel('dynpos_fit').astype(np.float64)
    P = _lib.P
    changed = sorted(int(i) for i in np.nonzero(base != fitp)[0])
    assert changed == sorted(P[k] for k in ('M22', 'YV', 'YVV', 'YR', 'NV', 'NR', 'NRR', 'YUR'))      # sway-yaw hull terms only: surge, thrusters, geometry stay
    assert np.array_equal(FD.shipped().astype(np.float32), _lib.default_vessel('dynpos_fit'))          # the oracle holds the same vector
    both, loss = _lib.default_vessel('dynpos_fit_thrust_loss'), _lib.default_vessel('thrust_loss')
    assert np.array_equal(both[[16, 17, 27, 28, 30, 31]], loss[[16, 17, 27, 28, 30, 31]]) and np.array_equal(both[:12], fitp[:12].astype(np.float32))
    cal, sk, W = FD._cal(), FD.StationKeeping(), FD.RC.load_windows()
    r0, r1 = FD.rows(base, cal, sk, W), FD.rows(fitp, cal, sk, W)
    # (e) the sway pin, met; surge and yaw kept
    assert abs(r1['manoeuvres']['sway'] - 0.35) < 0.005 and abs(r0['manoeuvres']['sway'] - 0.29) < 0.01
    assert abs(r1['manoeuvres']['yaw'] - 0.60) < 0.01 and abs(r1['manoeuvres']['surge_ahead'] - 2.20) < 0.01
    # (d) station keeping: the yaw-moment residual nearly halved, the sway residual down
    assert r1['dynpos_rms'][2] < 0.62 * r0['dynpos_rms'][2] and r1['dynpos_rms'][1] < 0.9 * r0['dynpos_rms'][1] and abs(r1['dynpos_rms'][0] - r0['dynpos_rms'][0]) < 0.01
    # (a)-(c) and the replay: within 0.02 m / 0.3 deg of the default hull's rows (why it is a preset, not the default)
    assert r1['drift_pos'] < r0['drift_pos'] + 0.025 and r1['drift_yaw_deg'] < r0['drift_yaw_deg'] + 0.3
    assert r1['box_N'] < r0['box_N'] + 0.02 and r1['box_E'] < r0['box_E'] + 0.02 and r1['box_yaw_deg'] < r0['box_yaw_deg'] + 0.1
    assert r1['replay_10s'][0] < r0['replay_10s'][0] + 0.02 and r1['replay_10s'][1] < r0['replay_10s'][1] + 0.3
    # with the thrust loss on top: the surge pins of the second set as before, yaw under losses still near the recorded 0.52
    m = F.manoeuvres(both.astype(np.float64))
    assert abs(m['surge_ahead'] - 1.40) < 0.01 and abs(m['surge_astern'] + 1.10) < 0.01 and abs(m['yaw'] - 0.52) < 0.035


def test_bench_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    """bench.dump_outputs past DUMP_LIMIT: every array keeps the same seeded sample of env rows, the indices go to env_index.npy
    (float64, exact), the files of all ranks together stay under the limit; under it the arrays are written whole, without an index."""
    import torch
    import bench
    n = 20000
    g = torch.Generator().manual_seed(0)
    arrays = {'obs': torch.randn((n, 9), generator=g), 'reward': torch.randn(n, generator=g),
              'done': torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8)}
    bench.dump_outputs(str(tmp_path / 'whole'), arrays, 0, 1)
    assert sorted(os.listdir(str(tmp_path / 'whole'))) == ['done.npy', 'obs.npy', 'reward.npy']
    assert np.array_equal(np.load(str(tmp_path / 'whole' / 'obs.npy')), arrays['obs'].numpy())
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 1 << 20)
    world = 2
    for rank in range(world):
        bench.dump_outputs(str(tmp_path / 'sampled'), arrays, rank, world)
    d = tmp_path / 'sampled'
    files = sorted(os.listdir(str(d)))
    assert files == sorted('r%d_%s.npy' % (r, k) for r in range(world) for k in ('done', 'env_index', 'obs', 'reward'))
    assert sum(os.path.getsize(str(d / f)) for f in files) <= 1 << 20
    for rank in range(world):
        idx = np.load(str(d / ('r%d_env_index.npy' % rank)))
        assert idx.dtype == np.float64 and 0 < idx.size < n and np.all(np.diff(idx) > 0) and idx.max() < n
        ii = idx.astype(np.int64)
        for k, a in arrays.items():
            got = np.load(str(d / ('r%d_%s.npy' % (rank, k))))
            assert got.dtype == np.float32 and np.array_equal(got, a.float().numpy()[ii]), k
    assert np.array_equal(np.load(str(d / 'r0_env_index.npy')), np.load(str(d / 'r1_env_index.npy')))
