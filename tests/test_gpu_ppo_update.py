"""The fused PPO update on the GPU (ml4ca_amd/train.py, dpenv_train.hip) against torch float64 autograd, its own host statements and
the torch update of examples/train_ppo.py.

THE BOUND of every parity check here.  Error is measured per parameter tensor, relative to that tensor's largest reference value.
The yardstick is the same error for torch's own float32 autograd on the same fixture; the bound is 8 x that (a factor 4 that a
split-f16 product, 2^-22, would have against float32's 2^-24, times 2 for a different summation order; the exact-f32 matrix
instruction the kernels use should sit well inside it), and never lower than K x 2^-24 with K the roundings along the longest
accumulation chain of a gradient element, derived like the floors of tests/tolerances.py (one rounding = half an ulp of an
input-sized number, K of them along the chain):
    forward to the output     (16 + 1) + 3 x (80 + 1)   one fma per k of the padded input layer and of each 80-wide layer, + the activation
    output gradient           20                        quotient, square, 7-term sum, exp, the clip products, dlogp/dmu
    backward to dZ0           16 + 80 + 80              three transposed products
    the rows                  rows per workgroup        dW accumulates over the tiles of ONE workgroup: 64 ceil(tiles / grid)
    the partials              grid + 1                  summed in f64, one rounding each to float32 on the way in, the division
Statistics: |kernel - float64| <= max(8 x |torch-f32 - float64|, K x 2^-24 x S).  S is NOT the statistic's own value where the statistic is
a cancelled mean (tests/tolerances.py: the roundings are those of the terms, whatever is left of their sum): pi_loss is a mean of
ratio x A, S = 2 max|A| (ratio < 2 in the fixture); approx_kl a mean of differences of log-probabilities, S = max|logp_old|; mean_ratio
S = 2; v_loss, a mean of squares, is its own scale.  That is looser than "relative to its own value" wherever the mean nearly cancels.
clip_frac is a count and must match exactly."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from ml4ca_amd import _lib
from ml4ca_amd import train as TR
from tests import ppo_fixture as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
LEAKS = (0.2, 0.0)
N_ROWS = 300                                   # n_rows > every count
# 1 row; one row short of a tile, a tile, one more; 165 = three workgroups with a ragged last tile (TR.grid: 64 rows per workgroup
# below 256 workgroups); 257 = five
COUNTS = (1, 63, 64, 65, 165, 257)
RECORD = os.environ.get('PPO_PARITY_RECORD', '')       # a path: the measured yardstick and kernel errors are appended there


def torch_():
    import torch
    return torch


def chain_K(count):
    tiles = (count + 63) // 64
    g = TR.grid(count)
    return (16 + 1) + 3 * (80 + 1) + 20 + (16 + 80 + 80) + 64 * ((tiles + g - 1) // g) + g + 1


assert [TR.grid(c) for c in COUNTS] == [1, 1, 1, 2, 3, 5] and 165 % 64 != 0
# above 16 384 rows a workgroup takes several tiles: accumulators, column sums and statistics carried from tile to tile, the barrier at the
# top of the tile loop.  33 000 rows = 516 tiles on 256 workgroups: two tiles each, three for the first four, the last tile ragged
MANY_TILES = 33000
assert TR.grid(MANY_TILES) == 256 and (MANY_TILES + 63) // 64 == 516 and MANY_TILES % 64 != 0


_cache = {}


def fixture(leak):
    """The shared fixture and its device copies (built once per leak, never changed)."""
    if leak not in _cache:
        torch = torch_()
        fx = F.make_fixture(N_ROWS, leak)
        dev = {k: torch.tensor(fx[k], device=DEV) for k in ('pi_theta', 'v_theta', 'obs', 'act', 'adv', 'ret', 'logp_old')}
        _cache[leak] = (fx, dev, {})
    return _cache[leak]


def references(leak, rows):
    """float64 autograd and the float32 yardstick on the CPU for the rows `rows` (cached per row set)."""
    torch = torch_()
    fx, _, refs = fixture(leak)
    key = np.asarray(rows).tobytes()
    if key not in refs:
        refs[key] = (F.torch_grads(fx, rows=rows), F.torch_grads(fx, rows=rows, dtype=torch.float32))
    return refs[key]


def rel_errors(got, ref, actor):
    """Per tensor max |got - ref| / max |ref|; a tensor whose reference is all zero (count 1 on a clipped row) must be all zero."""
    out = {}
    for name, sl in F.tensor_slices(actor):
        scale = np.abs(ref[sl]).max()
        d = np.abs(np.asarray(got, np.float64)[sl] - ref[sl]).max()
        out[name] = (d / scale) if scale > 0 else (0.0 if d == 0 else float('inf'))
    return out


def stat_scales(fx, rows, actor):
    """The input-sized numbers behind each statistic (tests/tolerances.py: a cancelled mean carries the roundings of its terms): pi_loss is a
    mean of ratio x A with ratio < 2 in this fixture, approx_kl a mean of differences of log-probabilities, mean_ratio of ratios < 2;
    v_loss is a mean of squares and its own scale."""
    if not actor:
        return None
    return (2.0 * float(np.abs(fx['adv'][rows]).max()), float(np.abs(fx['logp_old'][rows]).max()), 1.0, 2.0)


def check_parity(what, got, ref64, ref32, actor, count, nstat, scales=None):
    """got [P + nstat] float32 from the device against (grad, stats) references."""
    P = ref64[0].size
    got = np.asarray(got, np.float64)
    floor = chain_K(count) * 2.0 ** -24
    kern, yard = rel_errors(got[:P], ref64[0], actor), rel_errors(ref32[0], ref64[0], actor)
    lines = []
    for name in kern:
        bound = max(8.0 * yard[name], floor)
        lines.append('%s %-7s kernel %.3e  torch-f32 %.3e  bound %.3e' % (what, name, kern[name], yard[name], bound))
        print(lines[-1])
    names = ('pi_loss', 'approx_kl', 'clip_frac', 'mean_ratio') if actor else ('v_loss',)
    for j, name in enumerate(names):
        scale = max(abs(ref64[1][j]), 1e-300)
        k, y = abs(got[P + j] - ref64[1][j]) / scale, abs(ref32[1][j] - ref64[1][j]) / scale
        lines.append('%s %-10s kernel %.3e  torch-f32 %.3e' % (what, name, k, y))
        print(lines[-1])
    if RECORD:
        with open(RECORD, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    for name in kern:
        assert kern[name] <= max(8.0 * yard[name], floor), (what, name, kern[name], yard[name], floor)
    for j, name in enumerate(names):
        if name == 'clip_frac':
            assert got[P + j] == float(np.float32(ref64[1][j])), (what, got[P + j], ref64[1][j])       # the same count of rows, exactly
            continue
        scale = scales[j] if scales is not None else abs(ref64[1][j])
        assert abs(got[P + j] - ref64[1][j]) <= max(8.0 * abs(ref32[1][j] - ref64[1][j]), floor * scale), (what, name, got[P + j], ref64[1][j], ref32[1][j])
    assert len(got) == P + nstat


def index_rows(mode, count, seed):
    rng = np.random.RandomState(seed)
    if mode == 'none':
        return None, np.arange(count)
    rows = rng.permutation(N_ROWS)[:count] if mode == 'perm' else rng.randint(0, max(N_ROWS // 3, 1), size=count)
    return rows.astype(np.int32), rows


def run_parity(leak, idx_np, rows, count, what):
    torch = torch_()
    fx, d, _ = fixture(leak)
    idx = None if idx_np is None else torch.tensor(np.asarray(idx_np, np.int32), device=DEV)
    ref64, ref32 = references(leak, rows)
    out = TR.ppo_actor_grad(d['pi_theta'], d['obs'], d['act'], d['adv'], d['logp_old'], F.CLIP, idx=idx, leak=leak, count=count)
    vout = TR.value_grad(d['v_theta'], d['obs'], d['ret'], idx=idx, leak=leak, count=count)
    check_parity(what + ' actor ', out.cpu().numpy(), (ref64[0], ref64[1]), (ref32[0], ref32[1]), True, count, 4, stat_scales(fx, rows, True))
    check_parity(what + ' critic', vout.cpu().numpy(), (ref64[2], ref64[3]), (ref32[2], ref32[3]), False, count, 1)
    return ref64


@pytest.mark.parametrize('mode', ('none', 'perm', 'repeats'))
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('leak', LEAKS)
def test_gradient_parity(leak, count, mode):
    fx, d, _ = fixture(leak)
    what = 'leak %.1f count %3d idx %-7s' % (leak, count, mode)
    if count == 1:
        # ONE row: a row the clip rule cuts has a zero actor gradient (zero must come out), a live row has one (a tile with one live row
        # must come out right).  Without an index the row is row 0, which the fixture keeps live; with an index both kinds are run.
        cut = F.cut_rows(fx)
        order = np.random.RandomState(7 + len(mode)).permutation(N_ROWS)
        live_row, cut_row = int(order[~cut[order]][0]), int(order[cut[order]][0])
        for row, is_cut in ((0, False),) if mode == 'none' else ((live_row, False), (cut_row, True)):
            assert bool(cut[row]) == is_cut
            rows = np.array([row])
            ref64 = run_parity(leak, None if mode == 'none' else rows, rows, 1, what + (' cut ' if is_cut else ' live'))
            if is_cut:
                assert not ref64[0].any()
            else:
                assert all(np.abs(ref64[0][sl]).max() > 0 for _, sl in F.tensor_slices(True))         # no tensor compares zero with zero
            assert all(np.abs(ref64[2][sl]).max() > 0 for _, sl in F.tensor_slices(False))
        return
    idx_np, rows = index_rows(mode, count, 100 * count + len(mode))
    if mode == 'repeats':
        assert len(set(rows.tolist())) < count
    if count == 65 and mode == 'none':
        assert not F.cut_rows(fx)[64]                           # the lone row of the second workgroup carries a gradient
    run_parity(leak, idx_np, rows, count, what)


@pytest.mark.parametrize('leak', LEAKS)
def test_gradient_parity_several_tiles_per_workgroup(leak):
    rows = np.random.RandomState(33).randint(0, N_ROWS, size=MANY_TILES)
    run_parity(leak, rows, rows, MANY_TILES, 'leak %.1f count %d idx repeats' % (leak, MANY_TILES))


@pytest.mark.parametrize('leak', LEAKS)
def test_determinism(leak):
    torch = torch_()
    fx, d, _ = fixture(leak)
    idx = torch.tensor(index_rows('repeats', 257, 5)[0], device=DEV)
    a = [TR.ppo_actor_grad(d['pi_theta'], d['obs'], d['act'], d['adv'], d['logp_old'], F.CLIP, idx=idx, leak=leak) for _ in range(2)]
    v = [TR.value_grad(d['v_theta'], d['obs'], d['ret'], idx=idx, leak=leak) for _ in range(2)]
    assert torch.equal(a[0], a[1]) and torch.equal(v[0], v[1])
    assert bool(torch.isfinite(a[0]).all()) and bool(a[0].abs().max() > 0)


@pytest.mark.parametrize('leak', LEAKS)
def test_workgroup_partition(leak):
    """The same 64 rows as ONE workgroup (count 64) and, each three times in a shuffled order, as THREE (count 192): the mean gradient is
    the same number, so both must sit within the parity bound of the float64 reference of the 64 rows, with whatever the partition, the
    per-workgroup partials and the reduction add.  (There is no test-only grid override; the cap of 256 workgroups, where one workgroup
    takes several tiles, is exercised by test_gradient_parity_several_tiles_per_workgroup.)"""
    torch = torch_()
    fx, d, _ = fixture(leak)
    rng = np.random.RandomState(9)
    rows = rng.permutation(N_ROWS)[:64]
    rows3 = rng.permutation(np.tile(rows, 3))
    assert TR.grid(64) == 1 and TR.grid(192) == 3
    ref64, ref32 = references(leak, rows)
    for r, count in ((rows, 64), (rows3, 192)):
        idx = torch.tensor(r.astype(np.int32), device=DEV)
        out = TR.ppo_actor_grad(d['pi_theta'], d['obs'], d['act'], d['adv'], d['logp_old'], F.CLIP, idx=idx, leak=leak)
        vout = TR.value_grad(d['v_theta'], d['obs'], d['ret'], idx=idx, leak=leak)
        what = 'partition leak %.1f count %3d' % (leak, count)
        check_parity(what + ' actor ', out.cpu().numpy(), (ref64[0], ref64[1]), (ref32[0], ref32[1]), True, count, 4, stat_scales(fx, rows, True))
        check_parity(what + ' critic', vout.cpu().numpy(), (ref64[2], ref64[3]), (ref32[2], ref32[3]), False, count, 1)


# ---- Adam ----
def adam_case(P):
    rng = np.random.RandomState(P)
    theta = (rng.uniform(0.05, 1.0, P) * rng.choice([-1.0, 1.0], P)).astype(np.float32)
    return theta, [rng.normal(0.0, 1.0, P).astype(np.float32) for _ in range(5)]


@pytest.mark.parametrize('P', (1, 255, 257, 14334))
def test_adam_kernel_is_the_statement_bit_for_bit(P):
    torch = torch_()
    theta, grads = adam_case(P)
    T = lambda a: torch.tensor(a, device=DEV)
    th, m, v, ctr = T(theta), T(np.zeros(P, np.float32)), T(np.zeros(P, np.float32)), torch.zeros(1, dtype=torch.int32, device=DEV)
    rth, rm, rv, step = theta.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32), 0
    for g in grads[:3]:
        TR.adam_step(th, T(g), m, v, ctr, 3e-4)
        rth, rm, rv, step, _ = TR.adam_step_ref(rth, g, rm, rv, step, 3e-4)
        assert np.array_equal(th.cpu().numpy(), rth) and np.array_equal(m.cpu().numpy(), rm) and np.array_equal(v.cpu().numpy(), rv)
    assert int(ctr) == 3 == step


def kl_expr(theta, theta0):
    return (1e-3 + ((theta.double() - theta0.double()) ** 2).mean() * 1e4).float().reshape(1)


def test_adam_gate_five_queued_steps():
    """The three gate cases with 5 steps queued and no host read between them: the KL the gate reads is computed on the device from theta."""
    torch = torch_()
    P = 257
    theta, grads = adam_case(P)
    g = grads[0]
    T = lambda a: torch.tensor(a, device=DEV)
    # the ungated run of the statement gives the KLs to put the limit between
    rth, rm, rv, step, kls = theta.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32), 0, []
    states = [(rth, rm, rv)]
    for _ in range(5):
        kls.append(float(np.float32(1e-3 + np.mean((rth.astype(np.float64) - theta) ** 2) * 1e4)))
        rth, rm, rv, step, _ = TR.adam_step_ref(rth, g, rm, rv, step, 1e-3)
        states.append((rth, rm, rv))
    assert kls == sorted(kls) and kls[1] < kls[2]
    for limit, n_steps in ((0.0, 0), (float('inf'), 5), (0.5 * (kls[1] + kls[2]), 2)):
        th, th0, gd = T(theta), T(theta), T(g)
        m, v = torch.zeros(P, device=DEV), torch.zeros(P, device=DEV)
        ctr, flag = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        kl = torch.zeros(1, device=DEV)
        for _ in range(5):
            kl.copy_(kl_expr(th, th0))
            TR.adam_step(th, gd, m, v, ctr, 1e-3, gate_kl=kl, kl_limit=limit, stop_flag=flag)
        assert int(ctr) == n_steps and int(flag) == (0 if n_steps == 5 else 1), (limit, int(ctr), int(flag))
        want = states[n_steps]
        assert np.array_equal(th.cpu().numpy(), want[0]) and np.array_equal(m.cpu().numpy(), want[1]) and np.array_equal(v.cpu().numpy(), want[2])


# ---- the whole update against the example's torch loop ----
def example_module():
    spec = importlib.util.spec_from_file_location('train_ppo_example', os.path.join(ROOT, 'examples', 'train_ppo.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torch_arm(ex, ac, data, iters, mb=None, target_kl=0.01):
    torch = torch_()
    for p in ac.parameters():
        p.requires_grad_(True)
    pi_params, v_params = ac.pi_W + ac.pi_b + [ac.log_std], ac.v_W + ac.v_b
    res = ex.torch_update(ac, torch.optim.Adam(pi_params, lr=3e-4), torch.optim.Adam(v_params, lr=1e-3), pi_params, v_params, *data,
                          data[0].shape[0] if mb is None else mb, 0.2, target_kl, False, iters=iters)
    for p in ac.parameters():
        p.requires_grad_(False)
    return res


def flat_params(ac):
    return (TR.flatten([w.detach().double().cpu().numpy() for w in ac.pi_W], [b.detach().double().cpu().numpy() for b in ac.pi_b],
                       ac.log_std.detach().double().cpu().numpy()),
            TR.flatten([w.detach().double().cpu().numpy() for w in ac.v_W], [b.detach().double().cpu().numpy() for b in ac.v_b]))


@pytest.mark.parametrize('leak', LEAKS)
def test_whole_update_against_the_torch_loop(leak):
    torch = torch_()
    import ml4ca_amd
    from ml4ca_amd import rollout
    from ml4ca_amd.policy import ActorCritic, policy_forward
    ex = example_module()
    n, T = 64, 64
    env = ml4ca_amd.BatchedRevoltEnv(n, auto_reset=True, seed=4, device=DEV)
    mk = lambda device: ActorCritic(9, 7, (80, 80, 80), leak=leak, seed=2, device=device, activation='leaky' if leak else 'relu')
    ac_f, ac_t, ac_64 = mk(DEV), mk(DEV), mk('cpu')
    ac_64.pi_W, ac_64.pi_b, ac_64.v_W, ac_64.v_b = ([t.double() for t in ts] for ts in (ac_64.pi_W, ac_64.pi_b, ac_64.v_W, ac_64.v_b))
    ac_64.log_std = ac_64.log_std.double()
    buf = rollout.RolloutBuffer(T, env, gamma=0.99, lam=0.97)
    ac_f.upload(env, precision='f32')
    env.reset()
    buf.collect(env, sample=True)
    buf.finish()
    obs, act, adv, ret, lpo = buf.get()
    data = [obs.reshape(-1, 9).float().clone(), act.reshape(-1, 7).clone(), adv.reshape(-1).clone(), ret.reshape(-1).clone(), lpo.reshape(-1).clone()]
    upd = TR.PPOUpdater(ac_f, pi_lr=3e-4, v_lr=1e-3, clip=0.2, target_kl=0.01)
    assert ac_f.pi_W[0].data_ptr() == upd.pi_theta.data_ptr() and ac_f.log_std.data_ptr() == upd.pi_theta[14327:].data_ptr()
    start = flat_params(ac_f)
    it_f, kl_f, vl_f = upd.update(*data, iters=3)
    it_t, kl_t, vl_t = torch_arm(ex, ac_t, data, 3)
    it_64, kl_64, vl_64 = torch_arm(ex, ac_64, [x.double().cpu() for x in data], 3)
    assert it_f == it_t == it_64, (it_f, it_t, it_64)
    got, t32, t64 = flat_params(ac_f), flat_params(ac_t), flat_params(ac_64)
    floor = chain_K(n * T) * 2.0 ** -24
    for k, actor in ((0, True), (1, False)):
        assert np.abs(t64[k] - start[k]).max() > 1e-4                                  # the update moved the parameters
        kern, yard = rel_errors(got[k], t64[k], actor), rel_errors(t32[k], t64[k], actor)
        for name in kern:
            print('whole update leak %.1f %s %-7s fused %.3e  torch-f32-GPU %.3e' % (leak, 'actor ' if actor else 'critic', name, kern[name], yard[name]))
        for name in kern:
            assert kern[name] <= max(8.0 * yard[name], floor), (actor, name, kern[name], yard[name], floor)
    assert abs(kl_f - kl_64) <= max(8.0 * abs(kl_t - kl_64), floor) and abs(vl_f - vl_64) <= max(8.0 * abs(vl_t - vl_64), floor * abs(vl_64))
    # the re-homed views survive an upload and a new rollout: the kernels' parameters are what the env now flies and what forward_ref sees
    ac_f.log_std.clamp_(-4.0, 1.0)
    ac_f.upload(env, precision='f32')
    buf.collect(env, sample=True)
    buf.finish()
    obs, act, adv, ret, lpo = buf.get()
    data2 = [obs.reshape(-1, 9).float().clone(), act.reshape(-1, 7).clone(), adv.reshape(-1).clone(), ret.reshape(-1).clone(), lpo.reshape(-1).clone()]
    before = upd.pi_theta.clone()
    it2, kl2, vl2 = upd.update(*data2, iters=3)
    assert 0 <= it2 <= 3 and np.isfinite(kl2) and np.isfinite(vl2)
    assert ac_f.pi_W[0].data_ptr() == upd.pi_theta.data_ptr() and ac_f.v_W[0].data_ptr() == upd.v_theta.data_ptr()
    if it2:
        assert not torch.equal(before, upd.pi_theta) and not torch.equal(before[:720].view(9, 80), ac_f.pi_W[0])
    assert set(ac_f.state_dict()) == set(ac_t.state_dict())
    ac_f.upload(env, precision='f32')
    mu, v = policy_forward(env, data2[0][:256].contiguous())
    mu_ref, v_ref = ac_f.forward_ref(data2[0][:256])
    assert float((mu - mu_ref).abs().max()) < 1e-4 and float((v - v_ref).abs().max()) < 1e-4


_rows = {}


def rollout_rows(leak):
    """(rows of a real 64 envs x 64 steps policy_rollout through RolloutBuffer, the ActorCritic maker), once per leak."""
    if leak not in _rows:
        import ml4ca_amd
        from ml4ca_amd import rollout
        from ml4ca_amd.policy import ActorCritic
        mk = lambda device: ActorCritic(9, 7, (80, 80, 80), leak=leak, seed=2, device=device, activation='leaky' if leak else 'relu')
        env = ml4ca_amd.BatchedRevoltEnv(64, auto_reset=True, seed=4, device=DEV)
        buf = rollout.RolloutBuffer(64, env, gamma=0.99, lam=0.97)
        mk(DEV).upload(env, precision='f32')
        env.reset()
        buf.collect(env, sample=True)
        buf.finish()
        obs, act, adv, ret, lpo = buf.get()
        _rows[leak] = ([obs.reshape(-1, 9).float().clone(), act.reshape(-1, 7).clone(), adv.reshape(-1).clone(), ret.reshape(-1).clone(),
                        lpo.reshape(-1).clone()], mk)
    return _rows[leak]


@pytest.mark.parametrize('leak', LEAKS)
def test_whole_update_stops_early_on_the_device(leak):
    """The KL gate inside a queued update: an ungated run, step by step, gives the KL before every step; a limit between the KL before
    step j and everything before it must stop BOTH arms after j steps; the fused arm's parameters are the ungated run's after j steps bit
    for bit, the reported kl and the gradient buffer are what the stopping gradient call left (the launches queued behind it return at once)."""
    torch = torch_()
    data, mk = rollout_rows(leak)
    obs, act, adv, ret, lpo = data
    ex = example_module()
    P = 14334
    probe = TR.PPOUpdater(mk(DEV), target_kl=1e9)
    ws = probe._workspace(obs.shape[0])
    kls, thetas, grads = [], [], []
    for j in range(6):
        thetas.append(probe.pi_theta.clone())
        TR.ppo_actor_grad(probe.pi_theta, obs, act, adv, lpo, 0.2, out=probe.pi_grad, workspace=ws, leak=leak)
        grads.append(probe.pi_grad.clone())
        kls.append(float(probe.pi_grad[P + 1]))
        TR.adam_step(probe.pi_theta, probe.pi_grad, probe.pi_m, probe.pi_v, probe.pi_steps, 3e-4)
    print('KL before step j of an ungated update, leak %.1f: %s' % (leak, ' '.join('%.3e' % k for k in kls)))
    stops = [j for j in range(1, 6) if kls[j] > max(kls[:j]) + 1e-6]
    assert stops, kls
    j = stops[0]
    limit = 0.5 * (kls[j] + max(kls[:j]))
    upd = TR.PPOUpdater(mk(DEV), target_kl=limit / 1.5)
    it_f, kl_f, _ = upd.update(*data, iters=6)
    it_t, kl_t, _ = torch_arm(ex, mk(DEV), data, 6, target_kl=limit / 1.5)
    assert it_f == it_t == j < 6, (it_f, it_t, j)
    assert int(upd.stop) == 1 and int(upd.pi_steps) == j
    assert torch.equal(upd.pi_theta, thetas[j]) and torch.equal(upd.pi_grad, grads[j]) and kl_f == kls[j]
    assert abs(kl_t - kl_f) <= 1e-2 * abs(kl_f) + 1e-6, (kl_t, kl_f)
    # the early return itself: a gradient call that finds the flag set writes neither grad_out nor the workspace
    out, w = torch.full((P + 4,), 7.0, device=DEV), torch.full_like(ws, 7.0)
    TR.ppo_actor_grad(upd.pi_theta, obs, act, adv, lpo, 0.2, out=out, workspace=w, leak=leak, stop_flag=upd.stop)
    assert bool((out == 7.0).all()) and bool((w == 7.0).all())
    upd.stop.zero_()
    TR.ppo_actor_grad(upd.pi_theta, obs, act, adv, lpo, 0.2, out=out, workspace=w, leak=leak, stop_flag=upd.stop)
    assert torch.equal(out, grads[j])
    # a second update counts its own steps
    it2, _, _ = upd.update(*data, iters=2)
    assert 0 <= it2 <= 2 and int(upd.pi_steps) == j + it2


@pytest.mark.parametrize('leak', LEAKS)
def test_whole_update_on_minibatches(leak):
    """The minibatch branch (torch.randint -> int32 indices, count = minibatch): with the same torch seed the three arms draw the same
    rows, so fused, torch float32 and torch float64 (all on the GPU) compare as in the full-batch test."""
    torch = torch_()
    data, mk = rollout_rows(leak)
    ex = example_module()
    mb, iters = 1024, 2
    ac_f, ac_t, ac_64 = mk(DEV), mk(DEV), mk(DEV)
    ac_64.pi_W, ac_64.pi_b, ac_64.v_W, ac_64.v_b = ([t.double() for t in ts] for ts in (ac_64.pi_W, ac_64.pi_b, ac_64.v_W, ac_64.v_b))
    ac_64.log_std = ac_64.log_std.double()
    upd = TR.PPOUpdater(ac_f, target_kl=1e9)
    start = flat_params(ac_f)
    torch.manual_seed(5)
    it_f, kl_f, vl_f = upd.update(*data, iters=iters, minibatch=mb)
    torch.manual_seed(5)
    it_t, kl_t, vl_t = torch_arm(ex, ac_t, data, iters, mb=mb, target_kl=1e9)
    torch.manual_seed(5)
    it_64, kl_64, vl_64 = torch_arm(ex, ac_64, [x.double() for x in data], iters, mb=mb, target_kl=1e9)
    assert it_f == it_t == it_64 == iters
    got, t32, t64 = flat_params(ac_f), flat_params(ac_t), flat_params(ac_64)
    floor = chain_K(mb) * 2.0 ** -24
    for k, actor in ((0, True), (1, False)):
        assert np.abs(t64[k] - start[k]).max() > 1e-4
        kern, yard = rel_errors(got[k], t64[k], actor), rel_errors(t32[k], t64[k], actor)
        for name in kern:
            print('minibatch update leak %.1f %s %-7s fused %.3e  torch-f32-GPU %.3e' % (leak, 'actor ' if actor else 'critic', name, kern[name], yard[name]))
        for name in kern:
            assert kern[name] <= max(8.0 * yard[name], floor), (actor, name, kern[name], yard[name], floor)
    assert abs(vl_f - vl_64) <= max(8.0 * abs(vl_t - vl_64), floor * abs(vl_64))
    with pytest.raises(ValueError):
        TR.value_grad(upd.v_theta, data[0], data[3], idx=torch.zeros(8, dtype=torch.int32, device=DEV), count=9)


@pytest.mark.parametrize('leak', LEAKS)
def test_actor_step_in_a_graph_equals_eager(leak):
    """Gradient, reduction and gated Adam of one actor step captured with torch.cuda.graph (a chain: no parallel branches) and replayed,
    against the same calls made eagerly from the same state."""
    torch = torch_()
    fx, d, _ = fixture(leak)
    sh = TR.make_shape(9, 7, True, leak=leak)
    P = 14334

    def state():
        return dict(theta=d['pi_theta'].clone(), m=torch.zeros(P, device=DEV), v=torch.zeros(P, device=DEV), grad=torch.zeros(P + 4, device=DEV),
                    ctr=torch.zeros(1, dtype=torch.int32, device=DEV), flag=torch.zeros(1, dtype=torch.int32, device=DEV),
                    ws=torch.empty(TR.workspace_bytes(sh, 257) // 4, device=DEV))

    def step(s):
        TR.ppo_actor_grad(s['theta'], d['obs'], d['act'], d['adv'], d['logp_old'], F.CLIP, out=s['grad'], workspace=s['ws'], leak=leak, stop_flag=s['flag'],
                          count=257)
        TR.adam_step(s['theta'], s['grad'], s['m'], s['v'], s['ctr'], 3e-4, gate_kl=s['grad'][P + 1:P + 2], kl_limit=float('inf'), stop_flag=s['flag'])

    eager, graphed = state(), state()
    for _ in range(2):
        step(eager)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(graphed)                                            # warm up the launch path outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh = state()
    for k in ('theta', 'm', 'v', 'grad', 'ctr', 'flag'):
        graphed[k].copy_(fresh[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed)
    for k in ('theta', 'm', 'v', 'grad', 'ctr', 'flag'):
        graphed[k].copy_(fresh[k])                               # the capture ran nothing
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for k in ('theta', 'm', 'v', 'grad', 'ctr', 'flag'):
        assert torch.equal(eager[k], graphed[k]), k
    assert int(eager['ctr']) == 2 and not torch.equal(eager['theta'], d['pi_theta'])


def test_refusals_leave_everything_untouched():
    torch = torch_()
    lib = _lib.load()
    fx, d, _ = fixture(0.2)
    good, vshape = TR.make_shape(9, 7, True), TR.make_shape(9, 1, False)
    P = 14334
    out = torch.full((P + 4,), 7.0, device=DEV)
    vout = torch.full((13842,), 7.0, device=DEV)
    ws = torch.full((2 * (P + 4),), 7.0, device=DEV)
    flag, ctr = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), 3, dtype=torch.int32, device=DEV)
    idx = torch.arange(8, dtype=torch.int32, device=DEV)
    theta0, vtheta0 = d['pi_theta'].clone(), d['v_theta'].clone()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def actor(shape=good, theta=d['pi_theta'], obs=d['obs'], act=d['act'], adv=d['adv'], lpo=d['logp_old'], idx=None, count=64, n_rows=N_ROWS, out=out,
              ws=ws, ws_bytes=None):
        return lib.dpenv_ppo_actor_grad(C.byref(shape), p(theta), p(obs), p(act), p(adv), p(lpo), p(idx), count, n_rows, 0.2, p(flag), p(out), p(ws),
                                        ws.numel() * 4 if ws_bytes is None and ws is not None else (ws_bytes or 0), None)

    def critic(shape=vshape, obs=d['obs'], count=64, n_rows=N_ROWS, ws_bytes=None):
        return lib.dpenv_value_grad(C.byref(shape), p(d['v_theta']), p(obs), p(d['ret']), None, count, n_rows, p(vout), p(ws),
                                    ws.numel() * 4 if ws_bytes is None else ws_bytes, None)

    calls = [lambda: actor(count=0), lambda: actor(count=-1), lambda: critic(count=0),
             lambda: actor(theta=None), lambda: actor(obs=None), lambda: actor(act=None), lambda: actor(adv=None), lambda: actor(lpo=None),
             lambda: actor(out=None), lambda: actor(ws=None), lambda: critic(obs=None),
             lambda: actor(count=129, ws_bytes=2 * 4 * (P + 4)), lambda: critic(count=65, ws_bytes=4 * 13842),
             lambda: actor(shape=TR.make_shape(9, 7, True, activation='tanh')), lambda: critic(shape=TR.make_shape(9, 1, False, activation='tanh')),
             lambda: actor(shape=TR.make_shape(9, 7, True, hidden=(64, 64, 64))), lambda: actor(shape=TR.make_shape(9, 7, True, hidden=(80, 80))),
             lambda: actor(shape=TR.make_shape(9, 8, True)), lambda: actor(shape=TR.make_shape(9, 7, True, row_dtype=_lib.BF16)),
             lambda: actor(idx=idx, count=8, n_rows=0), lambda: actor(idx=idx, count=8, n_rows=-5),
             lambda: lib.dpenv_adam_step(p(d['pi_theta']), p(out), None, p(out), P, 3e-4, 0.9, 0.999, 1e-8, p(ctr), None, 0.0, None, None),
             lambda: lib.dpenv_adam_step(p(d['pi_theta']), p(out), p(out), p(out), 0, 3e-4, 0.9, 0.999, 1e-8, p(ctr), None, 0.0, None, None),
             lambda: lib.dpenv_adam_step(p(d['pi_theta']), p(out), p(out), p(out), P, 3e-4, 0.9, 0.999, 1e-8, p(ctr), p(out), 0.0, None, None)]
    for k, call in enumerate(calls):
        assert call() == _lib.EINVAL, k
        assert lib.dpenv_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((vout == 7.0).all()) and bool((ws == 7.0).all())
    assert torch.equal(d['pi_theta'], theta0) and torch.equal(d['v_theta'], vtheta0)
    assert int(flag) == 0 and int(ctr) == 3
    # and the same buffers are accepted by a call that is in order
    assert actor() == _lib.OK and critic() == _lib.OK
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
