"""The fused imitation gradient on the GPU (ml4ca_amd/train.py: imitation_grad, PPOUpdater.pretrain; dpenv_train.hip:
imitation_grad_kernel) against torch float64 autograd of the two losses, its own identities, the kernels it shares a body and a
workspace with, and a torch imitation loop.

THE BOUND is the one tests/test_gpu_ppo_update.py derives: error per parameter tensor relative to that tensor's largest float64-autograd
value, allowed max(8 x the same error of torch's float32 autograd on the same rows, K x 2^-24), K the roundings along the longest
accumulation chain.  K is that file's chain_K with ONE term shortened: its output-gradient term counts 20 roundings (quotient, square,
7-term sum, exp, the clip products, dlogp/dmu); this loss has no ratio and no clip, which leaves
    quotient 1, square 1, + 2 log_std and + log(2 pi) 2, the 7-term sum 7, the weight product 1, q / sd 1, the product with -w 1  = 14
(the MSE stage is shorter still - difference, square, 7-term sum, 2 w, product - and is held to the same 14).  Nothing is masked out of
a comparison: the rows keep their margin from the leaky-relu kink and the loss has no other.
Statistics: |kernel - float64| <= max(8 x |torch-f32 - float64|, K x 2^-24 x S) with the input-sized scales S = max|w| max_i |logp_i| for the
weighted NLL and S = max|w| max_i sum_j (mu_j - act_j)^2 for the weighted MSE (the chosen loss takes the scale of its kind); grad_out[P+3]
is +0.0 as bits.  A tensor or statistic whose reference is zero must come out zero."""
import ctypes as C
import os

import numpy as np
import pytest

from ml4ca_amd import _lib
from ml4ca_amd import train as TR
from tests import ppo_fixture as F
from tests.test_gpu_ppo_update import chain_K as ppo_chain_K
from tests.test_imitation_cpu import make_weights, rel_errors, slices, small_fixture, torch_imitation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEAKS = (0.2, 0.0)
LOSSES = ('nll', 'mse')
N_ROWS = 300
COUNTS = (1, 63, 64, 65, 165, 257)
MANY_TILES = 33000                                     # 516 tiles on 256 workgroups: two or three tiles each, the last tile ragged
assert TR.grid(MANY_TILES) == 256 and MANY_TILES % 64 != 0
RECORD = os.environ.get('IMITATION_PARITY_RECORD', '')  # a path: the measured yardstick and kernel errors are appended there
P = 14334


def torch_():
    import torch
    return torch


def chain_K(count):
    return ppo_chain_K(count) - 20 + 14


_cache = {}


def fixture(leak):
    """The shared fixture, its weight vector and their device copies (built once per leak, never changed)."""
    if leak not in _cache:
        torch = torch_()
        fx = F.make_fixture(N_ROWS, leak)
        w = make_weights(N_ROWS)
        w[[0, 64]] = (1.5, 0.5)                        # the lone rows of count 1 and of count 65's second workgroup carry a gradient
        assert 15 <= int((w == 0).sum()) <= 50 and w.max() <= 2.0
        fx['weight'] = w
        dev = {k: torch.tensor(fx[k], device=DEV) for k in ('pi_theta', 'v_theta', 'obs', 'act', 'adv', 'ret', 'logp_old', 'weight')}
        _cache[leak] = (fx, dev, {})
    return _cache[leak]


def references(fx, refs, rows, loss, weight, theta_key='pi_theta'):
    """float64 autograd and the float32 yardstick on the CPU (cached per row set, loss and weight vector)."""
    torch = torch_()
    key = (np.asarray(rows).tobytes(), loss, None if weight is None else np.asarray(weight).tobytes())
    if key not in refs:
        refs[key] = tuple(torch_imitation(fx[theta_key], fx['obs'], fx['act'], loss, weight=weight, rows=rows, leak=fx['leak'], dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return refs[key]


def stat_scales(fx, rows, weight, loss, theta_key='pi_theta'):
    """(S of the chosen loss, S_nll, S_mse): max|w| max|logp_i| and max|w| max_i sum_j (mu - act)^2 over the rows, in float64."""
    obs, act = fx['obs'][rows], fx['act'][rows].astype(np.float64)
    _, _, ls, _, _, mu = TR._forward64(fx[theta_key], obs, obs.shape[1], act.shape[1], True, fx['leak'])
    q = (act - mu) / (np.exp(ls) + 1e-8)
    logp = (-0.5 * ((q * q + 2.0 * ls) + np.log(2.0 * np.pi))).sum(1)
    wmax = 1.0 if weight is None else float(np.abs(np.asarray(weight)[rows]).max())
    s_nll, s_mse = wmax * float(np.abs(logp).max()), wmax * float(((mu - act) ** 2).sum(1).max())
    return (s_nll if loss == 'nll' else s_mse, s_nll, s_mse)


def check_parity(what, got, ref64, ref32, sls, count, scales):
    """got [P + 4] float32 from the device against the (grad, stats) references."""
    n = ref64[0].size
    bits = np.asarray(got, np.float32)
    got = bits.astype(np.float64)
    floor = chain_K(count) * 2.0 ** -24
    kern, yard = rel_errors(got[:n], ref64[0], sls), rel_errors(ref32[0], ref64[0], sls)
    lines = []
    for name in kern:
        lines.append('%s %-7s kernel %.3e  torch-f32 %.3e  bound %.3e' % (what, name, kern[name], yard[name], max(8.0 * yard[name], floor)))
    for j, name in enumerate(('loss', 'nll', 'mse')):
        lines.append('%s %-7s kernel %.3e  torch-f32 %.3e  bound %.3e (absolute; value %.6g)' % (
            what, name, abs(got[n + j] - ref64[1][j]), abs(ref32[1][j] - ref64[1][j]), max(8.0 * abs(ref32[1][j] - ref64[1][j]), floor * scales[j]),
            ref64[1][j]))
    print('\n'.join(lines))
    if RECORD:
        with open(RECORD, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert len(got) == n + 4
    for name in kern:
        assert kern[name] <= max(8.0 * yard[name], floor), (what, name, kern[name], yard[name], floor)
    for j, name in enumerate(('loss', 'nll', 'mse')):
        assert abs(got[n + j] - ref64[1][j]) <= max(8.0 * abs(ref32[1][j] - ref64[1][j]), floor * scales[j]), (what, name, got[n + j], ref64[1][j], ref32[1][j])
    assert bits[n + 3:].view(np.int32)[0] == 0, (what, 'the reserved slot is not +0.0')


def index_rows(mode, count, seed):
    rng = np.random.RandomState(seed)
    if mode == 'none':
        return None, np.arange(count)
    rows = rng.permutation(N_ROWS)[:count] if mode == 'perm' else rng.randint(0, max(N_ROWS // 3, 1), size=count)
    return rows.astype(np.int32), rows


def run_parity(leak, loss, idx_np, rows, count, what):
    """One index set, without weights and with the fixture's weight vector."""
    torch = torch_()
    fx, d, refs = fixture(leak)
    idx = None if idx_np is None else torch.tensor(np.asarray(idx_np, np.int32), device=DEV)
    ls = F.tensor_slices(True)[-1][1]
    for tag, w_np, w_dev in (('w none', None, None), ('w rand', fx['weight'], d['weight'])):
        ref64, ref32 = references(fx, refs, rows, loss, w_np)
        out = TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=w_dev, idx=idx, leak=leak, count=count).cpu().numpy()
        check_parity('%s %s %s' % (what, loss, tag), out, ref64, ref32, F.tensor_slices(True), count, stat_scales(fx, rows, w_np, loss))
        if loss == 'mse':
            assert not ref64[0][ls].any() and not out[ls].view(np.int32).any()       # MSE's log_std gradient: +0.0, as bits
        elif w_np is None or np.asarray(w_np)[rows].any():
            assert all(np.abs(ref64[0][sl]).max() > 0 for _, sl in F.tensor_slices(True))          # no tensor compares zero with zero


@pytest.mark.parametrize('mode', ('none', 'perm', 'repeats'))
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_gradient_parity(leak, loss, count, mode):
    idx_np, rows = index_rows(mode, count, 100 * count + len(mode))
    if mode == 'repeats' and count > 1:
        assert len(set(rows.tolist())) < count
    run_parity(leak, loss, idx_np, rows, count, 'leak %.1f count %3d idx %-7s' % (leak, count, mode))


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_gradient_parity_several_tiles_per_workgroup(leak, loss):
    rows = np.random.RandomState(33).randint(0, N_ROWS, size=MANY_TILES)
    run_parity(leak, loss, rows, rows, MANY_TILES, 'leak %.1f count %d idx repeats' % (leak, MANY_TILES))


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_all_selected_rows_masked_gives_zero(leak, loss):
    """count 64, every selected row with weight exactly 0 (rows outside the selection keep theirs): every tensor and statistic is zero."""
    torch = torch_()
    fx, d, refs = fixture(leak)
    rows = np.random.RandomState(2).permutation(N_ROWS)[:64]
    w = fx['weight'].copy()
    w[rows] = 0.0
    assert w.any()
    ref64, ref32 = references(fx, refs, rows, loss, w)
    assert not ref64[0].any() and not ref64[1].any()
    out = TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=torch.tensor(w, device=DEV),
                            idx=torch.tensor(rows.astype(np.int32), device=DEV), leak=leak).cpu().numpy()
    check_parity('leak %.1f count  64 masked %s' % (leak, loss), out, ref64, ref32, F.tensor_slices(True), 64, (0.0, 0.0, 0.0))
    assert not out.any()


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_gradient_parity_another_shape(leak, loss):
    """in = 3, out = 5 (the supervised allocator's widths) at count 65: the padded input and output tiles with other live widths."""
    torch = torch_()
    fx = small_fixture(leak)
    n = fx['obs'].shape[0]
    fx['weight'] = make_weights(n, seed=8)
    fx['weight'][64] = 0.75
    rows = np.arange(65)
    sls = slices(3, 5)
    T = lambda a: torch.tensor(a, device=DEV)
    refs = {}
    for tag, w in (('w none', None), ('w rand', fx['weight'])):
        ref64, ref32 = references(fx, refs, rows, loss, w, theta_key='theta')
        out = TR.imitation_grad(T(fx['theta']), T(fx['obs']), T(fx['act']), loss=loss, weight=None if w is None else T(w), leak=leak, count=65)
        assert out.numel() == TR.layout(3, 5, True)['P'] + 4
        check_parity('leak %.1f 3 -> 5 count 65 %s %s' % (leak, loss, tag), out.cpu().numpy(), ref64, ref32, sls, 65,
                     stat_scales(fx, rows, w, loss, theta_key='theta'))


# ---- identities and interplay ----
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_no_weight_is_weight_one_and_equal_calls_give_equal_bits(leak, loss):
    torch = torch_()
    fx, d, _ = fixture(leak)
    idx = torch.tensor(index_rows('repeats', 257, 5)[0], device=DEV)
    call = lambda w: TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=w, idx=idx, leak=leak)
    none, ones = call(None), call(torch.ones(N_ROWS, device=DEV))
    assert torch.equal(none.view(torch.int32), ones.view(torch.int32))
    a, b = call(d['weight']), call(d['weight'])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, none)
    assert bool(torch.isfinite(a).all()) and bool(a.abs().max() > 0)


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('leak', LEAKS)
def test_workgroup_partition(leak, loss):
    """The same 64 rows as ONE workgroup (count 64) and, each three times in a shuffled order, as the THREE TR.grid deals for count 192:
    the mean gradient is the same number, so both sit within the parity bound of the float64 reference of the 64 rows."""
    torch = torch_()
    fx, d, refs = fixture(leak)
    rng = np.random.RandomState(9)
    rows = rng.permutation(N_ROWS)[:64]
    rows3 = rng.permutation(np.tile(rows, 3))
    assert TR.grid(64) == 1 and TR.grid(192) == 3
    ref64, ref32 = references(fx, refs, rows, loss, fx['weight'])
    for r, count in ((rows, 64), (rows3, 192)):
        out = TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=d['weight'], idx=torch.tensor(r.astype(np.int32), device=DEV), leak=leak)
        check_parity('partition leak %.1f count %3d %s' % (leak, count, loss), out.cpu().numpy(), ref64, ref32, F.tensor_slices(True), count,
                     stat_scales(fx, rows, fx['weight'], loss))


def test_stop_flag_and_the_kernels_that_share_the_workspace():
    """A set stop_flag leaves grad_out and the workspace as they were; dpenv_ppo_actor_grad and dpenv_value_grad return the bits they
    returned before an imitation call went through their workspace."""
    torch = torch_()
    fx, d, _ = fixture(0.2)
    sh = TR.make_shape(9, 7, True)
    ws = torch.full((TR.workspace_bytes(sh, 257) // 4,), 7.0, device=DEV)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    out = torch.full((P + 4,), 7.0, device=DEV)
    ppo = lambda: TR.ppo_actor_grad(d['pi_theta'], d['obs'], d['act'], d['adv'], d['logp_old'], F.CLIP, workspace=ws, count=257).clone()
    val = lambda: TR.value_grad(d['v_theta'], d['obs'], d['ret'], workspace=ws, count=257).clone()
    for loss in LOSSES:
        TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=d['weight'], out=out, workspace=ws, stop_flag=flag, count=257)
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    before = (ppo(), val())
    flag.zero_()
    for loss in LOSSES:
        TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=d['weight'], out=out, workspace=ws, stop_flag=flag, count=257)
        assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
        after = (ppo(), val())
        assert torch.equal(before[0].view(torch.int32), after[0].view(torch.int32)) and torch.equal(before[1].view(torch.int32), after[1].view(torch.int32))
        fresh = TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=loss, weight=d['weight'], count=257)
        assert torch.equal(out, fresh)                            # ... and the imitation call is not disturbed by theirs


def test_refusals_leave_everything_untouched():
    torch = torch_()
    lib = _lib.load()
    fx, d, _ = fixture(0.2)
    good = TR.make_shape(9, 7, True)
    out = torch.full((P + 4,), 7.0, device=DEV)
    ws = torch.full((2 * (P + 4),), 7.0, device=DEV)
    idx = torch.arange(8, dtype=torch.int32, device=DEV)
    theta0 = d['pi_theta'].clone()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(shape=good, theta=d['pi_theta'], obs=d['obs'], act=d['act'], weight=d['weight'], idx=None, count=64, n_rows=N_ROWS, loss=_lib.IMITATE_MSE,
             out=out, ws=ws, ws_bytes=None):
        return lib.dpenv_imitation_grad(C.byref(shape), p(theta), p(obs), p(act), p(weight), p(idx), count, n_rows, loss, None, p(out), p(ws),
                                        ws.numel() * 4 if ws_bytes is None and ws is not None else (ws_bytes or 0), None)

    calls = [lambda: call(loss=2), lambda: call(shape=TR.make_shape(9, 1, False)), lambda: call(count=0), lambda: call(count=-1),
             lambda: call(theta=None), lambda: call(obs=None), lambda: call(act=None), lambda: call(out=None), lambda: call(ws=None),
             lambda: call(count=129, ws_bytes=2 * 4 * (P + 4)), lambda: call(count=65, ws_bytes=2 * 4 * (P + 4) - 1),
             lambda: call(idx=idx, count=8, n_rows=0), lambda: call(count=N_ROWS + 1),
             lambda: call(shape=TR.make_shape(9, 7, True, activation='tanh')), lambda: call(shape=TR.make_shape(9, 7, True, row_dtype=_lib.BF16)),
             lambda: call(shape=TR.make_shape(9, 7, True, hidden=(64, 64, 64))), lambda: call(shape=TR.make_shape(9, 8, True))]
    for k, c in enumerate(calls):
        assert c() == _lib.EINVAL, k
        assert lib.dpenv_last_error(None)
    with pytest.raises(ValueError):
        TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss='huber', out=out, workspace=ws)
    with pytest.raises(_lib.DpenvError):
        TR.imitation_grad(d['pi_theta'], d['obs'], d['act'], loss=2, out=out, workspace=ws, count=64)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all()) and torch.equal(d['pi_theta'], theta0)
    assert call() == _lib.OK and call(weight=None, loss=_lib.IMITATE_NLL, count=128) == _lib.OK      # the same buffers, calls that are in order
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize('loss', LOSSES)
def test_step_in_a_graph_equals_eager(loss):
    """Gradient, reduction and ungated Adam of one imitation step captured with torch.cuda.graph (a chain: no parallel branches) and
    replayed, against the same calls made eagerly from the same state.  The first call of the process is made outside the capture."""
    torch = torch_()
    fx, d, _ = fixture(0.2)
    sh = TR.make_shape(9, 7, True)

    def state():
        return dict(theta=d['pi_theta'].clone(), m=torch.zeros(P, device=DEV), v=torch.zeros(P, device=DEV), grad=torch.zeros(P + 4, device=DEV),
                    ctr=torch.zeros(1, dtype=torch.int32, device=DEV), ws=torch.empty(TR.workspace_bytes(sh, 257) // 4, device=DEV))

    def step(s):
        TR.imitation_grad(s['theta'], d['obs'], d['act'], loss=loss, weight=d['weight'], out=s['grad'], workspace=s['ws'], count=257)
        TR.adam_step(s['theta'], s['grad'], s['m'], s['v'], s['ctr'], 1e-3)

    keys = ('theta', 'm', 'v', 'grad', 'ctr')
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
    for k in keys:
        graphed[k].copy_(fresh[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed)
    for k in keys:
        graphed[k].copy_(fresh[k])                               # the capture ran nothing
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(eager[k], graphed[k]), k
    assert int(eager['ctr']) == 2 and not torch.equal(eager['theta'], d['pi_theta'])


# ---- end to end, small: clone the baseline, then PPO ----
_demo = {}


def demonstration():
    """(env, obs [16 384, 9], act [16 384, 7]): 256 envs with the default baseline on, one controller_rollout of 64 steps (built once)."""
    if not _demo:
        import ml4ca_amd
        from ml4ca_amd.policy import controller_rollout
        env = ml4ca_amd.BatchedRevoltEnv(256, auto_reset=True, seed=4, device=DEV)        # final variant, continuous angles, extended state
        env.set_dp_controller()
        env.reset()
        o = controller_rollout(env, 64)
        env.set_dp_controller(off=True)
        _demo['d'] = (env, o['obs'].reshape(-1, 9).float().contiguous().clone(), o['act'].reshape(-1, 7).contiguous().clone())
    return _demo['d']


def flat_actor(ac):
    return TR.flatten([w.detach().double().cpu().numpy() for w in ac.pi_W], [b.detach().double().cpu().numpy() for b in ac.pi_b],
                      ac.log_std.detach().double().cpu().numpy())


def torch_pretrain(ac, obs, act, loss, iters, lr):
    """The same loss through autograd + torch.optim.Adam, full batch; returns the MSE before every step."""
    torch = torch_()
    params = ac.pi_W + ac.pi_b + [ac.log_std]
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=lr)
    mses = []
    for _ in range(iters):
        mu = ac._mlp(obs, ac.pi_W, ac.pi_b)
        mse = ((mu - act) ** 2).sum(dim=1).mean()
        mses.append(float(mse.detach()))
        opt.zero_grad()
        (mse if loss == 'mse' else -ac.logp_ref(act, mu).mean()).backward()
        opt.step()
    for p in params:
        p.requires_grad_(False)
    return mses


@pytest.mark.parametrize('loss', ('mse', 'nll'))
def test_pretrain_against_the_torch_loop_then_ppo(loss):
    torch = torch_()
    from ml4ca_amd import rollout
    from ml4ca_amd.policy import ActorCritic, policy_forward
    env, obs, act = demonstration()
    assert obs.shape == (16384, 9) and act.shape == (16384, 7) and bool(torch.isfinite(obs).all()) and bool(torch.isfinite(act).all())
    mk = lambda device: ActorCritic(9, 7, (80, 80, 80), leak=0.2, seed=2, device=device)
    ac_f, ac_t, ac_64 = mk(DEV), mk(DEV), mk('cpu')
    ac_64.pi_W, ac_64.pi_b = ([t.double() for t in ts] for ts in (ac_64.pi_W, ac_64.pi_b))
    ac_64.log_std = ac_64.log_std.double()
    upd = TR.PPOUpdater(ac_f, pi_lr=3e-4, v_lr=1e-3)
    start = flat_actor(ac_f)
    hist = upd.pretrain(obs, act, 5, loss=loss, lr=1e-3)
    m32 = torch_pretrain(ac_t, obs, act, loss, 5, 1e-3)
    m64 = torch_pretrain(ac_64, obs.double().cpu(), act.double().cpu(), loss, 5, 1e-3)
    assert tuple(hist.shape) == (5, 4) and not hist[:, 3].any() and torch.equal(hist[:, 0], hist[:, 2 if loss == 'mse' else 1])
    got, t32, t64 = flat_actor(ac_f), flat_actor(ac_t), flat_actor(ac_64)
    floor = chain_K(16384) * 2.0 ** -24
    assert np.abs(t64 - start).max() > 1e-4                                            # the steps moved the parameters
    kern, yard = rel_errors(got, t64, F.tensor_slices(True)), rel_errors(t32, t64, F.tensor_slices(True))
    for name in kern:
        print('pretrain %s %-7s fused %.3e  torch-f32-GPU %.3e  bound %.3e' % (loss, name, kern[name], yard[name], max(8.0 * yard[name], floor)))
    for k in (0, 4):
        print('pretrain %s MSE before step %d: fused %.8g  torch-f32-GPU %.8g  float64 %.8g' % (loss, k, float(hist[k, 2]), m32[k], m64[k]))
    for name in kern:
        assert kern[name] <= max(8.0 * yard[name], floor), (name, kern[name], yard[name], floor)
    for k in (0, 4):
        assert abs(float(hist[k, 2]) - m64[k]) <= max(8.0 * abs(m32[k] - m64[k]), floor * abs(m64[k])), (k, float(hist[k, 2]), m32[k], m64[k])
    # Adam starts afresh for PPO, unless asked otherwise
    assert not upd.pi_m.any() and not upd.pi_v.any() and int(upd.pi_steps) == 0 and upd._pi_steps_host == 0
    upd.pretrain(obs, act, 2, loss=loss, lr=1e-3, minibatch=1024, keep_optimizer_state=True)
    assert bool(upd.pi_m.any()) and bool(upd.pi_v.any()) and int(upd.pi_steps) == 2 == upd._pi_steps_host
    upd.pretrain(obs, act, 1, loss=loss, lr=1e-3)
    assert not upd.pi_m.any() and int(upd.pi_steps) == 0 == upd._pi_steps_host
    # the critic's half: the existing value_grad + adam_step loop with the same history and reset behaviour
    ret = torch.linspace(-1.0, 1.0, 16384, device=DEV)
    hv = upd.pretrain_critic(obs, ret, 5)
    assert tuple(hv.shape) == (5, 1) and bool(torch.isfinite(hv).all()) and float(hv[0, 0]) > 0 and not upd.v_m.any() and not upd.v_v.any() and int(upd.v_steps) == 0
    # PPO from the clone: real policy_rollout rows, pi_iters counted from zero
    with torch.no_grad():
        ac_f.log_std.clamp_(-4.0, 1.0)
    ac_f.upload(env, precision='f32')
    env.reset()
    buf = rollout.RolloutBuffer(64, env, gamma=0.99, lam=0.97)
    buf.collect(env, sample=True)
    buf.finish()
    o, a, adv, rt, lpo = buf.get()
    data = [o.reshape(-1, 9).float().clone(), a.reshape(-1, 7).clone(), adv.reshape(-1).clone(), rt.reshape(-1).clone(), lpo.reshape(-1).clone()]
    it, kl, vl = upd.update(*data, iters=3)
    assert 0 <= it <= 3 and it == int(upd.pi_steps) and np.isfinite(kl) and np.isfinite(vl)
    assert ac_f.pi_W[0].data_ptr() == upd.pi_theta.data_ptr() and ac_f.log_std.data_ptr() == upd.pi_theta[14327:].data_ptr()
    ac_f.upload(env, precision='f32')
    mu, v = policy_forward(env, data[0][:256].contiguous())
    mu_ref, v_ref = ac_f.forward_ref(data[0][:256])
    assert float((mu - mu_ref).abs().max()) < 1e-4 and float((v - v_ref).abs().max()) < 1e-4
