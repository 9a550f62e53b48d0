"""The allocation gradient on the GPU (ml4ca_amd/train.py: allocation_grad, fit_nn_allocator(loss='wrench'); dpenv_train.hip:
allocation_grad_kernel) against torch float64 autograd of the loss written through the thrust map, its own identities, the kernels it
shares a body and a workspace with, the fit it is for and one small flight of the fitted network.

THE BOUND is the one tests/test_gpu_ppo_update.py derives and tests/test_gpu_imitation.py applies: error per parameter tensor relative to
that tensor's largest float64-autograd value, allowed max(8 x the same error of torch's float32 autograd on the same rows, K x 2^-24), K the
roundings along the longest accumulation chain.  K is that file's chain_K with ONE term re-counted: its output-gradient term counts 20
roundings; this stage's longest chain from the network's output p to dL/dp runs through a stern angle:
    p * angle_scale 1, sincos 8 (three reduction fmaf, the polynomial's four, the quadrant's sign: its stated 9.2e-8), b3 = lx s - ly c 2,
    b3 * F 1, the 3-term wrench sum 2, - tau 1, w_slack * r 1, Jm * wr 1, the 3-term sum over the wrench 2, + the power term 1, * dF 1,
    + the saturation term 1, * w_row 1                                                                                              = 23
(the thrust chain clip, * 100, K n, * |n| is shorter and runs beside the sincos).  Nothing is masked out of a comparison: the rows keep
their margin from the leaky-relu kink, from |p| = 1 and from p = 0 (tests/test_allocation_loss_cpu.py asserts the fixture's conditions).
Statistics: |kernel - float64| <= max(8 x |torch-f32 - float64|, K x 2^-24 x S) with the input-sized scales S = max|w| max_i of the row's
J, Js, Jp and Jx.  A tensor or statistic whose reference is zero must come out zero; the log_std slice is +0.0 as bits."""
import numpy as np
import pytest

from ml4ca_amd import deploy
from ml4ca_amd import train as TR
from tests import ppo_fixture as F
from tests.test_allocation_loss_cpu import FIT, alloc_fixture, loss_params, torch_alloc_loss
from tests.test_gpu_ppo_update import chain_K as ppo_chain_K
from tests.test_imitation_cpu import make_weights, rel_errors, slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEAKS = (0.2, 0.0)
IN_DIMS = (9, 3)
MODES = (0, 1)
N_ROWS = 300
COUNTS = (1, 63, 64, 65, 165, 257)
MANY_TILES = 33000                                     # 516 tiles on 256 workgroups: two or three tiles each, the last tile ragged
assert TR.grid(MANY_TILES) == 256 and MANY_TILES % 64 != 0
STATS = ('L', 'Js', 'Jp', 'Jx')


def torch_():
    import torch
    return torch


def chain_K(count):
    return ppo_chain_K(count) - 20 + 23


_cache = {}


def fixture(in_dim, leak):
    """The shared fixture, its weight vector and their device copies (built once per shape and leak, never changed)."""
    key = (in_dim, leak)
    if key not in _cache:
        torch = torch_()
        fx = dict(alloc_fixture(in_dim, leak, N_ROWS))
        w = make_weights(N_ROWS)
        w[[0, 64]] = (1.5, 0.5)                        # the lone rows of count 1 and of count 65's second workgroup carry a gradient
        assert 15 <= int((w == 0).sum()) <= 50 and w.max() <= 2.0
        fx['weight'] = w
        dev = {k: torch.tensor(fx[k], device=DEV) for k in ('theta', 'x', 'tau', 'weight')}
        _cache[key] = (fx, dev, {})
    return _cache[key]


def references(fx, refs, rows, q, weight):
    """float64 autograd and the float32 yardstick on the CPU (cached per row set, azimuth mode and weight vector)."""
    torch = torch_()
    key = (np.asarray(rows).tobytes(), int(q['azimuth_mode']), None if weight is None else np.asarray(weight).tobytes())
    if key not in refs:
        refs[key] = tuple(torch_alloc_loss(fx['theta'], fx['x'], fx['tau'], q, weight=weight, rows=rows, leak=fx['leak'], dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return refs[key]


def stat_scales(fx, rows, q, weight):
    p = TR._forward64(fx['theta'], fx['x'][rows], fx['in_dim'], 6, True, fx['leak'])[5]
    t = TR.alloc_loss_terms(p, fx['tau'][rows], q)
    wmax = 1.0 if weight is None else float(np.abs(np.asarray(weight)[rows]).max())
    return [wmax * float(t[k].max()) for k in ('J', 'Js', 'Jp', 'Jx')]


def check_parity(what, got, ref64, ref32, sls, count, scales):
    """got [P + 4] float32 from the device against the (grad, stats) references; every figure is printed before anything is asserted."""
    n = ref64[0].size
    bits = np.asarray(got, np.float32)
    got = bits.astype(np.float64)
    floor = chain_K(count) * 2.0 ** -24
    kern, yard = rel_errors(got[:n], ref64[0], sls), rel_errors(ref32[0], ref64[0], sls)
    for name in kern:
        print('%s %-7s kernel %.3e  torch-f32 %.3e  bound %.3e' % (what, name, kern[name], yard[name], max(8.0 * yard[name], floor)))
    for j, name in enumerate(STATS):
        print('%s %-7s kernel %.3e  torch-f32 %.3e  bound %.3e (absolute; value %.6g)' % (
            what, name, abs(got[n + j] - ref64[1][j]), abs(ref32[1][j] - ref64[1][j]), max(8.0 * abs(ref32[1][j] - ref64[1][j]), floor * scales[j]),
            ref64[1][j]))
    assert len(got) == n + 4
    for name in kern:
        assert kern[name] <= max(8.0 * yard[name], floor), (what, name, kern[name], yard[name], floor)
    for j, name in enumerate(STATS):
        assert abs(got[n + j] - ref64[1][j]) <= max(8.0 * abs(ref32[1][j] - ref64[1][j]), floor * scales[j]), (what, name, got[n + j], ref64[1][j], ref32[1][j])
    ls = sls[-1][1]
    assert not ref64[0][ls].any() and not bits[:n][ls].view(np.int32).any(), (what, 'the log_std slice is not +0.0')


def index_rows(mode, count, seed):
    rng = np.random.RandomState(seed)
    if mode == 'none':
        return None, np.arange(count)
    rows = rng.permutation(N_ROWS)[:count] if mode == 'perm' else rng.randint(0, max(N_ROWS // 3, 1), size=count)
    return rows.astype(np.int32), rows


def run_parity(in_dim, leak, mode, idx_np, rows, count, what):
    """One index set, without weights and with the fixture's weight vector; the NaN-filled columns 3..5 change no bit."""
    torch = torch_()
    fx, d, refs = fixture(in_dim, leak)
    q = loss_params(mode)
    idx = None if idx_np is None else torch.tensor(np.asarray(idx_np, np.int32), device=DEV)
    sls = slices(in_dim, 6)
    tau_nan = d['tau'].clone()
    tau_nan[:, 3:] = float('nan')
    for tag, w_np, w_dev in (('w none', None, None), ('w rand', fx['weight'], d['weight'])):
        ref64, ref32 = references(fx, refs, rows, q, w_np)
        out = TR.allocation_grad(d['theta'], d['x'], d['tau'], q, weight=w_dev, idx=idx, leak=leak, count=count)
        out_nan = TR.allocation_grad(d['theta'], d['x'], tau_nan, q, weight=w_dev, idx=idx, leak=leak, count=count)
        assert torch.equal(out.view(torch.int32), out_nan.view(torch.int32)), (what, tag, 'columns 3..5 of the target reached a result')
        check_parity('%s %s' % (what, tag), out.cpu().numpy(), ref64, ref32, sls, count, stat_scales(fx, rows, q, w_np))
        if w_np is None or np.asarray(w_np)[rows].any():
            assert all(np.abs(ref64[0][sl]).max() > 0 for _, sl in sls[:-1])              # no tensor compares zero with zero


@pytest.mark.parametrize('idx_mode', ('none', 'perm', 'repeats'))
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('leak', LEAKS)
@pytest.mark.parametrize('in_dim', IN_DIMS)
def test_gradient_parity(in_dim, leak, mode, count, idx_mode):
    idx_np, rows = index_rows(idx_mode, count, 100 * count + len(idx_mode))
    if idx_mode == 'repeats' and count > 1:
        assert len(set(rows.tolist())) < count
    run_parity(in_dim, leak, mode, idx_np, rows, count, 'in %d leak %.1f mode %d count %3d idx %-7s' % (in_dim, leak, mode, count, idx_mode))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('leak', LEAKS)
@pytest.mark.parametrize('in_dim', IN_DIMS)
def test_gradient_parity_several_tiles_per_workgroup(in_dim, leak, mode):
    rows = np.random.RandomState(33).randint(0, N_ROWS, size=MANY_TILES)
    run_parity(in_dim, leak, mode, rows, rows, MANY_TILES, 'in %d leak %.1f mode %d count %d idx repeats' % (in_dim, leak, mode, MANY_TILES))


# ---- bit-level behaviour ----
def test_equal_calls_give_equal_bits_and_no_weight_is_weight_one():
    torch = torch_()
    fx, d, _ = fixture(9, 0.2)
    q = loss_params()
    idx = torch.tensor(index_rows('repeats', 257, 5)[0], device=DEV)
    call = lambda w: TR.allocation_grad(d['theta'], d['x'], d['tau'], q, weight=w, idx=idx)
    none, ones = call(None), call(torch.ones(N_ROWS, device=DEV))
    assert torch.equal(none.view(torch.int32), ones.view(torch.int32))
    a, b = call(d['weight']), call(d['weight'])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, none)
    assert bool(torch.isfinite(a).all()) and bool(a.abs().max() > 0)
    other = TR.allocation_grad(d['theta'], d['x'], d['tau'], loss_params(w_power=0.05), weight=d['weight'], idx=idx)
    assert not torch.equal(a, other)                             # the loss's numbers reach the kernel


def test_stop_flag_and_the_kernels_that_share_the_workspace():
    """A set stop_flag leaves grad_out and the workspace as they were; dpenv_imitation_grad(mse) and dpenv_ppo_actor_grad return the bits
    they returned before an allocation call went through their workspace, and the allocation call is not disturbed by theirs."""
    torch = torch_()
    fx, d, _ = fixture(9, 0.2)
    q = loss_params()
    pf = F.make_fixture(N_ROWS, 0.2)
    pd = {k: torch.tensor(pf[k], device=DEV) for k in ('pi_theta', 'obs', 'act', 'adv', 'logp_old')}
    P, P7 = TR.layout(9, 6, True)['P'], TR.layout(9, 7, True)['P']
    ws = torch.full((TR.workspace_bytes(TR.make_shape(9, 7, True), 257) // 4,), 7.0, device=DEV)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    out = torch.full((P + 4,), 7.0, device=DEV)
    ppo = lambda: TR.ppo_actor_grad(pd['pi_theta'], pd['obs'], pd['act'], pd['adv'], pd['logp_old'], F.CLIP, workspace=ws, count=257).clone()
    imi = lambda: TR.imitation_grad(pd['pi_theta'], pd['obs'], pd['act'], loss='mse', workspace=ws, count=257).clone()
    TR.allocation_grad(d['theta'], d['x'], d['tau'], q, weight=d['weight'], out=out, workspace=ws, stop_flag=flag, count=257)
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    before = (ppo(), imi())
    assert before[0].numel() == P7 + 4
    flag.zero_()
    TR.allocation_grad(d['theta'], d['x'], d['tau'], q, weight=d['weight'], out=out, workspace=ws, stop_flag=flag, count=257)
    assert bool((out != 7.0).any()) and bool(torch.isfinite(out).all())
    after = (ppo(), imi())
    assert torch.equal(before[0].view(torch.int32), after[0].view(torch.int32)) and torch.equal(before[1].view(torch.int32), after[1].view(torch.int32))
    fresh = TR.allocation_grad(d['theta'], d['x'], d['tau'], q, weight=d['weight'], count=257)
    assert torch.equal(out.view(torch.int32), fresh.view(torch.int32))


def test_step_in_a_graph_equals_eager():
    """Gradient, reduction and ungated Adam of one allocation step captured with torch.cuda.graph (a chain on one stream: no parallel
    branches) and replayed, against the same calls made eagerly from the same state.  The first call is made outside the capture."""
    torch = torch_()
    fx, d, _ = fixture(9, 0.2)
    q = loss_params()
    P = TR.layout(9, 6, True)['P']
    sh = TR.make_shape(9, 6, True)

    def state():
        return dict(theta=d['theta'].clone(), m=torch.zeros(P, device=DEV), v=torch.zeros(P, device=DEV), grad=torch.zeros(P + 4, device=DEV),
                    ctr=torch.zeros(1, dtype=torch.int32, device=DEV), ws=torch.empty(TR.workspace_bytes(sh, 257) // 4, device=DEV))

    def step(s):
        TR.allocation_grad(s['theta'], d['x'], d['tau'], q, weight=d['weight'], out=s['grad'], workspace=s['ws'], count=257)
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
    assert int(eager['ctr']) == 2 and not torch.equal(eager['theta'], d['theta'])


# ---- the fit, and the fitted network in the closed loop ----
_fit = {}


def fitted():
    if not _fit:
        ds = deploy.nn_allocator_dataset(FIT['rows'], FIT['seed'])
        _fit['ds'] = ds
        _fit['net'] = TR.fit_nn_allocator(ds, iters=FIT['iters'], loss='wrench', alloc_loss=dict(w_power=FIT['w_power']), device=DEV)
    return _fit['ds'], _fit['net']


def test_wrench_fit_reduces_the_wrench_residual():
    ds, net = fitted()
    print('device fit: mean Js %.2f -> %.2f N^2 (x %.3f), J %.2f -> %.2f' % (
        net['wrench_ms_initial'], net['wrench_ms_final'], net['wrench_ms_final'] / net['wrench_ms_initial'], net['J_initial'], net['J_final']))
    assert net['loss'] == 'wrench' and 200.0 < net['wrench_ms_initial'] < 400.0
    assert net['wrench_ms_final'] <= FIT['cap'] * net['wrench_ms_initial'], (net['wrench_ms_initial'], net['wrench_ms_final'])
    assert net['J_final'] < net['J_initial'] and np.isfinite(net['mse_final'])


def test_mse_fit_is_unchanged_by_the_new_arguments():
    torch = torch_()
    ds = deploy.nn_allocator_dataset(FIT['rows'], FIT['seed'])
    a = TR.fit_nn_allocator(ds, iters=20, device=DEV)
    b = TR.fit_nn_allocator(ds, iters=20, device=DEV, loss='mse', alloc_loss=dict(w_power=0.05))
    assert torch.equal(a['theta'].view(torch.int32), b['theta'].view(torch.int32))
    assert a['loss'] == 'mse' and a['mse_initial'] == b['mse_initial'] and a['mse_final'] == b['mse_final'] and a['mse_final'] < a['mse_initial']
    # ... and equal to the loop as it was: the imitation gradient and the Adam step on the same start and minibatches
    theta = torch.as_tensor(TR.nn_allocator_init(9, 0)).to(DEV)
    P = theta.numel()
    x, y = torch.as_tensor(ds['x']).to(DEV), torch.as_tensor(ds['y']).to(DEV)
    m, v, step = torch.zeros(P, device=DEV), torch.zeros(P, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    idx = TR.nn_allocator_minibatches(FIT['rows'], 256, 20, 0).to(torch.int32).to(DEV)
    for it in range(20):
        g = TR.imitation_grad(theta, x, y, loss='mse', idx=idx[it], count=256)
        TR.adam_step(theta, g, m, v, step, 1e-3)
    assert torch.equal(theta.view(torch.int32), a['theta'].view(torch.int32))


def test_fitted_network_flies_and_the_loss_is_the_flown_laws():
    """64 envs, T = 5 with the fitted network behind the baseline's PID: every row finite.  Then the kernel's mean Js on the dataset's rows
    against the float64 Js of the outputs the DEPLOYED kernel (policy.thrust_alloc_nn, raw) gives for the same wrenches."""
    torch = torch_()
    import ml4ca_amd
    from ml4ca_amd.policy import controller_rollout, thrust_alloc_nn
    ds, net = fitted()
    env = ml4ca_amd.BatchedRevoltEnv(64, auto_reset=True, seed=4, device=DEV)
    env.set_dp_controller()
    env.set_nn_allocator(net)
    env.reset()
    o = controller_rollout(env, 5)
    for k in ('obs', 'act', 'rew'):
        assert bool(torch.isfinite(o[k].float()).all()), k
    assert tuple(o['act'].shape) == (5, 64, 7) and bool(o['act'][..., :3].abs().max() <= 1.0)
    q = TR.alloc_loss_params(dict(w_power=FIT['w_power']))
    n = FIT['rows']
    tau32 = ds['tau'].astype(np.float32)
    tau_dev = torch.as_tensor(np.ascontiguousarray(tau32.T)).to(DEV)
    _, raw = thrust_alloc_nn(tau_dev, net, raw=True)
    js = TR.alloc_loss_terms(raw.cpu().numpy().astype(np.float64), tau32, q)
    want = float(js['Js'].mean())
    tau6 = torch.as_tensor(np.concatenate([tau32, np.zeros_like(tau32)], 1)).to(DEV)
    out = TR.allocation_grad(net['theta'], torch.as_tensor(ds['x']).to(DEV), tau6, q)
    got = float(out[net['theta'].numel() + 1])
    bound = chain_K(n) * 2.0 ** -24 * float(js['Js'].max())
    print('mean Js: allocation_grad %.6f  deployed outputs in float64 %.6f  |diff| %.3e  bound %.3e' % (got, want, abs(got - want), bound))
    assert got == net["wrench_ms_final"]                         # equal inputs, equal bits: the figure the fit reported
    assert abs(got - want) <= bound, (got, want, bound)
