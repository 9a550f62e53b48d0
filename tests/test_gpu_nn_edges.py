"""The neural thrust allocator (dpenv_nn_law.h: nn_allocate, nn_pack_kernel, the host packer) and the allocation loss's per-row stage
(dpenv_train.hip: allocation_grad_kernel) on the GPU at the edges of their shapes and kinks, on the cases of tests/nn_edges.py, whose
fairness tests/test_nn_edges_cpu.py asserts without a GPU.

A. The allocator: the handle-free (in-place, clamped) form against the float32 host statement bit for bit at every width where the chunk
guard, the clamp and the last partial chunk decide what is computed; the same call on weights that are views in one NaN-filled block; the
closed loop (the zero-padded image, written by the packing kernel and by the host packer) against the handle-free call row by row at
those widths and with every constant away from its default; one handle's image re-packed from a large network to small ones and back;
weights scaled into, through and below the float32 subnormal range.
B. The allocation loss: the wire network of tests/nn_edges.py feeds the stage outputs p that sit exactly on its kinks; with count = 1 the
last bias slice of grad_out is the row's w * dL/dp and grad_out[P .. P+3] its w * (J, Js, Jp, Jx), each through one f64 partial rounded
once, i.e. the stage's own float32 values.  They are held to the header's exact statements (nn_edges.exact_properties), to
train.alloc_loss_terms in float64 under the running bound of nn_edges.alloc_law (derived there; the roundings of each chain are counted
in that module's docstring) and to the deployed law: dpenv_thrust_alloc_nn on the same wire and dpenv_thrust_map of its action.
Whole-gradient parity on rows of which every third sits on a kink: tests/test_gpu_allocation_loss.py's check_parity, against torch
float64 autograd and the float32 yardstick on ALL 130 rows: autograd's conventions at these kinks are the header's (clamp's bounds are
inclusive, d|n|/dn = 0 at n = 0 meets dF = 0, the relu slope at z = 0 is leak on both sides), which
tests/test_nn_edges_cpu.py::test_autograd_takes_the_headers_side_at_every_kink asserts against allocation_grad_ref - so the list of rows
that need allocation_grad_ref in autograd's place is empty, and no row is left out of anything."""
import numpy as np
import pytest

from ml4ca_amd import deploy
from ml4ca_amd import train as TR
from tests import helpers as H
from tests import nn_edges as NE
from tests.test_allocation_loss_cpu import torch_alloc_loss
from tests.test_gpu_allocation_loss import check_parity, stat_scales
from tests.test_gpu_nn_allocator import (N_FREE, NAN_LANE, INF_LANE, _act_rows_are_the_parts, _bits_equal, _check_against_host, _env, _np,
                                         _same, _start, free_tau)
from tests.test_imitation_cpu import slices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
N_LOOP, T_LOOP = 70, 3                                 # one full and one partial wave


def torch_():
    import torch
    return torch


def _only_bad():
    only = np.zeros(N_FREE, bool)
    only[[NAN_LANE, INF_LANE]] = True
    return only


# ---- A1: the handle-free form over the covering set ----
@pytest.mark.parametrize('case', NE.SHAPES, ids=NE.shape_id)
def test_handle_free_form_equals_the_host_statement_at_every_width(case):
    """n = 193 with the NaN and the inf lane: raw outputs and thrust entries bit for bit, heads within HEAD_TOL, the rest action exactly
    on the two bad lanes and nowhere else."""
    sizes, leak = case
    _, p, rest, fine, err = _check_against_host(NE.net_for(sizes), leak, free_tau(), want_rest=_only_bad())
    assert fine.sum() == N_FREE - 2 and np.abs(p[fine]).max() > 0
    print('sizes %s leak %g: largest head error %.3g' % (sizes, leak, err))


@pytest.mark.parametrize('name', sorted(NE.CONSTANTS))
@pytest.mark.parametrize('sizes', NE.CONSTANT_SHAPES)
def test_handle_free_form_with_every_constant_away_from_its_default(sizes, name):
    c = dict(NE.CONSTANTS[name])
    leak, mode = c.pop('leak'), c.pop('azimuth_mode', 0)
    act, _, _, fine, err = _check_against_host(NE.net_for(sizes, scale=3.0), leak, free_tau(), mode=mode, want_rest=_only_bad(), **c)
    assert fine.sum() == N_FREE - 2
    if mode == 1:                                           # the fixed heads are those of the f32 azimuths, well outside +-pi
        a = np.asarray(c['azimuth'], F64).astype(F32).astype(F64)
        want = np.array([np.sin(a[0]), np.cos(a[0]), np.sin(a[1]), np.cos(a[1])])
        assert np.abs(act[fine][:, 3:7] - want).max() <= 9.2e-8 + 2.0 ** -24


# ---- A2: guard bands ----
@pytest.mark.parametrize('sizes', NE.GUARD_SHAPES)
def test_reads_stay_inside_the_arrays(sizes):
    """Every W[l] and b[l] a view inside one device vector with 17 NaN floats before, between and behind them: the outputs are, bit for
    bit, those of separately allocated arrays - a clamped or padded read that reached a result would show as NaN."""
    torch = torch_()
    from ml4ca_amd.policy import thrust_alloc_nn
    net = NE.net_for(sizes)
    block_np, views = NE.guarded(net)
    block = H.to_dev(block_np)
    parts = [block[o:o + int(np.prod(shape))].view(*shape) for o, shape in views]
    inside = dict(W=parts[0::2], b=parts[1::2])
    assert all(t.is_contiguous() and t.untyped_storage().data_ptr() == block.untyped_storage().data_ptr() for t in parts)
    tau = H.to_dev(np.ascontiguousarray(free_tau().T))
    for leak in (0.0, 0.2):
        a0, p0 = thrust_alloc_nn(tau, net, raw=True, leak=leak)
        a1, p1 = thrust_alloc_nn(tau, inside, raw=True, leak=leak)
        torch.cuda.synchronize()
        assert _bits_equal(_np(p1), _np(p0)) and _bits_equal(_np(a1), _np(a0))
        good = np.isfinite(free_tau()).all(1)
        assert np.isfinite(_np(p1)[good]).all() and np.isfinite(_np(a1)).all()
    assert bool(torch.isnan(block).sum() == block.numel() - sum(t.numel() for t in parts))      # nothing wrote the block


# ---- A3: the padded form in the closed loop ----
def _fly(sizes, leak, nn, constants=None, scale=3.0):
    from ml4ca_amd.policy import controller_rollout
    net = dict(NE.net_for(sizes, scale=scale), leak=leak)
    env = _start(_env(N_LOOP, max_ep_len=40), nn=nn, net=net, constants=constants)
    z0 = env.get_dp_controller_state().clone()
    out = {k: v.clone() for k, v in controller_rollout(env, T_LOOP).items()}
    return env, z0, out


@pytest.mark.parametrize('case', NE.LOOP_SHAPES, ids=NE.shape_id)
def test_closed_loop_equals_the_handle_free_call_at_every_width(case):
    """n = 70, T = 3: every act row is the handle-free call on the host PID's wrench, bit for bit, with the image written by the packing
    kernel; the image the host packer writes from NumPy arrays flies the same rows."""
    torch = torch_()
    sizes, leak = case
    env, z0, out = _fly(sizes, leak, True)
    assert bool(torch.isfinite(out['act']).all()) and bool(out['act'][..., 0:3].abs().max() > 0)
    _act_rows_are_the_parts(env, out, z0)
    host, _, out_h = _fly(sizes, leak, 'host')
    assert isinstance(host.nn_allocator['net']['W'][0], np.ndarray) and not isinstance(env.nn_allocator['net']['W'][0], np.ndarray)
    _same(out, out_h, what='host packer %s' % (sizes,))


@pytest.mark.parametrize('name', sorted(NE.CONSTANTS))
@pytest.mark.parametrize('sizes', NE.CONSTANT_SHAPES)
def test_closed_loop_with_every_constant_away_from_its_default(sizes, name):
    torch = torch_()
    c = dict(NE.CONSTANTS[name])
    leak = c.pop('leak')
    env, z0, out = _fly(sizes, leak, True, constants=c)
    assert bool(torch.isfinite(out['act']).all())
    _act_rows_are_the_parts(env, out, z0)
    _, _, out_h = _fly(sizes, leak, 'host', constants=c)
    _same(out, out_h, what='host packer %s %s' % (sizes, name))
    _, _, plain = _fly(sizes, leak, True)
    assert not torch.equal(plain['act'], out['act'])                                      # the constants reach the kernel
    for k in c:                                                                           # ... each of them
        if (k == 'in_const' and sizes[0] == 3) or k == 'azimuth_mode':
            continue
        less = dict(c)
        less.pop(k)
        assert not torch.equal(_fly(sizes, leak, True, constants=less)[2]['act'], out['act']), k


# ---- A4: one image, many shapes ----
@pytest.mark.parametrize('order', ('down', 'up'))
def test_one_image_repacked_flies_what_a_fresh_handle_flies(order):
    """9-96-96-96-96-6, then 3-1-6, then 9-17-17-6 set on ONE handle (and once in the reverse order), each from device tensors and then
    from NumPy arrays; every flight starts from the same saved state and equals, bit for bit, the flight of a handle that only ever saw
    that network."""
    torch = torch_()
    from ml4ca_amd.policy import controller_rollout, nn_net_to
    shapes = NE.IMAGE_ORDER if order == 'down' else NE.IMAGE_ORDER[::-1]
    for nn in (True, 'host'):
        one = _start(_env(N_LOOP, max_ep_len=40), nn=False)
        state, ctr = (t.clone() for t in one.get_state())
        z0 = one.get_dp_controller_state().clone()
        seen = []
        for sizes in shapes:
            net = dict(NE.net_for(sizes, scale=3.0), leak=0.2)
            put = lambda env: env.set_nn_allocator(net if nn == 'host' else nn_net_to(net, env.device))
            fresh = _start(_env(N_LOOP, max_ep_len=40), nn=False)
            flights = []
            for env in (one, fresh):
                put(env)
                env.set_state(state, ctr)
                env.set_dp_controller_state(z0)
                flights.append({k: v.clone() for k, v in controller_rollout(env, T_LOOP).items()})
            _same(flights[0], flights[1], what='%s after %s' % (sizes, seen))
            assert bool(torch.isfinite(flights[0]['act']).all())
            assert all(not torch.equal(flights[0]['act'], a) for a in seen)
            seen.append(flights[0]['act'])


# ---- A5: the subnormal range ----
@pytest.mark.parametrize('kind', sorted(NE.SUB_SCALES))
@pytest.mark.parametrize('sizes', NE.SUB_SHAPES)
def test_subnormal_activations_are_ieee(sizes, kind):
    """The header states the law as IEEE fmaf in plain f32: weights that put activations and outputs into the subnormal range, and
    below it, give the host statement's bits (tests/test_nn_edges_cpu.py: the host values are subnormal and _fma32 is exact there)."""
    _, p, rest, fine, _ = _check_against_host(NE.subnormal_net(sizes, kind), NE.SUB_LEAK, free_tau(), want_rest=_only_bad())
    tiny = np.abs(p[fine])
    if kind == 'zero':
        assert not tiny.any()
    else:
        assert ((tiny > 0) & (tiny < NE.TINY)).sum() > tiny.size // 10


# ---- B: the allocation loss at its kinks ----
_case = {}


def case_data():
    """The case rows, their tau and weight variants and the wire, on the device (built once, never changed)."""
    if not _case:
        torch = torch_()
        names, P = NE.case_rows()
        R = len(names)
        rng = np.random.RandomState(3)
        _case.update(names=names, P=P, theta=torch.tensor(NE.wire_theta(), device=DEV), x=torch.tensor(NE.wire_x(P), device=DEV),
                     idx=torch.arange(R, dtype=torch.int32, device=DEV), taus={}, weights={None: None})
        for k, t in NE.tau_cases().items():                 # columns 3..5 may hold anything
            _case['taus'][k] = torch.tensor(np.concatenate([np.broadcast_to(t, (R, 3)), rng.normal(size=(R, 3)).astype(F32)], 1), device=DEV)
        for w in (2.0, 0.0):
            _case['weights'][w] = torch.full((R,), w, device=DEV)
    return _case


def launch(cfg, r, **over):
    """One row, count = 1: grad_out [P + 4] on the device"""
    d = case_data()
    c, q = NE.config(cfg)
    q = dict(q, **over)
    return TR.allocation_grad(d['theta'], d['x'], d['taus'][c['tau']], q, weight=d['weights'][c['weight']], idx=d['idx'][r:r + 1], leak=0.0, count=1)


_rows = {}


def stage_rows():
    """{(config, row): grad_out [P + 4] float32} of every launch of nn_edges.launches(), made once"""
    if not _rows:
        torch = torch_()
        outs = {k: launch(*k) for k in NE.launches()}
        torch.cuda.synchronize()
        _rows.update({k: v.cpu().numpy() for k, v in outs.items()})
    return _rows


def _dp_and_stats(out):
    L = TR.layout(9, 6, True)
    return out[L['b'][3]:L['b'][3] + 6], out[L['P']:L['P'] + 4]


def test_stage_holds_the_headers_exact_statements_at_every_kink():
    rows = stage_rows()
    assert len(rows) == len(NE.launches())
    NE.exact_properties({k: _dp_and_stats(v) for k, v in rows.items()})
    ls = slices(9, 6)[-1][1]
    for (cfg, r), out in rows.items():
        assert out.shape == (TR.layout(9, 6, True)['P'] + 4,) and np.isfinite(out).all()
        assert not out[ls].view(np.uint32).any()                                          # the log_std slice is +0.0
        if cfg == 'w0':
            assert not out.any(), (cfg, NE.case_rows()[0][r])                             # the WHOLE gradient and the statistics


def test_stage_against_float64_under_the_running_bound():
    """Every launch: w * dL/dp and the four statistics against train.alloc_loss_terms in float64 at the same f32 p and tau, element by
    element under nn_edges.alloc_law's running bound.  p is exact, so the reference takes the stage's branch at every kink: nothing is
    masked and no row is left out.  The largest share of the bound used is printed per configuration and quantity (DESIGN.md section 4
    records one MI355X run)."""
    d = case_data()
    rows = stage_rows()
    taus = NE.tau_cases()
    worst = dict.fromkeys(NE.QUANTITIES, 0.0)
    failed = []
    for cfg in NE.CONFIGS:
        c, q = NE.config(cfg)
        rs = [r for k, r in NE.launches() if k == cfg]
        got = [_dp_and_stats(rows[(cfg, r)]) for r in rs]
        w = None if c['weight'] is None else np.full(len(rs), c['weight'], F32)
        share, ok = NE.shares(np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), d['P'][rs], np.broadcast_to(taus[c['tau']], (len(rs), 3)), q, w)
        print('%-7s %s' % (cfg, ', '.join('%s %.3f' % kv for kv in share.items())))
        for k in share:
            worst[k] = max(worst[k], share[k])
        failed += [(cfg, d['names'][rs[i]], int(j)) for i, j in zip(*np.nonzero(~ok))]
    print('largest share of the running bound: ' + ', '.join('%s %.3f' % kv for kv in worst.items()))
    assert not failed, failed


def test_stage_is_the_deployed_law_at_the_kinks():
    """The same wire as the deployed allocator's network, the row's six outputs as its in_const (one call per row), mode 0: the raw output
    of dpenv_thrust_alloc_nn is p bit for bit (a zero of either sign for a zero), and dpenv_thrust_map of its action, minus tau, agrees
    with the stage's residual on the default hull - |r_m| = sqrt(Js) at w_slack = e_m, one launch per component - within the bound
    tests/test_gpu_nn_allocator.py::test_fit_lowers_the_loss_and_flies_the_box_test states for the thrust map."""
    torch = torch_()
    from ml4ca_amd.env import thrust_map
    from ml4ca_amd.policy import nn_net_to, thrust_alloc_nn
    d = case_data()
    R = len(d['names'])
    net = nn_net_to(NE.wire_net(), DEV)
    tau = NE.tau_cases()['interior']
    hull = deploy.alloc_loss_defaults()                     # dpenv_thrust_map flies the default hull: its kr, not the cases' 0.7 kf
    tau_dev = H.to_dev(tau.reshape(3, 1))
    acts, raws = torch.empty((R, 7), device=DEV), torch.empty((R, 6), device=DEV)
    js = []
    for r in range(R):
        thrust_alloc_nn(tau_dev, net, out=(acts[r:r + 1], raws[r:r + 1]), raw=True, leak=0.0, in_const=[float(v) for v in d['P'][r]])
        js.append([launch('base', r, w_slack=np.eye(3)[m], kr=hull['kr']) for m in range(3)])
    torch.cuda.synchronize()
    raw, act = _np(raws), _np(acts)
    same = (raw.view(np.uint32) == d['P'].view(np.uint32)) | ((raw == 0) & (d['P'] == 0))
    assert same.all(), [(d['names'][i], NE.P_NAMES[j]) for i, j in zip(*np.nonzero(~same))]
    assert np.array_equal(act[:, [1, 2, 0]], np.clip(d['P'][:, :3], -1, 1))
    alpha = np.stack([np.full(R, np.pi / 2), np.arctan2(act[:, 3], act[:, 4]), np.arctan2(act[:, 5], act[:, 6])]).astype(F32)
    flown = _np(thrust_map(H.to_dev((F32(100.0) * act[:, :3]).T), H.to_dev(alpha))).astype(F64) - tau.astype(F64)[:, None]
    stage = np.sqrt(np.array([[float(_dp_and_stats(o.cpu().numpy())[1][1]) for o in three] for three in js], F64)).T
    bound = (32 * 2.0 ** -24 + 2e-7) * 90.0
    diff = np.abs(np.abs(flown) - stage)
    print('|thrust map of the flown action - tau| against the stage\'s |r|: largest difference %.3g (bound %.3g), largest |r| %.3g' % (
        diff.max(), bound, stage.max()))
    assert diff.max() <= bound, [(d['names'][i], m) for m, i in zip(*np.nonzero(diff > bound))]
    assert stage.max() > 10.0                                                             # (residuals of tens of newtons: the agreement says something)


# ---- B2: the whole gradient on kink rows ----
@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('count', NE.B2_COUNTS)
def test_whole_gradient_parity_on_kink_rows(count, mode):
    """130 rows through the wire, rows 0, 3, 6, ... on kinks; count 1, 65 and 130 under check_parity's bound, all tensors and statistics
    against float64 autograd with the float32 yardstick, no row left out (the module docstring says why none needs another reference);
    the NaN-filled columns 3..5 of the target change no bit."""
    torch = torch_()
    fx = NE.kink_fixture()
    q = NE.loss_params(mode)
    rows = np.arange(count)
    dev = {k: torch.tensor(fx[k], device=DEV) for k in ('theta', 'x', 'tau', 'weight')}
    tau_nan = dev['tau'].clone()
    tau_nan[:, 3:] = float('nan')
    assert fx['kinks'][rows].any()
    for tag, w_np, w_dev in (('w none', None, None), ('w rand', fx['weight'], dev['weight'])):
        ref64, ref32 = (torch_alloc_loss(fx['theta'], fx['x'], fx['tau'], q, weight=w_np, rows=rows, leak=0.0, dtype=dt) for dt in (torch.float64, torch.float32))
        out = TR.allocation_grad(dev['theta'], dev['x'], dev['tau'], q, weight=w_dev, leak=0.0, count=count)
        out_nan = TR.allocation_grad(dev['theta'], dev['x'], tau_nan, q, weight=w_dev, leak=0.0, count=count)
        assert torch.equal(out.view(torch.int32), out_nan.view(torch.int32))
        check_parity('wire mode %d count %3d %s' % (mode, count, tag), out.cpu().numpy(), ref64, ref32, slices(9, 6), count, stat_scales(fx, rows, q, w_np))
        g, s = TR.allocation_grad_ref(fx['theta'], fx['x'][rows], fx['tau'][rows], q, weight=None if w_np is None else w_np[rows], leak=0.0)
        assert np.abs(g - ref64[0]).max() <= 1e-10 * np.abs(ref64[0]).max() and np.abs(s - ref64[1]).max() <= 1e-10 * np.abs(ref64[1]).max()
