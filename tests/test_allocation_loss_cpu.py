"""The allocation loss's host statement (ml4ca_amd/train.py: allocation_grad_ref, alloc_loss_terms) against torch float64 autograd of the
loss written out in torch through the thrust map, what the loss means against the deployed neural allocator and thrust_map_host, the
argument validation of dpenv_allocation_grad (a refused call launches nothing, so it needs no GPU), and the fitting condition the GPU
test uses, on the host.  The fixture (alloc_fixture) and the torch statement (torch_alloc_loss) are shared with
tests/test_gpu_allocation_loss.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ml4ca_amd import _lib, deploy
from ml4ca_amd import train as TR
from tests import ppo_fixture as F
from tests.test_imitation_cpu import make_weights, rel_errors, slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAKS = (0.2, 0.0)
IN_DIMS = (9, 3)
MODES = (0, 1)
P_MARGIN = 1e-3                                        # |p_j|, j < 3, stays this far from the clip's kink at 1 and from the thrust law's at 0
TAU_MAX = np.array([69.0, 30.0, 80.0])
_fx = {}


def loss_params(mode=0, **over):
    """The default hull's numbers with kr = 0.7 kf (the default hull has kr == kf, which would hide a wrong astern branch)."""
    p = deploy.alloc_loss_defaults()
    p['kr'] = 0.7 * np.asarray(p['kf'], np.float64)
    p['azimuth_mode'] = mode
    p.update(over)
    return p


def _rows(rng, n, in_dim):
    tau = (rng.uniform(-1.0, 1.0, size=(n, 3)) * TAU_MAX).astype(np.float32)
    xs = (tau.astype(np.float64) * np.asarray(deploy.NN_TAU_SCALE)).astype(np.float32)
    x = xs if in_dim == 3 else np.concatenate([np.broadcast_to(np.asarray(deploy.NN_IN_CONST, np.float32), (n, 6)), xs], 1)
    return np.ascontiguousarray(x), np.concatenate([tau, rng.normal(size=(n, 3)).astype(np.float32)], 1)


def _offending(theta, x, in_dim, leak):
    _, _, _, _, zs, p = TR._forward64(theta, x, in_dim, 6, True, leak)
    bad = np.zeros(x.shape[0], bool)
    for z in zs:
        bad |= (np.abs(z) < F.Z_MARGIN).any(1)
    a = np.abs(p[:, :3])
    return bad | (np.abs(a - 1.0) < P_MARGIN).any(1) | (a < P_MARGIN).any(1), p


def alloc_fixture(in_dim, leak, n_rows=300, seed=41):
    """dict(theta [P], x [n, in], tau [n, 6] - columns 3..5 random, nothing may read them -, leak, in_dim), float32: glorot kernels, small
    biases, a log_std tail that is not zero, wrenches uniform inside the dataset's bounds.  The last layer is scaled until at least a
    tenth of the rows have a saturated thrust output and at least a tenth have none; rows within a margin of a kink are drawn again."""
    key = (in_dim, leak, n_rows, seed)
    if key in _fx:
        return _fx[key]
    rng = np.random.RandomState(seed)
    sizes = [in_dim, 80, 80, 80, 6]
    Ws, bs = [], []
    for i in range(4):
        lim = math.sqrt(6.0 / (sizes[i] + sizes[i + 1]))
        Ws.append(rng.uniform(-lim, lim, size=(sizes[i], sizes[i + 1])).astype(np.float32))
        bs.append(rng.uniform(-0.1, 0.1, size=sizes[i + 1]).astype(np.float32))
    ls = rng.uniform(-0.8, -0.2, size=6).astype(np.float32)
    x, tau = _rows(rng, n_rows, in_dim)
    for scale in (1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
        theta = TR.flatten(Ws[:3] + [(Ws[3] * np.float32(scale))], bs[:3] + [(bs[3] * np.float32(scale))], ls)
        p = TR._forward64(theta, x, in_dim, 6, True, leak)[5]
        sat = (np.abs(p[:, :3]) > 1.0).any(1).mean()
        if 0.2 <= sat <= 0.8:
            break
    else:
        raise AssertionError('no scale of the last layer saturates between a fifth and four fifths of the rows')
    for _ in range(50):
        bad, _ = _offending(theta, x, in_dim, leak)
        if not bad.any():
            break
        x[bad], tau[bad] = _rows(rng, int(bad.sum()), in_dim)
    else:
        raise AssertionError('the fixture keeps rows within the margins after 50 redraws')
    _fx[key] = dict(theta=theta, x=x, tau=tau, leak=float(leak), in_dim=in_dim)
    return _fx[key]


def torch_alloc_loss(theta, x, tau, params, weight=None, rows=None, leak=0.2, dtype=torch.float64, device='cpu'):
    """(grad [P], stats [4] = L, mean w Js, mean w Jp, mean w Jx) as NumPy float64 from torch autograd in `dtype` over the rows `rows` (an
    index array, repeats allowed; None = all): the network as ActorCritic._mlp writes it, the commands decoded as the deployed allocator
    decodes them, the wrench as B(alpha) F of the thrust map, the loss as the issue states it.  The numbers are the struct's: float32."""
    in_dim = x.shape[1]
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
    leaf = lambda a: T(a).requires_grad_(True)
    Ws, bs, ls = TR.unflatten(np.asarray(theta), in_dim, 6, True)
    Ws, bs, ls = [leaf(w) for w in Ws], [leaf(b) for b in bs], leaf(ls)
    h, t = T(x[rows]), T(np.asarray(tau)[rows][:, :3])
    w = torch.ones(len(rows), dtype=dtype, device=device) if weight is None else T(np.asarray(weight)[rows])
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = torch.nn.functional.leaky_relu(h @ W + b, leak)
    p = h @ Ws[-1] + bs[-1]
    kf, kr, lx, ly, ws = (T(f32(params[k])) for k in ('kf', 'kr', 'lx', 'ly', 'w_slack'))
    u = p[:, [2, 0, 1]]                                        # bow, port, star
    n = 100.0 * torch.clamp(u, -1.0, 1.0)
    Fo = torch.where(n >= 0, kf, kr) * n * n.abs()
    if int(params['azimuth_mode']) == 0:
        al = p[:, 3:5] * float(f32(params['angle_scale']))
    else:
        al = T(f32(params['azimuth'])).expand(len(rows), 2)
    alpha = torch.cat([torch.full((len(rows), 1), math.pi / 2, dtype=dtype, device=device), al], 1)
    # the bow thruster is pure sway: its column is (0, 1, lx_b), not (cos(pi / 2) = 6e-17, ..)
    cb = torch.cat([torch.zeros(len(rows), 1, dtype=dtype, device=device), torch.cos(alpha[:, 1:])], 1)
    sb = torch.cat([torch.ones(len(rows), 1, dtype=dtype, device=device), torch.sin(alpha[:, 1:])], 1)
    wrench = torch.stack([(cb * Fo).sum(1), (sb * Fo).sum(1), ((lx * sb - ly * cb) * Fo).sum(1)], 1)
    r = wrench - t
    Js = (ws * r * r).sum(1)
    Jp = (Fo.abs() ** 3).sum(1)
    Jx = (torch.clamp(u.abs() - 1.0, min=0.0) ** 2).sum(1)
    J = 0.5 * (Js + float(f32(params['w_power'])) * Jp + float(f32(params['w_sat'])) * Jx)
    L = (w * J).mean()
    L.backward()
    g = lambda q: (torch.zeros_like(q) if q.grad is None else q.grad).detach().double().cpu().numpy()
    grad = TR.flatten([g(q) for q in Ws], [g(q) for q in bs], g(ls))
    return grad, np.array([float(L.detach()), float((w * Js).mean().detach()), float((w * Jp).mean().detach()), float((w * Jx).mean().detach())])


@pytest.mark.parametrize('leak', LEAKS)
@pytest.mark.parametrize('in_dim', IN_DIMS)
def test_fixture_conditions(in_dim, leak):
    fx = alloc_fixture(in_dim, leak)
    q = loss_params()
    assert np.array_equal(np.asarray(q['kr']), 0.7 * np.asarray(q['kf'])) and (np.asarray(q['kf']) > 0).all()
    bad, p = _offending(fx['theta'], fx['x'], in_dim, leak)
    assert not bad.any()
    zs = TR._forward64(fx['theta'], fx['x'], in_dim, 6, True, leak)[4]
    assert min(float(np.abs(z).min()) for z in zs) >= F.Z_MARGIN
    a = np.abs(p[:, :3])
    assert np.abs(a - 1.0).min() >= P_MARGIN and a.min() >= P_MARGIN
    sat = (a > 1.0).any(1)
    assert sat.mean() >= 0.1 and (~sat).mean() >= 0.1
    assert (p[:, :3] < 0).any() and (p[:, :3] > 0).any()       # both branches of K_i
    assert fx['tau'].shape == (300, 6) and fx['x'].shape == (300, in_dim) and fx['theta'].shape == (TR.layout(in_dim, 6, True)['P'],)


@pytest.mark.parametrize('rows', ('all', 'repeats'))
@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('leak', LEAKS)
@pytest.mark.parametrize('in_dim', IN_DIMS)
def test_closed_form_equals_float64_autograd(in_dim, leak, mode, weighted, rows):
    fx = alloc_fixture(in_dim, leak)
    q = loss_params(mode)
    n = fx['x'].shape[0]
    w = make_weights(n) if weighted else None
    idx = None if rows == 'all' else np.random.RandomState(3).randint(0, n // 3, size=200)
    if idx is not None:
        assert len(set(idx.tolist())) < len(idx)
    sel = slice(None) if idx is None else idx
    g, s = TR.allocation_grad_ref(fx['theta'], fx['x'][sel], fx['tau'][sel], q, weight=None if w is None else w[sel], leak=leak)
    tg, ts = torch_alloc_loss(fx['theta'], fx['x'], fx['tau'], q, weight=w, rows=idx, leak=leak)
    sls = slices(in_dim, 6)
    assert g.shape == (TR.layout(in_dim, 6, True)['P'],) and s.shape == (4,)
    for name, err in rel_errors(g, tg, sls).items():
        assert err <= 1e-10, (name, err)
    assert np.abs(s - ts).max() <= 1e-10 * np.abs(ts).max()
    assert s[0] == pytest.approx(0.5 * (s[1] + float(np.float32(q['w_power'])) * s[2] + float(np.float32(q['w_sat'])) * s[3]), rel=1e-12)
    assert s[1] > 0 and s[2] > 0 and s[3] > 0
    ls = sls[-1][1]
    assert not g[ls].any() and not tg[ls].any()                 # the loss does not see log_std: exactly zero on both sides
    assert all(np.abs(tg[sl]).max() > 0 for name, sl in sls[:-1])
    # the angle outputs get a gradient in mode 0 and none in mode 1; a_bow never does
    L = TR.layout(in_dim, 6, True)
    gb3 = g[L['b'][3]:L['b'][3] + 6]
    assert gb3[5] == 0.0 and np.abs(gb3[:3]).min() > 0
    assert (np.abs(gb3[3:5]).min() > 0) if mode == 0 else (not gb3[3:5].any())
    if weighted:
        assert (w[sel] == 0).any() and (w[sel] > 0).any()


def test_zero_weights_give_zero_and_tau_columns_3_to_5_are_not_read():
    fx = alloc_fixture(9, 0.2)
    q = loss_params()
    g0, s0 = TR.allocation_grad_ref(fx['theta'], fx['x'], fx['tau'], q, weight=np.zeros(300, np.float32))
    assert not g0.any() and not s0.any()
    tau_nan = fx['tau'].copy()
    tau_nan[:, 3:] = np.nan
    a, b = TR.allocation_grad_ref(fx['theta'], fx['x'], fx['tau'], q), TR.allocation_grad_ref(fx['theta'], fx['x'], tau_nan, q)
    c = TR.allocation_grad_ref(fx['theta'], fx['x'], fx['tau'][:, :3], q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


# ---- the loss means what the deployed law does ----
def test_residual_is_the_deployed_allocators_wrench_error():
    """p from the deployed allocator's host statement in float64; its ACTION through thrust_map_host (100 x the thrust part, pi / 2 and
    atan2 of the heads) minus tau is the loss's residual r.  Default hull (thrust_map_host's), azimuth_mode 0, rows with |p| > 1."""
    fx = alloc_fixture(9, 0.2)
    n = fx['x'].shape[0]
    Ws, bs, _ = TR.unflatten(fx['theta'], 9, 6, True)
    net = dict(W=list(Ws), b=list(bs), leak=0.2)
    tau = fx['tau'][:, :3].astype(np.float64)
    act, p = deploy.BatchedNNAllocator(n, net, dtype=np.float64).allocate(tau, raw=True)
    assert (np.abs(p[:, :3]) > 1.0).any(1).mean() >= 0.1 and (np.abs(p[:, :3]) < 1.0).all(1).any()
    q = deploy.alloc_loss_defaults()
    assert int(q['azimuth_mode']) == 0
    alpha = np.stack([np.full(n, np.pi / 2), np.arctan2(act[:, 3], act[:, 4]), np.arctan2(act[:, 5], act[:, 6])])
    want = deploy.thrust_map_host(100.0 * act[:, :3].T, alpha).T - tau
    r = TR.alloc_loss_terms(p, tau, q)['r']
    assert np.abs(r - want).max() <= 1e-9, np.abs(r - want).max()
    # the network the loss evaluates is the deployed one: the same p from the loss's own forward pass on the dataset's inputs
    p_loss = TR._forward64(fx['theta'], fx['x'], 9, 6, True, 0.2)[5]
    assert np.abs(p_loss - p).max() <= 1e-6                      # x is tau * tau_scale rounded to float32 here, formed in float64 there
    # a swapped thruster order or another angle scale is another wrench
    assert np.abs(TR.alloc_loss_terms(p[:, [1, 2, 0, 3, 4, 5]], tau, q)['r'] - want).max() > 1.0
    assert np.abs(TR.alloc_loss_terms(p[:, [0, 1, 2, 4, 3, 5]], tau, q)['r'] - want).max() > 1e-2
    assert np.abs(TR.alloc_loss_terms(p, tau, dict(q, angle_scale=1.0))['r'] - want).max() > 1.0


# ---- the C entry point's validation: refused before any device call, so this runs without a GPU ----
def test_defaults_match_and_struct_layout(tmp_path):
    lib = _lib.load()
    q = _lib.AllocLoss()
    assert lib.dpenv_alloc_loss_defaults(C.byref(q)) == _lib.OK
    assert lib.dpenv_alloc_loss_defaults(None) == _lib.EINVAL
    d = deploy.alloc_loss_defaults()
    assert q.struct_size == C.sizeof(_lib.AllocLoss)
    for k in ('w_slack', 'lx', 'ly', 'kf', 'kr', 'azimuth'):
        assert np.array_equal(np.array(getattr(q, k)[:], np.float32), np.asarray(d[k], np.float64).astype(np.float32)), k
    for k in ('w_power', 'w_sat', 'angle_scale'):
        assert np.float32(getattr(q, k)) == np.float32(d[k]), k
    assert q.azimuth_mode == d['azimuth_mode'] == 0 and q.w_sat == 100.0 and q.w_power == 1.0 and list(q.w_slack) == [1.0, 1.0, 1.0]
    qp, nn = deploy.qp_allocator_defaults(), deploy.nn_allocator_defaults()
    assert np.array_equal(d['kf'], qp['kf']) and np.array_equal(d['lx'], qp['lx']) and d['angle_scale'] == nn['angle_scale']
    s = TR.alloc_loss_struct(dict(w_power=0.05))
    assert s.w_power == np.float32(0.05) and bytes(s)[:16] == bytes(q)[:16] and bytes(s)[20:] == bytes(q)[20:]
    with pytest.raises(ValueError):
        TR.alloc_loss_struct(dict(w_dalpha=0.25))
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(dpenv_alloc_loss), offsetof(dpenv_alloc_loss, w_sat),'
                   ' offsetof(dpenv_alloc_loss, kf), offsetof(dpenv_alloc_loss, azimuth_mode));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.AllocLoss), _lib.AllocLoss.w_sat.offset, _lib.AllocLoss.kf.offset, _lib.AllocLoss.azimuth_mode.offset]


def _shape(**kw):
    return TR.make_shape(kw.pop('in_dim', 9), kw.pop('out_dim', 6), kw.pop('actor', True), **kw)


def test_refusals_launch_nothing_and_name_the_field():
    lib = _lib.load()
    fake = C.c_void_p(4096)                                    # never dereferenced: every one of these calls is refused on the host
    good = _shape()

    def loss(**kw):
        q = TR.alloc_loss_struct(loss_params())
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(q, k)[v[0]] = v[1]
            else:
                setattr(q, k, v)
        return q

    def call(shape=good, q=None, theta=fake, x=fake, tau=fake, weight=None, idx=None, count=64, n_rows=64, out=fake, ws=fake, ws_bytes=1 << 20):
        q = loss() if q is None else q
        return lib.dpenv_allocation_grad(C.byref(shape), None if q == 'null' else C.byref(q), theta, x, tau, weight, idx, count, n_rows, None, out,
                                         ws, ws_bytes, None)

    def refused(fn, word):
        assert fn() == _lib.EINVAL
        why = lib.dpenv_last_error(None)
        assert why and b'dpenv_allocation_grad' in why and word in why, (word, why)

    nan, inf = float('nan'), float('inf')
    refused(lambda: call(q=loss(struct_size=C.sizeof(_lib.AllocLoss) - 4)), b'struct_size')
    refused(lambda: call(q='null'), b'loss')
    refused(lambda: call(shape=_shape(out_dim=1, actor=False)), b'log_std')
    refused(lambda: call(shape=_shape(in_dim=6)), b'sizes[0]')
    refused(lambda: call(shape=_shape(in_dim=16)), b'sizes[0]')
    refused(lambda: call(shape=_shape(out_dim=7)), b'output width')
    refused(lambda: call(shape=_shape(out_dim=5)), b'output width')
    for k in range(3):
        refused(lambda: call(q=loss(w_slack=(k, -1.0))), b'w_slack')
        refused(lambda: call(q=loss(w_slack=(k, nan))), b'w_slack')
        refused(lambda: call(q=loss(lx=(k, inf))), b'lx')
        refused(lambda: call(q=loss(ly=(k, nan))), b'ly')
        refused(lambda: call(q=loss(kf=(k, 0.0))), b'kf')
        refused(lambda: call(q=loss(kf=(k, nan))), b'kf')
        refused(lambda: call(q=loss(kr=(k, -1e-3))), b'kr')
        refused(lambda: call(q=loss(kr=(k, inf))), b'kr')
    refused(lambda: call(q=loss(w_power=-0.5)), b'w_power')
    refused(lambda: call(q=loss(w_power=inf)), b'w_power')
    refused(lambda: call(q=loss(w_sat=-1.0)), b'w_sat')
    refused(lambda: call(q=loss(w_sat=nan)), b'w_sat')
    refused(lambda: call(q=loss(angle_scale=nan)), b'angle_scale')
    refused(lambda: call(q=loss(azimuth_mode=2)), b'azimuth_mode')
    refused(lambda: call(q=loss(azimuth_mode=-1)), b'azimuth_mode')
    refused(lambda: call(q=loss(azimuth=(1, inf))), b'azimuth')
    # ... and everything dpenv_imitation_grad refuses for the arguments they share
    refused(lambda: call(theta=None), b'theta')
    refused(lambda: call(x=None), b'x is NULL')
    refused(lambda: call(tau=None), b'tau_rows')
    refused(lambda: call(out=None), b'grad_out')
    refused(lambda: call(ws=None), b'workspace')
    refused(lambda: call(count=0), b'count')
    refused(lambda: call(count=-1), b'count')
    refused(lambda: call(count=2 ** 31 - 1, n_rows=2 ** 31 - 1, ws_bytes=1 << 40), b'at most')
    refused(lambda: call(idx=fake, count=8, n_rows=0), b'n_rows')
    refused(lambda: call(count=64, n_rows=32), b'n_rows')
    need = TR.workspace_bytes(good, 65)
    assert need == 2 * 4 * (TR.layout(9, 6, True)['P'] + 4)
    refused(lambda: call(count=65, n_rows=65, ws_bytes=need - 1), b'workspace')
    refused(lambda: call(shape=_shape(activation='tanh')), b'tanh')
    refused(lambda: call(shape=_shape(row_dtype=_lib.BF16)), b'bf16')
    refused(lambda: call(shape=_shape(hidden=(64, 64, 64))), b'80 wide')
    refused(lambda: call(shape=_shape(hidden=(80, 80))), b'n_layers')
    refused(lambda: call(shape=_shape(leak=1.5)), b'leak')


def test_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    assert re.search(r'^int dpenv_allocation_grad\(', header, re.M) and re.search(r'^int dpenv_alloc_loss_defaults\(', header, re.M)
    assert re.search(r'^#define DPENV_ABI_VERSION 6$', header, re.M)
    lib = _lib.load()
    assert hasattr(lib, 'dpenv_allocation_grad') and hasattr(lib, 'dpenv_alloc_loss_defaults')
    assert lib.dpenv_abi_version() == 6 == _lib.ABI_VERSION    # additive: the ABI number stays
    assert lib.dpenv_imitation_grad(C.byref(_shape(out_dim=7)), None, None, None, None, None, 64, 64, 2, None, None, None, 0, None) == _lib.EINVAL
    assert b'loss' in lib.dpenv_last_error(None)               # not a third code of the imitation entry point


def test_fit_refuses_an_unknown_loss():
    ds = deploy.nn_allocator_dataset(64, 0)
    with pytest.raises(ValueError, match='bogus'):
        TR.fit_nn_allocator(ds, iters=1, loss='bogus')
    with pytest.raises(ValueError):
        TR.alloc_loss_params(dict(w_bogus=1.0))
    assert TR.FIT_LOSSES == ('mse', 'wrench')


# ---- the condition tests/test_gpu_allocation_loss.py holds the device fit to, on the host ----
FIT = dict(rows=2048, seed=0, w_power=0.05, iters=300, minibatch=256, cap=0.25)


def test_host_fit_stays_inside_the_cap():
    """fit_nn_allocator(loss='wrench')'s loop on the host: the same start, the same minibatches, allocation_grad_ref (float64 arithmetic on
    the float32 parameters) + adam_step_ref (float32).  Mean Js over the whole dataset must fall to <= 0.25 of its start; plain torch float32
    runs of this condition reach x 0.08 - 0.09."""
    ds = deploy.nn_allocator_dataset(FIT['rows'], FIT['seed'])
    q = TR.alloc_loss_params(dict(w_power=FIT['w_power']))
    x, tau = ds['x'], ds['tau'].astype(np.float32)
    theta = TR.nn_allocator_init(9, FIT['seed'])
    P = theta.size
    m, v, step = np.zeros(P, np.float32), np.zeros(P, np.float32), 0
    idx = TR.nn_allocator_minibatches(FIT['rows'], FIT['minibatch'], FIT['iters'], FIT['seed']).numpy()
    js0 = TR.allocation_grad_ref(theta, x, tau, q)[1][1]
    for it in range(FIT['iters']):
        g = TR.allocation_grad_ref(theta, x[idx[it]], tau[idx[it]], q)[0]
        theta, m, v, step, _ = TR.adam_step_ref(theta, g, m, v, step, 1e-3)
    js1 = TR.allocation_grad_ref(theta, x, tau, q)[1][1]
    print('host fit: mean Js %.2f -> %.2f N^2 (x %.3f)' % (js0, js1, js1 / js0))
    assert step == FIT['iters'] and theta.dtype == np.float32
    assert 200.0 < js0 < 400.0
    assert js1 <= FIT['cap'] * js0, (js0, js1)
