"""dpenv_controller_label_qp_ex on the device (policy.controller_label_qp(flown=..., table=...)): the QP labelling scan with the thruster
state taken from the FLOWN action rows and / or one QP allocator per env.  With neither it is dpenv_controller_label_qp in bits; the flown
form is checked by its parts - labels and costs = dpenv_thrust_alloc_qp on the host PID's tau and the device's own thruster states, taken
from one-row calls - also on handles that cannot fly the QP; the device's S against the host statement; pieces, lanes, graph capture, an
untouched handle, the refusals; the table against the scalar call per row, refused rows; the objective by the float32 yardstick; and the
DAgger driver's thruster_state='flown' against the rounds made by hand."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_controller_label_qp import K, N, T, _bits, _np, _pinv_flight, _qp_flight
from tests.test_gpu_dp_controller_table import _same_state
from tests.test_gpu_qp_allocator import SHAPES, _env, _params, _start
from tests.test_gpu_qp_allocator_table import _sets, _table

pytestmark = pytest.mark.gpu

TL = 6                                # rows of the lane tests


def torch_():
    import torch
    return torch


@pytest.fixture(scope='module')
def flight():
    return _qp_flight()


@pytest.fixture(scope='module')
def foreign():
    return _pinv_flight()


def _raw_ex(env, obs, done, z=None, x=None, params=None, flown=None, table=None, iterations=0, refused=None, size=None, out=None, T_=None):
    """dpenv_controller_label_qp_ex as the C ABI takes it: (rc, message, (act, z_out, x_out, cost))."""
    from ml4ca_amd import _lib
    from ml4ca_amd.policy import qp_allocator_struct
    torch = torch_()
    Tb, n = obs.shape[0], obs.shape[1]
    if out is None:
        out = (torch.empty((Tb, n, 7), device=env.device), torch.empty((3, n), device=env.device), torch.empty((5, n), device=env.device),
               torch.empty((Tb, n), device=env.device))
    io = _lib.ControllerLabelQpExIO()
    io.struct_size = C.sizeof(io) if size is None else size
    io.T = Tb if T_ is None else T_
    io.obs, io.obs_dtype = obs.data_ptr(), 1 if obs.dtype == torch.bfloat16 else 0
    io.done = done.data_ptr() if done is not None else None
    io.z_in = z.data_ptr() if z is not None else None
    io.x_in = x.data_ptr() if x is not None else None
    io.act, io.z_out, io.x_out, io.cost = (t.data_ptr() for t in out)
    q = qp_allocator_struct(params) if params is not None else None
    io.q = C.pointer(q) if q is not None else None
    io.flown = flown.data_ptr() if flown is not None else None
    io.qp_table = table.data_ptr() if table is not None else None
    io.iterations = iterations
    io.refused_out = refused.data_ptr() if refused is not None else None
    rc = env.lib.dpenv_controller_label_qp_ex(env._h, C.byref(io), env._stream())
    return rc, env.lib.dpenv_last_error(env._h).decode(), out


# 1 ---- with neither flown rows nor a table the new entry point is the old one, bit for bit
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('which', ['qp', 'foreign'])
def test_ex_without_flown_rows_or_a_table_is_the_old_call_in_bits(which, bf16, flight, foreign):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    if which == 'qp':
        env, out, z0, x0 = flight
        p = None                                                                       # q = NULL: the handle's numbers
    else:
        env, out, z0, _ = foreign
        x0, p = None, _params(K)
    obs = out['obs'].to(torch.bfloat16) if bf16 else out['obs']
    want = controller_label_qp(env, obs, out['done'], z=z0, x=x0, params=p, cost=True)
    rc, msg, got = _raw_ex(env, obs, out['done'], z=z0, x=x0, params=p)
    assert rc == 0, msg
    for name, u, v in zip(('act', 'z_out', 'x_out'), got, want):
        assert _bits(u, v), name
    assert _bits(got[3], want[3]), 'cost'
    if which == 'qp' and not bf16:
        assert _bits(got[0], out['act'])                                               # ... which are the closed loop's own rows


# 2 ---- the flown form by its parts
def _device_states(env, out, z0, x0, params, flown, table=None, iterations=None):
    """One-row calls of the new entry point with z and x handed over: x_t [T][5, n] = the x_out of row t - 1 (x0 at t = 0), and the labels,
    costs, final z and x those calls gave."""
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    n = env.n_envs
    z = z0.clone()
    x = torch.zeros((5, n), device=env.device) if x0 is None else x0.clone()
    xs, acts, costs = [], [], []
    for t in range(out['obs'].shape[0]):
        xs.append(x.clone())
        a, z, x, J = controller_label_qp(env, out['obs'][t:t + 1].contiguous(), out['done'][t:t + 1].contiguous(), z=z, x=x, params=params,
                                         flown=flown[t:t + 1].contiguous(), table=table, iterations=iterations, cost=True)
        acts.append(a[0])
        costs.append(J[0])
    return torch.stack(xs), torch.stack(acts), torch.stack(costs), z, x


def _host_tau(env, out, z0, table=None):
    """The host PID's tau per row [T][3, n] on the device (NumPy float32, bit for bit the kernel's), z zeroed behind done rows; final z."""
    from ml4ca_amd.deploy import BatchedDPController
    n = env.n_envs
    ctrl = BatchedDPController(n, env.dp_controller if table is None else table, dt=env.control_period)
    ctrl.z = np.ascontiguousarray(_np(z0).T)
    obs, done = _np(out['obs'].float()), _np(out['done'])
    taus = []
    for t in range(obs.shape[0]):
        taus.append(np.ascontiguousarray(ctrl.wrench(obs[t]).T))
        ctrl.reset(done[t] != 0)
    return H.to_dev(np.array(taus), env.device), H.to_dev(np.ascontiguousarray(ctrl.z.T), env.device)


@pytest.mark.parametrize('kind', ['qp', 'shared', 'hulls', 'table'])
def test_flown_labels_are_the_allocator_on_the_devices_own_states_bit_for_bit(kind, flight, foreign):
    from ml4ca_amd.deploy import qp_state_from_action
    from ml4ca_amd.policy import controller_label_qp, thrust_alloc_qp
    torch = torch_()
    tab = None
    if kind == 'qp':
        env, out, z0, x0 = flight
    elif kind == 'shared':
        env, out, z0, _ = foreign
        x0 = None
    else:
        env, out, z0, tab = _pinv_flight(hulls=kind == 'hulls', table=kind == 'table')
        x0 = None
    p = _params(K)
    fl = out['act']
    act, z, x, J = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0, params=p, flown=fl, cost=True)
    xs, a1, J1, z1, x1 = _device_states(env, out, z0, x0, p, fl)
    assert _bits(act, a1) and _bits(J, J1) and _bits(z, z1) and _bits(x, x1)           # one-row pieces = one call
    taus, wz = _host_tau(env, out, z0, table=tab)
    for t in range(T):
        wa, _, wJ = thrust_alloc_qp(taus[t], xs[t], p, env.control_period, cost=True)
        assert _bits(act[t], wa), (t, int((act[t] != wa).sum()))
        assert _bits(J[t], wJ), t
    assert _bits(z, wz)
    # the states are S of the executed row (zero behind a done row), not the law's own advance
    done = _np(out['done'])
    S = np.stack([qp_state_from_action(p, _np(fl[t])) for t in range(T)])              # [T, n, 5]
    S[done != 0] = 0
    dev = np.concatenate([_np(xs[1:]), _np(x)[None]]).transpose(0, 2, 1)               # the state row t left
    assert np.array_equal(dev[..., 0:3].view(np.uint32), S[..., 0:3].view(np.uint32))
    d = np.abs((dev[..., 3:5].astype(np.float64) - S[..., 3:5] + np.pi) % (2 * np.pi) - np.pi)
    assert d.max() <= 1e-6
    own, _, x_own = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0, params=p)
    assert _bits(own[0], act[0]) and not _bits(own, act) and not _bits(x_own, x)
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(J).all())


# 3 ---- the device's S against the host statement
def test_state_from_action_on_the_device_against_the_host_statement():
    """x_out of a one-row call without a done byte is S(flown[0]).  Forces: the float32 host statement in bits (the same operations in
    the same order, no transcendental).  Azimuths: within 1e-6 rad on the circle of the float64 statement (atan2_lean's stated 2.6e-7 and
    two roundings at pi).  Entries that are not finite give 0, and labels from such states are finite."""
    state_from_action_against_the_host_statement(_params(K))


def state_from_action_against_the_host_statement(p):
    """The check of the test above for the QP numbers p (tests/test_gpu_qp_edges.py runs it on its asymmetric set)."""
    from ml4ca_amd.deploy import BatchedQPAllocator, qp_state_from_action
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    n = 130
    env = _start(_env(n), qp=False, nudge=False)
    rng = np.random.RandomState(7)
    a = rng.uniform(-1.3, 1.3, (TL, n, 7)).astype(np.float32)
    a[0, :, 3:7] *= rng.uniform(0.01, 30.0, (n, 1)).astype(np.float32)                 # heads of any length
    qp = BatchedQPAllocator(n, p, dt=env.control_period)
    xr = (rng.uniform(-1, 1, (n, 5)) * np.concatenate([np.asarray(p['f_max'], np.float64), [3.14, 3.14]])).astype(np.float32)
    s, c = np.sin(xr[:, 3:5]), np.cos(xr[:, 3:5])
    a[1] = np.concatenate([qp.thrust_columns(xr[:, 0:3]), np.stack([s[:, 0], c[:, 0], s[:, 1], c[:, 1]], 1)], 1)   # the law's own rows
    a[2, :, 0:3] = np.sign(a[2, :, 0:3]) * 1.5
    a[3, 0:7, :] = np.nan
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for col in range(7):
            a[3, 8 + 7 * k + col, col] = v
    a[4, 0:4, 3], a[4, 0:4, 4] = np.float32([0.0, -0.0, 0.0, -0.0]), np.float32([0.0, 0.0, -0.0, -0.0])
    a[4, 4:8, 5], a[4, 4:8, 6] = np.float32([0.0, -0.0, 0.0, -0.0]), np.float32([0.0, 0.0, -0.0, -0.0])
    obs = H.to_dev((rng.uniform(-1, 1, (TL, n, 9)) * (3, 3, 1, 0.5, 0.3, 0.2, 1, 1, 1)).astype(np.float32), env.device)
    fl = H.to_dev(a, env.device)
    for t in range(TL):
        _, _, x = controller_label_qp(env, obs[t:t + 1].contiguous(), None, params=p, flown=fl[t:t + 1].contiguous())
        got = _np(x).T
        h32, h64 = qp_state_from_action(p, a[t]), qp_state_from_action(p, a[t], dtype=np.float64)
        assert np.isfinite(got).all()
        assert np.array_equal(got[:, 0:3].view(np.uint32), h32[:, 0:3].view(np.uint32)), t
        d = np.abs((got[:, 3:5].astype(np.float64) - h64[:, 3:5] + np.pi) % (2 * np.pi) - np.pi)
        print('row %d: azimuth against the float64 statement, worst %.3g rad' % (t, d.max()))
        assert d.max() <= 1e-6, t
        assert ((h32 == 0) <= (got == 0)).all()                                        # what the host puts at rest is at rest
        assert (got[:, 3:5] >= -np.float32(np.pi)).all() and (got[:, 3:5] <= np.float32(np.pi)).all()
    assert (got[:, 0:3] != 0).all()
    x3 = qp_state_from_action(p, a[3])
    assert (x3[0:7] == 0).all()
    # the block in one call: every label finite, whatever was flown
    act, _, x, J = controller_label_qp(env, obs, None, params=p, flown=fl, cost=True)
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(J).all()) and bool(torch.isfinite(x).all())


# 4 ---- pieces and lanes on every shape, flown rows and a table together
def _synthetic(n, seed):
    rng = np.random.RandomState(seed)
    obs = (rng.uniform(-1, 1, (TL, n, 9)) * (5, 5, 1.2, 1, 0.5, 0.4, 1, 1, 1)).astype(np.float32)
    done = (rng.uniform(0, 1, (TL, n)) < 0.15).astype(np.uint8) * 3
    fl = rng.uniform(-1.1, 1.1, (TL, n, 7)).astype(np.float32)
    z0 = rng.uniform(-0.5, 0.5, (3, n)).astype(np.float32)
    x0 = (rng.uniform(-1, 1, (5, n)) * np.array([4, 8, 8, 2, 2])[:, None]).astype(np.float32)
    return obs, done, fl, z0, x0


@pytest.mark.parametrize('form', ['flown', 'table', 'both'])
@pytest.mark.parametrize('n', SHAPES)
def test_pieces_equal_one_call_and_lanes_do_not_mix(n, form):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env = _start(_env(n), qp=False, nudge=False)
    obs, done, fl, z0, x0 = (H.to_dev(v, env.device) for v in _synthetic(n, 30 + n))
    tab = H.to_dev(_table(n, K), env.device) if form != 'flown' else None
    kw = lambda sl, t=None: dict(params=_params(K) if tab is None else None, flown=fl[sl].contiguous() if form != 'table' else None,
                                 table=tab if t is None else t, iterations=K if tab is not None else None, cost=True)
    every = slice(0, TL)
    one = controller_label_qp(env, obs, done, z=z0, x=x0, **kw(every))
    assert all(bool(torch.isfinite(v).all()) for v in one)
    z, x = z0.clone(), x0.clone()
    a1 = torch.empty((2, n, 7), device=env.device)
    a2 = torch.empty((TL - 2, n, 7), device=env.device)
    J1 = controller_label_qp(env, obs[:2].contiguous(), done[:2].contiguous(), z=z, x=x, out=(a1, z, x), **kw(slice(0, 2)))[3]
    J2 = controller_label_qp(env, obs[2:].contiguous(), done[2:].contiguous(), z=z, x=x, out=(a2, z, x), **kw(slice(2, TL)))[3]
    assert _bits(torch.cat([a1, a2]), one[0]) and _bits(z, one[1]) and _bits(x, one[2]) and _bits(torch.cat([J1, J2]), one[3])
    if n == 1:
        return
    j, other = n - 1, 0                                                                # the last live lane takes lane 0's rows, state and numbers
    o2, d2, f2, z2, x2 = obs.clone(), done.clone(), fl.clone(), z0.clone(), x0.clone()
    o2[:, j], d2[:, j], f2[:, j], z2[:, j], x2[:, j] = obs[:, other], done[:, other], fl[:, other], z0[:, other], x0[:, other]
    t2 = None
    if tab is not None:
        t2 = tab.clone()
        t2[:, j] = tab[:, other]
    kw2 = dict(kw(every, t2), flown=f2 if form != 'table' else None)
    got = controller_label_qp(env, o2, d2, z=z2, x=x2, **kw2)
    keep = [i for i in range(n) if i != j]
    assert _bits(got[0][:, keep], one[0][:, keep]) and _bits(got[1][:, keep], one[1][:, keep]) and _bits(got[2][:, keep], one[2][:, keep])
    assert _bits(got[3][:, keep], one[3][:, keep])
    assert _bits(got[0][:, j], one[0][:, other]) and _bits(got[2][:, j], one[2][:, other]) and _bits(got[3][:, j], one[3][:, other])
    assert not _bits(got[0][:, j], one[0][:, j])
    if form != 'table':                                                                # row t ignores flown[t:], and depends on flown[t - 1]
        f3 = fl.clone()
        f3[3:] = fl[3:].flip(1) * 0.5
        late = controller_label_qp(env, obs, done, z=z0, x=x0, **dict(kw(every), flown=f3))
        assert _bits(late[0][:4], one[0][:4]) and (n < 3 or not _bits(late[0][4:], one[0][4:]))


# 5 ---- capture, the handle, the refusals
def test_captured_call_replays_like_eager_calls(foreign):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, src, _, _ = foreign
    tab = H.to_dev(_table(N, K), env.device)
    obs, done, fl = src['obs'].clone(), src['done'].clone(), src['act'].clone()
    z_in, x_in = torch.zeros((3, N), device=env.device), torch.zeros((5, N), device=env.device)
    ref = torch.zeros((N,), dtype=torch.uint8, device=env.device)
    kw = dict(z=z_in, x=x_in, flown=fl, table=tab, iterations=K, refused=ref)
    out = controller_label_qp(env, obs, done, **kw)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        controller_label_qp(env, obs, done, out=out, **kw)
    first = None
    for k in range(2):
        obs.copy_(src['obs'].flip(1) if k else src['obs'] * 0.5)
        done.copy_(src['done'].flip(1) if k else src['done'])
        fl.copy_(src['act'].flip(1) if k else src['act'] * 0.5)
        z_in.fill_(0.25 * k)
        x_in.fill_(0.5 * k)
        g.replay()
        eager = controller_label_qp(env, obs, done, **kw)
        torch.cuda.synchronize()
        assert all(_bits(u, v) for u, v in zip(out, eager)), 'replay %d' % k
        first = eager[0].clone() if first is None else first
    assert not _bits(out[0], first)


def test_labelling_leaves_the_handle_untouched(foreign):
    from ml4ca_amd.policy import controller_label_qp, controller_rollout
    torch = torch_()
    _, src, _, _ = foreign
    a, b = (_start(_env(N, auto_reset=True, terminate=True, max_ep_len=24, seed=11), K=K) for _ in range(2))
    h = T // 2
    controller_rollout(a, h), controller_rollout(b, h)
    tab = H.to_dev(_table(N, K), a.device)
    lab = controller_label_qp(a, src['obs'], src['done'], flown=src['act'])[0]         # the handle's own q
    lab2 = controller_label_qp(a, src['obs'], src['done'], flown=src['act'], table=tab, iterations=K)[0]
    assert bool(torch.isfinite(lab).all()) and not _bits(lab, lab2)
    _same_state(a, b)
    assert torch.equal(a.get_qp_allocator_state(), b.get_qp_allocator_state()) and bool(a.get_qp_allocator_state().any())
    oa, ob = controller_rollout(a, h), controller_rollout(b, h)
    assert all(torch.equal(oa[k], ob[k]) for k in ('obs', 'act', 'rew', 'done'))
    for u, v in zip(a.get_rng_counters(), b.get_rng_counters()):
        assert torch.equal(u, v)
    assert a.qp_allocator['iterations'] == K and a.qp_allocator_table is None


def test_refusals_touch_nothing_and_each_has_its_word(foreign):
    from ml4ca_amd import DpenvError, _lib
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    _, src, _, _ = foreign
    env = _env(N, auto_reset=True, terminate=True, max_ep_len=24)
    obs, done, fl = src['obs'], src['done'], src['act']
    out = (torch.full((T, N, 7), 7.5, device=env.device), torch.full((3, N), -3.5, device=env.device), torch.full((5, N), 1.25, device=env.device),
           torch.full((T, N), -9.0, device=env.device))
    ref = torch.full((N,), 9, dtype=torch.uint8, device=env.device)
    tab = H.to_dev(_table(N, K), env.device)
    good = _params(K)
    rc, msg, _ = _raw_ex(env, obs, done, params=good, flown=fl, out=out)
    assert rc == _lib.EINVAL and 'controller is off' in msg
    env.set_dp_controller()
    cases = ((dict(params=good, table=tab, iterations=K), 'not both'), (dict(params=good, refused=ref), 'refused_out'),
             (dict(table=tab, iterations=0), 'iterations'), (dict(table=tab, iterations=33), 'iterations'), (dict(flown=fl), 'no QP allocator'),
             (dict(), 'no QP allocator'), (dict(params=good, flown=fl, T_=0), 'T > 0'), (dict(params=good, flown=fl, size=C.sizeof(_lib.ControllerLabelQpIO)), 'ABI mismatch'),
             (dict(params=dict(good, iterations=40), flown=fl), 'iterations'), (dict(params=dict(good, w_dalpha=0.0), flown=fl), 'w_dalpha'))
    for kw, word in cases:
        rc, msg, _ = _raw_ex(env, obs, done, out=out, **kw)
        assert rc == _lib.EINVAL and word in msg, (kw.keys(), rc, msg)
    # a table in force on the handle and no numbers in the call: the message names q and qp_table
    flying = _start(_env(N, auto_reset=True, terminate=True, max_ep_len=24), qp=False, nudge=False)
    flying.set_qp_allocator_table(tab, iterations=K)
    rc, msg, _ = _raw_ex(flying, obs, done, flown=fl, out=out)
    assert rc == _lib.EINVAL and 'qp_table' in msg and 'pass q' in msg
    with pytest.raises(DpenvError, match='table'):
        controller_label_qp(flying, obs, done, flown=fl, out=out[:3])
    # the Python entry point's own checks
    for bad in (dict(flown=fl[:-1].contiguous()), dict(flown=fl.double()), dict(flown=fl.cpu()), dict(table=tab[:, :-1].contiguous(), params=None),
                dict(table=tab, params=good), dict(iterations=4), dict(refused=ref), dict(table=tab, params=None, refused=ref.float())):
        args = dict(params=good, flown=fl)
        args.update(bad)
        with pytest.raises(ValueError):
            controller_label_qp(env, obs, done, out=out[:3], **args)
    torch.cuda.synchronize()
    assert bool((out[0] == 7.5).all()) and bool((out[1] == -3.5).all()) and bool((out[2] == 1.25).all()) and bool((out[3] == -9.0).all())
    assert bool((ref == 9).all())
    # ... and the same arguments are served once nothing is wrong
    rc, msg, _ = _raw_ex(env, obs, done, flown=fl, table=tab, iterations=K, refused=ref, out=out)
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool(torch.isfinite(out[0]).all()) and not bool((out[0] == 7.5).any()) and not bool((out[3] == -9.0).any()) and not bool(ref.any())
    got = controller_label_qp(env, obs, done, flown=fl, table=tab, iterations=K)
    assert _bits(got[0], out[0]) and _bits(got[2], out[2])


# 6 ---- one QP allocator per env
@pytest.mark.parametrize('flown', [False, True])
def test_table_rows_are_the_scalar_call_per_row_and_refused_rows_rest(flown, foreign):
    from ml4ca_amd.deploy import QP_SLOTS, qp_allocator_table, qp_table_refused
    from ml4ca_amd.evaluate import qp_label_sweep
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, src, z0, _ = foreign
    obs, done = src['obs'], src['done']
    fl = src['act'] if flown else None
    sets = _sets(K)
    # equal rows give the scalar call's bits (without flown rows the scalar call is the OLD entry point)
    for s in (0, 2):
        eq = H.to_dev(qp_allocator_table(N, sets[s]), env.device)
        a = controller_label_qp(env, obs, done, z=z0, table=eq, iterations=K, flown=fl, cost=True)
        b = controller_label_qp(env, obs, done, z=z0, params=sets[s], flown=fl, cost=True)
        assert all(_bits(u, v) for u, v in zip(a, b)), s
    # distinct rows: lane i is the scalar call with row i's numbers (set i mod 4)
    tab_np = _table(N, K)
    tab = H.to_dev(tab_np, env.device)
    ref = torch.full((N,), 9, dtype=torch.uint8, device=env.device)
    d = controller_label_qp(env, obs, done, z=z0, table=tab, iterations=K, flown=fl, cost=True, refused=ref)
    assert not bool(ref.any())
    for s in range(4):
        e = controller_label_qp(env, obs, done, z=z0, params=sets[s], flown=fl, cost=True)
        assert _bits(d[0][:, s::4], e[0][:, s::4]) and _bits(d[2][:, s::4], e[2][:, s::4]) and _bits(d[3][:, s::4], e[3][:, s::4]), s
        assert _bits(d[1], e[1])                                                       # z does not see the allocator
    # another iteration count is another law
    d3 = controller_label_qp(env, obs, done, z=z0, table=tab, iterations=3, flown=fl)
    assert not _bits(d3[0], d[0])
    # refused rows: the rest allocator, NaN cost, their byte; the other lanes are not affected
    bad_np = tab_np.copy()
    bad_envs = (3, 63, 64, 65, N - 1)
    bad_np[QP_SLOTS['w_power'][0], 3] = np.nan
    bad_np[QP_SLOTS['w_dalpha'][0], 63] = 0.0
    bad_np[QP_SLOTS['f_max'][0] + 1, 64] = -1.0
    bad_np[QP_SLOTS['kf'][0] + 2, 65] = 0.0
    bad_np[QP_SLOTS['azimuth_rate'][0] + 1, N - 1] = -0.1
    bad_np[29, 5] = np.nan                                                             # a reserved slot: not read
    want = qp_table_refused(bad_np, env.control_period)
    assert sorted(np.nonzero(want)[0]) == sorted(bad_envs)
    g = controller_label_qp(env, obs, done, z=z0, table=H.to_dev(bad_np, env.device), iterations=K, flown=fl, cost=True, refused=ref)
    assert np.array_equal(_np(ref) != 0, want)
    ok = torch.from_numpy(~want).to(env.device)
    assert _bits(g[0][:, ok], d[0][:, ok]) and _bits(g[2][:, ok], d[2][:, ok]) and _bits(g[3][:, ok], d[3][:, ok]) and _bits(g[1], d[1])
    rest = _np(g[0][:, ~ok])
    assert (rest[..., 0:3] == 0).all() and np.isfinite(rest).all() and bool(torch.isnan(g[3][:, ~ok]).all()) and not bool(g[2][0:3][:, ~ok].any())
    if not flown:                                                                      # from rest and along the own recursion the azimuths are held at 0
        assert (rest[..., 3:7] == np.float32([0, 1, 0, 1])).all()
    else:
        # the sweep: K sets x m envs in one launch, the mean squared distance per set
        m = N // 4
        cols = np.stack([qp_allocator_table(1, s)[:, 0] for s in sets], 1)             # [32, 4]
        res = qp_label_sweep(env, src, cols, iterations=K)
        full = H.to_dev(np.repeat(cols, m, axis=1), env.device)
        lab = controller_label_qp(env, obs, done, flown=src['act'], table=full, iterations=K)[0]
        assert _bits(res['labels'], lab) and tuple(res['msd'].shape) == (4,) and not bool(res['refused'].any())
        by_hand = ((src['act'] - lab).double() ** 2).mean(2).mean(0).view(4, m).mean(1)
        assert torch.equal(res['msd'], by_hand) and len(set(res['msd'].tolist())) == 4
        with pytest.raises(ValueError):
            qp_label_sweep(env, src, cols[:, :3], iterations=K)                        # 3 does not divide 200


# 7 ---- the objective against the float64 host statement, from the device's own states
def test_objective_by_the_float32_yardstick(flight):
    """test_gpu_qp_allocator's yardstick on the flown scan: with J(D) the cost the device reports for row t, and H32, H64 the host law in
    the two precisions from the device's own state x_t and the host PID's tau, every host J in float64:
    |J(D) - J(H64)| <= 4 max |J(H32) - J(H64)| + 1e-6 (1 + J(H64)) over every row and env of the flight."""
    from ml4ca_amd.deploy import BatchedQPAllocator
    env, out, z0, x0 = flight
    p = _params(K)
    xs, _, J, _, _ = _device_states(env, out, z0, x0, p, out['act'])
    taus, _ = _host_tau(env, out, z0)
    xs, JD, taus = _np(xs).transpose(0, 2, 1), _np(J).astype(np.float64), _np(taus).transpose(0, 2, 1)
    h32, h64 = BatchedQPAllocator(N, p, env.control_period, np.float32), BatchedQPAllocator(N, p, env.control_period, np.float64)
    J32, J64 = np.zeros((T, N)), np.zeros((T, N))
    for t in range(T):
        pv, tv = xs[t].astype(np.float64), taus[t].astype(np.float64)
        x32, _ = h32.solve(taus[t], xs[t])
        x64, _ = h64.solve(tv, pv)
        J32[t] = h64.objective(x32.astype(np.float64), tv, pv)
        J64[t] = h64.objective(x64, tv, pv)
    yard = np.abs(J32 - J64).max()
    gap = np.abs(JD - J64)
    allow = 4.0 * yard + 1e-6 * (1.0 + J64)
    print('flown scan, K = %d: max |J(D) - J(H64)| = %.3g (yardstick %.3g, largest J %.4g), worst gap / allowed %.3g'
          % (K, gap.max(), yard, J64.max(), (gap / allow).max()))
    assert (gap <= allow).all()


# 8 ---- the driver
def test_dagger_driver_with_the_flown_state_fills_the_ring_like_the_rounds_by_hand():
    from ml4ca_amd.policy import ActorCritic, controller_label_qp, policy_rollout
    from ml4ca_amd.train import PPOUpdater
    torch = torch_()
    n, Tr, rounds, keep, iters = 128, 16, 3, 2, 2                                      # two waves; every env ends an episode in each round
    R = Tr * n
    p = _params(K)
    envs = [_start(_env(n, auto_reset=True, terminate=True, max_ep_len=12), qp=False, nudge=False) for _ in range(4)]
    acs = [ActorCritic(9, 7, (80, 80, 80), seed=3, device=envs[0].device) for _ in range(4)]
    ups = [PPOUpdater(ac) for ac in acs]
    rec = ups[0].dagger(envs[0], rounds, Tr, iters, keep=keep, expert='qp', qp_params=p, thruster_state='flown')
    env, ac, up = envs[1], acs[1], ups[1]
    d_obs, d_act = torch.empty((keep * R, 9), device=env.device), torch.empty((keep * R, 7), device=env.device)
    z, x = torch.zeros((3, n), device=env.device), torch.zeros((5, n), device=env.device)
    blocks = []
    for r in range(rounds):
        ac.upload(env)
        o = policy_rollout(env, Tr, sample=False)
        if r == 1:
            assert bool(x.any()), 'the flown thruster state is handed over'
            own = controller_label_qp(env, o['obs'], o['done'], z=z, x=x, params=p)[0]
        lab, z, x = controller_label_qp(env, o['obs'], o['done'], z=z, x=x, params=p, flown=o['act'])
        blocks.append((o['obs'].clone(), lab.clone(), o['act'].clone()))
        s = r % keep
        d_obs[s * R:(s + 1) * R] = o['obs'].reshape(R, 9)
        d_act[s * R:(s + 1) * R] = lab.reshape(R, 7)
        filled = min(r + 1, keep) * R
        up.pretrain(d_obs[:filled], d_act[:filled], iters, keep_optimizer_state=True)
    data = ups[0].dagger_data
    for slot, r in ((0, 2), (1, 1)):
        assert _bits(data['obs'][slot * R:(slot + 1) * R].view(Tr, n, 9), blocks[r][0]), 'obs of slot %d' % slot
        assert _bits(data['act'][slot * R:(slot + 1) * R].view(Tr, n, 7), blocks[r][1]), 'labels of slot %d' % slot
    assert not _bits(blocks[1][1], own)                                                # not the own recursion's labels
    assert _bits(ups[0].pi_theta, up.pi_theta)
    for r, rx in enumerate(rec):
        assert rx['label_msd'] == float(((blocks[r][2] - blocks[r][1]) ** 2).mean()) and rx['rows'] == min(r + 1, keep) * R
    # thruster_state='own' is the driver without the keyword, bit for bit
    ups[2].dagger(envs[2], rounds, Tr, iters, keep=keep, expert='qp', qp_params=p, thruster_state='own')
    ups[3].dagger(envs[3], rounds, Tr, iters, keep=keep, expert='qp', qp_params=p)
    assert _bits(ups[2].dagger_data['act'], ups[3].dagger_data['act']) and _bits(ups[2].dagger_data['obs'], ups[3].dagger_data['obs'])
    assert _bits(ups[2].pi_theta, ups[3].pi_theta) and not _bits(ups[2].dagger_data['act'], data['act'])
    # a table of equal rows labels like the scalar numbers
    from ml4ca_amd.deploy import qp_allocator_table
    tab = H.to_dev(qp_allocator_table(n, p), envs[0].device)
    e5 = _start(_env(n, auto_reset=True, terminate=True, max_ep_len=12), qp=False, nudge=False)
    u5 = PPOUpdater(ActorCritic(9, 7, (80, 80, 80), seed=3, device=e5.device))
    u5.dagger(e5, rounds, Tr, iters, keep=keep, expert='qp', qp_params=p, thruster_state='flown', qp_table=tab)
    assert _bits(u5.dagger_data['act'], data['act']) and _bits(u5.pi_theta, ups[0].pi_theta)
    with pytest.raises(ValueError, match='thruster_state'):
        ups[0].dagger(envs[0], 1, 4, 1, expert='qp', thruster_state='theirs')
    with pytest.raises(ValueError, match='thruster_state'):
        ups[0].dagger(envs[0], 1, 4, 1, expert='pinv', thruster_state='flown')
