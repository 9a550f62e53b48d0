"""The PID + rate-limited QP chain on rows some other flight wrote (include/dpenv.h dpenv_controller_label_qp, policy.controller_label_qp)
and the DAgger driver's QP expert (train.PPOUpdater.dagger(expert='qp')).  What is tested is the header's two identities - (A) labels =
the QP closed loop's own act rows, z and thruster state bit for bit, (B) labels = dpenv_thrust_alloc_qp row by row on the PID's tau on
states the QP never flew, also on handles that cannot fly it (per-env hulls, a controller table) - blocks in pieces, lanes that do not
mix, bf16 rows, a handle that is left untouched, graph capture, the refusals, dpenv_controller_label unchanged beside a QP, and the
driver's dataset against the same rounds made by hand on a twin env."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_dp_controller_table import _distinct_table, _same, _same_state
from tests.test_gpu_qp_allocator import _env, _params, _start

pytestmark = pytest.mark.gpu

N, T = 200, 40                       # three full waves and a tail of 8
K = 8


def torch_():
    import torch
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    torch = torch_()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _qp_flight(n=N, preset=False, iters=K, seed=5):
    """The QP closed loop, every env cut at row 23 at the latest and a quarter of them within a few rows: (env, rows, z0, x0)."""
    from ml4ca_amd.policy import controller_rollout
    env = _start(_env(n, preset=preset, auto_reset=True, terminate=True, max_ep_len=24, seed=seed), preset=preset, K=iters)
    z0, x0 = env.get_dp_controller_state().clone(), env.get_qp_allocator_state().clone()
    out = controller_rollout(env, T)
    done = _np(out['done'])
    assert (done[1:T - 1] != 0).any(0).all(), 'every env ends an episode in an interior row'
    assert (done[:6] != 0).any(), 'some envs end early'
    return env, out, z0, x0


def _pinv_flight(n=N, hulls=False, table=False):
    """The PSEUDO-INVERSE baseline's closed loop on a handle with no QP set - states the QP chain would not visit: (env, rows, z0, tab)."""
    from ml4ca_amd.policy import controller_rollout
    env = _env(n, auto_reset=True, terminate=True, max_ep_len=24)
    if hulls:                                                                          # every env on its own hull: per-env blocks
        env.set_vessel_params(H.to_dev(H.random_hulls(np.random.RandomState(21), n), env.device))
    _start(env, qp=False)
    tab = None
    if table:
        tab = _distinct_table(n, seed=12)
        env.set_dp_controller_table(H.to_dev(tab, env.device))
    assert env.qp_allocator is None
    z0 = env.get_dp_controller_state().clone()
    out = controller_rollout(env, T)
    assert (_np(out['done'])[1:T - 1] != 0).any(0).all()
    return env, out, z0, tab


@pytest.fixture(scope='module')
def flight():
    """One QP flight for the tests that only read it (they label with its env and leave its rows alone)."""
    return _qp_flight()


@pytest.fixture(scope='module')
def foreign():
    """One pseudo-inverse flight on a handle without a QP, read-only."""
    return _pinv_flight()


def _parts(env, out, z0, x0, params, table=None):
    """Identity (B) by its parts: dpenv_thrust_alloc_qp row by row on the host PID's tau (NumPy float32, bit for bit the kernel's), z and
    the thruster state zeroed behind a done row: (act [T, n, 7], J [T, n], z [3, n], x [5, n])."""
    from ml4ca_amd.deploy import BatchedDPController
    from ml4ca_amd.policy import thrust_alloc_qp
    torch = torch_()
    n = env.n_envs
    ctrl = BatchedDPController(n, env.dp_controller if table is None else table, dt=env.control_period)
    ctrl.z = np.ascontiguousarray(_np(z0).T)
    S = torch.zeros((5, n), device=env.device) if x0 is None else x0.clone()
    obs, done = _np(out['obs'].float()), _np(out['done'])
    acts, costs = [], []
    for t in range(obs.shape[0]):
        tau = H.to_dev(np.ascontiguousarray(ctrl.wrench(obs[t]).T), env.device)
        act, S, J = thrust_alloc_qp(tau, S, params, env.control_period, cost=True)
        acts.append(act)
        costs.append(J)
        ctrl.reset(done[t] != 0)
        S[:, torch.from_numpy(done[t] != 0).to(S.device)] = 0.0
    return torch.stack(acts), torch.stack(costs), torch.from_numpy(np.ascontiguousarray(ctrl.z.T)).to(env.device), S


@pytest.mark.parametrize('preset,iters', [(False, K), (True, K), (False, 1), (False, 32)])
def test_identity_a_labels_are_the_qp_closed_loops_rows_bit_for_bit(preset, iters, flight):
    from ml4ca_amd.policy import controller_label_qp
    env, out, z0, x0 = flight if (preset, iters) == (False, K) else _qp_flight(preset=preset, iters=iters)
    act, z, x = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0)          # q = NULL: the handle's
    assert act.shape == (T, N, 7) and z.shape == (3, N) and x.shape == (5, N)
    assert _bits(act, out['act']), int((act != out['act']).sum())
    assert _bits(z, env.get_dp_controller_state()) and _bits(x, env.get_qp_allocator_state())
    assert bool((z != 0).any()) and bool((x != 0).any())
    # the same numbers handed over explicitly are the same q
    act2, z2, x2 = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0, params=env.qp_allocator)
    assert _bits(act2, act) and _bits(z2, z) and _bits(x2, x)
    # ... and another iteration count is another law
    other = dict(env.qp_allocator, iterations=3 if iters != 3 else 4)
    act3, _, _ = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0, params=other)
    assert not _bits(act3, act)


@pytest.mark.parametrize('kind', ['shared', 'hulls', 'table'])
def test_identity_b_on_foreign_states_and_on_handles_that_cannot_fly_the_qp(kind, foreign):
    from ml4ca_amd import DpenvError
    from ml4ca_amd.policy import controller_label_qp
    env, out, z0, tab = foreign if kind == 'shared' else _pinv_flight(hulls=kind == 'hulls', table=kind == 'table')
    p = _params(K)
    if kind != 'shared':                                                               # the closed loop refuses this handle
        with pytest.raises(DpenvError):
            env.set_qp_allocator(p)
    act, z, x, J = controller_label_qp(env, out['obs'], out['done'], z=z0, params=p, cost=True)
    want, wJ, wz, wx = _parts(env, out, z0, None, p, table=tab)
    assert _bits(act, want), int((act != want).sum())
    assert _bits(J, wJ), int((J != wJ).sum())
    assert _bits(z, wz) and _bits(x, wx)
    assert bool(torch_().isfinite(J).all()) and bool((x != 0).any())
    assert not _bits(act, out['act'])                                                  # not the pseudo-inverse's rows
    assert env.qp_allocator is None
    if kind == 'table':                                                                # every env on its own row: the scalar numbers differ
        env.set_dp_controller_table(None)
        scalar, _, _ = controller_label_qp(env, out['obs'], out['done'], z=z0, params=p)
        assert not _bits(scalar, act)


def test_pieces_with_z_and_x_handed_over_equal_one_call(flight):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, out, z0, _ = flight
    obs, done = out['obs'], out['done']
    x0 = torch.zeros((5, N), device=env.device)
    x0[0:3] = 0.5
    x0[3:5] = -0.25
    one, z_one, x_one, J_one = controller_label_qp(env, obs, done, z=z0, x=x0, cost=True)
    k = 17
    z, x = z0.clone(), x0.clone()                                                      # the outputs alias the inputs in both pieces
    a1 = torch.empty((k, N, 7), device=env.device)
    a2 = torch.empty((T - k, N, 7), device=env.device)
    _, _, _, J1 = controller_label_qp(env, obs[:k].contiguous(), done[:k].contiguous(), z=z, x=x, out=(a1, z, x), cost=True)
    assert not _bits(z, z0) and not _bits(x, x0)
    _, _, _, J2 = controller_label_qp(env, obs[k:].contiguous(), done[k:].contiguous(), z=z, x=x, out=(a2, z, x), cost=True)
    assert _bits(torch.cat([a1, a2]), one) and _bits(z, z_one) and _bits(x, x_one) and _bits(torch.cat([J1, J2]), J_one)
    # done=None: no episode ends in the block
    no_done, z_nd, x_nd = controller_label_qp(env, obs, None, z=z0, x=x0)
    zero_done, z_zd, x_zd = controller_label_qp(env, obs, torch.zeros_like(done), z=z0, x=x0)
    assert _bits(no_done, zero_done) and _bits(z_nd, z_zd) and _bits(x_nd, x_zd)
    assert not _bits(no_done, one)                                                     # ... and the done rows matter
    # z=None and x=None start from zero, and the starting thruster state matters
    a0, _, _ = controller_label_qp(env, obs, done)
    az, _, _ = controller_label_qp(env, obs, done, z=torch.zeros_like(z0), x=torch.zeros_like(x0))
    assert _bits(a0, az)
    ax, _, _ = controller_label_qp(env, obs, done, x=x0)
    assert not _bits(ax, a0)


@pytest.mark.parametrize('n', [N, 65])                                                # 65: a full wave plus one lane
def test_lanes_do_not_mix(n, flight):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, out, z0, x0 = flight if n == N else _qp_flight(n)
    x0 = x0.clone()
    x0[0] = torch.linspace(-2.0, 2.0, n, device=env.device)                            # every lane its own thruster state
    j, other = 64 + (3 if n == N else 0), 5
    base, zb, xb, Jb = controller_label_qp(env, out['obs'], out['done'], z=z0, x=x0, cost=True)
    obs, done, z, x = out['obs'].clone(), out['done'].clone(), z0.clone(), x0.clone()
    obs[:, j], done[:, j], z[:, j], x[:, j] = obs[:, other], done[:, other], z[:, other], x[:, other]
    got, zg, xg, Jg = controller_label_qp(env, obs, done, z=z, x=x, cost=True)
    keep = [i for i in range(n) if i != j]
    assert _bits(got[:, keep], base[:, keep]) and _bits(zg[:, keep], zb[:, keep]) and _bits(xg[:, keep], xb[:, keep]) and _bits(Jg[:, keep], Jb[:, keep])
    assert not _bits(got[:, j], base[:, j])
    assert _bits(got[:, j], base[:, other]) and _bits(zg[:, j], zb[:, other]) and _bits(xg[:, j], xb[:, other])   # one law: the rows decide
    # a lane whose rows and state are not finite disturbs no other lane
    obs[:, j, 0:3] = float('nan')
    obs[::2, j, 3:6] = float('inf')
    x[:, j] = float('nan')
    got, zg, xg, Jg = controller_label_qp(env, obs, done, z=z, x=x, cost=True)
    assert _bits(got[:, keep], base[:, keep]) and _bits(zg[:, keep], zb[:, keep]) and _bits(xg[:, keep], xb[:, keep]) and _bits(Jg[:, keep], Jb[:, keep])
    assert not bool(torch.isfinite(got[:, j]).all())


def test_bf16_rows_are_widened_exactly(flight):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, out, z0, x0 = flight
    obs16 = out['obs'].to(torch.bfloat16)
    act, z, x, J = controller_label_qp(env, obs16, out['done'], z=z0, x=x0, cost=True)
    want, wz, wx, wJ = controller_label_qp(env, obs16.float(), out['done'], z=z0, x=x0, cost=True)
    assert _bits(act, want) and _bits(z, wz) and _bits(x, wx) and _bits(J, wJ)
    assert not _bits(act, out['act'])                                                  # the dtype switch is live


def test_labelling_leaves_the_handle_untouched(foreign):
    from ml4ca_amd.policy import controller_label_qp, controller_rollout
    torch = torch_()
    _, src, _, _ = foreign
    a, b = (_start(_env(N, auto_reset=True, terminate=True, max_ep_len=24, seed=11), K=K) for _ in range(2))
    h = T // 2
    _same(controller_rollout(a, h), controller_rollout(b, h), what='first half')
    lab, _, _ = controller_label_qp(a, src['obs'], src['done'])                        # the handle's own q
    lab2, _, _ = controller_label_qp(a, src['obs'], src['done'], params=_params(3))    # and an explicit one
    assert bool(torch.isfinite(lab).all()) and not _bits(lab, lab2)
    _same_state(a, b)
    assert torch.equal(a.get_qp_allocator_state(), b.get_qp_allocator_state()) and bool(a.get_qp_allocator_state().any())
    _same(controller_rollout(a, h), controller_rollout(b, h), what='second half')
    _same_state(a, b)
    assert torch.equal(a.get_qp_allocator_state(), b.get_qp_allocator_state())
    for x, y in zip(a.get_rng_counters(), b.get_rng_counters()):
        assert torch.equal(x, y)
    assert a.qp_allocator['iterations'] == K


def test_captured_label_replays_like_eager_calls(foreign):
    from ml4ca_amd.policy import controller_label_qp
    torch = torch_()
    env, src, _, _ = foreign
    p = _params(K)
    obs, done = src['obs'].clone(), src['done'].clone()
    z_in, x_in = torch.zeros((3, N), device=env.device), torch.zeros((5, N), device=env.device)
    out = controller_label_qp(env, obs, done, z=z_in, x=x_in, params=p)               # warm-up: the buffers the graph writes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        controller_label_qp(env, obs, done, z=z_in, x=x_in, params=p, out=out)
    first = None
    for k in range(2):                                                                 # new contents of the same buffers
        obs.copy_(src['obs'].flip(1) if k else src['obs'] * 0.5)
        done.copy_(src['done'].flip(1) if k else src['done'])
        z_in.fill_(0.25 * k)
        x_in.fill_(0.5 * k)
        g.replay()
        eager = controller_label_qp(env, obs, done, z=z_in, x=x_in, params=p)
        torch.cuda.synchronize()
        assert all(_bits(u, v) for u, v in zip(out, eager)), 'replay %d' % k
        first = eager[0].clone() if first is None else first
    assert not _bits(out[0], first)


def test_refusals_touch_nothing(foreign):
    from ml4ca_amd import DpenvError, _lib
    from ml4ca_amd.policy import controller_label_qp, qp_allocator_struct
    torch = torch_()
    _, src, _, _ = foreign
    env = _env(N, auto_reset=True, terminate=True, max_ep_len=24)
    obs, done = src['obs'], src['done']
    act = torch.full((T, N, 7), 7.5, device=env.device)
    z = torch.full((3, N), -3.5, device=env.device)
    x = torch.full((5, N), 1.25, device=env.device)
    cost = torch.full((T, N), -9.0, device=env.device)
    good = _params(K)

    def raw(T_=T, obs_=obs, act_=act, dtype=_lib.F32, size=None, q=None, **fields):
        io = _lib.ControllerLabelQpIO()
        io.struct_size = C.sizeof(_lib.ControllerLabelQpIO) if size is None else size
        io.T, io.obs, io.obs_dtype = T_, (obs_.data_ptr() if obs_ is not None else None), dtype
        io.done, io.z_in, io.z_out, io.x_in, io.x_out = done.data_ptr(), None, z.data_ptr(), None, x.data_ptr()
        io.act = act_.data_ptr() if act_ is not None else None
        io.cost = cost.data_ptr()
        if q != 'none':
            qs = qp_allocator_struct(good)
            for name, (k, v) in fields.items():
                if k is None:
                    setattr(qs, name, v)
                else:
                    getattr(qs, name)[k] = v
            io.q = C.pointer(qs)
        rc = env.lib.dpenv_controller_label_qp(env._h, C.byref(io), env._stream())
        return rc, env.lib.dpenv_last_error(env._h).decode()

    # the controller off: never turned on, and turned off again
    with pytest.raises(DpenvError, match='controller is off'):
        controller_label_qp(env, obs, done, params=good, out=(act, z, x))
    rc, msg = raw()
    assert rc == _lib.EINVAL and 'controller is off' in msg
    env.set_dp_controller()
    env.set_dp_controller(off=True)
    with pytest.raises(DpenvError, match='controller is off'):
        controller_label_qp(env, obs, done, params=good, out=(act, z, x))
    env.set_dp_controller()
    # no q in the call and none set on the handle - also after one was set and dropped
    with pytest.raises(DpenvError, match='no QP allocator'):
        controller_label_qp(env, obs, done, out=(act, z, x))
    rc, msg = raw(q='none')
    assert rc == _lib.EINVAL and 'no QP allocator' in msg
    env.set_qp_allocator(good)
    env.set_qp_allocator(off=True)
    with pytest.raises(DpenvError, match='no QP allocator'):
        controller_label_qp(env, obs, done, out=(act, z, x))
    nan = float('nan')
    for kw, word in ((dict(T_=0), 'T > 0'), (dict(T_=-3), 'T > 0'), (dict(obs_=None), 'obs and act'), (dict(act_=None), 'obs and act'),
                     (dict(dtype=2), 'obs_dtype'), (dict(dtype=-1), 'obs_dtype'),
                     (dict(size=C.sizeof(_lib.ControllerLabelQpIO) - 8), 'ABI mismatch'), (dict(size=0), 'ABI mismatch'),
                     (dict(size=C.sizeof(_lib.ControllerLabelIO)), 'ABI mismatch'),
                     (dict(struct_size=(None, 4)), 'dpenv_qp_allocator ABI mismatch'), (dict(iterations=(None, 0)), 'iterations'),
                     (dict(iterations=(None, 33)), 'iterations'), (dict(w_dalpha=(None, 0.0)), 'w_dalpha'), (dict(w_dforce=(None, -1.0)), 'w_dforce'),
                     (dict(w_slack=(1, -0.5)), 'w_slack'), (dict(f_max=(2, nan)), 'f_max'), (dict(force_rate=(0, float('inf'))), 'force_rate'),
                     (dict(azimuth_rate=(1, -1.0)), 'azimuth_rate'), (dict(kf=(0, 0.0)), 'kf'), (dict(kr=(2, -1.0)), 'kr'), (dict(lx=(1, nan)), 'lever')):
        rc, msg = raw(**kw)
        assert rc == _lib.EINVAL and word in msg, (kw, rc, msg)
    # the Python entry point's own checks
    for bad in (dict(obs=obs[:, :-1].contiguous()), dict(obs=obs.double()), dict(obs=obs[..., :6].contiguous()), dict(done=done[:-1].contiguous()),
                dict(done=done.float()), dict(z=z[:2].contiguous()), dict(x=x[:4].contiguous()), dict(x=z), dict(out=(act[:-1].contiguous(), z, x)),
                dict(out=(act, z, x[:3].contiguous())), dict(obs=obs.cpu())):
        args = dict(obs=obs, done=done, z=None, x=None, out=(act, z, x))
        args.update(bad)
        with pytest.raises(ValueError):
            controller_label_qp(env, args['obs'], args['done'], z=args['z'], x=args['x'], params=good, out=args['out'])
    with pytest.raises(ValueError):
        controller_label_qp(env, obs, done, params=dict(good, kf=[1.0, 1.0]), out=(act, z, x))
    torch.cuda.synchronize()
    assert bool((act == 7.5).all()) and bool((z == -3.5).all()) and bool((x == 1.25).all()) and bool((cost == -9.0).all())
    # ... and the same arguments are served once nothing is wrong
    rc, msg = raw()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool(torch.isfinite(act).all()) and not bool((act == 7.5).any()) and not bool((cost == -9.0).any())
    assert not bool((z == -3.5).any()) and not bool((x == 1.25).all())
    got, _, _ = controller_label_qp(env, obs, done, params=good)
    assert _bits(got, act)


def test_controller_label_beside_a_qp_still_gives_the_pseudo_inverse_labels(foreign):
    from ml4ca_amd.policy import controller_label, controller_label_qp
    _, src, z0, _ = foreign
    a = _start(_env(N, auto_reset=True, terminate=True, max_ep_len=24), K=K, nudge=False)              # the QP set
    b = _start(_env(N, auto_reset=True, terminate=True, max_ep_len=24), qp=False, nudge=False)         # its twin without
    assert a.qp_allocator is not None and b.qp_allocator is None
    la, za = controller_label(a, src['obs'], src['done'], z=z0)
    lb, zb = controller_label(b, src['obs'], src['done'], z=z0)
    assert _bits(la, lb) and _bits(za, zb)
    assert _bits(la, src['act'])                                                       # the foreign block IS a pseudo-inverse flight of this law
    lq, zq, _ = controller_label_qp(a, src['obs'], src['done'], z=z0)
    assert not _bits(lq, la) and _bits(zq, za)                                         # the PID lines are the same, the allocation is not


def test_dagger_driver_with_the_qp_expert_fills_the_ring_like_the_rounds_by_hand():
    from ml4ca_amd.policy import ActorCritic, controller_label, controller_label_qp, policy_rollout
    from ml4ca_amd.train import PPOUpdater
    torch = torch_()
    n, Tr, rounds, keep, iters = 256, 32, 3, 2, 2
    R = Tr * n
    p = _params(K)
    envs = [_start(_env(n, auto_reset=True, terminate=True, max_ep_len=24), qp=False, nudge=False) for _ in range(2)]
    acs = [ActorCritic(9, 7, (80, 80, 80), seed=3, device=envs[0].device) for _ in range(2)]
    ups = [PPOUpdater(ac) for ac in acs]
    theta0 = ups[0].pi_theta.clone()
    rec = ups[0].dagger(envs[0], rounds, Tr, iters, keep=keep, expert='qp', qp_params=p)
    # the same rounds by hand on the twin: the same actor snapshots fly the same rows; z AND x go from round to round
    env, ac, up = envs[1], acs[1], ups[1]
    d_obs, d_act = torch.empty((keep * R, 9), device=env.device), torch.empty((keep * R, 7), device=env.device)
    z, x = torch.zeros((3, n), device=env.device), torch.zeros((5, n), device=env.device)
    blocks = []
    for r in range(rounds):
        ac.upload(env)
        o = policy_rollout(env, Tr, sample=False)
        if r == 1:
            assert bool(x.any()), 'the thruster state is handed over'
            pinv, _ = controller_label(env, o['obs'], o['done'], z=z)
        lab, z, x = controller_label_qp(env, o['obs'], o['done'], z=z, x=x, params=p)
        blocks.append((o['obs'].clone(), lab.clone(), o['act'].clone(), float(o['rew'].mean())))
        s = r % keep
        d_obs[s * R:(s + 1) * R] = o['obs'].reshape(R, 9)
        d_act[s * R:(s + 1) * R] = lab.reshape(R, 7)
        filled = min(r + 1, keep) * R
        up.pretrain(d_obs[:filled], d_act[:filled], iters, keep_optimizer_state=True)
    data = ups[0].dagger_data
    assert data['filled'] == keep * R and data['obs'].shape == (keep * R, 9) and data['act'].shape == (keep * R, 7)
    for slot, r in ((0, 2), (1, 1)):                                                   # ring order: round 2 overwrote round 0
        assert _bits(data['obs'][slot * R:(slot + 1) * R].view(Tr, n, 9), blocks[r][0]), 'obs of slot %d' % slot
        assert _bits(data['act'][slot * R:(slot + 1) * R].view(Tr, n, 7), blocks[r][1]), 'labels of slot %d' % slot
    assert not _bits(blocks[1][1], pinv)                                               # the QP's labels, not the pseudo-inverse's
    assert _bits(ups[0].pi_theta, up.pi_theta)
    assert len(rec) == rounds
    for r, rx in enumerate(rec):
        assert tuple(rx['history'].shape) == (iters, 4) and bool(torch.isfinite(rx['history']).all())
        assert np.isfinite(rx['reward_per_step']) and np.isfinite(rx['label_msd']) and rx['label_msd'] > 0
        assert rx['rows'] == min(r + 1, keep) * R
        assert rx['reward_per_step'] == blocks[r][3]                                   # the same reductions of the same rows
        assert rx['label_msd'] == float(((blocks[r][2] - blocks[r][1]) ** 2).mean())
    assert not _bits(ups[0].pi_theta, theta0)
    assert envs[0].qp_allocator is None                                                # the driver sets nothing on the env
    with pytest.raises(ValueError, match='expert'):
        ups[0].dagger(envs[0], 1, 4, 1, expert='slsqp')
