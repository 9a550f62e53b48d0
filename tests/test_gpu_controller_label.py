"""The baseline DP controller's law on rows some other flight wrote (include/dpenv.h dpenv_controller_label, policy.controller_label) and
the DAgger driver built on it (train.PPOUpdater.dagger).  What is tested is labels = the closed loop's own act rows bit for bit (scalar
numbers and a per-env table), labels = deploy.label_rows on the host, blocks in pieces, lanes that do not mix, bf16 rows, a handle that
is left untouched, graph capture, the refusals, and the driver's dataset against the same rounds made by hand on a twin env."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_dp_controller_table import _distinct_table, _env, _host_actions, _same, _same_state, _start

pytestmark = pytest.mark.gpu

N, T = 200, 40                       # three full waves and a tail of 8


def torch_():
    import torch
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    torch = torch_()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _scalar_flight(n):
    """The scalar controller's closed loop, every env cut every 12 rows: (env, rows, the z the flight started from)."""
    from ml4ca_amd.policy import controller_rollout
    env = _env(n, auto_reset=True, terminate=True, max_ep_len=24)
    _start(env)
    z0 = env.get_dp_controller_state().clone()
    out = controller_rollout(env, T)
    done = _np(out['done'])
    assert (done[1:T - 1] != 0).any(0).all(), 'every env ends an episode in an interior row'
    return env, out, z0


@pytest.fixture(scope='module')
def flight():
    """One flight for the tests that only read it (they label with its env and leave its rows alone)."""
    return _scalar_flight(N)


def test_scalar_labels_are_the_closed_loops_act_rows_bit_for_bit(flight):
    from ml4ca_amd.policy import controller_label
    env, out, z0 = flight
    act, z = controller_label(env, out['obs'], out['done'], z=z0)
    assert act.shape == (T, N, 7) and z.shape == (3, N)
    assert _bits(act, out['act']), int((act != out['act']).sum())
    assert _bits(z, env.get_dp_controller_state())
    assert bool((z != 0).any())


def test_table_labels_are_the_closed_loops_and_the_host_laws():
    from ml4ca_amd.deploy import label_rows
    from ml4ca_amd.policy import controller_label, controller_rollout
    env = _env(auto_reset=True, terminate=False, max_ep_len=70)                        # every env is cut (and re-drawn) at row 34
    tab = _distinct_table(N)
    _start(env, H.to_dev(tab, env.device))
    z0 = env.get_dp_controller_state().clone()
    out = controller_rollout(env, T)
    act, z = controller_label(env, out['obs'], out['done'], z=z0)
    assert _bits(act, out['act']), int((act != out['act']).sum())
    assert _bits(z, env.get_dp_controller_state())
    want, wz = label_rows(tab, _np(out['obs']), _np(out['done']), _np(z0), dt=env.control_period)
    got = _np(act)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    assert np.array_equal(_np(z).view(np.uint32), wz.view(np.uint32))
    # the preconditions of the closed loop's own test: every clip of the law was exercised, and the re-draw
    _, _, hits = _host_actions(env, out, tab)
    done = _np(out['done'])
    assert hits['z'] > 0 and hits['tau'] > 0 and (np.abs(got[..., 0]) == 1).any() and (got[..., 1:3] == 1).any()
    assert (done[1:T - 1] != 0).any(0).all()


def test_pieces_with_z_handed_over_equal_one_call(flight):
    from ml4ca_amd.policy import controller_label
    torch = torch_()
    env, out, z0 = flight
    obs, done = out['obs'], out['done']
    one, z_one = controller_label(env, obs, done, z=z0)
    k = 17
    z = z0.clone()                                                                     # z_out aliases z_in in both pieces
    a1 = torch.empty((k, N, 7), device=env.device)
    a2 = torch.empty((T - k, N, 7), device=env.device)
    controller_label(env, obs[:k].contiguous(), done[:k].contiguous(), z=z, out=(a1, z))
    assert not _bits(z, z0)
    controller_label(env, obs[k:].contiguous(), done[k:].contiguous(), z=z, out=(a2, z))
    assert _bits(torch.cat([a1, a2]), one) and _bits(z, z_one)
    # done=None: no episode ends in the block
    no_done, z_nd = controller_label(env, obs, None, z=z0)
    zero_done, z_zd = controller_label(env, obs, torch.zeros_like(done), z=z0)
    assert _bits(no_done, zero_done) and _bits(z_nd, z_zd)
    assert not _bits(no_done, one)                                                     # ... and the done rows matter
    # z=None starts from zero
    a0, _ = controller_label(env, obs, done)
    az, _ = controller_label(env, obs, done, z=torch.zeros_like(z0))
    assert _bits(a0, az)


@pytest.mark.parametrize('n', [N, 65])                                                # 65: a full wave plus one lane
def test_lanes_do_not_mix(n, flight):
    from ml4ca_amd.policy import controller_label
    env, out, z0 = flight if n == N else _scalar_flight(n)
    j, other = 64 + (3 if n == N else 0), 5
    base, zb = controller_label(env, out['obs'], out['done'], z=z0)
    obs, done, z = out['obs'].clone(), out['done'].clone(), z0.clone()
    obs[:, j], done[:, j], z[:, j] = obs[:, other], done[:, other], z[:, other]
    got, zg = controller_label(env, obs, done, z=z)
    keep = [i for i in range(n) if i != j]
    assert _bits(got[:, keep], base[:, keep]) and _bits(zg[:, keep], zb[:, keep])
    assert not _bits(got[:, j], base[:, j])
    assert _bits(got[:, j], base[:, other]) and _bits(zg[:, j], zb[:, other])          # one law for every env: the rows decide


def test_bf16_rows_are_widened_exactly(flight):
    from ml4ca_amd.deploy import label_rows
    from ml4ca_amd.policy import controller_label
    torch = torch_()
    env, out, z0 = flight
    obs16 = out['obs'].to(torch.bfloat16)
    act, z = controller_label(env, obs16, out['done'], z=z0)
    want, wz = label_rows(env.dp_controller, _np(obs16.float()), _np(out['done']), _np(z0), dt=env.control_period)
    got = _np(act)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    assert np.array_equal(_np(z).view(np.uint32), wz.view(np.uint32))
    assert not _bits(act, out['act'])                                                  # the dtype switch is live


def test_labelling_leaves_the_handle_untouched(flight):
    from ml4ca_amd.policy import controller_label, controller_rollout
    _, foreign, _ = flight
    a, b = (_env(auto_reset=True, terminate=True, max_ep_len=24, seed=11) for _ in range(2))
    for e in (a, b):
        _start(e)
    h = T // 2
    _same(controller_rollout(a, h), controller_rollout(b, h), what='first half')
    lab, _ = controller_label(a, foreign['obs'], foreign['done'])
    assert bool(torch_().isfinite(lab).all())
    _same_state(a, b)
    _same(controller_rollout(a, h), controller_rollout(b, h), what='second half')
    _same_state(a, b)
    for x, y in zip(a.get_rng_counters(), b.get_rng_counters()):
        assert torch_().equal(x, y)


def test_captured_label_replays_like_eager_calls(flight):
    from ml4ca_amd.policy import controller_label
    torch = torch_()
    _, src, _ = flight
    env = _env(auto_reset=True, terminate=True, max_ep_len=24)
    tab = H.to_dev(_distinct_table(N, seed=14), env.device)
    _start(env, tab, check=False)                                                      # (the first call allocates the packed block)
    obs, done = src['obs'].clone(), src['done'].clone()
    z_in = torch.zeros((3, N), device=env.device)
    out = controller_label(env, obs, done, z=z_in)                                     # warm-up: the buffers the graph writes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        controller_label(env, obs, done, z=z_in, out=out)
    first = None
    for k in range(2):                                                                 # new contents of the same buffers
        obs.copy_(src['obs'].flip(1) if k else src['obs'] * 0.5)
        done.copy_(src['done'].flip(1) if k else src['done'])
        z_in.fill_(0.25 * k)
        g.replay()
        eager = controller_label(env, obs, done, z=z_in)
        torch.cuda.synchronize()
        assert _bits(out[0], eager[0]) and _bits(out[1], eager[1]), 'replay %d' % k
        first = eager[0].clone() if first is None else first
    assert not _bits(out[0], first)
    # the table re-packed between replays is the one flown
    before = out[0].clone()
    tab[0:9] *= 0.5
    env.set_dp_controller_table(tab, check=False)
    g.replay()
    eager = controller_label(env, obs, done, z=z_in)
    torch.cuda.synchronize()
    assert _bits(out[0], eager[0]) and _bits(out[1], eager[1])
    assert not _bits(out[0], before)


def test_refusals_touch_nothing(flight):
    from ml4ca_amd import DpenvError, _lib
    from ml4ca_amd.policy import controller_label
    torch = torch_()
    _, src, _ = flight
    env = _env(auto_reset=True, terminate=True, max_ep_len=24)
    obs, done = src['obs'], src['done']
    act = torch.full((T, N, 7), 7.5, device=env.device)
    z = torch.full((3, N), -3.5, device=env.device)

    def raw(T_=T, obs_=obs, act_=act, dtype=_lib.F32, size=None):
        io = _lib.ControllerLabelIO()
        io.struct_size = C.sizeof(_lib.ControllerLabelIO) if size is None else size
        io.T, io.obs, io.obs_dtype = T_, (obs_.data_ptr() if obs_ is not None else None), dtype
        io.done, io.z_in, io.z_out = done.data_ptr(), None, z.data_ptr()
        io.act = act_.data_ptr() if act_ is not None else None
        rc = env.lib.dpenv_controller_label(env._h, C.byref(io), env._stream())
        return rc, env.lib.dpenv_last_error(env._h).decode()

    # the controller off: never turned on, and turned off again
    with pytest.raises(DpenvError, match='controller is off'):
        controller_label(env, obs, done, out=(act, z))
    rc, msg = raw()
    assert rc == _lib.EINVAL and 'controller is off' in msg
    env.set_dp_controller()
    env.set_dp_controller(off=True)
    with pytest.raises(DpenvError, match='controller is off'):
        controller_label(env, obs, done, out=(act, z))
    env.set_dp_controller()
    for kw, word in ((dict(T_=0), 'T > 0'), (dict(T_=-3), 'T > 0'), (dict(obs_=None), 'obs and act'), (dict(act_=None), 'obs and act'),
                     (dict(dtype=2), 'obs_dtype'), (dict(dtype=-1), 'obs_dtype'),
                     (dict(size=C.sizeof(_lib.ControllerLabelIO) - 8), 'ABI mismatch'), (dict(size=0), 'ABI mismatch')):
        rc, msg = raw(**kw)
        assert rc == _lib.EINVAL and word in msg, (kw, rc, msg)
    # the Python entry point's own checks
    for bad in (dict(obs=obs[:, :-1].contiguous()), dict(obs=obs.double()), dict(obs=obs[..., :6].contiguous()), dict(done=done[:-1].contiguous()),
                dict(done=done.float()), dict(z=z[:2].contiguous()), dict(out=(act[:-1].contiguous(), z)), dict(obs=obs.cpu())):
        args = dict(obs=obs, done=done, z=None, out=(act, z))
        args.update(bad)
        with pytest.raises(ValueError):
            controller_label(env, args['obs'], args['done'], z=args['z'], out=args['out'])
    torch.cuda.synchronize()
    assert bool((act == 7.5).all()) and bool((z == -3.5).all())
    # ... and the same arguments are served once nothing is wrong
    got, _ = controller_label(env, obs, done, out=(act, z))
    assert bool(torch.isfinite(got).all()) and not bool((act == 7.5).all())


def test_dagger_driver_fills_the_ring_with_the_actors_own_rows():
    from ml4ca_amd.policy import ActorCritic, controller_label, policy_rollout
    from ml4ca_amd.train import PPOUpdater
    torch = torch_()
    n, Tr, rounds, keep, iters = 256, 32, 3, 2, 2
    R = Tr * n
    envs = [_env(n, auto_reset=True, terminate=True, max_ep_len=24) for _ in range(2)]
    for e in envs:
        _start(e)
    acs = [ActorCritic(9, 7, (80, 80, 80), seed=3, device=envs[0].device) for _ in range(2)]
    ups = [PPOUpdater(ac) for ac in acs]
    theta0 = ups[0].pi_theta.clone()
    rec = ups[0].dagger(envs[0], rounds, Tr, iters, keep=keep)
    # the same rounds by hand on the twin: the same actor snapshots fly the same rows
    env, ac, up = envs[1], acs[1], ups[1]
    d_obs, d_act = torch.empty((keep * R, 9), device=env.device), torch.empty((keep * R, 7), device=env.device)
    z = torch.zeros((3, n), device=env.device)
    blocks = []
    for r in range(rounds):
        ac.upload(env)
        o = policy_rollout(env, Tr, sample=False)
        lab, z = controller_label(env, o['obs'], o['done'], z=z)
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
    assert not _bits(blocks[0][0], blocks[2][0]) and bool((torch.stack([b[0] for b in blocks]).diff(dim=0) != 0).any())
    assert _bits(ups[0].pi_theta, up.pi_theta)
    assert len(rec) == rounds
    for r, x in enumerate(rec):
        assert tuple(x['history'].shape) == (iters, 4) and bool(torch.isfinite(x['history']).all())
        assert np.isfinite(x['reward_per_step']) and np.isfinite(x['label_msd']) and x['label_msd'] > 0
        assert x['rows'] == min(r + 1, keep) * R
        assert x['reward_per_step'] == blocks[r][3]                                    # the same reductions of the same rows
        assert x['label_msd'] == float(((blocks[r][2] - blocks[r][1]) ** 2).mean())
    assert not _bits(ups[0].pi_theta, theta0)
    # bf16 rows are refused before anything flies
    e16 = _env(64, auto_reset=True, obs_dtype='bfloat16')
    _start(e16)
    with pytest.raises(ValueError, match='float32'):
        ups[0].dagger(e16, 1, 4, 1)
