"""A population of neural allocators on the device (include/dpenv.h: dpenv_set_nn_allocator_population /
dpenv_thrust_alloc_nn_population): K networks of one shape, env i flies network ((env_id_base + i) // envs_per_net) % K.  The yardstick is
the one-network flight (dpenv_set_nn_allocator), which tests/test_gpu_nn_allocator.py ties to the host statement: every env's rows under a
population are, bit for bit, its rows on an identically configured handle that flies its network alone."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_nn_allocator import HEAD_TOL, REST, _bits_equal, _env, _np, _refs, _refused, _same, _start, free_tau
from tests.test_nn_allocator_cpu import seeded_net

pytestmark = pytest.mark.gpu

DEEP = (9, 20, 20, 20, 20, 6)
ROWS = ('obs', 'act', 'rew', 'done', 'last_obs')
AXIS = dict(obs=1, act=1, rew=1, done=1, last_obs=0, z=1, st=1, ctr=1, ref=1)     # the env axis of every block of a record


def _nets(K, sizes=DEEP, scale=3.0, leak=0.0, seed=60):
    """K seeded random networks (NumPy), outputs of order 1 and distinct per network"""
    return [dict(seeded_net(sizes, seed=seed + k, scale=scale), leak=leak) for k in range(K)]


def _dev(nets, device='cuda:0'):
    from ml4ca_amd.policy import nn_population_to
    return nn_population_to(nets, device)


def _one(net, device='cuda:0'):
    from ml4ca_amd.policy import nn_net_to
    return nn_net_to(net, device)


def _record(env, T, switch=True):
    """flies T steps (a setpoint switch at step 3) and returns the rows with the final z and state beside them"""
    from ml4ca_amd.policy import controller_rollout
    kw = dict(switch_steps=(3,), refs=_refs(env.device, env.n_envs)) if switch and T > 3 else {}
    rec = {k: v.clone() for k, v in controller_rollout(env, T, **kw).items()}
    rec['z'] = env.get_dp_controller_state()
    rec['st'], rec['ctr'] = env.get_state()
    return rec


def _flight(n, T, allocator, env_kw=None, **start):
    """a fresh handle, configured by test_gpu_nn_allocator's _start without a network, `allocator(env)` then sets its allocation stage"""
    env = _start(_env(n, **(env_kw or {})), nn=False, **start)
    allocator(env)
    return env, _record(env, T)


def _same_on(a, b, mask, what=''):
    """records a and b agree bit for bit on the envs of mask (NumPy bool [n])"""
    import torch
    m = torch.from_numpy(np.flatnonzero(mask)).to(a['act'].device)
    for k in a:
        x, y = a[k].index_select(AXIS[k], m), b[k].index_select(AXIS[k], m)
        assert torch.equal(x, y), '%s %s: %d elements differ' % (what, k, int((x != y).sum()))


def _population_equals_its_networks(n, T, K, E, sizes=DEEP, env_kw=None, **start):
    """The population's flight, then per network in use the one-network flight on an identically configured handle: equal on that
    network's envs, bit for bit - rows, final z and state.  Returns the population's record and the index map."""
    import torch
    from ml4ca_amd.deploy import nn_population_index
    nets = _nets(K, sizes)
    _, pop = _flight(n, T, lambda e: e.set_nn_allocator_population(_dev(nets), envs_per_net=E), env_kw, **start)
    idx = nn_population_index(n, K, E, (env_kw or {}).get('env_id_base', 0))
    assert bool(torch.isfinite(pop['act']).all()) and float(pop['act'][..., 0:3].abs().max()) > 0.05
    first = None
    for k in np.unique(idx):
        _, one = _flight(n, T, lambda e: e.set_nn_allocator(_one(nets[k])), env_kw, **start)
        _same_on(pop, one, idx == k, what='network %d' % k)
        if first is None:
            first = one
        else:                                                    # the networks are distinct: network 0's flight is not network k's
            m = torch.from_numpy(np.flatnonzero(idx == k)).to(pop['act'].device)
            assert not torch.equal(first['act'][:, m], pop['act'][:, m])
    return pop, idx


# ---- 1. K = 1 is the scalar flight ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [DEEP, (3, 1, 6)])
def test_one_network_population_equals_the_scalar_flight(sizes):
    """n = 130, T = 8: obs, act, reward, done rows, final z and state bit for bit"""
    pop, idx = _population_equals_its_networks(130, 8, 1, 64, sizes)
    assert not idx.any()
    assert bool((pop['done'][:-1] != 0).any()), 'no episode ended inside the launch'


# ---- 2., 3. the index map in the closed loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,E,n', [(3, 64, 200), (2, 128, 320), (5, 64, 130)])
def test_every_env_flies_its_network(K, E, n):
    """K = 3, E = 64, n = 200: waves map to networks 0, 1, 2, 0 and the last wave has 8 live lanes.  K = 2, E = 128, n = 320: two waves
    per network, 0 0 1 1 0.  K = 5, n = 130: networks 3 and 4 go unused."""
    _, idx = _population_equals_its_networks(n, 8, K, E)
    want = {(3, 64, 200): [0, 1, 2, 0], (2, 128, 320): [0, 0, 1, 1, 0], (5, 64, 130): [0, 1, 2]}[(K, E, n)]
    assert idx[::64].tolist() == want


# ---- 4. shapes at the edges of the image stride -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [(9, 96, 96, 96, 96, 6), (9, 17, 17, 6)])
def test_shapes_at_the_edges_of_the_image_stride(sizes):
    """five layers of the largest width (the largest image per network) and a width one past a chunk (the pad edge), T = 4, K = 3"""
    _population_equals_its_networks(130, 4, 3, 64, sizes)


# ---- 5. every vessel source, with and without the filter --------------------------------------------------------------------------------
def _source(kind, n):
    import ml4ca_amd
    if kind == 'loss':                                           # the single class carries thrust-loss coefficients: the shared-loss kernels
        vp = np.asarray(ml4ca_amd.default_vessel(), np.float32).copy()
        vp[26:32] = [0.05, 0.1, 0.08, 0.02, 0.06, 0.04]
        return dict(env_kw=dict(vessel_params=vp))
    if kind == 'hulls':
        return dict(hulls=H.random_hulls(np.random.RandomState(3), n))
    if kind == 'randomised':
        return dict(randomise=0.15)
    return {}


@pytest.mark.parametrize('filt', [False, True])
@pytest.mark.parametrize('kind', ['shared', 'loss', 'hulls', 'randomised'])
def test_every_vessel_source_with_and_without_the_filter(kind, filt):
    """n = 130, T = 6, K = 3: the shared hull, the thrust-loss preset, per-env blocks and randomised hulls - the eight kernel forms"""
    _population_equals_its_networks(130, 6, 3, 64, filt=filt, **_source(kind, 130))


# ---- 6. the handle-free call ------------------------------------------------------------------------------------------------------------
N_FREE, K_FREE = 200, 3                                          # waves -> networks 0, 1, 2, 0; free_tau's NaN lane 70 and inf lane 131


def test_handle_free_call_against_the_scalar_call_and_the_host_statement():
    import torch
    from ml4ca_amd.deploy import BatchedNNAllocatorPopulation, nn_population_index
    from ml4ca_amd.policy import thrust_alloc_nn, thrust_alloc_nn_population
    nets = _nets(K_FREE)
    tau = free_tau(N_FREE)
    idx = nn_population_index(N_FREE, K_FREE, 64)
    dtau = H.to_dev(np.ascontiguousarray(tau.T))
    act, p = thrust_alloc_nn_population(dtau, _dev(nets), raw=True)
    torch.cuda.synchronize()
    act, p = _np(act), _np(p)
    # the scalar call per network, on that network's lanes
    for k in range(K_FREE):
        a1, p1 = thrust_alloc_nn(dtau, _one(nets[k]), raw=True)
        assert _bits_equal(act[idx == k], _np(a1)[idx == k]) and _bits_equal(p[idx == k], _np(p1)[idx == k]), k
    assert not _bits_equal(act[idx == 1], _np(a1)[idx == 1])     # (a1 is network 2's)
    # the host statement: everything outside the heads bit for bit, the heads within the polynomial's bound plus a rounding
    h_act, h_p = BatchedNNAllocatorPopulation(N_FREE, nets, envs_per_net=64).allocate(tau, raw=True)
    assert _bits_equal(p, h_p) and _bits_equal(act[:, 0:3], h_act[:, 0:3])
    rest = ~(np.isfinite(tau).all(1) & np.isfinite(h_p).all(1))
    assert np.flatnonzero(rest).tolist() == [70, 131]
    assert np.array_equal(act[rest], np.broadcast_to(REST, (2, 7)))
    ang = (h_p[:, 3:5] * np.float32(np.pi)).astype(np.float64)
    err = np.maximum(np.abs(act[:, [3, 5]] - np.sin(ang)), np.abs(act[:, [4, 6]] - np.cos(ang)))[~rest]
    print('largest head error %.3g (bound %.3g)' % (err.max(), HEAD_TOL))
    assert err.max() <= HEAD_TOL
    # a list of NumPy nets is stacked and copied: the same answer
    assert _bits_equal(_np(thrust_alloc_nn_population(dtau, nets)), act)


def test_rest_rule_stays_in_its_lane_and_in_its_network():
    from ml4ca_amd.deploy import nn_population_index
    from ml4ca_amd.policy import thrust_alloc_nn_population
    nets = _nets(K_FREE)
    tau = free_tau(N_FREE)
    idx = nn_population_index(N_FREE, K_FREE, 64)
    act = _np(thrust_alloc_nn_population(H.to_dev(np.ascontiguousarray(tau.T)), nets))
    for lane in (70, 131):                                       # a NaN / an inf tau rests that lane only
        clean = tau.copy()
        clean[lane] = 1.0
        a2 = _np(thrust_alloc_nn_population(H.to_dev(np.ascontiguousarray(clean.T)), nets))
        assert np.array_equal(act[lane], REST) and not np.array_equal(a2[lane], REST)
        assert _bits_equal(np.delete(a2, lane, 0), np.delete(act, lane, 0))
    # an inf weight in network 1 rests network 1's lanes only (relu: 0 * -inf = NaN, which every later layer spreads)
    bad = [dict(n, W=[w.copy() for w in n['W']]) for n in nets]
    bad[1]['W'][0][0, 0] = np.inf
    a3 = _np(thrust_alloc_nn_population(H.to_dev(np.ascontiguousarray(tau.T)), bad))
    assert np.array_equal(a3[idx == 1], np.broadcast_to(REST, (int((idx == 1).sum()), 7)))
    assert _bits_equal(a3[idx != 1], act[idx != 1]) and not np.array_equal(act[idx == 1][0], REST)


def test_handle_free_refusals():
    from ml4ca_amd.policy import thrust_alloc_nn_population
    nets, dtau = _nets(2), H.to_dev(np.zeros((3, 130), np.float32))
    for kw, word in ((dict(envs_per_net=32), 'envs_per_net'), (dict(envs_per_net=96), 'envs_per_net'), (dict(envs_per_net=0), 'envs_per_net'),
                     (dict(leak=1.5), 'leak')):
        _refused(lambda: thrust_alloc_nn_population(dtau, nets, **kw), word)


# ---- 7. the rows against the scan -------------------------------------------------------------------------------------------------------
def test_act_rows_are_the_handle_free_call_on_the_scans_wrench():
    """K = 3, n = 200, T = 12, episodes ending inside the launch.  With the population in force the wrench-only scan runs, the scan
    without a network is refused, the scan with an explicit network labels with it; and the closed loop's act rows are
    thrust_alloc_nn_population on the scan's tau, row by row, bit for bit."""
    import torch
    from ml4ca_amd.policy import controller_label_nn, thrust_alloc_nn, thrust_alloc_nn_population
    nets = _nets(3)
    stacked = _dev(nets)
    env = _start(_env(200), nn=False)
    env.set_nn_allocator_population(stacked)
    z0 = env.get_dp_controller_state().clone()
    out = _record(env, 12)
    assert bool((out['done'][:-1] != 0).any())
    _, z, tau = controller_label_nn(env, out['obs'], done=out['done'], z=z0, act=False, tau=True)
    assert torch.equal(z, out['z'])
    for t in range(12):
        act = thrust_alloc_nn_population(tau[t].t().contiguous(), stacked)
        assert torch.equal(act, out['act'][t]), (t, int((act != out['act'][t]).sum()))
    _refused(lambda: controller_label_nn(env, out['obs'], done=out['done'], z=z0), 'pass a')
    lab, _, tau1 = controller_label_nn(env, out['obs'], done=out['done'], z=z0, net=_one(nets[1]), tau=True)
    assert torch.equal(tau1, tau) and torch.equal(lab[:, 64:128], out['act'][:, 64:128]) and not torch.equal(lab[:, :64], out['act'][:, :64])
    assert torch.equal(lab[3], thrust_alloc_nn(tau[3].t().contiguous(), _one(nets[1])))
    _same(_record(env, 4, switch=False), _record_after(200, stacked, 12, 4), what='the scans changed nothing')


def _record_after(n, stacked, T0, T1):
    """a twin of the scan test's handle: T0 steps, then the T1 that are compared"""
    env = _start(_env(n), nn=False)
    env.set_nn_allocator_population(stacked)
    _record(env, T0)
    return _record(env, T1, switch=False)


# ---- 8. launch composition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filt', [False, True])
def test_two_launches_of_six_write_the_rows_of_one_of_twelve(filt):
    import torch
    from ml4ca_amd.policy import controller_rollout
    stacked = _dev(_nets(3))
    a, b = (_start(_env(200), filt, nn=False) for _ in range(2))
    for e in (a, b):
        e.set_nn_allocator_population(stacked)
    refs = _refs(a.device, 200)
    one = controller_rollout(a, 12, switch_steps=(3,), refs=refs)
    h1 = {k: v.clone() for k, v in controller_rollout(b, 6, switch_steps=(3,), refs=refs).items()}
    h2 = controller_rollout(b, 6)
    for k in ('obs', 'act', 'rew', 'done') + (('ref',) if filt else ()):
        assert torch.equal(one[k][:6], h1[k]) and torch.equal(one[k][6:], h2[k]), k
    assert torch.equal(one['last_obs'], h2['last_obs'])
    assert torch.equal(a.get_dp_controller_state(), b.get_dp_controller_state())
    assert bool((one['done'] != 0).any())


def test_host_array_upload_flies_the_device_pointer_rows():
    from ml4ca_amd.policy import controller_rollout
    nets = _nets(3)
    a, b = (_start(_env(200), nn=False) for _ in range(2))
    a.set_nn_allocator_population(_dev(nets))
    b.set_nn_allocator_population(nets)                           # NumPy: device_pointers = 0
    assert isinstance(b.nn_allocator['net']['W'][0], np.ndarray) and b.nn_allocator['K'] == 3
    _same(controller_rollout(a, 6), controller_rollout(b, 6), what='host arrays')


def test_upload_captured_with_the_rollout_replays_the_updated_weights():
    """The setter (device pointers: one packing launch, no allocation once the image of that shape and K exists) and the launch in one
    graph; the stacked weight tensors are overwritten in place between replays, and each replay flies what an eager handle flies."""
    import torch
    from ml4ca_amd.policy import controller_rollout
    nets = _nets(3)
    st_c, st_a = _dev(nets), _dev(nets)
    a, c = (_start(_env(200, max_ep_len=40), nn=False) for _ in range(2))
    a.set_nn_allocator_population(st_a)
    c.set_nn_allocator_population(st_c)
    buf = controller_rollout(c, 6)                                # warm-up outside the capture (and the image's allocation)
    _same(buf, controller_rollout(a, 6), what='warm-up')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.set_nn_allocator_population(st_c)
        controller_rollout(c, 6, out=buf)
    first = None
    for k in range(3):
        for st in (st_c, st_a):
            for w in st['W']:
                w.mul_(1.25 if k else 1.0)
            st['b'][-1][1].add_(0.05 * k)                         # network 1 alone moves its output bias
        g.replay()
        a.set_nn_allocator_population(st_a)
        eager = controller_rollout(a, 6)
        torch.cuda.synchronize()
        _same(buf, eager, what='replay %d' % k)
        if first is None:
            first = buf['act'].clone()
    assert not torch.equal(first, buf['act'])


def test_env_id_base_counts_in_the_index():
    """a 128-env handle at env_id_base = 128 flies envs 128 .. 255 of a 256-env handle (K = 3: networks 2, 0 of 0, 1, 2, 0)"""
    stacked = _dev(_nets(3))
    whole = _start(_env(256), nn=False)
    part = _start(_env(128, env_id_base=128), nn=False)
    for e in (whole, part):
        e.set_nn_allocator_population(stacked)
    w, p = _record(whole, 8), _record(part, 8)
    import torch
    for k in p:
        x = w[k].narrow(AXIS[k], 128, 128)
        assert torch.equal(x, p[k]), '%s: %d elements differ' % (k, int((x != p[k]).sum()))
    assert not torch.equal(w['act'][:, :128], p['act'])


# ---- 9. refusals and returns ------------------------------------------------------------------------------------------------------------
def test_refusals_and_returns():
    import torch
    from ml4ca_amd.deploy import dp_controller_table, qp_allocator_table
    from ml4ca_amd.policy import controller_rollout
    n = 128
    nets = _nets(2)
    stacked = _dev(nets)
    fly = lambda e: {k: v.clone() for k, v in controller_rollout(e, 2).items()}
    # handles on which no population can be set: each refusal, then the flight of a twin that never got the call
    f = _env(n)
    f.reset()
    _refused(lambda: f.set_nn_allocator_population(stacked), 'DP controller is off')
    q, q2 = (_start(_env(n), nn=False) for _ in range(2))
    for e in (q, q2):
        e.set_qp_allocator()
    _refused(lambda: q.set_nn_allocator_population(stacked), 'QP allocator is set')
    _same(fly(q), fly(q2), what='a QP handle')
    for e in (q, q2):
        e.set_qp_allocator_table(torch.from_numpy(qp_allocator_table(n)).to(e.device))
    _refused(lambda: q.set_nn_allocator_population(stacked), 'QP allocator is set')
    _same(fly(q), fly(q2), what='a QP table handle')
    tab = torch.from_numpy(dp_controller_table(n)).to(q.device)
    t, t2 = (_start(_env(n), nn=False) for _ in range(2))
    for e in (t, t2):
        e.set_dp_controller_table(tab)
    _refused(lambda: t.set_nn_allocator_population(stacked), 'per-env controller table is in force')
    _same(fly(t), fly(t2), what='a controller table handle')
    u = _start(_env(n), nn=False)
    u.set_integral_action()
    _refused(lambda: u.set_nn_allocator_population(stacked), 'integral action off')
    s = _start(_env(64, env_id_base=32), nn=False)
    _refused(lambda: s.set_nn_allocator_population(stacked), 'env_id_base')
    # a handle with a population in force: every refused call leaves the flight what the twin's is
    a, b = (_start(_env(n), nn=False) for _ in range(2))
    for e in (a, b):
        e.set_nn_allocator_population(stacked)
    import ctypes as C
    from ml4ca_amd import _lib
    from ml4ca_amd.policy import nn_allocator_struct

    def raw_set(K, E):                                           # (the Python layer derives K from the stack: K < 1 needs the C call)
        s_, keep = nn_allocator_struct(_one(nets[0]), a.nn_allocator, a.device)
        _lib.check(a.lib.dpenv_set_nn_allocator_population(a._h, C.byref(s_), K, E, a._stream()), a._h)
    for call, word in ((lambda: raw_set(0, 64), 'K must be'), (lambda: raw_set(-3, 64), 'K must be'),
                       (lambda: a.set_nn_allocator_population(stacked, envs_per_net=32), 'envs_per_net'),
                       (lambda: a.set_nn_allocator_population(stacked, envs_per_net=96), 'envs_per_net'),
                       (lambda: a.set_nn_allocator_population(stacked, envs_per_net=0), 'envs_per_net'),
                       (lambda: a.set_nn_allocator_population(stacked, leak=1.5), 'leak'),
                       (lambda: a.set_nn_allocator_population(stacked, azimuth_mode=3), 'azimuth_mode'),
                       (lambda: a.set_nn_allocator_population(stacked, tau_scale=[1.0, float('nan'), 1.0]), 'tau_scale'),
                       (a.set_qp_allocator, 'neural allocator is set'),
                       (lambda: a.set_qp_allocator_table(torch.from_numpy(qp_allocator_table(n)).to(a.device), check=False), 'neural allocator is set'),
                       (lambda: a.set_dp_controller_table(tab, check=False), 'neural allocator is set')):
        _refused(call, word)
        _same(fly(a), fly(b), what='after the refusal of %s' % word)
    with pytest.raises(ValueError):                              # an empty stack does not reach the library
        a.set_nn_allocator_population(dict(W=[w[:0] for w in stacked['W']], b=[x[:0] for x in stacked['b']]))
    # set_nn_allocator after a population flies the single network; a population after one network flies the population
    net1 = _one(nets[1])
    x, single, y, pop = (_start(_env(n), nn=False) for _ in range(4))
    x.set_nn_allocator_population(stacked)
    x.set_nn_allocator(net1)
    single.set_nn_allocator(net1)
    assert 'K' not in x.nn_allocator
    _same(fly(x), fly(single), what='one network after a population')
    y.set_nn_allocator(net1)
    y.set_nn_allocator_population(stacked)
    pop.set_nn_allocator_population(stacked)
    pop_rows = fly(pop)
    _same(fly(y), pop_rows, what='a population after one network')
    # NULL restores the pseudo-inverse's rows; set_dp_controller drops the population
    c, d, plain = (_start(_env(n), nn=False) for _ in range(3))
    for e in (c, d):
        e.set_nn_allocator_population(stacked)
    c.set_nn_allocator_population(off=True)
    d.set_dp_controller()
    assert c.nn_allocator is None and d.nn_allocator is None
    ref = fly(plain)
    _same(fly(c), ref, what='NULL')
    _same(fly(d), ref, what='set_dp_controller')
    assert not torch.equal(ref['act'], pop_rows['act'])          # ... which are not the population's rows
    c.set_qp_allocator()                                         # and nothing stands against a QP any more


# ---- 10. the sweep ----------------------------------------------------------------------------------------------------------------------
def test_sweep_equals_one_box_test_per_network():
    """K = 2, D = 16, E = 64, n = 128, T = 50, chunk = 25: per env the IAE and the work are those of
    baseline_box_test_streamed(allocator='nn') with the env's network under the same currents, exactly."""
    import math
    import torch
    from ml4ca_amd import evaluate
    from ml4ca_amd.evaluate import pareto_front
    K, D, E, n, T = 2, 16, 64, 128, 50
    nets = _nets(K)
    mk = lambda: H.make_pair('final_cont', n, terminate=False, seed=3, current=True)[0]
    res = evaluate.nn_allocator_sweep(mk(), _dev(nets), directions=D, T=T, chunk=25, envs_per_net=E)
    assert res['iae'].shape == (K, D) and res['work'].shape == (K, D, 3) and res['env_iae'].shape == (n,) and res['env_work'].shape == (n, 3)
    assert bool(torch.isfinite(res['env_iae']).all()) and bool(torch.isfinite(res['env_work']).all())
    for k in range(K):
        env = mk()
        beta = (2.0 * math.pi / D) * (torch.arange(n, device=env.device) % D).float()
        env.set_current(torch.full((n,), 0.2, device=env.device), beta.contiguous())
        one = evaluate.baseline_box_test_streamed(env, T=T, reference_filter=True, chunk=25, allocator='nn', net=_one(nets[k]))
        sl = slice(k * E, (k + 1) * E)
        assert torch.equal(res['env_iae'][sl], one['iae'][sl]) and torch.equal(res['env_work'][sl], one['work'][sl]), k
        assert torch.equal(res['iae'][k], one['iae'][sl].reshape(E // D, D).mean(0))
        assert torch.equal(res['work'][k], one['work'][sl].reshape(E // D, D, 3).mean(0))
    assert torch.equal(res['mean_iae'], res['iae'].mean(1)) and torch.equal(res['mean_work'], res['work'].mean(1))
    assert np.array_equal(res['front'], pareto_front(_np(res['mean_iae']), _np(res['mean_work'].sum(1))))
    assert not torch.equal(res['iae'][0], res['iae'][1])


# ---- 11. one handle through both setters ------------------------------------------------------------------------------------------------
def test_one_handle_walked_through_both_setters_flies_each_setting_alone():
    """The two setters share one image layout and one installer; what that can get wrong is an address or a stride that survives from
    the call before.  One handle of n = 192 (three waves), T = 4, walked through: one network from host arrays; a population of K = 3 of
    the largest shape from device tensors; one network (3, 1, 6) from device tensors; K = 2 of (9, 17, 17, 6) from host arrays (another
    shape and K: the image is re-allocated); K = 2 of that shape with other weights (the image in place); off.  Every flight starts
    from the same saved state, and after every setter the rows are, bit for bit, those of a fresh handle given that setting alone -
    after "off" the pseudo-inverse's."""
    import torch
    from ml4ca_amd.policy import controller_rollout
    n, T, E = 192, 4, 64
    pad_edge, largest = (9, 17, 17, 6), (9, 96, 96, 96, 96, 6)
    walk = [
        ('one network, host arrays', lambda e: e.set_nn_allocator(_nets(1, pad_edge, seed=70)[0])),
        ('K = 3 of the largest shape, device tensors', lambda e: e.set_nn_allocator_population(_dev(_nets(3, largest, seed=71)), envs_per_net=E)),
        ('one network (3, 1, 6), device tensors', lambda e: e.set_nn_allocator(_one(_nets(1, (3, 1, 6), seed=74)[0]))),
        ('K = 2, host arrays, a new image', lambda e: e.set_nn_allocator_population(_nets(2, pad_edge, seed=75), envs_per_net=E)),
        ('K = 2, other weights, the image in place', lambda e: e.set_nn_allocator_population(_nets(2, pad_edge, seed=77), envs_per_net=E)),
        ('off', lambda e: e.set_nn_allocator_population(off=True)),
    ]
    env = _start(_env(n), nn=False)
    st0, ctr0 = env.get_state()
    z0 = torch.zeros((3, n), device=env.device)

    def fly(e, setting):
        setting(e)
        e.set_state(st0, ctr0)
        e.set_dp_controller_state(z0)
        return {k: v.clone() for k, v in controller_rollout(e, T).items()}

    pinv = fly(_start(_env(n), nn=False), lambda e: None)
    before = pinv
    for what, setting in walk:
        rows = fly(env, setting)
        alone = pinv if what == 'off' else fly(_start(_env(n), nn=False), setting)
        _same(rows, alone, what=what)
        assert bool(torch.isfinite(rows['act']).all())
        assert not torch.equal(rows['act'], before['act']), '%s: the rows of the setting before' % what
        before = rows
