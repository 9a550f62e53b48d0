"""The on-policy fit of the neural allocator (train.fit_nn_allocator_on_policy): fit_nn_allocator's `init` leaves the default start's bits
alone, the driver equals the same rounds written out by hand, its pool holds the wrenches that were flown, and nn_wrench_rows forms the
input bits the kernels form.  No test asserts that the fit flies better: that is a measurement."""
import numpy as np
import pytest

from tests.test_gpu_nn_allocator import _env, _np, _start

pytestmark = pytest.mark.gpu

N, T, ROUNDS, ITERS = 128, 8, 2, 3


def torch_():
    import torch
    return torch


def _bits(a, b):
    torch = torch_()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def dataset():
    from ml4ca_amd.deploy import nn_allocator_dataset
    return nn_allocator_dataset(256, seed=4)


@pytest.mark.parametrize('loss', ['mse', 'wrench'])
def test_init_none_is_the_fit_as_it_was_bit_for_bit(loss, dataset):
    """fit_nn_allocator's loop written out from its parts - nn_allocator_init, nn_allocator_minibatches, the gradient call, adam_step - as
    it stood before `init` existed; init=None and init=nn_allocator_init(...) give its theta, another start does not."""
    from ml4ca_amd import train as TR
    torch = torch_()
    dev = 'cuda:0'
    kw = dict(in_dim=9, iters=ITERS, lr=1e-3, minibatch=64, seed=5, leak=0.2, device=dev, loss=loss, alloc_loss=dict(w_power=0.05))
    fit = TR.fit_nn_allocator(dataset, **kw)
    x = torch.as_tensor(np.ascontiguousarray(dataset['x'])).to(dev)
    y = torch.as_tensor(np.ascontiguousarray(dataset['y'])).to(dev)
    tau32 = np.asarray(dataset['tau'], np.float32)
    tau = torch.as_tensor(np.ascontiguousarray(np.concatenate([tau32, np.zeros_like(tau32)], 1))).to(dev)
    theta = torch.as_tensor(TR.nn_allocator_init(9, 5)).to(dev)
    P = TR.layout(9, 6, True)['P']
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.empty(P + TR.NSTAT_ACTOR, device=dev)
    idx = TR.nn_allocator_minibatches(256, 64, ITERS, 5).to(torch.int32).to(dev)
    qp = TR.alloc_loss_params(dict(w_power=0.05))
    for it in range(ITERS):
        if loss == 'mse':
            TR.imitation_grad(theta, x, y, loss='mse', idx=idx[it], out=g, leak=0.2, count=64)
        else:
            TR.allocation_grad(theta, x, tau, qp, idx=idx[it], out=g, leak=0.2, count=64)
        TR.adam_step(theta, g, m, v, step, 1e-3)
    assert _bits(fit['theta'], theta)
    start = TR.nn_allocator_init(9, 5)
    again = TR.fit_nn_allocator(dataset, init=start, **kw)
    assert _bits(again['theta'], theta) and again['J_initial'] == fit['J_initial'] and again['J_final'] == fit['J_final']
    assert np.array_equal(start, TR.nn_allocator_init(9, 5))                           # init is copied, not changed
    on_dev = torch.as_tensor(start).to(dev)
    third = TR.fit_nn_allocator(dataset, init=on_dev, **kw)
    assert _bits(third['theta'], theta) and _bits(on_dev, torch.as_tensor(start).to(dev))
    other = TR.fit_nn_allocator(dataset, init=fit['theta'], **kw)                      # a second leg from the first one's end
    assert not _bits(other['theta'], theta) and other['J_initial'] == fit['J_final']
    # tensors in the dataset are the arrays' rows
    tens = dict(x=x, y=y, tau=torch.as_tensor(tau32).to(dev))
    assert _bits(TR.fit_nn_allocator(tens, **kw)['theta'], theta)


def _hand_rounds(env, base, keep, seed=3):
    """fit_nn_allocator_on_policy's rounds from their parts: (theta, [the flown tau block of each round], records)."""
    from ml4ca_amd import train as TR
    from ml4ca_amd.policy import controller_label_nn, controller_rollout
    torch = torch_()
    kw = dict(in_dim=9, iters=ITERS, lr=1e-3, minibatch=64, leak=0.2, device=env.device, loss='wrench', alloc_loss=dict(w_power=0.05))
    if base is not None:
        fit = TR.fit_nn_allocator(base, seed=seed, **kw)
        theta = fit['theta']
        bx, bt = torch.as_tensor(np.asarray(base['x'], np.float32)).to(env.device), torch.as_tensor(np.asarray(base['tau'], np.float32)).to(env.device)
    else:
        theta = torch.as_tensor(TR.nn_allocator_init(9, seed)).to(env.device)
    flown, recs, slots = [], [], {}
    for r in range(ROUNDS):
        W, b, _ = TR.unflatten(theta, 9, 6, True)
        env.set_nn_allocator(dict(W=list(W), b=list(b), leak=0.2))
        z = env.get_dp_controller_state()
        out = controller_rollout(env, T)
        _, _, tau = controller_label_nn(env, out['obs'], out['done'], z=z, act=False, tau=True)
        flown.append((out['obs'].clone(), out['done'].clone(), z.clone(), tau.clone()))
        slots[r % keep] = tau.reshape(T * N, 3).clone()
        rows = torch.cat([slots[s] for s in sorted(slots)])
        rows = rows[torch.isfinite(rows).all(1)]
        ds = TR.nn_wrench_rows(rows, 9)
        if base is not None:
            ds = dict(x=torch.cat([bx, ds['x']]), tau=torch.cat([bt, ds['tau']]))
        fit = TR.fit_nn_allocator(ds, seed=seed + 1 + r, init=theta, **kw)
        theta = fit['theta']
        recs.append(fit)
    return theta, flown, recs


@pytest.mark.parametrize('with_base,keep', [(True, None), (False, 1)])
def test_on_policy_fit_equals_the_rounds_by_hand_and_its_pool_holds_the_flown_wrenches(with_base, keep, dataset):
    from ml4ca_amd import train as TR
    from ml4ca_amd.deploy import BatchedDPController
    torch = torch_()
    base = dataset if with_base else None
    a, b = (_start(_env(N), nn=False) for _ in range(2))
    res = TR.fit_nn_allocator_on_policy(a, ROUNDS, T, ITERS, base=base, keep=keep, minibatch=64, seed=3, leak=0.2, alloc_loss=dict(w_power=0.05))
    k = ROUNDS if keep is None else keep
    theta, flown, recs = _hand_rounds(b, base, k)
    assert _bits(res['theta'], theta)
    hW, hb, _ = TR.unflatten(theta, 9, 6, True)
    assert all(_bits(u, v) for u, v in zip(list(res['W']) + list(res['b']), list(hW) + list(hb)))
    assert res['pool'].shape == (k * T * N, 3) and res['filled'] == k * T * N and (res['T'], res['n'], res['keep']) == (T, N, k)
    R = T * N
    for r in range(ROUNDS):                                                            # ring order: with keep = 1 the last round owns the slot
        if r + k >= ROUNDS:
            s = r % k
            assert _bits(res['pool'][s * R:(s + 1) * R].view(T, N, 3), flown[r][3]), 'slot %d' % s
    # the flown wrenches are the host PID's on the flown rows, z carried from the launch's start and zeroed behind done rows
    obs, done, z0, tau = (_np(t) for t in flown[-1])
    ctrl = BatchedDPController(N, b.dp_controller, dt=b.control_period)
    ctrl.z = np.ascontiguousarray(z0.T)
    for t in range(T):
        assert np.array_equal(ctrl.wrench(obs[t]).view(np.uint32), tau[t].view(np.uint32)), t
        ctrl.reset(done[t] != 0)
    assert (done != 0).any() and np.abs(tau).max() > 1.0
    assert len(res['rounds']) == ROUNDS and (res['base'] is not None) == with_base
    for r, (rec, want) in enumerate(zip(res['rounds'], recs)):
        assert rec['rows'] == (256 if with_base else 0) + min(r + 1, k) * R
        for key in ('J_initial', 'J_final', 'wrench_ms_initial', 'wrench_ms_final'):
            assert rec[key] == want[key] and np.isfinite(rec[key]), key
    assert a.nn_allocator is not None                                                  # the last network flown stays set
    for bad in (dict(rounds=0), dict(T=0), dict(iters=0), dict(keep=0)):
        args = dict(rounds=1, T=2, iters=1)
        args.update(bad)
        with pytest.raises(ValueError):
            TR.fit_nn_allocator_on_policy(a, args.pop('rounds'), args.pop('T'), args.pop('iters'), **args)


@pytest.mark.parametrize('in_dim', [9, 3])
def test_nn_wrench_rows_forms_the_kernels_input_bits(in_dim):
    """A two-layer wire network hands the scaled wrench through as bits - hidden units 2j and 2j + 1 carry relu(x_j) and relu(-x_j) of
    the last three inputs, p_j = h_2j - h_2j+1; products with 1 and sums with 0 are exact - so raw[:, 0:3] of dpenv_thrust_alloc_nn IS the
    input column the kernel formed from tau."""
    from ml4ca_amd import train as TR
    from ml4ca_amd.policy import thrust_alloc_nn
    torch = torch_()
    rng = np.random.RandomState(2)
    tau = (rng.uniform(-1, 1, size=(193, 3)) * (69.0, 30.0, 80.0)).astype(np.float32)
    tau[0], tau[1] = (69.0, 30.0, 80.0), (-69.0, -30.0, -80.0)
    tau[2] = (1e-30, -1e-30, 1e-30)
    W0, W1 = np.zeros((in_dim, 6), np.float32), np.zeros((6, 6), np.float32)
    for j in range(3):
        W0[in_dim - 3 + j, 2 * j], W0[in_dim - 3 + j, 2 * j + 1] = 1.0, -1.0
        W1[2 * j, j], W1[2 * j + 1, j] = 1.0, -1.0
    wire = dict(W=[W0, W1], b=[np.zeros(6, np.float32), np.zeros(6, np.float32)], leak=0.0)
    dtau = torch.as_tensor(tau).cuda()
    _, raw = thrust_alloc_nn(dtau.t().contiguous(), wire, raw=True)
    rows = TR.nn_wrench_rows(dtau, in_dim)
    x = rows['x']
    assert x.shape == (193, in_dim) and rows['tau'] is dtau
    got, want = _np(raw[:, 0:3]), _np(x[:, in_dim - 3:])
    assert (want != 0).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if in_dim == 9:
        from ml4ca_amd.deploy import nn_allocator_defaults
        assert np.array_equal(_np(x[:, :6]), np.broadcast_to(np.asarray(nn_allocator_defaults()['in_const'], np.float64).astype(np.float32), (193, 6)))
