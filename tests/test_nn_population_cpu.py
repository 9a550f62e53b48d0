"""A population of neural allocators without a GPU (include/dpenv.h: dpenv_set_nn_allocator_population): the host statement per env is
the one-network statement of that env's network, the index map is the header's law, the stack refuses mixed shapes, the sweep checks its
arguments before it touches the env, and the two entry points are declared, exported and bound."""
import re
import subprocess
import types

import numpy as np
import pytest

from tests.test_nn_allocator_cpu import seeded_net

SIZES = (9, 20, 20, 20, 20, 6)
TAU_MAX = np.array([69.0, 30.0, 80.0])


def _nets(K, sizes=SIZES, scale=3.0):
    return [seeded_net(sizes, seed=40 + k, scale=scale) for k in range(K)]


def _tau(n, seed=3):
    tau = (np.random.RandomState(seed).uniform(-1, 1, size=(n, 3)) * TAU_MAX).astype(np.float32)
    tau[5, 1] = np.nan                                   # the REST RULE, in one lane
    return tau


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n,K,E,base', [(130, 3, 64, 0), (200, 3, 64, 0), (320, 2, 128, 128)])
def test_population_statement_is_the_one_network_statement_per_env(dtype, n, K, E, base):
    """Per env the population's host statement equals BatchedNNAllocator of that env's network on that env's tau: bit for bit in
    float32 (the device's arithmetic), exactly in float64."""
    from ml4ca_amd.deploy import BatchedNNAllocator, BatchedNNAllocatorPopulation, nn_population_index, nn_population_stack
    nets = _nets(K)
    tau = _tau(n)
    pop = BatchedNNAllocatorPopulation(n, nets, envs_per_net=E, env_id_base=base, dtype=dtype)
    act, p = pop.allocate(tau, raw=True)
    assert act.dtype == dtype and act.shape == (n, 7) and p.shape == (n, 6)
    idx = nn_population_index(n, K, E, base)
    seen = 0
    for k in range(K):
        one_act, one_p = BatchedNNAllocator(n, nets[k], dtype=dtype).allocate(tau, raw=True)
        r = idx == k
        seen += int(r.sum())
        assert np.array_equal(_bits(act[r]), _bits(one_act[r])) and np.array_equal(_bits(p[r]), _bits(one_p[r])), k
    assert seen == n
    assert np.array_equal(act[5], [0, 0, 0, 0, 1, 0, 1]) and not np.array_equal(act[4], act[5])
    # the stacked dict is the same population
    act2 = BatchedNNAllocatorPopulation(n, nn_population_stack(nets), envs_per_net=E, env_id_base=base, dtype=dtype).allocate(tau)
    assert np.array_equal(_bits(act2), _bits(act))
    # ... and the networks are distinct: network 0 everywhere is another answer on network 1's envs
    if K > 1 and (idx == 1).any():
        assert not np.array_equal(BatchedNNAllocator(n, nets[0], dtype=dtype).allocate(tau)[idx == 1], act[idx == 1])


def test_index_map():
    from ml4ca_amd.deploy import nn_population_index
    i = nn_population_index(130, 3, 64)
    assert i.dtype == np.int64 and i.tolist() == [0] * 64 + [1] * 64 + [2] * 2
    # wrap-around: n > K E flies network 0 again behind K - 1
    i = nn_population_index(200, 3, 64)
    assert i.tolist() == [0] * 64 + [1] * 64 + [2] * 64 + [0] * 8
    i = nn_population_index(64 * 7, 2, 64)
    assert i[::64].tolist() == [0, 1, 0, 1, 0, 1, 0]
    # K larger than the wave count: the trailing networks go unused
    i = nn_population_index(130, 5, 64)
    assert sorted(set(i.tolist())) == [0, 1, 2]
    # E = 128: two waves per network
    i = nn_population_index(320, 2, 128)
    assert i[::64].tolist() == [0, 0, 1, 1, 0]
    # the global env id counts: a handle at env_id_base = 128 flies envs 128.. of the population
    assert np.array_equal(nn_population_index(128, 3, 64, env_id_base=128), nn_population_index(256, 3, 64)[128:])
    assert np.array_equal(nn_population_index(64, 2, 128, env_id_base=2 ** 40 + 64), [(2 ** 40 + 64) // 128 % 2] * 64)
    for bad in (dict(K=0), dict(envs_per_net=0), dict(envs_per_net=32), dict(envs_per_net=96), dict(env_id_base=32), dict(env_id_base=-64),
                dict(n=0)):
        with pytest.raises(ValueError):
            nn_population_index(**dict(dict(n=130, K=3, envs_per_net=64, env_id_base=0), **bad))


def test_stack_keeps_shapes_and_refuses_mixed_ones():
    from ml4ca_amd.deploy import nn_population_net, nn_population_stack
    nets = _nets(3)
    st = nn_population_stack(nets)
    assert [w.shape for w in st['W']] == [(3, 9, 20), (3, 20, 20), (3, 20, 20), (3, 20, 20), (3, 20, 6)]
    assert [b.shape for b in st['b']] == [(3, 20)] * 4 + [(3, 6)] and all(a.dtype == np.float32 for a in st['W'] + st['b'])
    for k in range(3):
        one = nn_population_net(st, k)
        assert all(np.array_equal(a, b) for a, b in zip(one['W'] + one['b'], nets[k]['W'] + nets[k]['b']))
    assert nn_population_stack(st) is st
    assert nn_population_stack([dict(n, leak=0.2) for n in nets])['leak'] == 0.2
    with pytest.raises(ValueError, match='one shape'):
        nn_population_stack(nets + [seeded_net((9, 17, 17, 6), seed=1)])
    with pytest.raises(ValueError, match='one shape'):
        nn_population_stack(nets + [seeded_net((3, 20, 20, 20, 20, 6), seed=1)])
    with pytest.raises(ValueError, match='one leak'):
        nn_population_stack([dict(nets[0], leak=0.0), dict(nets[1], leak=0.2)])
    with pytest.raises(ValueError):
        nn_population_stack([])
    with pytest.raises(ValueError):
        nn_population_stack(nets[0])                          # one net's dict is not a stack
    with pytest.raises(ValueError):
        nn_population_stack(dict(W=st['W'], b=[b[:2] for b in st['b']]))


def test_sweep_checks_its_arguments_before_it_touches_the_env():
    """The env here is a stand-in that has only what the checks read: anything past them would raise AttributeError, not ValueError."""
    from ml4ca_amd.evaluate import nn_allocator_sweep
    nets = _nets(2)
    env = lambda n, current=True: types.SimpleNamespace(n_envs=n, cfg=types.SimpleNamespace(current_enabled=current))
    with pytest.raises(ValueError, match='need an env of 128 envs'):
        nn_allocator_sweep(env(130), nets)
    with pytest.raises(ValueError, match='current=True'):
        nn_allocator_sweep(env(128, current=False), nets)
    with pytest.raises(ValueError, match='divide'):
        nn_allocator_sweep(env(128), nets, directions=24)
    with pytest.raises(ValueError, match='multiple of 64'):
        nn_allocator_sweep(env(96), nets, envs_per_net=48)
    with pytest.raises(ValueError, match='one shape'):
        nn_allocator_sweep(env(128), [nets[0], seeded_net((9, 7, 6), seed=1)])
    with pytest.raises(AttributeError):
        nn_allocator_sweep(env(128), nets)                    # the checks pass: the flight begins


def test_population_entry_points_are_declared_exported_and_bound():
    import os
    from ml4ca_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'dpenv.h')).read()
    _lib.load()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for name in ('dpenv_set_nn_allocator_population', 'dpenv_thrust_alloc_nn_population'):
        assert re.search(r'^int %s\(' % name, hdr, flags=re.M), name
        assert re.search(r' T %s$' % name, exported, flags=re.M), name
        assert name in _lib.SYMBOLS
    assert not re.search(r'launch_nn_\w*pop', exported), 'the cross-unit launchers stay out of the dynamic symbol table'
    assert len(_lib.SYMBOLS['dpenv_set_nn_allocator_population'][1]) == 5
    assert len(_lib.SYMBOLS['dpenv_thrust_alloc_nn_population'][1]) == 8
