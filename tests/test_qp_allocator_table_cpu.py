"""One QP allocator per env (include/dpenv.h: dpenv_set_qp_allocator_table, dpenv_thrust_alloc_qp_table) without a GPU: the public
table's slots in the header, the binding and deploy.py; the table's builder and its inverse; the per-env host law
(deploy.BatchedQPAllocator with a table) against the scalar one, bit for bit; and the weight population of the scored sweep."""
import os
import re

import numpy as np
import pytest

from tests.test_qp_allocator_cpu import wrench_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'WSLACK': 'w_slack', 'WPOWER': 'w_power', 'WDALPHA': 'w_dalpha', 'WDFORCE': 'w_dforce', 'FMAX': 'f_max', 'FRATE': 'force_rate',
         'ARATE': 'azimuth_rate', 'LX': 'lx', 'LY': 'ly', 'KF': 'kf', 'KR': 'kr'}


def _params(K=16, f32=False):
    """The defaults; f32: every number rounded to float32 first - what a table can hold, so the float64 law sees the same numbers."""
    from ml4ca_amd.deploy import qp_allocator_defaults
    p = qp_allocator_defaults()
    p['iterations'] = K
    if f32:
        p = {k: (v if k == 'iterations' else np.asarray(v, np.float32).astype(np.float64)) for k, v in p.items()}
    return p


def _distinct(n, seed=3):
    """n distinct parameter sets, every slot group different from env to env: (per-env dict with a leading n, list of scalar dicts)."""
    from ml4ca_amd.deploy import QP_SLOTS
    rng = np.random.default_rng(seed)
    base = _params(f32=True)
    per = {}
    for name, (_, width) in QP_SLOTS.items():
        b = np.asarray(base[name], np.float64).reshape(-1)
        f = rng.uniform(0.6, 1.6, (n, width))
        v = (b[None] * f + (b[None] == 0.0) * (f - 1.0)).astype(np.float32).astype(np.float64)   # (ly of the bow thruster is 0)
        per[name] = v[:, 0] if width == 1 else v
    rows = [dict({k: (float(v[i]) if v.ndim == 1 else v[i].copy()) for k, v in per.items()}, iterations=16) for i in range(n)]
    return per, rows


def test_slots_of_the_header_the_binding_and_deploy_agree():
    from ml4ca_amd import _lib
    from ml4ca_amd.deploy import QP_NPARAM, QP_SLOTS
    txt = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'^#define DPENV_QP_(\w+) (\d+)', txt, re.M)}
    assert defs.pop('NPARAM') == QP_NPARAM == 32
    assert {NAMES[k]: v for k, v in defs.items()} == {k: first for k, (first, _) in QP_SLOTS.items()}
    # the slots tile 0..25 without overlap, in the order of dpenv_qp_allocator's fields
    used = sorted(s for first, width in QP_SLOTS.values() for s in range(first, first + width))
    assert used == list(range(26))
    order = [k for k, _ in sorted(QP_SLOTS.items(), key=lambda kv: kv[1][0])]
    fields = [f[0] for f in _lib.QPAllocator._fields_ if f[0] not in ('struct_size', 'iterations')]
    assert order == fields
    lib = _lib.load()
    for name, nargs in (('dpenv_set_qp_allocator_table', 5), ('dpenv_thrust_alloc_qp_table', 11)):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert re.search(r'\bint %s\(' % name, txt)
    assert lib.dpenv_abi_version() == _lib.ABI_VERSION == 6


def test_table_round_trips_and_refuses_bad_shapes():
    from ml4ca_amd.deploy import QP_SLOTS, qp_allocator_table, qp_allocator_table_params
    n = 5
    per, rows = _distinct(n)
    tab = qp_allocator_table(n, **per)
    assert tab.shape == (32, n) and tab.dtype == np.float32 and not tab[26:].any()
    back = qp_allocator_table_params(tab, iterations=7)
    assert back['iterations'] == 7
    for name in QP_SLOTS:
        assert np.array_equal(back[name], per[name]), name
    assert np.array_equal(qp_allocator_table(n, **back), tab)
    # shared entries come from params, per-env ones override them
    p = _params()
    mixed = qp_allocator_table(n, p, w_power=per['w_power'])
    assert np.array_equal(mixed[3], per['w_power'].astype(np.float32))
    assert np.array_equal(mixed[6:9], np.repeat(np.asarray(p['f_max'], np.float32)[:, None], n, 1))
    assert np.array_equal(qp_allocator_table(n)[:26, 0], qp_allocator_table(1, p)[:26, 0])
    with pytest.raises(TypeError, match='unknown'):
        qp_allocator_table(n, w_pwr=np.ones(n))
    with pytest.raises(ValueError, match='shape'):
        qp_allocator_table(n, w_slack=np.ones((n, 2)))
    with pytest.raises(ValueError, match='shape'):
        qp_allocator_table(n, w_power=np.ones(n + 1))
    with pytest.raises(ValueError, match='entries'):
        qp_allocator_table(n, dict(p, kf=np.ones(2)))
    with pytest.raises(ValueError, match=r'\[32, n\]'):
        qp_allocator_table_params(np.zeros((31, n), np.float32))


def _walk(n, steps=40):
    """[steps, n, 3]: the random walk with rate-infeasible jumps, a per-env offset and scale."""
    rng = np.random.default_rng(11)
    seq = wrench_sequence(steps)
    return seq[:, None, :] * rng.uniform(0.5, 1.0, (1, n, 3)) + rng.uniform(-3.0, 3.0, (1, n, 3))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_law_with_equal_rows_is_the_scalar_law_bit_for_bit(dtype):
    """The table holds float32 numbers, so in float64 the scalar law is given the float32-rounded numbers too; in float32 both round the
    defaults the same way."""
    from ml4ca_amd.deploy import BatchedQPAllocator, qp_allocator_table
    n = 6
    p = _params(16, f32=dtype == np.float64)
    tab = qp_allocator_table(n, p)
    a, b = BatchedQPAllocator(n, p, 0.2, dtype), BatchedQPAllocator(n, tab, 0.2, dtype, iterations=16)
    assert b.iterations == 16 and b.ws.shape == (n, 3) and a.ws.shape == (3,)
    jumps = 0
    for tau in _walk(n):
        ya, yb = a.allocate(tau), b.allocate(tau)
        assert ya.dtype == yb.dtype == np.dtype(dtype)
        for u, v in ((ya, yb), (a.x, b.x), (a.last_x, b.last_x), (a.last_J, b.last_J)):
            assert u.shape == v.shape and np.array_equal(u, v, equal_nan=True) and u.tobytes() == v.tobytes()
        jumps += int((a.last_J[-1] > 1.0).any())
    assert jumps >= 1                                            # the rate-infeasible jump left a residual no solve could close


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_law_with_distinct_rows_is_one_scalar_law_per_env(dtype):
    from ml4ca_amd.deploy import BatchedQPAllocator, qp_allocator_table
    n = 8
    per, rows = _distinct(n)
    tab = qp_allocator_table(n, **per)
    assert all(len(np.unique(tab[s])) == n for s in range(26))   # every slot differs from env to env
    whole = BatchedQPAllocator(n, tab, 0.2, dtype)
    by_dict = BatchedQPAllocator(n, dict(per, iterations=16), 0.2, dtype)
    ones = [BatchedQPAllocator(1, rows[i], 0.2, dtype) for i in range(n)]
    for tau in _walk(n):
        y = whole.allocate(tau)
        assert by_dict.allocate(tau).tobytes() == y.tobytes()
        for i in range(n):
            yi = ones[i].allocate(tau[i:i + 1])
            assert yi.tobytes() == y[i:i + 1].tobytes(), i
            assert ones[i].x.tobytes() == whole.x[i:i + 1].tobytes() and ones[i].last_J.tobytes() == whole.last_J[:, i:i + 1].tobytes(), i
    assert len({whole.x[i].tobytes() for i in range(n)}) == n
    with pytest.raises(ValueError, match='shape'):
        BatchedQPAllocator(n + 1, tab, 0.2, dtype)


def test_weight_population():
    from ml4ca_amd.deploy import QP_SLOTS, qp_allocator_defaults, qp_weight_population
    base = qp_allocator_defaults()
    K, span = 9, 3.0
    pop = qp_weight_population(K, base, span=span, seed=4)
    what = ('w_power', 'w_dalpha', 'w_dforce')
    assert sorted(pop['factors']) == sorted(what)
    for name in what:
        f = pop['factors'][name]
        assert f.shape == (K,) and pop[name].shape == (K,)
        assert pop[name][0] == base[name] and f[0] == 1.0                               # row 0 is the base
        assert (f >= 1.0 / span).all() and (f <= span).all() and len(np.unique(f)) == K
        assert np.array_equal(pop[name], base[name] * f)
    for name in set(QP_SLOTS) - set(what):                                              # what it does not name is untouched
        assert pop[name] is base[name] or np.array_equal(pop[name], base[name])
    assert pop['iterations'] == base['iterations']
    again = qp_weight_population(K, base, span=span, seed=4)
    other = qp_weight_population(K, base, span=span, seed=5)
    for name in what:
        assert np.array_equal(again[name], pop[name]) and not np.array_equal(other[name], pop[name])
    vec = qp_weight_population(4, None, what=('w_slack', 'f_max'))
    assert vec['w_slack'].shape == (4, 3) and vec['factors']['f_max'].shape == (4, 3) and np.ndim(vec['w_power']) == 0
    assert np.array_equal(vec['w_slack'][0], base['w_slack'])
    assert np.array_equal(qp_weight_population(1)['w_power'], [base['w_power']])
    for bad in (dict(K=0), dict(K=3, span=0.5), dict(K=3, what=('kp',))):
        with pytest.raises(ValueError):
            qp_weight_population(**bad)
