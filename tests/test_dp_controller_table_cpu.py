"""Host side of the per-env controller table (include/dpenv.h dpenv_set_dp_controller_table): the batched allocation matrix against
the one-row recipe bit for bit, the table's slot order against the header's defines, the per-env host law against the shared one, the
Pareto front against its definition, the gain population, and the new symbol in header, library and binding table."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'dpenv.h')).read()


def _draw_geometry(rng, n):
    """Lever arms the defaults x (1 +- 0.1 u), weights log-uniform in [0.25, 4]."""
    from ml4ca_amd.deploy import dp_controller_defaults
    p = dp_controller_defaults()
    lx = p['lx'][None] * (1.0 + 0.1 * rng.uniform(-1, 1, (n, 3)))
    ly = p['ly'][None] * (1.0 + 0.1 * rng.uniform(-1, 1, (n, 3)))
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), (n, 5)))
    return lx, ly, w


def test_batched_allocation_matrix_equals_the_one_row_recipe_bit_for_bit():
    from ml4ca_amd.deploy import allocation_matrix, allocation_matrix_batched
    n = 2000
    lx, ly, w = _draw_geometry(np.random.RandomState(11), n)
    G = allocation_matrix_batched(lx, ly, w)
    assert G.shape == (n, 5, 3) and G.dtype == np.float64
    for i in range(n):                                                                 # no row is near singular: none is skipped
        want = allocation_matrix(lx[i], ly[i], w[i])
        assert np.array_equal(G[i].view(np.uint64), want.view(np.uint64)), i
    # a singular row (T of rank 2: lx all equal, ly port = star; every product exact in f64) and a bad weight are refused like the one-row form
    import pytest
    with pytest.raises(ValueError, match='singular'):
        allocation_matrix([1.0, 1.0, 1.0], [0.0, 0.5, 0.5])
    with pytest.raises(ValueError, match='singular'):
        allocation_matrix_batched(np.ones((2, 3)), np.full((2, 3), 0.5), np.ones((2, 5)))
    with pytest.raises(ValueError, match='weights'):
        allocation_matrix_batched(lx[:2], ly[:2], np.array([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], float))
    bad = allocation_matrix_batched(np.ones((2, 3)), np.full((2, 3), 0.5), np.ones((2, 5)), check=False)
    assert not np.isfinite(bad).all()


def test_table_slots_are_the_headers_defines():
    from ml4ca_amd import deploy
    defs = {k: int(v) for k, v in re.findall(r'#define\s+DPENV_CTRL_(\w+)\s+(\d+)', _header())}
    assert defs.pop('NPARAM') == 32 == deploy.CTRL_NPARAM
    names = dict(KP='kp', KD='kd', KI='ki', ZB='z_bound', TMAX='tau_max', WEIGHT='weight', LX='lx', LY='ly', KF='kf', KR_BOW='kr_bow',
                 F_EPS='f_eps')
    assert set(defs) == set(names)
    assert {names[k]: v for k, v in defs.items()} == {k: first for k, (first, _) in deploy.CTRL_SLOTS.items()}
    # the slots tile 0..30 without overlap, 31 is reserved
    used = sorted(s for first, width in deploy.CTRL_SLOTS.values() for s in range(first, first + width))
    assert used == list(range(31))
    # defaults are broadcast ...
    n = 7
    p = deploy.dp_controller_defaults()
    tab = deploy.dp_controller_table(n)
    assert tab.shape == (32, n) and tab.dtype == np.float32
    for name, (first, width) in deploy.CTRL_SLOTS.items():
        want = np.asarray(p[name], np.float64).reshape(-1).astype(np.float32)
        assert np.array_equal(tab[first:first + width], np.repeat(want[:, None], n, 1)), name
    assert np.all(tab[31] == 0)
    # ... and overrides land in their slots, every other slot as before
    rng = np.random.RandomState(2)
    over = {name: rng.uniform(0.5, 2.0, (n, width) if width > 1 else (n,)) for name, (_, width) in deploy.CTRL_SLOTS.items()}
    for name, (first, width) in deploy.CTRL_SLOTS.items():
        one = deploy.dp_controller_table(n, p, **{name: over[name]})
        assert np.array_equal(one[first:first + width], over[name].reshape(n, width).T.astype(np.float32)), name
        rest = np.ones(32, bool)
        rest[first:first + width] = False
        assert np.array_equal(one[rest], tab[rest]), name
    import pytest
    with pytest.raises(TypeError):
        deploy.dp_controller_table(n, G=np.zeros((n, 5, 3)))
    with pytest.raises(ValueError):
        deploy.dp_controller_table(n, kp=np.zeros((n + 1, 3)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_per_env_host_law_equals_the_shared_form_and_one_env_controllers():
    from ml4ca_amd import deploy
    n, steps = 37, 50
    rng = np.random.RandomState(4)
    p = deploy.dp_controller_defaults()
    obs = (rng.normal(0.0, 1.0, (steps, n, 9)) * (3.0, 3.0, 0.5, 0.5, 0.5, 0.1, 1, 1, 1)).astype(np.float32)
    obs[5, :4, :6] = 0.0                                                               # the (0, 1) direction branch
    # all rows equal: the shared form, bit for bit, from a table and from a dict with a leading n
    shared = deploy.BatchedDPController(n, p)
    tab = deploy.dp_controller_table(n, p)
    as_dict = {k: np.repeat(np.asarray(p[k], np.float64)[None], n, 0) for k in ('kp', 'kd', 'ki', 'z_bound', 'tau_max', 'G', 'kf')}
    as_dict.update(kr_bow=np.full(n, p['kr_bow']), f_eps=np.full(n, p['f_eps']))
    forms = [deploy.BatchedDPController(n, tab), deploy.BatchedDPController(n, as_dict)]
    for t in range(steps):
        want = shared.act(obs[t])
        for c in forms:
            got = c.act(obs[t])
            assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), t
            assert np.array_equal(_bits(c.z), _bits(shared.z)), t
    assert (np.abs(shared.z) == np.float32(p['z_bound'])).any() and (shared.z != 0).all(0).all()
    # distinct rows: env i is a one-env controller with row i
    lx, ly, w = _draw_geometry(rng, n)
    f = lambda lo, hi, k: np.exp(rng.uniform(np.log(lo), np.log(hi), (n, k)))
    tab = deploy.dp_controller_table(n, p, kp=p['kp'] * f(0.25, 4, 3), kd=p['kd'] * f(0.25, 4, 3), ki=p['ki'] * f(0.25, 4, 3),
                                     z_bound=p['z_bound'] * f(0.5, 2, 3), tau_max=p['tau_max'] * f(0.5, 2, 3), weight=w, lx=lx, ly=ly,
                                     kf=p['kf'] * f(0.5, 2, 3), kr_bow=p['kr_bow'] * f(0.5, 2, 1)[:, 0], f_eps=np.full(n, 1e-3))
    per = deploy.BatchedDPController(n, tab)
    assert per.G.shape == (n, 5, 3) and per.G.dtype == np.float32
    ones = [deploy.BatchedDPController(1, np.ascontiguousarray(tab[:, i:i + 1])) for i in range(n)]
    for i in (0, n - 1):                                                               # ... whose G is the one-row recipe's, rounded once
        want = deploy.allocation_matrix(tab[20:23, i], tab[23:26, i], tab[15:20, i]).astype(np.float32)
        assert np.array_equal(_bits(per.G[i]), _bits(want))
    for t in range(steps):
        got = per.act(obs[t])
        for i in range(n):
            assert np.array_equal(_bits(got[i:i + 1]), _bits(ones[i].act(obs[t, i:i + 1]))), (t, i)
    for i in range(n):
        assert np.array_equal(_bits(per.z[i:i + 1]), _bits(ones[i].z))
    assert len({got[i].tobytes() for i in range(n)}) == n


def _front_by_definition(a, b):
    keep = []
    for i in range(len(a)):
        if not any(a[j] <= a[i] and b[j] <= b[i] and (a[j] < a[i] or b[j] < b[i]) for j in range(len(a))):
            keep.append(i)
    return sorted(keep, key=lambda i: (a[i], b[i], i))


def test_pareto_front_equals_the_definition():
    from ml4ca_amd.evaluate import pareto_front
    rng = np.random.RandomState(6)
    for trial in range(20):
        m = int(rng.randint(1, 60))
        if trial % 2:                                                                  # a coarse grid: ties in a, in b, and duplicates
            a, b = rng.randint(0, 6, m).astype(float), rng.randint(0, 6, m).astype(float)
        else:
            a, b = rng.uniform(0, 1, m), rng.uniform(0, 1, m)
        got = pareto_front(a, b)
        assert got.tolist() == _front_by_definition(a, b), trial
        assert np.all(np.diff(a[got]) >= 0)
    assert pareto_front([1.0, 1.0, 2.0, 0.5], [1.0, 1.0, 0.5, 3.0]).tolist() == [3, 0, 1, 2]   # duplicates are both kept
    assert pareto_front([1.0, 1.0], [2.0, 1.0]).tolist() == [1]
    assert pareto_front([3.0], [4.0]).tolist() == [0]


def test_gain_population():
    from ml4ca_amd import deploy
    base = deploy.dp_controller_defaults()
    K, span = 64, 4.0
    pop = deploy.gain_population(K, base, span=span, seed=3)
    for name in ('kp', 'kd', 'ki'):
        f = pop['factors'][name]
        assert pop[name].shape == (K, 3) and f.shape == (K, 3)
        assert np.array_equal(pop[name][0], np.asarray(base[name], np.float64))       # row 0 is the base itself
        assert f.min() >= 1.0 / span and f.max() <= span and np.all(f[0] == 1.0)
        assert np.array_equal(pop[name], np.asarray(base[name])[None] * f)
        assert f[1:].min() < 0.5 and f[1:].max() > 2.0                                 # ... and the span is used
    for name in ('z_bound', 'tau_max', 'kf', 'lx', 'ly', 'weight'):
        assert np.array_equal(pop[name], base[name])
    again, other = deploy.gain_population(K, base, span=span, seed=3), deploy.gain_population(K, base, span=span, seed=4)
    assert all(np.array_equal(pop[k], again[k]) for k in ('kp', 'kd', 'ki')) and not np.array_equal(pop['kp'], other['kp'])
    only = deploy.gain_population(5, base, span=2.0, what=('ki',))
    assert only['ki'].shape == (5, 3) and np.array_equal(only['kp'], base['kp']) and set(only['factors']) == {'ki'}
    # the population goes into a table: gain set k in column k
    tab = deploy.dp_controller_table(K, {k: v for k, v in pop.items() if k not in ('kp', 'kd', 'ki')}, kp=pop['kp'], kd=pop['kd'], ki=pop['ki'])
    assert np.array_equal(tab[0:3], pop['kp'].T.astype(np.float32)) and np.array_equal(tab[:, 0], deploy.dp_controller_table(1, base)[:, 0])


def test_abi_declares_exports_and_binds_the_table_call():
    from ml4ca_amd import _lib
    name = 'dpenv_set_dp_controller_table'
    decl = re.search(r'^int %s\(([^;]*)\);' % name, _header(), re.M)
    assert decl and decl.group(1).count(',') == 3
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r' T %s$' % name, nm, re.M)
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 4
    lib = _lib.load()
    assert lib.dpenv_set_dp_controller_table(None, None, None, None) == _lib.EINVAL    # a NULL handle
    assert lib.dpenv_abi_version() == 6
