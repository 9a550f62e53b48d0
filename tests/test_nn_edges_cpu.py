"""Are the cases of tests/nn_edges.py fair?  (CPU only: the host statements deploy.BatchedNNAllocator, _num._fma32, train.alloc_loss_terms,
train.allocation_grad_ref and torch autograd - no kernel runs here.)  Everything tests/test_gpu_nn_edges.py relies on is asserted here:
the covering set covers what it says, the guard bands surround every view, the subnormal nets do produce subnormal non-zero values and
_fma32 is the exact fmaf there, the wire network hands its inputs through as bits, the running bound of the allocation loss holds the
float32 evaluation of the law and is not vacuous, and autograd's conventions at the kinks are the header's."""
import numpy as np
import pytest

import tests.test_gpu_nn_allocator as GN
import tests.test_nn_allocator_cpu as NC
from ml4ca_amd import _num, deploy
from ml4ca_amd import train as TR
from tests import nn_edges as NE
from tests.test_allocation_loss_cpu import torch_alloc_loss
from tests.test_imitation_cpu import rel_errors, slices

F32, F64 = np.float32, np.float64


# ---- A. the allocator ----
def test_the_covering_set_covers_what_the_issue_lists():
    S = NE.SHAPES
    assert len(S) == len(set(S)) == 30
    for sizes, leak in S:
        net = NE.net_for(sizes)
        assert deploy.nn_net_sizes(net['W'], net['b']) == list(sizes) and leak in NE.LEAKS
    assert {s[1] for s, _ in S} == set(NE.WIDTHS) == {1, 15, 16, 17, 31, 32, 33, 48, 79, 81, 95, 96}
    assert {(s[0], s[1]) for s, _ in NE.LOOP_SHAPES} == {(i, h) for i in (3, 9) for h in NE.WIDTHS} and len(NE.LOOP_SHAPES) == 24
    cls = lambda s: NE.width_class(s[1])
    assert NE.width_class(1) == NE.width_class(15) == 'small' and NE.width_class(96) == 'top' and NE.width_class(16) == 'other'
    assert all(NE.width_class(h) == 'plus1' for h in (17, 33, 81))
    for c in ('small', 'plus1', 'top'):
        assert {len(s) - 1 for s, _ in S if cls(s) == c} == {2, 3, 4, 5}, c              # every depth ...
        assert {s[0] for s, _ in S if cls(s) == c} == {3, 9}, c                            # ... and both input widths meet the class
    assert {(len(s) - 1, s[0]) for s, _ in S if s[1] == 96} == {(d, i) for d in (2, 3, 4, 5) for i in (3, 9)}
    assert {leak for _, leak in S} == {0.0, 0.2, 1.0}
    for leak in (0.2, 1.0):                                                             # each leak at a partial chunk and at a full one
        assert {cls(s) for s, l in S if l == leak} >= {'small', 'plus1', 'top'}, leak
    assert [s[1] for s in NE.GUARD_SHAPES] == [1, 17, 96] and {s[0] for s in NE.GUARD_SHAPES} == {3, 9}
    assert NE.IMAGE_ORDER == ((9, 96, 96, 96, 96, 6), (3, 1, 6), (9, 17, 17, 6))
    assert {s[0] for s in NE.CONSTANT_SHAPES} == {3, 9}
    c = NE.CONSTANTS
    assert {c['scaled']['leak'], c['fixed']['leak']} == {0.2, 1.0} and c['scaled']['angle_scale'] == 0.5 and c['fixed']['azimuth_mode'] == 1
    assert all(np.pi < abs(a) < 3.0e4 for a in c['fixed']['azimuth'])
    assert GN.N_FREE == 193 and NE.NN_CHUNK == 16


@pytest.mark.parametrize('case', NE.SHAPES, ids=NE.shape_id)
def test_host_statement_holds_its_running_bound_at_every_shape(case):
    """tests/test_nn_allocator_cpu.py's float32-against-float64 check of the host statement, at the covering set's shapes and leaks."""
    sizes, leak = case
    NC.test_float32_statement_stays_within_its_running_error_bound(sizes, leak, 1.0)


@pytest.mark.parametrize('sizes', NE.CONSTANT_SHAPES)
def test_every_constant_reaches_the_host_statement(sizes):
    tau = GN.free_tau()
    net = NE.net_for(sizes, scale=3.0)
    base = deploy.BatchedNNAllocator(len(tau), net).allocate(tau)
    for name, consts in NE.CONSTANTS.items():
        full = deploy.nn_allocator_params(net, **consts)
        ref = deploy.BatchedNNAllocator(len(tau), net, params=full).allocate(tau)
        assert not np.array_equal(ref, base), name
        for k in consts:
            if k == 'in_const' and sizes[0] == 3:
                continue                                                               # (the three-input form does not read it)
            if k == 'azimuth_mode':
                continue                                                               # (its partner `azimuth` is read in mode 1 alone)
            less = dict(full)
            less[k] = deploy.nn_allocator_defaults()[k]
            assert not np.array_equal(deploy.BatchedNNAllocator(len(tau), net, params=less).allocate(tau), ref), (name, k)


@pytest.mark.parametrize('sizes', NE.GUARD_SHAPES)
def test_guard_bands_surround_every_view(sizes):
    net = NE.net_for(sizes)
    block, views = NE.guarded(net)
    parts = [a for pair in zip(net['W'], net['b']) for a in pair]
    inside = np.zeros(block.size, bool)
    for (o, shape), a in zip(views, parts):
        n = int(np.prod(shape))
        assert np.array_equal(block[o:o + n].reshape(shape), a) and not inside[o:o + n].any()
        assert np.isnan(block[o - NE.NN_CHUNK:o]).all() and np.isnan(block[o + n:o + n + NE.NN_CHUNK]).all()
        inside[o:o + n] = True
    assert np.isnan(block[~inside]).all() and np.isfinite(block[inside]).all()


def _forward_sub(sizes, kind):
    tau = GN.free_tau()
    net = NE.subnormal_net(sizes, kind)
    a = deploy.BatchedNNAllocator(len(tau), net, params=dict(deploy.nn_allocator_defaults(), leak=NE.SUB_LEAK))
    _, x = a.inputs(tau)
    p, hs = a.forward(x)
    lanes = np.isfinite(tau).all(1)
    return a, net, p[lanes], [h[lanes] for h in hs]


def _subnormal(v):
    v = np.abs(np.asarray(v, F64))
    return (v > 0) & (v < NE.TINY)


@pytest.mark.parametrize('sizes', NE.SUB_SHAPES)
def test_subnormal_nets_produce_subnormal_values_in_the_host_statement(sizes):
    for kind in NE.SUB_SCALES:
        a, net, p, hs = _forward_sub(sizes, kind)
        assert all(np.isfinite(w).all() and w.any() for w in net['W']), kind
        hidden = np.concatenate([h.reshape(-1) for h in hs[1:]])
        n_sub_h, n_sub_p = int(_subnormal(hidden).sum()), int(_subnormal(p).sum())
        print('%s %s: %d of %d hidden activations and %d of %d outputs subnormal and non-zero; %d outputs zero' % (
            sizes, kind, n_sub_h, hidden.size, n_sub_p, p.size, int((p == 0).sum())))
        if kind == 'edge':                                   # around 2^-126: both sides of the boundary, and leak * y below it
            assert n_sub_h > hidden.size // 10 and (np.abs(hidden) >= NE.TINY).sum() > hidden.size // 10
            assert n_sub_p > p.size // 10
        elif kind == 'deep':                                 # normal operands, subnormal results
            assert n_sub_h == 0 and (hidden != 0).all() and n_sub_p > p.size // 2
        else:                                                # below 2^-150: signed zeros (and at most the smallest subnormals)
            assert (hidden != 0).all() and (np.abs(p) <= 2.0 ** -148).all() and (p == 0).sum() > p.size // 2
            assert np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()


@pytest.mark.parametrize('sizes', NE.SUB_SHAPES)
def test_fma32_is_the_exact_fmaf_in_the_subnormal_range(sizes):
    """The last layer's chains of four lanes, every output and every k, and the first hidden layer's of `edge`: _num._fma32 against the
    exact rational product-sum rounded once (nearest even, gradual underflow)."""
    from fractions import Fraction
    checked = sub = 0
    for kind in NE.SUB_SCALES:
        a, net, p, hs = _forward_sub(sizes, kind)
        layers = [len(net['W']) - 1] + ([0] if kind == 'edge' else [])
        for l in layers:
            W, b, h = a.Ws32[l], a.bs32[l], hs[l]
            for lane in (4, 5, 6, 7):
                for j in range(min(W.shape[1], 6)):
                    y = b[j]
                    for k in range(W.shape[0]):
                        want = NE.round_f32(Fraction(float(W[k, j])) * Fraction(float(h[lane, k])) + Fraction(float(y)))
                        got = _num._fma32(W[k, j], h[lane, k], y)[0]
                        assert got.view(np.uint32) == want.view(np.uint32), (kind, l, lane, j, k, got, want)
                        y = got
                        checked += 1
                        sub += bool(_subnormal(got))
                    if l == len(net['W']) - 1:
                        assert y.view(np.uint32) == p[lane, j].view(np.uint32)
    print('%s: %d fmaf checked against the exact rational value, %d with a subnormal non-zero result' % (sizes, checked, sub))
    assert sub > 100
    # the rational rounding itself, at the places that matter
    assert NE.round_f32(Fraction(3, 2) * Fraction(2) ** -149) == F32(2.0 ** -148) and NE.round_f32(Fraction(1, 2) * Fraction(2) ** -149) == 0
    assert NE.round_f32(Fraction(5, 2) * Fraction(2) ** -149) == F32(2.0 ** -148) and NE.round_f32(-Fraction(2) ** -150 * Fraction(3, 2)) == -F32(2.0 ** -149)
    assert NE.round_f32(Fraction(1) + Fraction(2) ** -24) == F32(1.0) and NE.round_f32(Fraction(1) + Fraction(3) * Fraction(2) ** -24) == F32(1.0 + 2.0 ** -22)


# ---- B. the allocation loss ----
def _same_or_both_zero(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def test_the_wire_hands_its_inputs_through_as_bits():
    """p == x[:, :6] for every case row and every row of the whole-gradient fixture, in the float32 fmaf statement and in _forward64."""
    names, P = NE.case_rows()
    assert len(names) == len(set(names)) == len(P) == 1 + 3 * len(NE.THRUST_VALUES) + len(NE.ANGLE_VALUES) + 2
    assert set(NE.KEY_ROWS) <= set(names)
    fx = NE.kink_fixture()
    for p in (P, fx['p']):
        x = NE.wire_x(p)
        assert np.array_equal(x[:, :6].view(np.uint32), p.view(np.uint32))
        got32, _ = deploy.BatchedNNAllocator(len(p), NE.wire_net()).forward(x)
        assert got32.dtype == F32 and _same_or_both_zero(got32, p)
        got64 = TR._forward64(NE.wire_theta(), x, 9, 6, True, 0.0)[5]
        assert np.array_equal(got64, p.astype(F64))
    # the flat vector is the layers
    Ws, bs, _ = TR.unflatten(NE.wire_theta(), 9, 6, True)
    assert all(np.array_equal(a, b) for a, b in zip(Ws, NE.wire_layers()[0])) and not any(b.any() for b in bs)


def test_the_case_rows_sit_where_they_say():
    names, P = NE.case_rows()
    one = F32(1.0)
    assert NE.OUT_P > one and NE.OUT_P - one == NE.E_OUT == F32(2.0 ** -23) and -NE.OUT_M - one == NE.E_OUT and NE.IN_P < one
    assert np.abs(NE.OUT_P) - one == 2.0 ** -23                                          # |p| - 1 is exact there
    vals = dict(NE.THRUST_VALUES)
    assert np.signbit(vals['-0']) and not np.signbit(vals['+0']) and vals['-0'] == 0
    assert 0 < vals['+2^-140'] < NE.TINY == vals['+2^-126']
    asc = F32(deploy.alloc_loss_defaults()['angle_scale'])
    assert 2.9999e4 < F32(NE.BIG_ANGLE * asc) < 3.0e4 and F64(NE.BIG_ANGLE) * F64(asc) < 3.0e4
    q = NE.config('base')[1]
    assert (np.asarray(q['kr']) != np.asarray(q['kf'])).all() and F32(q['w_sat']) == 100 and F32(q['w_power']) == F32(0.05)
    taus = NE.tau_cases()
    assert not taus['zero'].any() and np.array_equal(taus['+max'], -taus['-max']) and (np.abs(taus['interior']) < taus['+max']).all()
    L = NE.launches()
    assert len(L) == len(set(L)) and 100 <= len(L) <= 200
    for c in NE.CONFIGS:
        assert sum(1 for k, _ in L if k == c) == (len(names) if c == 'base' else len(NE.KEY_ROWS))
    assert {NE.config(c)[0]['mode'] for c in NE.CONFIGS} == {0, 1} and {NE.config(c)[0]['weight'] for c in NE.CONFIGS} == {None, 2.0, 0.0}
    assert {NE.config(c)[0]['tau'] for c in NE.CONFIGS} == set(taus) and {NE.config(c)[0]['w_power'] for c in NE.CONFIGS} == {0.0, 0.05}


def _host_rows(tracked):
    """the law on every launch of the GPU test, config by config: {(config, row): (dp, stats[, dp_err, stats_err])}"""
    names, P = NE.case_rows()
    taus = NE.tau_cases()
    out = {}
    for cfg in NE.CONFIGS:
        c, q = NE.config(cfg)
        rows = [r for k, r in NE.launches() if k == cfg]
        p = P[rows]
        tau = np.broadcast_to(taus[c['tau']], (len(rows), 3))
        w = None if c['weight'] is None else np.full(len(rows), c['weight'], F32)
        out[cfg] = (rows, p, tau, q, w, NE.alloc_law(p, tau, q, w, tracked=tracked))
    return out


def test_the_tracked_values_are_alloc_loss_terms():
    for cfg, (rows, p, tau, q, w, law) in _host_rows(True).items():
        ref_dp, ref_st = NE.reference(p, tau, q, w)
        for got, ref in ((law['dp'], ref_dp), (law['stats'], ref_st)):
            assert (np.abs(got - ref) <= 1e-13 * np.maximum(np.abs(ref), 1e-290) + 1e-300).all(), cfg
        assert np.isfinite(law['dp_err']).all() and np.isfinite(law['stats_err']).all() and (law['dp_err'] >= 0).all()


def test_the_float32_law_lies_inside_the_running_bound_and_differs_from_float64():
    worst = dict.fromkeys(NE.QUANTITIES, 0.0)
    differs = 0
    res = {}
    with np.errstate(under='ignore'):
        rows32 = _host_rows(False)
    for cfg, (rows, p, tau, q, w, law) in rows32.items():
        assert law['dp'].dtype == law['stats'].dtype == F32
        share, ok = NE.shares(law['dp'], law['stats'], p, tau, q, w)
        ref_dp, ref_st = NE.reference(p, tau, q, w)
        differs += int((law['dp'].astype(F64) != ref_dp).any(1).sum())
        for k in share:
            worst[k] = max(worst[k], share[k])
        assert ok.all(), (cfg, [(NE.case_rows()[0][rows[i]], j) for i, j in zip(*np.nonzero(~ok))])
        for i, r in enumerate(rows):
            res[(cfg, r)] = (law['dp'][i], law['stats'][i])
    print('float32 NumPy evaluation of the law, largest share of the running bound: ' + ', '.join('%s %.3f' % kv for kv in worst.items()))
    assert differs > len(res) // 2                                                       # not vacuous: float32 is not float64 here
    assert all(0.0 < v <= 1.0 for k, v in worst.items() if k != 'Jx')
    assert worst['Jx'] == 0.0                                                            # every term of Jx is exact at these rows: exact_properties holds it to the bit
    NE.exact_properties(res)                                                             # the header's kinks, in the host float32 law


def test_autograd_takes_the_headers_side_at_every_kink():
    """The whole-gradient fixture: float64 autograd = allocation_grad_ref on all 130 rows and on the first 1 and 65 - clamp's inclusive
    bounds are |p| <= 1, d|n|/dn = 0 at 0 meets dF = 0 there, relu's slope at z = 0 is leak on both sides - so no row of
    tests/test_gpu_nn_edges.py's whole-gradient test needs another reference."""
    fx = NE.kink_fixture()
    assert fx['x'].shape == (NE.B2_ROWS, 9) and fx['kinks'][::3].all() and fx['kinks'].sum() == 44
    a = np.abs(fx['p'][~fx['kinks'], :3])
    assert (np.abs(a - 1) >= 1e-3).all() and (a >= 1e-3).all()
    vals = {float(v) for _, v in NE.THRUST_VALUES}
    assert all(float(v) in vals for v in fx['p'][fx['kinks'], :3].reshape(-1))
    assert (fx['weight'][[0, 64, 128]] > 0).all() and (fx['weight'] == 0).any()
    sls = slices(9, 6)
    for mode in (0, 1):
        q = NE.loss_params(mode)
        for count in NE.B2_COUNTS:
            rows = np.arange(count)
            g, s = TR.allocation_grad_ref(fx['theta'], fx['x'][rows], fx['tau'][rows], q, weight=fx['weight'][rows], leak=0.0)
            tg, ts = torch_alloc_loss(fx['theta'], fx['x'], fx['tau'], q, weight=fx['weight'], rows=rows, leak=0.0)
            for name, err in rel_errors(g, tg, sls).items():
                assert err <= 1e-10, (mode, count, name, err)
            assert np.abs(s - ts).max() <= 1e-10 * np.abs(ts).max()
            assert all(np.abs(tg[sl]).max() > 0 for _, sl in sls[:-1]), (mode, count)
