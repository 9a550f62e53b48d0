"""Are the cases of tests/qp_edges.py fair?  (CPU only: deploy.BatchedQPAllocator in float32 and float64 - no kernel runs here.)  Everything
tests/test_gpu_qp_edges.py relies on is asserted here of the host law by itself, for every regime, at K in (1, 2, 16, 32).  The measured
figures are printed, and appended to the file the environment variable QP_EDGES_RECORD names, if it is set."""
import os

import numpy as np
import pytest

from tests import qp_edges as QE

RECORD = os.environ.get('QP_EDGES_RECORD', '')
F32, F64 = np.float32, np.float64


def test_the_regimes_are_the_issues_and_every_pinned_edge_is_met():
    R = QE.regimes()
    assert len(R) == 17 and set(QE.EXACT_ONLY) <= set(R) and set(QE.PREFIX_REGIMES) <= set(QE.well_conditioned())
    d = R['default']
    assert (d['kf'] == d['kr']).all() and d['kf'][1] == d['kf'][2] and d['lx'][1] == d['lx'][2]       # the symmetry `asym` is there to break
    a = R['asym']
    for name in ('w_slack', 'f_max', 'force_rate', 'lx', 'ly', 'kf', 'kr'):
        assert len(set(np.asarray(a[name]).tolist())) == 3, name
    assert a['azimuth_rate'][0] != a['azimuth_rate'][1] and (a['kf'] != a['kr']).all()
    for regime in R:
        S, tau = QE.inputs(regime)
        fmax = np.asarray(R[regime]['f_max'], F64).astype(F32)
        assert S.shape == (QE.N, 5) and tau.shape == (QE.N, 3) and S.dtype == F32 and tau.dtype == F32
        assert np.isfinite(S).all() and np.isfinite(tau).all() and (np.abs(S[:, :3]) <= fmax).all()
        lo, hi = QE.box(regime)
        assert (lo <= S).all() and (S <= hi).all() and np.array_equal(QE.canon(regime, QE.start(regime)).view(np.uint32), QE.canon(regime, S).view(np.uint32))
        for i in QE.lanes_with(0, 'top'):
            assert (S[i, :3] == fmax).all() and (S[i, :3] == hi[i, :3]).all()
        for i in QE.lanes_with(0, 'bottom'):
            assert (S[i, :3] == -fmax).all() and (S[i, :3] == lo[i, :3]).all()
        for i in QE.lanes_with(0, 'zeros'):
            assert (S[i, :3] == 0).all() and np.array_equal(np.signbit(S[i, :3]), [True, False, True])
        for i in QE.lanes_with(0, 'tiny'):
            assert (S[i, :3] == F32(1e-30) * fmax).all()
        for i in QE.lanes_with(1, 'ends'):
            assert S[i, 3] == -F32(np.pi) and S[i, 4] == np.nextafter(F32(np.pi), F32(0)) and S[i, 4] < F32(np.pi)
        for i in QE.lanes_with(1, 'range_edge'):
            assert S[i, 3] == 29999 and S[i, 4] == -31000 and not QE.lane_domain(regime)[i]
        for i in QE.lanes_with(1, 'far') + QE.lanes_with(1, 'turns'):
            assert (np.abs(S[i, 3:5]) > 2 * np.pi).all() and (np.abs(S[i, 3:5]) <= QE.AZ_LIMIT).all()
        over = QE.overflow_lanes(regime)
        for i in QE.lanes_with(2, 'overflow'):
            assert over[i] and np.isfinite(tau[i]).all()
        for i in QE.lanes_with(2, 'huge'):
            assert not over[i] and QE.wrench_class(regime)[i] == 1
        for i in QE.lanes_with(2, 'jump') + QE.lanes_with(2, 'jump_back'):
            assert not over[i] and QE.wrench_class(regime)[i] == 0 and (np.abs(tau[i]) == F32(10 * QE.TAU_MAX)).all()
        for i in QE.lanes_with(2, 'denormal'):
            assert 0 < tau[i, 2] < np.finfo(F32).tiny and np.signbit(tau[i, 0]) and not tau[i, :2].any()
        assert tau[QE.lanes_with(2, 'zero')].any() == False
        assert len(QE.lanes_with(2, 'overflow_x')) == 2
        # the pinned lanes sit at the first and last lane of each wave and at the tail
        assert {0, 63, 64, 127, 128, 129} <= set(QE.PINNED)
        assert 2 <= over.sum() <= 4 and QE.lane_domain(regime).sum() >= QE.N - 5
    # 1e19 overflows the float32 J only where w_slack lifts it past float32's range; with w_slack = 0 the J of such a lane is 0 * inf
    assert not QE.overflow_lanes('default')[65] and QE.overflow_lanes('track_heavy')[65]
    assert np.isnan(QE.solve('track_off', 1, F32)['J'][0][66])


@pytest.mark.parametrize('regime', QE.names())
def test_the_host_law_keeps_the_exact_properties(regime):
    """Inside [lo, hi] with no tolerance; J never increases; J64 of the float32 result is not above J64 of the start; overflow lanes hold the
    clipped start bit for bit and command a finite action; all_dead keeps the forces 0, all_frozen moves nothing."""
    from ml4ca_amd.deploy import BatchedQPAllocator
    S, tau = QE.inputs(regime)
    over = QE.overflow_lanes(regime)
    x0 = QE.start(regime)
    j0 = QE.J64(regime, x0)
    for K in QE.CPU_ITERATIONS:
        for dtype in (F32, F64):
            r = QE.solve(regime, K, dtype)
            x, J = r['x'], r['J']
            h = QE.host(regime, dtype, K)
            lo, hi = h.box(S.astype(dtype))
            assert x.dtype == dtype and (lo <= x).all() and (x <= hi).all()
            fin = np.isfinite(J[0])
            assert np.isfinite(J[:, fin]).all() and (J[1:, fin] <= J[:-1, fin]).all()
            assert r['accept'].shape == (K, QE.N) and r['frozen'].shape == (K, QE.N, 5) and r['trial_J'].shape == (K, QE.N)
            if dtype == F32:
                assert np.array_equal(fin, ~over)
                assert np.array_equal(x[over].view(np.uint32), x0[over].view(np.uint32)) and (x0 == S).all()       # (x0: signed zeros as canon() says)
                assert not r['accept'][:, over].any()
                h.x = S.copy()
                with np.errstate(all='ignore'):
                    act = h.allocate(tau)
                assert np.isfinite(act).all() and np.isfinite(h.x).all()
                excess = (QE.J64(regime, x) - j0)[fin]
                QE.record(RECORD, 'host   %-12s K %2d  J64(H32) - J64(x0): largest %.3g (of J up to %.3g)' % (regime, K, excess.max(), j0[fin].max()))
                assert (excess <= 0).all()
            if regime == 'all_dead':
                assert (x[:, :3] == 0).all()
            if regime == 'all_frozen':
                assert np.array_equal(QE.canon(regime, x).view(np.uint8), QE.canon(regime, S.astype(dtype)).view(np.uint8))
    # trace= changes nothing: the same solve without it, bit for bit
    with np.errstate(all='ignore'):
        x, J = BatchedQPAllocator(QE.N, QE.params(regime, 16), QE.DT, F32).solve(tau, S)
    r = QE.solve(regime, 16, F32)
    assert np.array_equal(x.view(np.uint32), r['x'].view(np.uint32)) and np.array_equal(J.view(np.uint32), r['J'].view(np.uint32))
    # the lane at rest stays where it is, signed zeros included
    if QE.keeps_signed_zeros(regime):
        assert np.array_equal(QE.solve(regime, 16, F32)['x'][QE.AT_REST].view(np.uint32), S[QE.AT_REST].view(np.uint32))


SWAPS = [('kf<->kr', None)] + [(name, name) for name in ('f_max', 'force_rate', 'azimuth_rate', 'lx', 'kf')]


@pytest.mark.parametrize('what,field', SWAPS)
def test_asym_tells_the_components_apart(what, field):
    """Swap kf and kr, or port and starboard in one field: the host law's answer (the action of one control step at K = 1) changes on at
    least 33 lanes of 130, so that agreeing with the host on `asym` can only mean no swap."""
    from ml4ca_amd.deploy import BatchedQPAllocator
    S, tau = QE.inputs('asym')
    p = QE.params('asym', 1)
    q = dict(p)
    if field is None:
        q['kf'], q['kr'] = p['kr'], p['kf']
    else:
        v = np.array(p[field], F64)
        v[-2:] = v[-2:][::-1].copy()                  # port <-> starboard: the last two entries of every field
        q[field] = v
    out = []
    for pp in (p, q):
        h = BatchedQPAllocator(QE.N, pp, QE.DT, F32)
        h.x = S.copy()
        with np.errstate(all='ignore'):
            act = h.allocate(tau)
        out.append(np.concatenate([act, h.x], 1))
    changed = (out[0].view(np.uint32) != out[1].view(np.uint32)).any(1)
    # ... and by more than rounding: further than the one-iteration bound of the GPU module, on the state or on the thrust columns
    far = (np.abs(out[0].astype(F64) - out[1]) / np.maximum(np.abs(out[0].astype(F64)), 1.0)).max(1) > QE.parity_bound('asym')
    QE.record(RECORD, 'swap   %-12s lanes changed %3d, beyond the parity bound %3d of %d' % (what, changed.sum(), far.sum(), QE.N))
    assert changed.sum() >= 33 and far.sum() >= 33


@pytest.mark.parametrize('regime', QE.names())
def test_the_two_host_laws_decide_alike_and_the_lanes_left_out_stay_under_the_cap(regime):
    """K = 1: float32 and float64 take the same accept decision and the same frozen set on at least 95 % of the lanes, and the
    one-iteration comparison leaves out no more than 5 % - in every well-conditioned regime.  Prints the regime's yardsticks."""
    a, b = QE.solve(regime, 1, F32), QE.solve(regime, 1, F64)
    m = QE.lane_domain(regime)
    same = (a['accept'][0] == b['accept'][0]) & (a['frozen'][0] == b['frozen'][0]).all(1)
    out = QE.left_out(regime)
    err = QE.parity_err(a['x'], b['x'])
    worst_all = float(err[m].max())
    line = 'parity %-12s same decisions %5.1f %%  left out %2d  ' % (regime, 100.0 * same[m].mean(), out.sum())
    if 'parity' not in QE.domain(regime):
        QE.record(RECORD, line + 'float32 against float64 host iterate, every in-domain lane: %.3g  (exact only)' % worst_all)
        return
    yard = QE.parity_yardstick(regime)
    QE.record(RECORD, line + 'yardstick %.3g  bound %.3g  (every in-domain lane: %.3g)' % (yard, QE.parity_bound(regime), worst_all))
    assert same[m].mean() >= 0.95
    assert out.sum() <= QE.CAP * QE.N
    assert np.isfinite(yard) and yard < 1e-3                      # a yardstick this side of it still tells a swap from rounding
    for K in (16, 32):
        yj, j64 = QE.objective_yardstick(regime, K)
        QE.record(RECORD, 'object %-12s K %2d  yardstick max |J64(H32) - J64(H64)| %.3g (nominal wrenches) %.3g (huge), J up to %.4g / %.4g' % (
            regime, K, yj[QE.wrench_class(regime) == 0].max(), yj[QE.wrench_class(regime) == 1].max(),
            j64[m & (QE.wrench_class(regime) == 0)].max(), j64[m & (QE.wrench_class(regime) == 1)].max()))
        assert np.isfinite(yj).all()


def test_the_roundings_counted():
    assert QE.KC == 96 and QE.KC * 2.0 ** -24 < 6e-6
