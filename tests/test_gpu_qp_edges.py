"""The rate-limited QP thrust allocation at the edges of its numbers (-m gpu): policy.thrust_alloc_qp (dpenv_thrust_alloc_qp and
dpenv_thrust_alloc_qp_table) on the regimes and lanes of tests/qp_edges.py against the FLOAT64 host law, deploy.BatchedQPAllocator.

Every regime is flown twice per iteration count K: alone in the scalar form, and all 17 side by side in one launch of the table form,
regime r on lanes 130 r .. 130 r + 129 (2 210 lanes, the largest launch here).

  1  exact properties        no tolerance: finite, inside the box of the device's own input, the thrust columns the stated map of state_out
                             in bits with the regime's own kf and kr, heads within 2e-7, overflow lanes hold, dead thrusters stay at 0,
                             frozen ones where they are, the table form the scalar form in bits.
  2  the loop's prefix       K = 1 .. 32 from the same inputs: cost_out never rises, equal costs mean equal bits, other costs another state.
                             No host number enters: the run-time iteration count and the accept / reject selects.
  3  never worse than holding  J64(D) <= J64(x0) + slack, and cost_out is J64(D) to 1e-5 of 1 + J.  The slack is the float32 evaluation
                             error of J measured on the host law (tests/qp_edges.py derives it); the host law itself needs none.
  4  one-iteration parity    K = 1, the check a self-correcting solver cannot absorb: the device's iterate against the float64 host iterate
                             within max(4 x the float32 host law's own error, KC 2^-24), KC = 96 roundings along one iteration's longest
                             chain (counted in tests/qp_edges.py).  On `asym` this is the anchor against any swap of two components.
  5  the objective reached   K = 16, 32: |J64(D) - J64(H64)| <= 4 max |J64(H32) - J64(H64)| + 1e-6 (1 + J64(H64)), the yardstick of
                             tests/test_gpu_qp_allocator.py taken per regime (and per wrench class: a lane whose J is 1e12 sets no
                             allowance for a lane whose J is 10).
  6  S(q, a) on `asym`       the labelling scan's state from a flown action row, kf and kr both in play.
Lanes leave 3 - 5 by the host law's evidence alone (qp_edges.lane_domain, qp_edges.left_out), never by what the device returned.
tests/test_qp_edges_cpu.py holds what these lean on.  Every measured figure is printed, and appended to the file the environment variable
QP_EDGES_RECORD names, if it is set (DESIGN.md section 7 holds such a record)."""
import os

import numpy as np
import pytest
import torch            # before anything loads libdpenv.so, as in every other GPU test module: the process then has one HIP runtime, torch's

from tests import helpers as H
from tests import qp_edges as QE
from tests.test_gpu_qp_allocator import thrust_columns_f32, wrap32, wrapped_from_the_box

pytestmark = pytest.mark.gpu
RECORD = os.environ.get('QP_EDGES_RECORD', '')
F32, F64 = np.float32, np.float64
_FLOWN = {}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _dev(a):
    return H.to_dev(np.ascontiguousarray(a))


def _scalar(regime, K):
    """(state_out [N, 5], act [N, 7], cost [N]) of one scalar launch on the regime's inputs."""
    from ml4ca_amd.policy import thrust_alloc_qp
    S, tau = QE.inputs(regime)
    act, So, J = thrust_alloc_qp(_dev(tau.T), _dev(S.T), QE.params(regime, K), QE.DT, cost=True)
    return _np(So).T.copy(), _np(act), _np(J)


def _table():
    """[32, 17 N] float32: regime r on lanes N r .. N r + N - 1."""
    from ml4ca_amd.deploy import QP_SLOTS, qp_allocator_table
    R = QE.regimes()
    per = {}
    for name, (_, width) in QP_SLOTS.items():
        v = np.array([np.asarray(R[r][name], F64).reshape(width) for r in R for _ in range(QE.N)])
        per[name] = v[:, 0] if width == 1 else v
    return qp_allocator_table(QE.N * len(R), **per)


def flown(K):
    """regime -> dict(scalar=(state_out, act, cost), table=(...)) at K iterations, flown once for the module."""
    if K not in _FLOWN:
        import torch
        from ml4ca_amd.policy import thrust_alloc_qp
        names = QE.names()
        rec = {r: dict(scalar=_scalar(r, K)) for r in names}
        S = np.concatenate([QE.inputs(r)[0] for r in names])
        tau = np.concatenate([QE.inputs(r)[1] for r in names])
        refused = torch.full((len(S),), 9, dtype=torch.uint8, device='cuda:0')
        act, So, J = thrust_alloc_qp(_dev(tau.T), _dev(S.T), table=_dev(_table()), iterations=K, dt=QE.DT, cost=True, refused=refused)
        assert not bool(refused.any())                            # every regime is one the library accepts
        So, act, J = _np(So).T, _np(act), _np(J)
        for k, r in enumerate(names):
            sl = slice(QE.N * k, QE.N * (k + 1))
            rec[r]['table'] = (So[sl].copy(), act[sl].copy(), J[sl].copy())
        _FLOWN[K] = rec
    return _FLOWN[K]


def unwrapped(regime, K, state_out, cost=None):
    """D [N, 5] float32: the device's solution, its azimuths un-wrapped into the box.  Only in rates_open does more than one turn fit:
    there the turn is the one cost_out names (qp_edges.unwrap_by_cost) or, for the one-iteration comparison, the one nearest the float64
    host iterate."""
    if cost is not None and QE.turns_of(regime) > 2:
        return QE.unwrap_by_cost(regime, state_out, cost)
    near = QE.solve(regime, K, F64)['x'][:, 3:5]
    return np.concatenate([state_out[:, 0:3], QE.unwrap(regime, state_out[:, 3:5], near)], 1)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def check_exact(regime, K, state, act, cost):
    S, tau = QE.inputs(regime)
    p = QE.params(regime, K)
    lo, hi = QE.box(regime)
    over = QE.overflow_lanes(regime)
    assert state.dtype == F32 and np.isfinite(state).all() and np.isfinite(act).all()
    # inside the box of the device's own input, no tolerance: forces everywhere, azimuths where the wrap is the identity ...
    assert (lo[:, :3] <= state[:, :3]).all() and (state[:, :3] <= hi[:, :3]).all()
    assert (state[:, 3:5] >= -QE.PI32).all() and (state[:, 3:5] < QE.PI32).all()
    plain = (lo[:, 3:5] > -QE.PI32) & (hi[:, 3:5] < QE.PI32)
    assert (lo[:, 3:5][plain] <= state[:, 3:5][plain]).all() and (state[:, 3:5][plain] <= hi[:, 3:5][plain]).all()
    # ... elsewhere some float32 x inside [lo, hi] wraps to state_out bit for bit
    k0 = np.floor((S[:, 3:5].astype(F64) + np.pi) / (2 * np.pi))
    turns = QE.turns_of(regime)
    found = wrapped_from_the_box(state[:, 3:5], lo[:, 3:5], hi[:, 3:5], turns=turns, k0=k0)
    assert found.all(), np.nonzero(~found.all(1))[0]
    # the thrust columns are the stated map of state_out with the regime's own kf and kr, bit for bit; a -0.0 that stays commands -0.0
    assert np.array_equal(_bits(act[:, :3]), _bits(thrust_columns_f32(state[:, :3], p)))
    if QE.keeps_signed_zeros(regime):
        assert np.array_equal(_bits(state[QE.AT_REST, :3]), _bits(S[QE.AT_REST, :3]))
        assert np.array_equal(_bits(act[QE.AT_REST, :3]), _bits(S[QE.AT_REST, :3])) and np.signbit(act[QE.AT_REST, 0])
    # the heads: within 2e-7 of float64 sin / cos of the final angle wherever |angle| <= 3e4 - the un-wrapped angle, which is some turn
    # of state_out inside the box
    best = np.full((QE.N, 2), np.inf)
    two_pi = F64(F32(2.0) * QE.PI32)
    for dk in range(-turns, turns + 1):
        c = (state[:, 3:5].astype(F64) + (k0 + dk) * two_pi).astype(F32)
        ok = (lo[:, 3:5] <= c) & (c <= hi[:, 3:5])
        c64 = c.astype(F64)
        e = np.maximum(np.abs(act[:, 3:7:2] - np.sin(c64)), np.abs(act[:, 4:7:2] - np.cos(c64)))
        e = np.where(np.abs(c64) <= QE.AZ_LIMIT, e, 0.0)          # past 3e4 sincos_lean promises a rotation, not this accuracy
        best = np.where(ok, np.minimum(best, e), best)
    heads = float(best.max())
    assert np.abs(act[:, 3:7]).max() <= 1.0 + 2e-7
    # overflow lanes hold the (wrapped) start bit for bit, command a finite action and report a J that is not finite
    held = np.concatenate([S[:, :3], wrap32(S[:, 3:5])], 1)
    assert over.sum() >= 2
    assert np.array_equal(_bits(QE.canon(regime, state[over])), _bits(QE.canon(regime, held[over])))
    assert not np.isfinite(cost[over]).any() and np.isfinite(cost[~over]).all()
    if regime == 'all_dead':
        assert (state[:, :3] == 0).all() and (act[:, :3] == 0).all()
    if regime == 'all_frozen':
        assert np.array_equal(_bits(QE.canon(regime, state)), _bits(QE.canon(regime, held)))
    return heads, int(np.argmax(best.max(1)))


@pytest.mark.parametrize('K', QE.GPU_ITERATIONS)
@pytest.mark.parametrize('regime', QE.names())
def test_exact_properties(regime, K):
    rec = flown(K)[regime]
    for a, b in zip(rec['scalar'], rec['table']):                 # the table launch is the scalar launch of each regime, bit for bit
        assert np.array_equal(_bits(a), _bits(b))
    heads, lane = check_exact(regime, K, *rec['scalar'])
    check_exact(regime, K, *rec['table'])
    QE.record(RECORD, 'exact  %-12s K %2d  heads max abs err %.3g (lane %d)' % (regime, K, heads, lane))
    assert heads <= 2e-7


def test_the_regimes_fly_apart():
    """The 17 blocks of the table launch are not each other's: every regime but the defaults differs from `default` on some lane."""
    rec = flown(16)
    for r in QE.names():
        if r != 'default':
            assert not np.array_equal(_bits(rec[r]['table'][1]), _bits(rec['default']['table'][1])), r


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', QE.PREFIX_REGIMES)
def test_the_loops_prefix_property(regime):
    """K = 1 .. 32 from the same inputs: cost_out(K) <= cost_out(K - 1) as float32 numbers on every finite lane; where the two are equal
    state_out and the action are equal bit for bit; where they differ the state differs."""
    runs = [_scalar(regime, K) for K in range(1, 33)]
    fin = np.isfinite(runs[0][2])
    assert np.array_equal(fin, ~QE.overflow_lanes(regime))
    moved = np.zeros(32, int)
    for K in range(1, 32):
        (s0, a0, c0), (s1, a1, c1) = runs[K - 1], runs[K]
        assert np.isfinite(c1[fin]).all() and (c1[fin] <= c0[fin]).all(), K + 1
        eq = (c1 == c0) & fin
        same_state, same_act = (_bits(s0) == _bits(s1)).all(1), (_bits(a0) == _bits(a1)).all(1)
        assert same_state[eq].all() and same_act[eq].all(), K + 1
        assert not same_state[fin & ~eq].any(), K + 1
        assert same_state[~fin].all() and same_act[~fin].all()
        moved[K] = int((fin & ~eq).sum())
    QE.record(RECORD, 'prefix %-12s lanes that moved at iteration 2 .. 32: %s' % (regime, moved[1:].tolist()))
    assert (moved[1:] > 0).sum() >= 4                             # the later iterations did something


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', QE.GPU_ITERATIONS)
@pytest.mark.parametrize('regime', QE.names())
def test_never_worse_than_holding(regime, K):
    state, act, cost = flown(K)[regime]['scalar']
    m = QE.lane_domain(regime)
    D = unwrapped(regime, K, state, cost)
    assert np.isfinite(D[m]).all()
    jD, j0 = QE.J64(regime, D), QE.J64(regime, QE.start(regime))
    slack = QE.hold_slack(regime, D)
    excess = (jD - j0)[m]
    cerr = (np.abs(cost.astype(F64) - jD) / (1.0 + np.abs(jD)))[m]
    QE.record(RECORD, 'hold   %-12s K %2d  J64(D) - J64(x0): largest %.3g, largest / slack %.3g;  |cost_out - J64(D)| / (1 + J) %.3g' % (
        regime, K, excess.max(), (excess / slack[m]).max(), cerr.max()))
    assert (excess <= slack[m]).all()
    assert np.allclose(cost[m], jD[m], rtol=1e-5, atol=1e-5)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', QE.well_conditioned())
def test_one_iteration_parity(regime):
    state, act, cost = flown(1)[regime]['scalar']
    m = QE.kept(regime)
    assert (QE.left_out(regime).sum() <= QE.CAP * QE.N) and m.sum() >= QE.N - 12
    x64 = QE.solve(regime, 1, F64)['x']
    D = unwrapped(regime, 1, state)
    assert np.isfinite(D[m]).all()
    err = QE.parity_err(D, x64)
    yard, bound = QE.parity_yardstick(regime), QE.parity_bound(regime)
    worst = int(np.argmax(np.where(m, err, 0)))
    QE.record(RECORD, 'parity %-12s device %.3g (lane %d)  float32 host law %.3g  bound %.3g  device / bound %.3g  lanes %d' % (
        regime, err[m].max(), worst, yard, bound, err[m].max() / bound, m.sum()))
    assert (err[m] <= bound).all(), (regime, worst, float(err[worst]), bound)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', (16, 32))
@pytest.mark.parametrize('regime', QE.well_conditioned())
def test_objective_by_the_float32_yardstick(regime, K):
    state, act, cost = flown(K)[regime]['scalar']
    m = QE.lane_domain(regime)
    yard, j64 = QE.objective_yardstick(regime, K)
    gap = np.abs(QE.J64(regime, unwrapped(regime, K, state, cost)) - j64)
    allow = 4.0 * yard + 1e-6 * (1.0 + j64)
    cls = QE.wrench_class(regime)
    for c, what in ((0, 'nominal'), (1, 'huge')):
        sel = m & (cls == c)
        QE.record(RECORD, 'object %-12s K %2d  %-7s max |J64(D) - J64(H64)| %.3g  yardstick %.3g  worst gap / allowed %.3g  largest J %.4g' % (
            regime, K, what, gap[sel].max(), yard[sel].max(), (gap / allow)[sel].max(), j64[sel].max()))
    assert (gap[m] <= allow[m]).all(), (regime, K, np.nonzero(m & ~(gap <= allow))[0])


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_state_from_action_on_asym():
    """One labelling call per row with flown= and params = asym: forces in bits against deploy.qp_state_from_action with kf != kr on every
    thruster (the rows saturate thrust both ways), azimuths by the bound of the test this is shared with."""
    from tests.test_gpu_controller_label_qp_flown import state_from_action_against_the_host_statement
    state_from_action_against_the_host_statement(QE.params('asym', 16))
