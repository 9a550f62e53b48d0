"""Edge cases of the rate-limited QP thrust allocation (plain NumPy, no GPU, never calls the library's kernels): the regimes, the lanes,
the references and the bounds shared by tests/test_qp_edges_cpu.py (are the cases fair - does the host law by itself keep what the GPU
module relies on?) and tests/test_gpu_qp_edges.py (dpenv_thrust_alloc_qp against the float64 host law).

Every reference is deploy.BatchedQPAllocator, the host statement of include/dpenv.h, in float32 and in float64, solved from the same float32
state and wrench; `trace=` of its solve() gives the trial J, the accept flag, the frozen set and the gradient of every iteration.

REGIMES: name -> parameter dict.  `default` is qp_allocator_defaults(); `asym` makes every field asymmetric at once (ahead / astern, port /
starboard, the three wrench axes), so that any swap of two components changes the answer (the CPU module counts the lanes on which it
does); the others change one thing and reach the ends of what include/dpenv.h accepts: a dead thruster, a frozen azimuth or force, a
weight of zero, weights across ten decades, arms of zero.

LANES: N = 130 (two waves plus two) of (state [5], tau [3]) per regime, fixed seed: forces uniform in +-f_max of the regime, azimuths in
[-pi, pi), wrenches in +-TAU_MAX; PINNED lanes at the first and last lane of each wave and the tail carry the edges (forces on their
bounds, signed zeros, 1e-30; azimuths at +-pi, many turns out, at and past sincos_lean's range; wrenches of 0, denormal, 10 x TAU_MAX, 1e6,
and 1e19 / 3e19 at which the float32 J of the start overflows while tau is finite).

DOMAIN: domain(regime) names the checks a regime takes.  Every regime takes 'exact' (the properties with no tolerance) and 'hold' (never
worse than holding, which the host law meets with slack 0).  'parity' and 'objective' are for the well-conditioned regimes.  Outside:
  track_heavy, arms_long   the LDL' without pivoting amplifies float32 rounding: the host law's own float32 and float64 one-step iterates
                           differ by up to 0.3 relative there;
  all_dead, all_frozen     no step moves J (no force can change / nothing can move), so every accept margin is 0 and the one-iteration
                           comparison has no lane left to stand on.  What they promise is exact: forces 0, nothing moves.
lane_domain(regime) is the lanes the accuracy checks take: every azimuth the box allows within 3e4 (beyond it sincos_lean folds in float32 and
promises a valid rotation only - in rates_open the box is 200 rad either side, so the lanes at 29999 leave too) and a finite float32 J of
the start.

THE SLACK of 'hold'.  With D the device's result and x0 the clipped start, J64 the float64 host objective: J64(D) <= J64(x0) + slack.  The
device accepts a step when ITS float32 J went down, so it can be wrong about J64 by the float32 evaluation error of J at the two points
compared, and by nothing else.  That error is measured on the host, never on the device:
    slack = 4 (|J_h32(D) - J_h64(D)| + |J_h32(x0) - J_h64(x0)|) + 1e-6 (1 + J64(x0))
4 and the relative floor are those of tests/test_gpu_qp_allocator.py::test_objective_by_the_float32_yardstick.

THE BOUND of 'parity' (K = 1).  err(x) = max_k |x_k - x64_k| / max(|x64_k|, 1) against the float64 host iterate.  yardstick = the regime's
maximum of err(x32) of the float32 host law over the lanes kept; bound = max(4 yardstick, KC 2^-24): the device differs from the float32
host law in its sin / cos polynomial only.  KC counts the roundings along the longest dependent chain of one iteration, as
tests/test_gpu_ppo_update.py counts chain_K - one per operation of include/dpenv.h's text:
    evaluate   sincos 12 (reduction and the degree-7 kernel), b3 2, r_2 4                                               18
    g          wr 1, the three-term sum 3, + the power / change terms 1  (H is the shorter arm: sincos 12, d3 2, F d3 1, WJ 1,
               the sum 3, the diagonal 1, lambda 2 = 22 against g's 23; the factorisation it feeds is counted in full below)  5
    LDL'       column j: v 1, D_j 2 j, iD_j 1, L[i][j] 2 j + 1, the columns one after the other: sum_j (3 + 4 j), j = 0..4  55
    solve      y_4 after y_3: 8;  d_0 after d_1: 1 + 2 x 4 = 9                                                          17
    x + d                                                                                                                1
KC = 96, a floor of 5.7e-6.
Lanes are left out of 'parity' by the HOST's evidence only (left_out): the float32 and float64 host laws disagree on accept or on the
frozen set; the float64 accept margin |J_trial - J| / (1 + J) is below 1e-5; a coordinate sits on its bound with |g| within 1e-5 of zero
relative to the lane's largest |g| (the frozen test is then decided by rounding).  At most 5 % of a regime's lanes: CAP, a condition the
CPU module asserts of the host law."""
import numpy as np

from tests.test_qp_allocator_cpu import TAU_MAX, box_of

F32, F64 = np.float32, np.float64
N = 130
DT = 0.2
SEED = 17
GPU_ITERATIONS = (1, 16, 32)
CPU_ITERATIONS = (1, 2, 16, 32)
AZ_LIMIT = 3e4
KC = 18 + 5 + 55 + 17 + 1
MARGIN = 1e-5
CAP = 0.05
PI32 = F32(np.pi)
EXACT_ONLY = ('track_heavy', 'arms_long', 'all_dead', 'all_frozen')
PREFIX_REGIMES = ('default', 'asym', 'port_dead', 'smooth_tiny', 'rates_open')
# (the names apart from the numbers: a test module lists its cases when it is collected, and nothing loads the library then)
NAMES = ('default', 'asym', 'track_heavy', 'track_off', 'power_off', 'power_heavy', 'smooth_tiny', 'smooth_heavy', 'bow_dead', 'port_dead',
         'all_dead', 'az_frozen', 'force_frozen', 'all_frozen', 'rates_open', 'arms_zero', 'arms_long')
_cache = {}


# ---------------------------------------------------------------- regimes
def regimes():
    """name -> parameter dict (iterations left at the default; the callers set K)."""
    if 'regimes' in _cache:
        return _cache['regimes']
    from ml4ca_amd.deploy import qp_allocator_defaults
    d = qp_allocator_defaults()

    def mk(**kw):
        p = qp_allocator_defaults()
        p.update(kw)
        return p

    A = lambda *v: np.array(v, F64)
    R = dict(default=mk())
    R['asym'] = mk(w_slack=A(2.0, 1.0, 0.5), f_max=A(7.0, 20.5, 12.0), force_rate=A(10.0, 25.0, 15.0),
                   azimuth_rate=d['azimuth_rate'] * A(1.7, 0.6), lx=d['lx'] * A(1.0, 1.05, 0.9), ly=A(0.02, -0.15, 0.11),
                   kf=d['kf'] * A(1.3, 4.0, 2.0), kr=d['kr'] * A(0.7, 0.25, 0.5))
    R['track_heavy'] = mk(w_slack=np.full(3, 1e4))
    R['track_off'] = mk(w_slack=np.zeros(3))
    R['power_off'] = mk(w_power=0.0)
    R['power_heavy'] = mk(w_power=1e3)
    R['smooth_tiny'] = mk(w_dalpha=1e-6, w_dforce=1e-6)
    R['smooth_heavy'] = mk(w_dalpha=1e4, w_dforce=1e4)
    R['bow_dead'] = mk(f_max=d['f_max'] * A(0.0, 1.0, 1.0))
    R['port_dead'] = mk(f_max=d['f_max'] * A(1.0, 0.0, 1.0))
    R['all_dead'] = mk(f_max=np.zeros(3))
    R['az_frozen'] = mk(azimuth_rate=np.zeros(2))
    R['force_frozen'] = mk(force_rate=np.zeros(3))
    R['all_frozen'] = mk(azimuth_rate=np.zeros(2), force_rate=np.zeros(3))
    R['rates_open'] = mk(force_rate=np.full(3, 1e4), azimuth_rate=np.full(2, 1e3))
    R['arms_zero'] = mk(lx=np.zeros(3), ly=np.zeros(3))
    R['arms_long'] = mk(lx=d['lx'] * 100.0, ly=d['ly'] * 100.0)
    assert tuple(R) == NAMES
    _cache['regimes'] = R
    return R


def names():
    return NAMES


def params(regime, K=16):
    return dict(regimes()[regime], iterations=int(K))


def domain(regime):
    """The checks a regime takes: 'exact' and 'hold' always, 'parity' and 'objective' where the law is well conditioned."""
    return ('exact', 'hold') if regime in EXACT_ONLY else ('exact', 'hold', 'parity', 'objective')


def well_conditioned():
    return tuple(r for r in names() if 'parity' in domain(r))


# ---------------------------------------------------------------- lanes
# forces (a factor of f_max per thruster, or None = the random bulk), azimuths, wrench
FORCES = dict(top=(1.0, 1.0, 1.0), bottom=(-1.0, -1.0, -1.0), mixed=(1.0, -1.0, 1.0), zeros=(-0.0, 0.0, -0.0), tiny=(1e-30, 1e-30, 1e-30))
AZIMUTHS = dict(ends=(-PI32, np.nextafter(PI32, F32(0.0))), turns=(100.0, -2999.0), range_edge=(29999.0, -31000.0), far=(29999.0, -2999.0))
WRENCHES = dict(zero=(0.0, 0.0, 0.0), denormal=(-0.0, 0.0, 1e-42), tiny=(1e-30, 1e-30, 1e-30), jump=tuple(10.0 * TAU_MAX),
                jump_back=tuple(-10.0 * TAU_MAX), huge=(1e6, -1e6, 1e6), overflow_x=(1e19, 0.0, 0.0), overflow=(3e19, 3e19, 3e19))
# lane -> (forces, azimuths, wrench); the first and last lanes of the two waves, the tail, and their neighbours
PINNED = {0: ('top', None, None), 1: ('bottom', None, None), 2: ('zeros', None, 'zero'), 3: (None, None, 'jump'), 4: ('tiny', None, None),
          60: (None, 'range_edge', 'overflow_x'), 61: ('top', None, 'jump'), 62: (None, None, 'huge'), 63: ('tiny', 'ends', 'denormal'),
          64: (None, 'turns', 'tiny'), 65: (None, None, 'overflow_x'), 66: (None, None, 'overflow'), 67: (None, None, 'zero'),
          124: (None, None, 'jump_back'), 125: ('bottom', 'range_edge', None), 126: (None, 'far', None), 127: ('zeros', 'turns', None),
          128: (None, 'ends', 'zero'), 129: ('mixed', None, 'overflow')}
AT_REST = 2                                   # signed-zero forces, no wrench: nothing moves, and -0.0 stays -0.0


def lanes_with(kind, name):
    """The pinned lanes that carry pattern `name` of kind 0 (forces), 1 (azimuths) or 2 (wrench)."""
    return [i for i, spec in PINNED.items() if spec[kind] == name]


def inputs(regime):
    """(state [N, 5], tau [N, 3]) float32 of a regime: the same draws for every regime, the forces scaled by its f_max."""
    key = ('inputs', regime)
    if key not in _cache:
        rng = np.random.default_rng(SEED)
        uF, az, ut = rng.uniform(-1, 1, (N, 3)), rng.uniform(-np.pi, np.pi, (N, 2)), rng.uniform(-1, 1, (N, 3))
        fmax = np.asarray(regimes()[regime]['f_max'], F64).astype(F32)
        F = np.clip((uF * fmax).astype(F32), -fmax, fmax)
        S = np.concatenate([F, np.clip(az.astype(F32), -PI32, np.nextafter(PI32, F32(0.0)))], 1).astype(F32)
        tau = (ut * TAU_MAX).astype(F32)
        for i, (f, a, w) in PINNED.items():
            if f is not None:
                S[i, 0:3] = F32(FORCES[f]) * fmax
            if a is not None:
                S[i, 3:5] = F32(AZIMUTHS[a])
            if w is not None:
                tau[i] = F32(WRENCHES[w])
        assert S.dtype == F32 and tau.dtype == F32 and np.isfinite(S).all() and np.isfinite(tau).all()
        assert (np.abs(S[:, 0:3]) <= fmax).all()                                  # the header's precondition
        S.setflags(write=False)
        tau.setflags(write=False)
        _cache[key] = (S, tau)
    return _cache[key]


# ---------------------------------------------------------------- references
def host(regime, dtype, K=1, p=None):
    from ml4ca_amd.deploy import BatchedQPAllocator
    return BatchedQPAllocator(N, params(regime, K) if p is None else dict(p, iterations=int(K)), DT, dtype)


def solve(regime, K, dtype, p=None):
    """dict(x [N, 5] un-wrapped, J [K + 1, N], trial_J, accept, frozen, g) of the host law in dtype from the regime's float32 inputs; p
    replaces the regime's parameters (the swaps of the CPU module)."""
    key = ('solve', regime, int(K), np.dtype(dtype).name)
    if p is None and key in _cache:
        return _cache[key]
    S, tau = inputs(regime)
    tr = {}
    with np.errstate(all='ignore'):
        x, J = host(regime, dtype, K, p).solve(tau.astype(dtype), S.astype(dtype), trace=tr)
    out = dict(tr, x=x, J=J)
    if p is None:
        _cache[key] = out
    return out


def J64(regime, x):
    """The float64 host objective of x [N, 5] (any dtype) at the regime's inputs."""
    S, tau = inputs(regime)
    with np.errstate(all='ignore'):
        return host(regime, F64).objective(np.asarray(x, F64), tau.astype(F64), S.astype(F64))


def J32(regime, x):
    """The float32 host objective of x [N, 5] float32, as float64 numbers."""
    S, tau = inputs(regime)
    with np.errstate(all='ignore'):
        return host(regime, F32).objective(np.asarray(x, F32), tau, S).astype(F64)


def box(regime):
    """(lo, hi) [N, 5] float32 by the header's single operations, from the regime's input state."""
    return box_of(host(regime, F32), inputs(regime)[0])


def start(regime):
    """x0 [N, 5] float32: clip(state, lo, hi) - the state itself under the precondition."""
    lo, hi = box(regime)
    return np.fmin(np.fmax(inputs(regime)[0], lo), hi)


def canon(regime, x):
    """x with the sign of zero dropped on the forces of thrusters that are dead (f_max = 0) or frozen (force_rate = 0): there lo = -0.0 and
    hi = +0.0 around a force of -0.0, clip(-0.0, -0.0, +0.0) may return either zero (fminf and np.fmin are free to differ on it), and the
    header does not say which.  Everything else is compared in bits."""
    x = np.array(x)
    p = regimes()[regime]
    loose = (np.asarray(p['f_max'], F64) == 0) | (np.asarray(p['force_rate'], F64) == 0)
    x[:, :3][:, loose] = x[:, :3][:, loose] + x.dtype.type(0.0)
    return x


def keeps_signed_zeros(regime):
    """True where no thruster is dead or frozen: a force of -0.0 at rest then stays -0.0 in bits."""
    p = regimes()[regime]
    return bool((np.asarray(p['f_max'], F64) > 0).all() and (np.asarray(p['force_rate'], F64) > 0).all())


def overflow_lanes(regime):
    """[N] bool: the float32 J of the start is not finite (tau is)."""
    return ~np.isfinite(solve(regime, 1, F32)['J'][0])


def lane_domain(regime):
    """[N] bool: the lanes the accuracy checks take."""
    lo, hi = box(regime)
    return (np.maximum(np.abs(lo[:, 3:5]), np.abs(hi[:, 3:5])) <= AZ_LIMIT).all(1) & ~overflow_lanes(regime)


def wrench_class(regime):
    """[N] int: 0 for wrenches up to 10 x TAU_MAX, 1 for the huge ones - the objective's yardstick is taken per class, so that a lane
    whose J is 1e12 does not set the allowance of a lane whose J is 10."""
    _, tau = inputs(regime)
    return (np.abs(tau) > 10.0 * TAU_MAX * (1 + 1e-6)).any(1).astype(int)


def left_out(regime):
    """[N] bool, the in-domain lanes the one-iteration comparison leaves out - by the host's evidence at K = 1 alone."""
    a, b = solve(regime, 1, F32), solve(regime, 1, F64)
    disagree = (a['accept'][0] != b['accept'][0]) | (a['frozen'][0] != b['frozen'][0]).any(1)
    J0 = b['J'][0]
    with np.errstate(all='ignore'):
        margin = np.abs(b['trial_J'][0] - J0) / (1.0 + J0)
        S, _ = inputs(regime)
        h = host(regime, F64)
        lo, hi = h.box(S.astype(F64))
        x0 = np.fmin(np.fmax(S.astype(F64), lo), hi)
        g = np.abs(b['g'][0])
        tie = (((x0 <= lo) | (x0 >= hi)) & (g <= MARGIN * g.max(1, keepdims=True))).any(1)
    return lane_domain(regime) & (disagree | ~(margin >= MARGIN) | tie)


def kept(regime):
    return lane_domain(regime) & ~left_out(regime)


def parity_err(x, x64):
    """[N]: max_k |x_k - x64_k| / max(|x64_k|, 1)"""
    x, x64 = np.asarray(x, F64), np.asarray(x64, F64)
    return (np.abs(x - x64) / np.maximum(np.abs(x64), 1.0)).max(1)


def parity_yardstick(regime):
    """The float32 host law's own one-iteration error against the float64 host law, the maximum over the lanes kept."""
    m = kept(regime)
    return float(parity_err(solve(regime, 1, F32)['x'], solve(regime, 1, F64)['x'])[m].max())


def parity_bound(regime):
    return max(4.0 * parity_yardstick(regime), KC * 2.0 ** -24)


def hold_slack(regime, D):
    """[N]: the slack of `never worse than holding` for a result D [N, 5] float32 (module docstring)."""
    x0 = start(regime)
    j0 = J64(regime, x0)
    return 4.0 * (np.abs(J32(regime, D) - J64(regime, D)) + np.abs(J32(regime, x0) - j0)) + 1e-6 * (1.0 + j0)


def objective_yardstick(regime, K):
    """[N]: per lane the yardstick of its wrench class, max |J64(H32) - J64(H64)| over the class's in-domain lanes, and J64(H64) [N]."""
    j32, j64 = J64(regime, solve(regime, K, F32)['x']), J64(regime, solve(regime, K, F64)['x'])
    m, cls = lane_domain(regime), wrench_class(regime)
    yard = np.zeros(N)
    for c in (0, 1):
        sel = m & (cls == c)
        if sel.any():
            yard[cls == c] = np.abs(j32 - j64)[sel].max()
    return yard, j64


# ---------------------------------------------------------------- the wrapped state
def wrap32(v):
    from tests.test_gpu_qp_allocator import wrap32 as w
    return w(np.asarray(v, F32))


def turns_of(regime):
    """How many turns either side of the box's middle an un-wrapped azimuth can lie: 1 where the box is narrower than a turn."""
    da = float(np.max(host(regime, F32).da))
    return 1 + int(np.ceil(da / np.pi))


def unwrap(regime, az, near):
    """The un-wrapped azimuths [N, 2] float32 of wrapped ones: a + 2 pi k rounded to float32, of the k for which that lies inside the
    regime's box the one nearest `near` [N, 2] (the box is narrower than a turn in every regime but rates_open, so the k is unique
    there).  The wrap is one fused step and the un-wrapped number is the coarser of the two, so rounding gives it back exactly.  Lanes with
    no such k get NaN."""
    lo, hi = box(regime)
    lo, hi = lo[:, 3:5], hi[:, 3:5]
    two_pi = F64(F32(2.0) * PI32)
    k0 = np.floor((inputs(regime)[0][:, 3:5].astype(F64) + np.pi) / (2 * np.pi))
    best = np.full(az.shape, np.nan, F32)
    dist = np.full(az.shape, np.inf)
    for dk in range(-turns_of(regime), turns_of(regime) + 1):
        c = (az.astype(F64) + (k0 + dk) * two_pi).astype(F32)
        ok = (lo <= c) & (c <= hi)
        d = np.abs(c.astype(F64) - near)
        take = ok & (d < dist)
        best, dist = np.where(take, c, best), np.where(take, d, dist)
    return best


def unwrap_by_cost(regime, state_out, cost):
    """D [N, 5] float32 where the box is wider than a turn (rates_open) and the wrapped state alone does not say which turn the solution
    is on: the device's other output does.  J depends on the turn through 1/2 w_dalpha (e_3^2 + e_4^2) alone, so of the turns (k_p, k_s)
    that lie in the box the pair is taken whose e_3^2 + e_4^2 is nearest 2 (cost_out - J64 without that term) / w_dalpha.  A lane whose
    J is too large for cost_out to resolve a turn gets one of them, and no check on J can tell them apart either."""
    S, _ = inputs(regime)
    lo, hi = box(regime)
    T = turns_of(regime)
    ks = np.arange(-T, T + 1, dtype=F64)
    k0 = np.floor((S[:, 3:5].astype(F64) + np.pi) / (2 * np.pi))
    cand = (state_out[:, 3:5, None].astype(F64) + (k0[:, :, None] + ks) * F64(F32(2.0) * PI32)).astype(F32)          # [N, 2, M]
    ok = (lo[:, 3:5, None] <= cand) & (cand <= hi[:, 3:5, None])
    e2 = np.where(ok, (cand.astype(F64) - S[:, 3:5, None].astype(F64)) ** 2, np.inf)
    first = np.argmin(e2, 2)                                                                     # the turn nearest the state in force
    pick = lambda idx: np.take_along_axis(cand, idx[:, :, None], 2)[:, :, 0]
    wda = float(regimes()[regime]['w_dalpha'])
    base = np.concatenate([state_out[:, 0:3], pick(first)], 1)
    rest = J64(regime, base) - 0.5 * wda * np.take_along_axis(e2, first[:, :, None], 2)[:, :, 0].sum(1)
    with np.errstate(all='ignore'):
        target = 2.0 * (np.asarray(cost, F64) - rest) / wda
        miss = np.abs(e2[:, 0, :, None] + e2[:, 1, None, :] - target[:, None, None])            # [N, M, M]
        miss = np.where(np.isfinite(miss), miss, np.inf).reshape(N, -1)
    best = np.argmin(miss, 1)
    idx = np.stack([best // len(ks), best % len(ks)], 1)
    idx = np.where(np.isfinite(miss.min(1))[:, None], idx, first)
    return np.concatenate([state_out[:, 0:3], pick(idx)], 1)


def record(path, line):
    print(line)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')
