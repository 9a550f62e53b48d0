"""Deployment-side adapters of the RL allocator: what the thesis' ROS node wraps around the trained actor
(src/rl/ROS/rl_allocator/src/rl_allocator.py, utils.py:88-115, errorFrame.py), without ROS.

Host logic (NumPy, float64), not on the accelerated path: SURVEY section 8(f) rank 4.  It exists so that a policy
trained on the batched env can be driven exactly the way the vessel's node drives it - state assembly with the radian
wrap the node uses (unlike the training env, quirk Q1), network order -> ROS thruster order, default commands for the
thrusters a variant does not control, the optional body-frame integral action, and the message fields published.
BatchedBodyFrameIntegrator is the torch form of that integral action for a batch of envs (the law the closed-loop
kernels apply while it is on, include/dpenv.h); BatchedReferenceFilter is the same for the setpoint reference filter
the node took its reference from.

  network order  [n_bow, n_port, n_star, (a_bow,) a_port, a_star]       (customEnv.py:47-61)
  ROS order      [n_port, n_star, n_bow, a_port, a_star, a_bow]         (rl_allocator.py:92-106)
"""
import numpy as np

from ._num import _fma32

ROS_ORDER = ('n_port', 'n_star', 'n_bow', 'a_port', 'a_star', 'a_bow')

# rl_allocator.py:92-106
ACT_BND = {'simple': [100.0] * 3, 'limited': [100.0] * 3 + [np.pi / 2] * 2, 'final': [100.0] * 3 + [np.pi] * 2,
           'full': [100.0] * 3 + [np.pi] * 3}
ACT_MAP = {'simple': {0: 2, 1: 0, 2: 1}, 'limited': {0: 2, 1: 0, 2: 1, 3: 3, 4: 4}, 'final': {0: 2, 1: 0, 2: 1, 3: 3, 4: 4},
           'full': {0: 2, 1: 0, 2: 1, 3: 5, 4: 3, 5: 4}}
ACT_DEF = {'simple': [0, 0, 0, np.pi / 2, -3 * np.pi / 4, 3 * np.pi / 4], 'limited': [0, 0, 0, np.pi / 2, 0, 0],
           'final': [0, 0, 0, np.pi / 2, 0, 0], 'full': [0] * 6}


def wrap_angle(angle, deg=False):
    """errorFrame.py:14-25 of the ROS package: the node's wrap defaults to RADIANS (the training env's to degrees)."""
    ref = 180.0 if deg else np.pi
    return np.mod(np.asarray(angle, np.float64) + ref, 2 * ref) - ref


def shortest_path(a_prev, a, deg=False):
    """rl_allocator.py:284-299: signed shortest angular distance from a_prev to a."""
    ref = 180.0 if deg else np.pi
    shortest = np.mod(np.mod(a - a_prev, 2 * ref) + 2 * ref, 2 * ref)
    return shortest - 2 * ref if shortest > ref else shortest


def to_ros_order(action, variant='final', cont_ang=True):
    """Raw network output(s) [..., act_dim] -> thruster commands in the ROS order [..., 6] (percent, radians):
    handle_continuous_angles (rl_allocator.py:275-283), scale_and_clip (:222-226), defaults and maps (:228-250)."""
    a = np.asarray(action, np.float64)
    lead = a.shape[:-1]
    a = a.reshape(-1, a.shape[-1])
    bnd = np.asarray(ACT_BND[variant], np.float64)
    if variant == 'final' and cont_ang:
        a = np.concatenate([a[:, 0:3], np.arctan2(a[:, 3:4], a[:, 4:5]) / bnd[-1], np.arctan2(a[:, 5:6], a[:, 6:7]) / bnd[-1]], 1)
    a = np.clip(a * bnd, -bnd, bnd)
    out = np.zeros((a.shape[0], 6))
    for i, default in enumerate(ACT_DEF[variant]):          # (1) defaults through the FULL map
        out[:, ACT_MAP['full'][i]] = default
    for i in range(a.shape[1]):                             # (2) the variant's own commands
        out[:, ACT_MAP[variant][i]] = a[:, i]
    return out.reshape(lead + (6,))


def publishable(u, simulation=True):
    """utils.py:88-115: the fields of the three messages the node publishes for one command vector in ROS order."""
    u = np.asarray(u, np.float64)
    msg = {'pod_angle.port': float(np.rad2deg(u[3])), 'pod_angle.star': float(np.rad2deg(u[4])),
           'stern.port_effort': float(u[0]), 'stern.star_effort': float(u[1]), 'bow.lin_act_bow': 2}
    if simulation:
        msg['bow.position_bow'] = int(np.rad2deg(u[5]))
        msg['bow.throttle_bow'] = float(u[2])
    else:
        msg['bow.position_bow'] = 45                                           # utils.py:112
        msg['bow.throttle_bow'] = float(np.clip(float(u[2]) * 2.5, -100.0, 100.0))   # utils.py:113
    return msg


class BodyFrameIntegrator(object):
    """rl_allocator.py:252-273: integral action added to the body-frame error once the vessel has dwelt near the
    setpoint.  Leaving the 5 m / 140 deg box resets it; after 5 s inside, it integrates 0.05 * error * step, clipped to
    [0.5 m, 1 m, pi/32 rad].  `now` replaces the node's wall clock."""
    GAIN = np.array([0.05, 0.05, 0.05])
    BOUND = np.array([0.5, 1.0, np.pi / 32])

    def __init__(self, now=0.0):
        self.value = np.zeros(3)
        self.time_arrival = float(now)

    def update(self, err, step, now):
        err = np.asarray(err, np.float64)
        if abs(err[0]) > 5.0 or abs(err[1]) > 5.0 or abs(err[2]) > np.deg2rad(140):
            self.value = np.zeros(3)
            self.time_arrival = float(now)
        elif (now - self.time_arrival) > 5.0:
            self.value = np.clip(self.value + step * self.GAIN * err, -self.BOUND, self.BOUND)
        return err + self.value


def dwell_steps(dwell_s, dt):
    """D: the smallest integer with D * dt > dwell_s, in float64 - the node's (now - time_arrival) > dwell_s in control steps."""
    D = max(int(np.floor(float(dwell_s) / float(dt))), 0)
    while D > 0 and (D - 1) * float(dt) > float(dwell_s):
        D -= 1
    while not D * float(dt) > float(dwell_s):
        D += 1
    return D


class BatchedBodyFrameIntegrator(object):
    """BodyFrameIntegrator for n envs at once, as torch tensors: the law the closed-loop kernels apply while
    dpenv_set_integral_action is on (include/dpenv.h), in its operation order, so that in float32 it reproduces the
    kernels' policy inputs bit for bit.  The dwell clock is a count of control steps (c, capped at D = dwell_steps):
        outside = any |e_j| > box_j;  outside: I = 0, c = 0;  else c = min(c + 1, D) and, once c >= D,
        I_j = min(max(I_j + step_s * (gain_j * e_j), -bound_j), bound_j)
    update(e) applies it once (one control step) and returns e[:, :3] + I; reset(mask) zeroes I and c (a new episode).
    With env.step / policy_forward it is the eager form of the deployed controller; the fused launch is
    policy.policy_rollout with env.set_integral_action on."""
    GAIN = (0.05, 0.05, 0.05)
    BOUND = (0.5, 1.0, np.pi / 32)
    BOX = (5.0, 5.0, float(np.deg2rad(140.0)))

    def __init__(self, n, gain=GAIN, bound=BOUND, box=BOX, dwell_s=5.0, dt=0.2, step_s=None, dtype=None, device='cpu'):
        import torch
        self.dtype = torch.float32 if dtype is None else dtype
        t = lambda v: torch.as_tensor(np.asarray(v, np.float64), dtype=self.dtype, device=device)
        self.gain, self.bound, self.box = t(gain), t(bound), t(box)
        self.step_s = t(dt if step_s is None else step_s)
        self.dwell = dwell_steps(dwell_s, dt)
        self.I = torch.zeros((n, 3), dtype=self.dtype, device=device)
        self.count = torch.zeros(n, dtype=torch.int32, device=device)

    def update(self, e):
        """e: [n, >=3] (the observation's pose-error columns first).  Returns the policy input's first three columns."""
        import torch
        e = e[:, :3].to(self.dtype)
        outside = (e.abs() > self.box).any(dim=1)
        self.count = torch.where(outside, torch.zeros_like(self.count), torch.clamp(self.count + 1, max=self.dwell))
        grow = (~outside) & (self.count >= self.dwell)
        new = torch.fmin(torch.fmax(self.I + self.step_s * (self.gain * e), -self.bound), self.bound)    # fminf(fmaxf()): a NaN is dropped
        self.I = torch.where(outside[:, None], torch.zeros_like(self.I), torch.where(grow[:, None], new, self.I))
        return e + self.I

    def reset(self, mask=None):
        """Zero I and c of the envs in mask (bool [n]; None = all)."""
        if mask is None:
            self.I.zero_()
            self.count.zero_()
        else:
            self.I[mask] = 0
            self.count[mask] = 0


# the setpoint reference filter's defaults: the least-squares fit to the recorded filter output of the thesis' box, current box and
# large-setpoint runs (tools/gen_golden_reffilter.py prints it; tests/golden/reference_filter.npz keeps it)
REFERENCE_FILTER_OMEGA = (0.619, 0.619, 1.51)
REFERENCE_FILTER_ZETA = (1.0, 1.0, 1.0)


def reference_filter_coeffs_f64(omega, zeta, dt):
    """(phi [3, 3, 3], gam [3, 3]) float64: per axis j the exact zero-order hold of the third-order reference model over dt,
    exp([[A_j, B_j], [0, 0]] dt) by scaling and squaring of its degree-18 Taylor polynomial - the recipe of dpenv.h, which rounds
    the result to f32 (dpenv_reference_filter_coeffs)."""
    phi, gam = np.zeros((3, 3, 3)), np.zeros((3, 3))
    for j in range(3):
        w, c = float(omega[j]), 2.0 * float(zeta[j]) + 1.0
        M = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [-w * w * w, -c * w * w, -c * w, w * w * w], [0.0] * 4]) * float(dt)
        norm, sq = float(np.abs(M).sum(0).max()), 0
        while norm > 0.5 and sq < 200:
            norm *= 0.5
            sq += 1
        M = M * np.ldexp(1.0, -sq)
        E, T = np.eye(4), np.eye(4)
        for k in range(1, 19):
            T = (T @ M) / float(k)
            E = E + T
        for _ in range(sq):
            E = E @ E
        phi[j], gam[j] = E[:3, :3], E[:3, 3]
    return phi, gam


def reference_filter_coeffs(omega=REFERENCE_FILTER_OMEGA, zeta=REFERENCE_FILTER_ZETA, dt=0.2):
    """The library's f32 coefficients (dpenv_reference_filter_coeffs): (phi [3, 3, 3], gam [3, 3]) float32.  A pure host call;
    bad inputs raise DpenvError."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    rf = _lib.ReferenceFilter()
    rf.struct_size = C.sizeof(_lib.ReferenceFilter)
    for j in range(3):
        rf.omega[j], rf.zeta[j] = float(omega[j]), float(zeta[j])
    phi, gam = (C.c_float * 9 * 3)(), (C.c_float * 3 * 3)()
    _lib.check(lib.dpenv_reference_filter_coeffs(C.byref(rf), float(dt), C.byref(phi), C.byref(gam)))
    return np.array(phi, np.float32).reshape(3, 3, 3), np.array(gam, np.float32).reshape(3, 3)


class BatchedReferenceFilter(object):
    """The setpoint reference filter of the deployed controller for n envs, as torch tensors: per axis j in (N, E, psi) the
    third-order reference model x''' + (2 zeta + 1) omega x'' + (2 zeta + 1) omega^2 x' + omega^3 x = omega^3 r, stepped by its
    exact zero-order hold over dt, in the f32 operation order of include/dpenv.h with the library's coefficients - the law the
    closed-loop kernels apply while dpenv_set_reference_filter is on, bit for bit.  dtype=torch.float64 uses the f64 coefficients
    instead (the recorded pin).  State: x [3 (pos, vel, acc), 3 (N, E, psi), n] and the targets r [3, n]; heading in rad, unwrapped.
    Eager use: env.step(a, new_ref=F.advance()), F.switch(target) when the setpoint changes, F.reset(env reference, mask) after an
    auto-reset - the fused launch is policy.policy_rollout with env.set_reference_filter on."""

    def __init__(self, n, omega=REFERENCE_FILTER_OMEGA, zeta=REFERENCE_FILTER_ZETA, dt=0.2, device='cpu', dtype=None):
        import torch
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype == torch.float32:
            phi, gam = reference_filter_coeffs(omega, zeta, dt)
        else:
            phi, gam = reference_filter_coeffs_f64(omega, zeta, dt)
        t = lambda v: torch.as_tensor(v, device=device).to(self.dtype)
        self.phi, self.gam = t(phi), t(gam)                                   # [j][m][k], [j][m]
        if self.dtype == torch.float32:
            self.two_pi, self.inv_two_pi = t(np.float32(2 * np.pi)), t(np.float32(1 / (2 * np.pi)))
        else:
            self.two_pi, self.inv_two_pi = t(2 * np.pi), t(1 / (2 * np.pi))
        self.x = torch.zeros((3, 3, n), dtype=self.dtype, device=device)
        self.r = torch.zeros((3, n), dtype=self.dtype, device=device)

    @property
    def pos(self):
        return self.x[0]

    def advance(self):
        """One control period; returns the position eta_d [3, n] (contiguous): the step's new_ref."""
        import torch
        p, v, a = self.x[0], self.x[1], self.x[2]
        P, G = self.phi, self.gam
        rows = [((P[:, m, 0:1] * p + P[:, m, 1:2] * v) + P[:, m, 2:3] * a) + G[:, m:m + 1] * self.r for m in range(3)]
        self.x = torch.stack(rows)
        return self.x[0].clone().contiguous()

    def switch(self, target, mask=None):
        """New targets [3, n] for the envs in mask (bool [n]; None = all); heading the short way from the present heading."""
        import torch
        target = torch.as_tensor(target, device=self.r.device).to(self.dtype)
        d = target[2] - self.x[0, 2]
        psi = self.x[0, 2] + (d - self.two_pi * torch.round(d * self.inv_two_pi))
        new = torch.stack([target[0], target[1], psi])
        self.r = new if mask is None else torch.where(mask[None, :], new, self.r)

    def reset(self, ref, mask=None):
        """At rest on ref [3, n] (pos = target = ref, vel = acc = 0) for the envs in mask (None = all): every reset path."""
        import torch
        ref = torch.as_tensor(ref, device=self.r.device).to(self.dtype)
        rest = torch.stack([ref, torch.zeros_like(ref), torch.zeros_like(ref)])
        if mask is None:
            self.x, self.r = rest, ref.clone()
        else:
            self.x = torch.where(mask[None, None, :], rest, self.x)
            self.r = torch.where(mask[None, :], ref, self.r)


# ---- the classical baseline: PID motion controller + weighted pseudo-inverse allocation (include/dpenv.h has the law) -------------------
DP_TAU_MAX = (69.0, 30.0, 80.0)                 # SupervisedTau.py:37
DP_Z_BOUND = (10.0, 10.0, 2.0)
DP_F_EPS = 1e-6


def allocation_matrix(lx, ly, weight=(1.0, 1.0, 1.0, 1.0, 1.0)):
    """G [5, 3] float64: the weighted pseudo-inverse W^-1 T' (T W^-1 T')^-1 of the extended-thrust matrix
        T = [[0, 1, 0, 1, 0], [1, 0, 1, 0, 1], [lx_bow, -ly_port, lx_port, -ly_star, lx_star]],   W = diag(weight)
    whose columns are Fy_bow, Fx_port, Fy_port, Fx_star, Fy_star; lx, ly in env order bow, port, star.  The recipe and the
    operation order of dpenv_dp_allocation_matrix (V = W^-1 T', M = T V, G = V adj(M) / det(M)), which rounds the result to f32."""
    lx, ly, w = [float(v) for v in lx], [float(v) for v in ly], [float(v) for v in weight]
    if len(w) != 5 or not all(np.isfinite(v) and v > 0 for v in w):
        raise ValueError('allocation_matrix: five finite weights > 0')
    T = [[0.0, 1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0, 1.0], [lx[0], -ly[1], lx[1], -ly[2], lx[2]]]
    V = [[T[j][m] / w[m] for j in range(3)] for m in range(5)]
    M = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for m in range(5):
                acc += T[r][m] * V[m][c]
            M[r][c] = acc
    adj = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            adj[r][c] = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]
    det = (M[0][0] * adj[0][0] + M[0][1] * adj[1][0]) + M[0][2] * adj[2][0]
    if not np.isfinite(det) or det == 0.0:
        raise ValueError("allocation_matrix: T W^-1 T' is singular")
    G = np.zeros((5, 3))
    for m in range(5):
        for c in range(3):
            acc = 0.0
            for j in range(3):
                acc += V[m][j] * adj[j][c]
            G[m, c] = acc / det
    return G


def allocation_matrix_batched(lx, ly, weight, check=True):
    """allocation_matrix for n rows at once: lx, ly [n, 3], weight [n, 5] -> G [n, 5, 3] float64.  The vectorised NumPy statement of the
    same recipe - the same operations in the same order, so every row equals allocation_matrix of that row bit for bit - and the host
    statement of what the library's packing kernel computes for every env of a controller table (dpenv_set_dp_controller_table) before it
    rounds to f32.  check=True raises ValueError for a row allocation_matrix would refuse; check=False leaves such rows non-finite."""
    lx, ly, w = (np.asarray(v, np.float64) for v in (lx, ly, weight))
    n = lx.shape[0]
    if lx.shape != (n, 3) or ly.shape != (n, 3) or w.shape != (n, 5):
        raise ValueError('allocation_matrix_batched: lx, ly [n, 3] and weight [n, 5]')
    bad = ~(np.isfinite(w) & (w > 0)).all(1)
    if check and bad.any():
        raise ValueError('allocation_matrix_batched: five finite weights > 0 (rows %s)' % np.flatnonzero(bad)[:8].tolist())
    zero, one = np.zeros(n), np.ones(n)
    T = [[zero, one, zero, one, zero], [one, zero, one, zero, one], [lx[:, 0], -ly[:, 1], lx[:, 1], -ly[:, 2], lx[:, 2]]]
    with np.errstate(all='ignore'):
        V = [[T[j][m] / w[:, m] for j in range(3)] for m in range(5)]
        M = [[None] * 3 for _ in range(3)]
        for r in range(3):
            for c in range(3):
                acc = np.zeros(n)
                for m in range(5):
                    acc = acc + T[r][m] * V[m][c]
                M[r][c] = acc
        adj = [[None] * 3 for _ in range(3)]
        for r in range(3):
            for c in range(3):
                r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
                adj[r][c] = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]
        det = (M[0][0] * adj[0][0] + M[0][1] * adj[1][0]) + M[0][2] * adj[2][0]
        bad = ~np.isfinite(det) | (det == 0.0)
        if check and bad.any():
            raise ValueError("allocation_matrix_batched: T W^-1 T' is singular (rows %s)" % np.flatnonzero(bad)[:8].tolist())
        G = np.zeros((n, 5, 3))
        for m in range(5):
            for c in range(3):
                acc = np.zeros(n)
                for j in range(3):
                    acc = acc + V[m][j] * adj[j][c]
                G[:, m, c] = acc / det
    return G


# the public per-env controller table float[32][n] (include/dpenv.h DPENV_CTRL_*): parameter name -> (first slot, width)
CTRL_NPARAM = 32
CTRL_SLOTS = dict(kp=(0, 3), kd=(3, 3), ki=(6, 3), z_bound=(9, 3), tau_max=(12, 3), weight=(15, 5), lx=(20, 3), ly=(23, 3), kf=(26, 3),
                  kr_bow=(29, 1), f_eps=(30, 1))


def dp_controller_table(n, params=None, **per_env):
    """The public controller table [32, n] float32 in the slot order of include/dpenv.h (env.set_dp_controller_table takes it as a
    tensor): every env starts from params (the dict of dp_controller_defaults; None = the default hull's), and any of kp, kd, ki, z_bound,
    tau_max, weight, lx, ly, kf, kr_bow, f_eps may be given per env as an array with a leading n.  The table carries lever arms and
    weights, not G: the library computes every env's G from them (allocation_matrix_batched is that computation)."""
    p = dp_controller_defaults() if params is None else params
    unknown = sorted(set(per_env) - set(CTRL_SLOTS))
    if unknown:
        raise TypeError('dp_controller_table: unknown per-env parameter(s) %s (of %s)' % (unknown, sorted(CTRL_SLOTS)))
    tab = np.zeros((CTRL_NPARAM, int(n)), np.float32)
    for name, (first, width) in CTRL_SLOTS.items():
        if name in per_env:
            v = np.asarray(per_env[name], np.float64)
            if v.shape not in ((n, width),) + (((n,),) if width == 1 else ()):
                raise ValueError('dp_controller_table: %s has shape %s, want [%d, %d]' % (name, v.shape, n, width))
            tab[first:first + width] = v.reshape(n, width).T
        else:
            v = np.asarray(p[name], np.float64).reshape(-1)
            if v.shape != (width,):
                raise ValueError('dp_controller_table: params[%r] has %d entries, want %d' % (name, v.size, width))
            tab[first:first + width] = v[:, None]
    return tab


def dp_controller_table_params(table):
    """The per-env parameter dict BatchedDPController takes for a public table [32, n]: every entry with a leading n, G [n, 5, 3] the
    float64 allocation matrix of each row's f32 lever arms and weights (rounded to f32 by the controller, once, as the library does).
    Rows the library would refuse are not treated here (their G is non-finite or the law meaningless)."""
    tab = np.asarray(table, np.float32)
    if tab.ndim != 2 or tab.shape[0] != CTRL_NPARAM:
        raise ValueError('dp_controller_table_params: a [32, n] table')
    p = {}
    for name, (first, width) in CTRL_SLOTS.items():
        v = tab[first:first + width].T.astype(np.float64)
        p[name] = v[:, 0] if width == 1 else v
    p['G'] = allocation_matrix_batched(p['lx'], p['ly'], p['weight'], check=False)
    return p


def gain_population(K, base=None, span=4.0, seed=0, what=('kp', 'kd', 'ki')):
    """K parameter sets around base (the dict of dp_controller_defaults; None = the default hull's) for evaluate.baseline_gain_sweep: the
    dict of base with every entry named in `what` as an array [K, 3].  Row 0 is the base itself; the others multiply each named gain, per
    axis, by a factor drawn log-uniformly from [1 / span, span] (np.random.RandomState(seed): the same sets for the same arguments).
    'factors' holds the factors drawn, name -> [K, 3]."""
    base = dp_controller_defaults() if base is None else base
    span = float(span)
    if K < 1 or not span >= 1.0:
        raise ValueError('gain_population: K >= 1 and span >= 1')
    rng = np.random.RandomState(seed)
    lo, hi = 1.0 / span, span
    pop = dict(base)
    pop['factors'] = {}
    for name in what:
        b = np.asarray(base[name], np.float64)
        f = np.clip(np.exp(rng.uniform(np.log(lo), np.log(hi), size=(K,) + b.shape)), lo, hi)
        f[0] = 1.0
        pop['factors'][name] = f
        pop[name] = b[None] * f
    return pop


def dp_controller_defaults(vessel=None, omega=REFERENCE_FILTER_OMEGA, zeta=(1.0, 1.0, 1.0), weight=(1.0, 1.0, 1.0, 1.0, 1.0)):
    """The baseline's default numbers for a hull (public parameter vector; None = the default hull), float64: Fossen's pole placement
    with the reference filter's bandwidths - Kp = m omega^2, Kd = 2 zeta omega m - d, Ki = Kp omega / 10 with m = (m11, m22, m33) and
    d = (Xu, Yv, Nr) - z_bound (10, 10, 2), tau_max (69, 30, 80) (SupervisedTau.py:37), f_eps 1e-6 N, the hull's thrust constants and
    G = allocation_matrix of its lever arms.  Returns the dict BatchedDPController and env.set_dp_controller take."""
    from . import _lib
    v = np.asarray(_lib.default_vessel() if vessel is None else vessel, np.float64)
    P = _lib.P
    m = np.array([v[P['M11']], v[P['M22']], v[P['M33']]])
    d = np.array([v[P['XU']], v[P['YV']], v[P['NR']]])
    w, z = np.asarray(omega, np.float64), np.asarray(zeta, np.float64)
    kp = m * w * w
    lx, ly = v[P['LX_BOW']:P['LX_BOW'] + 3], v[P['LY_BOW']:P['LY_BOW'] + 3]
    return dict(kp=kp, kd=2.0 * z * w * m - d, ki=kp * w / 10.0, z_bound=np.array(DP_Z_BOUND), tau_max=np.array(DP_TAU_MAX),
                G=allocation_matrix(lx, ly, weight), kf=v[P['KF_BOW']:P['KF_BOW'] + 3].copy(), kr_bow=float(v[P['KR_BOW']]),
                f_eps=DP_F_EPS, lx=lx.copy(), ly=ly.copy(), weight=np.asarray(weight, np.float64))


class BatchedDPController(object):
    """The baseline law for n envs on the host: the statement of include/dpenv.h, operation by operation.  With NumPy float32 on the CPU
    (the default) it reproduces the closed-loop kernel's actions bit for bit; dtype=np.float64 is the form for checks.  device other than
    'cpu' (or a torch dtype) runs the same expressions on torch tensors - the eager composition env.step(ctrl.act(obs)) on the device.
    params: the dict of dp_controller_defaults.  act(obs [n, >=6]) advances z [n, 3] one control step and returns the action [n, 7];
    reset(mask) zeroes z of the envs in mask (None = all); allocate(tau [n, 3]) is the stateless allocation.
    Per-env parameters (the law of dpenv_set_dp_controller_table, env i on its own row): params is a public table [32, n]
    (dp_controller_table) or a dict whose entries carry a leading n - kp [n, 3] ... G [n, 5, 3], kr_bow and f_eps [n]; shared and per-env
    entries may be mixed.  The expressions are the same, so all-equal rows give the shared form's bits."""

    def __init__(self, n, params=None, dt=0.2, dtype=None, device='cpu'):
        p = dp_controller_defaults() if params is None else params
        if not isinstance(p, dict):
            p = dp_controller_table_params(p.detach().cpu().numpy() if hasattr(p, 'detach') else p)
        for name, shape in (('kp', (3,)), ('kd', (3,)), ('ki', (3,)), ('z_bound', (3,)), ('tau_max', (3,)), ('G', (5, 3)), ('kf', (3,)),
                            ('kr_bow', ()), ('f_eps', ())):
            if np.shape(p[name]) not in (shape, (n,) + shape):
                raise ValueError('BatchedDPController: %s has shape %s, want %s or %s' % (name, np.shape(p[name]), shape, (n,) + shape))
        self.torch = None
        if str(device) != 'cpu' or type(dtype).__module__ == 'torch':
            import torch
            self.torch = torch
            self.dtype = torch.float32 if dtype is None else dtype
            is32 = self.dtype == torch.float32
            t = lambda v: torch.as_tensor(np.asarray(v, np.float64), device=device).to(self.dtype)
            self.z = torch.zeros((n, 3), dtype=self.dtype, device=device)
        else:
            self.dtype = np.dtype(np.float32 if dtype is None else dtype)
            is32 = self.dtype == np.dtype(np.float32)
            t = lambda v: np.asarray(v, np.float64).astype(self.dtype)
            self.z = np.zeros((n, 3), self.dtype)
        self.kp, self.kd, self.ki, self.zb, self.tmax = t(p['kp']), t(p['kd']), t(p['ki']), t(p['z_bound']), t(p['tau_max'])
        self.G, self.kf, self.kr_bow, self.f_eps = t(p['G']), t(p['kf']), t(p['kr_bow']), t(p['f_eps'])
        self.dt = t(np.float32(dt)) if is32 else t(dt)          # f32: n_substeps * substep_dt as the library forms it
        self.hundred, self.one, self.zero = t(100.0), t(1.0), t(0.0)

    def _xp(self):
        return self.torch if self.torch is not None else np

    def allocate(self, tau):
        xp = self._xp()
        G = self.G
        f = [(G[..., m, 0] * tau[:, 0] + G[..., m, 1] * tau[:, 1]) + G[..., m, 2] * tau[:, 2] for m in range(5)]
        kb = xp.where(f[0] >= self.zero, self.kf[..., 0], self.kr_bow)
        nb = xp.copysign(xp.sqrt(xp.abs(f[0]) / kb), f[0])
        cols = [xp.fmin(xp.fmax(nb / self.hundred, -self.one), self.one)]       # every clip is the stated fminf(fmaxf()): a NaN is dropped
        sc = []
        with np.errstate(invalid='ignore', divide='ignore'):
            for k in range(2):
                Fx, Fy = f[1 + 2 * k], f[2 + 2 * k]
                F = xp.sqrt(Fx * Fx + Fy * Fy)
                ns = xp.sqrt(F / self.kf[..., 1 + k])
                cols.append(xp.fmin(ns / self.hundred, self.one))
                dirn = F > self.f_eps
                sc += [xp.where(dirn, Fy / F, self.zero), xp.where(dirn, Fx / F, self.one)]
        return xp.stack(cols + sc, 1)

    def wrench(self, obs):
        """Advance z on obs and return the clipped tau [n, 3]."""
        xp = self._xp()
        e, nu = obs[:, 0:3], obs[:, 3:6]
        if self.torch is not None:
            e, nu = e.to(self.dtype), nu.to(self.dtype)
        else:
            e, nu = np.asarray(e, self.dtype), np.asarray(nu, self.dtype)
        self.z = xp.fmin(xp.fmax(self.z + self.dt * e, -self.zb), self.zb)
        tau = -((self.kp * e + self.kd * nu) + self.ki * self.z)
        return xp.fmin(xp.fmax(tau, -self.tmax), self.tmax)

    def act(self, obs):
        return self.allocate(self.wrench(obs))

    def reset(self, mask=None):
        if mask is None:
            self.z = self.z * 0
        else:
            self.z[mask] = 0


def label_rows(params_or_table, obs, done=None, z=None, dt=0.2, dtype=None):
    """The baseline's actions on a block of observation rows some other flight wrote - the host statement of dpenv_controller_label
    (policy.controller_label), NumPy on the CPU.  obs [T, n, >= 6] (columns 0:6 read), done [T, n] (any non-zero byte ends an episode) or
    None, z [3, n] the integral each env starts from (get_dp_controller_state's layout) or None = 0.  Per row t, in this order:
        tau = ctrl.wrench(obs[t]);  act[t] = ctrl.allocate(tau);  ctrl.reset(done[t] != 0)
    - z is advanced before the wrench and zeroed BEHIND a done row, so the next row is a new episode's first.  params_or_table: the dict
    of dp_controller_defaults (None = the defaults) or a public table [32, n], as BatchedDPController takes them; dt the control period.
    Returns (act [T, n, 7], z [3, n]) in dtype (None = float32, which reproduces the kernel's bits); labelling rows [0:k] and [k:T] with z
    handed over equals one call."""
    obs, done, T, n = _label_block('label_rows', obs, done)
    ctrl = BatchedDPController(n, params_or_table, dt=dt, dtype=dtype)
    (act,), z = _label_scan('label_rows', ctrl, obs, done, z, (7,), lambda t, tau, ended: (ctrl.allocate(tau),))
    return act, z


def _label_block(who, obs, done):
    """The block a host labelling scan reads, checked under the caller's name: (obs [T, n, >= 6], done [T, n] or None, T, n) as arrays."""
    obs = np.asarray(obs)
    if obs.ndim != 3 or obs.shape[2] < 6:
        raise ValueError('%s: obs is [T, n, >= 6]' % who)
    T, n = obs.shape[0], obs.shape[1]
    if done is not None:
        done = np.asarray(done)
        if done.shape != (T, n):
            raise ValueError('%s: done is [T, n]' % who)
    return obs, done, T, n


def _label_scan(who, ctrl, obs, done, z, widths, stage):
    """The host labelling scan of label_rows, label_rows_qp and label_rows_nn on a block of _label_block: ctrl, the PID
    (BatchedDPController), starts from z [3, n] (None = where it is), and per row t, in this order:
        tau = ctrl.wrench(obs[t]);  outputs[t] = stage(t, tau, ended);  ctrl.reset(ended)
    with ended = (done[t] != 0), or None where done is None (nothing is reset then).  stage is the allocation stage: it returns one row
    [n, w] per width w in `widths` and resets its OWN state behind an ended row.  Returns (one [T, n, w] array per width in ctrl's
    dtype, z [3, n])."""
    T, n = obs.shape[0], obs.shape[1]
    if z is not None:
        z = np.asarray(z)
        if z.shape != (3, n):
            raise ValueError('%s: z is [3, n]' % who)
        ctrl.z = np.ascontiguousarray(z.T).astype(ctrl.dtype)
    outs = tuple(np.empty((T, n, w), ctrl.dtype) for w in widths)
    for t in range(T):
        ended = None if done is None else done[t] != 0
        for o, row in zip(outs, stage(t, ctrl.wrench(obs[t]), ended)):
            o[t] = row
        if ended is not None:
            ctrl.reset(ended)
    return outs, np.ascontiguousarray(np.asarray(ctrl.z).T)


QP_MAX_ITERATIONS = 32


def qp_allocator_defaults(vessel=None):
    """The rate-limited QP allocator's default numbers (dpenv_qp_allocator_defaults; qp_allocator.py:52-58,116-150), env order bow, port,
    star: slack, power and change weights, force bounds, force rates [N/s] and azimuth rates [rad/s] (2, 5, 5 N and pi/12 per 0.2 s
    step), and the lever arms and thrust constants of `vessel` (public parameter vector; None = the default hull).  Returns the dict
    BatchedQPAllocator and policy.thrust_alloc_qp take."""
    from . import _lib
    v = np.asarray(_lib.default_vessel() if vessel is None else vessel, np.float64)
    P = _lib.P
    return dict(iterations=16, w_slack=np.ones(3), w_power=1.0, w_dalpha=0.25, w_dforce=0.25, f_max=np.array([9.0, 20.5, 20.5]),
                force_rate=np.array([10.0, 25.0, 25.0]), azimuth_rate=np.full(2, 5.0 * np.pi / 12.0),
                lx=v[P['LX_BOW']:P['LX_BOW'] + 3].copy(), ly=v[P['LY_BOW']:P['LY_BOW'] + 3].copy(),
                kf=v[P['KF_BOW']:P['KF_BOW'] + 3].copy(), kr=v[P['KR_BOW']:P['KR_BOW'] + 3].copy())


# the public per-env QP table float[32][n] (include/dpenv.h DPENV_QP_*): parameter name -> (first slot, width), in the order of
# dpenv_qp_allocator's fields; the iteration count is not in the table (one number per call)
QP_NPARAM = 32
QP_SLOTS = dict(w_slack=(0, 3), w_power=(3, 1), w_dalpha=(4, 1), w_dforce=(5, 1), f_max=(6, 3), force_rate=(9, 3), azimuth_rate=(12, 2),
                lx=(14, 3), ly=(17, 3), kf=(20, 3), kr=(23, 3))


def qp_allocator_table(n, params=None, **per_env):
    """The public QP table [32, n] float32 in the slot order of include/dpenv.h (env.set_qp_allocator_table and policy.thrust_alloc_qp take
    it as a tensor): every env starts from params (the dict of qp_allocator_defaults; None = the default hull's), and any of w_slack,
    w_power, w_dalpha, w_dforce, f_max, force_rate, azimuth_rate, lx, ly, kf, kr may be given per env as an array with a leading n.  The
    table carries rates, not per-step limits: the library multiplies by its dt.  The iteration count is not in the table: an `iterations`
    entry is accepted and ignored, so qp_allocator_table(n, **qp_allocator_table_params(table)) is the table again."""
    p = qp_allocator_defaults() if params is None else params
    per_env.pop('iterations', None)
    unknown = sorted(set(per_env) - set(QP_SLOTS))
    if unknown:
        raise TypeError('qp_allocator_table: unknown per-env parameter(s) %s (of %s)' % (unknown, sorted(QP_SLOTS)))
    tab = np.zeros((QP_NPARAM, int(n)), np.float32)
    for name, (first, width) in QP_SLOTS.items():
        if name in per_env:
            v = np.asarray(per_env[name], np.float64)
            if v.shape not in ((n, width),) + (((n,),) if width == 1 else ()):
                raise ValueError('qp_allocator_table: %s has shape %s, want [%d, %d]' % (name, v.shape, n, width))
            tab[first:first + width] = v.reshape(n, width).T
        else:
            v = np.asarray(p[name], np.float64).reshape(-1)
            if v.shape != (width,):
                raise ValueError('qp_allocator_table: params[%r] has %d entries, want %d' % (name, v.size, width))
            tab[first:first + width] = v[:, None]
    return tab


def qp_allocator_table_params(table, iterations=16):
    """The per-env parameter dict BatchedQPAllocator takes for a public table [32, n]: every entry with a leading n (float64 of the
    table's f32 numbers), plus iterations.  qp_allocator_table(n, **that dict without iterations) is the table again.  Rows the library
    would refuse are not treated here."""
    tab = np.asarray(table, np.float32)
    if tab.ndim != 2 or tab.shape[0] != QP_NPARAM:
        raise ValueError('qp_allocator_table_params: a [32, n] table')
    p = dict(iterations=int(iterations))
    for name, (first, width) in QP_SLOTS.items():
        v = tab[first:first + width].T.astype(np.float64)
        p[name] = v[:, 0] if width == 1 else v
    return p


def qp_weight_population(K, base=None, span=4.0, seed=0, what=('w_power', 'w_dalpha', 'w_dforce')):
    """K QP parameter sets around base (the dict of qp_allocator_defaults; None = the default hull's) for evaluate.qp_weight_sweep:
    gain_population's contract.  The dict of base with every entry named in `what` as an array with a leading K; row 0 is the base
    itself, the others multiply each named entry (per component) by a factor drawn log-uniformly from [1 / span, span]
    (np.random.RandomState(seed): the same sets for the same arguments).  'factors' holds the factors drawn, name -> [K, ...]."""
    base = qp_allocator_defaults() if base is None else base
    span = float(span)
    if K < 1 or not span >= 1.0:
        raise ValueError('qp_weight_population: K >= 1 and span >= 1')
    unknown = sorted(set(what) - set(QP_SLOTS))
    if unknown:
        raise ValueError('qp_weight_population: unknown parameter(s) %s (of %s)' % (unknown, sorted(QP_SLOTS)))
    rng = np.random.RandomState(seed)
    lo, hi = 1.0 / span, span
    pop = dict(base)
    pop['factors'] = {}
    for name in what:
        b = np.asarray(base[name], np.float64)
        f = np.clip(np.exp(rng.uniform(np.log(lo), np.log(hi), size=(K,) + b.shape)), lo, hi)
        f[0] = 1.0
        pop['factors'][name] = f
        pop[name] = b[None] * f
    return pop


def _qp_wrap(a, dtype):
    """[-pi, pi) in dtype: a - 2 pi floor((a + pi) / (2 pi)), the last step one fused multiply-add (formed in float64 and rounded once)."""
    dtype = np.dtype(dtype)
    t = dtype.type
    pi = t(np.float32(np.pi)) if dtype == np.dtype(np.float32) else t(np.pi)
    k = np.floor((a + pi) * (t(0.5) / pi))
    return (np.asarray(a, np.float64) - np.asarray(k, np.float64) * np.float64(t(2.0) * pi)).astype(dtype)


def _qp_state(kf, kr, fmax, act, dtype):
    """S of include/dpenv.h on act [n, 7] with kf, kr, fmax [3] or [n, 3] already in dtype: x [n, 5]."""
    dtype = np.dtype(dtype)
    t = dtype.type
    a = np.asarray(act).astype(dtype)
    pi = t(np.float32(np.pi)) if dtype == np.dtype(np.float32) else t(np.pi)
    with np.errstate(all='ignore'):
        n3 = a[:, 0:3]
        thr = np.fmin(np.fmax(n3 * t(100.0), -t(100.0)), t(100.0))
        K = np.where(thr >= 0, kf, kr)
        F = (K * thr) * np.abs(thr)
        F = np.fmin(np.fmax(F, -fmax), fmax)
        F = np.where(np.isfinite(n3) & np.isfinite(F), F, t(0.0))
        s, c = a[:, 3:7:2], a[:, 4:7:2]
        al = np.arctan2(s, c).astype(dtype)
        al = _qp_wrap(np.fmin(np.fmax(al, -pi), pi), dtype)
        al = np.where(np.isfinite(s) & np.isfinite(c) & np.isfinite(al), al, t(0.0))
    return np.concatenate([F, al], 1).astype(dtype)


def qp_state_from_action(params_or_table, act, dtype=None):
    """S(q, a) of include/dpenv.h (dpenv_controller_label_qp_ex): the thruster state x [n, 5] = F_bow, F_port, F_star, a_port, a_star that
    the EXECUTED action rows act [n, 7] of the final variant's continuous-angle form leave - the env's command decode (thrust percent
    clipped to +-100, azimuth = arctan2 of the heads clipped to +-pi), the QP's thrust law F = K n |n| clipped to +-f_max, the azimuths
    wrapped to [-pi, pi).  A component fed by an entry that is not finite is 0.  params_or_table: the dict of qp_allocator_defaults (None =
    the defaults; entries may carry a leading n) or a public table [32, n]; of it kf, kr and f_max are read.  dtype float32 (the default)
    is the kernel's arithmetic except for the arctangent (np.arctan2 here, the kernel's own polynomial there: the forces agree in bits);
    float64 is the form for checks."""
    p = qp_allocator_defaults() if params_or_table is None else params_or_table
    if not isinstance(p, dict):
        p = qp_allocator_table_params(p.detach().cpu().numpy() if hasattr(p, 'detach') else p)
    dtype = np.dtype(np.float32 if dtype is None else dtype)
    act = np.asarray(act)
    if act.ndim != 2 or act.shape[1] != 7:
        raise ValueError('qp_state_from_action: act is [n, 7]')
    kf, kr, fmax = (np.asarray(p[k], np.float64).astype(dtype) for k in ('kf', 'kr', 'f_max'))
    for v in (kf, kr, fmax):
        if v.shape not in ((3,), (act.shape[0], 3)):
            raise ValueError('qp_state_from_action: kf, kr and f_max are [3] or [n, 3]')
    return _qp_state(kf, kr, fmax, act, dtype)


# the REST allocator a refused row of a per-env QP table is replaced by (include/dpenv.h): zero thrust, azimuths held, every output finite
QP_REST = dict(w_slack=0.0, w_power=0.0, w_dalpha=1.0, w_dforce=1.0, f_max=0.0, force_rate=0.0, azimuth_rate=0.0, lx=0.0, ly=0.0, kf=1.0, kr=1.0)


def qp_table_refused(table, dt):
    """The mask [n] (bool) of the rows of a public QP table [32, n] the library refuses - the byte dpenv_thrust_alloc_qp_table,
    dpenv_set_qp_allocator_table and dpenv_controller_label_qp_ex set in refused_out: a number that is not finite, a weight < 0, w_dalpha
    or w_dforce <= 0, a bound or rate < 0, kf or kr <= 0, or a dF = force_rate * dt / da = azimuth_rate * dt (one float32 product each)
    that is not finite.  Slots 26-31 are not read."""
    tab = np.asarray(table.detach().cpu().numpy() if hasattr(table, 'detach') else table, np.float32)
    if tab.ndim != 2 or tab.shape[0] != QP_NPARAM:
        raise ValueError('qp_table_refused: a [32, n] table')
    dt = np.float32(dt)
    ok = np.isfinite(tab[0:26]).all(0)
    with np.errstate(all='ignore'):
        for name in ('w_slack', 'w_power', 'f_max', 'force_rate', 'azimuth_rate'):
            first, width = QP_SLOTS[name]
            ok &= (tab[first:first + width] >= 0).all(0)
        for name in ('w_dalpha', 'w_dforce', 'kf', 'kr'):
            first, width = QP_SLOTS[name]
            ok &= (tab[first:first + width] > 0).all(0)
        for name in ('force_rate', 'azimuth_rate'):
            first, width = QP_SLOTS[name]
            ok &= np.isfinite(tab[first:first + width] * dt).all(0)
    return ~ok


class BatchedQPAllocator(object):
    """The rate-limited QP thrust allocation for n envs on the host: the statement of include/dpenv.h (dpenv_thrust_alloc_qp), operation
    by operation, in batched NumPy.  dtype float32 (the default) is the kernel's arithmetic except for sin / cos (np.sin / np.cos here, the
    kernel's own polynomial there); float64 is the form for checks.  params: the dict of qp_allocator_defaults; dt the control period.
    State x [n, 5] = F_bow, F_port, F_star, a_port, a_star (the thruster state in force, azimuths wrapped to [-pi, pi)).
    allocate(tau [n, 3]) advances the state one control step and returns the action [n, 7]; an env whose tau is not finite keeps its
    state and commands it.  reset(mask) zeroes the state of the envs in mask (None = all).  objective(x, tau, prev) is J [n].
    After allocate: last_x is the un-wrapped solution, last_J the objective per iteration [iterations + 1, n].
    Per-env parameters (the law of dpenv_set_qp_allocator_table, env i on its own row): params is a public table [32, n]
    (qp_allocator_table; `iterations` then gives the count, default 16) or a dict whose entries carry a leading n - w_slack [n, 3] ...
    w_power [n]; shared and per-env entries may be mixed.  The expressions are the same, so all-equal rows give the shared form's bits."""

    def __init__(self, n, params=None, dt=0.2, dtype=None, iterations=None):
        p = qp_allocator_defaults() if params is None else params
        if not isinstance(p, dict):
            p = qp_allocator_table_params(p.detach().cpu().numpy() if hasattr(p, 'detach') else p, 16 if iterations is None else iterations)
        elif iterations is not None:
            p = dict(p, iterations=iterations)
        self.dtype = np.dtype(np.float32 if dtype is None else dtype)
        is32 = self.dtype == np.dtype(np.float32)
        t = lambda v: np.asarray(v, np.float64).astype(self.dtype)
        self.n = int(n)
        self.iterations = int(p['iterations'])
        if not 1 <= self.iterations <= QP_MAX_ITERATIONS:
            raise ValueError('BatchedQPAllocator: iterations must be in 1..%d' % QP_MAX_ITERATIONS)
        for name, shape in (('w_slack', (3,)), ('f_max', (3,)), ('force_rate', (3,)), ('azimuth_rate', (2,)), ('lx', (3,)), ('ly', (3,)),
                            ('kf', (3,)), ('kr', (3,))):
            if np.shape(p[name]) not in (shape, (self.n,) + shape):
                raise ValueError('BatchedQPAllocator: %s has shape %s, want %s or %s' % (name, np.shape(p[name]), shape, (self.n,) + shape))
        for name in ('w_power', 'w_dalpha', 'w_dforce'):
            if np.shape(p[name]) not in ((), (self.n,)):
                raise ValueError('BatchedQPAllocator: %s has shape %s, want a scalar or %s' % (name, np.shape(p[name]), (self.n,)))
        self.ws, self.wp, self.wda, self.wdf = t(p['w_slack']), t(p['w_power']), t(p['w_dalpha']), t(p['w_dforce'])
        self.fmax, self.lx, self.ly, self.kf, self.kr = t(p['f_max']), t(p['lx']), t(p['ly']), t(p['kf']), t(p['kr'])
        dt = t(np.float32(dt)) if is32 else t(dt)                 # f32: the library's n_substeps * substep_dt
        self.dF, self.da = t(p['force_rate']) * dt, t(p['azimuth_rate']) * dt
        self.x = np.zeros((self.n, 5), self.dtype)
        self.last_x, self.last_J = self.x.copy(), None

    def box(self, prev):
        """(lo, hi) [n, 5] of one control step from the state prev [n, 5]."""
        Fp, ap = prev[:, 0:3], prev[:, 3:5]
        lo = np.concatenate([np.fmax(-self.fmax, Fp - self.dF), ap - self.da], 1)
        hi = np.concatenate([np.fmin(self.fmax, Fp + self.dF), ap + self.da], 1)
        return lo, hi

    def _residual(self, x, tau):
        """sin, cos [n, 2], the moment arms b3 [n, 2] and r [n, 3] at x."""
        F = x[:, 0:3]
        s, c = np.sin(x[:, 3:5]).astype(self.dtype), np.cos(x[:, 3:5]).astype(self.dtype)
        b3 = self.lx[..., 1:3] * s - self.ly[..., 1:3] * c
        r0 = (c[:, 0] * F[:, 1] + c[:, 1] * F[:, 2]) - tau[:, 0]
        r1 = ((F[:, 0] + s[:, 0] * F[:, 1]) + s[:, 1] * F[:, 2]) - tau[:, 1]
        r2 = ((self.lx[..., 0] * F[:, 0] + b3[:, 0] * F[:, 1]) + b3[:, 1] * F[:, 2]) - tau[:, 2]
        return s, c, b3, np.stack([r0, r1, r2], 1)

    def _objective(self, x, r, prev):
        t = self.dtype.type
        F, ws = x[:, 0:3], self.ws
        Js = (ws[..., 0] * (r[:, 0] * r[:, 0]) + ws[..., 1] * (r[:, 1] * r[:, 1])) + ws[..., 2] * (r[:, 2] * r[:, 2])
        c3 = np.abs(F) * (F * F)
        Jp = (c3[:, 0] + c3[:, 1]) + c3[:, 2]
        e = x - prev
        e2 = e * e
        Ja = e2[:, 3] + e2[:, 4]
        Jf = (e2[:, 0] + e2[:, 1]) + e2[:, 2]
        return t(0.5) * (((Js + self.wp * Jp) + self.wda * Ja) + self.wdf * Jf)

    def objective(self, x, tau, prev):
        x, tau, prev = (np.asarray(v, self.dtype) for v in (x, tau, prev))
        return self._objective(x, self._residual(x, tau)[3], prev)

    def solve(self, tau, prev, trace=None):
        """The K iterations from the state prev on tau: (x [n, 5] un-wrapped, J [K + 1, n]).  trace: a dict that receives what the
        iterations computed on their way, one entry per iteration - 'trial_J' [K, n] (J of x_t, step 7), 'accept' [K, n] (step 8),
        'frozen' [K, n, 5] (step 5) and 'g' [K, n, 5] (the gradient of step 2, before the frozen entries are zeroed).  Nothing of the
        solve depends on it."""
        t = self.dtype.type
        tau, prev = np.asarray(tau, self.dtype), np.asarray(prev, self.dtype)
        n = prev.shape[0]
        lo, hi = self.box(prev)
        x = np.fmin(np.fmax(prev, lo), hi)
        s, c, b3, r = self._residual(x, tau)
        J = self._objective(x, r, prev)
        lam = np.zeros(n, self.dtype)
        hist = [J]
        if trace is not None:
            trace.update(trial_J=[], accept=[], frozen=[], g=[])
        zero, one = np.zeros(n, self.dtype), np.ones(n, self.dtype)
        with np.errstate(all='ignore'):
            for _ in range(self.iterations):
                F = x[:, 0:3]
                # the 3 x 5 Jacobian, columns F_bow, F_port, F_star, a_port, a_star
                d3 = self.lx[..., 1:3] * c + self.ly[..., 1:3] * s
                Jm = [[zero, c[:, 0], c[:, 1], -(F[:, 1] * s[:, 0]), -(F[:, 2] * s[:, 1])],
                      [one, s[:, 0], s[:, 1], F[:, 1] * c[:, 0], F[:, 2] * c[:, 1]],
                      [self.lx[..., 0] * one, b3[:, 0], b3[:, 1], F[:, 1] * d3[:, 0], F[:, 2] * d3[:, 1]]]
                wr = [self.ws[..., j] * r[:, j] for j in range(3)]
                WJ = [[self.ws[..., j] * Jm[j][k] for k in range(5)] for j in range(3)]
                g, H = [None] * 5, [[None] * 5 for _ in range(5)]
                for k in range(5):
                    g[k] = (Jm[0][k] * wr[0] + Jm[1][k] * wr[1]) + Jm[2][k] * wr[2]
                    for l in range(k + 1):
                        H[k][l] = (Jm[0][k] * WJ[0][l] + Jm[1][k] * WJ[1][l]) + Jm[2][k] * WJ[2][l]
                for k in range(3):
                    g[k] = g[k] + ((t(1.5) * self.wp) * (F[:, k] * np.abs(F[:, k])) + self.wdf * (F[:, k] - prev[:, k]))
                    H[k][k] = H[k][k] + ((t(3.0) * self.wp) * np.abs(F[:, k]) + self.wdf)
                for k in range(3, 5):
                    g[k] = g[k] + self.wda * (x[:, k] - prev[:, k])
                    H[k][k] = H[k][k] + self.wda
                fr = []
                for k in range(5):
                    H[k][k] = H[k][k] + lam * H[k][k]
                    fr.append(((x[:, k] <= lo[:, k]) & (g[k] > 0)) | ((x[:, k] >= hi[:, k]) & (g[k] < 0)))
                if trace is not None:
                    trace['frozen'].append(np.stack(fr, 1))
                    trace['g'].append(np.stack(g, 1))
                for k in range(5):
                    g[k] = np.where(fr[k], zero, g[k])
                    H[k][k] = np.where(fr[k], one, H[k][k])
                    for l in range(k):
                        H[k][l] = np.where(fr[k] | fr[l], zero, H[k][l])
                # LDL' without pivoting: H = L D L', L unit lower triangular
                L, D, iD = [[None] * 5 for _ in range(5)], [None] * 5, [None] * 5
                for j in range(5):
                    v = [L[j][m] * D[m] for m in range(j)]
                    D[j] = H[j][j]
                    for m in range(j):
                        D[j] = D[j] - L[j][m] * v[m]
                    iD[j] = one / D[j]
                    for i in range(j + 1, 5):
                        a = H[i][j]
                        for m in range(j):
                            a = a - L[i][m] * v[m]
                        L[i][j] = a * iD[j]
                y = [None] * 5
                for i in range(5):
                    a = -g[i]
                    for m in range(i):
                        a = a - L[i][m] * y[m]
                    y[i] = a
                d = [None] * 5
                for i in range(4, -1, -1):
                    a = y[i] * iD[i]
                    for m in range(i + 1, 5):
                        a = a - L[m][i] * d[m]
                    d[i] = a
                xt = np.fmin(np.fmax(x + np.stack(d, 1), lo), hi)
                st, ct, b3t, rt = self._residual(xt, tau)
                Jt = self._objective(xt, rt, prev)
                acc = Jt < J
                if trace is not None:
                    trace['trial_J'].append(Jt)
                    trace['accept'].append(acc)
                a1 = acc[:, None]
                x, s, c, b3, r = np.where(a1, xt, x), np.where(a1, st, s), np.where(a1, ct, c), np.where(a1, b3t, b3), np.where(a1, rt, r)
                J = np.where(acc, Jt, J)
                lam = np.where(acc, t(0.25) * lam, t(8.0) * np.fmax(lam, t(0.125)))
                hist.append(J)
        if trace is not None:
            for k in ('trial_J', 'accept', 'frozen', 'g'):
                trace[k] = np.stack(trace[k])
        return x, np.stack(hist)

    def thrust_columns(self, F):
        """F [n, 3] -> the action's thrust columns: clip(copysign(sqrt(|F| / K), F) / 100, -1, 1), K forward or reverse by F's sign."""
        t = self.dtype.type
        K = np.where(F >= 0, self.kf, self.kr)
        nn = np.copysign(np.sqrt(np.abs(F) / K), F)
        return np.fmin(np.fmax(nn / t(100.0), -t(1.0)), t(1.0))

    def wrap(self, a):
        """[-pi, pi): a - 2 pi floor((a + pi) / (2 pi)), the last step one fused multiply-add (exact here in float64)."""
        return _qp_wrap(a, self.dtype)

    def allocate(self, tau):
        tau = np.asarray(tau, self.dtype)
        prev = self.x
        x, self.last_J = self.solve(tau, prev)
        ok = np.isfinite(tau).all(1)[:, None]
        x = np.where(ok, x, prev)
        self.last_x = x
        self.x = np.where(ok, np.concatenate([x[:, 0:3], self.wrap(x[:, 3:5])], 1), prev)
        s, c = np.sin(x[:, 3:5]).astype(self.dtype), np.cos(x[:, 3:5]).astype(self.dtype)
        return np.concatenate([self.thrust_columns(x[:, 0:3]), np.stack([s[:, 0], c[:, 0], s[:, 1], c[:, 1]], 1)], 1)

    def reset(self, mask=None):
        if mask is None:
            self.x = self.x * 0
        else:
            self.x[mask] = 0


def label_rows_qp(params_or_table, qp_params, obs, done=None, z=None, x=None, dt=0.2, dtype=None, flown=None, iterations=None):
    """The PID + rate-limited QP chain's actions on a block of observation rows some other flight wrote - the host statement of
    dpenv_controller_label_qp (policy.controller_label_qp), NumPy on the CPU.  obs, done and z as label_rows takes them; x [5, n] the
    thruster state each env starts from (get_qp_allocator_state's layout) or None = 0.  Per row t, in this order:
        tau = ctrl.wrench(obs[t]);  act[t] = qp.allocate(tau);  ctrl.reset(done[t] != 0);  qp.reset(done[t] != 0)
    - z is advanced before the wrench, x by the allocation, and both are zeroed BEHIND a done row.  params_or_table: the dict of
    dp_controller_defaults (None = the defaults) or a public table [32, n]; qp_params: the dict of qp_allocator_defaults (None = the
    defaults); dt the control period.  Returns (act [T, n, 7], z [3, n], x [5, n]) in dtype (None = float32: the kernel's arithmetic
    except for its own sin / cos polynomial, as BatchedQPAllocator says; float64 is the form for checks); labelling rows [0:k] and [k:T]
    with z and x handed over equals one call.
    flown [T, n, 7] (dpenv_controller_label_qp_ex): the actions that were EXECUTED on these rows.  Row t is then solved from the thruster
    state the executed row t - 1 left, qp_state_from_action(flown[t - 1]), instead of the expert's own recursion - after the allocation
    of row t, qp.x = S(flown[t]), then the resets; the label of row t does not depend on flown[t:], and x out is the last such state.
    qp_params may be a public QP table [32, n] (env i labelled with row i, in `iterations` solver steps, None = 16): rows the library
    refuses (qp_table_refused) run the rest allocator here too - zero thrust, azimuths held."""
    obs, done, T, n = _label_block('label_rows_qp', obs, done)
    if flown is not None:
        flown = np.asarray(flown)
        if flown.shape != (T, n, 7):
            raise ValueError('label_rows_qp: flown is [T, n, 7]')
    if qp_params is not None and not isinstance(qp_params, dict):                      # a public table: refused rows fly the rest allocator
        tab = np.array(qp_params.detach().cpu().numpy() if hasattr(qp_params, 'detach') else qp_params, np.float32)
        if tab.shape != (QP_NPARAM, n):
            raise ValueError('label_rows_qp: a QP table is [32, n]')
        bad = qp_table_refused(tab, dt)
        for name, (first, width) in QP_SLOTS.items():
            tab[first:first + width, bad] = QP_REST[name]
        qp_params = qp_allocator_table_params(tab, 16 if iterations is None else iterations)
    elif iterations is not None:
        raise ValueError('label_rows_qp: iterations goes with a QP table (the dict carries its own)')
    ctrl = BatchedDPController(n, params_or_table, dt=dt, dtype=dtype)
    qp = BatchedQPAllocator(n, qp_params, dt=dt, dtype=dtype)
    if x is not None:
        x = np.asarray(x)
        if x.shape != (5, n):
            raise ValueError('label_rows_qp: x is [5, n]')
        qp.x = np.ascontiguousarray(x.T).astype(qp.dtype)

    def stage(t, tau, ended):
        act = qp.allocate(tau)
        if flown is not None:                                                          # the law's own advance of x is dropped
            qp.x = _qp_state(qp.kf, qp.kr, qp.fmax, flown[t], qp.dtype)
        if ended is not None:
            qp.reset(ended)
        return (act,)

    (act,), z = _label_scan('label_rows_qp', ctrl, obs, done, z, (7,), stage)
    return act, z, np.ascontiguousarray(np.asarray(qp.x).T)


class RLAllocatorNode(object):
    """The node's callbacks as plain methods (rl_allocator.py:168-220).  `actor(state[9]) -> action[act_dim]` is any
    callable: ActorCritic.forward_ref on the CPU, or policy_forward on the GPU for one env."""

    def __init__(self, actor, variant='final', cont_ang=True, integrator=False, simulation=True, now=0.0):
        if variant == 'simple':
            raise ValueError('no simple environment was trained with the extended state vector')   # rl_allocator.py:126
        self.actor, self.variant, self.cont_ang = actor, variant, cont_ang
        self.simulation = simulation
        self.state = np.zeros(9)
        self.velocities = np.zeros(3)
        self.prev_thrust_state = np.zeros(6)
        self.pos = [0.0, 0.0, 0.0]
        self.ref = [0.0, 0.0, 0.0]
        self.integrator = BodyFrameIntegrator(now) if integrator else None
        self.time_prev = float(now)
        self.h = 0.0

    def _error(self):
        """errorFrame.py transform: rotation by the wrapped heading, yaw error wrapped in radians"""
        e = [a - b for a, b in zip(self.pos, self.ref)]
        rot = float(wrap_angle(self.pos[2]))
        c, s = np.cos(rot), np.sin(rot)
        return np.array([c * e[0] + s * e[1], -s * e[0] + c * e[1], float(wrap_angle(e[2]))])

    def _error_states(self, step, now):
        err = self._error()
        if self.integrator is None:
            return err
        return self.integrator.update(err, step, now)

    def on_eta(self, north, east, heading_deg, now):
        """eta_obs_callback (rl_allocator.py:168-178); note the node integrates here too, with its default step 0.1"""
        self.pos = [float(north), float(east), float(wrap_angle(np.deg2rad(heading_deg)))]
        self.state[0:3] = self._error_states(0.1, now)

    def on_nu(self, u, v, r):
        """nu_obs_callback (:180-187)"""
        self.velocities = np.array([u, v, r], np.float64)
        self.state[3:6] = self.velocities

    def on_reference(self, north, east, heading_deg, now):
        """state_desired_callback (:189-220): returns (u in ROS order, message fields)"""
        self.h = now - self.time_prev
        self.time_prev = now
        self.ref = [float(north), float(east), float(np.deg2rad(heading_deg))]
        self.state[0:3] = self._error_states(self.h, now)
        self.state[3:6] = self.velocities
        u = to_ros_order(np.asarray(self.actor(self.state.copy()), np.float64), self.variant, self.cont_ang)
        self.prev_thrust_state = u.copy()
        self.state[-3:] = np.array([u[2], u[0], u[1]]) / 100.0          # back to network order (:218)
        return u, publishable(u, self.simulation)


# ---- the neural thrust allocation: the reference's supervised allocator (src/sl) ---------------------------------------------------------
NN_TAU_SCALE = (1.0 / 54.0, 1.0 / 69.2, 1.0 / 76.9)              # neural_allocator.py:60, SupervisedTau.py:189
NN_IN_CONST = (-1.12, -0.15, -1.12, 0.15, 1.08, 0.0)             # neural_allocator.py:74-79: lx, ly of port, star, bow
NN_FIXED_AZIMUTH = (-3.0 * np.pi / 4.0, 3.0 * np.pi / 4.0)       # neural_allocator.py:225
NN_REST_ACTION = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0)


def nn_allocator_defaults():
    """The neural allocator's constants (dpenv_nn_allocator_defaults; the node's, neural_allocator.py:50-79,225), float64: leak 0 (relu,
    src/sl/train.py:111), the six lever-arm inputs, the wrench scale, the angle scale pi, azimuth_mode 0 (the network's stern angles; 1 =
    the pods fixed at `azimuth`).  Returns the dict BatchedNNAllocator, policy.thrust_alloc_nn and env.set_nn_allocator take."""
    return dict(leak=0.0, in_const=np.array(NN_IN_CONST), tau_scale=np.array(NN_TAU_SCALE), angle_scale=float(np.pi), azimuth_mode=0,
                azimuth=np.array(NN_FIXED_AZIMUTH))


ALLOC_LOSS_W_SAT = 100.0


def alloc_loss_defaults(vessel=None):
    """The allocation loss's default numbers (dpenv_alloc_loss_defaults; include/dpenv.h, ALLOCATION LOSS), env order bow, port, star: the
    QP's slack and power weights, w_sat = 100 on the thrust commands' excess over +-1, the lever arms and thrust constants of `vessel`
    (public parameter vector; None = the default hull) and the neural allocator's angle_scale, azimuth_mode and azimuth.  Returns the
    dict train.allocation_grad, train.allocation_grad_ref and train.fit_nn_allocator(loss='wrench') take."""
    qp, nn = qp_allocator_defaults(vessel), nn_allocator_defaults()
    return dict(w_slack=qp['w_slack'], w_power=qp['w_power'], w_sat=ALLOC_LOSS_W_SAT, lx=qp['lx'], ly=qp['ly'], kf=qp['kf'], kr=qp['kr'],
                angle_scale=nn['angle_scale'], azimuth_mode=nn['azimuth_mode'], azimuth=nn['azimuth'])


def nn_allocator_params(net=None, **constants):
    """nn_allocator_defaults with `constants` on top; a net dict that carries 'leak' (train.fit_nn_allocator's does) supplies the leak
    unless constants names one."""
    p = nn_allocator_defaults()
    if isinstance(net, dict) and 'leak' in net:
        p['leak'] = float(net['leak'])
    for k, v in constants.items():
        if k not in p:
            raise ValueError('nn allocator: unknown constant %r (known: %s)' % (k, sorted(p)))
        p[k] = v
    return p


def nn_net_sizes(Ws, bs):
    """The layer widths [in, H, ..., H, 6] of dense kernels Ws and biases bs (arrays or tensors; only their shapes are read), with the
    shape dpenv_nn_allocator admits checked: inputs 3 or 9, 2..5 dense layers, equal hidden widths in 1..96, 6 outputs."""
    L = len(Ws)
    if L != len(bs) or not 2 <= L <= 5:
        raise ValueError('nn allocator: 2..5 dense layers, as many W as b')
    if any(len(w.shape) != 2 for w in Ws):
        raise ValueError('nn allocator: W[l] is [in][out]')
    sizes = [int(Ws[0].shape[0])] + [int(w.shape[1]) for w in Ws]
    if any(int(Ws[l].shape[0]) != sizes[l] or int(np.prod(bs[l].shape)) != sizes[l + 1] for l in range(L)):
        raise ValueError('nn allocator: W[l] is [in][out], b[l] is [out], layer by layer')
    if sizes[0] not in (3, 9) or sizes[-1] != 6 or any(h != sizes[1] for h in sizes[1:-1]) or not 1 <= sizes[1] <= 96:
        raise ValueError('nn allocator: sizes %s - inputs 3 or 9, equal hidden widths in 1..96, 6 outputs' % (sizes,))
    return sizes


def nn_net_arrays(net):
    """(Ws, bs) of a net - a dict with 'W' and 'b' (lists of arrays or tensors, W[l] [in][out]) or a pair (Ws, bs) - as float32 NumPy
    arrays, shape checked (nn_net_sizes)."""
    Ws, bs = (net['W'], net['b']) if isinstance(net, dict) else net
    nn_net_sizes(Ws, bs)
    cv = lambda a: np.ascontiguousarray((a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)), dtype=np.float32)
    return [cv(w) for w in Ws], [cv(b).reshape(-1) for b in bs]


class BatchedNNAllocator(object):
    """The neural thrust allocation for n envs on the host: the statement of include/dpenv.h, operation by operation, in batched NumPy.
    dtype float32 (the default) is the device's arithmetic - every product-sum of a layer through the exact host fmaf, in the order of
    k - except for sin / cos (np.sin / np.cos of the f32 angle here, the library's polynomial on the device: the heads agree to 9.2e-8
    plus a rounding, everything else bit for bit); dtype=np.float64 is the form for checks, on the same f32 constants and weights.
    net: see nn_net_arrays; params: the dict of nn_allocator_defaults (None = the defaults, with the net's leak if it carries one).
    allocate(tau [n, 3]) returns the action [n, 7]; with raw=True also the network's outputs p [n, 6].  The law has no state."""

    def __init__(self, n, net, dtype=None, params=None):
        self.n = int(n)
        self.dtype = np.dtype(np.float32 if dtype is None else dtype)
        self.is32 = self.dtype == np.dtype(np.float32)
        self.Ws32, self.bs32 = nn_net_arrays(net)
        p = nn_allocator_params(net) if params is None else params
        t = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(self.dtype)    # the struct's f32 numbers
        self.Ws, self.bs = [w.astype(self.dtype) for w in self.Ws32], [b.astype(self.dtype) for b in self.bs32]
        self.leak, self.in_const, self.tau_scale = t(p['leak']), t(p['in_const']), t(p['tau_scale'])
        self.angle_scale, self.azimuth, self.mode = t(p['angle_scale']), t(p['azimuth']), int(p['azimuth_mode'])
        if self.mode not in (0, 1) or not 0.0 <= float(self.leak) <= 1.0:
            raise ValueError('BatchedNNAllocator: azimuth_mode is 0 or 1, leak in [0, 1]')

    def inputs(self, tau):
        tau = np.asarray(tau, self.dtype)
        if tau.shape != (self.n, 3):
            raise ValueError('BatchedNNAllocator: tau is [n, 3]')
        with np.errstate(all='ignore'):
            x = tau * self.tau_scale
        if self.Ws[0].shape[0] == 9:
            x = np.concatenate([np.broadcast_to(self.in_const, (self.n, 6)), x], 1)
        return tau, x

    def forward(self, x):
        """The network on its inputs x [n, in]: (p [n, 6], hs) with hs[l] the input of dense layer l."""
        h, hs = np.asarray(x, self.dtype), []
        L = len(self.Ws)
        with np.errstate(all='ignore'):
            for l in range(L):
                hs.append(h)
                W, b = self.Ws[l], self.bs[l]
                if self.is32:
                    y = np.broadcast_to(b, (h.shape[0], b.shape[0])).copy()
                    for k in range(W.shape[0]):
                        y = _fma32(W[k][None, :], h[:, k:k + 1], y)
                else:
                    y = h @ W + b
                h = y if l == L - 1 else np.where(y > 0, y, self.leak * y)
        return h, hs

    def allocate(self, tau, raw=False):
        tau, x = self.inputs(tau)
        p, _ = self.forward(x)
        one = self.dtype.type(1.0)
        with np.errstate(all='ignore'):
            thr = np.fmin(np.fmax(p[:, 0:3], -one), one)
            ang = np.broadcast_to(self.azimuth, (self.n, 2)) if self.mode == 1 else p[:, 3:5] * self.angle_scale
            s, c = np.sin(ang.astype(np.float64)).astype(self.dtype), np.cos(ang.astype(np.float64)).astype(self.dtype)
        act = np.stack([thr[:, 2], thr[:, 0], thr[:, 1], s[:, 0], c[:, 0], s[:, 1], c[:, 1]], 1)
        ok = np.isfinite(tau).all(1) & np.isfinite(p).all(1)
        act[~ok] = np.asarray(NN_REST_ACTION, self.dtype)
        return (act, p) if raw else act


# ---- a population of neural allocators: K networks of one shape, one per envs_per_net envs (dpenv_set_nn_allocator_population) ----------
def _is_stacked(nets):
    return isinstance(nets, dict) and len(nets['W']) > 0 and len(nets['W'][0].shape) == 3


def nn_population_stack(nets):
    """K nets of ONE shape -> the stacked dict the population calls take: W[l] [K, in, out], b[l] [K, out], float32.  nets: a list of net
    dicts (nn_net_arrays' forms; train.fit_nn_allocator_population returns one), or a dict that is already stacked (checked and
    returned).  If every array of every net is a torch tensor the stack is a torch tensor on their device (so that
    env.set_nn_allocator_population and policy.thrust_alloc_nn_population read it in place), else float32 NumPy.  A 'leak' the nets
    carry is kept if they agree on it.  ValueError if the shapes differ, the leaks differ, or the list is empty."""
    if isinstance(nets, dict):
        if not _is_stacked(nets):
            raise ValueError('nn_population_stack: a dict is the stacked form, W[l] [K, in, out] and b[l] [K, out] (for one net pass [net])')
        K = int(nets['W'][0].shape[0])
        if K < 1 or any(int(a.shape[0]) != K for a in list(nets['W']) + list(nets['b'])):
            raise ValueError('nn_population_stack: every W[l] and b[l] has the same leading K >= 1')
        nn_net_sizes([w[0] for w in nets['W']], [b[0] for b in nets['b']])
        return nets
    nets = list(nets)
    if not nets:
        raise ValueError('nn_population_stack: no nets')
    pairs = [((n['W'], n['b']) if isinstance(n, dict) else n) for n in nets]
    sizes = [nn_net_sizes(Ws, bs) for Ws, bs in pairs]
    if any(s != sizes[0] for s in sizes):
        raise ValueError('nn_population_stack: the nets of a population have one shape, got %s' % sorted(set(map(tuple, sizes))))
    leaks = set(float(n['leak']) for n in nets if isinstance(n, dict) and 'leak' in n)
    if len(leaks) > 1 or (leaks and not all(isinstance(n, dict) and 'leak' in n for n in nets)):
        raise ValueError('nn_population_stack: the nets of a population share one leak, got %s' % sorted(leaks))
    L = len(sizes[0]) - 1
    if all(hasattr(a, 'detach') for Ws, bs in pairs for a in list(Ws) + list(bs)):
        import torch
        out = dict(W=[torch.stack([p[0][l].detach().float() for p in pairs]).contiguous() for l in range(L)],
                   b=[torch.stack([p[1][l].detach().float().reshape(-1) for p in pairs]).contiguous() for l in range(L)])
    else:
        arrs = [nn_net_arrays(p) for p in pairs]
        out = dict(W=[np.stack([a[0][l] for a in arrs]) for l in range(L)], b=[np.stack([a[1][l] for a in arrs]) for l in range(L)])
    if leaks:
        out['leak'] = leaks.pop()
    return out


def nn_population_net(stacked, k):
    """Network k of a stacked dict (nn_population_stack), as views: dict(W, b[, leak])."""
    out = dict(W=[w[k] for w in stacked['W']], b=[b[k] for b in stacked['b']])
    if 'leak' in stacked:
        out['leak'] = stacked['leak']
    return out


def nn_population_index(n, K, envs_per_net, env_id_base=0):
    """Which network each env flies (the law of dpenv_set_nn_allocator_population): int64 [n], entry i = ((env_id_base + i) //
    envs_per_net) % K.  K >= 1; envs_per_net and env_id_base are multiples of 64 (a wave flies one network), env_id_base >= 0."""
    n, K, E, base = int(n), int(K), int(envs_per_net), int(env_id_base)
    if n < 1 or K < 1:
        raise ValueError('nn_population_index: n and K are >= 1')
    if E < 64 or E % 64:
        raise ValueError('nn_population_index: envs_per_net is a multiple of 64, >= 64 (got %d)' % E)
    if base < 0 or base % 64:
        raise ValueError('nn_population_index: env_id_base is >= 0 and a multiple of 64 (got %d)' % base)
    return ((base + np.arange(n, dtype=np.int64)) // E) % K


class BatchedNNAllocatorPopulation(object):
    """The population's host statement: env i is allocated by BatchedNNAllocator with network nn_population_index(...)[i] - per env
    exactly that class's float32 / float64 statement of the env's network, nothing else.  nets: a list of nets or the stacked dict;
    params, dtype: BatchedNNAllocator's, shared by the K networks.  allocate(tau [n, 3]) -> action [n, 7] (and p [n, 6] with raw=True)."""

    def __init__(self, n, nets, envs_per_net=64, env_id_base=0, dtype=None, params=None):
        st = nn_population_stack(nets)
        self.n, self.K = int(n), int(st['W'][0].shape[0])
        self.index = nn_population_index(n, self.K, envs_per_net, env_id_base)
        self.dtype = np.dtype(np.float32 if dtype is None else dtype)
        self.rows = {int(k): np.flatnonzero(self.index == k) for k in np.unique(self.index)}
        self.allocators = {k: BatchedNNAllocator(len(r), nn_population_net(st, k), dtype=dtype, params=params) for k, r in self.rows.items()}

    def allocate(self, tau, raw=False):
        tau = np.asarray(tau, self.dtype)
        if tau.shape != (self.n, 3):
            raise ValueError('BatchedNNAllocatorPopulation: tau is [n, 3]')
        act, p = np.empty((self.n, 7), self.dtype), np.empty((self.n, 6), self.dtype)
        for k, r in self.rows.items():
            act[r], p[r] = self.allocators[k].allocate(tau[r], raw=True)
        return (act, p) if raw else act


def label_rows_nn(params_or_table, net, obs, done=None, z=None, dt=0.2, dtype=None, nn_params=None):
    """The PID + network chain's actions on a block of observation rows some other flight wrote - the host statement of
    dpenv_controller_label_nn (policy.controller_label_nn), NumPy on the CPU.  obs, done, z, params_or_table and dt as label_rows takes
    them; net and nn_params as BatchedNNAllocator takes them (nn_params None = the defaults with the net's leak).  Per row t, in this order:
        tau[t] = ctrl.wrench(obs[t]);  act[t], raw[t] = alloc.allocate(tau[t], raw=True);  ctrl.reset(done[t] != 0)
    - z is advanced before the wrench and zeroed BEHIND a done row; the network has no state.  Returns (act [T, n, 7], z [3, n],
    raw [T, n, 6], tau [T, n, 3]) in dtype (None = float32: the kernel's bits except for the sin / cos heads, see BatchedNNAllocator);
    labelling rows [0:k] and [k:T] with z handed over equals one call."""
    obs, done, T, n = _label_block('label_rows_nn', obs, done)
    ctrl = BatchedDPController(n, params_or_table, dt=dt, dtype=dtype)
    alloc = BatchedNNAllocator(n, net, dtype=dtype, params=nn_params)
    def stage(t, tau, ended):
        # the law's clip drops a NaN (z_j = -z_bound_j, tau_j = -tau_max_j); the scan says it again: tau_j = NaN if o_j or o_{3+j} is,
        # so the rest rule answers such a row.  z_j stays the law's.
        o = np.asarray(obs[t], ctrl.dtype)
        tau = np.where(np.isnan(o[:, 0:3]) | np.isnan(o[:, 3:6]), ctrl.dtype.type(np.nan), tau)
        return (tau,) + tuple(alloc.allocate(tau, raw=True))

    (tau, act, raw), z = _label_scan('label_rows_nn', ctrl, obs, done, z, (3, 7, 6), stage)
    return act, z, raw, tau


def thrust_map_host(n_pct, alpha, vessel=None):
    """tau = B(alpha) F(n) on the host, float64 - SupervisedTau.tau (SupervisedTau.py:42-83) with the hull's numbers, the statement of
    dpenv_thrust_map without the inflow thrust loss: n_pct, alpha [3, n] in env order (bow, port, star), F_i = K_i n_i |n_i| with K_i =
    kf_i ahead and kr_i astern; returns [3, n] = Fx, Fy, Mz."""
    from . import _lib
    v = np.asarray(_lib.default_vessel() if vessel is None else vessel, np.float64)
    P = _lib.P
    n_pct, alpha = np.asarray(n_pct, np.float64), np.asarray(alpha, np.float64)
    kf, kr = v[P['KF_BOW']:P['KF_BOW'] + 3, None], v[P['KR_BOW']:P['KR_BOW'] + 3, None]
    lx, ly = v[P['LX_BOW']:P['LX_BOW'] + 3, None], v[P['LY_BOW']:P['LY_BOW'] + 3, None]
    F = np.where(n_pct >= 0, kf, kr) * n_pct * np.abs(n_pct)
    c, s = np.cos(alpha), np.sin(alpha)
    return np.stack([(c * F).sum(0), (s * F).sum(0), ((lx * s - ly * c) * F).sum(0)])


def nn_allocator_dataset(rows, seed, vessel=None, angle_range=0.4 * np.pi, tau_min=0.01, tau_max=DP_TAU_MAX, in_dim=9, params=None):
    """A supervised dataset for the neural allocator by SupervisedTau.generateData's law (SupervisedTau.py:86-197): both stern pods at one
    angle a0 in [-angle_range, angle_range] (:104,153), the bow thruster at pi / 2 (:110), the three throttles in [-100, 100] % (:111);
    tau = thrust_map_host(u, a); rows with any |tau_j| < tau_min (:158) or any |tau_j| > tau_max_j (:181; (69, 30, 80), :37) are dropped;
    labels u / 100 and a / angle_scale (:185-186), inputs the lever-arm constants and tau * tau_scale (:189-193).
    The DRAW is build-defined: uniform draws from numpy.random.RandomState(seed), drawn in blocks until `rows` rows have passed the
    filters.  The reference walks a 37 x 21^3 grid whose throttle axis it perturbs with UNSEEDED draws (:114-124) and builds with
    np.linspace(.., np.floor(..)), which current NumPy refuses - its exact rows cannot be regenerated, its law can.
    Returns dict(x [rows, in_dim] float32, y [rows, 6] float32 = (u_port, u_star, u_bow, a_port, a_star, a_bow) scaled, and the draws
    behind them in float64: u [rows, 3] and a [rows, 3] in the NODE's order port, star, bow, tau [rows, 3] unscaled)."""
    p = nn_allocator_defaults() if params is None else params
    rng = np.random.RandomState(seed)
    tmax = np.asarray(tau_max, np.float64)
    us, as_, taus, have = [], [], [], 0
    while have < rows:
        m = max(2 * (rows - have), 256)
        a0 = rng.uniform(-angle_range, angle_range, size=m)
        u = rng.uniform(-100.0, 100.0, size=(m, 3))                      # port, star, bow
        a = np.stack([a0, a0, np.full(m, np.pi / 2)], 1)
        tau = thrust_map_host(u[:, [2, 0, 1]].T, a[:, [2, 0, 1]].T, vessel).T
        keep = (np.abs(tau) >= tau_min).all(1) & (np.abs(tau) <= tmax).all(1)
        us.append(u[keep]); as_.append(a[keep]); taus.append(tau[keep])
        have += int(keep.sum())
    u, a, tau = (np.concatenate(v)[:rows] for v in (us, as_, taus))
    xs = tau * np.asarray(p['tau_scale'], np.float64)
    x = xs if in_dim == 3 else np.concatenate([np.broadcast_to(np.asarray(p['in_const'], np.float64), (rows, 6)), xs], 1)
    y = np.concatenate([u / 100.0, a / float(p['angle_scale'])], 1)
    return dict(x=x.astype(np.float32), y=y.astype(np.float32), u=u, a=a, tau=tau)
