"""Edge tables of the single step (plain NumPy, no GPU): the inputs at which hand-written device math goes wrong, shared row for
row by tests/test_step_edges_cpu.py (float32 oracle against float64 oracle: are the rows fair?) and tests/test_gpu_step_edges.py
(the HIP kernels against the float64 oracle).  Every input is a float32 value; truth is the float64 oracle ON those float32 values.

A table is a `Table`: canonical state [15, n], counters [2, n], actions [n, A], the keyword arguments of tests.helpers.make_pair,
one tag per row, and per row the DISCONTINUOUS ARGUMENT if the row sits on a jump of the reference law (an odd integer of the
wrapped azimuth action, a zero sine head on the negative cosine axis, a heading or a yaw error at the wrap): such a row passes if it
agrees - in every quantity at once - with the truth at the input or at one of the two float32 neighbours of that argument.

Comparison: `ratios` = |a - b| / tolerance per row for the quantities of test_gpu_parity.compare with the floors of tests/tolerances.py
unchanged; `judge` applies the neighbour rule and returns the per-quantity worst ratios.
"""
import numpy as np

from tests import tolerances as TOL

F32 = np.float32
PI32 = F32(np.pi)
ALL_CASES = [('full', True), ('full', False), ('simple', False), ('limited', True), ('limited', False),
             ('final_wrap', True), ('final_wrap', False), ('final_cont', True), ('final_cont', False)]
ACT_DIM = {'full': 6, 'simple': 3, 'limited': 5, 'final_wrap': 5, 'final_cont': 7}
RAGGED = 4096 + 37
DISC_NONE, DISC_ACT, DISC_STATE = 0, 1, 2
DONE_TERMINAL, DONE_TIMELIMIT, DONE_FAULT = 1, 2, 4
FOLD = 30000.0                       # sincos_lean folds larger arguments by 2 pi in plain float32: a valid rotation, nothing more
# radians wrap mode: the float32 law subtracts k * float32(2 pi), whose relative error 2.8e-8 becomes |x| * 2.8e-8 rad in ANY float32
# evaluation of wrap(x) (the float32 oracle included).  From this |psi| on, the radians-mode heading rows therefore put the yaw setpoint next
# to the heading (the yaw error is small and never wrapped) - the wrap of a large yaw error is what the yaw-error rows at +-180 hold
RADIANS_NEAR_SETPOINT = 100.0
# ... and from this |psi| on (2.8e-8 |psi| is 1.4e-5 rad and growing to 8.4e-4 rad at 29999) they start at rest a millimetre from the setpoint, so that the turned
# position error stays well inside its floor
RADIANS_AT_REST = 500.0


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def default_angles(mode):
    """the reset default azimuths as the kernels form them (float32 arithmetic)"""
    if mode == 'full':
        return np.zeros(3, F32)
    if mode == 'simple':
        return np.array([PI32 * F32(0.5), F32(-3.0) * PI32 * F32(0.25), F32(3.0) * PI32 * F32(0.25)], F32)
    return np.array([PI32 * F32(0.5), 0.0, 0.0], F32)


def mid_action(mode):
    a = {'full': [0.25, 0.5, -0.375, 0.25, -0.125, 0.375], 'simple': [0.25, 0.5, -0.375],
         'limited': [0.25, 0.5, -0.375, -0.25, 0.375], 'final_wrap': [0.25, 0.5, -0.375, 0.625, -0.375],
         'final_cont': [0.25, 0.5, -0.375, 0.5, 0.75, -0.625, 0.25]}[mode]
    return np.array(a, F32)


def rest_state(mode):
    s = np.zeros(15, F32)
    s[12:15] = default_angles(mode)
    return s


def moving_state(mode):
    s = np.array([1.5, -2.25, 0.25, 0.5, -0.0625, 0.03125, 0.5, 0.25, 0.125, 10.0, -20.0, 30.0, 0.0, 0.25, -0.5], F32)
    s[12:15] = default_angles(mode)
    if mode != 'simple':
        s[13], s[14] = 0.25, -0.5
    return s


class Table(object):
    def __init__(self, mode, ext, kw):
        self.mode, self.ext, self.kw = mode, ext, dict(kw)
        self.rows = []

    def add(self, tag, state, action, disc=(DISC_NONE, 0)):
        self.rows.append((tag, np.array(state, F32), np.array(action, F32), disc))

    def finish(self):
        self.tag = np.array([r[0] for r in self.rows])
        self.st = np.ascontiguousarray(np.stack([r[1] for r in self.rows], 1))
        self.act = np.ascontiguousarray(np.stack([r[2] for r in self.rows], 0))
        self.disc = np.array([r[3] for r in self.rows], np.int64).reshape(-1, 2)
        self.ctr = np.zeros((2, self.st.shape[1]), np.int32)
        del self.rows
        return self

    @property
    def n(self):
        return self.st.shape[1]


def padded(t, mid_state, mid_act, total=RAGGED):
    """the table's rows spread evenly over `total` rows of copies of an ordinary row: the last workgroup is partial and holds an edge
    row (the last one), and every edge row sits between ordinary ones"""
    assert t.n < total // 2
    pos = np.round(np.linspace(1, total - 1, t.n)).astype(np.int64)
    assert len(set(pos.tolist())) == t.n
    out = Table(t.mode, t.ext, t.kw)
    out.tag = np.array(['pad'] * total, dtype=object)
    out.st = np.ascontiguousarray(np.tile(np.asarray(mid_state, F32)[:, None], (1, total)))
    out.act = np.ascontiguousarray(np.tile(np.asarray(mid_act, F32)[None, :], (total, 1)))
    out.disc = np.zeros((total, 2), np.int64)
    out.ctr = np.zeros((2, total), np.int32)
    out.tag[pos] = t.tag
    out.st[:, pos] = t.st
    out.act[pos] = t.act
    out.disc[pos] = t.disc
    out.tag = out.tag.astype(str)
    del out.rows
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A. action decode
# ------------------------------------------------------------------------------------------------------------------------------
COMPONENT_VALUES = [0.0, 1e-40, 1e-30, 0.5, float(np.nextafter(F32(1), F32(0))), 1.0, float(np.nextafter(F32(1), F32(2))), 3.0, 1e6]
HEAD_MAGNITUDES = [2.0 ** -60, 1e-3, 1.0, 1e3, 2.0 ** 60]
A_KW = dict(terminate=False, time_limit=False)


def head_directions(m):
    """16 directions with max(|s|, |c|) = m: the axes, the diagonals, and one ulp either side of |s| == |c|"""
    m = F32(m)
    lo = np.nextafter(m, F32(0))
    out = [(m, F32(0)), (F32(0), m), (-m, F32(0)), (F32(0), -m)]
    for ss in (1, -1):
        for sc in (1, -1):
            out += [(ss * m, sc * m), (ss * m, sc * lo), (ss * lo, sc * m)]
    return out


def table_a(mode, ext):
    t = Table(mode, ext, A_KW)
    A = ACT_DIM[mode]
    mid = mid_action(mode)
    states = [('rest', rest_state(mode)), ('moving', moving_state(mode))]
    for sname, st in states:
        for j in range(A):
            for v in COMPONENT_VALUES:
                for sg in (1.0, -1.0):
                    a = mid.copy()
                    a[j] = F32(sg) * F32(v)          # -0.0 for v = 0
                    # the wrapped azimuth action jumps at odd integers, and float32 forms (a + 1) / 2 with a rounding: the neighbours of an
                    # odd integer are on the jump as well
                    seam = mode == 'final_wrap' and j >= 3 and 0.9 < v < 3.5 and min(abs(v - 1.0), abs(v - 3.0)) < 1e-6
                    t.add('component_wrap_odd' if seam else 'component', st, a, (DISC_ACT, j) if seam else (DISC_NONE, 0))
        if mode == 'final_wrap':
            for j in (3, 4):
                for k in (1.0, 3.0, 2.0 ** 23 + 1.0):
                    for sg in (1.0, -1.0):
                        odd = F32(sg * k)
                        for v, tag in ((odd, 'wrap_odd'), (down(odd), 'wrap_odd_nbr'), (up(odd), 'wrap_odd_nbr')):
                            a = mid.copy()
                            a[j] = v
                            t.add(tag, st, a, (DISC_ACT, j))       # (the float32 law rounds a + 1: the neighbours sit on the jump too)
                for k in (1.0, 3.0):
                    for sg in (1.0, -1.0):
                        for half in (F32(sg * k + 0.5), F32(sg * k - 0.5)):
                            for v in (half, down(half), up(half)):
                                a = mid.copy()
                                a[j] = v
                                t.add('wrap_half', st, a)
        if mode == 'final_cont':
            for js in (3, 5):
                for m in HEAD_MAGNITUDES:
                    for s, c in head_directions(m):
                        a = mid.copy()
                        a[js], a[js + 1] = s, c
                        on_seam = (s == 0) and (c < 0)
                        t.add('heads_seam' if on_seam else 'heads', st, a, (DISC_ACT, js) if on_seam else (DISC_NONE, 0))
                for s in (0.0, -0.0):
                    for c in (0.0, -0.0):
                        a = mid.copy()
                        a[js], a[js + 1] = F32(s), F32(c)
                        t.add('heads_zero', st, a)
                    for c in (1.0, -1.0):
                        a = mid.copy()
                        a[js], a[js + 1] = F32(s), F32(c)
                        t.add('heads_seam' if c < 0 else 'heads_unit', st, a, (DISC_ACT, js) if c < 0 else (DISC_NONE, 0))
                for s in (1.0, -1.0):
                    for c in (0.0, -0.0):
                        a = mid.copy()
                        a[js], a[js + 1] = F32(s), F32(c)
                        t.add('heads_unit', st, a)
    return t.finish()


def table_a_out_of_range():
    """continuous-angle heads outside the supported magnitudes (include/dpenv.h: 2^-60 <= max(|s|, |c|) <= 2^60): finite outputs and
    no fault bit are all that is promised"""
    t = Table('final_cont', True, A_KW)
    mid = mid_action('final_cont')
    for st in (rest_state('final_cont'), moving_state('final_cont')):
        for js in (3, 5):
            for m in (2.0 ** -70, 2.0 ** 70):
                for s, c in head_directions(m):
                    a = mid.copy()
                    a[js], a[js + 1] = s, c
                    t.add('heads_out_of_range', st, a)
    return t.finish()


def zero_head_fact_rows():
    """the rows the fix rests on: full port thrust from rest with the port heads (0, +0), (0, -0), (-0, -0), (-0, +0), (1e-30, 0)"""
    t = Table('final_cont', True, A_KW)
    st = rest_state('final_cont')
    for s, c in ((0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (1e-30, 0.0)):
        t.add('fact', st, np.array([0.0, 1.0, 0.0, s, c, 0.0, 1.0], F32))
    return t.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# B. heading and wrap (final / continuous angles / extended state: the shipped shape)
# ------------------------------------------------------------------------------------------------------------------------------
def _psi_list():
    out = []
    for sg in (1.0, -1.0):
        p = F32(sg) * PI32
        out += [p, down(p), up(p)]
        out += [F32(sg * 179.9)]
        p = F32(sg * 180.0)
        out += [p, down(p), up(p)]
        out += [F32(sg * 181.0), F32(sg * 1000.0), F32(sg * 29999.0), F32(sg * 30001.0)]
    out += [F32(200.0), F32(539.9), F32(540.1), F32(3.5), F32(-7.0), F32(10.0), F32(-20.0)]
    return out


def table_b(wrap_mode):
    """general rows: every listed heading with nonzero N - N_ref, E - E_ref, yaw rate and thrust, as far as float32 can hold such a row
    (a centimetre-sized position error from |psi| = 16 on; from |psi| = 500 on, where one ulp of psi is no longer small against a sub-step's
    increment, no yaw rate, no yaw setpoint and a thrust without yaw moment; radians mode, whose wrap constant float32(2 pi) is inexact,
    needs more: RADIANS_NEAR_SETPOINT, RADIANS_AT_REST above).  Only |psi| > 30000 ('fold') is outside parity, in both modes;
    exact rows: v = r = 0 and equal stern thrusts straight ahead, so that the heading does not move AT ALL during the step and the wrap
    is evaluated at exactly the tabulated value - the heading, or the yaw error, on +-180 and +-pi and one ulp either side;
    yaw-error rows with the plant turning: the yaw error starts on +-180 / +-pi and the step itself carries it to either side"""
    mode = 'final_cont'
    t = Table(mode, True, dict(terminate=False, time_limit=False, wrap_mode=wrap_mode))
    mid = mid_action(mode)
    jump = F32(180.0) if wrap_mode == 'reference' else PI32
    sym = np.array([0.0, 0.5, 0.5, 0.0, 1.0, 0.0, 1.0], F32)       # bow idle, both stern thrusters 50 % straight ahead: no sway force, no yaw moment
    for psi in _psi_list():
        st = moving_state(mode)
        a = mid
        st[2] = psi
        ap = abs(float(psi))
        if ap >= 16.0:
            # one ulp of such a heading is 1.9e-6 rad (1.5e-5 rad at 180) and the plant adds twenty increments to it: any float32 evaluation
            # turns the position error by that much, so it is kept at centimetres (nonzero all the same) for the turn to stay well inside the floor
            st[0], st[1] = st[6] + F32(0.0625), st[7] - F32(0.03125)
        if ap >= 500.0:
            # one ulp of psi is no longer small against a sub-step's increment: no yaw rate and no yaw moment, the heading stays where it is
            st[4], st[5], st[8] = 0.0, 0.0, 0.0
            a = sym
        if wrap_mode == 'radians' and ap >= RADIANS_NEAR_SETPOINT:
            # a yaw error of 0.375 rad between headings whose ulp is 1.5e-5 rad and more: twenty rounded increments of psi would show in it,
            # so the heading is kept where it is (no sway, no yaw rate, a thrust without yaw moment)
            st[8] = psi - F32(0.375) * F32(np.sign(psi))                # exact in float32: 0.375 is a multiple of the ulp of every such heading
            assert float(psi) - float(st[8]) == 0.375 * np.sign(psi)
            st[4], st[5] = 0.0, 0.0
            a = sym
        if wrap_mode == 'radians' and ap >= RADIANS_AT_REST:
            st[0], st[1], st[3] = st[6] + F32(2.0 ** -10), st[7] - F32(2.0 ** -11), 0.0
            a = sym * np.array([1, 0.25, 0.25, 1, 1, 1, 1], F32)         # a sixteenth of the force: the hull stays within millimetres over three steps
        t.add('fold' if ap > FOLD else 'heading', st, a)
    for sg in (1.0, -1.0):
        for other in (F32(180.0), PI32):
            j = F32(sg) * other
            on_jump = other == jump
            # the heading itself on the jump, yaw setpoint 0
            for psi, d in ((j, True), (down(j), False), (up(j), False)):
                st = moving_state(mode)
                st[2], st[4], st[5], st[8] = psi, 0.0, 0.0, 0.0
                if abs(float(psi)) >= 179.0:
                    st[0], st[1] = st[6] + F32(0.0625), st[7] - F32(0.03125)     # (as above: one ulp of the heading turns it by 1.5e-5 rad)
                # (float32 forms psi + 180 with a rounding: the neighbours of the jump sit on it as well)
                flag = on_jump
                t.add(('heading_jump' if d else 'heading_jump_nbr') if flag else 'heading_exact', st, sym, (DISC_STATE, 2) if flag else (DISC_NONE, 0))
            # the yaw error psi - psi_ref on the jump: psi = +-1 or 0, psi_ref = psi - j (exact in float32)
            for psi in (F32(sg), F32(0.0)):
                ref = F32(psi - j)
                assert float(psi) - float(ref) == float(j)
                for r_, d in ((ref, True), (down(ref), False), (up(ref), False)):
                    st = moving_state(mode)
                    st[2], st[4], st[5], st[8] = psi, 0.0, 0.0, r_
                    flag = on_jump
                    t.add(('yaw_error_jump' if d else 'yaw_error_jump_nbr') if flag else 'yaw_error_exact', st, sym, (DISC_STATE, 8) if flag else (DISC_NONE, 0))
                # and with the plant turning: both sides of the jump are reached by the step itself
                for rate in (0.03125, -0.03125):
                    st = moving_state(mode)
                    st[2], st[5], st[8] = psi, rate, ref
                    t.add('yaw_error', st, mid)
    return t.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# C. termination bounds (plant held, psi = 0, setpoint 0: the observation IS the state)
# ------------------------------------------------------------------------------------------------------------------------------
def bounds32(mode):
    """the termination bounds as float32 arithmetic forms them"""
    b = [F32(8.0), F32(8.0), PI32 * F32(0.5), F32(1.4), F32(0.30), F32(0.52)]
    if mode == 'simple':
        b[3], b[5] = F32(1.75), F32(0.51)
    if mode in ('limited', 'final_wrap', 'final_cont'):
        b[2] = F32(45.0) * PI32 / F32(180.0)
    return b


def table_c(mode, ext):
    t = Table(mode, ext, dict(terminate=True, time_limit=False, hold_plant=True))
    mid = mid_action(mode)
    base = moving_state(mode)
    base[0:9] = [1.0, -2.0, 0.0, 0.5, 0.125, -0.25, 0.0, 0.0, 0.0]
    t.add('inside', base, mid)
    for k, b in enumerate(bounds32(mode)):
        for sg in (1.0, -1.0):
            for v, tag in ((b, 'at_bound'), (up(b), 'above_bound'), (down(b), 'below_bound')):
                st = base.copy()
                if k == 2:
                    st[0], st[1] = 0.0, 0.0            # a heading other than 0 rotates the position error: none to rotate
                st[k] = F32(sg) * v
                t.add(tag, st, mid)
    return t.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# D. force map
# ------------------------------------------------------------------------------------------------------------------------------
def table_d():
    """(n_pct [3, n], alpha [3, n], thruster index [n]): one thruster at a time at +-100 %, the two others idle at azimuth 0"""
    al = []
    for sg in (1.0, -1.0):
        al += [F32(sg * 0.0), F32(sg * 1e-40), F32(sg * 29999.9), F32(sg * 30000.1), F32(sg * 1e5), F32(sg * 1e8)]
        for k in list(range(0, 9)) + [19098]:
            x = F32(sg * (k * (np.pi / 2)))
            al += [x, down(x), up(x)]
    al = np.array(al, F32)
    n_pct, alpha, which = [], [], []
    for i in range(3):
        for pct in (100.0, -100.0):
            for a in al:
                n = np.zeros(3, F32)
                x = np.zeros(3, F32)
                n[i], x[i] = pct, a
                n_pct.append(n); alpha.append(x); which.append(i)
    return np.ascontiguousarray(np.stack(n_pct, 1)), np.ascontiguousarray(np.stack(alpha, 1)), np.array(which)


# ------------------------------------------------------------------------------------------------------------------------------
# non-finite rows
# ------------------------------------------------------------------------------------------------------------------------------
def poisoned(mode, ext, n=256 + 37):
    """(clean table of n ordinary rows, poisoned copy, indices of the poisoned rows): NaN, +Inf and -Inf in each action component and in
    each of the six pose / velocity components, one row each, three rows apart"""
    clean = Table(mode, ext, dict(terminate=True, time_limit=False))
    st, a = moving_state(mode), mid_action(mode)
    for _ in range(n):
        clean.add('pad', st, a)
    clean.finish()
    bad = Table(mode, ext, clean.kw)
    bad.tag, bad.st, bad.act, bad.disc, bad.ctr = clean.tag.copy(), clean.st.copy(), clean.act.copy(), clean.disc.copy(), clean.ctr.copy()
    del bad.rows
    idx = []
    i = 2
    for v in (np.nan, np.inf, -np.inf):
        for j in range(ACT_DIM[mode]):
            bad.act[i, j] = v
            idx.append(i); i += 3
        for k in range(6):
            bad.st[k, i] = v
            idx.append(i); i += 3
    assert i < n + 3
    return clean, bad, np.array(idx)


# ------------------------------------------------------------------------------------------------------------------------------
# truth and comparison
# ------------------------------------------------------------------------------------------------------------------------------
def make_oracle(mode, ext, dtype, kw, n_substeps=20):
    """the oracle of tests.helpers.make_pair's configuration, without the GPU half"""
    from oracle import oracle as O
    var, cont = O.MODES[mode]
    cfg = O.make_config(variant=var, extended_state=int(ext), cont_ang=cont, n_substeps=n_substeps,
                        wrap_mode=O.WRAP_RADIANS if kw.get('wrap_mode') == 'radians' else O.WRAP_REFERENCE,
                        terminate=int(kw.get('terminate', True)), max_ep_len=0 if not kw.get('time_limit', True) else int(8000 / n_substeps))
    return O.Oracle(cfg, dtype)


def oracle_steps(orc, t, steps=1, st=None, act=None):
    """`steps` oracle steps from the table's rows (or from st / act given instead); a list of dicts like test_gpu_parity.step_both's"""
    st = (t.st if st is None else st).astype(orc.dtype).copy()
    act = t.act if act is None else act
    ctr = t.ctr.copy()
    out = []
    for _ in range(steps):
        hold = np.ascontiguousarray(st[0:6]) if t.kw.get('hold_plant') else None
        with np.errstate(all='ignore'):
            r = orc.step(st, ctr, act.astype(orc.dtype), plant_override=hold, want_parts=True)
        out.append(dict(obs=r[0].copy(), rew=r[1].copy(), done=r[2].copy(), parts=r[3].copy(), st=st.copy(), ctr=ctr.copy()))
    return out


def variant_inputs(t, direction):
    """the table with the discontinuous argument of every flagged row moved to its float32 neighbour below (-1) or above (+1)"""
    st, act = t.st.copy(), t.act.copy()
    step = down if direction < 0 else up
    for i in np.nonzero(t.disc[:, 0] == DISC_ACT)[0]:
        act[i, t.disc[i, 1]] = step(act[i, t.disc[i, 1]])
    for i in np.nonzero(t.disc[:, 0] == DISC_STATE)[0]:
        st[t.disc[i, 1], i] = step(st[t.disc[i, 1], i])
    return st, act


def truth_variants(orc, t, steps=1):
    """[truth at the input, at the neighbour below, at the neighbour above]; the two others differ from the first in flagged rows only"""
    out = [oracle_steps(orc, t, steps)]
    if (t.disc[:, 0] != DISC_NONE).any():
        for d in (-1, 1):
            st, act = variant_inputs(t, d)
            out.append(oracle_steps(orc, t, steps, st=st, act=act))
    return out


def _rel(a, b, floor, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    tol = TOL.RTOL_F32 * np.maximum(np.abs(b), floor) * scale
    with np.errstate(all='ignore'):
        r = np.abs(a - b) / tol
    r[~np.isfinite(r)] = np.inf
    return r.max(1)


def ratios(g, o, od, scale=1.0, state=True):
    """per-row |g - o| / tolerance for the quantities of test_gpu_parity.compare (floors of tests/tolerances.py); g without 'parts' (the
    lean and fixed kernels do not write them) or without 'st' (rows of a fused launch) skips those"""
    R = {}
    names = ('x', 'y', 'psi', 'u', 'v', 'r', 'n_bow', 'n_port', 'n_star')
    for k in range(od):
        R['obs.' + names[k]] = _rel(g['obs'][:, k], o['obs'][:, k], TOL.OBS_FLOOR[k], scale)
    R['reward'] = _rel(g['rew'], o['rew'], TOL.REWARD_FLOOR, scale)
    if 'parts' in g:
        R['reward parts'] = _rel(g['parts'], o['parts'], TOL.PARTS_FLOOR, scale)
    if state and 'st' in g:
        R['eta'] = _rel(g['st'][0:3].T, o['st'][0:3].T, TOL.ETA_FLOOR, scale)
        R['nu'] = _rel(g['st'][3:6].T, o['st'][3:6].T, TOL.NU_FLOOR, scale)
        R['ref'] = _rel(g['st'][6:9].T, o['st'][6:9].T, TOL.ETA_FLOOR, scale)
        R['thrust cmd'] = _rel(g['st'][9:12].T, o['st'][9:12].T, TOL.THRUST_FLOOR, scale)
        R['azimuth cmd'] = _rel(g['st'][12:15].T, o['st'][12:15].T, TOL.ANGLE_FLOOR, scale)
        R['counters'] = np.where((g['ctr'] == o['ctr']).all(0), 0.0, np.inf)
    R['done'] = np.where(np.asarray(g['done']) == np.asarray(o['done']), 0.0, np.inf)
    return R


def judge(g_steps, variants, t, od, rows, limit=1.0):
    """g_steps: one dict per step; variants: truth_variants(...).  For each row of `rows` (a boolean mask) the best variant is the one
    whose worst ratio over all quantities AND all steps is smallest - a row takes ONE side with everything it has; unflagged rows only
    have the truth at the input.  Every step of a multi-step run is held to the single-step tolerance.  Returns ({quantity: worst ratio over rows}, the failing row indices)."""
    per_variant = []
    for v in variants:
        R = {}
        for k, (g, o) in enumerate(zip(g_steps, v)):
            last = k == len(g_steps) - 1
            for q, r in ratios(g, o, od, state=last).items():
                R[q] = np.maximum(R[q], r) if q in R else r
        per_variant.append(R)
    quantities = sorted(per_variant[0])
    worst = np.stack([np.max(np.stack([R[q] for q in quantities]), 0) for R in per_variant])          # [variant, row]
    flagged = t.disc[:, 0] != DISC_NONE
    if len(variants) > 1:
        worst[1:, ~flagged] = np.inf
    pick = np.argmin(worst, 0)
    report = {}
    for q in quantities:
        chosen = np.stack([R[q] for R in per_variant])[pick, np.arange(t.n)]
        report[q] = float(chosen[rows].max()) if rows.any() else 0.0
    best = worst[pick, np.arange(t.n)]
    return report, np.nonzero(rows & ~(best <= limit))[0]


def parity_rows(t):
    """rows held to parity: everything but the 'fold' rows (|psi| > 30000, where sincos_lean promises a valid rotation and no more)"""
    return t.tag != 'fold'


def describe(t, i):
    return 'row %d tag %s state %r action %r' % (i, t.tag[i], t.st[:, i].tolist(), t.act[i].tolist())


def record(path, title, report):
    """append one comparison's per-quantity worst ratios to a text record (path None: no record is kept)"""
    if not path:
        return
    with open(path, 'a') as f:
        f.write('%-58s %s\n' % (title, '  '.join('%s %.3f' % (q, r) for q, r in sorted(report.items()) if r > 0)))
