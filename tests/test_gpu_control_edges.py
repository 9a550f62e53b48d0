"""The classical baseline at the edges of its numbers (-m gpu): the tables of tests/control_edges.py through dpenv_thrust_alloc,
dpenv_controller_label (scalar numbers and a per-env table, f32 and bf16 rows) and one dpenv_controller_rollout, the device's outputs
handed to the judges tests/test_control_edges_cpu.py proves fair on the float32 host law: the float64 law within derived bounds wherever
it makes a claim, the float32 host statement bit for bit (any NaN equal to any NaN) elsewhere - outside the allocation's domain, and on
a non-finite observation row and the rows behind it.  Then the packing kernel's refusals and its G (C), integ_update in the fused launch
against the eager path at the edges of its state, counts and parameters (D), and reff_target / reff_advance on the filter's edge rows
(E).  Every non-finite value here is an input include/dpenv.h defines an answer for.
n = 193 or 65, T <= 8.  Every figure is printed, and appended to the file CONTROL_EDGES_RECORD names, if it is set."""
import os

import numpy as np
import pytest
import torch            # before anything loads libdpenv.so, as in every other GPU test module

from tests import control_edges as CE
from tests import helpers as H

pytestmark = pytest.mark.gpu
RECORD = os.environ.get('CONTROL_EDGES_RECORD', '')
F32, F64 = np.float32, np.float64
F_EPS = (1e-6, 0.0)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return H.to_dev(np.ascontiguousarray(a))


@pytest.fixture(scope='module')
def env():
    """One handle of 193 envs with the controller on; the labelling calls read its numbers and leave its state alone."""
    from tests.test_gpu_dp_controller_table import _env, _start
    e = _env(CE.N, auto_reset=True, terminate=False, max_ep_len=400)
    _start(e)
    assert F32(e.control_period) == CE.DT
    return e


def _label(env, case, bf16=False):
    from ml4ca_amd.policy import controller_label
    env.set_dp_controller_table(_dev(case['table']), check=True)
    obs = _dev(case['obs'])
    act, z = controller_label(env, obs.to(torch.bfloat16) if bf16 else obs, _dev(case['done']), z=_dev(case['z0']))
    torch.cuda.synchronize()
    return _np(act), _np(z)


# A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f_eps', F_EPS)
def test_allocation_through_thrust_alloc(f_eps):
    from ml4ca_amd.env import thrust_alloc
    tau, kink, names = CE.alloc_cases(f_eps)
    p = CE.params(f_eps)
    got = _np(thrust_alloc(_dev(tau.T), p))
    res = CE.judge_alloc(f_eps, got)
    CE.report(RECORD, 'A dpenv_thrust_alloc, f_eps %g' % f_eps, res)
    assert res['ok'].all(), [names[i] for i in np.flatnonzero(~res['ok'])]
    assert np.array_equal(res['used_kink'], kink)
    rows, ratio = CE.judge_decode(p, tau, CE.alloc_truth(p, tau), got, kink)
    CE.record(RECORD, 'A decode on the device, f_eps %g: %d rows, worst error / bound %s' % (f_eps, rows.sum(), ratio.max(0)))
    assert (ratio <= 1).all(), [names[i] for i in np.flatnonzero((ratio > 1).any(1))]
    # the statement both follow, bit for bit on every row: the kernel and the float32 host law are one text
    assert CE.bits_equal(got, CE.host_alloc(p, tau)).all()


@pytest.mark.parametrize('f_eps', F_EPS)
def test_allocation_through_controller_label(env, f_eps):
    """Gains that make the wrench the chosen value (control_edges.alloc_label_case); tau_max = +inf is a bound the library accepts."""
    case = CE.alloc_label_case(f_eps)
    names = case['rows']
    act, z = _label(env, case)
    res = CE.judge_pid(case, act, z)
    CE.record(RECORD, 'A dpenv_controller_label, f_eps %g: %d rows with a float64 claim, %d without, %d kink rows; worst error / bound %s' % (
        f_eps, res['domain'].sum(), (~res['domain']).sum(), res['used_kink'].sum(), res['ratio'].max((0, 1))))
    bad = np.flatnonzero(~res['ok'].reshape(-1))
    assert not len(bad), [names[i] if i < len(names) else i for i in bad]
    assert res['z_ok'].all() and res['demoted'] == 0


# B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_pid_lines_through_controller_label(env, bf16):
    from ml4ca_amd.deploy import label_rows
    case = CE.pid_cases(bf16)
    act, z = _label(env, case, bf16)
    res = CE.judge_pid(case, act, z)
    CE.record(RECORD, 'B dpenv_controller_label %s: %d rows with a float64 claim, %d without; worst error / bound %s, z %.3g' % (
        'bf16' if bf16 else 'f32', res['domain'].sum(), (~res['domain']).sum(), res['ratio'].max((0, 1)), res['z_ratio'].max()))
    assert res['ok'].all() and res['z_ok'].all(), [case['names'].get(i, i) for i in np.flatnonzero(~res['ok'].all(0) | ~res['z_ok'])]
    assert res['demoted'] == 0
    # label_rows on the block - NaN, +inf and -inf rows and the rows behind them included - is the device's, bit for bit, z_out too
    with np.errstate(all='ignore'):
        want, wz = label_rows(case['table'], case['obs'], case['done'], case['z0'], dt=env.control_period)
    # (z_bound_j = 0: fminf(fmaxf(v, -0.0f), 0.0f) is a zero whose sign neither C nor NumPy's fmin / fmax defines - include/dpenv.h says
    # so - and on those lanes alone z_j is held in value)
    free_zero = (case['table'][9:12] == 0) & (z == 0) & (wz == 0)
    assert CE.bits_equal(act, want).all() and (CE.bits_equal(z, wz) | free_zero).all(), np.argwhere(~(CE.bits_equal(z, wz) | free_zero))
    CE.record(RECORD, 'B z_bound = 0 lanes: sign bit of z on the device %s, on the host %s' % (
        np.signbit(z[case['table'][9:12] == 0]).astype(int).tolist(), np.signbit(wz[case['table'][9:12] == 0]).astype(int).tolist()))
    assert np.isfinite(act).all() and np.isfinite(z).all()                             # every clip drops a NaN: nothing non-finite is flown
    # the neighbours of every case lane are what they are without the cases
    plain = dict(case)
    plain['obs'], plain['done'], plain['z0'] = case['obs'].copy(), case['done'].copy(), case['z0'].copy()
    for i in case['names']:
        plain['obs'][:, i], plain['done'][:, i], plain['z0'][:, i] = case['obs'][:, 0], case['done'][:, 0], case['z0'][:, 0]
    pa, pz = _label(env, plain, bf16)
    nb = list(CE.NEIGHBOURS)
    assert CE.bits_equal(act[:, nb], pa[:, nb]).all() and CE.bits_equal(z[:, nb], pz[:, nb]).all()
    assert not CE.bits_equal(act, pa).all()


# C (the refusal conditions of the packing kernel, each alone at its boundary) ------------------------------------------------------------
def test_packing_refuses_at_the_boundaries_and_a_refused_row_rests(env):
    """Through dpenv_set_dp_controller_table with a refused mask, on table B's block: a weight or a kf of 0 or -0.0 is refused; a kf of
    the smallest subnormal, f_eps = -0.0 and tau_max = +inf are kept; ONE weight of the smallest subnormal beside unit weights is refused by
    `det != 0`, not by `> 0` (M is of rank one to working precision and adj and det cancel to exactly 0; all five weights subnormal is a
    kept row: test_packed_G_is_the_recipes_f32_rounding); a refused row flies [0, 0, 0, 0, 1, 0, 1] in value on every
    row, the NaN, +inf and -inf observations of table B included, and no other lane changes."""
    from ml4ca_amd.deploy import CTRL_SLOTS
    from ml4ca_amd.policy import controller_label
    case = CE.pid_cases()
    base_act, base_z = _label(env, case)
    table = case['table'].copy()
    nonfinite = [i for i, s in sorted(case['names'].items()) if 'in o[' in s]
    plain = [i for i, s in sorted(case['names'].items()) if 'at' in s and 'z_bound, error' in s]
    sub = F32(CE.SUB)
    w0, kf1, fe, tm = CTRL_SLOTS['weight'][0], CTRL_SLOTS['kf'][0] + 1, CTRL_SLOTS['f_eps'][0], CTRL_SLOTS['tau_max'][0]
    edits = [(w0 + 2, F32(0.0), True), (w0 + 2, F32(-0.0), True), (kf1, F32(0.0), True), (kf1, F32(-0.0), True), (w0, F32(0.0), True),
             (w0 + 4, F32(-0.0), True)] * 3
    want = np.zeros(CE.N, bool)
    for i, (slot, v, refused) in zip(nonfinite, edits):
        table[slot, i], want[i] = v, refused
    kept = [(kf1, sub), (fe, F32(-0.0)), (tm + 1, F32(np.inf))]
    for i, (slot, v) in zip(plain, kept):
        table[slot, i] = v
    assert want.sum() == 18
    # one weight of the smallest subnormal beside unit weights passes `> 0`, and the row is refused all the same: 1 / w = 7e44 swamps the
    # other columns, M is of rank one to working precision, adj and det cancel to exactly 0 (nothing overflows) and G is x / 0 - the
    # condition of the 'det is 0' row, as the host statement of the recipe says too
    from ml4ca_amd.deploy import dp_controller_table_params
    i = plain[len(kept)]
    table[w0 + 2, i] = sub
    with np.errstate(all='ignore'):
        G32 = dp_controller_table_params(table)['G'].astype(F32)
    assert not np.isfinite(G32[i]).all() and np.isfinite(G32[plain[:len(kept)]]).all()
    want[i] = True
    mask = torch.full((CE.N,), 9, dtype=torch.uint8, device=env.device)
    _lib_check(env, _dev(table), mask)
    act, z = controller_label(env, _dev(case['obs']), _dev(case['done']), z=_dev(case['z0']))
    torch.cuda.synchronize()
    act, z, mask = _np(act), _np(z), _np(mask)
    assert np.array_equal(mask, want.astype(np.uint8)), (np.flatnonzero(mask != want), [case['names'][i] for i in np.flatnonzero(mask != want)])
    assert (act[:, want] == F32([0, 0, 0, 0, 1, 0, 1])).all() and (z[:, want] == 0).all()
    same = np.ones(CE.N, bool)
    same[want] = False
    same[plain[:len(kept)]] = False
    assert CE.bits_equal(act[:, same], base_act[:, same]).all() and CE.bits_equal(z[:, same], base_z[:, same]).all()
    assert np.isfinite(act).all()
    env.set_dp_controller_table(None)


def _lib_check(env, table, mask):
    """dpenv_set_dp_controller_table with a refused mask and no read-back (env.set_dp_controller_table(check=False) passes no mask)."""
    from ml4ca_amd import _lib
    _lib.check(env.lib.dpenv_set_dp_controller_table(env._h, env._ptr(table), env._ptr(mask), env._stream()), env._h)
    env.dp_controller_table = table


def test_pid_lines_through_one_rollout():
    """T = 4 closed-loop steps from a state put back with set_state and z set to +-z_bound lane by lane: the launch's own act rows
    against the float64 scan of its own obs rows."""
    from ml4ca_amd.deploy import dp_controller_table
    from ml4ca_amd.policy import controller_rollout
    from tests.test_gpu_dp_controller_table import _env, _start
    n = 65
    e = _env(n, auto_reset=True, terminate=False, max_ep_len=400)
    p = CE.params()
    table = dp_controller_table(n, p)
    _start(e, _dev(table))
    st, ctr = e.get_state()
    e.set_state(st.clone(), ctr.clone())
    z0 = np.zeros((3, n), F32)
    z0[:, 0::3] = F32(p['z_bound'])[:, None]
    z0[:, 1::3] = -F32(p['z_bound'])[:, None]
    e.set_dp_controller_state(_dev(z0))
    out = controller_rollout(e, 4)
    torch.cuda.synchronize()
    case = dict(obs=_np(out['obs'].float()), done=_np(out['done']), z0=z0, table=table, names={})
    res = CE.judge_pid(case, _np(out['act']), _np(e.get_dp_controller_state()))
    CE.record(RECORD, 'B dpenv_controller_rollout T = 4: %d rows with a float64 claim; worst error / bound %s, z %.3g' % (
        res['domain'].sum(), res['ratio'].max((0, 1)), res['z_ratio'].max()))
    assert np.isfinite(case['obs']).all() and res['ok'].all() and res['z_ok'].all() and res['domain'].sum() >= 4 * n - 8
    tr = CE.pid_truth(case)
    assert (np.abs(tr['z']) == p['z_bound'][:, None]).any()                            # an error pushing outwards left z on its bound


def test_nn_scan_rows_behind_a_nan_row_are_the_host_statements():
    """dpenv_controller_label_nn: tau_j = NaN on the NaN row, z_i stays the law's, and the rows BEHIND it in the same episode - tau, the
    network's outputs, the thrust columns and z_out - are deploy.label_rows_nn's bit for bit: that comparison is made, on every row of
    the block, inside tests.test_gpu_controller_label_nn._identity_b; the asserts here only show the rows are the ones meant."""
    from tests.test_gpu_controller_label_nn import SHAPES_A, _dev_net, _env, _identity_b, _rows, _start
    n, Tn = 65, 5
    e = _start(_env(n), nn=False)
    net = _dev_net(e, SHAPES_A[0])
    obs, done, z0 = _rows(n, Tn, seed=9)
    obs, done = obs.clone(), done.clone()
    for lane, col in ((64, 1), (5, 3), (33, 2)):
        obs[1, lane, col] = float('nan')
        done[:, lane] = 0                                                              # one episode: rows 2 .. 4 are behind the NaN row
    act, z, raw, tau = _identity_b(e, obs, done, z0, net)
    assert bool(torch.isnan(tau[1, 64, 1])) and bool(torch.isnan(tau[1, 5, 0])) and bool(torch.isnan(tau[1, 33, 2]))
    assert bool(torch.isfinite(tau[2:]).all()) and bool(torch.isfinite(z).all())


# D (integ_update in the fused launch: T = 8, n = 193, f32, one wave, against the eager path of tests/test_gpu_integral_action.py) -------------
IA_T = 8
IA_BASE = dict(gain=(0.05, 0.05, 0.05), bound=(0.02, 0.03, 0.004), box=(5.0, 5.0, 2.5), dwell_s=0.5)     # D = 3


def _dt64(env):
    return float(F64(F32(env.cfg.substep_dt)) * env.cfg.n_substeps)


def _ia_states(n, D, bound):
    """(I0 [3, n] float32, c0 [n] int32): I at +-bound, half of it and 0 lane by lane; counts 0, 1, D - 1, D, D + 1 and, outside [0, D],
    -3, 1000 and INT32_MAX - 1 (include/dpenv.h says what those do)."""
    I0 = np.zeros((3, n), F32)
    pattern = (1.0, -1.0, 0.0, 0.5, -0.5)
    for j in range(3):
        I0[j] = [pattern[(i + j) % len(pattern)] for i in range(n)]
        I0[j] *= F32(bound[j])
    counts = (0, 1, D - 1, D, D + 1, -3, 1000, 2 ** 31 - 2)
    c0 = np.array([counts[(i // 5) % len(counts)] for i in range(n)], np.int32)
    return I0, c0


def _ia_flight(ia, seed=3, watch=None):
    """One fused launch against the eager replay, bit for bit in every row and in the state left; the envs start at zero heading on a
    reference at the origin with heading 0.3, so e_0, e_1 are the position offsets exactly and e_2 is about -0.3.  Returns (rows, I, c at the end, D, the pose errors every update saw)."""
    from ml4ca_amd.policy import policy_rollout
    from tests import test_gpu_integral_action as TI
    n = CE.N
    envA, envB = TI._make('final_cont', n, 'f32', 'one_wave', seed=seed)
    envA.set_integral_action(**ia)
    g = torch.Generator(device='cpu').manual_seed(seed)
    init = torch.zeros((6, n))
    init[0:2] = (torch.rand((2, n), generator=g) * 1.5 + 0.5) * torch.where(torch.rand((2, n), generator=g) < 0.5, -1.0, 1.0)
    init = init.to(envA.device)
    ref0 = torch.zeros((3, n), device=envA.device)
    ref0[2] = 0.3                                                                      # a reference heading: e_2 is about -0.3, not 0
    obs0 = [e.reset(init=init, new_ref=ref0).clone() for e in (envA, envB)][-1]
    assert bool((obs0[:, 2].abs() > 0.25).all())
    law = TI._law(envA)
    I0, c0 = _ia_states(n, law.dwell, ia['bound'])
    envA.set_integral_state(_dev(I0), _dev(c0))
    law.I, law.count = _dev(I0.T).clone(), _dev(c0).clone()
    seen, update = [], law.update
    law.update = lambda pre: (seen.append(pre[:, :3].clone()), update(pre))[1]
    a = policy_rollout(envA, IA_T, sample=False)
    b = TI.replay(envB, law, IA_T, obs0=obs0)
    TI._assert_rows(a, b, IA_T, envB)
    I, c = envA.get_integral_state()
    assert torch.equal(I.T, law.I) and torch.equal(c, law.count)
    assert not bool((a['done'] != 0).any())
    return a, _np(I), _np(c), law.dwell, [_np(s) for s in seen], c0


def test_integral_action_states_and_counts_at_the_edges():
    """I at +-bound with e pushing either way, counts D - 1, D, D + 1 and outside [0, D] handed in: the launch is the eager path's, and
    the out-of-range counts do what include/dpenv.h says - a negative count waits that much longer, one above D acts as D."""
    a, I, c, D, seen, c0 = _ia_flight(IA_BASE)
    assert D == 3
    integ = _np(a['integ'])
    bound = F32(IA_BASE['bound'])
    assert (np.abs(integ) == bound).any() and (integ[0] != integ[-1]).any()
    assert (c[c0 >= D - 1] == D).all() and (c[c0 == 2 ** 31 - 2] == D).all() and (c[c0 == -3] == min(-3 + IA_T, D)).all()
    late = c0 == -3                                                                    # c reaches D at the 6th update: I holds until then
    assert (integ[1:6, late] == integ[0, late]).all() and (integ[6, late] != integ[0, late]).any()
    CE.record(RECORD, 'D integ_update: %d lanes x %d rows equal the eager path; counts handed in %s end at %s' % (
        CE.N, IA_T, sorted(set(c0.tolist())), [int(c[c0 == v][0]) for v in sorted(set(c0.tolist()))]))


@pytest.mark.parametrize('what', ['box0', 'box0_heading', 'bound0', 'dwell0'])
def test_integral_action_parameters_at_the_edges(what):
    ia = dict(IA_BASE)
    if what == 'box0':
        ia['box'] = (0.0, 0.0, 0.0)
    elif what == 'box0_heading':                                                       # only the third term of `outside` can trip
        ia['box'] = (5.0, 5.0, 0.0)
    elif what == 'bound0':
        ia['bound'] = (0.0, 0.0, 0.0)
    elif what == 'dwell0':
        ia['dwell_s'] = 0.0
    a, I, c, D, seen, c0 = _ia_flight(ia)
    if what.startswith('box0'):                                                        # every error is outside: I and c are 0 from the first update on
        assert (I == 0).all() and (c == 0).all() and (_np(a['integ'])[1:] == 0).all()
    if what == 'bound0':
        assert (_np(a['integ']) == 0).all()
    if what == 'dwell0':
        assert D == 1 and (c[c0 >= 0] == 1).all()


@pytest.mark.parametrize('side', ['below', 'at_or_above'])
def test_dwell_boundary_in_float64(side):
    """dwell_s the f32 values about 3 dt64 (dt64 = (double)f32(substep_dt) n_substeps): just below it D = 3, at or above it D = 4."""
    probe_dt = float(F64(F32(0.01)) * 20)
    x = F32(3 * probe_dt)
    below = x if float(x) < 3 * probe_dt else np.nextafter(x, F32(0))
    above = np.nextafter(below, F32(np.inf))
    assert float(below) < 3 * probe_dt <= float(above)
    ia = dict(IA_BASE, dwell_s=float(below if side == 'below' else above))
    a, I, c, D, seen, c0 = _ia_flight(ia)
    assert D == (3 if side == 'below' else 4)
    assert (c[c0 == 0] == D).all() or IA_T < D
    first = _np(a['integ'])
    fresh = (c0 == 0)
    assert (first[1:D, fresh] == first[0, fresh]).all() and (first[D, fresh] != first[0, fresh]).any()


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_error_exactly_at_the_box_and_one_ulp_beyond(axis):
    """The box set to the |e_j| one lane's first update sees (read from a first flight with a wide box - the flights are identical up to
    that update): that lane is inside (strict >), I integrates; with the box one f32 smaller it is outside, I = 0 and c = 0."""
    a, I, c, D, seen, c0 = _ia_flight(IA_BASE)
    lane = int(np.flatnonzero(c0 == D)[0])
    e = np.abs(seen[0][lane, axis])
    for box_j, inside in ((e, True), (np.nextafter(e, F32(0)), False)):
        box = list(IA_BASE['box'])
        box[axis] = float(box_j)
        a2, I2, c2, D2, seen2, _ = _ia_flight(dict(IA_BASE, box=tuple(box)))
        assert np.array_equal(seen2[0].view(np.uint32), seen[0].view(np.uint32))
        integ = _np(a2['integ'])
        if inside:
            assert (integ[1, lane] != 0).any() and np.array_equal(integ[1, lane], _np(a['integ'])[1, lane])
        else:
            assert (integ[1, lane] == 0).all()


# E (reff_target and reff_advance in the fused launch) --------------------------------------------------------------------------------------
def test_reference_filter_switch_and_advance_through_one_launch():
    """The filter's state handed in (dpenv_set_reference_filter_state), one closed-loop step with a switch on it, the state read back:
    bit for bit deploy.BatchedReferenceFilter's switch + advance in f32, and inside the float64 bounds of control_edges.judge_reff - the
    ties at +-pi_f and +-3 pi_f go to even, a heading of 1e4 rad takes the short way.  The host-only lanes (a state of 1e30) are flown at
    rest on 0 instead."""
    from ml4ca_amd.policy import policy_rollout
    from tests import test_gpu_reference_filter as TR
    case = CE.reff_cases()
    n = CE.N
    flown = {k: case[k].copy() for k in ('x', 'r', 'target')}
    host_only = ~case['device']
    flown['x'][:, :, host_only], flown['r'][:, host_only], flown['target'][:, host_only] = 0.0, 0.0, 0.0
    flown['names'] = case['names']
    envA, _ = TR._make('final_cont', n, 'f32', 'one_wave', terminate=False)
    envA.set_reference_filter()
    assert F32(envA.control_period) == CE.DT
    envA.reset(init=torch.zeros((6, n), device=envA.device), new_ref=torch.zeros((3, n), device=envA.device))
    envA.set_reference_filter_state(_dev(flown['x'].reshape(9, n)), _dev(flown['r']))
    out = policy_rollout(envA, 1, sample=False, switch_steps=(0,), refs=_dev(flown['target'][None]))
    torch.cuda.synchronize()
    assert not bool((out['done'] != 0).any())
    x, r = envA.get_reference_filter_state()
    x, r = _np(x).reshape(3, 3, n), _np(r)
    hx, hr = CE.reff_host(flown)
    assert CE.bits_equal(x, hx).all() and CE.bits_equal(r, hr).all(), [case['names'].get(i, i) for i in np.flatnonzero(~CE.bits_equal(r, hr).all(0))]
    ok, rr, xr, k = CE.judge_reff(flown, x, r)
    CE.record(RECORD, 'E filter on the device: %d lanes, worst error / bound r %.3g, x %.3g' % (n, rr, xr))
    assert ok.all(), [case['names'].get(i, i) for i in np.flatnonzero(~ok)]
    by = {s: int(k[i]) for i, s in case['names'].items()}
    assert by['heading difference %r' % CE.PI32] == 0 and by['heading difference %r' % (F32(3) * CE.PI32)] == 2
    assert by['heading difference %r' % (F32(-3) * CE.PI32)] == -2 and by['unwrapped heading 1e4, target 0.3'] == -1592


# C, the arithmetic of pack_controllers_kernel ------------------------------------------------------------------------------------------------
def test_packed_G_is_the_recipes_f32_rounding(env):
    """Lever arms and weights of control_edges.pack_cases through dpenv_set_dp_controller_table: the refused mask is the recipe's (det
    exactly 0, by construction or by cancellation, a G that rounds to inf in f32); on the kept rows - a cond of 1e12 and all five weights at the
    smallest subnormal (the boundary of `> 0`: a weight flushed to 0 there would refuse the row) among them - G is read back
    through the law with wrenches along the axes and the actions are the float32 host law's on the recipe's G rounded once, bit for bit
    (one f32 ulp in one entry of G would show: tests/test_control_edges_cpu.py); the recipe itself is held to 60 digits there."""
    from ml4ca_amd.policy import controller_label
    case = CE.pack_label_case()
    mask = torch.full((CE.N,), 9, dtype=torch.uint8, device=env.device)
    _lib_check(env, _dev(case['table']), mask)
    act, z = controller_label(env, _dev(case['obs']), _dev(case['done']), z=_dev(case['z0']))
    torch.cuda.synchronize()
    act, mask = _np(act), _np(mask)
    env.set_dp_controller_table(None)
    assert np.array_equal(mask, case['refused'].astype(np.uint8)), [case['names'].get(i, i) for i in np.flatnonzero(mask != case['refused'])]
    want, _ = CE.pid_host32(case)
    keep = ~case['refused']
    assert CE.bits_equal(act[:, keep], want[:, keep]).all(), [case['names'].get(i, i) for i in np.flatnonzero(~CE.bits_equal(act, want).all((0, 2)) & keep)]
    assert (act[:, ~keep] == F32([0, 0, 0, 0, 1, 0, 1])).all()
    near = [i for i, s in case['names'].items() if 'nearly' in s][0]
    assert (np.abs(act[:, near, 0:3]) < 1).all() and (act[:, near, 1:3] > 0.01).any()    # a G of 1e5 flown below saturation
