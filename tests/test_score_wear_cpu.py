"""Host side of the score card's wear axis (IADC, the integral absolute derivative of the commands): the reference pin of
evaluate.iadc_series (tests/golden/iadc.npz, written by tools/gen_golden_iadc.py from the reference's own script on the recorded QP and RL
box tests), the uniform-grid metric evaluate.iadc, the n-objective front, and the C ABI's sizes, struct layout and refusals - all decided on
the host before any device call, so none of this needs a GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from ml4ca_amd import _lib
from ml4ca_amd import evaluate as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a non-NULL, 16-byte aligned "device pointer": a refused call never touches it


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'iadc.npz'))


def _series(g, name, **kw):
    return EV.iadc_series(g[name + '_nbow'], g[name + '_time_bow'], g[name + '_nport'], g[name + '_nstar'], g[name + '_aport'],
                          g[name + '_astar'], g[name + '_time_stern'], **kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()) if a.size else 0.0


# ---- the reference pin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['QP', 'RL'])
def test_iadc_series_reproduces_the_reference(golden, name):
    """float64 against float64, the same operations: per-interval entries of all six lists, the per-interval totals and the running sums."""
    r = _series(golden, name)
    for k in range(6):
        assert _rel(r['derivs'][k], golden['%s_derivs%d' % (name, k)]) < 1e-12, k
    assert golden['%s_IADC' % name][0] == 0.0
    assert _rel(r['iadc'], golden['%s_IADC' % name][1:]) < 1e-12
    # the script's IADC_cumsums is cumsums[:-1]: its printed total leaves out the last interval
    assert _rel(r['cumsum'][:-1], golden['%s_IADC_cumsums' % name]) < 1e-12
    assert len(r['cumsum']) == len(golden['%s_IADC_cumsums' % name]) + 1
    # the split is the same numbers: thrust part + azimuth part = the total (nothing here is near the clip)
    assert _rel(r['rps'] + r['angle'], r['iadc']) < 1e-12
    assert _rel(r['cum_rps'][-1] + r['cum_angle'][-1], r['cumsum'][-1]) < 1e-12
    assert float(np.abs(r['derivs'][1]).max()) == 0.0                       # the bow azimuth is not counted


def test_the_recorded_totals_are_the_thesis_numbers(golden):
    want = dict(pseudo=965.35, QP=488.27, RL=44.87, RLintegral=54.67)
    got = dict(zip([str(m) for m in golden['methods']], golden['totals']))
    for k, v in want.items():
        assert abs(got[k] - v) < 0.005, (k, got[k])
    assert abs(_series(golden, 'QP')['cumsum'][-2] - got['QP']) < 1e-9 and abs(_series(golden, 'RL')['cumsum'][-2] - got['RL']) < 1e-9


def test_the_pin_exercises_the_short_interval_rule(golden):
    """QP is the recording with intervals under 0.1 s; without the rule the function does NOT reproduce it.  RL never fires the rule."""
    short = int((np.diff(golden['QP_time_stern'])[1:] < 0.1).sum())
    assert short > 0 and int((np.diff(golden['QP_time_bow'])[1:] < 0.1).sum()) > 0
    plain = _series(golden, 'QP', short_rule=False)
    assert _rel(plain['iadc'], golden['QP_IADC'][1:]) > 1e-3
    assert abs(plain['cumsum'][-2] - golden['QP_IADC_cumsums'][-1]) > 1.0
    assert int((np.diff(golden['RL_time_stern'])[1:] < 0.1).sum()) == 0 and int((np.diff(golden['RL_time_bow'])[1:] < 0.1).sum()) == 0
    assert _rel(_series(golden, 'RL', short_rule=False)['iadc'], golden['RL_IADC'][1:]) == 0.0


def test_the_short_interval_rule_is_the_quirk_as_written():
    """an interval under 0.1 s re-uses the previous entry, which is already multiplied by its dt, and multiplies it by 0.1 again"""
    t = np.array([0.0, 0.2, 0.25, 0.45])
    n = np.array([0.0, 10.0, 50.0, 50.0])
    z = np.zeros(4)
    r = EV.iadc_series(n, t, z, z, z, z, t)
    first = (abs(10.0 - 0.0) / 0.2 / 100.0) * 0.2
    assert r['derivs'][0][0] == first and r['derivs'][0][1] == first * 0.1 and r['derivs'][0][2] == 0.0
    # sums by index over the SHORTER series
    r = EV.iadc_series(n, t, z[:3], z[:3], z[:3], z[:3], t[:3])
    assert len(r['iadc']) == 2 and len(r['derivs'][0]) == 3


# ---- the uniform-grid metric ------------------------------------------------------------------------------------------------------
def test_iadc_on_a_uniform_grid_equals_the_series_function():
    """evaluate.iadc has no dt: (x / dt) * dt against x.  With u = 2^-53, per term: the series form rounds x / dt, / scale and * dt
    (three roundings; dt itself - a difference of rounded grid times - cancels up to them), the grid form rounds x / scale (one): 4 u
    relative.  Summing m non-negative terms adds at most (m - 1) u relative.  So each part agrees within (4 + m) u relative - the thrust
    part as it stands.  The azimuth part is fed in degrees to one form and in radians to the other, and a difference of two converted
    angles loses RELATIVE accuracy when it is small, so its terms get an absolute allowance: each angle is converted with at most 180 u
    deg of error (two per difference: 2 u after / 180), the wrap's d + 180 and the radian form's 2 pi - d round by at most 360 u deg and
    2 pi u rad (2 u each after the scale), and the conversions' own relative roundings on a term of at most 1 add 2 u more: 8 u per
    angle term, 16 u per interval, 16 m u in all."""
    torch = pytest.importorskip('torch')
    rng = np.random.RandomState(3)
    T, n = 120, 5
    act = rng.uniform(-1.3, 1.3, size=(T, n, 7))
    a = torch.from_numpy(act)
    got = EV.iadc(a, 'final', True)
    thr = EV.commanded_thrust(a).numpy()
    alpha = np.degrees(EV.commanded_azimuth(a, 'final', True).numpy())
    t = 0.2 * np.arange(T)
    m, u = T - 1, 2.0 ** -53
    bound, abs_angle = (4 + m) * u, 16 * m * u
    for i in range(n):
        r = EV.iadc_series(thr[:, i, 0], t, thr[:, i, 1], thr[:, i, 2], alpha[:, i, 0], alpha[:, i, 1], t)
        assert abs(r['cum_rps'][-1] - float(got['iadc_rps'][i])) <= bound * r['cum_rps'][-1]
        assert abs(r['cum_angle'][-1] - float(got['iadc_angle'][i])) <= bound * r['cum_angle'][-1] + abs_angle
        assert abs(r['cumsum'][-1] - float(got['iadc'][i])) <= (bound + 2 * m * u) * r['cumsum'][-1] + abs_angle      # + the by-interval sum order
    per = EV.iadc(a, 'final', True, per_step=True)
    assert per['iadc'].shape == (T - 1, n) and torch.allclose(per['iadc'].sum(0), got['iadc'], rtol=1e-13, atol=0)


def test_the_azimuth_change_is_counted_the_short_way_round():
    torch = pytest.importorskip('torch')
    a0, a1 = math.radians(179.0), math.radians(-179.0)
    act = torch.zeros((2, 1, 7), dtype=torch.float64)
    act[0, 0, 3], act[0, 0, 4] = math.sin(a0), math.cos(a0)        # port head: +179 deg, then -179 deg
    act[1, 0, 3], act[1, 0, 4] = math.sin(a1), math.cos(a1)
    act[:, 0, 6] = 1.0                                              # star head: 0 deg throughout
    r = EV.iadc(act, 'final', True)
    assert abs(float(r['iadc_angle'][0]) - 2.0 / 180.0) < 1e-12 and float(r['iadc_rps'][0]) == 0.0
    s = EV.iadc_series([0, 0], [0.0, 0.2], [0, 0], [0, 0], [179.0, -179.0], [0, 0], [0.0, 0.2])
    assert abs(s['angle'][0] - 2.0 / 180.0) < 1e-12 and abs(s['angle'][0] - 358.0 / 180.0) > 1.0
    # the same in the full variant's linear decode
    act = torch.zeros((2, 1, 6), dtype=torch.float64)
    act[0, 0, 4], act[1, 0, 4] = 179.0 / 180.0, -179.0 / 180.0
    assert abs(float(EV.iadc(act, 'full', False)['iadc_angle'][0]) - 2.0 / 180.0) < 1e-12


def test_an_interval_is_at_most_8_far_below_the_reference_clip():
    torch = pytest.importorskip('torch')
    act = torch.zeros((2, 1, 6), dtype=torch.float64)
    act[0, 0, :3], act[1, 0, :3] = -5.0, 5.0                        # -100 % -> +100 % on all three: 3 * 2
    act[0, 0, 4:6], act[1, 0, 4:6] = 0.5, -0.5                      # +90 deg -> -90 deg on both: 2 * 1 (the most the short way round gives)
    r = EV.iadc(act, 'full', False)
    assert float(r['iadc_rps'][0]) == 6.0 and abs(float(r['iadc_angle'][0]) - 2.0) < 1e-15 and float(r['iadc'][0]) <= 8.0 < 400.0
    rng = np.random.RandomState(0)
    big = torch.from_numpy(rng.normal(0, 50.0, size=(400, 3, 7)))
    for variant, ca in (('full', False), ('simple', False), ('limited', False), ('final', False), ('final', True)):
        assert float(EV.iadc(big, variant, ca, per_step=True)['iadc'].max()) <= 8.0
    assert float(EV.iadc(big, 'simple', False)['iadc_angle'].abs().max()) == 0.0


def test_commanded_azimuth_per_variant():
    torch = pytest.importorskip('torch')
    a = torch.tensor([[0.1, 0.2, 0.3, 0.25, -0.5, 1.5, 0.0]], dtype=torch.float64)
    pi = math.pi
    assert torch.allclose(EV.commanded_azimuth(a, 'full', False), torch.tensor([[-0.5 * pi, pi]], dtype=torch.float64))
    assert torch.allclose(EV.commanded_azimuth(a, 'limited', False), torch.tensor([[0.125 * pi, -0.25 * pi]], dtype=torch.float64))
    assert torch.allclose(EV.commanded_azimuth(a, 'final', False), torch.tensor([[0.25 * pi, -0.5 * pi]], dtype=torch.float64))
    assert torch.allclose(EV.commanded_azimuth(a, 'final', True), torch.tensor([[math.atan2(0.25, -0.5), math.atan2(1.5, 0.0)]], dtype=torch.float64))
    assert EV.commanded_azimuth(a, 'simple', False).abs().max() == 0
    w = torch.tensor([[0, 0, 0, 1.25, -1.5]], dtype=torch.float64)          # the wrap form: 1.25 -> -0.75, -1.5 -> 0.5
    assert torch.allclose(EV.commanded_azimuth(w, 'final', False), torch.tensor([[-0.75 * pi, 0.5 * pi]], dtype=torch.float64))
    with pytest.raises(ValueError):
        EV.commanded_azimuth(a[:, :5], 'final', True)
    with pytest.raises(ValueError):
        EV.commanded_azimuth(a, 'other', False)


# ---- the n-objective front --------------------------------------------------------------------------------------------------------
def test_pareto_front_nd_agrees_with_the_two_objective_front_and_brute_force():
    rng = np.random.RandomState(5)
    for trial in range(20):
        m = int(rng.randint(1, 25))
        a, b, c = (np.round(rng.uniform(0, 1, m), 1 if trial % 2 else 6) for _ in range(3))     # coarse rounding: ties and equal points
        assert np.array_equal(EV.pareto_front_nd(a, b), EV.pareto_front(a, b))
        got = EV.pareto_front_nd(a, b, c)
        P = np.stack([a, b, c], 1)
        want = [i for i in range(m) if not any(all(P[j] <= P[i]) and any(P[j] < P[i]) for j in range(m))]
        assert sorted(got.tolist()) == want
        assert got.tolist() == sorted(want, key=lambda i: (a[i], b[i], c[i], i))
        assert np.array_equal(EV.pareto_front_nd(P), got)
        if len(set(zip(a.tolist(), b.tolist()))) == m:                   # no two points tie on both: the 2-front survives a third objective
            assert set(EV.pareto_front(a, b).tolist()) <= set(got.tolist())
    with pytest.raises(ValueError):
        EV.pareto_front_nd([1.0, 2.0], [1.0])


# ---- the C ABI: sizes, layout, refusals -------------------------------------------------------------------------------------------
def test_abi_is_still_6_and_the_score_state_is_untouched():
    lib = _lib.load()
    assert lib.dpenv_abi_version() == 6
    assert lib.dpenv_score_state_bytes(1) == 128


def test_wear_state_bytes_linear_and_zero_below_one():
    lib = _lib.load()
    b1 = lib.dpenv_score_wear_state_bytes(1)
    assert b1 == 64
    for n in (2, 3, 63, 64, 65, 200, 65536, 1 << 24):
        assert lib.dpenv_score_wear_state_bytes(n) == n * b1
    assert lib.dpenv_score_wear_state_bytes(0) == 0 and lib.dpenv_score_wear_state_bytes(-5) == 0
    w = lib.dpenv_score_wear_summary_workspace_bytes
    assert w(1) == _lib.SCORE_WEAR_NOUT * 3 * 8 and w(64) == w(1) and w(65) == 2 * w(1) and w(0) == 0 and w(-1) == 0


def test_struct_layout_matches_header(tmp_path):
    import subprocess
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(dpenv_score_wear_io), offsetof(dpenv_score_wear_io, struct_size),'
                   ' offsetof(dpenv_score_wear_io, variant), offsetof(dpenv_score_wear_io, cont_ang), DPENV_SCORE_WEAR_RPS, DPENV_SCORE_WEAR_ANGLE,'
                   ' DPENV_SCORE_WEAR_EP_RPS, DPENV_SCORE_WEAR_EP_ANGLE, DPENV_SCORE_WEAR_NOUT);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.ScoreWearIO
    assert got == [C.sizeof(S), S.struct_size.offset, S.variant.offset, S.cont_ang.offset, _lib.SCORE_WEAR_RPS, _lib.SCORE_WEAR_ANGLE,
                   _lib.SCORE_WEAR_EP_RPS, _lib.SCORE_WEAR_EP_ANGLE, _lib.SCORE_WEAR_NOUT]
    assert C.sizeof(S) == 12


def _io(**kw):
    lib = _lib.load()
    io = _lib.ScoreIO()
    assert lib.dpenv_score_default_io(C.byref(io)) == _lib.OK
    io.T, io.n = 4, 8
    io.obs, io.act, io.rew = FAKE, FAKE, FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(io, k)[j] = x
        else:
            setattr(io, k, v)
    return lib, io


def _wio(variant=_lib.FINAL, cont_ang=1, struct_size=None):
    w = _lib.ScoreWearIO()
    w.struct_size = C.sizeof(w) if struct_size is None else struct_size
    w.variant, w.cont_ang = variant, cont_ang
    return w


# everything dpenv_score_accumulate refuses (tests/test_score_cpu.py's list) ...
SCORE_REFUSALS = [
    ('struct_size', dict(struct_size=8), b'struct_size'),
    ('T', dict(T=0), b'T'),
    ('T negative', dict(T=-3), b'T'),
    ('n', dict(n=0), b'n ='),
    ('obs_stride', dict(obs_stride=2), b'obs_stride'),
    ('act_stride', dict(act_stride=2), b'act_stride'),
    ('integ without obs', dict(obs=None, integ=FAKE), b'integ'),
    ('obs_dtype', dict(obs_dtype=7), b'obs_dtype'),
    ('dt zero', dict(dt=0.0), b'dt'),
    ('dt negative', dict(dt=-0.2), b'dt'),
    ('dt nan', dict(dt=float('nan')), b'dt'),
    ('dt inf', dict(dt=float('inf')), b'dt'),
    ('norm zero', dict(norm=(5.0, 0.0, 25.0)), b'norm[1]'),
    ('norm negative', dict(norm=(-5.0, 5.0, 25.0)), b'norm[0]'),
    ('norm nan', dict(norm=(5.0, 5.0, float('nan'))), b'norm[2]'),
    ('norm inf', dict(norm=(float('inf'), 5.0, 25.0)), b'norm[0]'),
    ('power_coeff', dict(power_coeff=(float('nan'), 1.0, 1.0)), b'power_coeff[0]'),
    ('rps_max', dict(rps_max=(33.0, float('inf'), 11.0)), b'rps_max[1]'),
]


@pytest.mark.parametrize('what,kw,field', SCORE_REFUSALS, ids=[r[0] for r in SCORE_REFUSALS])
def test_the_one_pass_call_refuses_what_accumulate_refuses(what, kw, field):
    lib, io = _io(**kw)
    w = _wio()
    assert lib.dpenv_score_accumulate_wear(FAKE, FAKE, C.byref(io), C.byref(w), None) == _lib.EINVAL, what
    msg = lib.dpenv_last_error(None)
    assert b'dpenv_score_accumulate_wear' in msg and field in msg, msg


# ... and what the wear axis adds: (io fields, wio arguments, the field named)
WEAR_REFUSALS = [
    ('wio struct_size', {}, dict(struct_size=8), b'wio struct_size'),
    ('variant above', {}, dict(variant=4, cont_ang=0), b'variant'),
    ('variant below', {}, dict(variant=-1, cont_ang=0), b'variant'),
    ('cont_ang on full', dict(act_stride=7), dict(variant=_lib.FULL, cont_ang=1), b'cont_ang'),
    ('cont_ang on simple', dict(act_stride=7), dict(variant=_lib.SIMPLE, cont_ang=1), b'cont_ang'),
    ('cont_ang on limited', dict(act_stride=7), dict(variant=_lib.LIMITED, cont_ang=1), b'cont_ang'),
    ('act NULL', dict(act=None), {}, b'act is NULL'),
    ('act_stride full', dict(act_stride=5), dict(variant=_lib.FULL, cont_ang=0), b'act_stride'),
    ('act_stride limited', dict(act_stride=4), dict(variant=_lib.LIMITED, cont_ang=0), b'act_stride'),
    ('act_stride final wrap', dict(act_stride=4), dict(variant=_lib.FINAL, cont_ang=0), b'act_stride'),
    ('act_stride final cont', dict(act_stride=6), dict(variant=_lib.FINAL, cont_ang=1), b'act_stride'),
]


@pytest.mark.parametrize('what,kw,wkw,field', WEAR_REFUSALS, ids=[r[0] for r in WEAR_REFUSALS])
def test_the_one_pass_call_refuses_on_the_host(what, kw, wkw, field):
    lib, io = _io(**kw)
    w = _wio(**wkw)
    assert lib.dpenv_score_accumulate_wear(FAKE, FAKE, C.byref(io), C.byref(w), None) == _lib.EINVAL, what
    msg = lib.dpenv_last_error(None)
    assert b'dpenv_score_accumulate_wear' in msg and field in msg, msg


def test_act_stride_is_measured_against_the_variants_act_dim():
    lib = _lib.load()
    for variant, ca in ((_lib.FULL, 0), (_lib.SIMPLE, 0), (_lib.LIMITED, 0), (_lib.FINAL, 0), (_lib.FINAL, 1)):
        cfg = _lib.Config()
        assert lib.dpenv_default_config(C.byref(cfg)) == _lib.OK
        cfg.variant, cfg.cont_ang = variant, ca
        ad = lib.dpenv_act_dim(C.byref(cfg))
        if ad > 3:
            _, io = _io(act_stride=ad - 1)
            w = _wio(variant, ca)
            assert lib.dpenv_score_accumulate_wear(FAKE, FAKE, C.byref(io), C.byref(w), None) == _lib.EINVAL
            assert ('>= %d' % ad).encode() in lib.dpenv_last_error(None)


def test_null_and_misaligned_pointers_are_refused():
    lib, io = _io()
    w = _wio()
    f = lib.dpenv_score_accumulate_wear
    assert f(None, FAKE, C.byref(io), C.byref(w), None) == _lib.EINVAL and b'state' in lib.dpenv_last_error(None)
    assert f(FAKE + 8, FAKE, C.byref(io), C.byref(w), None) == _lib.EINVAL and b'state' in lib.dpenv_last_error(None)
    assert f(FAKE, None, C.byref(io), C.byref(w), None) == _lib.EINVAL and b'wear is NULL' in lib.dpenv_last_error(None)
    assert f(FAKE, FAKE + 4, C.byref(io), C.byref(w), None) == _lib.EINVAL and b'wear must be 16-byte aligned' in lib.dpenv_last_error(None)
    assert f(FAKE, FAKE, None, C.byref(w), None) == _lib.EINVAL and b'io is NULL' in lib.dpenv_last_error(None)
    assert f(FAKE, FAKE, C.byref(io), None, None) == _lib.EINVAL and b'wio is NULL' in lib.dpenv_last_error(None)
    r = lib.dpenv_score_wear_read
    assert r(None, 8, FAKE, None) == _lib.EINVAL and b'wear' in lib.dpenv_last_error(None)
    assert r(FAKE + 8, 8, FAKE, None) == _lib.EINVAL and b'wear' in lib.dpenv_last_error(None)
    assert r(FAKE, 0, FAKE, None) == _lib.EINVAL and b'n =' in lib.dpenv_last_error(None)
    assert r(FAKE, 8, None, None) == _lib.EINVAL and b'out' in lib.dpenv_last_error(None)
    s = lib.dpenv_score_wear_summary
    assert s(None, 8, FAKE, FAKE, None) == _lib.EINVAL and b'wear' in lib.dpenv_last_error(None)
    assert s(FAKE, 8, None, FAKE, None) == _lib.EINVAL and b'out' in lib.dpenv_last_error(None)
    assert s(FAKE, 8, FAKE, None, None) == _lib.EINVAL and b'workspace' in lib.dpenv_last_error(None)
    assert s(FAKE, 0, FAKE, FAKE, None) == _lib.EINVAL and b'n =' in lib.dpenv_last_error(None)


def test_header_states_the_wear_law():
    txt = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    for line in ('d_n = ((|n_0 - n_0\'| + |n_1 - n_1\'|) + |n_2 - n_2\'|) / 100',
                 'w_k = fminf(|alpha_k - alpha_k\'|, 2pi_f - |alpha_k - alpha_k\'|)',
                 'd_a = (w_1 + w_2) / pi_f',
                 'iadc_rps += (double)d_n ;  iadc_angle += (double)d_a',
                 'cannot act - an interval is at most 3*2 + 2*1 = 8',
                 'Non-finite actions.'):
        assert line in txt, line
