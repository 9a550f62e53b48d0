"""tests/train_edges.py without a GPU: the tables reach what they name, the references are fair (train.py's closed forms equal torch float64
autograd of the module's MLP), torch float32 autograd put in the kernel's place passes every judge, and one wrong kernel per group - a
host-side mutant of the law - fails its group's judge.  tests/test_gpu_train_edges.py relies on all of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ml4ca_amd import train as TR
from tests import train_edges as E

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_buffer(grad_stats):
    """(grad, stats) as the float32 buffer [P + nstat] a kernel returns."""
    with np.errstate(over='ignore'):
        return np.concatenate([grad_stats[0], grad_stats[1]]).astype(F32)


_y = {}


def yard(name, case, stage, rows=None, dtype='float32'):
    """torch_law, once per (table, stage, rows, dtype)."""
    key = (name, stage, None if rows is None else np.asarray(rows).tobytes(), dtype)
    if key not in _y:
        _y[key] = E.torch_law(case, stage, rows, dtype=dtype)
    return _y[key]


def rows_of(count):
    return np.array([0]) if count == 1 else np.arange(65)


def parity(name, case, stage, rows, got=None, what='cpu'):
    """The parity judge with torch float32 in the kernel's place unless `got` is given."""
    actor = stage != 'value'
    sls = E.slices(case['in_dim'], case['out_dim'] if actor else 1, actor)
    ref32 = yard(name, case, stage, rows)
    got = as_buffer(ref32) if got is None else got
    return E.judge('%s %s %s count %d' % (what, name, stage, len(rows)), got, E.reference(case, stage, rows), ref32, sls, len(rows), stage,
                   E.stat_scales(case, stage, rows))


def fair(name, case, stage, rows):
    """train.py's closed form equals torch float64 autograd of the module's MLP to 1e-9, per tensor and per statistic; and actor_law /
    value_law with every knob at its default is that closed form."""
    actor = stage != 'value'
    sls = E.slices(case['in_dim'], case['out_dim'] if actor else 1, actor)
    g, s = E.closed_form(case, stage, rows)
    tg, ts = yard(name, case, stage, rows, dtype='float64')
    for tensor, err in E.rel_errors(g, tg, sls).items():
        assert err <= 1e-9, (name, stage, tensor, err)
    assert np.abs(s - ts).max() <= 1e-9 * max(1.0, np.abs(ts).max()), (name, stage, s, ts)
    g2, s2 = E.reference(case, stage, rows)
    assert np.array_equal(g, g2) and np.array_equal(s, s2), (name, stage)


# ---- the restated constants ----
def test_chain_K_is_the_two_files():
    from tests.test_gpu_imitation import chain_K as imit_K
    from tests.test_gpu_ppo_update import chain_K as ppo_K
    for count in (1, 63, 64, 65, 165, 257, 33000):
        assert E.chain_K(count, 'ppo') == E.chain_K(count, 'value') == ppo_K(count)
        assert E.chain_K(count, 'nll') == E.chain_K(count, 'mse') == imit_K(count)


def test_the_module_imports_without_torch():
    code = "import sys; import tests.train_edges; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT).returncode == 0


# ---- A ----
@pytest.mark.parametrize('shape', E.A_ACTORS + ((9, 7, 0.2),))
def test_a_actor_tables(shape):
    case = E.table_a(*shape)
    name = 'A %d->%d leak %.1f' % shape
    assert case['obs'].shape == (65, shape[0]) and case['act'].shape == (65, shape[1]) and case['pi_theta'].size == TR.layout(shape[0], shape[1], True)['P']
    assert not E.near_kink(case).any() and not E.cut_rows(case)[[0, 64]].any()
    for stage in E.ACTOR_STAGES:
        for count in E.COUNTS:
            rows = rows_of(count)
            ref = E.reference(case, stage, rows)
            live = [n for n, sl in E.slices(shape[0], shape[1]) if np.abs(ref[0][sl]).max() > 0]
            assert len(live) == (8 if stage == 'mse' else 9), (name, stage, count, live)        # no tensor compares zero with zero (MSE: log_std is zero)
            fair(name, case, stage, rows)
            parity(name, case, stage, rows)


@pytest.mark.parametrize('shape', E.A_CRITICS)
def test_a_critic_tables(shape):
    case = E.critic_case(*shape)
    name = 'A %d->1 leak %.1f' % shape
    for count in E.COUNTS:
        rows = rows_of(count)
        assert all(np.abs(E.reference(case, 'value', rows)[0][sl]).max() > 0 for _, sl in E.slices(shape[0], 1, False))
        fair(name, case, 'value', rows)
        parity(name, case, 'value', rows)


def test_a_mutant_garbage_in_the_padding_fails():
    for (i, o, leak), stage in (((6, 7, 0.2), 'ppo'), ((1, 1, 0.2), 'nll'), ((9, 1, 0.2), 'mse'), ((6, 7, 0.2), 'value')):
        case = E.table_a(i, o, leak)
        with pytest.raises(AssertionError):
            parity('A %d->%d' % (i, o), case, stage, np.arange(65), got=as_buffer(E.padding_mutant(case, stage, np.arange(65))), what='mutant')
    case = E.table_a(16, 7, 0.2)                                 # in = 16 has no padding: the mutant is the law, and passes
    g, s = E.padding_mutant(case, 'ppo', np.arange(65))
    assert np.array_equal(g, E.reference(case, 'ppo')[0])


# ---- B ----
@pytest.mark.parametrize('log_std', E.B_LOG_STDS)
def test_b_tables(log_std):
    case = E.table_b(log_std)
    name = 'B log_std %g' % log_std
    Ws, bs, ls = TR.unflatten(case['pi_theta'], 9, 7, True)
    assert not Ws[3].any() and (ls == F32(log_std)).all()
    mu = TR._forward64(case['pi_theta'], case['obs'], 9, 7, True, 0.2)[5]
    assert np.array_equal(mu, np.broadcast_to(bs[3].astype(F64), mu.shape))           # W3 = 0 gives mu == b3
    r = E.ratios(case)
    assert (np.abs(r - 1.2) >= E.RATIO_MARGIN).all() and (np.abs(r - 0.8) >= E.RATIO_MARGIN).all() and (np.abs(r[[0, 64]] - 1.0) < 0.1).all()
    zero = E.below_b3()
    for stage in E.B_STAGES:
        for count in E.COUNTS:
            rows = rows_of(count)
            ref = E.reference(case, stage, rows)
            for n, sl in E.slices(9, 7):
                assert (np.abs(ref[0][sl]).max() == 0) == (n in zero), (name, stage, n)
            fair(name, case, stage, rows)
            parity(name, case, stage, rows)


@pytest.mark.parametrize('knob', (dict(ls_factor=False), dict(sd_eps=0.0)))
def test_b_mutants_fail(knob):
    """The e^ls / sd factor dropped, and the + 1e-8 dropped: each fails somewhere in the table - and passes at log_std 1 and 5, which is why
    the suite's log_std in [-0.8, -0.2] never saw them."""
    failed = {}
    for log_std in E.B_LOG_STDS:
        case = E.table_b(log_std)
        rows = np.arange(65)
        failed[log_std] = not E.passes(parity, 'B log_std %g' % log_std, case, 'ppo', rows, got=as_buffer(E.reference(case, 'ppo', rows, **knob)), what='mutant')
    assert failed[-18.0] and failed[-14.0], failed
    assert not failed[1.0] and not failed[5.0], failed


# ---- C ----
@pytest.mark.parametrize('clip', E.C_CLIPS)
def test_c_ties(clip):
    case = E.table_c(clip)
    b3, act = case['b3'], case['act']
    assert not np.mod(b3 * 8, 1).any() and not np.mod((act - b3[None, :]).astype(F64) * 8, 1).any()
    assert F32(np.exp(F32(0.0))) + F32(1e-8) == F32(1.0)
    # the float32 restatement: logp - logp_old is +0 and the ratio exactly 1, in NumPy ...
    logp = E.logp_f32(b3, act)
    d = (logp - case['logp_old']).astype(F32)
    assert not d.any() and not np.signbit(d).any() and (np.exp(d) == F32(1.0)).all()
    # ... and it is the float64 log-probability rounded (the restatement is a fair float32 evaluation)
    assert np.abs(logp - E.logp64(case['pi_theta'], case['obs'], act, 0.2)[0]).max() <= 16 * 2.0 ** -24 * np.abs(logp).max()
    assert (case['adv'] > 0).any() and (case['adv'] < 0).any() and case['adv'].all()
    sls = E.slices(9, 7)
    for count in E.COUNTS:
        rows = rows_of(count)
        # the reference: the header's law with the ratio float32 forms.  Every row flows, with -A / count.
        ref = E.reference(case, 'ppo', rows, ratio=1.0)
        A = case['adv'][rows].astype(F64)
        assert ref[1][2] == 0.0 and ref[1][3] == 1.0 and ref[1][0] == -A.mean()
        live = E.reference(case, 'ppo', rows, ratio=1.0, flows=np.ones(len(rows), bool))
        assert np.array_equal(ref[0], live[0]) and np.abs(ref[0][sls[6][1]]).max() > 0
        ref[1][1] = 0.0                                            # approx_kl: logp_old IS the float32 logp
        ref32 = yard('C clip %g' % clip, case, 'ppo', rows)
        assert ref32[1][1] == 0.0 and ref32[1][2] == 0.0 and ref32[1][3] == 1.0, ref32[1]       # torch float32 forms the same ratio
        E.judge('cpu C clip %g count %d' % (clip, len(rows)), as_buffer(ref32), ref, ref32, sls, len(rows), 'ppo', E.stat_scales(case, 'ppo', rows))


def c_reference(case, rows, **knobs):
    ref = E.reference(case, 'ppo', rows, ratio=1.0, **knobs)
    ref[1][1] = 0.0
    return ref


@pytest.mark.parametrize('knob,clips', ((dict(strict_tie=True), (0.2, 0.0)), (dict(clip_frac_ge=True), (0.0,))))
def test_c_mutants_fail(knob, clips):
    """s1 < s2 drops every tied row (both clips); clip_frac with >= counts the rows on the bounds (clip 0)."""
    for clip in clips:
        case = E.table_c(clip)
        rows = np.arange(65)
        ref32 = yard('C clip %g' % clip, case, 'ppo', rows)
        with pytest.raises(AssertionError):
            E.judge('mutant C clip %g' % clip, as_buffer(c_reference(case, rows, **knob)), c_reference(case, rows), ref32, E.slices(9, 7), 65, 'ppo',
                    E.stat_scales(case, 'ppo', rows))


@pytest.mark.parametrize('all_zero', (False, True))
def test_c_zero_advantages(all_zero):
    case = E.table_c_zero_adv(all_zero)
    adv = case['adv']
    assert not adv[list(E.C_PLUS_ZERO + E.C_MINUS_ZERO)].any() and np.signbit(adv[list(E.C_MINUS_ZERO)]).all() and not np.signbit(adv[list(E.C_PLUS_ZERO)]).any()
    assert adv.any() != all_zero
    rows = np.arange(65)
    ref = E.reference(case, 'ppo', rows)
    if all_zero:
        assert not ref[0].any() and ref[1][0] == 0.0 and ref[1][2] > 0
    else:
        # the rows contribute nothing: the call without them, rescaled to the same count, is the same gradient
        rest = np.flatnonzero(adv != 0)
        g2, _ = E.reference(case, 'ppo', rest)
        assert np.abs(ref[0] - g2 * len(rest) / 65.0).max() <= 1e-15 * np.abs(ref[0]).max()
    fair('C zero adv %d' % all_zero, case, 'ppo', rows)
    parity('C zero adv %d' % all_zero, case, 'ppo', rows)


# ---- D ----
def test_d_tags_are_the_rows_in_the_band():
    case = E.table_d()
    band, amb = np.flatnonzero(E.band_rows(case)), np.flatnonzero(E.ambiguous_rows(case))
    assert band.tolist() == [20, 64, 65, 66, 67, 68]
    assert amb.tolist() == [20, 64] + [65 + k for k, (_, _, a) in enumerate(E.D_SINGLE) if a] == [20, 64, 65, 68]
    assert np.flatnonzero(E.ambiguous_rows(case)[E.D_CALL_ROWS]).tolist() == np.flatnonzero(E.band_rows(case)[E.D_CALL_ROWS]).tolist() == list(E.D_CALL_BAND)
    r = E.ratios(case)
    for k, (bound, a, _) in enumerate(E.D_SINGLE):
        assert abs(r[65 + k] / (1.2 if bound == 'upper' else 0.8) - 1.0) < E.BAND and case['adv'][65 + k] == a
    for row in band:                                            # powers of two: ratio x A and bound x A are exact
        assert np.frexp(np.abs(case['adv'][row]))[0] == 0.5
    assert not E.near_kink(case, skip=band.tolist()).any()
    fair('D', case, 'ppo', np.setdiff1d(np.arange(69), band))     # D's references are the closed form on the ordinary rows ...
    fair('D call', case, 'ppo', E.D_CALL_ROWS)                     # ... and on the call, whatever side float64 puts the two rows on


def test_d_torch_float32_is_accepted():
    case = E.table_d()
    sls = E.slices(9, 7)
    for k, (bound, a, ambiguous) in enumerate(E.D_SINGLE):
        rows = np.array([65 + k])
        got = as_buffer(yard('D', case, 'ppo', rows))
        flows, outside = E.judge_either_side('cpu D %s A %+g' % (bound, a), got, case, rows, (0,), sls)
        assert flows[0] == ((not outside[0]) if ambiguous else True)
    got = as_buffer(yard('D call', case, 'ppo', E.D_CALL_ROWS))
    E.judge_either_side('cpu D call', got, case, E.D_CALL_ROWS, E.D_CALL_BAND, sls)


def test_d_the_judge_lets_nothing_else_choose():
    """A decided row that is cut, a third row that changes sides, and a clip_frac that disagrees with the side taken are all refused."""
    case = E.table_d()
    sls = E.slices(9, 7)
    rows = np.array([66])                                       # upper bound, A < 0: flows on both sides
    for outside in (False, True):
        E.judge_either_side('cpu D decided', as_buffer(E.reference(case, 'ppo', rows, flows=np.array([True]), outside=np.array([outside]))), case, rows, (0,), sls)
        cut = as_buffer(E.reference(case, 'ppo', rows, flows=np.array([False]), outside=np.array([outside])))
        with pytest.raises(AssertionError):
            E.judge_either_side('mutant D decided row cut', cut, case, rows, (0,), sls)
    rows = np.array([65])                                       # upper bound, A > 0: either side, but clip_frac goes with it
    for flows in (True, False):
        g, s = E.reference(case, 'ppo', rows, flows=np.array([flows]), outside=np.array([not flows]))
        assert s[2] == (0.0 if flows else 1.0) and bool(g.any()) == flows
        E.judge_either_side('cpu D', as_buffer((g, s)), case, rows, (0,), sls)
        s[2] = 1.0 - s[2]
        with pytest.raises(AssertionError):
            E.judge_either_side('mutant D clip_frac on the other side', as_buffer((g, s)), case, rows, (0,), sls)
    base = ~E.cut_rows(case)[E.D_CALL_ROWS]
    third = base.copy()
    third[int(np.flatnonzero(base & (np.arange(65) != 20) & (np.arange(65) != 64))[0])] = False
    with pytest.raises(AssertionError):
        E.judge_either_side('mutant D a third row cut', as_buffer(E.reference(case, 'ppo', E.D_CALL_ROWS, flows=third)), case, E.D_CALL_ROWS,
                            E.D_CALL_BAND, sls)
    for pick in ((True, True), (True, False), (False, True), (False, False)):        # each of the four references of the call is accepted
        flows, outside = base.copy(), np.zeros(65, bool) | ((E.ratios(case, E.D_CALL_ROWS) > 1.2) | (E.ratios(case, E.D_CALL_ROWS) < 0.8))
        for pos, f in zip(E.D_CALL_BAND, pick):
            flows[pos], outside[pos] = f, not f
        got = as_buffer(E.reference(case, 'ppo', E.D_CALL_ROWS, flows=flows, outside=outside))
        f2, o2 = E.judge_either_side('cpu D call %s' % (pick,), got, case, E.D_CALL_ROWS, E.D_CALL_BAND, sls)
        assert np.array_equal(f2, flows) and np.array_equal(o2, outside)


def test_d_extreme_ratios():
    """exp(-+200) leaves float32: the expectation is the law with ratio 0 or +inf.  torch float32 autograd is NOT put in the kernel's place
    for +200: its exp backward multiplies the zero gradient of the cut row by the infinite ratio and returns NaN where the header's rule
    (the gradient is 0 where s1 > s2) gives zero."""
    case = E.table_d_extreme()
    with np.errstate(over='ignore', under='ignore'):
        r32 = np.exp((E.logp64(case['pi_theta'], case['obs'], case['act'], 0.2)[0] - case['logp_old']).astype(F32))
    assert r32.tolist() == [0.0, 0.0, np.inf]
    P = case['pi_theta'].size
    for row, (d, a) in enumerate(E.D_EXTREME):
        want = E.extreme_expectation(case, row)
        assert abs(abs(want[1]) - 200.0) < 1e-3 and np.sign(want[1]) == -np.sign(d)
        with np.errstate(over='ignore'):
            E.judge_extreme('cpu D extreme %+g A %+g' % (d, a), np.concatenate([np.zeros(P), want]).astype(F32), case, row)
        if d < 0:                                                # torch float32 forms ratio 0 and passes
            E.judge_extreme('cpu D extreme torch %+g A %+g' % (d, a), as_buffer(yard('D extreme', case, 'ppo', np.array([row]))), case, row)
        bad = np.concatenate([np.zeros(P), want]).astype(F32)
        bad[7] = 1e-30
        with pytest.raises(AssertionError):
            E.judge_extreme('mutant D extreme', bad, case, row)


# ---- E ----
@pytest.mark.parametrize('leak', E.E_LEAKS)
@pytest.mark.parametrize('kind', E.E_KINDS)
def test_e_tables(kind, leak):
    case = E.table_e(kind, leak)
    name = 'E %s leak %.1f' % (kind, leak)
    layers = E.zero_preactivation_layers(case)
    assert layers == {'pi_theta': [0] if kind == 'first' else [0, 1, 2], 'v_theta': [0] if kind == 'first' else [0, 1, 2]}
    assert not E.near_kink(case, skip=(64,)).any() and not E.cut_rows(case)[[0, 64]].any()
    for stage in E.E_STAGES:
        actor = stage == 'ppo'
        sls = E.slices(9, 7 if actor else 1, actor)
        for rows in (np.array([64]), np.arange(65)):
            fair(name, case, stage, rows)                        # torch float64 autograd takes the slope `leak` at z = 0: the header's claim
            parity(name, case, stage, rows)
        alone = E.reference(case, stage, np.array([64]))[0]
        zero = [n for n, sl in sls if not alone[sl].any()]
        if kind == 'all' and leak == 0.0:
            assert zero == [n for n, _ in sls][:7]               # everything below b3
        elif kind == 'all':
            assert zero == ['W0', 'W1', 'W2', 'W3']
        else:
            assert zero == (['W0', 'b0', 'W1'] if leak == 0.0 else ['W0', 'W1'])


@pytest.mark.parametrize('stage', E.E_STAGES)
def test_e_mutant_slope_one_at_zero_fails(stage):
    actor = stage == 'ppo'
    for kind, leak, rows in (('first', 0.2, np.array([64])), ('all', 0.0, np.array([64])), ('all', 0.2, np.arange(65))):
        case = E.table_e(kind, leak)
        with pytest.raises(AssertionError):
            parity('E %s leak %.1f' % (kind, leak), case, stage, rows, got=as_buffer(E.reference(case, stage, rows, slope_at_zero=1.0)), what='mutant')
    case = E.table_e('all', 1.0)                                 # at leak 1 the slope is 1 everywhere: the mutant is the law
    assert np.array_equal(E.reference(case, stage, None, slope_at_zero=1.0)[0], E.reference(case, stage)[0])


# ---- F ----
def scaled_reference(case):
    g, s = E.reference(case, 'ppo')
    s = s.copy()
    s[0] /= E.F_SCALE
    return g / E.F_SCALE, s


def test_f_scale():
    base, case = E.table_a(9, 7, 0.2), E.table_f()
    sls = E.slices(9, 7)
    g, s = E.reference(case, 'ppo')
    tiny = F32(2.0 ** -126)
    for n, sl in sls:
        assert np.abs(g[sl]).max() >= tiny                       # the largest element of every tensor stays normal ...
    sub = np.abs(g) < tiny
    assert sub.mean() > 0.2 and np.abs(case['adv']).max() * 2 > 2.0 ** -120     # ... and many of the rest are subnormal
    ref = scaled_reference(case)
    # the scaled law is the unscaled law up to the advantages that went subnormal in the float32 product
    for n, err in E.rel_errors(ref[0], E.reference(base, 'ppo')[0], sls).items():
        assert err < 1e-6, (n, err)
    ref32 = yard('A 9->7 leak 0.2', base, 'ppo', np.arange(65))           # the same bound: the unscaled rows' yardstick
    scales = E.stat_scales(case, 'ppo')
    # torch float32 on the scaled rows, in the kernel's place
    E.judge('cpu F', as_buffer(yard('F', case, 'ppo', np.arange(65))), ref, ref32, sls, 65, 'ppo', scales, rescale=1.0 / E.F_SCALE)
    # the mutant: a unit that flushes what is below 2^-126
    mutant = E.flush(as_buffer((g, s)))
    assert (mutant[:g.size] != as_buffer((g, s))[:g.size]).mean() > 0.2
    with pytest.raises(AssertionError):
        E.judge('mutant F', mutant, ref, ref32, sls, 65, 'ppo', scales, rescale=1.0 / E.F_SCALE)


# ---- G ----
def adam_mutant(kind, tab, t, gate_kl=None, kl_limit=float('inf'), stop=0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """TR.adam_step_ref with one error: 'eps_in_sqrt' (denom = sqrt(v + eps) / bc2s), 'powf' (the bias corrections' powers in float32),
    'gate_ge' (the gate closes at gate_kl >= kl_limit)."""
    f = F32
    theta, grad, m, v = (np.asarray(tab[k], f) for k in ('theta', 'grad', 'm', 'v'))
    closed = (F32(gate_kl) >= F32(kl_limit)) if kind == 'gate_ge' else (F32(gate_kl) > F32(kl_limit)) if gate_kl is not None else False
    if gate_kl is not None and (stop or closed):
        return theta.copy(), m.copy(), v.copy(), t - 1, 1
    b1, b2 = f(beta1), f(beta2)
    if kind == 'powf':
        def powi32(b, e):                                        # the statement's square-and-multiply, every product rounded to float32
            p = f(1)
            while e > 0:
                if e & 1:
                    p = f(p * b)
                b = f(b * b)
                e >>= 1
            return p
        with np.errstate(all='ignore'):
            p1, p2 = powi32(b1, t), powi32(b2, t)
    else:
        p1, p2 = TR._powi(float(b1), t), TR._powi(float(b2), t)
    with np.errstate(all='ignore'):
        step_size = f(lr) / f(1.0 - float(p1))
        bc2s = np.sqrt(f(1.0 - float(p2)))
        m2 = TR._fma32(f(1) - b1, grad - m, m)
        v2 = TR._fma32((f(1) - b2) * grad, grad, b2 * v)
        denom = (np.sqrt(v2 + f(eps)) / bc2s) if kind == 'eps_in_sqrt' else (np.sqrt(v2) / bc2s + f(eps))
        theta2 = TR._fma32(-step_size, m2 / denom, theta)
    return theta2, m2, v2, t, int(stop)


def test_g_table_reaches_its_limits():
    tab = E.table_g()
    g, m, v = tab['grad'], tab['m'], tab['v']
    tiny, big = F32(2.0 ** -126), float(np.finfo(F32).max)
    assert tab['theta'].size == E.G_P == 257 and E.G_P % 4 == 1
    assert ((v > 0) & (v < tiny)).any() and ((np.abs(m) > 0) & (np.abs(m) < tiny)).any()                  # subnormal v and m
    assert (g.astype(F64) ** 2 > big).any() and ((g != 0) & (np.abs(g) < tiny)).any()                      # g^2 above FLT_MAX; subnormal g
    assert ((g == 0) & ~np.signbit(g) & (m == 0) & (v == 0)).any() and ((g == 0) & np.signbit(g)).any()    # g = 0 on m = v = 0; g = -0.0
    c2g2 = ((F32(1) - F32(0.999)) * g).astype(F64) * g.astype(F64)
    assert ((c2g2 > 0) & (c2g2 < float(tiny))).any() and (c2g2 > big).any()                                # (1 - beta2) g^2 subnormal, and overflowing
    for g0, (m0, v0) in ((x, p) for x in E.G_GRADS for p in E.G_PRIORS):                                   # the whole cross product is there
        assert ((g == F32(g0)) & (np.abs(m) == F32(m0)) & (v == F32(v0))).any(), (g0, m0, v0)
    for t in E.G_STEPS:
        th, m2, v2, step, stop = E.adam_statement(tab, t)
        assert step == t and stop == 0
        inf = np.isinf(v2)
        assert inf.any() and np.array_equal(th[inf].view(np.int32), tab['theta'][inf].view(np.int32))      # denom = inf: theta keeps its bits
        assert not np.isnan(th).any()
        E.judge_adam('cpu G t %d' % t, (th, m2, v2, step, stop), E.adam_statement(tab, t))
    assert TR._powi(float(F32(0.999)), 100000) < 2.0 ** -126 and TR._powi(float(F32(0.9)), 10 ** 9) == 0.0
    th = E.adam_statement(tab, 1, eps=0.0)[0]
    assert np.isnan(th).any() and not np.isnan(th).all()                                                   # eps = 0 on v = 0: 0 / 0


@pytest.mark.parametrize('kind', ('eps_in_sqrt', 'powf'))
def test_g_mutants_fail(kind):
    tab = E.table_g()
    failed = [t for t in E.G_STEPS if not E.passes(E.judge_adam, 'mutant G %s t %d' % (kind, t), adam_mutant(kind, tab, t), E.adam_statement(tab, t))]
    assert failed, kind
    assert (1 if kind == 'eps_in_sqrt' else 2) in failed, (kind, failed)


def test_g_gate():
    tab = E.table_g()
    expected = {'kl == limit': 0, 'kl one ulp above': 1, 'kl NaN': 0, 'limit +inf': 0, 'limit -inf': 1, 'flag already set': 1}
    ge_differs = []
    for name, kl, limit, flag in E.gate_cases():
        want = E.adam_statement(tab, 3, gate_kl=kl, kl_limit=limit, stop=flag)
        assert want[4] == expected[name] and want[3] == (2 if expected[name] else 3), name
        if expected[name]:
            assert all(np.array_equal(a.view(np.int32), tab[k].view(np.int32)) for a, k in zip(want[:3], ('theta', 'm', 'v')))
        E.judge_adam('cpu G gate %s' % name, want, want)
        if not E.passes(E.judge_adam, 'mutant G gate >= %s' % name, adam_mutant('gate_ge', tab, 3, gate_kl=kl, kl_limit=limit, stop=flag), want):
            ge_differs.append(name)
    assert ge_differs == ['kl == limit']
