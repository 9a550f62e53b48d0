"""Are the cases of tests/policy_edges.py fair, and does the DOCUMENTED arithmetic of the in-kernel networks hold its contract on them?
(CPU only: split_model, float64 and torch float32 - no kernel runs here.)  These are the conditions tests/test_gpu_policy_edges.py leans on.
The measured figures are printed, and appended to the file the environment variable POLICY_EDGES_RECORD names, if it is set."""
import os
import re

import numpy as np
import pytest

from tests import policy_edges as PE

RECORD = os.environ.get('POLICY_EDGES_RECORD', '')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_ACT = [(c, a) for c in PE.CASES for a in PE.ACTIVATIONS]


@pytest.mark.parametrize('case,activation', [(c, a) for c, a in CASE_ACT if c != 'overflow'])
def test_documented_arithmetic_meets_the_contract_in_its_domain(case, activation):
    """|split_model - ref64| <= C max(S, 1) per output tensor wherever domain() says so (C = 1e-5 for F32, include/dpenv.h; 2e-3 for F16,
    tests/test_gpu_policy.py), float64 and float32 are finite, and torch float32 itself is well inside the F32 constant."""
    ev = PE.evaluate(case, activation)
    assert ev['obs'].shape == (PE.N_ROWS, PE.OBS_DIM) and ev['obs'].dtype == np.float32
    for j, name in enumerate(('mu', 'v')):
        ref = ev['ref'][j]
        S = PE.scale_of(ref)
        assert np.isfinite(ref).all() and np.isfinite(ev['y32'][j]).all()
        e32 = PE.err(ev['y32'][j], ref)
        assert e32 <= 0.5 * PE.C['f32'] * S                 # the fp32 evaluation the header measures against, against the yardstick
        for prec in ('f16', 'f32'):
            e = PE.err(ev['model'][prec][j], ref)
            ok = PE.domain(case, activation, prec)
            PE.record(RECORD, 'model  %-9s %-5s %-3s %-2s model %.3e  y32 %.3e  C*S %.3e  S %.4g  %s' % (
                case, activation, prec, name, e, e32, PE.C[prec] * S, S, 'in domain' if ok else 'OUTSIDE'))
            if ok:
                assert e <= PE.C[prec] * S, (case, activation, prec, name, e / S)


JITTER = (1.0, 0.93, 0.81, 0.71, 0.62, 0.55)            # scalings that are no power of two: other mantissas, other roundings


def _tanh_worst(wscale, precision, growths):
    """worst |split_model - ref64| / max(S, 1) over mu and v with tanh, on the nominal draw rescaled so that growth_of() is each of `growths`
    (skipped where the weights alone exceed it; None = the rows as drawn); also whether in_domain() holds at every one of them / at none"""
    p, base = PE.params('tanh', wscale), PE.nominal_obs()
    worst, inside = 0.0, []
    for g in growths:
        if g is None:                                       # the nominal rows as drawn: growth = the weight scale alone
            obs = base
        else:
            top = PE.NOMINAL_OBS * g / PE.weight_scale(p)
            if top < PE.NOMINAL_OBS:
                continue
            obs = (base * np.float32(top / np.abs(base).max())).astype(np.float32)
            assert abs(PE.growth_of(p, obs) / g - 1.0) < 1e-6
        inside.append(PE.in_domain(p, obs, 'tanh', precision))
        ref = PE.ref64(p, obs, 'tanh')
        m = PE.split_model(p, obs, 'tanh', PE.LEAK['tanh'], precision)
        worst = max(worst, max(PE.err(m[j], ref[j]) / PE.scale_of(ref[j]) for j in (0, 1)))
    return worst, inside


@pytest.mark.parametrize('precision', ['f32', 'f16'])
@pytest.mark.parametrize('wscale', [1.0, 2.0, 4.0])
def test_tanh_growth_limit_holds_just_inside_and_the_contract_breaks_beyond(wscale, precision):
    """The tanh limit of include/dpenv.h, growth = max(1, max|obs| / 16) x weight scale, evaluated as stated - growth_of() on the actual rows and
    kernels - at weights x 1, x 2 and x 4.  Just inside (growth = 0.999 of the limit, and 0.93 ... 0.55 of it): in_domain() holds and the documented
    arithmetic meets C with a factor 2 to spare.  Beyond (32 x the limit for F32, 16 x for F16, and the same fractions of it): in_domain() does
    not hold, and the documented arithmetic misses C - the limit is conservative, but what it excludes does break the contract."""
    lim = PE.TANH_GROWTH_LIMIT[precision]
    if wscale <= lim:
        worst, inside = _tanh_worst(wscale, precision, [None] + [lim * j for j in (0.999,) + JITTER[1:]])
        PE.record(RECORD, 'tanh   weights x %g %-3s at growth <= %-4g model %.3e  C %.0e' % (wscale, precision, lim, worst, PE.C[precision]))
        assert inside and all(inside) and worst <= 0.5 * PE.C[precision]
    else:
        # the weights alone are past the limit: already the nominal rows are outside
        assert not PE.in_domain(PE.params('tanh', wscale), PE.nominal_obs(), 'tanh', precision)
    far = lim * (32.0 if precision == 'f32' else 16.0)
    worst, inside = _tanh_worst(wscale, precision, [far * j for j in JITTER])
    PE.record(RECORD, 'tanh   weights x %g %-3s at growth ~  %-4g model %.3e  C %.0e' % (wscale, precision, far, worst, PE.C[precision]))
    assert inside and not any(inside) and worst > PE.C[precision]


def test_domain_of_the_cases_is_the_stated_formula():
    """domain() is in_domain() of the case's own rows and kernels, nothing per case: growth 1 for `nominal`, `zero`, `tiny`; max|obs| / 16 for
    `far`; twice that for `far_heavy`; 4 for `heavy`.  Leaky-relu and relu are inside everywhere below the overflow, nothing is inside in it."""
    top = float(np.abs(PE.case_obs('far')).max())
    want = {'nominal': 1.0, 'zero': 1.0, 'tiny': 1.0, 'far': top / 16.0, 'far_heavy': 2.0 * top / 16.0, 'heavy': 4.0}
    for case, g in want.items():
        got = PE.growth_of(PE.case_params(case, 'tanh'), PE.case_obs(case))
        assert abs(got / g - 1.0) < 1e-3, (case, got, g)
        for prec in ('f16', 'f32'):
            assert PE.domain(case, 'leaky', prec) and PE.domain(case, 'relu', prec)
            assert PE.domain(case, 'tanh', prec) == (got <= PE.TANH_GROWTH_LIMIT[prec]), (case, prec)
        assert PE.domain(case, 'tanh', 'f32_actor') == (PE.domain(case, 'tanh', 'f16') and PE.domain(case, 'tanh', 'f32'))
    assert PE.TANH_GROWTH_LIMIT == {'f32': 32.0, 'f16': 2.0} and PE.NOMINAL_OBS == 16.0 and PE.HIDDEN_LIMIT == 2.0 ** 15
    assert not any(PE.domain('overflow', a, prec) for a in PE.ACTIVATIONS for prec in PE.PRECISIONS)


@pytest.mark.parametrize('case,activation', [(c, a) for c, a in CASE_ACT if c != 'overflow'])
def test_inputs_and_hidden_values_stay_below_2_15(case, activation):
    """Every number the networks convert to f16 - observations, and the hidden values of both networks in float64 and in both modelled
    arithmetics - is below 2^15 in every case but `overflow`: a factor 2 from f16's largest number."""
    ev = PE.evaluate(case, activation)
    top = float(np.abs(ev['obs']).max())
    for scope in ('pi', 'v'):
        top = max(top, max(float(np.abs(z).max()) for z in PE.hidden64(ev['params'], ev['obs'], activation, scope)))
        for prec in ('f16', 'f32'):
            hs = ev['hidden'][prec][scope]
            assert all(np.isfinite(h).all() for h in hs)
            top = max(top, max(float(np.abs(h).max()) for h in hs))
    PE.record(RECORD, 'range  %-9s %-5s largest input / hidden magnitude %.4g' % (case, activation, top))
    assert top < PE.HIDDEN_LIMIT


@pytest.mark.parametrize('activation', PE.ACTIVATIONS)
def test_overflow_rows_are_far_past_f16_and_the_rest_far_below(activation):
    """`overflow`: each of the six poisoned rows holds an input that f16 turns into inf - an exact conversion of a float32 value, 2.5 % or
    more past the threshold 65 520, so no summation order decides it - and with it a first-layer hidden value that is no number below
    2^17 (inf or NaN) in the modelled arithmetics; every input of every row is away from that threshold; the clean rows stay below 2^15
    throughout; float64 and float32 are finite on all 97 rows (fp32 does not overflow there)."""
    ev = PE.evaluate('overflow', activation)
    obs, bad = ev['obs'], list(PE.POISONED)
    clean = np.setdiff1d(np.arange(PE.N_ROWS), bad)
    assert (np.abs(obs[bad]).max(1) >= 65520.0 * 1.025).all()
    a = np.abs(obs)
    assert not ((a > PE.F16_MAX * (1 - 2.0 ** -6)) & (a < 65520.0 * 1.025)).any()
    assert np.array_equal(obs[clean], PE.case_obs('nominal')[clean])
    for j in (0, 1):
        assert np.isfinite(ev['ref'][j]).all() and np.isfinite(ev['y32'][j]).all()
    for scope in ('pi', 'v'):
        for z in PE.hidden64(ev['params'], obs[clean], activation, scope):
            assert float(np.abs(z).max()) < PE.HIDDEN_LIMIT
        for prec in ('f16', 'f32'):
            hs = ev['hidden'][prec][scope]
            with np.errstate(invalid='ignore'):                 # the modelled first-layer accumulator (tanh then squashes inf to +-1)
                assert (~(np.abs(ev['hidden'][prec][scope + '_z'][0][bad]) <= 2.0 ** 17)).any(1).all()
            assert all(float(np.abs(h[clean]).max()) < PE.HIDDEN_LIMIT for h in hs)
    for prec in ('f16', 'f32'):
        mu, v = ev['model'][prec]
        assert np.isfinite(mu[clean]).all() and np.isfinite(v[clean]).all()
        if activation == 'tanh' and prec == 'f16':
            # f16(x) = +-inf goes through tanh as +-1: finite rows that have nothing to do with float64's
            assert np.isfinite(mu[bad]).all() and PE.err(mu[bad], ev['ref'][0][bad]) > 0.05
        else:
            assert not np.isfinite(mu[bad]).any() and not np.isfinite(v[bad]).any()
        PE.record(RECORD, 'overflow %-5s %-3s poisoned rows finite: mu %d of 42, v %d of 6' % (
            activation, prec, int(np.isfinite(mu[bad]).sum()), int(np.isfinite(v[bad]).sum())))


@pytest.mark.parametrize('case', PE.RANGE_CASES)
@pytest.mark.parametrize('activation', ['leaky', 'relu'])
def test_a_hidden_unit_on_the_other_branch_moves_no_output_past_the_bound(case, activation):
    """A float32 or f16 evaluation may put a hidden unit on the other branch of the leaky-relu than float64 does.  The activation is
    CONTINUOUS, so such a unit's pre-activation is within the evaluation's own error of zero and the other branch changes its value by
    no more than that error: no margin from the kink is needed and no row is masked.  Checked instead: every unit that the modelled
    arithmetic does put on the other branch is flipped, one at a time, in the float64 evaluation, and no output moves by more than
    C max(S, 1)."""
    ev = PE.evaluate(case, activation)
    p, obs = ev['params'], ev['obs']
    lk = 0.0 if activation == 'relu' else float(np.float32(PE.LEAK[activation]))
    flips, worst = 0, 0.0
    for j, scope in enumerate(('pi', 'v')):
        Ws, bs = PE.net_layers(p, scope)
        zs = PE.hidden64(p, obs, activation, scope)
        ref = ev['ref'][j].reshape(PE.N_ROWS, -1)
        for prec in ('f16', 'f32'):
            bound = PE.C[prec] * PE.scale_of(ref)
            for l, z in enumerate(zs):
                other = (ev['hidden'][prec][scope][l] > 0) != (z > 0)
                for i, u in zip(*np.nonzero(other)):
                    flips += 1
                    x = np.where(z[i] > 0, z[i], lk * z[i])
                    x[u] = lk * z[i, u] if z[i, u] > 0 else z[i, u]
                    for W, b in zip(Ws[l + 1:-1], bs[l + 1:-1]):
                        zz = x @ W.astype(np.float64) + b
                        x = np.where(zz > 0, zz, lk * zz)
                    out = x @ Ws[-1].astype(np.float64) + bs[-1]
                    d = float(np.abs(out - ref[i]).max())
                    worst = max(worst, d / bound)
                    assert d <= bound, (case, activation, scope, prec, l, i, u, z[i, u], d, bound)
    PE.record(RECORD, 'flip   %-9s %-5s units on the other branch %d, worst output change / bound %.3g' % (case, activation, flips, worst))


def test_the_noise_block_of_the_log_std_test_holds_its_edges():
    xi = PE.ends_noise(3, PE.N_ROWS)
    assert xi.dtype == np.float32 and (xi[:, 0] == 0).all() and (xi[:, :, 3] == 0).all()
    assert (xi == 5).any() and (xi == -5).any() and 0.8 < xi[:, 3:, [0, 1, 2, 4, 5, 6]].std() < 1.2
    assert min(PE.LOG_STD_ENDS) == -4.0 and max(PE.LOG_STD_ENDS) == 1.0          # the clamp of examples/train_ppo.py
    src = open(os.path.join(ROOT, 'examples', 'train_ppo.py')).read()
    assert re.search(r'clamp_?\(\s*-4(\.0)?\s*,\s*1(\.0)?\s*\)', src)
