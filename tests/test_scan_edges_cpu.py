"""tests/scan_edges.py without a GPU: the references are fair (the NumPy restatements are the oracle's scans bit for bit, the oracle's
float32 scan sits inside the running bound around its float64 scan on every case), the case tables reach the partial counts, forms and
trips they are there for (from the restatement of the launchers' arithmetic), and the cases are not vacuous: each mutant, a NumPy variant
of the reference, breaks its group's assertion on the group's own inputs."""
import math

import numpy as np
import pytest

from tests import scan_edges as SE

F32, F64 = np.float32, np.float64


def _gae_args(T, n, mode):
    inp = SE.gae_inputs(T, n)
    return (inp['rew'], inp['val']) + SE.gae_mode_args(inp, mode)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def test_gae_table_covers_the_banks_lanes_and_end_bytes():
    assert {T for T, _ in SE.GAE_CASES} == {1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33}
    assert {n for _, n in SE.GAE_CASES} == {1, 2, 3, 63, 64, 65, 126, 128, 130}
    assert 18 <= len(SE.GAE_CASES) <= 24
    lanes = {(SE.gae_form(n), SE.ceil_div(n, SE.gae_form(n))) for _, n in SE.GAE_CASES}
    assert {(1, 63), (1, 65), (2, 63), (2, 64), (2, 65)} <= lanes and (1, 64) in {(SE.gae_form(n, 4), n) for _, n in SE.GAE_FORM_CASES}
    assert {SE.gamma_lam(k) for k in range(len(SE.GAE_CASES))} == set(SE.GAMMA_LAM)
    seen, at0, at_last, every, none, low, high = set(), 0, 0, 0, 0, 0, 0
    for T, n in SE.GAE_CASES:
        e = SE.gae_inputs(T, n)['end']
        seen |= set(np.unique(e).tolist())
        at0 += int(e[0].any()); at_last += int(e[T - 1].any())
        every += int((e != 0).all(0).any()); none += int((e == 0).all(0).any())
        ev, od = e[:, 0:n - n % 2:2], e[:, 1:n:2]
        low += int(((ev == 0x80) & (od == 0)).any()); high += int(((ev == 0) & (od == 0xFF)).any())
    assert seen == {0} | set(SE.END_BYTES)
    assert min(at0, at_last, every, none, low, high) >= 5, (at0, at_last, every, none, low, high)


def test_tables_give_the_partial_counts_forms_and_trips_they_name():
    for (T, n), parts, V in zip(SE.GAE_PARTIAL_CASES, SE.GAE_PARTIAL_COUNTS, SE.GAE_PARTIAL_FORMS):
        assert SE.gae_form(n) == V and SE.gae_partials(n, V) == parts, (T, n)
        assert SE.gae_partials(n, V) * 16 <= SE.gae_workspace_bytes(n)
    assert [SE.score_partials(n) for n in SE.SCORE_SUMMARY_N] == list(SE.SCORE_SUMMARY_PARTIALS) == [257, 513]
    assert SE.score_partials(65536) == 1024 and SE.gae_partials(65536, 2) == 512
    for T, n in SE.GAE_FORM_CASES:
        assert n % 2 == 0 and SE.gae_form(n) == 2 and SE.gae_form(n, float_offset=4) == 1 and SE.gae_form(n, end_offset=1) == 1
    g = SE.sum_geometry
    assert SE.reduce_grid(262149) == 257 and SE.reduce_grid(2097152) == 2048 == SE.reduce_grid(2097153) == SE.reduce_grid(400 * 65536)
    assert g(2097152)['vec_trips'] == 1 and g(2097153)['vec_trips'] == 1 and g(2097153)['tail_trips'] == 1
    assert g(4194311)['vec_trips'] == 3 and 4194311 - 4 * g(4194311)['nvec'] == 3
    assert g(400 * 65536)['vec_trips'] == 13
    for count in SE.SUM_COUNTS:
        assert g(count, 4)['nvec'] == 0 and g(count, 4)['tail_trips'] == SE.ceil_div(count, g(count)['stride'])
    assert g(262149, 4)['tail_trips'] == 4 and g(4194311, 4)['tail_trips'] == 9
    assert SE.k_sum(4194311) == 4 * 3 + 1 + 6 + 4 + 8 + 8 and SE.k_gae_stats(2, 32770, 2) == 4 + 6 + 2 + 8 and SE.k_score_summary(32832) == 1 + 6 + 3 + 8
    assert {c[2] for c in SE.SCORE_CASES} == set(SE.OBS_STRIDES) and {c[4] for c in SE.SCORE_CASES} == set(SE.ACT_STRIDES)
    assert {(c[2], c[3]) for c in SE.SCORE_CASES} == {(s, b) for s in SE.OBS_STRIDES for b in (False, True)}
    assert {(c[0], c[1]) for c in SE.SCORE_CASES} == {(T, n) for T in SE.SCORE_T for n in SE.SCORE_N}


# ---- GAE: the references are fair -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(SE.GAE_CASES)), ids=[SE.gae_case_id(c) for c in SE.GAE_CASES])
def test_gae_float32_oracle_sits_inside_the_bound_around_float64(k):
    """On every case and mode: the NumPy restatements are the oracle's two scans bit for bit, and the oracle's float32 scan differs from
    its float64 scan by no more than gae_f64_bound allows."""
    T, n = SE.GAE_CASES[k]
    gamma, lam = SE.gamma_lam(k)
    worst = 0.0
    for mode in SE.GAE_MODES:
        ref = SE.gae_reference(T, n, mode, gamma, lam)
        rew, val, end, boot, lv = _gae_args(T, n, mode)
        a32, r32 = SE.gae_scan(F32, rew, val, end, boot, lv, gamma, lam)
        assert np.array_equal(a32, ref['adv32']) and np.array_equal(r32, ref['ret32']), mode
        a64, r64, _, _ = SE.gae_f64_bound(rew, val, end, boot, lv, gamma, lam)
        assert np.array_equal(a64, ref['adv64']) and np.array_equal(r64, ref['ret64']), mode
        for got, want, bound in ((ref['adv32'], ref['adv64'], ref['badv']), (ref['ret32'], ref['ret64'], ref['bret'])):
            err = np.abs(got.astype(F64) - want)
            assert (err <= bound).all(), mode
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print('T %d n %d: float32 oracle at %.3f of the bound' % (T, n, worst))


def test_gae_bound_holds_on_long_random_blocks():
    """The prototype's statement, T up to 400, every (gamma, lam): a float32 scan stays inside the bound."""
    rng = np.random.RandomState(0)
    worst = 0.0
    for T, n in ((1, 3), (33, 130), (400, 50)):
        for gamma, lam in SE.GAMMA_LAM:
            rew, val = rng.randn(T, n).astype(F32), rng.randn(T, n).astype(F32)
            end = np.where(rng.rand(T, n) < 0.1, rng.choice(SE.END_BYTES, size=(T, n)), 0).astype(np.uint8)
            boot = (rng.randn(T, n) * (rng.rand(T, n) < 0.5)).astype(F32)
            a32, r32 = SE.gae_scan(F32, rew, val, end, boot, None, gamma, lam)
            a64, r64, ba, br = SE.gae_f64_bound(rew, val, end, boot, None, gamma, lam)
            ea, er = np.abs(a32.astype(F64) - a64), np.abs(r32.astype(F64) - r64)
            assert (ea <= ba).all() and (er <= br).all(), (T, n, gamma, lam)
            worst = max(worst, float((ea / np.maximum(ba, 1e-300)).max()), float((er / np.maximum(br, 1e-300)).max()))
    assert 0.05 < worst <= 1.0                       # not vacuous either: the scan uses a real share of it
    print('worst float32 error / bound %.3f' % worst)


# ---- GAE: the mutants -------------------------------------------------------------------------------------------------------------------
def _mutants_met(T, n, gamma):
    """Which mutants a case can tell from the scan.  With gamma = 0 nothing crosses a row (adv = r - v, ret = r), so no path end and no
    extra row shows; an end on the last row changes nothing (the path ends there anyway); a row 0 consumed twice shows only in a column
    whose path does not end at row 0 (an end resets the carry to the same values)."""
    end = SE.gae_inputs(T, n)['end']
    inner = end[:T - 1]
    return dict(eq1=bool(gamma != 0 and np.isin(inner, (2, 3, 5, 0x80, 0xFF)).any()),
                swap=bool(gamma != 0 and n % 2 == 0 and ((inner[:, 0::2] != 0) != (inner[:, 1::2] != 0)).any()),
                fewer=bool(T % SE.GAE_U != 0),
                more=bool(T % SE.GAE_U != 0 and T > 1 and gamma != 0 and (end[0] == 0).any()))


@pytest.mark.parametrize('k', range(len(SE.GAE_CASES)), ids=[SE.gae_case_id(c) for c in SE.GAE_CASES])
def test_gae_mutants_break_the_bit_for_bit_assertion(k):
    T, n = SE.GAE_CASES[k]
    gamma, lam = SE.gamma_lam(k)
    ref = SE.gae_reference(T, n, 'boot', gamma, lam)
    rew, val, end, boot, lv = _gae_args(T, n, 'boot')

    def same(**kw):
        a, r = SE.gae_scan(F32, rew, val, end, boot, lv, gamma, lam, **kw)
        return np.array_equal(a, ref['adv32']) and np.array_equal(r, ref['ret32'])

    assert same()
    met = _mutants_met(T, n, gamma)
    if met['eq1']:
        assert not same(end_rule='eq1')
    if met['swap']:
        assert not same(swap_pairs=True)
    if met['fewer']:
        assert not same(rows=-1)
    if met['more']:
        assert not same(rows=+1)
    if T == 1:                                           # row 0 is the last row: consumed twice it gives the same values, counted twice
        (s1, s1abs), _ = SE.gae_stats_reference(ref['adv32'])
        assert abs(s1) > SE.sum_bound(SE.k_gae_stats(T, n, SE.gae_form(n)), s1abs)         # the mutant's sum is 2 s1


def test_gae_mutants_are_met_by_the_table():
    hit = dict(eq1=0, swap=0, more=0, fewer=0)
    for k, (T, n) in enumerate(SE.GAE_CASES):
        for name, met in _mutants_met(T, n, SE.gamma_lam(k)[0]).items():
            hit[name] += int(met)
    assert min(hit.values()) >= 6, hit


@pytest.mark.parametrize('k', range(len(SE.GAE_PARTIAL_CASES)), ids=[SE.gae_case_id(c) for c in SE.GAE_PARTIAL_CASES])
def test_a_fold_that_stops_after_256_partials_breaks_the_statistics(k):
    T, n = SE.GAE_PARTIAL_CASES[k]
    V = SE.gae_form(n)
    adv = SE.gae_reference(T, n, 'boot', 0.99, 0.97)['adv32']
    (s1, s1abs), (s2, _) = SE.gae_stats_reference(adv)
    parts = SE.gae_block_partials(adv, V)
    K = SE.k_gae_stats(T, n, V)
    for j, (want, scale) in enumerate(((s1, s1abs), (s2, s2))):
        p = [q[j] for q in parts]
        assert abs(SE.fold_model(p) - want) <= SE.sum_bound(K, scale)
        assert abs(SE.fold_model(p, limit=256) - want) > SE.sum_bound(K, scale), (T, n, j)


# ---- sums and apply -------------------------------------------------------------------------------------------------------------------
def test_a_grid_stride_loop_of_one_trip_breaks_the_sums():
    for count, offset in ((4194311, 0), (4194311, 4), (2097153, 4), (262149, 4), (1025, 4)):
        x = SE.sum_block('offset', count)
        ref = SE.sum_reference('offset', count)
        bound = SE.sum_bound(SE.k_sum(count, offset), ref['s1abs']) + SE.U * abs(ref['s1'])
        assert abs(SE.sum_model(x, offset) - ref['s1']) <= bound
        assert abs(SE.sum_model(x, offset, one_trip=True) - ref['s1']) > bound, (count, offset)
    for count in (2097152, 2097153):                                   # one trip of the float4 loop is all there is: the mutant is the kernel
        assert SE.sum_model(SE.sum_block('offset', count), 0, one_trip=True) == SE.sum_reference('offset', count)['s1']


def test_epsilon_1e_6_breaks_the_normalisation_bound():
    """Three-pass form on the offset block (std 0.01: 1e-6 against it is 1e-4 relative, the bound 3 u) and one-pass form on the
    advantages of a partial-count case (std of order 1, no offset for the cast of the mean to hide behind)."""
    count = 1025
    x, ref = SE.sum_block('offset', count), SE.sum_reference('offset', count)
    assert 0.005 < float(ref['std']) < 0.02 and abs(float(ref['mean']) - 1000.0) < 0.01
    y, bound = SE.norm_reference(x, mean=ref['mean'], std=ref['std'])
    mut, _ = SE.norm_reference(x, mean=ref['mean'], std=ref['std'], eps=F32(1e-6))
    own = ((x - ref['mean']) * (F32(1.0) / (ref['std'] + SE.EPS))).astype(F64)       # the kernel's own f32 order sits inside
    assert (np.abs(own - y) <= bound).all() and (np.abs(mut - y) > bound).mean() > 0.9
    T, n = SE.GAE_PARTIAL_CASES[1]
    adv = SE.gae_reference(T, n, 'boot', 0.99, 0.97)['adv32']
    (s1, s1abs), (s2, _) = SE.gae_stats_reference(adv)
    kw = dict(stats=(s1, s2), total=adv.size, K=SE.k_gae_stats(T, n, 1), s1abs=s1abs)
    y, bound = SE.norm_reference(adv.ravel(), **kw)
    mut, _ = SE.norm_reference(adv.ravel(), eps=F32(1e-6), **kw)
    assert (np.abs(mut - y) > bound).mean() > 0.5
    assert abs(float(y.mean())) < 1e-6 and abs(float(y.std()) - 1.0) < 1e-6


def test_constant_block_normalises_to_positive_zero():
    x, ref = SE.sum_block('const', 1025), SE.sum_reference('const', 1025)
    assert ref['mean'] == F32(1.5) and ref['std'] == F32(0.0) and ref['s2'] == 2.25 * 1025
    y, bound = SE.norm_reference(x, stats=(ref['s1'], ref['s2']), total=1025)
    assert not y.any() and not np.signbit(y).any()


# ---- score card -----------------------------------------------------------------------------------------------------------------------
def test_score_statement_against_evaluates_float64_functions():
    """The NumPy statement of the per-row update is the score the project's float64 evaluation gives, to float32 accuracy: 1e-6 relative
    on single-signed sums (the yardstick and the tolerance of tests/test_gpu_score.py)."""
    import torch
    from ml4ca_amd import evaluate as EV
    T, n = 5, 65
    r = SE.score_rows(T, n, 9, 7)
    act = np.abs(r['act']) * np.where(np.arange(n)[None, :, None] % 2 == 0, 1.0, -1.0).astype(F32)
    st = SE.score_update(SE.score_fresh(n), dict(obs=r['obs'], integ=r['integ'], act=act, rew=r['rew']), SE.score_consts())
    got = SE.score_read(st)
    e = torch.from_numpy(r['obs'][..., :3].astype(F64) - r['integ'].astype(F64))
    e = torch.stack([e[..., 0], e[..., 1], torch.rad2deg(e[..., 2])], dim=-1)
    dt = float(F32(0.2))
    _, cum = EV.iae_series(e, torch.zeros_like(e), torch.arange(T, dtype=torch.float64) * dt)
    work = EV.work(EV.commanded_thrust(torch.from_numpy(act.astype(F64))), dt)
    assert np.abs(got[0] - cum[-1].numpy()).max() <= 1e-6 * np.abs(cum[-1].numpy()).max()
    assert (np.abs(got[1:4].T - work.numpy()) <= 1e-6 * np.abs(work.numpy())).all()
    assert np.array_equal(got[4], np.cumsum(r['rew'].astype(F64), 0)[-1]) and (got[5] == T).all() and not got[6:].any()


@pytest.mark.parametrize('T', [1, 3, 5])
def test_score_mutants_break_the_bit_for_bit_assertion(T):
    n = 65
    r = SE.score_rows(T, n, 9, 7)
    consts = SE.score_consts()
    for kind in SE.DONE_PATTERNS:
        blk = dict(r, done=SE.done_pattern(kind, T, n))
        want = SE.score_read(SE.score_update(SE.score_fresh(n), blk, consts))
        again = SE.score_read(SE.score_update(SE.score_fresh(n), blk, consts))
        assert np.array_equal(want, again)
        assert T % SE.SCORE_U == 1
        for rows in (+1, -1):
            assert not np.array_equal(SE.score_read(SE.score_update(SE.score_fresh(n), blk, consts, rows=rows)), want), (kind, rows)
        for piece in (1, 2):                                            # the statement itself carries across pieces
            st = SE.score_fresh(n)
            for t0, t1 in SE.score_pieces(T, piece):
                SE.score_update(st, SE.slice_block(blk, t0, t1), consts)
            assert np.array_equal(SE.score_read(st), want), (kind, piece)


def test_bf16_round_is_torchs():
    import torch
    x = SE.score_rows(5, 65, 12, 7)['obs']
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).float().numpy()
    assert np.array_equal(SE.bf16_round(x), want) and not np.array_equal(want, x)


@pytest.mark.parametrize('n', SE.SCORE_SUMMARY_N)
def test_summary_cases_and_mutants(n):
    """Every env its own values, the minimum of the open iae and the maximum of the open (negative) return on env n-1; a neutral element of
    0 and a fold that stops after 256 partials each break the summary's assertions."""
    r = SE.summary_rows(n)
    consts = SE.score_consts()
    st = SE.score_update(SE.score_fresh(n), r, consts, cut_at_end=True)
    got = SE.score_read(SE.score_update(st, r, consts))
    K = SE.k_score_summary(n)
    names = SE.SCORE_SLOTS
    for slot in ('iae', 'work0', 'work1', 'work2', 'ret', 'ep_iae', 'ep_work0', 'ep_work1', 'ep_work2', 'ep_ret'):
        v = got[names.index(slot)]
        assert np.unique(v).size == n, slot
        tot, tot_abs = SE.fsum_terms(v)
        s, lo, hi = SE.summary_model(v)
        assert (lo, hi) == (v.min(), v.max()) and abs(s - tot) <= SE.sum_bound(K, tot_abs)
        s, lo, hi = SE.summary_model(v, limit=256)
        assert abs(s - tot) > SE.sum_bound(K, tot_abs), slot
        _, lo0, hi0 = SE.summary_model(v, neutral_zero=True)
        assert (lo0, hi0) != (v.min(), v.max()), slot
    iae, ret = got[names.index('iae')], got[names.index('ret')]
    assert int(iae.argmin()) == n - 1 and int(ret.argmax()) == n - 1 and ret.max() < 0 and iae.min() > 0
    for slot, fn in (('iae', 'min'), ('ret', 'max')):                   # the ragged last wave is where they sit: the short fold loses them
        v = got[names.index(slot)]
        _, lo, hi = SE.summary_model(v, limit=256)
        assert (lo if fn == 'min' else hi) != (v.min() if fn == 'min' else v.max())
