"""What tests/test_gpu_control_edges.py leans on, proven without a GPU (tests/control_edges.py holds tables, truths and bounds): the float32
host law is inside every bound on every row with a float64 claim, the kink rule is used by exactly the tagged rows, the physical
statement holds, the tables have teeth (the host law with one seeded error fails the judge), the host statement's clips are the stated
fminf(fmaxf()) - a NaN is dropped, in label_rows and behind it -, and the reference filter's f64 coefficient recipe is within its
measured distance of a 60-digit matrix exponential."""
import os

import numpy as np
import pytest

from tests import control_edges as CE

RECORD = os.environ.get('CONTROL_EDGES_RECORD', '')
F32, F64 = np.float32, np.float64
F_EPS = (1e-6, 0.0)


# A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f_eps', F_EPS)
def test_allocation_host_law_is_inside_every_bound(f_eps):
    tau, kink, names = CE.alloc_cases(f_eps)
    p = CE.params(f_eps)
    got = CE.host_alloc(p, tau)
    res = CE.judge_alloc(f_eps, got)
    CE.report(RECORD, 'A host f32, f_eps %g' % f_eps, res)
    assert res['ok'].all(), [names[i] for i in np.flatnonzero(~res['ok'])]
    tr = CE.alloc_truth(p, tau)
    assert np.isfinite(tr['bound'][tr['domain']]).all()                                # a bound that is not finite would pass anything
    # the kink rule: used by exactly the tagged rows, and only this table (f_eps > 0) has any
    assert int(res['used_kink'].sum()) == int(kink.sum()) == (21 if f_eps > 0 else 0)
    assert np.array_equal(res['used_kink'], kink)
    # both sides of every kind of row are there
    dom = res['domain']
    assert dom.sum() >= 60 and (~dom).sum() >= 60
    assert (np.abs(got[dom, 0]) == 1).any() and (got[dom, 1] == 1).any() and (got[dom, 2] == 1).any()
    assert ((got[dom, 3] == 0) & (got[dom, 4] == 1)).any() and (got[dom, 0] < 0).any() and (got[dom, 0] > 0).any()


@pytest.mark.parametrize('f_eps', F_EPS)
def test_allocation_decodes_to_the_wrench(f_eps):
    tau, kink, names = CE.alloc_cases(f_eps)
    p = CE.params(f_eps)
    tr = CE.alloc_truth(p, tau)
    rows, ratio = CE.judge_decode(p, tau, tr, CE.host_alloc(p, tau), kink)
    CE.record(RECORD, 'A decode, f_eps %g: %d rows, worst error / bound %s' % (f_eps, rows.sum(), ratio.max(0)))
    assert rows.sum() >= 30 and (ratio <= 1).all(), [names[i] for i in np.flatnonzero((ratio > 1).any(1))]
    # the float64 law itself decodes to tau to 1e-6 relative (G is an f32 rounding of the pseudo-inverse)
    t64, _ = CE.decode(p, tr['act'])
    assert (np.abs(t64 - tau)[rows] <= 1e-6 * np.abs(tau[rows]).max(1, keepdims=True)).all()


def test_outside_the_domain_the_heads_are_what_the_header_says():
    """|f| from 1.3e19: F = inf, heads (+-0, +-0) or NaN; squares that underflow to 0: F = 0, heads (0, 1)."""
    p = CE.params(0.0)
    with np.errstate(all='ignore'):
        a = CE.host_alloc(p, np.array([[0, 1e20, 0], [0, 1e-25, 0], [0, np.nan, 0]], F32))
    assert (a[0, 3:7] == 0).all() and a[0, 1] == 1 and a[0, 2] == 1
    assert np.array_equal(a[1, 3:7], F32([0, 1, 0, 1]))
    assert np.array_equal(a[2], F32([-1, 1, 1, 0, 1, 0, 1]))                            # a NaN wrench: every clip drops it


def _flip_G42(c):
    c.G = c.G.copy()
    c.G[..., 4, 2] = -c.G[..., 4, 2]


def _kr_is_kf0(c):
    c.kr_bow = c.kf[..., 0]


def _ge_at_f_eps(c):
    c.f_eps = np.nextafter(c.f_eps, F32(-np.inf))                                      # F > pred(f_eps) is F >= f_eps


def _swap_clip(c):
    c.zb = -c.zb                                                                       # fmin(fmax(v, zb), -zb)


@pytest.mark.parametrize('mutate', [_flip_G42, _kr_is_kf0, _ge_at_f_eps], ids=['G42_sign', 'kr_bow_is_kf0', 'ge_at_f_eps'])
def test_allocation_table_has_teeth(mutate):
    """`>=` at f_eps cannot be caught at f_eps > 0: F32 == f_eps only on kink rows, where either branch passes by the rule.  It is caught by
    the row tau = 0 of the f_eps = 0 table alone (dF = 0: the law is decided, and `>=` answers 0 / 0)."""
    caught = 0
    for f_eps in F_EPS:
        tau, _, _ = CE.alloc_cases(f_eps)
        res = CE.judge_alloc(f_eps, CE.host_alloc(CE.params(f_eps), tau, mutate=mutate))
        caught += int((~res['ok'] & res['domain']).sum())
    assert caught > 0


# B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_pid_host_law_is_inside_every_bound(bf16):
    case = CE.pid_cases(bf16)
    act, z = CE.pid_host32(case)
    res = CE.judge_pid(case, act, z)
    CE.record(RECORD, 'B host f32 %s: %d rows with a float64 claim, %d without; worst error / bound %s, z %.3g' % (
        'bf16' if bf16 else 'f32', res['domain'].sum(), (~res['domain']).sum(), res['ratio'].max((0, 1)), res['z_ratio'].max()))
    assert res['ok'].all() and res['z_ok'].all(), [case['names'].get(i, i) for i in np.flatnonzero(~res['ok'].all(0) | ~res['z_ok'])]
    assert res['domain'][:, list(CE.NEIGHBOURS)].all() and res['demoted'] == 0
    if not bf16:
        tr = CE.pid_truth(case)
        assert (~tr['claim']).sum() == 18 * 5 + 4 and (~tr['z_claim']).sum() == 18          # a done row ends the spell
        p = CE.params()
        assert (np.abs(tr['z']) == p['z_bound'][:, None]).any() and (np.abs(tr['tau']) == p['tau_max']).any()


@pytest.mark.parametrize('f_eps', F_EPS)
def test_allocation_as_a_labelling_block_is_inside_every_bound(f_eps):
    case = CE.alloc_label_case(f_eps)
    act, z = CE.pid_host32(case)
    res = CE.judge_pid(case, act, z)
    CE.record(RECORD, 'A as labelling block, host f32, f_eps %g: %d rows with a float64 claim, %d without, %d kink rows; worst error / bound %s' % (
        f_eps, res['domain'].sum(), (~res['domain']).sum(), res['used_kink'].sum(), res['ratio'].max((0, 1))))
    assert res['ok'].all() and res['z_ok'].all()
    assert int(res['used_kink'].sum()) == int(case['kink'].sum()) and res['demoted'] == 0
    for mutate in (_flip_G42, _kr_is_kf0, _ge_at_f_eps):
        bad = CE.judge_pid(case, *CE.pid_host32(case, mutate=mutate))
        assert f_eps > 0 and mutate is _ge_at_f_eps or (~bad['ok'] & bad['domain']).any(), mutate.__name__


def test_pid_table_has_teeth():
    case = CE.pid_cases()
    act, z = CE.pid_host32(case, mutate=_swap_clip)
    res = CE.judge_pid(case, act, z)
    assert (~res['ok'] & res['domain']).any() and not res['z_ok'].all()


def test_a_nan_row_is_dropped_by_every_clip_and_the_scan_carries_on():
    """The host statement at a NaN: z_j = -z_bound_j, tau_j = -tau_max_j, finite rows behind it - what the device's stated law does."""
    from ml4ca_amd.deploy import label_rows, label_rows_nn
    p = CE.params()
    obs = np.zeros((4, 2, 9), F32)
    obs[..., 0:6] = 0.125
    obs[1, 0, 0] = np.nan
    act, z = label_rows(p, obs, dt=CE.DT)
    assert np.isfinite(act).all() and np.isfinite(z).all()
    step = CE.DT * F32(0.125)
    assert z[0, 0] == (F32(-p['z_bound'][0]) + step) + step and z[0, 1] == ((step + step) + step) + step
    from ml4ca_amd.deploy import BatchedDPController
    c = BatchedDPController(1, p, dt=CE.DT)
    tau = c.wrench(np.array([[np.nan, 0, 0, 0, 0, 0]], F32))
    assert tau[0, 0] == -F32(p['tau_max'][0]) and c.z[0, 0] == -F32(p['z_bound'][0])
    # the network scan says NaN again in tau (the rest rule answers the row); z stays the law's, so the rows behind are the law's
    rng = np.random.RandomState(0)
    net = ([rng.normal(0, 0.3, (9, 8)), rng.normal(0, 0.3, (8, 6))], [np.zeros(8), np.zeros(6)])
    a_nn, z_nn, raw, tau_nn = label_rows_nn(p, net, obs, dt=CE.DT)
    assert np.isnan(tau_nn[1, 0, 0]) and np.isfinite(tau_nn[2:]).all() and np.isfinite(tau_nn[1, 0, 1:]).all()
    assert np.array_equal(z_nn, z)


def test_torch_and_numpy_host_laws_agree_at_a_nan():
    import torch
    from ml4ca_amd.deploy import BatchedDPController
    p = CE.params()
    o = np.array([[np.nan, 1, -1, 0.5, np.inf, -np.inf], [0.1, np.nan, 0.2, np.nan, 0.3, 0.4]], F32)
    a, b = BatchedDPController(2, p, dt=CE.DT), BatchedDPController(2, p, dt=CE.DT, dtype=torch.float32)
    with np.errstate(all='ignore'):
        x, y = a.act(o), b.act(torch.from_numpy(o)).numpy()
    assert CE.bits_equal(x, y).all() and CE.bits_equal(a.z, b.z.numpy()).all()


# D ---------------------------------------------------------------------------------------------------------------------------------
def test_integral_host_law_against_its_float64_form():
    import torch
    case = CE.integral_cases()
    I, c = CE.integral_run(case, torch.float32)
    ok, worst = CE.judge_integral(case, I, c)
    CE.record(RECORD, 'D host f32: %d lanes, D = %d, worst error / bound %.3g' % (len(ok), case['D'], worst))
    assert ok.all(), [case['names'][i] for i in np.flatnonzero(~ok)]
    # every branch happened: a reset on a beyond-the-box row and none at the box, I at both bounds, a count that grows to D
    names = case['names']
    beyond = np.array(['beyond' in s for s in names])
    at = np.array(['at the box' in s for s in names])
    assert (c[5, beyond] == 0).all() and (I[5, beyond] == 0).all() and (c[5, at] == case['D']).all() and (I[5, at] != 0).any()
    assert (np.abs(I) == F32(CE.IA['bound'])).any()


def test_tie_to_even_in_the_heading_switch():
    """rintf and torch.round both tie to even: the switch's wrap at d = +-pi_f and +-3 pi_f."""
    import torch
    half = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5])
    assert torch.equal(torch.round(half), torch.tensor([0.0, 2.0, 2.0, -0.0, -2.0, -2.0]))
    assert np.array_equal(np.rint(half.numpy()), torch.round(half).numpy())


def _dwell_gt(law):
    law.dwell = law.dwell + 1                                                          # c >= D + 1 is c > D (the cap moves with it)


def _box_ge(law):
    import torch
    law.box = torch.nextafter(law.box, torch.full_like(law.box, -np.inf))              # |e| > pred(box) is |e| >= box


@pytest.mark.parametrize('mutate', [_dwell_gt, _box_ge], ids=['dwell_gt', 'box_ge'])
def test_integral_table_has_teeth(mutate):
    import torch
    case = CE.integral_cases()
    I, c = CE.integral_run(case, torch.float32, mutate=mutate)
    ok, _ = CE.judge_integral(case, I, c)
    assert not ok.all()


# E ---------------------------------------------------------------------------------------------------------------------------------
def test_reference_filter_coefficients_against_60_digits():
    from ml4ca_amd.deploy import reference_filter_coeffs, reference_filter_coeffs_f64
    a_worst, worst32 = {}, 0.0
    for w, z in CE.coeff_table():
        w32, z32, dt = float(F32(w)), float(F32(z)), float(CE.DT)
        tp, tg = CE.coeff_truth(w, z)
        p64, g64 = reference_filter_coeffs_f64((w32,) * 3, (z32,) * 3, dt)
        a = max(np.abs(p64[0] - tp).max(), np.abs(g64[0] - tg).max())
        a_worst[w] = max(a_worst.get(w, 0.0), a)
        allow = 4 * CE.COEFF_A_MEASURED[w]
        CE.record(RECORD, 'E omega %-6g zeta %-5g f64 recipe abs err %.3g' % (w, z, a))
        p32, g32 = reference_filter_coeffs((w32,) * 3, (z32,) * 3, dt)
        assert p32.dtype == F32
        for got, want in ((p32[j], tp) for j in range(3)):
            r = np.abs(got.astype(F64) - want) / (CE.U * np.abs(want) + allow)
            worst32 = max(worst32, r.max())
            assert (r <= 1).all(), (w, z)
        for j in range(3):
            r = np.abs(g32[j].astype(F64) - tg) / (CE.U * np.abs(tg) + allow)
            worst32 = max(worst32, r.max())
            assert (r <= 1).all(), (w, z)
    CE.record(RECORD, 'E f64 recipe: largest abs err per omega %s (recorded %s); f32 coefficients worst error / bound %.3g' % (
        {w: '%.2g' % a for w, a in a_worst.items()}, CE.COEFF_A_MEASURED, worst32))
    for w, a in a_worst.items():
        assert a <= 4 * CE.COEFF_A_MEASURED[w], (w, a)


def test_reference_filter_switch_and_advance_at_the_edges():
    """deploy.BatchedReferenceFilter in f32 (the kernels' reff_target / reff_advance) on the rows of control_edges.reff_cases against
    float64: the turn taken at +-pi_f and +-3 pi_f is the tie to even, the neighbours go either side, a heading of 1e4 rad is wrapped
    the short way, and states at rest, of 1e30 and a target 1e-30 away stay inside the rounding bound."""
    case = CE.reff_cases()
    x, r = CE.reff_host(case)
    ok, rr, xr, k = CE.judge_reff(case, x, r)
    CE.record(RECORD, 'E filter host f32: %d lanes, worst error / bound r %.3g, x %.3g' % (len(ok), rr, xr))
    assert ok.all(), [case['names'].get(i, i) for i in np.flatnonzero(~ok)]
    by = {s: int(k[i]) for i, s in case['names'].items()}
    pi, n_ = CE.PI32, np.nextafter
    for v, turn in ((pi, 0), (-pi, 0), (n_(pi, F32(4)), 1), (n_(-pi, F32(-4)), -1), (n_(pi, F32(0)), 0),
                    (F32(3) * pi, 2), (F32(-3) * pi, -2), (n_(F32(3) * pi, F32(0)), 1), (n_(F32(-3) * pi, F32(0)), -1), (n_(F32(3) * pi, F32(10)), 2)):
        assert by['heading difference %r' % v] == turn and by['heading difference %r from a moving filter' % v] == turn, (v, turn)
    assert PI_TIES()
    assert by['unwrapped heading 1e4, target 0.3'] == -1592 and by['unwrapped heading 1e4, target 10003'] == 0
    assert np.isfinite(x).all()

    def wrong_wrap(F):                                                                 # teeth: a wrap that rounds half away from zero
        import torch
        F.switch = lambda target: setattr(F, 'r', torch.stack([target[0], target[1], F.x[0, 2] + (
            (target[2] - F.x[0, 2]) - F.two_pi * torch.sign(target[2] - F.x[0, 2]) * torch.floor(((target[2] - F.x[0, 2]) * F.inv_two_pi).abs() + 0.5))]))
    bad, _, _, kb = CE.judge_reff(case, *CE.reff_host(case, mutate=wrong_wrap))
    assert (kb != k).any()                                                             # ... takes another turn at the exact ties


def PI_TIES():
    """The f32 products at +-pi_f and +-3 pi_f ARE exact half-integers (else the tie rule would not be exercised)."""
    return all(F32(s) * (F32(m) * CE.PI32) * CE.INV_TWO_PI32 == F32(s * m * 0.5) for m in (1, 3) for s in (1, -1))


# C ---------------------------------------------------------------------------------------------------------------------------------
def test_packing_recipe_against_60_digits():
    lx, ly, w, kinds, names = CE.pack_cases()
    G64, refused = CE.pack_recipe(lx, ly, w)
    assert [k != 'kept' for k in kinds] == refused.tolist(), list(zip(names, refused))
    for i, (kind, name) in enumerate(zip(kinds, names)):
        if kind == 'kept':
            truth, cond = CE.pack_truth(lx[i], ly[i], w[i])
            err = np.abs(G64[i] - truth).max()
            bound = CE.K_PACK * CE.U53 * cond * np.abs(truth).max()
            CE.record(RECORD, 'C %-34s cond %.3g  max |G| %.3g  recipe err / bound %.3g' % (name, cond, np.abs(truth).max(), err / bound))
            assert err <= bound, name
            assert np.isfinite(G64[i].astype(F32)).all()
            if 'nearly' in name:
                assert 1e11 <= cond <= 1e13 and np.abs(truth).max() > 1e5
    with np.errstate(all='ignore'):
        assert np.isfinite(G64[kinds.index('G rounds to inf in f32')]).all()           # finite in f64, not in f32
        assert not np.isfinite(G64[kinds.index('det cancels to 0')]).all()
    # det is exactly 0 on the singular row: every entry of M is a small dyadic number
    from ml4ca_amd.deploy import allocation_matrix
    i = kinds.index('det is 0')
    with pytest.raises(ValueError, match='singular'):
        allocation_matrix(lx[i], ly[i], w[i])
    # the labelling block: the float32 host law on the recipe's G passes its own judge off the refused lanes, and a G with one entry an
    # f32 ulp off does not equal it bit for bit (the read-back sees G)
    case = CE.pack_label_case()
    act, z = CE.pid_host32(case)
    keep = ~case['refused']
    assert np.isfinite(act[:, keep]).all() and (np.abs(act[:, keep][..., 0:3]) < 1).all()   # nothing saturates: the actions carry G

    # ... and the read-back sees every one of G's 15 entries: one f32 ulp in G[m][j], either way, changes the bits of some action on some
    # kept lane - on most of them; the bow's square root can swallow an ulp of G[0][j] on a given row, which is why the block hands in
    # eight wrenches and not three
    seen, G32 = np.zeros((5, 3, 2)), case_G(case)
    for m in range(5):
        for j in range(3):
            for k, way in enumerate((np.inf, -np.inf)):
                def off_by_an_ulp(c, m=m, j=j, way=way):
                    c.G = c.G.copy()
                    c.G[:, m, j] = np.nextafter(c.G[:, m, j], F32(way))
                bad, _ = CE.pid_host32(case, mutate=off_by_an_ulp)
                lanes = G32[keep][:, m, j] != 0          # (an entry that is exactly 0 has no f32 ulp: its neighbours are subnormals, and
                assert lanes.any()                       # sub / kf underflows; G[0][0] is 0 on every symmetric hull)
                seen[m, j, k] = (~CE.bits_equal(bad[:, keep], act[:, keep])).any((0, 2))[lanes].mean()
    CE.record(RECORD, 'C read-back: share of kept lanes with G[m][j] != 0 on which one f32 ulp in G[m][j] shows, least over the two directions\n%s' % seen.min(2))
    assert (seen > 0).all() and seen.min() >= 0.5, seen.min(2)


def case_G(case):
    from ml4ca_amd.deploy import dp_controller_table_params
    with np.errstate(all='ignore'):
        return dp_controller_table_params(case['table'])['G'].astype(F32)
