"""The scans and reductions between a flight and what is read off it, on the GPU at production grid sizes and ragged edges, on the cases
of tests/scan_edges.py (whose fairness tests/test_scan_edges_cpu.py asserts without a GPU), through rollout.gae,
rollout.normalize_advantages, the dpenv_adv_* entry points and evaluate.ScoreCard.

1. GAE banks and lanes: T around one, two, three and four banks of 8 rows, 63 / 64 / 65 live lanes in both forms, end bytes of
   {1, 2, 3, 5, 0x80, 0xFF}; adv / ret equal the oracle's float32 scan bit for bit and sit inside the running bound around its float64
   scan; the statistics fall under the double-sum bound.
2. GAE forms: the scalar form chosen by a float block 4 bytes, or `end` 1 byte, off its alignment equals the two-column form bit for bit;
   the bytes around adv, ret and the workspace stay untouched.
3. GAE partial counts: 257 partials in either form, 512 and 513: the strided part of gae_finalize_kernel's fold.
4. Sums and apply: the counts around the float4 tail, one and 257 workgroups, the grid cap and the second trip behind it, aligned
   (float4 reads) and carved 4 bytes in (the scalar fallback), a constant and an offset block.
5. Score card: read() equals the NumPy statement of include/dpenv.h's per-row update bit for bit.
6. Score summary: 257 and 513 partials, min / max on env n-1, all returns negative.
Every bound is derived in tests/scan_edges.py.  The largest measured error as a fraction of its bound is printed per case and appended
to the file the environment variable SCAN_EDGES_RECORD names, if it is set (profiles/scan_edges_errors.txt holds such a record)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import scan_edges as SE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
RECORD = os.environ.get('SCAN_EDGES_RECORD', '')
PAT = {'torch.float32': -77.25, 'torch.float64': 12345.678, 'torch.uint8': 0xA5}


def torch_():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def record(group, case, **ratios):
    line = '%-22s %-28s %s' % (group, case, '  '.join('%s %.3g' % kv for kv in ratios.items()))
    print(line)
    if RECORD:
        with open(RECORD, 'a') as f:
            f.write(line + '\n')


def ratio(err, bound):
    """Largest err / bound, the elements with err = 0 left out (a bound of 0 asks for exactly that)."""
    err, bound = np.atleast_1d(np.asarray(err, F64)), np.atleast_1d(np.asarray(bound, F64))
    assert (err <= bound).all(), 'error above the derived bound: %.3g of it' % float((err / np.maximum(bound, 1e-300)).max())
    nz = err > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def dev(x):
    return None if x is None else torch_().from_numpy(np.array(x)).to(DEV)


def carve(x, lead, tail=16):
    """x (a NumPy array) as a contiguous view `lead` elements into a pattern-filled device vector: (vector, view)."""
    torch = torch_()
    t = torch.from_numpy(np.array(x))
    buf = torch.full((lead + t.numel() + tail,), PAT[str(t.dtype)], dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous()
    return buf, view


def guards_intact(buf, view, lead):
    pat = PAT[str(buf.dtype)]
    return bool((buf[:lead] == pat).all()) and bool((buf[lead + view.numel():] == pat).all())


def _p(t):
    return C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch_().cuda.current_stream().cuda_stream)


def check_stats(stats, adv32, K, what):
    """stats (device float64[2]) against fsum of the float32 advantages under the double-sum bound; returns the two ratios."""
    (s1, s1abs), (s2, _) = SE.gae_stats_reference(adv32)
    got = stats.cpu().numpy()
    return (ratio(abs(got[0] - s1), SE.sum_bound(K, s1abs)), ratio(abs(got[1] - s2), SE.sum_bound(K, s2)))


# ---- 1. GAE banks and lanes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(SE.GAE_CASES)), ids=[SE.gae_case_id(c) for c in SE.GAE_CASES])
def test_gae_banks_and_lanes(k):
    torch = torch_()
    from ml4ca_amd import rollout
    T, n = SE.GAE_CASES[k]
    gamma, lam = SE.gamma_lam(k)
    inp = SE.gae_inputs(T, n)
    rew, val = dev(inp['rew']), dev(inp['val'])
    V = SE.gae_form(n)
    worst = dict(adv=0.0, ret=0.0, s1=0.0, s2=0.0)
    for mode in SE.GAE_MODES:
        ref = SE.gae_reference(T, n, mode, gamma, lam)
        end, boot, lv = (dev(a) for a in SE.gae_mode_args(inp, mode))
        stats = torch.zeros(2, dtype=torch.float64, device=DEV)
        adv, ret = rollout.gae(rew, val, end=end, boot=boot, last_val=lv, gamma=gamma, lam=lam, stats=stats)
        a, r = adv.cpu().numpy(), ret.cpu().numpy()
        assert np.array_equal(a, ref['adv32']) and np.array_equal(r, ref['ret32']), mode
        worst['adv'] = max(worst['adv'], ratio(np.abs(a.astype(F64) - ref['adv64']), ref['badv']))
        worst['ret'] = max(worst['ret'], ratio(np.abs(r.astype(F64) - ref['ret64']), ref['bret']))
        q1, q2 = check_stats(stats, ref['adv32'], SE.k_gae_stats(T, n, V), mode)
        worst['s1'], worst['s2'] = max(worst['s1'], q1), max(worst['s2'], q2)
        plain = rollout.gae(rew, val, end=end, boot=boot, last_val=lv, gamma=gamma, lam=lam)       # without statistics: the same rows
        assert torch.equal(plain[0], adv) and torch.equal(plain[1], ret), mode
    record('gae_banks_lanes', SE.gae_case_id((T, n)), **worst)


# ---- 2. GAE forms -----------------------------------------------------------------------------------------------------------------------
def _run_form(T, n, gamma, lam, float_off, end_off):
    """One dpenv_gae_stats with every float block float_off bytes and `end` end_off bytes behind a 16-byte boundary, adv, ret and the
    workspace inside pattern-filled vectors: (adv, ret, stats) on the host after the guards were found intact."""
    torch = torch_()
    from ml4ca_amd import _lib, rollout
    inp = SE.gae_inputs(T, n)
    fl, el, wl = 4 + float_off // 4, 16 + end_off, 2
    blk = {k: carve(inp[k], fl)[1] for k in ('rew', 'val', 'boot', 'last_val')}
    end = carve(inp['end'], el)[1]
    abuf, adv = carve(np.zeros((T, n), F32), fl)
    rbuf, ret = carve(np.zeros((T, n), F32), fl)
    nws = int(_lib.load().dpenv_gae_workspace_bytes(n))
    assert nws == SE.gae_workspace_bytes(n)
    wbuf, ws = carve(np.zeros(nws // 8, F64), wl)
    for t in list(blk.values()) + [adv, ret]:
        assert t.data_ptr() % 16 == float_off
    assert end.data_ptr() % 16 == end_off and ws.data_ptr() % 16 == 0
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    rollout.gae(blk['rew'], blk['val'], end=end, boot=blk['boot'], gamma=gamma, lam=lam, out=(adv, ret), stats=stats, workspace=ws)
    torch.cuda.synchronize()
    assert guards_intact(abuf, adv, fl) and guards_intact(rbuf, ret, fl) and guards_intact(wbuf, ws, wl)
    return adv.cpu().numpy(), ret.cpu().numpy(), stats


@pytest.mark.parametrize('carved', ['floats_4_bytes', 'end_1_byte'])
@pytest.mark.parametrize('case', SE.GAE_FORM_CASES, ids=SE.gae_case_id)
def test_gae_scalar_form_behind_a_misaligned_view(case, carved):
    T, n = case
    gamma, lam = SE.GAMMA_LAM[0]
    float_off, end_off = (4, 0) if carved == 'floats_4_bytes' else (0, 1)
    assert SE.gae_form(n) == 2 and SE.gae_form(n, float_off, end_off) == 1
    ref = SE.gae_reference(T, n, 'boot', gamma, lam)
    a2, r2, st2 = _run_form(T, n, gamma, lam, 0, 0)
    a1, r1, st1 = _run_form(T, n, gamma, lam, float_off, end_off)
    assert np.array_equal(a2, ref['adv32']) and np.array_equal(r2, ref['ret32'])
    assert np.array_equal(a1, a2) and np.array_equal(r1, r2)
    q2 = check_stats(st2, ref['adv32'], SE.k_gae_stats(T, n, 2), 'two columns')
    q1 = check_stats(st1, ref['adv32'], SE.k_gae_stats(T, n, 1), 'scalar')
    record('gae_forms', '%s-%s' % (SE.gae_case_id(case), carved), s1=max(q1[0], q2[0]), s2=max(q1[1], q2[1]))


# ---- 3. GAE partial counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(SE.GAE_PARTIAL_CASES)), ids=[SE.gae_case_id(c) for c in SE.GAE_PARTIAL_CASES])
def test_gae_statistics_over_more_than_256_partials(k):
    torch = torch_()
    from ml4ca_amd import rollout
    T, n = SE.GAE_PARTIAL_CASES[k]
    V = SE.gae_form(n)
    assert SE.gae_partials(n, V) == SE.GAE_PARTIAL_COUNTS[k] > 256
    gamma, lam = SE.GAMMA_LAM[0]
    inp = SE.gae_inputs(T, n)
    ref = SE.gae_reference(T, n, 'boot', gamma, lam)
    blk = {key: dev(inp[key]) for key in ('rew', 'val', 'end', 'boot')}

    def run(sl=slice(None)):
        stats = torch.zeros(2, dtype=torch.float64, device=DEV)
        adv, _ = rollout.gae(blk['rew'][:, sl].contiguous(), blk['val'][:, sl].contiguous(), end=blk['end'][:, sl].contiguous(),
                             boot=blk['boot'][:, sl].contiguous(), gamma=gamma, lam=lam, stats=stats)
        return adv, stats

    adv, stats = run()
    assert np.array_equal(adv.cpu().numpy(), ref['adv32'])
    K = SE.k_gae_stats(T, n, V)
    q = check_stats(stats, ref['adv32'], K, 'whole')
    _, again = run()
    assert torch.equal(stats, again)                                   # the same bits
    # two "ranks": each scans its half of the env columns, the statistics add
    h = n // 2
    tot, bound = torch.zeros(2, dtype=torch.float64, device=DEV), np.zeros(2)
    for sl in (slice(0, h), slice(h, n)):
        a_, s_ = run(sl)
        part = ref['adv32'][:, sl]
        assert np.array_equal(a_.cpu().numpy(), part)
        (p1, p1abs), (p2, _) = SE.gae_stats_reference(part)
        Kh = SE.k_gae_stats(T, part.shape[1], SE.gae_form(part.shape[1]))
        bound += (SE.sum_bound(Kh, p1abs), SE.sum_bound(Kh, p2))
        tot += s_
    (s1, s1abs), (s2, _) = SE.gae_stats_reference(ref['adv32'])
    got = tot.cpu().numpy()
    qh = (ratio(abs(got[0] - s1), bound[0] + SE.U53 * abs(s1)), ratio(abs(got[1] - s2), bound[1] + SE.U53 * s2))
    # the one-pass normalisation fed by these statistics
    x = ref['adv32'].ravel()
    want, nb = SE.norm_reference(x, stats=(s1, s2), total=x.size, K=K, s1abs=s1abs)
    one, _, _ = rollout.normalize_advantages(adv.clone(), stats=stats)
    qn = ratio(np.abs(one.cpu().numpy().ravel().astype(F64) - want), nb)
    record('gae_partials', SE.gae_case_id((T, n)), s1=q[0], s2=q[1], halves_s1=qh[0], halves_s2=qh[1], one_pass_norm=qn)


# ---- 4. sums and apply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', SE.SUM_OFFSETS, ids=['aligned', 'carved_4_bytes'])
@pytest.mark.parametrize('count', SE.SUM_COUNTS)
def test_sums_and_apply(count, offset):
    torch = torch_()
    from ml4ca_amd import _lib
    lib = _lib.load()
    lead = 4 + offset // 4
    K = SE.k_sum(count, offset)
    worst = {}
    for kind in SE.SUM_BLOCKS:
        x, ref = SE.sum_block(kind, count), SE.sum_reference(kind, count)
        xbuf, xv = carve(x, lead)
        assert xv.data_ptr() % 16 == offset
        out = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
        _lib.check(lib.dpenv_adv_sum(_p(xv), count, _p(out), _s()))
        worst[kind + '_sum'] = ratio(abs(float(out) - ref['s1']), SE.sum_bound(K, ref['s1abs']) + SE.U * abs(ref['s1']))
        mean, std = dev(np.array([ref['mean']], F32)), dev(np.array([ref['std']], F32))
        _lib.check(lib.dpenv_adv_sumsq(_p(xv), count, _p(mean), _p(out), _s()))
        worst[kind + '_sumsq'] = ratio(abs(float(out) - ref['ssq']), SE.sum_bound(K, ref['ssq']) + SE.U * ref['ssq'])
        assert torch.equal(xv.cpu(), torch.from_numpy(np.array(x))) and guards_intact(xbuf, xv, lead)      # the sums only read
        # three-pass apply, from the f32 scalars
        _lib.check(lib.dpenv_adv_apply(_p(xv), count, _p(mean), _p(std), _s()))
        torch.cuda.synchronize()
        assert guards_intact(xbuf, xv, lead)
        got = xv.cpu().numpy()
        want, bound = SE.norm_reference(x, mean=ref['mean'], std=ref['std'])
        worst[kind + '_apply'] = ratio(np.abs(got.astype(F64) - want), bound)
        if kind == 'const':
            assert not got.view(np.uint32).any()                       # +0.0 bits
        # one-pass apply, from the two doubles
        xbuf, xv = carve(x, lead)
        stats = dev(np.array([ref['s1'], ref['s2']], F64))
        _lib.check(lib.dpenv_adv_apply_stats(_p(xv), count, _p(stats), float(count), _s()))
        torch.cuda.synchronize()
        assert guards_intact(xbuf, xv, lead)
        got = xv.cpu().numpy()
        want, bound = SE.norm_reference(x, stats=(ref['s1'], ref['s2']), total=count, K=0, s1abs=ref['s1abs'])
        worst[kind + '_apply_stats'] = ratio(np.abs(got.astype(F64) - want), bound)
        if kind == 'const':
            assert not got.view(np.uint32).any()
    record('sums_apply', '%d-%s' % (count, 'aligned' if offset == 0 else 'carved'), **worst)


# ---- 5. score card ----------------------------------------------------------------------------------------------------------------------
def read_slots(sc):
    """ScoreCard.read() as float64 [13, n] in the order of DPENV_SCORE_*."""
    r = sc.read()
    w, ew = r['work'].T, r['ep_work'].T
    torch = torch_()
    return torch.stack([r['iae'], w[0], w[1], w[2], r['ret'], r['len'], r['episodes'], r['ep_iae'], ew[0], ew[1], ew[2], r['ep_ret'],
                        r['ep_len']]).cpu().numpy()


def same_bits(got, want, what):
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), '%s: slots %s differ, first at env %d: %r against %r' % (
        what, sorted({SE.SCORE_SLOTS[s] for s in np.nonzero(bad)[0]}), int(np.nonzero(bad)[1][0]), got[bad][0], want[bad][0])


def device_block(blk, bf16):
    torch = torch_()
    out = {k: dev(v) for k, v in blk.items() if v is not None}
    if bf16 and 'obs' in out:
        out['obs'] = out['obs'].to(torch.bfloat16)                     # exact: the rows are bf16-representable
    return out


def card(n):
    from ml4ca_amd import evaluate as EV
    sc = EV.ScoreCard(n, DEV)
    c = SE.score_consts()
    assert F32(sc._io.dt) == c['dt'] and [F32(v) for v in sc._io.norm] == list(c['norm'])
    assert [F32(v) for v in sc._io.power_coeff] == list(c['coeff']) and [F32(v) for v in sc._io.rps_max] == list(c['rps'])
    return sc, c


def fly(n, blk, bf16, cuts, piece):
    """The block once per entry of `cuts` (cut_at_end of that pass), each pass in pieces of `piece` rows: (device slots, host slots)."""
    sc, consts = card(n)
    st = SE.score_fresh(n)
    T = next(v.shape[0] for v in blk.values() if v is not None)
    dblk = device_block(blk, bf16)
    for cut in cuts:
        for t0, t1 in SE.score_pieces(T, piece):
            last = cut and t1 == T
            sc.add(SE.slice_block(dblk, t0, t1), cut_at_end=last)
            SE.score_update(st, SE.slice_block(blk, t0, t1), consts, cut_at_end=last)
    return read_slots(sc), SE.score_read(st)


@pytest.mark.parametrize('case', SE.SCORE_CASES, ids=SE.score_case_id)
def test_score_card_equals_the_headers_statement_bit_for_bit(case):
    T, n, obs_stride, bf16, act_stride = case
    rows = SE.score_rows(T, n, obs_stride, act_stride, bf16)
    moved = 0
    for kind in SE.DONE_PATTERNS:
        blk = dict(rows, done=SE.done_pattern(kind, T, n))
        for cut in (False, True):
            for piece in (0, 1, 2):
                got, want = fly(n, blk, bf16, (cut, False), piece)     # a second pass: the trapezoid is carried into it (or not, after a cut)
                same_bits(got, want, '%s cut %d pieces of %d' % (kind, cut, piece))
                moved += int(np.count_nonzero(want))
    assert moved > 0
    blk = dict(rows, done=None)
    blk.pop('integ')                                                   # without the integral action: e = obs
    got, want = fly(n, blk, bf16, (False,), 0)
    same_bits(got, want, 'no integ, no done')


@pytest.mark.parametrize('only', ['obs', 'act', 'rew'])
def test_score_card_with_one_block_alone(only):
    n = 65
    rows = SE.score_rows(1, n, 9, 7)
    blk = {only: rows[only]}
    got, want = fly(n, blk, False, (False, False, True), 0)            # T = 1 three times: two segments, then closed
    same_bits(got, want, only)
    names = SE.SCORE_SLOTS
    feeds = dict(obs='ep_iae', act='ep_work0', rew='ep_ret')
    for src, slot in feeds.items():
        assert bool(got[names.index(slot)].any()) == (src == only), (only, slot)
    assert (got[names.index('ep_len')] == 3).all() and (got[names.index('episodes')] == 1).all()


def test_score_card_on_an_all_negative_reward_block():
    n, T = 65, 5
    rows = SE.score_rows(T, n, 9, 7, negative_rew=True)
    assert rows['rew'].max() < 0
    sc, consts = card(n)
    sc.add(device_block(rows, False))
    want = SE.score_read(SE.score_update(SE.score_fresh(n), rows, consts))
    got = read_slots(sc)
    same_bits(got, want, 'negative rewards')
    s = sc.summary()
    k = SE.SCORE_SLOTS.index('ret')
    assert float(s['max']['ret']) == got[k].max() < 0 and float(s['min']['ret']) == got[k].min()


# ---- 6. score summary -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SE.SCORE_SUMMARY_N)
def test_score_summary_over_more_than_256_partials(n):
    torch = torch_()
    assert SE.score_partials(n) > 256
    rows = SE.summary_rows(n)
    sc, consts = card(n)
    dblk = device_block(rows, False)
    sc.add(dblk, cut_at_end=True).add(dblk)
    st = SE.score_update(SE.score_fresh(n), rows, consts, cut_at_end=True)
    want = SE.score_read(SE.score_update(st, rows, consts))
    got = read_slots(sc)
    same_bits(got, want, 'summary rows')
    names = SE.SCORE_SLOTS
    assert int(got[names.index('iae')].argmin()) == n - 1 and int(got[names.index('ret')].argmax()) == n - 1
    assert got[names.index('ret')].max() < 0 and got[names.index('ep_ret')].max() < 0
    s1, s2 = sc.summary(), sc.summary()
    K = SE.k_score_summary(n)
    worst = 0.0
    for key in ('iae', 'work', 'ret', 'len', 'episodes', 'ep_iae', 'ep_work', 'ep_ret', 'ep_len'):
        slots = [names.index(key)] if key in names else [names.index(key + str(j)) for j in range(3)]
        for what in ('sum', 'min', 'max'):
            assert torch.equal(s1[what][key], s2[what][key]), (what, key)                          # the same bits every run
        for j, slot in enumerate(slots):
            v = got[slot]
            pick = (lambda t: float(t.reshape(-1)[j]))
            assert pick(s1['min'][key]) == v.min() and pick(s1['max'][key]) == v.max(), key
            tot, tot_abs = SE.fsum_terms(v)
            worst = max(worst, ratio(abs(pick(s1['sum'][key]) - tot), SE.sum_bound(K, tot_abs)))
    record('score_summary', 'n%d' % n, sums=worst)
