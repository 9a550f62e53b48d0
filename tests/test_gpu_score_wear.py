"""The score card's wear axis on the device (dpenv_score_accumulate_wear / evaluate.ScoreCard(wear=)): IADC, the integral absolute
derivative of the commands, accumulated in the pass that updates the score state.

Yardsticks.  (a) A NumPy float32 restatement of the per-row law of include/dpenv.h, bit for bit, for the variants whose command decode is
exact in f32 (full, simple, limited, final without cont_ang).  (b) evaluate.iadc in float64 for final with cont_ang, whose azimuths pass
through the kernels' own atan2 (max abs error 2.6e-7, dpenv.h): the bound per interval is derived in BOUND below from that figure and the
f32 roundings counted from the law.  (c) dpenv_score_accumulate itself, byte for byte, for the score state."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NMAX, TMAX = 200, 50
SIZES_N = (1, 63, 64, 65, 200)              # one lane, a ragged wave, a full wave, one lane into the next, three waves and a tail
SIZES_T = (1, 2, 3, 4, 5, 7, 50)            # the two banks' odd / even / single-row trips
F = np.float32
PI_F = F(math.pi)
VARIANTS = {'full': ('full', False, 6), 'simple': ('simple', False, 3), 'limited': ('limited', False, 5), 'final_wrap': ('final', False, 5),
            'final_cont': ('final', True, 7)}

# ---- the bound of (b), per interval, absolute, in IADC's own units ---------------------------------------------------------------------
U = 2.0 ** -24                               # unit roundoff of f32
ATAN2 = 2.6e-7                               # dpenv.h: max abs error of the kernels' atan2
# thrust part: six reads n = f32(act * 100) (|n| <= 100: 100 U each), three differences (<= 200: 200 U each), two additions (<= 600:
# 600 U each), all / 100; the division's own rounding on a value <= 6
BOUND_RPS = (6 * 100 + 3 * 200 + 2 * 600) * U / 100.0 + 6 * U
# azimuth part: four angle reads (ATAN2 each), two differences (<= 2 pi: 2 pi U each), two 2 pi_f - d (2 pi U each, and 2 pi_f is not
# 2 pi: 2 |pi_f - pi| each), one addition (<= 2 pi: 2 pi U), all / pi; the division's rounding on a value <= 2 and pi_f for pi in it
DPI = abs(float(PI_F) - math.pi)
BOUND_ANGLE = (4 * ATAN2 + 2 * 2 * math.pi * U + 2 * (2 * math.pi * U + 2 * DPI) + 2 * math.pi * U) / math.pi + 2 * U + 2 * DPI / math.pi
BOUND = BOUND_RPS + BOUND_ANGLE              # ~3.0e-6 per interval; the f64 sums add ~1e-16 relative per term


def _mods():
    import torch
    from ml4ca_amd import evaluate as EV
    return torch, EV


_ROWS = {}


def rows(seed=0):
    """Seeded host rows [TMAX, NMAX, .] float32: test_gpu_score.py's magnitudes (actions in +-1.3: every clip is hit, the wrap form wraps),
    with exact repeats (a zero change), +-1 (the seam of the linear decodes) and done bytes of several non-zero values."""
    if seed not in _ROWS:
        rng = np.random.RandomState(2000 + seed)
        obs = rng.normal(0.0, 1.0, size=(TMAX, NMAX, 9)).astype(F)
        obs[..., 0:2] *= 2.0
        obs[..., 2] *= 0.3
        integ = (rng.uniform(-1, 1, size=(TMAX, NMAX, 3)) * np.array([0.02, 0.03, 0.004])).astype(F)
        act = rng.uniform(-1.3, 1.3, size=(TMAX, NMAX, 7)).astype(F)
        act[3::7, 2::5] = act[2:-1:7, 2::5][:act[3::7, 2::5].shape[0]]                   # a row repeated: nothing moves
        act[1::6, 3::4, 3:6] = np.where(rng.uniform(size=act[1::6, 3::4, 3:6].shape) < 0.5, -1.0, 1.0)
        rew = rng.uniform(-1.0, 3.5, size=(TMAX, NMAX)).astype(F)
        d = np.where(rng.uniform(size=(TMAX, NMAX)) < 0.1, rng.choice([1, 2, 3, 5, 128, 255], size=(TMAX, NMAX)), 0).astype(np.uint8)
        d[:, 0] = 0; d[0, 0] = 1                        # done at t = 0
        d[:, 2] = 0; d[3, 2] = 1; d[4, 2] = 5           # on two consecutive rows: a one-row episode
        d[:, 3] = 0                                     # an env with none
        d[:, 4] = 3                                     # every row: one-row episodes only
        _ROWS[seed] = dict(obs=obs, integ=integ, act=act, rew=rew, done=d)
    return _ROWS[seed]


def block(r, n=NMAX, t0=0, t1=TMAX, adim=7, bf16=False, keys=('obs', 'act', 'rew', 'done', 'integ')):
    torch, _ = _mods()
    out = {}
    for k in keys:
        x = r[k][t0:t1, :n]
        if k == 'act':
            x = x[..., :adim]
        t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        out[k] = t.to(torch.bfloat16) if (k == 'obs' and bf16) else t
    return out


# ---- (a) the law, restated in NumPy float32 ---------------------------------------------------------------------------------------------
def clipf(v, b):
    return np.minimum(np.maximum(v, -b), b)


def decode(act, variant, cont_ang):
    """(n [n, 3] percent, alpha [n, 2] rad) of one row block act [n, A] float32: the env's command decode in f32, operation by operation"""
    thr = clipf((act[:, :3] * F(100.0)).astype(F), F(100.0))
    if variant == 'full':
        ang = clipf((act[:, 4:6] * PI_F).astype(F), PI_F)
    elif variant == 'limited':
        h = F(PI_F * F(0.5))
        ang = clipf((act[:, 3:5] * h).astype(F), h)
    elif variant == 'final' and not cont_ang:
        a = act[:, 3:5]
        w = (a - (F(2.0) * np.floor(((a + F(1.0)).astype(F) * F(0.5)).astype(F))).astype(F)).astype(F)
        ang = clipf((w * PI_F).astype(F), PI_F)
    elif variant == 'simple':
        ang = np.zeros((act.shape[0], 2), F)
    else:
        raise ValueError(variant)
    return thr, ang


class Restated(object):
    """The wear state of n envs and the per-row update of dpenv.h."""

    def __init__(self, n):
        self.rps, self.ang, self.c_rps, self.c_ang = (np.zeros(n, np.float64) for _ in range(4))
        self.np_, self.ap = np.zeros((n, 3), F), np.zeros((n, 2), F)
        self.has_prev = np.zeros(n, bool)

    def add(self, act, done, variant, cont_ang, cut_at_end=False):
        T = act.shape[0]
        two_pi = F(F(2.0) * PI_F)
        for t in range(T):
            thr, ang = decode(act[t], variant, cont_ang)
            dn = (((np.abs(thr[:, 0] - self.np_[:, 0]) + np.abs(thr[:, 1] - self.np_[:, 1])).astype(F)
                   + np.abs(thr[:, 2] - self.np_[:, 2])).astype(F) / F(100.0)).astype(F)
            d = np.abs((ang - self.ap).astype(F))
            w = np.minimum(d, (two_pi - d).astype(F))
            da = ((w[:, 0] + w[:, 1]).astype(F) / PI_F).astype(F)
            self.rps += np.where(self.has_prev, dn.astype(np.float64), 0.0)
            self.ang += np.where(self.has_prev, da.astype(np.float64), 0.0)
            self.np_, self.ap = thr, ang
            self.has_prev[:] = True
            end = (done[t] != 0) if done is not None else np.zeros(act.shape[1], bool)
            if cut_at_end and t == T - 1:
                end = np.ones_like(end)
            self.c_rps += np.where(end, self.rps, 0.0)
            self.c_ang += np.where(end, self.ang, 0.0)
            self.rps[end] = 0.0; self.ang[end] = 0.0; self.has_prev[end] = False
            self.np_ = np.where(end[:, None], F(0.0), self.np_); self.ap = np.where(end[:, None], F(0.0), self.ap)
        return self

    def slots(self):
        return np.stack([self.rps, self.ang, self.c_rps, self.c_ang])


def wear_slots(sc):
    torch, _ = _mods()
    r = sc.read()
    return torch.stack([r['iadc_rps'], r['iadc_angle'], r['ep_iadc_rps'], r['ep_iadc_angle']]).cpu().numpy()


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('mode', ['full', 'simple', 'limited', 'final_wrap'])
def test_wear_is_the_restated_law_bit_for_bit(mode, bf16):
    """Every (n, T) of the bank scheme's trips and the ragged last wave: a block with done bytes, then the same block again with cut_at_end
    (the previous sample travels across the call), against the restatement - the four read slots, bit for bit."""
    torch, EV = _mods()
    variant, cont_ang, adim = VARIANTS[mode]
    r = rows()
    moved = 0.0
    for n in SIZES_N:
        for T in SIZES_T:
            blk = block(r, n=n, t1=T, adim=adim, bf16=bf16)
            sc = EV.ScoreCard(n, DEV, wear=dict(variant=variant, cont_ang=cont_ang)).add(blk).add(blk, cut_at_end=True)
            a, d = r['act'][:T, :n, :adim], r['done'][:T, :n]
            want = Restated(n).add(a, d, variant, cont_ang).add(a, d, variant, cont_ang, cut_at_end=True).slots()
            got = wear_slots(sc)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, T, np.abs(got - want).max())
            assert not got[:2].any()                                       # cut_at_end: nothing stays open
            moved += got[2].sum()
            if mode == 'simple':
                assert not got[3].any()
            tot = sc.totals()
            assert torch.equal(tot['iadc'], tot['iadc_rps'] + tot['iadc_angle'])
    assert moved > 0


# ---- (b) final with cont_ang against float64 --------------------------------------------------------------------------------------------
def seam_rows():
    """rows() with heads on both sides of the +-pi seam (sin = +-eps, cos < 0) and both-zero head pairs of either cos sign planted"""
    r = dict(rows(seed=1))
    act = r['act'].copy()
    eps = [F(1e-7), F(-1e-7), F(1e-30), F(-1e-30), F(3e-4), F(-3e-4)]
    for t in range(TMAX):
        act[t, 10:16, 3] = np.roll(eps, t); act[t, 10:16, 4] = F(-1.0 - 0.01 * (t % 3))          # port: across the seam row after row
        act[t, 10:16, 5], act[t, 10:16, 6] = F(0.0), F(1.0)                                      # (their star azimuth at rest)
        act[t, 16:22, 5] = np.roll(eps, 2 * t); act[t, 16:22, 6] = F(-0.5)                       # star likewise
        z = [F(0.0), F(-0.0)]
        act[t, 22, 3], act[t, 22, 4] = z[t % 2], z[(t // 2) % 2]                                  # both-zero pairs: angle +-0 or +-pi
        act[t, 23, 5], act[t, 23, 6] = z[(t // 2) % 2], z[t % 2]
    r['act'] = act
    return r


def test_final_cont_against_float64_within_the_derived_bound():
    torch, EV = _mods()
    r = seam_rows()
    worst = 0.0
    for n, T in ((200, 50), (65, 7), (1, 2)):
        blk = block(r, n=n, t1=T, keys=('obs', 'act', 'rew'))
        got = EV.ScoreCard(n, DEV, wear=dict(variant='final', cont_ang=True)).add(blk).read()
        want = EV.iadc(blk['act'].cpu(), 'final', True)
        for key, per in (('iadc_rps', BOUND_RPS), ('iadc_angle', BOUND_ANGLE), ('iadc', BOUND)):
            err = float((got[key].cpu() - want[key]).abs().max())
            share = err / ((T - 1) * per)
            print('final cont_ang n = %d T = %d %s: max |err| %.3e, bound %.3e, share %.3f' % (n, T, key, err, (T - 1) * per, share))
            worst = max(worst, share)
            assert err <= (T - 1) * per, (n, T, key, err)
        assert float(want['iadc_angle'].min()) > 0 or n == 1
    print('final cont_ang: largest share of the bound used %.3f' % worst)
    # the seam is crossed the short way: a head pair hopping between sin = +eps and sin = -eps at cos < 0 moves by ~2 eps, not by 2 pi
    blk = block(r, n=32, t1=50, keys=('act', 'rew'))
    per = EV.iadc(blk['act'].cpu(), 'final', True, per_step=True)['iadc_angle'][:, 10:16]
    assert 0.0 < float(per.max()) < 1e-3


# ---- (c) the score state --------------------------------------------------------------------------------------------------------------
CASES = [dict(), dict(done=False), dict(integ=False), dict(cut=True), dict(done=False, cut=True), dict(obs=False, integ=False), dict(rew=False),
         dict(bf16=True), dict(obs=False, integ=False, rew=False, done=False)]


@pytest.mark.parametrize('case', CASES, ids=['all', 'no_done', 'no_integ', 'cut', 'no_done_cut', 'no_obs', 'no_rew', 'bf16', 'act_only'])
def test_score_state_is_accumulates_byte_for_byte(case):
    torch, EV = _mods()
    keys = tuple(k for k in ('obs', 'act', 'rew', 'done', 'integ') if case.get(k, True))
    r = rows(seed=2)
    for n, T in ((200, 50), (65, 7)):
        plain, wear = EV.ScoreCard(n, DEV), EV.ScoreCard(n, DEV, wear=dict(variant='final', cont_ang=True))
        for t0, t1 in ((0, T // 2), (T // 2, T)):
            blk = block(r, n=n, t0=t0, t1=t1, bf16=case.get('bf16', False), keys=keys)
            plain.add(blk, cut_at_end=case.get('cut', False))
            wear.add(blk, cut_at_end=case.get('cut', False))
        assert torch.equal(plain._state, wear._state), (n, T)
        assert bool(plain._state.any()) and bool(wear._wear.any())
        a, b = plain.read(), wear.read()
        assert all(torch.equal(a[k], b[k]) for k in a)


# ---- blocks and episodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'final_cont'])
def test_pieces_equal_one_block_bit_for_bit(mode):
    torch, EV = _mods()
    variant, cont_ang, adim = VARIANTS[mode]
    r = rows(seed=3)
    w = dict(variant=variant, cont_ang=cont_ang)
    for T in (2, 5, 50):
        one = EV.ScoreCard(NMAX, DEV, wear=w).add(block(r, t1=T, adim=adim))
        for cuts in ((1,), (T - 1,), (2, 3), (1, 2, 3, 4)):
            edges = [0] + sorted(set(c for c in cuts if 0 < c < T)) + [T]
            sc = EV.ScoreCard(NMAX, DEV, wear=w)
            for t0, t1 in zip(edges[:-1], edges[1:]):
                sc.add(block(r, t0=t0, t1=t1, adim=adim))
            assert torch.equal(one._state, sc._state) and torch.equal(one._wear, sc._wear), (T, cuts)


def test_any_nonzero_done_byte_ends_the_episode():
    """Two rows, the first with a done byte: nothing is counted across it, whatever the byte's value; without the byte the change counts."""
    torch, EV = _mods()
    act = np.zeros((2, 8, 6), F)
    act[1, :, 0], act[1, :, 4] = 0.5, 0.25                       # 50 % on the bow thrust, pi / 4 on the port azimuth
    done = np.zeros((2, 8), np.uint8)
    done[0, :7] = [1, 2, 3, 5, 64, 128, 255]                     # env 7: no done
    blk = dict(act=torch.from_numpy(act).to(DEV), rew=torch.zeros((2, 8), device=DEV), done=torch.from_numpy(done).to(DEV))
    got = EV.ScoreCard(8, DEV, wear=dict(variant='full')).add(blk).read()
    assert not bool(got['iadc'][:7].any()) and not bool(got['ep_iadc'].any())
    assert float(got['iadc_rps'][7]) == 0.5 and float(got['iadc_angle'][7]) == float(F(F(0.25) * PI_F) / PI_F)
    assert torch.equal(got['episodes'].cpu(), torch.tensor([1.0] * 7 + [0.0], dtype=torch.float64))
    want = Restated(8).add(act, done, 'full', False).slots()
    assert np.array_equal(wear_slots(EV.ScoreCard(8, DEV, wear=dict(variant='full')).add(blk)), want)


def test_a_fresh_wear_state_joined_in_mid_episode_counts_nothing_for_its_first_row():
    torch, EV = _mods()
    r = rows(seed=4)
    nodone = dict(r, done=np.zeros_like(r['done']))
    sc = EV.ScoreCard(NMAX, DEV, wear=dict(variant='full')).add(block(nodone, t1=10, adim=6))
    assert float(sc.read()['iadc'].min()) > 0
    sc._wear.zero_()                                            # the score state stays in mid-episode (has_prev = 1)
    sc.add(block(nodone, t0=10, t1=21, adim=6))
    want = Restated(NMAX).add(nodone['act'][10:21, :, :6], None, 'full', False).slots()
    assert np.array_equal(wear_slots(sc).view(np.uint64), want.view(np.uint64))
    differenced_against_zeros = Restated(NMAX)
    differenced_against_zeros.has_prev[:] = True
    assert not np.array_equal(differenced_against_zeros.add(nodone['act'][10:21, :, :6], None, 'full', False).slots(), want)
    plain = EV.ScoreCard(NMAX, DEV).add(block(nodone, t1=21, adim=6))
    assert torch.equal(plain._state, sc._state)
    sc.reset()
    assert not bool(sc._state.any()) and not bool(sc._wear.any())


# ---- lanes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'final_wrap', 'final_cont'])
def test_a_nan_and_an_inf_in_one_env_leave_every_other_env_alone(mode):
    torch, EV = _mods()
    variant, cont_ang, adim = VARIANTS[mode]
    r = rows(seed=5)
    bad = dict(r, act=r['act'].copy())
    i = 70                                                       # in the second wave
    bad['act'][3, i, 0] = np.nan; bad['act'][5, i, 1] = np.inf; bad['act'][7, i, 2] = -np.inf
    bad['act'][4, i, 3] = np.nan; bad['act'][6, i, 4] = np.inf; bad['act'][8, i, adim - 1] = -np.inf
    bad['act'][9, i, 3:adim] = np.inf; bad['act'][11, i, 3:adim] = np.nan
    w = dict(variant=variant, cont_ang=cont_ang)
    clean, dirty = (EV.ScoreCard(NMAX, DEV, wear=w).add(block(x, t1=20, adim=adim)) for x in (r, bad))
    others = torch.arange(NMAX, device=DEV) != i
    for a, b in ((clean._state, dirty._state), (clean._wear, dirty._wear)):
        a, b = a.view(-1, NMAX, 16), b.view(-1, NMAX, 16)                      # 16-byte streams [s][n]
        assert torch.equal(a[:, others], b[:, others])
        assert not torch.equal(a[:, i], b[:, i])
    got = dirty.totals()
    assert bool(torch.isfinite(got['iadc']).all())                            # every non-finite entry decodes to a finite command (dpenv.h)


# ---- guards, summary, capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 65])
def test_wear_state_and_workspace_guards_stay_intact(n):
    torch, EV = _mods()
    from ml4ca_amd import _lib
    lib = _lib.load()
    G = 4096
    r = rows(seed=6)
    sc = EV.ScoreCard(n, DEV, wear=dict(variant='final', cont_ang=True))
    nb, nw = int(lib.dpenv_score_wear_state_bytes(n)), int(lib.dpenv_score_wear_summary_workspace_bytes(n))
    sbuf = torch.full((nb + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((nw + 2 * G,), 0x5A, dtype=torch.uint8, device=DEV)
    sbuf[G:G + nb] = 0
    sc._wear, sc._wear_ws = sbuf[G:G + nb], wbuf[G:G + nw]
    sc.add(block(r, n=n)).add(block(r, n=n, t1=7), cut_at_end=True)
    sc.read()
    sc.summary()
    torch.cuda.synchronize()
    assert bool((sbuf[:G] == 0xA5).all()) and bool((sbuf[G + nb:] == 0xA5).all())
    assert bool((wbuf[:G] == 0x5A).all()) and bool((wbuf[G + nw:] == 0x5A).all())
    assert bool(sbuf[G:G + nb].any())


def test_wear_summary_against_read():
    torch, EV = _mods()
    r = rows(seed=7)
    sc = EV.ScoreCard(NMAX, DEV, wear=dict(variant='final', cont_ang=True)).add(block(r)).add(block(r, t1=9))
    rd, s1, s2 = sc.read(), sc.summary(), sc.summary()
    for k in ('iadc_rps', 'iadc_angle', 'ep_iadc_rps', 'ep_iadc_angle'):
        x = rd[k].cpu()
        for what in ('sum', 'min', 'max'):
            assert torch.equal(s1[what][k], s2[what][k]), (what, k)                  # identical bits
        assert float(s1['min'][k]) == float(x.min()) and float(s1['max'][k]) == float(x.max()), k
        # the fixed order: a wave's shuffle tree (offsets 32 ... 1) per 64 envs, then thread k of 256 takes partials k, k + 256, ... and a
        # halving tree folds the 256
        parts = []
        for b in range(0, NMAX, 64):
            v = np.zeros(64, np.float64)
            v[:min(64, NMAX - b)] = x[b:b + 64].numpy()
            off = 32
            while off:
                v = v + np.concatenate([v[off:], v[:off]])              # lane l takes lane l + off (modulo: only lane 0's chain is read)
                off //= 2
            parts.append(v[0])
        red = np.zeros(256, np.float64)
        red[:len(parts)] = parts
        h = 128
        while h:
            red[:h] = red[:h] + red[h:2 * h]
            h //= 2
        assert float(s1['sum'][k]) == red[0], k
    assert float(s1['sum']['iadc']) == float(s1['sum']['iadc_rps'] + s1['sum']['iadc_angle']) and 'iadc' not in s1['min']
    assert float(s1['sum']['ep_iadc_rps']) > 0 and float(s1['sum']['iae']) == float(EV.ScoreCard(NMAX, DEV).add(block(r)).add(block(r, t1=9)).summary()['sum']['iae'])


def test_add_with_wear_recorded_into_a_graph():
    torch, EV = _mods()
    r = rows(seed=8)
    blk = block(r, t1=37)
    w = dict(variant='final', cont_ang=True)
    eager = EV.ScoreCard(NMAX, DEV, wear=w)
    for _ in range(3):
        eager.add(blk)
    sc = EV.ScoreCard(NMAX, DEV, wear=w)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc.add(blk)
    sc.reset()                                    # whatever the capture did or did not execute
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager._state, sc._state) and torch.equal(eager._wear, sc._wear)
    tot = sc.totals()['iadc']
    assert float(tot[3]) > 0 and float(tot[4]) == 0.0           # env 3 never ends; env 4 ends on every row: one-row episodes move nothing


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------
_LOOP = {}
LOOP_N, LOOP_T = 128, 60


def loop_env():
    if 'env' not in _LOOP:
        import ml4ca_amd
        from ml4ca_amd.policy import ActorCritic
        env = ml4ca_amd.BatchedRevoltEnv(LOOP_N, device=DEV, terminate=False, time_limit=False, seed=11)
        _LOOP['ac'] = ActorCritic(9, 7, (80, 80, 80), seed=3, device=DEV).upload(env)
        _LOOP['env'] = env
    return _LOOP['env']


@pytest.mark.parametrize('who', ['controller', 'policy'])
def test_closed_loop_blocks_in_one_piece_and_in_chunks(who):
    torch, EV = _mods()
    from ml4ca_amd.policy import controller_rollout, policy_rollout
    env = loop_env()
    env.reset()
    if who == 'controller':
        EV._baseline_on(env)
        out = controller_rollout(env, LOOP_T)
    else:
        if env.integral_action is not None:
            env.set_integral_action(None)
        out = policy_rollout(env, LOOP_T, sample=False)
    blk = {k: out[k] for k in ('obs', 'act', 'rew', 'done')}
    one = EV.ScoreCard(LOOP_N, DEV, dt=env.dt, wear=env).add(blk)
    sc = EV.ScoreCard(LOOP_N, DEV, dt=env.dt, wear=env)
    for t0 in range(0, LOOP_T, 25):
        sc.add({k: v[t0:t0 + 25] for k, v in blk.items()})
    assert torch.equal(one._state, sc._state) and torch.equal(one._wear, sc._wear)
    tot = one.totals()
    want = EV.iadc(out['act'].cpu(), env.variant, env.cont_ang)
    assert float(tot['iadc'].min()) > 0
    assert float((tot['iadc'].cpu() - want['iadc']).abs().max()) <= (LOOP_T - 1) * BOUND


def test_streamed_baseline_box_test_against_the_resident_one():
    torch, EV = _mods()
    env = loop_env()
    one = EV.baseline_box_test(env, T=LOOP_T, reference_filter=True, wear=True)
    st = EV.baseline_box_test_streamed(env, T=LOOP_T, reference_filter=True, chunk=25, wear=True)
    assert {'iadc', 'iadc_rps', 'iadc_angle'} <= set(one) and {'iadc', 'iadc_rps', 'iadc_angle'} <= set(st)
    # without wear the results keep their keys
    assert set(EV.baseline_box_test_streamed(env, T=LOOP_T, reference_filter=True, chunk=25)) == {'iae', 'work', 'ret', 'score'}
    for key, per in (('iadc_rps', BOUND_RPS), ('iadc_angle', BOUND_ANGLE), ('iadc', BOUND)):
        assert st[key].shape == (LOOP_N,) and st[key].dtype == torch.float64
        err = float((st[key] - one[key]).abs().max())
        print('baseline box test, streamed against resident, %s: max |err| %.3e, bound %.3e' % (key, err, (LOOP_T - 1) * per))
        assert err <= (LOOP_T - 1) * per, key
    assert float(one['iadc'].min()) > 0


def test_a_qp_flights_azimuth_wear_respects_its_rate_limit():
    """The QP's azimuths move by at most da = azimuth_rate * dt per step (dpenv.h), so an interval's angle term is at most 2 da / pi, plus
    the angle part of the derived bound."""
    torch, EV = _mods()
    from ml4ca_amd import deploy
    env = loop_env()
    one = EV.baseline_box_test(env, T=330, reference_filter=False, allocator='qp', wear=True)    # unfiltered steps: surge at row 50, sway at row 300
    rate = float(np.max(deploy.qp_allocator_defaults()['azimuth_rate']))
    da = float(F(F(rate) * F(env.dt)))
    per = EV.iadc(one['out']['act'], env.variant, env.cont_ang, per_step=True)['iadc_angle']
    print('QP flight: largest per-step iadc_angle %.6f, limit %.6f' % (float(per.max()), 2 * da / math.pi))
    assert float(per.max()) <= 2 * da / math.pi + BOUND_ANGLE
    assert float(per.max()) > 0
    env.set_qp_allocator(off=True)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------
def test_gain_sweep_with_the_wear_axis():
    import ml4ca_amd
    from ml4ca_amd.deploy import dp_controller_defaults, gain_population
    torch, EV = _mods()
    K, D, T_ = 2, 2, 30
    env = ml4ca_amd.BatchedRevoltEnv(K * D, device=DEV, current=True, terminate=False, auto_reset=False, seed=5)
    pop = gain_population(K, dp_controller_defaults(), seed=1)
    res = EV.baseline_gain_sweep(env, pop, directions=D, vc=0.2, reference_filter=True, T=T_, chunk=10, wear=True)
    assert res['iadc'].shape == (K, D) and res['mean_iadc'].shape == (K,) and res['iadc'].dtype == torch.float64
    assert torch.equal(res['mean_iadc'], res['iadc'].mean(1)) and float(res['iadc'].min()) > 0
    mi, mw = res['mean_iae'].cpu().numpy(), res['mean_work'].sum(1).cpu().numpy()
    assert np.array_equal(res['front'], EV.pareto_front(mi, mw))
    assert np.array_equal(res['front3'], EV.pareto_front_nd(mi, mw, res['mean_iadc'].cpu().numpy()))
    if len(set(zip(mi.tolist(), mw.tolist()))) == K:
        assert set(res['front'].tolist()) <= set(res['front3'].tolist())
    plain = EV.baseline_gain_sweep(env, pop, directions=D, vc=0.2, reference_filter=True, T=T_, chunk=10)
    assert 'iadc' not in plain and 'front3' not in plain
    assert torch.equal(plain['iae'], res['iae']) and torch.equal(plain['work'], res['work']) and np.array_equal(plain['front'], res['front'])
