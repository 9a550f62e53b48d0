"""The streaming score card on the device (dpenv_score_* / evaluate.ScoreCard) against evaluate's own reference-pinned functions in float64.

Shapes: n = 200 (three full waves + 8 lanes), T = 37 (a ragged row prefetch).  Yardstick, from the same f32 / bf16 inputs widened to
float64 on the CPU: evaluate.iae_series(e_deg, 0, t), evaluate.work(evaluate.commanded_thrust(act), dt), rew.sum(0).

Tolerances.  iae and work: 1e-6 relative - every term passes through at most 8 f32 roundings (<= 8 * 2^-24 = 4.8e-7 relative), a sum of
terms of ONE sign inherits that bound, the f64 accumulation adds ~1e-13.  IAE terms are non-negative.  A work term carries the sign of its
thrust command, so the premise holds for work exactly when a thruster's command keeps its sign within an episode: the seeded rows draw one
sign per (env, thruster) - both signs occur, the clip is hit - and the bound is asserted relative to the value, as for IAE.  Commands that
change sign (a sum with cancellation, where "relative to the value" bounds nothing) are covered by test_mixed_sign_work against the same
1e-6, relative to the sum of the terms' magnitudes.  ret: |a - b| <= 1e-12 * sum |rew|.  len, episodes: exact."""
import math

import numpy as np
import pytest

from tests import tolerances as TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, T = 200, 37
DT = float(np.float32(0.2))          # the f32 sample period the card integrates with


def _mods():
    import torch
    from ml4ca_amd import evaluate as EV
    return torch, EV


_ROWS = {}


def rows(od=9, seed=0, n=N, nt=T, mixed=False):
    """Seeded host rows (float32 numpy): pose errors of order 2 m / 0.3 rad, integ within +-(0.02, 0.03, 0.004), actions in +-1.3 (the clip
    is hit), rewards in [-1, 3.5]."""
    key = (od, seed, n, nt, mixed)
    if key not in _ROWS:
        rng = np.random.RandomState(1000 + seed)
        obs = rng.normal(0.0, 1.0, size=(nt, n, od)).astype(np.float32)
        obs[..., 0:2] *= 2.0
        obs[..., 2] *= 0.3
        integ = (rng.uniform(-1, 1, size=(nt, n, 3)) * np.array([0.02, 0.03, 0.004])).astype(np.float32)
        act = rng.uniform(-1.3, 1.3, size=(nt, n, 7)).astype(np.float32)
        if not mixed:
            sign = np.where(rng.uniform(size=(n, 3)) < 0.5, -1.0, 1.0).astype(np.float32)
            act[..., :3] = np.abs(act[..., :3]) * sign
        rew = rng.uniform(-1.0, 3.5, size=(nt, n)).astype(np.float32)
        _ROWS[key] = dict(obs=obs, integ=integ, act=act, rew=rew)
    return _ROWS[key]


def device_block(r, bf16=False, integ=True, done=None):
    torch, _ = _mods()
    obs = torch.from_numpy(r['obs']).to(DEV)
    blk = dict(obs=obs.to(torch.bfloat16) if bf16 else obs, act=torch.from_numpy(r['act']).to(DEV), rew=torch.from_numpy(r['rew']).to(DEV))
    if integ:
        blk['integ'] = torch.from_numpy(r['integ']).to(DEV)
    if done is not None:
        blk['done'] = torch.from_numpy(done).to(DEV)
    return blk


def widen(blk):
    """The block's own values in float64 on the CPU: (true error in m, m, deg [T, n, 3]; act; rew)."""
    torch, _ = _mods()
    e = blk['obs'][..., :3].cpu().double()
    if blk.get('integ') is not None:
        e = e - blk['integ'].cpu().double()
    e = torch.stack([e[..., 0], e[..., 1], torch.rad2deg(e[..., 2])], dim=-1)
    return e, blk['act'].cpu().double(), blk['rew'].cpu().double()


def yardstick(e_deg, act, rew):
    """(iae [n], work [n, 3], ret [n], sum |rew| [n]) of the rows given, float64, by evaluate's reference-pinned functions."""
    torch, EV = _mods()
    t = torch.arange(e_deg.shape[0], dtype=torch.float64) * DT
    _, cum = EV.iae_series(e_deg, torch.zeros_like(e_deg), t)
    return cum[-1], EV.work(EV.commanded_thrust(act), DT), rew.sum(0), rew.abs().sum(0)


def close_rel(got, want, what, rtol=1e-6):
    got, want = got.cpu().double(), want.double()
    err = (got - want).abs()
    rel = float((err / want.abs().clamp_min(1e-300)).max()) if want.numel() else 0.0
    print('%s: max relative error %.3e' % (what, rel))
    assert bool((err <= rtol * want.abs()).all()), '%s: max relative error %.3e > %.0e' % (what, rel, rtol)


def close_ret(got, want, scale, what):
    err = (got.cpu().double() - want).abs()
    print('%s: max |err| / sum|rew| %.3e' % (what, float((err / scale.clamp_min(1e-300)).max())))
    assert bool((err <= 1e-12 * scale).all()), what


# ---- 1. one episode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('integ', [True, False], ids=['integ', 'no_integ'])
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('od', [9, 6])
def test_one_episode(od, bf16, integ):
    torch, EV = _mods()
    blk = device_block(rows(od), bf16=bf16, integ=integ)
    sc = EV.ScoreCard(N, DEV).add(blk)
    got = sc.read()
    iae, work, ret, absrew = yardstick(*widen(blk))
    close_rel(got['iae'], iae, 'iae')
    close_rel(got['work'], work, 'work')
    close_ret(got['ret'], ret, absrew, 'ret')
    assert torch.equal(got['len'].cpu(), torch.full((N,), float(T), dtype=torch.float64))
    for k in ('episodes', 'ep_iae', 'ep_ret', 'ep_len'):
        assert not bool(got[k].any()), k
    assert not bool(got['ep_work'].any())
    assert float(got['work'].abs().max()) > 0 and float((blk['act'][..., :3].abs() > 1.0).float().mean()) > 0.1      # the clip is hit


def test_mixed_sign_work():
    """Thrust commands that change sign from row to row: the trapezoid sums terms of both signs, so the error is bounded by 1e-6 of the
    sum of their magnitudes (work of |thrust|: the power law is odd), not of the sum itself."""
    torch, EV = _mods()
    blk = device_block(rows(9, seed=5, mixed=True))
    got = EV.ScoreCard(N, DEV).add(blk).read()
    e, act, rew = widen(blk)
    iae, work, _, _ = yardstick(e, act, rew)
    scale = EV.work(EV.commanded_thrust(act).abs(), DT)
    err = (got['work'].cpu() - work).abs()
    print('mixed-sign work: max |err| / sum|terms| %.3e' % float((err / scale).max()))
    assert bool((err <= 1e-6 * scale).all())
    close_rel(got['iae'], iae, 'iae')


def test_missing_blocks_leave_their_sums_untouched():
    torch, EV = _mods()
    blk = device_block(rows(9))
    full = EV.ScoreCard(N, DEV).add(blk).read()
    for drop in ('obs', 'act', 'rew'):
        part = {k: v for k, v in blk.items() if k != drop and not (drop == 'obs' and k == 'integ')}
        got = EV.ScoreCard(N, DEV).add(part).read()
        for key, src in (('iae', 'obs'), ('work', 'act'), ('ret', 'rew')):
            if src == drop:
                assert not bool(got[key].any()), (drop, key)
            else:
                assert torch.equal(got[key], full[key]), (drop, key)
        assert torch.equal(got['len'], full['len'])


# ---- 2. episodes ----------------------------------------------------------------------------------------------------------------------
def done_bytes(seed=3, n=N, nt=T):
    rng = np.random.RandomState(seed)
    d = np.where(rng.uniform(size=(nt, n)) < 0.1, rng.choice([1, 2, 3, 5], size=(nt, n)), 0).astype(np.uint8)
    d[:, 0] = 0; d[0, 0] = 1                       # done at t = 0
    d[:, 1] = 0; d[nt - 1, 1] = 2                  # at t = T - 1
    d[:, 2] = 0; d[10, 2] = 1; d[11, 2] = 5        # on two consecutive rows: a one-row episode
    d[:, 3] = 0                                    # an env with none
    d[:, 4] = 3                                    # every row: T one-row episodes
    d[:, n - 1] = 0; d[nt - 1, n - 1] = 1; d[0, n - 1] = 2       # the tail lane: first and last row
    return d


_EPISODES = {}


def episode_yardstick(blk, done):
    """Per env: (closed sums, closed count and length, open remainder) by the yardstick applied to each episode segment."""
    key = id(blk)
    if key in _EPISODES:
        return _EPISODES[key][1]
    torch, _ = _mods()
    e, act, rew = widen(blk)
    nt, n = done.shape
    z = lambda *s: np.zeros(s, np.float64)
    cl = dict(iae=z(n), work=z(n, 3), ret=z(n), absrew=z(n), len=z(n), episodes=z(n))
    op = dict(iae=z(n), work=z(n, 3), ret=z(n), absrew=z(n), len=z(n))
    for i in range(n):
        ends = [int(t) for t in np.nonzero(done[:, i])[0]]
        t0 = 0
        for t1 in ends + ([nt - 1] if (not ends or ends[-1] != nt - 1) else []):
            iae, work, ret, ab = yardstick(e[t0:t1 + 1, i:i + 1], act[t0:t1 + 1, i:i + 1], rew[t0:t1 + 1, i:i + 1])
            tgt = cl if done[t1, i] else op
            tgt['iae'][i] += float(iae); tgt['work'][i] += work[0].numpy(); tgt['ret'][i] += float(ret); tgt['absrew'][i] += float(ab)
            tgt['len'][i] += t1 + 1 - t0
            if done[t1, i]:
                cl['episodes'][i] += 1
            t0 = t1 + 1
    res = ({k: torch.from_numpy(v) for k, v in cl.items()}, {k: torch.from_numpy(v) for k, v in op.items()})
    _EPISODES[key] = (blk, res)               # the block is kept alive beside its result: the id stays unique
    return res


_EP_BLOCK = []


def episode_block():
    if not _EP_BLOCK:
        d = done_bytes()
        _EP_BLOCK.append((device_block(rows(9, seed=2), done=d), d))
    return _EP_BLOCK[0]


@pytest.mark.parametrize('cut', [False, True], ids=['open_end', 'cut_at_end'])
def test_episodes(cut):
    torch, EV = _mods()
    blk, d = episode_block()
    cl, op = episode_yardstick(blk, d)
    got = EV.ScoreCard(N, DEV).add(blk, cut_at_end=cut).read()
    if cut:                                       # the open remainder is closed too
        has_open = (op['len'] > 0).double()
        cl = {k: cl[k] + (op[k] if k != 'episodes' else has_open) for k in cl}
        op = {k: torch.zeros_like(v) for k, v in op.items()}
    close_rel(got['ep_iae'], cl['iae'], 'closed iae')
    close_rel(got['ep_work'], cl['work'], 'closed work')
    close_ret(got['ep_ret'], cl['ret'], cl['absrew'], 'closed ret')
    close_rel(got['iae'], op['iae'], 'open iae')
    close_rel(got['work'], op['work'], 'open work')
    close_ret(got['ret'], op['ret'], op['absrew'], 'open ret')
    assert torch.equal(got['ep_len'].cpu(), cl['len']) and torch.equal(got['len'].cpu(), op['len'])
    assert torch.equal(got['episodes'].cpu(), cl['episodes'])
    # one-row episodes: nothing to iae and work, their reward to ret, 1 to len
    assert float(got['episodes'][4]) == T and float(got['ep_len'][4]) == T
    assert float(got['ep_iae'][4]) == 0.0 and not bool(got['ep_work'][4].any())
    assert abs(float(got['ep_ret'][4]) - float(blk['rew'][:, 4].double().sum())) <= 1e-12 * float(blk['rew'][:, 4].double().abs().sum())
    assert float(got['episodes'][3]) == (1.0 if cut else 0.0) and float(got['episodes'][0]) == (2.0 if cut else 1.0)
    tot = EV.ScoreCard(N, DEV).add(blk, cut_at_end=cut).totals()
    assert torch.equal(tot['len'].cpu(), torch.full((N,), float(T), dtype=torch.float64))


# ---- 3. pieces ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_done', [False, True], ids=['no_done', 'done'])
def test_pieces_equal_one_call_bit_for_bit(with_done):
    torch, EV = _mods()
    d = None
    if with_done:
        d = done_bytes(seed=8)
        d[5, 7] = 1; d[5, N - 2] = 3; d[0, 9] = 2; d[36, 11] = 1           # on the last row of a piece, the first and the last of the block
    blk = device_block(rows(9, seed=4), done=d)
    one = EV.ScoreCard(N, DEV).add(blk).read()
    sc = EV.ScoreCard(N, DEV)
    for t0, t1 in ((0, 1), (1, 6), (6, 37)):
        sc.add({k: v[t0:t1] for k, v in blk.items()})
    pieces = sc.read()
    for k in one:
        assert torch.equal(one[k], pieces[k]), k
    assert float(one['iae'].sum() + one['ep_iae'].sum()) > 0


# ---- 4. bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [200, 1])
def test_state_and_workspace_guards_stay_intact(n):
    torch, EV = _mods()
    from ml4ca_amd import _lib
    lib = _lib.load()
    G = 4096
    r = rows(9, seed=6)
    d = done_bytes(seed=6)
    blk = {k: v[:, :n].contiguous() for k, v in device_block(r, done=d).items()}
    sc = EV.ScoreCard(n, DEV)
    nb, nw = int(lib.dpenv_score_state_bytes(n)), int(lib.dpenv_score_summary_workspace_bytes(n))
    sbuf = torch.full((nb + G,), 0xA5, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((nw + G,), 0x5A, dtype=torch.uint8, device=DEV)
    sbuf[:nb] = 0
    sc._state, sc._ws = sbuf[:nb], wbuf[:nw]
    sc.add(blk).add(blk, cut_at_end=True)
    got = sc.read()
    sc.summary()
    torch.cuda.synchronize()
    assert bool((sbuf[nb:] == 0xA5).all()) and bool((wbuf[nw:] == 0x5A).all())
    assert float(got['ep_len'].min()) == 2 * T and bool(sbuf[:nb].any())


# ---- 5. summary -----------------------------------------------------------------------------------------------------------------------
def test_summary_against_read():
    torch, EV = _mods()
    blk, _ = episode_block()
    sc = EV.ScoreCard(N, DEV).add(blk).add({k: v[:9] for k, v in blk.items()})
    rd, s1, s2 = sc.read(), sc.summary(), sc.summary()
    for what in ('sum', 'min', 'max'):
        for k in rd:
            assert torch.equal(s1[what][k], s2[what][k]), (what, k)           # identical bits
    for k, x in rd.items():
        x = x.cpu()
        assert torch.equal(s1['min'][k].cpu(), x.min(0).values if x.dim() == 2 else x.min()), k
        assert torch.equal(s1['max'][k].cpu(), x.max(0).values if x.dim() == 2 else x.max()), k
        cols = x.T if x.dim() == 2 else x[None]
        got = s1['sum'][k].cpu().reshape(-1)
        for j, col in enumerate(cols):
            want = math.fsum(col.tolist())
            assert abs(float(got[j]) - want) <= 1e-12 * math.fsum(abs(v) for v in col.tolist()), (k, j)
    assert float(s1['sum']['episodes']) > N and float(s1['max']['iae']) > float(s1['min']['iae'])


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------
def test_add_recorded_into_a_graph():
    torch, EV = _mods()
    blk, _ = episode_block()
    eager = EV.ScoreCard(N, DEV)
    for _ in range(3):
        eager.add(blk)
    want = eager.read()
    sc = EV.ScoreCard(N, DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc.add(blk)
    sc.reset()                                    # whatever the capture did or did not execute
    for _ in range(3):
        g.replay()
    got = sc.read()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert float(got['len'].sum() + got['ep_len'].sum()) == 3 * T * N


# ---- 7. closed loop -------------------------------------------------------------------------------------------------------------------
_LOOP = {}


def closed_loop(deployed):
    """One env batch and actor for every case; the one-launch flight and a ScoreCard fed its rows, once per mode."""
    torch, EV = _mods()
    if 'env' not in _LOOP:
        import ml4ca_amd
        from ml4ca_amd.policy import ActorCritic
        env = ml4ca_amd.BatchedRevoltEnv(128, device=DEV, terminate=False, time_limit=False, seed=11)
        _LOOP['ac'] = ActorCritic(9, 7, (80, 80, 80), seed=3, device=DEV).upload(env)
        _LOOP['env'] = env
    env = _LOOP['env']
    if deployed not in _LOOP:
        one = EV.deployment_box_test(env, T=120, integral=deployed, reference_filter=deployed)
        o = one['out']
        card = EV.ScoreCard(128, DEV, dt=env.dt).add(dict(obs=o['obs'], act=o['act'], rew=o['rew'], done=o['done'],
                                                          integ=one['integ'] if deployed else None)).totals()
        _LOOP[deployed] = (dict(iae=one['iae'].cpu(), work=one['work'].cpu(),
                                work_scale=EV.work(EV.commanded_thrust(o['act']).abs(), dt=env.dt).cpu()), card)
    return (env,) + _LOOP[deployed]


@pytest.mark.parametrize('deployed', [False, True], ids=['plain', 'integral_filter'])
@pytest.mark.parametrize('chunk', [40, 50, 51])
def test_streamed_box_test(chunk, deployed):
    """The box schedule's switch at step 50 falls inside a launch (chunk 40), on a launch's first step (50) and on its last (51).

    Without the reference filter a switch on a launch's last step is in the stored state when the launch ends, and the next launch would
    rebuild its first policy input against the NEW setpoint, where the one launch of T forms that row against the old one (measured that
    way: IAE 16.3861 against 16.0595, the 5 m step seen one row early).  deployment_box_test_streamed therefore flies the step behind
    such a launch through policy_forward + env.step - the eager composition the fused launch equals row for row - and [51-plain] holds
    bit for bit like the other five cases; the filter's launches keep the last step's setpoint pending and need nothing."""
    torch, EV = _mods()
    env, one, card = closed_loop(deployed)
    st = EV.deployment_box_test_streamed(env, T=120, chunk=chunk, integral=deployed, reference_filter=deployed)
    for k in ('iae', 'work', 'ret'):                                            # (a) bit for bit
        assert st[k].dtype == torch.float64 and torch.equal(st[k], card[k]), k
    assert float(st['score'].read()['len'].min()) == 120 and float(st['iae'].min()) > 0
    for name, res in (('streamed', st), ('card', card)):                        # (b) the one-launch f32 evaluation, 1e-5 relative
        TOL.assert_close(res['iae'].cpu().numpy(), one['iae'].numpy(), 1e-2, rtol=1e-5, what=name + ' iae')
        # work sums terms of both signs: relative to the sum of their magnitudes where that is larger (the floor of the project's assert_close)
        TOL.assert_close(res['work'].cpu().numpy(), one['work'].numpy(), one['work_scale'].numpy(), rtol=1e-5, what=name + ' work')


def test_streamed_box_test_refuses_what_it_cannot_continue():
    """Integral action on, filter off, a switch on a launch's last step: the step behind it would have to go through env.step, which has no
    form with the integral action - refused before anything flies, with the way out named; the same flight with another chunk is flown."""
    torch, EV = _mods()
    env, _, _ = closed_loop(False)
    with pytest.raises(ValueError, match='reference_filter=True'):
        EV.deployment_box_test_streamed(env, T=120, chunk=51, integral=True, reference_filter=False)
    st = EV.deployment_box_test_streamed(env, T=120, chunk=50, integral=True, reference_filter=False)
    one = EV.deployment_box_test(env, T=120, integral=True, reference_filter=False)
    TOL.assert_close(st['iae'].cpu().numpy(), one['iae'].cpu().numpy(), 1e-2, rtol=1e-5, what='integral, no filter')
