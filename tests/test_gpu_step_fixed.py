"""The fixed step (dpenv_kernels.hip step_fixed_kernel) against the general body, bit for bit (-m gpu).

dpenv_step takes the fixed instantiation family when the lean step would serve the launch AND the plant runs its shipped 20
sub-steps and is not held; wrap mode, end conditions and the presence of a setpoint pick the instantiation.  Asking for the
reward parts sends the same step through the general body.  Both run from the same state with the same actions and setpoints:
observation, reward, done bits, the state written back and the counters must be the same bytes, and - the kernel's tail stores
being dropped by the buffer range check - the bytes past row n of every output must be untouched.  Launches with another
sub-step count or a held plant take the older kernels and must match all the same."""
import itertools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
MODES = ['full', 'simple', 'limited', 'final_wrap', 'final_cont']
SIZES = [1, 31, 65, 100, 257, 1000, 4099]


def _step(torch, env, st, ctr, act, nr, parts):
    """one step from (st, ctr) into outputs with sentinel tails; returns numpy obs, rew, done, state, counters and the tails"""
    n, od = env.n_envs, env.num_states
    env.set_state(H.to_dev(st), H.to_dev(ctr))
    obs_big = torch.full((n + 64, od), 7.5, dtype=torch.float32, device=env.device)
    rew_big = torch.full((n + 64,), 7.5, dtype=torch.float32, device=env.device)
    done_big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=env.device)
    p = torch.empty((4, n), dtype=torch.float32, device=env.device) if parts else None
    env.step(H.to_dev(act), new_ref=H.to_dev(nr) if nr is not None else None, out=(obs_big[:n], rew_big[:n], done_big[:n]), reward_parts=p)
    s2, c2 = env.get_state()
    torch.cuda.synchronize()
    tails = (obs_big[n:].cpu().numpy(), rew_big[n:].cpu().numpy(), done_big[n:].cpu().numpy())
    return (obs_big[:n].cpu().numpy(), rew_big[:n].cpu().numpy(), done_big[:n].cpu().numpy(), s2.cpu().numpy(), c2.cpu().numpy()), tails


def _compare(torch, env, rng, n, what):
    """three steps, with and without a setpoint handed over, each through both bodies from the same state"""
    st = H.random_state(rng, n, spread=0.6)
    st[2, ::5] += rng.choice([-3.5, 3.5], size=st[2, ::5].shape).astype(np.float32)      # headings past the wrap, both ways
    ctr = np.zeros((2, n), np.int32)
    ctr[0] = rng.randint(0, max(2, env.max_ep_len), size=n)
    ctr[0, ::3] = env.max_ep_len - 2                                                      # the time limit falls inside the three steps
    for t in range(3):
        act = H.random_actions(rng, n, env.num_actions)
        nr = rng.uniform(-4, 4, size=(3, n)).astype(np.float32) if t % 2 else None
        fixed, tails = _step(torch, env, st, ctr, act, nr, parts=False)
        gen, _ = _step(torch, env, st, ctr, act, nr, parts=True)
        for name, x, y in zip(('obs', 'reward', 'done', 'state', 'counters'), fixed, gen):
            assert x.tobytes() == y.tobytes(), '%s differs from the general body (%s, step %d, n %d)' % (name, what, t, n)
        assert (tails[0] == 7.5).all() and (tails[1] == 7.5).all() and (tails[2] == 0xA5).all(), 'wrote past row n (%s, n %d)' % (what, n)
        st, ctr = fixed[3], fixed[4]


@pytest.mark.parametrize('mode,ext', [(m, e) for m in MODES for e in (True, False) if not (m == 'simple' and e)])   # (simple has no extended state)
def test_fixed_step_matches_general(mode, ext):
    """every instantiation of a (mode, ext) pair: both wrap modes x end conditions (none, bounds, time limit, both), each with and
    without a setpoint (the steps of _compare alternate), over the ragged sizes in turn"""
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    rng = np.random.RandomState(7300 + 2 * MODES.index(mode) + int(ext))
    sizes = itertools.cycle(SIZES[MODES.index(mode):] + SIZES[:MODES.index(mode)])
    for wrap, terminate, time_limit in itertools.product(['reference', 'radians'], [False, True], [False, True]):
        n = next(sizes)
        env, _ = H.make_pair(mode, n, ext=ext, wrap_mode=wrap, terminate=terminate, time_limit=time_limit)
        assert env.n_steps == 20
        _compare(torch, env, rng, n, '%s ext=%d %s terminate=%d time_limit=%d' % (mode, ext, wrap, terminate, time_limit))


@pytest.mark.parametrize('n', SIZES)
def test_fixed_step_headline_every_ragged_size(n):
    """the headline instantiations (final / continuous angles / extended state, degrees, no end conditions) at every ragged size"""
    import torch
    rng = np.random.RandomState(7400 + n)
    env, _ = H.make_pair('final_cont', n, ext=True, wrap_mode='reference', terminate=False, time_limit=False)
    _compare(torch, env, rng, n, 'headline')


@pytest.mark.parametrize('kw', [dict(n_steps=1), dict(n_steps=5), dict(n_steps=19), dict(n_steps=21), dict(n_steps=33),
                                dict(hold_plant=True), dict(n_steps=10, hold_plant=True)],
                         ids=lambda kw: '-'.join('%s%s' % (k, v) for k, v in sorted(kw.items())))
def test_other_plant_lengths_keep_the_older_kernels(kw):
    """another sub-step count, or a held plant: not the fixed step's launch - the lean kernel serves it and matches the general body"""
    import torch
    rng = np.random.RandomState(7500 + kw.get('n_steps', 0) + 100 * int(kw.get('hold_plant', False)))
    for mode, n in (('final_cont', 257), ('full', 100)):
        env, _ = H.make_pair(mode, n, ext=True, terminate=False, time_limit=False, **kw)
        _compare(torch, env, rng, n, '%s %r' % (mode, kw))
