"""The lean step (dpenv_kernels.hip step_kernel<.., LEAN>) against the general one, bit for bit (-m gpu).

dpenv_step takes the lean instantiation when the launch uses none of the features it compiles out; asking for the reward parts
sends the same step through the general body.  Both run from the same state with the same actions and setpoints: observation,
reward, done bits and the state written back must be the same bytes.  The lean kernel's tail stores are dropped by the
buffer range check, so the bytes just past the output rows must be untouched."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
MODES = ['full', 'simple', 'limited', 'final_wrap', 'final_cont']


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


@pytest.mark.parametrize('case', range(16))
def test_lean_step_matches_general(case):
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    rng = np.random.RandomState(7100 + case)
    mode = MODES[case % 5] if case < 10 else MODES[rng.randint(5)]
    ext = bool(rng.randint(2)) and mode != 'simple'
    n = int(rng.choice([1, 31, 65, 100, 257, 1000, 4099]))
    kw = dict(wrap_mode=['reference', 'radians'][rng.randint(2)], terminate=bool(rng.randint(2)), time_limit=bool(rng.randint(2)),
              n_steps=[None, 1, 5, 20, 33][rng.randint(5)], hold_plant=bool(rng.randint(8) == 0))
    env, _ = H.make_pair(mode, n, ext=ext, **kw)
    st = H.random_state(rng, n, spread=0.6)
    ctr = np.zeros((2, n), np.int32)
    ctr[0] = rng.randint(0, max(2, env.max_ep_len), size=n)
    for t in range(3):
        act = H.random_actions(rng, n, env.num_actions)
        nr = rng.uniform(-4, 4, size=(3, n)).astype(np.float32) if (t + case) % 2 else None
        lean, tails = _step(torch, env, st, ctr, act, nr, parts=False)
        gen, _ = _step(torch, env, st, ctr, act, nr, parts=True)
        for name, x, y in zip(('obs', 'reward', 'done', 'state', 'counters'), lean, gen):
            assert x.tobytes() == y.tobytes(), '%s: lean and general step differ (case %d, step %d, n %d)' % (name, case, t, n)
        assert (tails[0] == 7.5).all() and (tails[1] == 7.5).all() and (tails[2] == 0xA5).all(), 'the lean step wrote past row n'
        st, ctr = lean[3], lean[4]


@pytest.mark.parametrize('n', [63, 1000])
def test_lean_step_matches_soa_layout(n):
    """the [dim][n] layout always takes the general body: its rows, transposed, are the lean step's [n][dim] rows"""
    import torch
    rng = np.random.RandomState(n)
    env_a, _ = H.make_pair('final_cont', n, ext=True, layout='aos', terminate=False, time_limit=False)
    env_s, _ = H.make_pair('final_cont', n, ext=True, layout='soa', terminate=False, time_limit=False)
    st = H.random_state(rng, n, spread=0.6)
    ctr = np.zeros((2, n), np.int32)
    act = H.random_actions(rng, n, env_a.num_actions)
    nr = rng.uniform(-4, 4, size=(3, n)).astype(np.float32)
    for e in (env_a, env_s):
        e.set_state(H.to_dev(st), H.to_dev(ctr))
    oa, ra, da, _ = env_a.step(H.to_dev(act), new_ref=H.to_dev(nr))
    os_, rs, ds, _ = env_s.step(H.to_dev(act.T.copy()), new_ref=H.to_dev(nr))
    torch.cuda.synchronize()
    assert oa.cpu().numpy().tobytes() == os_.cpu().numpy().T.copy().tobytes()
    assert ra.cpu().numpy().tobytes() == rs.cpu().numpy().tobytes()
    assert da.cpu().numpy().tobytes() == ds.cpu().numpy().tobytes()
    assert env_a.get_state()[0].cpu().numpy().tobytes() == env_s.get_state()[0].cpu().numpy().tobytes()
