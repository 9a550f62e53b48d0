"""The PPO update's host statements (ml4ca_amd/train.py) against torch on the CPU, the conditions of the fixture the GPU tests share
(tests/ppo_fixture.py), the argument validation of the C entry points (a refused call launches nothing, so it needs no GPU) and the
ISA of the training unit."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ml4ca_amd import _lib
from ml4ca_amd import train as TR
from tests import ppo_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAKS = (0.2, 0.0)
_fx = {}


def fixture(leak):
    if leak not in _fx:
        _fx[leak] = F.make_fixture(257, leak)
    return _fx[leak]


@pytest.mark.parametrize('leak', LEAKS)
def test_closed_form_equals_float64_autograd(leak):
    fx = fixture(leak)
    g, s = TR.ppo_actor_grad_ref(fx['pi_theta'], fx['obs'], fx['act'], fx['adv'], fx['logp_old'], F.CLIP, leak=leak)
    vg, vs = TR.value_grad_ref(fx['v_theta'], fx['obs'], fx['ret'], leak=leak)
    pg, ps, tvg, tvs = F.torch_grads(fx)
    assert g.shape == (14334,) and vg.shape == (13841,)          # the numbers in dist.average_gradients' docstring
    for actor, got, ref in ((True, g, pg), (False, vg, tvg)):
        for name, err in F.tensor_errors(got, ref, actor).items():
            assert err <= 1e-12, (actor, name, err)
    assert np.abs(s - ps).max() <= 1e-12 and abs(vs[0] - tvs[0]) <= 1e-12
    assert s[2] == ps[2]


def torch_ratio(fx):
    """The ratio per row as torch's float64 forward pass evaluates it."""
    from ml4ca_amd.policy import ActorCritic
    ac = ActorCritic(9, 7, (80, 80, 80), leak=fx['leak'])
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    pW, pb, pls = TR.unflatten(fx['pi_theta'], 9, 7, True)
    ac.pi_W, ac.pi_b, ac.log_std = [t64(w) for w in pW], [t64(b) for b in pb], t64(pls)
    logp = ac.logp_ref(t64(fx['act']), ac._mlp(t64(fx['obs']), ac.pi_W, ac.pi_b))
    return torch.exp(logp - t64(fx['logp_old'])).numpy()


@pytest.mark.parametrize('side', ('upper', 'lower'))
@pytest.mark.parametrize('leak', LEAKS)
def test_tie_rule_rows_exactly_on_a_bound_and_zero_advantage(leak, side):
    """Rows with ratio == 1 + clip (or 1 - clip) bit for bit in the closed form's AND in torch's evaluation, with advantages of both signs,
    and rows with A == 0: torch.minimum splits a tie half and half and torch.clamp passes its gradient at the bounds, bounds included,
    which adds up to the header's rule `s1 <= s2`.  The bound is put ON a row: clip = |ratio - 1| of a row both sides evaluate to the same
    bits (1 + (r - 1) and 1 - (1 - r) are exact for r in [0.5, 2]), and that row is copied to eight places."""
    fx = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fixture(leak).items()}
    _, _, _, r_np = TR.ppo_actor_grad_ref(fx['pi_theta'], fx['obs'], fx['act'], fx['adv'], fx['logp_old'], F.CLIP, leak=leak, hidden_z=True)
    r_t = torch_ratio(fx)
    same = (r_np == r_t) & ((r_np > 1.05) & (r_np < 1.6) if side == 'upper' else (r_np < 0.95) & (r_np > 0.6))
    assert same.any()
    row = int(np.flatnonzero(same)[0])
    clip = float(r_np[row] - 1.0) if side == 'upper' else float(1.0 - r_np[row])
    bound = 1.0 + clip if side == 'upper' else 1.0 - clip
    assert bound == r_np[row]
    for k in ('obs', 'act', 'logp_old'):
        fx[k][:8] = fx[k][row]
    fx['adv'][:8] = np.array([0.7, -0.3, 1.3, -0.9, 0.1, -0.2, 2.0, -1.1], np.float32)      # both signs, not cancelling
    fx['adv'][96:128] = 0.0
    g, s, _, ratio = TR.ppo_actor_grad_ref(fx['pi_theta'], fx['obs'], fx['act'], fx['adv'], fx['logp_old'], clip, leak=leak, hidden_z=True)
    assert (ratio[:8] == bound).all() and (torch_ratio(fx)[:8] == bound).all()          # the rows sit on the bound on both sides
    pg, ps, _, _ = F.torch_grads(fx, clip=clip)
    for name, err in F.tensor_errors(g, pg, True).items():
        assert err <= 1e-12, (name, err)
    assert np.abs(s - ps).max() <= 1e-12
    # and the rule is not vacuous here: dropping the tie rows' gradient (a strict `s1 < s2`) changes the answer
    strict = fx['adv'].copy()
    strict[:8] = 0.0
    g0, _ = TR.ppo_actor_grad_ref(fx['pi_theta'], fx['obs'], fx['act'], strict, fx['logp_old'], clip, leak=leak)
    assert max(F.tensor_errors(g0, pg, True).values()) > 1e-3


@pytest.mark.parametrize('leak', LEAKS)
def test_fixture_conditions(leak):
    fx = fixture(leak)
    n = fx['obs'].shape[0]
    _, stats, zs, ratio = TR.ppo_actor_grad_ref(fx['pi_theta'], fx['obs'], fx['act'], fx['adv'], fx['logp_old'], F.CLIP, leak=leak, hidden_z=True)
    A = fx['adv'].astype(np.float64)
    assert (A > 0).sum() >= n / 4 and (A < 0).sum() >= n / 4
    outside = (ratio > 1 + F.CLIP) | (ratio < 1 - F.CLIP)                              # clip_frac's rows
    cut = ratio * A > np.clip(ratio, 1 - F.CLIP, 1 + F.CLIP) * A                       # rows whose gradient the clip removes
    assert 0.2 <= outside.mean() <= 0.8 and 0.2 <= cut.mean() <= 0.8, (outside.mean(), cut.mean())
    assert np.abs(ratio - (1 + F.CLIP)).min() >= F.RATIO_MARGIN and np.abs(ratio - (1 - F.CLIP)).min() >= F.RATIO_MARGIN
    _, _, _, _, vzs, _ = TR._forward64(fx['v_theta'], fx['obs'], 9, 1, False, leak)
    for z in list(zs) + list(vzs):
        assert np.abs(z).min() >= F.Z_MARGIN
    assert not F.offending_rows(fx).any()
    # rows 0 and 64 (count 1 and the second workgroup of count 65 without an index) carry an actor gradient; both kinds of row exist
    assert not F.cut_rows(fx)[0] and not F.cut_rows(fx)[64] and F.cut_rows(fx).any()
    assert np.array_equal(F.cut_rows(fx), cut)
    for k in ('obs', 'act', 'adv', 'ret', 'logp_old', 'pi_theta', 'v_theta'):
        assert fx[k].dtype == np.float32
    # the same call gives the same fixture (the GPU tests build their own copy)
    again = F.make_fixture(257, leak)
    assert all(np.array_equal(fx[k], again[k]) for k in ('obs', 'act', 'adv', 'ret', 'logp_old', 'pi_theta', 'v_theta'))


def adam_case(P, seed=0):
    rng = np.random.RandomState(1000 * seed + P)
    # parameters away from zero: "2 ulp of the parameter" is a statement about the update's last rounding, not about cancellation
    theta = (rng.uniform(0.05, 1.0, P) * rng.choice([-1.0, 1.0], P)).astype(np.float32)
    grads = [rng.normal(0.0, 1.0, P).astype(np.float32) for _ in range(5)]
    return theta, grads


@pytest.mark.parametrize('P', (1, 255, 257, 14334))
def test_adam_statement_against_torch_optim_adam(P):
    theta, grads = adam_case(P)
    p = torch.tensor(theta.copy(), requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    th, m, v, step = theta.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32), 0
    for g in grads:
        p.grad = torch.tensor(g.copy())
        opt.step()
        th, m, v, step, stop = TR.adam_step_ref(th, g, m, v, step, 1e-3)
        want = p.detach().numpy()
        assert (np.abs(th - want) <= 2 * np.spacing(np.abs(want))).all(), float((np.abs(th - want) / np.spacing(np.abs(want))).max())
    assert step == 5 and stop == 0 and th.dtype == np.float32


def test_fma_statement_is_correctly_rounded():
    rng = np.random.RandomState(3)
    a, b, c = (rng.normal(0, 1, 20000).astype(np.float32) for _ in range(3))
    c[:5000] = (-(a[:5000].astype(np.float64) * b[:5000])).astype(np.float32)          # cancellation: the product's low bits decide
    from fractions import Fraction
    got = TR._fma32(a, b, c)
    for i in list(range(0, 20000, 97)) + list(range(0, 5000, 13)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                         # float(Fraction) rounds correctly to float64 ...
        # ... so compare against the two float32 neighbours of the exact value directly
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.float32(x).view(np.int32)) & 1))
        assert got[i] == best, (i, got[i], best)


def kl_of(theta, theta0):
    return np.float32(1e-3 + np.mean((theta.astype(np.float64) - theta0) ** 2) * 1e4)        # positive from the start, growing with every step


def gated_run(theta0, g, limit, steps=5):
    th, m, v, step, stop = theta0.copy(), np.zeros_like(theta0), np.zeros_like(theta0), 0, 0
    kls = []
    for _ in range(steps):
        kl = kl_of(th, theta0)
        kls.append(float(kl))
        th, m, v, step, stop = TR.adam_step_ref(th, g, m, v, step, 1e-3, gate_kl=kl, kl_limit=limit, stop=stop)
    return th, m, v, step, stop, kls


def test_adam_gate_on_the_statement():
    theta0, grads = adam_case(257)
    g = grads[0]
    th, m, v, step, stop, _ = gated_run(theta0, g, 0.0)        # limit 0: nothing changes, flag set, counter 0
    assert np.array_equal(th, theta0) and not m.any() and not v.any() and (step, stop) == (0, 1)
    th_all, _, _, step, stop, kls = gated_run(theta0, g, float('inf'))
    assert (step, stop) == (5, 0) and kls == sorted(kls) and kls[1] < kls[2]
    th2, m2, v2, step, stop, _ = gated_run(theta0, g, 0.5 * (kls[1] + kls[2]))         # between the KLs of steps 2 and 3 of the ungated run
    assert (step, stop) == (2, 1)
    ref = (theta0.copy(), np.zeros_like(theta0), np.zeros_like(theta0), 0)
    for _ in range(2):
        ref = TR.adam_step_ref(ref[0], g, ref[1], ref[2], ref[3], 1e-3)[:4]
    assert np.array_equal(th2, ref[0]) and np.array_equal(m2, ref[1]) and np.array_equal(v2, ref[2])


# ---- the C entry points' validation: refused before any device call, so this runs without a GPU ----
def _shape(**kw):
    return TR.make_shape(kw.pop('in_dim', 9), kw.pop('out_dim', 7), kw.pop('actor', True), **kw)


def test_param_counts_and_workspace():
    assert TR.param_count(_shape()) == 14334 == TR.layout(9, 7, True)['P']
    assert TR.param_count(_shape(out_dim=1, actor=False)) == 13841 == TR.layout(9, 1, False)['P']
    assert TR.param_count(_shape(in_dim=6)) == 14334 - 3 * 80
    assert TR.workspace_bytes(_shape(), 1) == 4 * 14338 and TR.workspace_bytes(_shape(), 65) == 2 * 4 * 14338
    assert TR.workspace_bytes(_shape(), 1 << 20) == 256 * 4 * 14338                     # the grid is capped
    assert [TR.grid(c) for c in (1, 64, 65, 128, 129, 16384, 16385)] == [1, 1, 2, 2, 3, 256, 256]


def test_refusals_launch_nothing_and_name_the_reason():
    lib = _lib.load()
    fake = C.c_void_p(4096)                                    # never dereferenced: every one of these calls is refused on the host
    good = _shape()

    def actor(shape=good, theta=fake, obs=fake, act=fake, adv=fake, lpo=fake, idx=None, count=64, n_rows=64, clip=0.2, out=fake, ws=fake, ws_bytes=1 << 20):
        return lib.dpenv_ppo_actor_grad(C.byref(shape), theta, obs, act, adv, lpo, idx, count, n_rows, clip, None, out, ws, ws_bytes, None)

    def critic(shape, count=64, n_rows=64, ws_bytes=1 << 20, obs=fake):
        return lib.dpenv_value_grad(C.byref(shape), fake, obs, fake, None, count, n_rows, fake, fake, ws_bytes, None)

    def refused(fn, word):
        assert fn() == _lib.EINVAL
        assert word in lib.dpenv_last_error(None), (word, lib.dpenv_last_error(None))

    vshape = _shape(out_dim=1, actor=False)
    refused(lambda: actor(count=0), b'count')
    refused(lambda: actor(count=-3), b'count')
    refused(lambda: actor(count=2 ** 31 - 1, n_rows=2 ** 31 - 1, ws_bytes=1 << 40), b'at most')      # no 32-bit overflow of the grid behind the check
    out = C.c_int64(-7)
    assert lib.dpenv_train_workspace_bytes(C.byref(good), 2 ** 31 - 1, C.byref(out)) == _lib.EINVAL and out.value == -7
    assert lib.dpenv_train_workspace_bytes(C.byref(good), 2 ** 30, C.byref(out)) == _lib.OK and out.value == 256 * 4 * 14338
    for kw in ({'theta': None}, {'obs': None}, {'act': None}, {'adv': None}, {'lpo': None}, {'out': None}):
        refused(lambda: actor(**kw), b'NULL')
    refused(lambda: actor(ws=None), b'workspace')
    refused(lambda: actor(count=65, n_rows=65, ws_bytes=4 * 14338), b'workspace')       # one workgroup's worth for a two-workgroup count
    refused(lambda: actor(shape=_shape(activation='tanh')), b'tanh')
    refused(lambda: actor(shape=_shape(hidden=(64, 64, 64))), b'80 wide')
    refused(lambda: actor(shape=_shape(hidden=(80, 80))), b'n_layers')
    refused(lambda: actor(shape=_shape(in_dim=17)), b'input width')
    refused(lambda: actor(shape=_shape(out_dim=8)), b'output width')
    refused(lambda: actor(shape=_shape(row_dtype=_lib.BF16)), b'bf16')
    refused(lambda: actor(shape=_shape(leak=1.5)), b'leak')
    refused(lambda: actor(idx=fake, count=8, n_rows=0), b'n_rows')
    refused(lambda: actor(idx=fake, count=8, n_rows=-1), b'n_rows')
    refused(lambda: actor(count=64, n_rows=32), b'n_rows')
    refused(lambda: actor(clip=float('nan')), b'clip')
    refused(lambda: actor(shape=vshape), b'log_std')
    refused(lambda: critic(vshape, count=0), b'count')
    refused(lambda: critic(vshape, obs=None), b'NULL')
    refused(lambda: critic(vshape, ws_bytes=16), b'workspace')
    refused(lambda: critic(_shape(out_dim=2, actor=False)), b'output width')
    refused(lambda: critic(good), b'log_std')

    def adam(theta=fake, grad=fake, m=fake, v=fake, P=16, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, ctr=fake, kl=None, limit=0.0, flag=None):
        return lib.dpenv_adam_step(theta, grad, m, v, P, lr, b1, b2, eps, ctr, kl, limit, flag, None)

    refused(lambda: adam(theta=None), b'NULL')
    refused(lambda: adam(ctr=None), b'NULL')
    refused(lambda: adam(P=0), b'P = 0')
    refused(lambda: adam(m=C.c_void_p(4100)), b'aligned')
    refused(lambda: adam(b1=1.0), b'beta1')
    refused(lambda: adam(kl=fake), b'stop_flag')
    out = C.c_int64(-7)
    assert lib.dpenv_train_workspace_bytes(C.byref(good), 0, C.byref(out)) == _lib.EINVAL and out.value == -7
    assert lib.dpenv_train_param_count(C.byref(_shape(activation='tanh'))) == _lib.EINVAL


def test_training_unit_is_built_like_the_library():
    """tests/test_abi_cpu.py scans the units of the Makefile's SRC list; the training unit is listed beside it (SRC_TRAIN) and gets the same
    scan here: the library's flags, no packed fp32 arithmetic, the exact-f32 matrix instruction on the hot path and no scratch."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    csrc = os.path.join(ROOT, 'ml4ca_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1).split()
    assert '-fno-slp-vectorize' in flags and '-ffp-contract=off' in flags
    assert re.search(r'^SRC_TRAIN := (.*)$', mk, re.M).group(1).split() == ['dpenv_train.hip']
    assert '$(SRC) $(SRC_TRAIN)' in mk
    asm = subprocess.run([hipcc, '--offload-arch=gfx950'] + flags + ['--cuda-device-only', '-S', '-o', '-', os.path.join(csrc, 'dpenv_train.hip')],
                         check=True, capture_output=True, text=True).stdout
    assert not re.findall(r'\bv_pk_\w+', asm)
    assert asm.count('v_mfma_f32_16x16x4_f32') > 1000 and 'v_fma_f32' in asm
    for k in ('mlp_grad_kernelILb1', 'mlp_grad_kernelILb0', 'adam_step_kernel', 'adam_commit_kernel', 'grad_reduce_kernel'):
        assert k in asm, k
    assert set(re.findall(r'\.private_segment_fixed_size:\s*(\d+)', asm)) == {'0'}
