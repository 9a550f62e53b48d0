"""The training kernels (dpenv_train.hip, dpenv_train_grad_body.inc: the PPO actor gradient, the critic gradient, the two imitation
gradients, the gated Adam step) on the GPU at the edges of their laws, on the tables of tests/train_edges.py (whose fairness
tests/test_train_edges_cpu.py asserts without a GPU) and under that module's judges, through train.ppo_actor_grad, train.value_grad,
train.imitation_grad and train.adam_step.

A. Shapes at the limits of train_shape_check: in -> out of 1 -> 1, 6 -> 7, 16 -> 7, 9 -> 1 (critics: in of 1, 6, 16), counts 1 and 65, leak 0.2
   and, at in = 16, 0 and 1; 64 sentinel floats behind grad_out and behind the workspace stay as they were.
B. log_std at -18, -14, -4, 1, 5 with W3 = 0: the e^ls / sd factor and the + 1e-8 of sd; W0 .. b2 come out zero.
C. ratio == 1 exactly, with clip 0.2 (a tie inside the band) and clip 0 (a row on both bounds): every row flows with -A / count, clip_frac
   0, mean_ratio 1, approx_kl 0, exactly.  Rows with A = +-0 contribute nothing.
D. Rows within 2^-20 of ratio = 1 +- clip, alone and two in a call of 65: decided where the law decides, either side - with everything
   the row has - where float32 may land on either.  exp(-+200): ratio 0 and +inf.
E. Hidden pre-activations of exactly zero take the slope `leak`, at leak 0.2, 0 and 1.
F. Advantages times 2^-120: subnormal products are kept, not flushed.
G. Adam against train.adam_step_ref bit for bit: zero, subnormal and overflowing gradients and moments, t up to 10^9, eps = 0, lr = 0,
   beta = 0, and the gate on its limit.
Every bound is tests/test_gpu_ppo_update.py's, restated and held in tests/train_edges.py; nothing here introduces a tolerance.  Every measured
figure is printed and appended to the file the environment variable TRAIN_EDGES_RECORD names, if it is set (profiles/train_edges_errors.txt
holds such a record)."""
import numpy as np
import pytest

from ml4ca_amd import train as TR
from tests import train_edges as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def torch_():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


_dev, _refs = {}, {}


def dev(case, key):
    """The device copy of a table's array (made once, never changed)."""
    k = (id(case), key)
    if k not in _dev:
        _dev[k] = (case, torch_().tensor(np.ascontiguousarray(case[key]), device=DEV))        # the case is held: its id stays its own
    return _dev[k][1]


def yard(case, stage, rows):
    """The float32 yardstick on the CPU, once per (table, stage, rows)."""
    k = (id(case), stage, np.asarray(rows).tobytes())
    if k not in _refs:
        _refs[k] = (case, E.torch_law(case, stage, rows, dtype='float32'))
    return _refs[k][1]


def launch(case, stage, rows):
    """One gradient call on the rows `rows` of a table (no index where they are 0 .. count-1), grad_out and the workspace each with
    E.SENTINELS floats behind them that must stay untouched.  Returns the float32 buffer [P + nstat]."""
    torch = torch_()
    rows = np.asarray(rows)
    count = len(rows)
    actor = stage != 'value'
    in_dim, out_dim = case['in_dim'], (case['out_dim'] if actor else 1)
    total = TR.layout(in_dim, out_dim, actor)['P'] + (TR.NSTAT_ACTOR if actor else TR.NSTAT_CRITIC)
    sh = TR.make_shape(in_dim, out_dim, actor, leak=case['leak'])
    assert TR.param_count(sh) + (4 if actor else 1) == total and TR.workspace_bytes(sh, count) == 4 * TR.grid(count) * total
    out_buf = torch.full((total + E.SENTINELS,), E.SENTINEL, device=DEV)
    ws_buf = torch.full((TR.grid(count) * total + E.SENTINELS,), E.SENTINEL, device=DEV)
    out, ws = out_buf[:total], ws_buf[:TR.grid(count) * total]
    idx = None if np.array_equal(rows, np.arange(count)) else torch.tensor(rows.astype(np.int32), device=DEV)
    kw = dict(idx=idx, out=out, workspace=ws, leak=case['leak'], count=count)
    if stage == 'value':
        TR.value_grad(dev(case, 'v_theta'), dev(case, 'obs'), dev(case, 'ret'), **kw)
    elif stage == 'ppo':
        TR.ppo_actor_grad(dev(case, 'pi_theta'), dev(case, 'obs'), dev(case, 'act'), dev(case, 'adv'), dev(case, 'logp_old'), case.get('clip', E.CLIP), **kw)
    else:
        TR.imitation_grad(dev(case, 'pi_theta'), dev(case, 'obs'), dev(case, 'act'), loss=stage, weight=dev(case, 'weight'), **kw)
    got = out_buf.cpu().numpy()
    assert (got[total:] == F32(E.SENTINEL)).all() and bool((ws_buf[TR.grid(count) * total:] == E.SENTINEL).all()), 'a sentinel behind a buffer was written'
    assert not (got[:total] == F32(E.SENTINEL)).any() and not bool((ws == E.SENTINEL).any())                 # ... and the buffers themselves were
    return got[:total].copy()


def parity(what, case, stage, rows, ref64=None):
    actor = stage != 'value'
    sls = E.slices(case['in_dim'], case['out_dim'] if actor else 1, actor)
    got = launch(case, stage, rows)
    ref64 = E.reference(case, stage, rows) if ref64 is None else ref64
    E.judge('%s %s count %d' % (what, stage, len(rows)), got, ref64, yard(case, stage, rows), sls, len(rows), stage, E.stat_scales(case, stage, rows))
    return got


def rows_of(count):
    return np.array([0]) if count == 1 else np.arange(65)


# ---- A ----
@pytest.mark.parametrize('shape', E.A_ACTORS)
def test_a_actor_shapes(shape):
    case = E.table_a(*shape)
    for stage in E.ACTOR_STAGES:
        for count in E.COUNTS:
            got = parity('A %d->%d leak %.1f' % shape, case, stage, rows_of(count))
            if stage == 'mse':
                assert not got[-4 - shape[1]:-4].view(np.int32).any()          # MSE's log_std gradient: +0.0 as bits (the header's promise)


@pytest.mark.parametrize('shape', E.A_CRITICS)
def test_a_critic_shapes(shape):
    case = E.critic_case(*shape)
    for count in E.COUNTS:
        parity('A %d->1 leak %.1f' % shape, case, 'value', rows_of(count))


# ---- B ----
@pytest.mark.parametrize('log_std', E.B_LOG_STDS)
def test_b_log_std(log_std):
    """W0 .. b2 have a zero reference and must be zero as a VALUE (+0.0 or -0.0): the header promises no sign of a zero gradient, and the
    float32 yardstick itself returns -0.0 there (tests/train_edges.py, THE BOUND)."""
    case = E.table_b(log_std)
    for stage in E.B_STAGES:
        for count in E.COUNTS:
            got = parity('B log_std %g' % log_std, case, stage, rows_of(count))
            for name, sl in E.slices(9, 7):
                assert (name in E.below_b3()) == (not got[sl].any()), (log_std, stage, count, name)


# ---- C ----
@pytest.mark.parametrize('clip', E.C_CLIPS)
def test_c_ties(clip):
    case = E.table_c(clip)
    for count in E.COUNTS:
        rows = rows_of(count)
        ref = E.reference(case, 'ppo', rows, ratio=1.0)           # the header's law with the ratio the float32 arithmetic forms
        ref[1][1] = 0.0                                           # logp_old is the float32 logp: approx_kl is +0
        assert ref[1][2] == 0.0 and ref[1][3] == 1.0 and ref[1][0] == -case['adv'][rows].astype(F64).mean()
        got = parity('C clip %g' % clip, case, 'ppo', rows, ref64=ref)
        assert got[-3] == 0.0 and got[-2] == 0.0 and got[-1] == 1.0, got[-4:]     # approx_kl, clip_frac, mean_ratio: exactly (the judge asked already)


@pytest.mark.parametrize('all_zero', (False, True))
def test_c_zero_advantages(all_zero):
    case = E.table_c_zero_adv(all_zero)
    got = parity('C zero advantages%s' % (', all' if all_zero else ''), case, 'ppo', np.arange(65))
    if all_zero:
        assert not got[:-3].any()                                 # every tensor and pi_loss
        rows = np.array(E.C_PLUS_ZERO[:1] + E.C_MINUS_ZERO[:1])
        assert not parity('C zero advantages, two rows', case, 'ppo', rows)[:-3].any()


# ---- D ----
@pytest.mark.parametrize('k', range(len(E.D_SINGLE)))
def test_d_single_rows_at_a_bound(k):
    bound, a, ambiguous = E.D_SINGLE[k]
    case = E.table_d()
    rows = np.array([65 + k])
    flows, outside = E.judge_either_side('D %s bound A %+g' % (bound, a), launch(case, 'ppo', rows), case, rows, (0,), E.slices(9, 7))
    assert flows[0] or ambiguous


def test_d_two_ambiguous_rows_in_a_call():
    case = E.table_d()
    E.judge_either_side('D call of 65', launch(case, 'ppo', E.D_CALL_ROWS), case, E.D_CALL_ROWS, E.D_CALL_BAND, E.slices(9, 7))


@pytest.mark.parametrize('row', range(len(E.D_EXTREME)))
def test_d_ratio_beyond_float32(row):
    case = E.table_d_extreme()
    E.judge_extreme('D logp - logp_old %+g A %+g' % E.D_EXTREME[row], launch(case, 'ppo', np.array([row])), case, row)


# ---- E ----
@pytest.mark.parametrize('leak', E.E_LEAKS)
@pytest.mark.parametrize('kind', E.E_KINDS)
def test_e_zero_preactivations(kind, leak):
    case = E.table_e(kind, leak)
    for stage in E.E_STAGES:
        for rows in (np.array([64]), np.arange(65)):
            parity('E %s leak %.1f' % (kind, leak), case, stage, rows)      # a tensor the reference has at zero is asked to be zero by the judge


# ---- F ----
def test_f_subnormal_products():
    base, case = E.table_a(9, 7, 0.2), E.table_f()
    g, s = E.reference(case, 'ppo')
    s = s.copy()
    s[0] /= E.F_SCALE
    got = launch(case, 'ppo', np.arange(65))
    E.judge('F advantages x 2^-120', got, (g / E.F_SCALE, s), yard(base, 'ppo', np.arange(65)), E.slices(9, 7), 65, 'ppo', E.stat_scales(case, 'ppo'),
            rescale=1.0 / E.F_SCALE)
    assert (np.abs(got[:-4]) < F32(2.0 ** -126)).mean() > 0.2 and (got[:-4] != 0).mean() > 0.99       # subnormal outputs, and they are there


# ---- G ----
def adam_launch(tab, t, gate_kl=None, kl_limit=float('inf'), stop=0, **hyper):
    torch = torch_()
    h = dict(E.G_DEFAULTS, **hyper)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    th, g, m, v = T(tab['theta']), T(tab['grad']), T(tab['m']), T(tab['v'])
    ctr, flag = torch.full((1,), t - 1, dtype=torch.int32, device=DEV), torch.full((1,), int(stop), dtype=torch.int32, device=DEV)
    kl = None if gate_kl is None else T(np.array([gate_kl], F32))
    TR.adam_step(th, g, m, v, ctr, h['lr'], h['beta1'], h['beta2'], h['eps'], gate_kl=kl, kl_limit=kl_limit, stop_flag=None if kl is None else flag)
    assert np.array_equal(g.cpu().numpy().view(np.int32), tab['grad'].view(np.int32))
    return th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), int(ctr), int(flag)


@pytest.mark.parametrize('t', E.G_STEPS)
def test_g_adam_table(t):
    tab = E.table_g()
    E.judge_adam('G t %d' % t, adam_launch(tab, t), E.adam_statement(tab, t))


@pytest.mark.parametrize('hyper', E.G_SINGLE, ids=lambda h: '%s=%g' % next(iter(h.items())))
def test_g_adam_single_parameter(hyper):
    tab = E.table_g()
    for t in (1, 1000):
        E.judge_adam('G %s t %d' % (hyper, t), adam_launch(tab, t, **hyper), E.adam_statement(tab, t, **hyper))


def test_g_adam_gate():
    tab = E.table_g()
    for name, kl, limit, flag in E.gate_cases():
        E.judge_adam('G gate %s' % name, adam_launch(tab, 3, gate_kl=kl, kl_limit=limit, stop=flag), E.adam_statement(tab, 3, gate_kl=kl, kl_limit=limit, stop=flag))
