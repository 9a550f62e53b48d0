"""Case tables, float64 references, bounds and judges for the training kernels (dpenv_train.hip, dpenv_train_grad_body.inc: the PPO actor
gradient, the critic gradient, the two imitation gradients, the gated Adam step) at the edges of their laws.  Not collected:
tests/test_train_edges_cpu.py asserts of these tables and judges everything tests/test_gpu_train_edges.py relies on - that the tables
reach what they name, that the references are fair, that torch float32 passes and that a mutant of each group does not - and the GPU file
puts the kernels in the judged place.  No GPU here and no torch at import (the yardstick imports it when called).

THE BOUND is tests/test_gpu_ppo_update.py's and no other: error per parameter tensor relative to that tensor's largest float64 value, allowed
max(8 x the same error of torch float32 autograd on the same rows, chain_K(count) x 2^-24); chain_K is that file's for the PPO and value
stages and tests/test_gpu_imitation.py's for the imitation stages (both restated below; the CPU file holds them to the originals).  The
input and output layers are padded to 16 whatever in and out are, so K does not depend on the widths.  Statistics carry the scales of
stat_scales (PPO: 2 max|A|, max|logp_old|, -, 2) and of the imitation file (max|w| max|logp|, max|w| max se); v_loss is its own scale;
clip_frac is a count and exact.  A tensor or statistic whose reference is exactly zero must come out zero: as a VALUE, +0.0 or -0.0 - the
header promises no sign of a zero gradient, and torch float32 autograd, which must pass in the kernel's place, returns -0.0 where a zero
output gradient meets a negative activation.

THE LAW is include/dpenv.h's, evaluated in float64 by the closed forms of ml4ca_amd/train.py (ppo_actor_grad_ref, imitation_grad_ref,
value_grad_ref).  actor_law / value_law below are the same closed forms with the knobs the tables and the mutants need - a given ratio
(group C), a given set of rows that flow (group D), and the errors a kernel could make - and the CPU file holds their default form to
train.py's.  The yardstick is torch_law: a small torch MLP for any (in, out, leak) in float32 or float64, the loss written as the header
writes it (the log-probability summed over j from 0, so that its float32 form is the header's operation order).

GROUPS (the issue's letters).  A shapes at the limits of train_shape_check.  B log_std at -18, -14, -4, 1, 5 on an actor with W3 = 0 (mu =
b3 in both arithmetics).  C the clip rule's ties, exactly: ratio == 1.0f by construction.  D rows within 2^-20 of ratio = 1 +- clip, and
ratios beyond float32's range.  E hidden pre-activations of exactly zero.  F advantages times 2^-120.  G Adam, bit for bit."""
import math
import os

import numpy as np

from ml4ca_amd import train as TR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
HIDDEN = TR.HIDDEN
CLIP = 0.2
RATIO_MARGIN, Z_MARGIN = 1e-4, 1e-5                      # tests/ppo_fixture.py's margins from the two kinds of kink
BAND = 2.0 ** -20                                       # group D: |ratio / bound - 1| below this
LOG_2PI = math.log(2.0 * math.pi)
RECORD = os.environ.get('TRAIN_EDGES_RECORD', '')        # a path: every measured figure is appended there
SENTINELS, SENTINEL = 64, -77.25                         # floats behind grad_out and behind the workspace, and what they hold


def ceil_div(a, b):
    return -(-int(a) // int(b))


def chain_K(count, stage='ppo'):
    """Roundings along the longest accumulation chain of a gradient element: tests/test_gpu_ppo_update.py's chain_K, and for the imitation
    stages tests/test_gpu_imitation.py's (the output-gradient term 14 instead of 20)."""
    g = TR.grid(count)
    K = (16 + 1) + 3 * (80 + 1) + 20 + (16 + 80 + 80) + 64 * ceil_div(ceil_div(count, 64), g) + g + 1
    return K - 20 + 14 if stage in ('nll', 'mse') else K


def floor(count, stage='ppo'):
    return chain_K(count, stage) * U


def slices(in_dim, out_dim, actor=True):
    """[(name, slice)] of a flat parameter vector."""
    L = TR.layout(in_dim, out_dim, actor)
    s = L['sizes']
    out = []
    for i in range(4):
        out.append(('W%d' % i, slice(L['W'][i], L['W'][i] + s[i] * s[i + 1])))
        out.append(('b%d' % i, slice(L['b'][i], L['b'][i] + s[i + 1])))
    if actor:
        out.append(('log_std', slice(L['log_std'], L['log_std'] + s[4])))
    return out


# ---- the law in float64, with knobs ---------------------------------------------------------------------------------------------------
def backward64(Ws, hs, zs, dout, leak, extra=None, slope_at_zero=None):
    """train._backward64 with the slope at z == 0 as a knob (None: leak, the header's)."""
    s0 = leak if slope_at_zero is None else slope_at_zero
    gW, gb = [None] * 4, [None] * 4
    g = dout
    for i in (3, 2, 1, 0):
        gW[i] = hs[i].T @ g
        gb[i] = g.sum(0)
        if i > 0:
            z = zs[i - 1]
            g = (g @ Ws[i].T) * np.where(z > 0, 1.0, np.where(z == 0, s0, leak))
    return TR.flatten(gW, gb, extra)


def actor_law(theta, obs, act, adv, logp_old, clip, leak, stage='ppo', weight=None, ratio=None, flows=None, outside=None, sd_eps=1e-8, ls_factor=True,
              strict_tie=False, clip_frac_ge=False, slope_at_zero=None):
    """The header's actor law in float64: (grad [P], stats [4]).  stage 'ppo' (adv, logp_old, clip), 'nll' or 'mse' (weight or None).
    The knobs, every default being the header:
      ratio          the per-row ratio to use instead of exp(logp - logp_old) (group C: the ratio the float32 arithmetic forms)
      flows, outside a bool per row each: the rows whose gradient flows, instead of s1 <= s2, and the rows clip_frac counts, instead of
                     ratio > 1 + clip or ratio < 1 - clip (group D: a float32 ratio may land on either side of a bound it is next to)
      sd_eps, ls_factor, strict_tie, clip_frac_ge, slope_at_zero      what a wrong kernel would compute (the CPU file's mutants)."""
    obs, act = np.asarray(obs, F64), np.asarray(act, F64)
    count, in_dim, out_dim = obs.shape[0], obs.shape[1], act.shape[1]
    Ws, bs, ls, hs, zs, mu = TR._forward64(theta, obs, in_dim, out_dim, True, leak)
    sd = np.exp(ls) + sd_eps
    q = (act - mu) / sd
    logp = (-0.5 * ((q * q + 2.0 * ls) + LOG_2PI)).sum(1)
    dlogp_dmu = q / sd
    dlogp_dls = q * q * (np.exp(ls) / sd if ls_factor else 1.0) - 1.0
    if stage == 'ppo':
        A, lpo = np.asarray(adv, F64), np.asarray(logp_old, F64)
        r = np.exp(logp - lpo) if ratio is None else np.broadcast_to(np.asarray(ratio, F64), (count,))
        lo, hi = 1.0 - clip, 1.0 + clip
        s1, s2 = r * A, np.minimum(np.maximum(r, lo), hi) * A
        rule = (s1 < s2) if strict_tie else (s1 <= s2)
        out = ((r >= hi) | (r <= lo)) if clip_frac_ge else ((r > hi) | (r < lo))
        rule = rule if flows is None else np.asarray(flows, bool)
        outside = out if outside is None else np.asarray(outside, bool)
        gl = np.where(rule, -A * r, 0.0) / count
        dmu = gl[:, None] * dlogp_dmu
        dls = (gl[:, None] * dlogp_dls).sum(0)
        stats = np.array([(-np.minimum(s1, s2)).mean(), (lpo - logp).mean(), outside.mean(), r.mean()])
    else:
        w = np.ones(count) if weight is None else np.asarray(weight, F64)
        e = mu - act
        nll, mse = (w * -logp).sum() / count, (w * (e * e).sum(1)).sum() / count
        if stage == 'nll':
            gl = -w / count
            dmu, dls = gl[:, None] * dlogp_dmu, (gl[:, None] * dlogp_dls).sum(0)
        elif stage == 'mse':
            dmu, dls = (2.0 * w / count)[:, None] * e, np.zeros(out_dim)
        else:
            raise ValueError(stage)
        stats = np.array([nll if stage == 'nll' else mse, nll, mse, 0.0])
    return backward64(Ws, hs, zs, dmu, leak, dls, slope_at_zero), stats


def value_law(theta, obs, ret, leak, slope_at_zero=None):
    obs, ret = np.asarray(obs, F64), np.asarray(ret, F64)
    count = obs.shape[0]
    Ws, bs, _, hs, zs, out = TR._forward64(theta, obs, obs.shape[1], 1, False, leak)
    e = out[:, 0] - ret
    return backward64(Ws, hs, zs, (2.0 * e / count)[:, None], leak, None, slope_at_zero), np.array([(e * e).mean()])


def reference(case, stage, rows=None, **knobs):
    """(grad, stats) of the float64 law for the rows `rows` of a case (None: all of them)."""
    r = slice(None) if rows is None else np.asarray(rows)
    if stage == 'value':
        return value_law(case['v_theta'], case['obs'][r], case['ret'][r], case['leak'], **knobs)
    w = case.get('weight')
    return actor_law(case['pi_theta'], case['obs'][r], case['act'][r], case['adv'][r], case['logp_old'][r], case.get('clip', CLIP), case['leak'],
                     stage=stage, weight=None if (w is None or stage == 'ppo') else w[r], **knobs)


def closed_form(case, stage, rows=None):
    """The same through ml4ca_amd/train.py's closed forms, the references the issue names."""
    r = slice(None) if rows is None else np.asarray(rows)
    if stage == 'value':
        return TR.value_grad_ref(case['v_theta'], case['obs'][r], case['ret'][r], leak=case['leak'])
    if stage == 'ppo':
        return TR.ppo_actor_grad_ref(case['pi_theta'], case['obs'][r], case['act'][r], case['adv'][r], case['logp_old'][r], case.get('clip', CLIP),
                                     leak=case['leak'])
    w = case.get('weight')
    return TR.imitation_grad_ref(case['pi_theta'], case['obs'][r], case['act'][r], stage, weight=None if w is None else w[r], leak=case['leak'])


# ---- the yardstick: a torch MLP of any (in, out, leak), float32 or float64 --------------------------------------------------------------
def torch_law(case, stage, rows=None, dtype='float64'):
    """(grad [P], stats) as NumPy float64 from torch autograd in `dtype` on the CPU.  The loss as the header writes it; the log-probability
    is summed over j from 0, one addition per component, so its float32 form has the header's operation order."""
    import torch
    dt = getattr(torch, dtype)
    r = slice(None) if rows is None else np.asarray(rows)
    actor = stage != 'value'
    in_dim, out_dim = case['obs'].shape[1], (case['act'].shape[1] if actor else 1)
    leaf = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dt).requires_grad_(True)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dt)
    Ws, bs, ls = TR.unflatten(np.asarray(case['pi_theta' if actor else 'v_theta']), in_dim, out_dim, actor)
    Ws, bs = [leaf(w) for w in Ws], [leaf(b) for b in bs]
    x = T(case['obs'][r])
    n = x.shape[0]
    for W, b in zip(Ws[:-1], bs[:-1]):
        x = torch.nn.functional.leaky_relu(x @ W + b, float(case['leak']))
    out = x @ Ws[-1] + bs[-1]
    if not actor:
        e = out[:, 0] - T(case['ret'][r])
        loss = (e * e).mean()
        loss.backward()
        stats = np.array([float(loss.detach())])
        ls = None
    else:
        ls = leaf(ls)
        a = T(case['act'][r])
        q = (a - out) / (torch.exp(ls) + 1e-8)
        terms = -0.5 * ((q * q + 2 * ls) + LOG_2PI)
        logp = terms[:, 0]
        for j in range(1, out_dim):
            logp = logp + terms[:, j]
        if stage == 'ppo':
            A, lpo, clip = T(case['adv'][r]), T(case['logp_old'][r]), case.get('clip', CLIP)
            ratio = torch.exp(logp - lpo)
            s1 = ratio * A
            loss = -torch.min(s1, torch.clamp(ratio, 1 - clip, 1 + clip) * A).mean()
            loss.backward()
            with torch.no_grad():
                stats = np.array([float(loss), float((lpo - logp).mean()), float(((ratio > 1 + clip) | (ratio < 1 - clip)).to(dt).mean()),
                                  float(ratio.mean())])
        else:
            w = case.get('weight')
            w = torch.ones(n, dtype=dt) if w is None else T(w[r])
            nll = -(w * logp).mean()
            mse = (w * ((out - a) ** 2).sum(dim=1)).mean()
            chosen = nll if stage == 'nll' else mse
            chosen.backward()
            stats = np.array([float(chosen.detach()), float(nll.detach()), float(mse.detach()), 0.0])
    g = lambda p: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().numpy()
    return TR.flatten([g(p) for p in Ws], [g(p) for p in bs], None if ls is None else g(ls)), stats


# ---- the judges -----------------------------------------------------------------------------------------------------------------------
def rel_errors(got, ref, sls):
    """Per tensor max |got - ref| / max |ref|; a tensor whose reference is all zero must be all zero (inf otherwise)."""
    out = {}
    got = np.asarray(got, F64)
    for name, sl in sls:
        scale = np.abs(ref[sl]).max()
        if not np.isfinite(got[sl]).all():
            out[name] = float('inf')
            continue
        d = np.abs(got[sl] - ref[sl]).max()
        out[name] = (d / scale) if scale > 0 else (0.0 if d == 0 else float('inf'))
    return out


def stat_names(stage):
    return {'ppo': ('pi_loss', 'approx_kl', 'clip_frac', 'mean_ratio'), 'value': ('v_loss',)}.get(stage, ('loss', 'nll', 'mse', 'reserved'))


def stat_scales(case, stage, rows=None):
    """The input-sized number behind each statistic (tests/test_gpu_ppo_update.py's stat_scales, tests/test_gpu_imitation.py's): pi_loss 2
    max|A| (ratio < 2), approx_kl max|logp_old|, mean_ratio 2; the weighted NLL max|w| max|logp|, the weighted MSE max|w| max se; None
    where the statistic is its own scale (v_loss) or exact (clip_frac, the reserved slot)."""
    r = slice(None) if rows is None else np.asarray(rows)
    if stage == 'value':
        return (None,)
    if stage == 'ppo':
        return (2.0 * float(np.abs(case['adv'][r]).max()), float(np.abs(case['logp_old'][r]).max()), None, 2.0)
    obs, act = case['obs'][r], case['act'][r].astype(F64)
    _, _, ls, _, _, mu = TR._forward64(case['pi_theta'], obs, obs.shape[1], act.shape[1], True, case['leak'])
    q = (act - mu) / (np.exp(ls) + 1e-8)
    logp = (-0.5 * ((q * q + 2.0 * ls) + LOG_2PI)).sum(1)
    w = case.get('weight')
    wmax = 1.0 if w is None else float(np.abs(w[r]).max())
    s_nll, s_mse = wmax * float(np.abs(logp).max()), wmax * float(((mu - act) ** 2).sum(1).max())
    return (s_nll if stage == 'nll' else s_mse, s_nll, s_mse, None)


def write_record(lines):
    print('\n'.join(lines))
    if RECORD:
        with open(RECORD, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def judge(what, got, ref64, ref32, sls, count, stage, scales, rescale=1.0, record=True):
    """got [P + nstat] (the kernel's float32 buffer, or whatever stands in its place) against (grad, stats) of the float64 law, with the
    float32 yardstick ref32 = (grad, stats) or None (then the floor alone is the bound: group D).  rescale: got's gradient and the
    statistics that scale with the advantage are multiplied by it first (group F).  Prints and records every figure, then asserts.
    Returns the largest share of a bound used."""
    P = ref64[0].size
    names = stat_names(stage)
    bits = np.asarray(got, F32) if np.asarray(got).dtype == F32 else None
    got = np.array(got, F64)
    assert got.size == P + len(names), (what, got.size, P)
    got[:P] *= rescale
    if stage == 'ppo':
        got[P] *= rescale
    fl = floor(count, stage)
    kern = rel_errors(got[:P], ref64[0], sls)
    yard = rel_errors(ref32[0], ref64[0], sls) if ref32 is not None else {k: 0.0 for k in kern}
    lines, failures, worst = [], [], 0.0
    for name in kern:
        bound = max(8.0 * yard[name], fl)
        zero = not np.abs(ref64[0][dict(sls)[name]]).max() > 0
        share = kern[name] / bound
        worst = max(worst, share if np.isfinite(share) else worst)
        lines.append('%s %-10s kernel %.3e  torch-f32 %.3e  bound %.3e  share %.3f%s' % (what, name, kern[name], yard[name], 0.0 if zero else bound,
                                                                                        0.0 if zero else share, '  (zero reference: zero asked)' if zero else ''))
        if not kern[name] <= bound:
            failures.append((what, name, kern[name], yard[name], fl))
    for j, name in enumerate(names):
        k, want = got[P + j], ref64[1][j]
        y = abs(ref32[1][j] - want) if ref32 is not None else 0.0
        if name in ('clip_frac', 'reserved') or want == 0.0:
            ok = (k == float(F32(want))) and (name != 'reserved' or bits is None or bits[P + j:].view(np.int32)[0] == 0)
            lines.append('%s %-10s kernel %.9g  float64 %.9g  (exact)' % (what, name, k, want))
        else:
            scale = abs(want) if scales[j] is None else scales[j] * (rescale if (stage == 'ppo' and j == 0) else 1.0)
            bound = max(8.0 * y, fl * scale)
            err = abs(k - want)
            ok = bool(np.isfinite(k)) and err <= bound
            worst = max(worst, err / bound if np.isfinite(err) else worst)
            lines.append('%s %-10s kernel %.3e  torch-f32 %.3e  bound %.3e  share %.3f (absolute; value %.6g)' % (what, name, err, y, bound, err / bound, want))
        if not ok:
            failures.append((what, name, k, want))
    if record:
        write_record(lines)
    assert not failures, failures
    return worst


def passes(fn, *a, **k):
    """True if a judge accepts, False if it raises AssertionError (the CPU file's mutants, and the references a group D call may choose from)."""
    try:
        fn(*a, **k)
        return True
    except AssertionError:
        return False


# ---- networks and rows ------------------------------------------------------------------------------------------------------------------
def make_net(in_dim, out_dim, rng, log_std=None, w3_zero=False, zero_biases=()):
    """A flat float32 network in -> 80 -> 80 -> 80 -> out: glorot-uniform kernels, biases uniform in +-0.1 (zero biases would hide a bias
    bug) except the layers of zero_biases; log_std None: a critic; a number: that value in every component; 'fixture': uniform in [-0.8, -0.2]."""
    sizes = [in_dim, HIDDEN, HIDDEN, HIDDEN, out_dim]
    Ws, bs = [], []
    for i in range(4):
        lim = math.sqrt(6.0 / (sizes[i] + sizes[i + 1]))
        Ws.append(rng.uniform(-lim, lim, size=(sizes[i], sizes[i + 1])).astype(F32))
        bs.append(rng.uniform(-0.1, 0.1, size=sizes[i + 1]).astype(F32))
    for i in zero_biases:
        bs[i][:] = 0.0
    if w3_zero:
        Ws[3][:] = 0.0
    if log_std is None:
        return TR.flatten(Ws, bs)
    ls = rng.uniform(-0.8, -0.2, size=out_dim).astype(F32) if isinstance(log_std, str) else np.full(out_dim, log_std, F32)
    return TR.flatten(Ws, bs, ls)


def logp64(pi_theta, obs, act, leak):
    """(logp, mu, log_std) of the float64 evaluation of float32 parameters and rows."""
    obs, act = np.asarray(obs), np.asarray(act, F64)
    _, _, ls, _, _, mu = TR._forward64(pi_theta, obs, obs.shape[1], act.shape[1], True, leak)
    q = (act - mu) / (np.exp(ls) + 1e-8)
    return (-0.5 * ((q * q + 2.0 * ls) + LOG_2PI)).sum(1), mu, ls


def _draw(rng, n, in_dim, out_dim):
    return (rng.normal(0.0, 1.0, size=(n, in_dim)).astype(F32), rng.normal(0.0, 1.0, size=(n, out_dim)), rng.uniform(-0.6, 0.6, size=n),
            rng.normal(0.0, 1.0, size=n).astype(F32), rng.normal(0.0, 1.0, size=n).astype(F32))


def _finish(pi_theta, obs, noise, delta, leak):
    """act = mu + sd noise and logp_old = logp - delta from the float64 evaluation, rounded to float32 (tests/ppo_fixture.py's)."""
    _, _, ls, _, _, mu = TR._forward64(pi_theta, obs, obs.shape[1], noise.shape[1], True, leak)
    act = (mu + np.exp(ls) * noise).astype(F32)
    return act, (logp64(pi_theta, obs, act, leak)[0] - delta).astype(F32)


def ratios(case, rows=None):
    r = slice(None) if rows is None else np.asarray(rows)
    return np.exp(logp64(case['pi_theta'], case['obs'][r], case['act'][r], case['leak'])[0] - case['logp_old'][r].astype(F64))


def hidden_z(case, net='pi_theta'):
    actor = net == 'pi_theta'
    return TR._forward64(case[net], case['obs'], case['obs'].shape[1], case['act'].shape[1] if actor else 1, actor, case['leak'])[4]


def near_kink(case, skip=()):
    """Rows within the margins of a kink in the float64 evaluation of either network; the rows `skip` are not looked at."""
    clip = case.get('clip', CLIP)
    r = ratios(case)
    bad = (np.abs(r - (1.0 + clip)) < RATIO_MARGIN) | (np.abs(r - (1.0 - clip)) < RATIO_MARGIN)
    for net in ('pi_theta', 'v_theta'):
        for z in hidden_z(case, net):
            bad |= (np.abs(z) < Z_MARGIN).any(1)
    bad[list(skip)] = False
    return bad


def cut_rows(case):
    """Rows whose actor gradient the clip rule removes (s1 > s2), in float64."""
    clip, r, A = case.get('clip', CLIP), ratios(case), case['adv'].astype(F64)
    return r * A > np.clip(r, 1.0 - clip, 1.0 + clip) * A


def make_rows(pi_theta, v_theta, in_dim, out_dim, n_rows, leak, rng, keep=()):
    """A case dict of n_rows ordinary rows for the two networks: every row keeps ppo_fixture's margins from both kinds of kink in both
    networks (rows that do not are drawn again; nothing is masked afterwards), rows 0 and 64 - the lone rows of count 1 and of count 65's
    second workgroup - carry an actor gradient, and the imitation weights are uniform in [0.25, 2].  keep: rows the redraw leaves alone
    (a caller overwrites them with its edge rows)."""
    obs, noise, delta, adv, ret = _draw(rng, n_rows, in_dim, out_dim)
    act, lpo = _finish(pi_theta, obs, noise, delta, leak)
    case = dict(in_dim=in_dim, out_dim=out_dim, leak=float(leak), clip=CLIP, pi_theta=pi_theta, v_theta=v_theta, obs=obs, act=act, adv=adv, ret=ret,
                logp_old=lpo, weight=rng.uniform(0.25, 2.0, size=n_rows).astype(F32))
    for _ in range(50):
        bad = near_kink(case, skip=keep)
        if not bad.any():
            break
        o2, n2, d2, a2, r2 = _draw(rng, int(bad.sum()), in_dim, out_dim)
        act2, lpo2 = _finish(pi_theta, o2, n2, d2, leak)
        case['obs'][bad], case['act'][bad], case['adv'][bad], case['ret'][bad], case['logp_old'][bad] = o2, act2, a2, r2, lpo2
    else:
        raise AssertionError('rows within the margins after 50 redraws')
    for r in (0, 64):
        if n_rows > r and r not in keep and cut_rows(case)[r]:
            live = np.flatnonzero(~cut_rows(case))
            live = [k for k in live if k not in (0, 64) and k not in keep]
            for k in ('obs', 'act', 'adv', 'ret', 'logp_old', 'weight'):
                case[k][[r, live[0]]] = case[k][[live[0], r]]
    return case


def make_fixture(in_dim, out_dim, n_rows, leak, seed):
    """The general form of tests/ppo_fixture.make_fixture: an actor in -> out with log_std in [-0.8, -0.2], a critic in -> 1, n_rows rows."""
    rng = np.random.RandomState(seed)
    pi_theta = make_net(in_dim, out_dim, rng, log_std='fixture')
    v_theta = make_net(in_dim, 1, rng)
    return make_rows(pi_theta, v_theta, in_dim, out_dim, n_rows, leak, rng)


_memo = {}


def memo(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _memo:
            _memo[key] = fn(*a)
        return _memo[key]
    wrapped.__name__ = fn.__name__
    return wrapped


# ---- A. shapes ------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 65)
A_ACTORS = ((1, 1, 0.2), (6, 7, 0.2), (16, 7, 0.2), (9, 1, 0.2), (16, 7, 0.0), (16, 7, 1.0))         # (in, out, leak)
A_CRITICS = ((1, 0.2), (6, 0.2), (16, 0.2), (16, 0.0), (16, 1.0))                                   # (in, leak)
ACTOR_STAGES = ('ppo', 'nll', 'mse')
N_ROWS = 65


@memo
def table_a(in_dim, out_dim, leak):
    return make_fixture(in_dim, out_dim, N_ROWS, leak, 1000 + 100 * in_dim + 10 * out_dim + int(10 * leak))


def critic_case(in_dim, leak):
    """The critic in -> 1 rides in the actor fixture of the same input width."""
    return table_a(in_dim, {1: 1, 6: 7, 16: 7}[in_dim], leak)


def padding_mutant(case, stage, rows):
    """What a kernel without its padding guards would return: the input tile's columns >= in and W0's rows >= in hold what lies behind them
    in memory (modelled as 1.0 and 0.05) instead of zeros; the gradient rows < in are what it writes.  (grad, stats) in float64."""
    in_dim, actor = case['in_dim'], stage != 'value'
    out_dim = case['out_dim'] if actor else 1
    net = 'pi_theta' if actor else 'v_theta'
    Ws, bs, ls = TR.unflatten(np.asarray(case[net], F64), in_dim, out_dim, actor)
    W0 = np.concatenate([Ws[0], np.full((16 - in_dim, HIDDEN), 0.05)], 0)
    wide = dict(case, in_dim=16, obs=np.concatenate([case['obs'], np.ones((case['obs'].shape[0], 16 - in_dim), F32)], 1))
    wide[net] = TR.flatten([W0] + list(Ws[1:]), list(bs), ls)
    g, s = reference(wide, stage, rows)
    gW, gb, gls = TR.unflatten(g, 16, out_dim, actor)
    return TR.flatten([gW[0][:in_dim]] + list(gW[1:]), list(gb), gls), s


# ---- B. log_std and the epsilon ---------------------------------------------------------------------------------------------------------
B_LOG_STDS = (-18.0, -14.0, -4.0, 1.0, 5.0)
B_STAGES = ('ppo', 'nll')


@memo
def table_b(log_std):
    """An actor 9 -> 7 with W3 = 0 - mu = b3 exactly in both arithmetics, so q = (act - b3) / sd is the same number on both sides whatever
    sd is - and log_std the same in every component.  act = float32(b3 + e^ls noise), logp_old = float32(logp - delta), delta in +-0.6;
    rows near ratio = 1 +- clip draw delta again, rows 0 and 64 sit inside the band (they flow whatever the advantage)."""
    rng = np.random.RandomState(2000 + int(10 * log_std))
    theta = make_net(9, 7, rng, log_std=log_std, w3_zero=True)
    obs, noise, delta, adv, ret = _draw(rng, N_ROWS, 9, 7)
    delta[[0, 64]] = (0.05, -0.07)
    act, lpo = _finish(theta, obs, noise, delta, 0.2)
    case = dict(in_dim=9, out_dim=7, leak=0.2, clip=CLIP, pi_theta=theta, obs=obs, act=act, adv=adv, ret=ret, logp_old=lpo,
                weight=rng.uniform(0.25, 2.0, size=N_ROWS).astype(F32))
    for _ in range(50):
        r = ratios(case)
        bad = (np.abs(r - (1.0 + CLIP)) < RATIO_MARGIN) | (np.abs(r - (1.0 - CLIP)) < RATIO_MARGIN)
        if not bad.any():
            return case
        d2 = rng.uniform(-0.6, 0.6, size=int(bad.sum()))
        case['logp_old'][bad] = (logp64(theta, obs[bad], act[bad], 0.2)[0] - d2).astype(F32)
    raise AssertionError('rows within the margin after 50 redraws')


def below_b3(in_dim=9, out_dim=7):
    """The tensors under b3 - W0 .. b2 - which an actor with W3 = 0 gives a zero gradient."""
    return [name for name, _ in slices(in_dim, out_dim)][:6]


# ---- C. the clip rule's ties, exactly -----------------------------------------------------------------------------------------------------
C_CLIPS = (0.2, 0.0)


def logp_f32(b3, act, log_std=0.0):
    """The kernel's float32 log-probability restated in NumPy float32, in the header's order: q, then -0.5 ((q^2 + 2 ls) + log 2 pi), summed
    over j from 0.  Valid as a restatement where mu == b3 (W3 = 0)."""
    ls = F32(log_std)
    sd = F32(np.exp(ls)) + F32(1e-8)
    logp = np.zeros(act.shape[0], F32)
    for j in range(act.shape[1]):
        q = ((act[:, j] - b3[j]) / sd).astype(F32)
        logp = (logp + F32(-0.5) * (((q * q).astype(F32) + F32(2.0) * ls).astype(F32) + F32(LOG_2PI)).astype(F32)).astype(F32)
    return logp


def _tie_net(rng):
    theta = make_net(9, 7, rng, log_std=0.0, w3_zero=True)
    L = TR.layout(9, 7, True)
    theta[L['b'][3]:L['b'][3] + 7] = rng.randint(-8, 9, size=7) / 8.0          # b3: multiples of 1/8
    return theta, theta[L['b'][3]:L['b'][3] + 7].copy()


@memo
def table_c(clip):
    """W3 = 0, log_std = 0 exactly (sd = 1 + 1e-8 is 1.0f), b3 and act - b3 multiples of 1/8: q and q^2 are exact, the float32 logp is
    logp_f32 on any correct float32 machine, logp_old is that number, logp - logp_old = +0 and ratio = exp(+0) = 1 exactly: with clip 0.2 a
    tie inside the band, with clip 0 (lo = hi = 1) a row on both bounds.  Advantages of both signs, none zero."""
    rng = np.random.RandomState(3000)
    theta, b3 = _tie_net(rng)
    obs = rng.normal(0.0, 1.0, size=(N_ROWS, 9)).astype(F32)
    act = (b3[None, :] + rng.randint(-16, 17, size=(N_ROWS, 7)) / 8.0).astype(F32)
    adv = rng.normal(0.0, 1.0, size=N_ROWS).astype(F32)
    adv[[0, 64]] = (0.75, -1.25)
    return dict(in_dim=9, out_dim=7, leak=0.2, clip=float(clip), pi_theta=theta, b3=b3, obs=obs, act=act, adv=adv, logp_old=logp_f32(b3, act))


C_PLUS_ZERO, C_MINUS_ZERO = (3, 17, 64), (0, 5, 40)


@memo
def table_c_zero_adv(all_zero):
    """The tie actor with ordinary ratios (delta in +-0.6, off the bounds) and rows whose advantage is +0.0 or -0.0 among them; all_zero:
    every advantage is +-0."""
    rng = np.random.RandomState(3100)
    theta, b3 = _tie_net(rng)
    obs, noise, delta, adv, _ = _draw(rng, N_ROWS, 9, 7)
    act = (b3[None, :] + rng.randint(-16, 17, size=(N_ROWS, 7)) / 8.0).astype(F32)
    near = np.abs(np.abs(delta) - 0.2) < 0.03                                   # exp(+-0.2) is within 0.03 of 1 +- 0.2: keep away
    delta[near] *= 0.5
    if all_zero:
        adv = np.where(np.arange(N_ROWS) % 2 == 0, F32(0.0), F32(-0.0)).astype(F32)
    adv[list(C_PLUS_ZERO)] = 0.0
    adv[list(C_MINUS_ZERO)] = -0.0
    case = dict(in_dim=9, out_dim=7, leak=0.2, clip=CLIP, pi_theta=theta, b3=b3, obs=obs, act=act, adv=adv)
    case['logp_old'] = (logp64(theta, obs, act, 0.2)[0] - delta).astype(F32)
    r = ratios(case)
    assert (np.abs(r - 1.2) > RATIO_MARGIN).all() and (np.abs(r - 0.8) > RATIO_MARGIN).all()
    return case


# ---- D. rows at the bounds that cannot be hit exactly, and ratios beyond float32 --------------------------------------------------------
D_SINGLE = (('upper', 1.0, True), ('upper', -1.0, False), ('lower', 1.0, False), ('lower', -1.0, True))      # (bound, A, ambiguous)


def _to_bound(case, row, target_log_ratio):
    """logp_old of `row` so that logp - logp_old is target_log_ratio up to float32's rounding of logp_old."""
    lp = logp64(case['pi_theta'], case['obs'][[row]], case['act'][[row]], case['leak'])[0][0]
    case['logp_old'][row] = F32(lp - target_log_ratio)


def band_rows(case):
    """Rows whose float64 ratio is within BAND (relative) of 1 + clip or of 1 - clip."""
    clip, r = case.get('clip', CLIP), ratios(case)
    return (np.abs(r / (1.0 + clip) - 1.0) < BAND) | (np.abs(r / (1.0 - clip) - 1.0) < BAND)


def ambiguous_rows(case):
    """The rows a float32 evaluation may put on either side of the rule: in the band, and with the sign of A that the bound cuts (A > 0
    above, A < 0 below).  The other two sign cases flow on both sides of the bound."""
    clip, r, A = case.get('clip', CLIP), ratios(case), case['adv']
    return band_rows(case) & np.where(r > 1.0, A > 0, A < 0)


@memo
def table_d():
    """An ordinary 9 -> 7 fixture of 65 + 4 rows.  Rows 65 .. 68 are D_SINGLE's, each run alone; rows 20 and 64 of the first 65 are the two
    ambiguous rows of the count-65 call (above with A = +0.5, below with A = -2: the second sits alone in its workgroup).  The advantages
    of band rows are powers of two, so that ratio x A and bound x A are exact products and s1 <= s2 is ratio <= bound itself: the
    gradient and clip_frac then cannot disagree about the side."""
    rng = np.random.RandomState(4000)
    pi_theta = make_net(9, 7, rng, log_std='fixture')
    v_theta = make_net(9, 1, rng)
    edge = (20, 64, 65, 66, 67, 68)
    case = make_rows(pi_theta, v_theta, 9, 7, N_ROWS + 4, 0.2, rng, keep=edge)
    spec = {20: ('upper', 0.5), 64: ('lower', -2.0)}
    spec.update({65 + k: (b, a) for k, (b, a, _) in enumerate(D_SINGLE)})
    for row, (bound, a) in spec.items():
        case['adv'][row] = a
        _to_bound(case, row, math.log(1.0 + CLIP if bound == 'upper' else 1.0 - CLIP))
    assert not near_kink(case, skip=edge).any()
    return case


D_CALL_ROWS = np.arange(N_ROWS)
D_CALL_BAND = (20, 64)                            # both ambiguous
D_EXTREME = ((-200.0, 1.0), (-200.0, -1.0), (200.0, 1.0))          # (logp - logp_old, A); +200 with A < 0 is non-finite by the law: not run


@memo
def table_d_extreme():
    """Three rows of table A's 9 -> 7 fixture with logp_old moved by -+200: exp(-200) = 0 and exp(+200) = inf in float32."""
    base = table_a(9, 7, 0.2)
    case = {k: (v[:3].copy() if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == N_ROWS else v) for k, v in base.items()}
    for row, (d, a) in enumerate(D_EXTREME):
        case['adv'][row] = a
        _to_bound(case, row, d)
    return case


def extreme_expectation(case, row):
    """(stats [4]) the law gives a row of D_EXTREME with the ratio float32 forms: 0 (both signs: the gradient -A ratio is zero, or the row
    is cut) or +inf with A > 0 (cut: s2 = (1 + clip) A is the minimum).  The gradient is zero in all three."""
    d, a = D_EXTREME[row]
    clip = case['clip']
    lp = logp64(case['pi_theta'], case['obs'][[row]], case['act'][[row]], case['leak'])[0][0]
    kl = float(case['logp_old'][row]) - lp
    if d < 0:
        return np.array([0.0 if a > 0 else -(1.0 - clip) * a, kl, 1.0, 0.0])
    return np.array([-(1.0 + clip) * a, kl, 1.0, np.inf])


def judge_extreme(what, got, case, row):
    """A row whose ratio left float32's range: every gradient element zero, pi_loss within the floor of its expectation, approx_kl within
    the floor x max|logp_old|, clip_frac 1, mean_ratio 0 or +inf exactly."""
    got = np.asarray(got, F64)
    P = got.size - 4
    want = extreme_expectation(case, row)
    fl = floor(1)
    errs = (abs(got[P] - want[0]), abs(got[P + 1] - want[1]))
    bounds = (fl * 2.0 * abs(float(case['adv'][row])), fl * abs(float(case['logp_old'][row])))
    write_record(['%s gradient max |g| %.3g (zero asked)  pi_loss err %.3e bound %.3e  approx_kl err %.3e bound %.3e  clip_frac %g  mean_ratio %g'
                  % (what, float(np.abs(got[:P]).max()) if np.isfinite(got[:P]).all() else float('nan'), errs[0], bounds[0], errs[1], bounds[1],
                     got[P + 2], got[P + 3])])
    assert np.isfinite(got[:P]).all() and not got[:P].any(), (what, 'gradient not zero')
    assert np.isfinite(got[P:P + 3]).all() and errs[0] <= bounds[0] and errs[1] <= bounds[1], (what, got[P:], want)
    assert got[P + 2] == 1.0 and got[P + 3] == want[3], (what, got[P:], want)


def judge_either_side(what, got, case, rows, band, sls):
    """Group D's judge.  band: the positions in `rows` of the rows within BAND of a bound (at most two).  The float32 ratio of such a row may
    land inside or outside its bound, and the row goes there with everything it has: clip_frac counts it iff it is outside, and a row the
    table tags ambiguous (ambiguous_rows: the bound cuts its sign of A) flows iff it is inside; the other rows of the band flow on both sides.
    got must pass judge() against one of the 2^k references so formed.  The bound is the floor alone: the float32 yardstick may sit on the
    other side (torch float32 itself uses at most 0.02 of the floor here).  Returns the (flows, outside) accepted."""
    rows = np.asarray(rows)
    assert len(band) <= 2
    count = len(rows)
    amb = ambiguous_rows(case)[rows]
    r = ratios(case, rows)
    clip = case.get('clip', CLIP)
    for pick in range(2 ** len(band)):
        flows, outside = ~cut_rows(case)[rows], (r > 1.0 + clip) | (r < 1.0 - clip)
        for k, pos in enumerate(band):
            outside[pos] = bool(pick >> k & 1)
            flows[pos] = (not outside[pos]) if amb[pos] else True
        ref = reference(case, 'ppo', rows, flows=flows, outside=outside)
        tag = '%s [%s]' % (what, ' '.join('row %d %s, %s' % (rows[p], 'outside' if outside[p] else 'inside', 'flows' if flows[p] else 'cut') for p in band))
        args = (tag, got, ref, None, sls, count, 'ppo', stat_scales(case, 'ppo', rows))
        if passes(judge, *args, record=False):
            judge(*args)
            return flows, outside
    raise AssertionError((what, 'matches none of the %d references' % 2 ** len(band)))


# ---- E. pre-activations of exactly zero ---------------------------------------------------------------------------------------------------
E_LEAKS = (0.2, 0.0, 1.0)
E_KINDS = ('first', 'all')            # b0 = 0: the 80 first-layer pre-activations of the zero row are +0;  b0 = b1 = b2 = 0: every hidden one
E_STAGES = ('ppo', 'value')


@memo
def table_e(kind, leak):
    """A 9 -> 7 actor and a 9 -> 1 critic with b0 = 0 ('first') or b0 = b1 = b2 = 0 ('all'), 65 rows; row 64 is the all-zero observation, whose
    pre-activations are then exactly zero in the first or in every hidden layer, in both arithmetics.  It flows (ratio inside the band) and is
    run alone and as row 64 of the count-65 call; the other 64 rows keep their margins."""
    rng = np.random.RandomState(5000 + (kind == 'all') + int(10 * leak))
    zb = (0,) if kind == 'first' else (0, 1, 2)
    pi_theta = make_net(9, 7, rng, log_std='fixture', zero_biases=zb)
    v_theta = make_net(9, 1, rng, zero_biases=zb)
    case = make_rows(pi_theta, v_theta, 9, 7, N_ROWS, leak, rng, keep=(64,))
    case['obs'][64] = 0.0
    noise = rng.normal(0.0, 1.0, size=(1, 7))
    act, lpo = _finish(pi_theta, case['obs'][[64]], noise, np.array([0.04]), leak)
    case['act'][64], case['logp_old'][64], case['adv'][64], case['ret'][64] = act[0], lpo[0], -0.8, 0.6
    return case


def zero_preactivation_layers(case, row=64):
    """Per network, the hidden layers whose 80 pre-activations of `row` are all exactly zero (float64)."""
    return {net: [i for i, z in enumerate(hidden_z(case, net)) if not z[row].any()] for net in ('pi_theta', 'v_theta')}


# ---- F. scale -----------------------------------------------------------------------------------------------------------------------------
F_SCALE = 2.0 ** -120


@memo
def table_f():
    """The 9 -> 7 fixture of table A's maker with the advantages times 2^-120 (a float32 product: exact unless it goes subnormal; the
    reference is the float64 law of the float32 rows the kernel gets)."""
    base = table_a(9, 7, 0.2)
    return dict(base, adv=(base['adv'] * F32(F_SCALE)).astype(F32))


def flush(x):
    """x with every float32 value below 2^-126 in magnitude replaced by zero: a unit that flushes subnormals."""
    x = np.array(x, F32)
    x[np.abs(x) < F32(2.0 ** -126)] = 0.0
    return x


# ---- G. Adam, bit for bit -----------------------------------------------------------------------------------------------------------------
G_P = 257                                                  # 64 float4 of the vector body and one element of the scalar tail
G_GRADS = (0.0, -0.0, 2.0 ** -149, 1e-38, 1e-22, 1e-19, 1.0, 1e19, 3e38, 2e19)      # 3e38, 2e19: g^2 above FLT_MAX; 3e38: v = inf, theta keeps its bits
G_PRIORS = ((0.0, 0.0), (1e-40, 1e-42), (0.3, 0.02), (1e30, 1e30))                  # (m, v): zero, subnormal, ordinary, large
G_STEPS = (1, 2, 1000, 100000, 10 ** 9)                    # t; from 100 000 on beta2^t, from 10^9 on both powers, have underflowed
G_DEFAULTS = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
G_SINGLE = (dict(eps=0.0), dict(lr=0.0), dict(beta1=0.0), dict(beta2=0.0))


@memo
def table_g():
    """dict(theta, grad, m, v) [257] float32: the cross product of G_GRADS and G_PRIORS (both signs of m), cycled over the vector."""
    rng = np.random.RandomState(7000)
    combos = [(g, sm * m, v) for g in G_GRADS for (m, v) in G_PRIORS for sm in (1.0, -1.0)]
    assert len(combos) <= G_P
    pick = [combos[i % len(combos)] for i in range(G_P)]
    g, m, v = (np.array([p[k] for p in pick], F32) for k in range(3))
    sign = np.where(rng.uniform(size=G_P) < 0.5, -1.0, 1.0)
    g = (g * np.where(np.arange(G_P) >= len(combos), sign, 1.0)).astype(F32)         # the second pass over the combos: random signs of g
    theta = (rng.uniform(0.05, 1.0, G_P) * rng.choice([-1.0, 1.0], G_P)).astype(F32)
    return dict(theta=theta, grad=g, m=m, v=v)


def adam_statement(tab, t, gate_kl=None, kl_limit=float('inf'), stop=0, **hyper):
    """TR.adam_step_ref on the table before step t: (theta, m, v, step, stop) after the call."""
    h = dict(G_DEFAULTS, **hyper)
    with np.errstate(all='ignore'):
        return TR.adam_step_ref(tab['theta'], tab['grad'], tab['m'], tab['v'], t - 1, h['lr'], h['beta1'], h['beta2'], h['eps'], gate_kl=gate_kl,
                                kl_limit=kl_limit, stop=stop)


def gate_cases():
    """(name, gate_kl, kl_limit, flag before): the statement's gate decides what is expected."""
    kl = F32(0.015)
    return (('kl == limit', kl, float(kl), 0), ('kl one ulp above', np.nextafter(kl, F32(1.0)), float(kl), 0), ('kl NaN', F32(np.nan), float(kl), 0),
            ('limit +inf', kl, float('inf'), 0), ('limit -inf', kl, float('-inf'), 0), ('flag already set', F32(0.0), float(kl), 1))


def judge_adam(what, got, want):
    """got, want: (theta, m, v, step, stop).  The three vectors equal bit for bit, NaN where the statement has NaN (any NaN), and the
    counter and the flag equal."""
    lines, bad = [], []
    for name, g, w in zip(('theta', 'm', 'v'), got[:3], want[:3]):
        g, w = np.asarray(g, F32), np.asarray(w, F32)
        nan = np.isnan(w)
        differ = np.flatnonzero(np.where(nan, ~np.isnan(g), g.view(np.int32) != w.view(np.int32)))
        lines.append('%s %-5s %d of %d elements differ from the statement (NaN in the statement: %d)' % (what, name, differ.size, w.size, int(nan.sum())))
        if differ.size:
            bad.append((what, name, int(differ[0]), float(g[differ[0]]), float(w[differ[0]])))
    write_record(lines)
    assert not bad, bad
    assert (int(got[3]), int(got[4])) == (int(want[3]), int(want[4])), (what, 'step, stop', got[3:], want[3:])
