"""The PPO update on the device (include/dpenv.h, "The PPO update"): PPO-clip actor gradient, the critic's MSE gradient and a
device-gated Adam step, so that the 80 + 80 gradient steps of an epoch (ppo.py:265-273) queue without a host round trip.

``ppo_actor_grad`` / ``value_grad`` / ``imitation_grad`` / ``adam_step`` bind the handle-free C entry points; ``PPOUpdater`` re-homes
the tensors of a ``policy.ActorCritic`` as views of two flat parameter vectors and runs the whole update, and - before it - the
supervised warm start on demonstration rows (``pretrain`` / ``pretrain_critic``).  The host statements of the same law -
``ppo_actor_grad_ref`` / ``value_grad_ref`` / ``imitation_grad_ref`` (closed form, float64) and ``adam_step_ref`` (NumPy float32 in
the header's operation order) - are what the tests hold the kernels to.  ``allocation_grad`` (host statement ``allocation_grad_ref``) is
the same gradient kernel with the allocation loss - the QP law's objective at a thrust-allocator network's output, through the force map -
and ``fit_nn_allocator`` fits that network with it or with the label MSE.  There is no fallback: without the library or a GPU the device functions raise.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import _p, _req, _s, _torch
from ._num import _fma32          # (the exact host fmaf; deploy.BatchedNNAllocator shares it)

HIDDEN = 80
NSTAT_ACTOR, NSTAT_CRITIC = 4, 1          # pi_loss, approx_kl, clip_frac, mean_ratio | v_loss
ROWS_PER_TILE, MAX_WORKGROUPS = 64, 256   # the gradient kernel's grid: min(ceil(count / 64), 256) workgroups


def grid(count):
    """Workgroups the gradient kernel runs for `count` rows (a function of count alone: dpenv.h, DETERMINISM)."""
    return min((int(count) + ROWS_PER_TILE - 1) // ROWS_PER_TILE, MAX_WORKGROUPS)


def layout(in_dim, out_dim, actor):
    """Offsets of the flat parameter vector: {'W': [...], 'b': [...], 'log_std': off or None, 'P': P, 'sizes': [...]}."""
    sizes = [int(in_dim), HIDDEN, HIDDEN, HIDDEN, int(out_dim)]
    W, b, o = [], [], 0
    for i in range(4):
        W.append(o)
        o += sizes[i] * sizes[i + 1]
        b.append(o)
        o += sizes[i + 1]
    ls = o if actor else None
    if actor:
        o += sizes[4]
    return dict(W=W, b=b, log_std=ls, P=o, sizes=sizes)


def flatten(Ws, bs, log_std=None):
    """[W0 [in][out], b0, W1, b1, ...] (+ log_std) -> one flat vector of the same kind (torch tensor or NumPy array)."""
    parts = []
    for W, b in zip(Ws, bs):
        parts += [W.reshape(-1), b.reshape(-1)]
    if log_std is not None:
        parts.append(log_std.reshape(-1))
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    return _torch().cat(parts)


def unflatten(theta, in_dim, out_dim, actor):
    """Views of a flat vector: (Ws, bs, log_std or None)."""
    L = layout(in_dim, out_dim, actor)
    s = L['sizes']
    Ws = [theta[L['W'][i]:L['W'][i] + s[i] * s[i + 1]].reshape(s[i], s[i + 1]) for i in range(4)]
    bs = [theta[L['b'][i]:L['b'][i] + s[i + 1]] for i in range(4)]
    return Ws, bs, (theta[L['log_std']:L['log_std'] + s[4]] if actor else None)


def make_shape(in_dim, out_dim, actor, leak=0.2, activation='leaky', hidden=(HIDDEN, HIDDEN, HIDDEN), row_dtype=_lib.F32):
    sh = _lib.TrainShape()
    sh.struct_size = C.sizeof(_lib.TrainShape)
    sizes = [int(in_dim)] + [int(h) for h in hidden] + [int(out_dim)]
    if len(sizes) > 6:
        raise ValueError('at most 5 dense layers')
    sh.n_layers = len(sizes) - 1
    for i, v in enumerate(sizes):
        sh.sizes[i] = v
    sh.activation = _lib.ACT_TANH if activation == 'tanh' else _lib.ACT_LEAKY_RELU
    sh.leak = 0.0 if activation == 'relu' else float(leak)
    sh.row_dtype = int(row_dtype)
    sh.log_std = 1 if actor else 0
    return sh


def param_count(shape):
    n = int(_lib.load().dpenv_train_param_count(C.byref(shape)))
    if n < 0:
        _lib.check(n)
    return n


def workspace_bytes(shape, max_count):
    out = C.c_int64(0)
    _lib.check(_lib.load().dpenv_train_workspace_bytes(C.byref(shape), int(max_count), C.byref(out)))
    return int(out.value)


def _grad_call(actor, theta, obs, act, adv, logp_old, clip, idx, out, workspace, leak, stop_flag, count, loss=None):
    """The one binding of the three gradient entry points.  loss (a code of LOSSES): dpenv_imitation_grad, `adv` then being the row
    weight or None."""
    torch = _torch()
    f32 = torch.float32
    n_rows, in_dim = obs.shape
    out_dim = act.shape[1] if actor else 1
    sh = make_shape(in_dim, out_dim, actor, leak=leak)
    P = param_count(sh)
    _req(theta, (P,), f32, 'theta')
    _req(obs, (n_rows, in_dim), f32, 'obs')
    _req(act, (n_rows, out_dim), f32, 'act')
    _req(adv, (n_rows,), f32, 'weight' if loss is not None else ('adv' if actor else 'ret'))
    _req(logp_old, (n_rows,), f32, 'logp_old')
    _req(idx, None, torch.int32, 'idx')
    _req(stop_flag, (1,), torch.int32, 'stop_flag')
    if count is None:
        count = int(idx.numel()) if idx is not None else n_rows
    if idx is not None and int(count) > idx.numel():
        raise ValueError('count = %d, idx holds %d indices' % (count, idx.numel()))
    nstat = NSTAT_ACTOR if actor else NSTAT_CRITIC
    if out is None:
        out = torch.empty(P + nstat, dtype=f32, device=theta.device)
    _req(out, (P + nstat,), f32, 'out')
    if workspace is None:
        workspace = torch.empty((workspace_bytes(sh, max(count, 1)) + 3) // 4, dtype=f32, device=theta.device)
    lib = _lib.load()
    ws_bytes = workspace.numel() * workspace.element_size()
    with torch.cuda.device(theta.device):
        if loss is not None:
            _lib.check(lib.dpenv_imitation_grad(C.byref(sh), _p(theta), _p(obs), _p(act), _p(adv), _p(idx), int(count), int(n_rows), int(loss),
                                                _p(stop_flag), _p(out), _p(workspace), ws_bytes, _s(theta)))
        elif actor:
            _lib.check(lib.dpenv_ppo_actor_grad(C.byref(sh), _p(theta), _p(obs), _p(act), _p(adv), _p(logp_old), _p(idx), int(count), int(n_rows),
                                                float(clip), _p(stop_flag), _p(out), _p(workspace), ws_bytes, _s(theta)))
        else:
            _lib.check(lib.dpenv_value_grad(C.byref(sh), _p(theta), _p(obs), _p(adv), _p(idx), int(count), int(n_rows), _p(out), _p(workspace),
                                            ws_bytes, _s(theta)))
    return out


def ppo_actor_grad(theta, obs, act, adv, logp_old, clip, idx=None, out=None, workspace=None, leak=0.2, stop_flag=None, count=None):
    """dpenv_ppo_actor_grad: the PPO-clip gradient of the flat actor `theta` over rows `idx` (int32; None = all rows) of
    obs [n, in] / act [n, out] / adv / logp_old [n].  Returns out [P + 4]: the gradient, then pi_loss, approx_kl, clip_frac, mean_ratio.
    stop_flag: int32 [1]; a call that finds it set leaves `out` as it is.  Stream-ordered, nothing is read back."""
    return _grad_call(True, theta, obs, act, adv, logp_old, clip, idx, out, workspace, leak, stop_flag, count)


def value_grad(theta, obs, ret, idx=None, out=None, workspace=None, leak=0.2, count=None):
    """dpenv_value_grad: the gradient of mean((ret - v)^2) for the flat critic `theta`.  Returns out [P + 1]: the gradient, then v_loss."""
    return _grad_call(False, theta, obs, None, ret, None, 0.0, idx, out, workspace, leak, None, count)


LOSSES = {'nll': _lib.IMITATE_NLL, 'mse': _lib.IMITATE_MSE}


def _loss_code(loss):
    if loss in LOSSES:
        return LOSSES[loss]
    if isinstance(loss, str):
        raise ValueError("loss must be 'nll' or 'mse' (got %r)" % (loss,))
    return int(loss)                                           # a raw code goes to the library, which refuses what it does not know


def imitation_grad(theta, obs, act, loss='nll', weight=None, idx=None, out=None, workspace=None, leak=0.2, stop_flag=None, count=None):
    """dpenv_imitation_grad: the gradient of the weighted imitation loss of the flat actor `theta` over rows `idx` (int32; None = all rows)
    of obs [n, in] / act [n, out], weight [n] or None = 1.  loss: 'nll' (-mean(w logp)) or 'mse' (mean(w sum_j (mu_j - act_j)^2)).
    Returns out [P + 4]: the gradient, then the chosen loss, the weighted NLL, the weighted MSE, 0.  Stream-ordered, nothing is read back."""
    return _grad_call(True, theta, obs, act, weight, None, 0.0, idx, out, workspace, leak, stop_flag, count, loss=_loss_code(loss))


ALLOC_LOSS_FIELDS = ('w_slack', 'w_power', 'w_sat', 'lx', 'ly', 'kf', 'kr', 'angle_scale', 'azimuth_mode', 'azimuth')


def alloc_loss_params(params=None, vessel=None):
    """deploy.alloc_loss_defaults(vessel) with the entries of `params` on top (None = the defaults; a partial dict such as
    dict(w_power=0.05) is enough)."""
    from .deploy import alloc_loss_defaults
    p = alloc_loss_defaults(vessel)
    for k, v in (params or {}).items():
        if k not in p:
            raise ValueError('allocation loss: unknown number %r (known: %s)' % (k, sorted(p)))
        p[k] = v
    return p


def alloc_loss_struct(params=None):
    """The dpenv_alloc_loss of a dict of deploy.alloc_loss_defaults (None or partial: see alloc_loss_params)."""
    p = alloc_loss_params(params)
    q = _lib.AllocLoss()
    q.struct_size = C.sizeof(_lib.AllocLoss)
    for name in ('w_slack', 'lx', 'ly', 'kf', 'kr'):
        v = np.asarray(p[name], np.float64).reshape(-1)
        if v.shape != (3,):
            raise ValueError('allocation loss: %s has three entries (bow, port, star)' % name)
        getattr(q, name)[:] = [float(t) for t in v]
    az = np.asarray(p['azimuth'], np.float64).reshape(-1)
    if az.shape != (2,):
        raise ValueError('allocation loss: azimuth has two entries (port, star)')
    q.azimuth[:] = [float(t) for t in az]
    q.w_power, q.w_sat, q.angle_scale, q.azimuth_mode = float(p['w_power']), float(p['w_sat']), float(p['angle_scale']), int(p['azimuth_mode'])
    return q


def allocation_grad(theta, x, tau, params=None, weight=None, idx=None, out=None, workspace=None, leak=0.2, stop_flag=None, count=None):
    """dpenv_allocation_grad: the gradient of the allocation loss (include/dpenv.h, ALLOCATION LOSS) - the QP law's objective at the
    network's output, through the force map - of the flat allocator network `theta` ({in, 80, 80, 80, 6} + the carried log_std tail, in =
    3 or 9) over rows `idx` (int32; None = all rows) of x [n, in] (the network's inputs) and tau [n, 6] (columns 0..2 the demanded wrench
    in N, N, Nm; 3..5 never enter a result), weight [n] or None = 1.  params: the dict of deploy.alloc_loss_defaults, whole or in part
    (None = the defaults).  Returns out [P + 4]: the gradient, then L, the weighted mean Js (wrench residual), Jp (power) and Jx
    (saturation).  Stream-ordered, nothing is read back."""
    torch = _torch()
    f32 = torch.float32
    n_rows, in_dim = x.shape
    sh = make_shape(in_dim, 6, True, leak=leak)
    q = alloc_loss_struct(params)
    P = layout(in_dim, 6, True)['P']
    _req(theta, (P,), f32, 'theta')
    _req(x, (n_rows, in_dim), f32, 'x')
    _req(tau, (n_rows, 6), f32, 'tau')
    _req(weight, (n_rows,), f32, 'weight')
    _req(idx, None, torch.int32, 'idx')
    _req(stop_flag, (1,), torch.int32, 'stop_flag')
    if count is None:
        count = int(idx.numel()) if idx is not None else n_rows
    if idx is not None and int(count) > idx.numel():
        raise ValueError('count = %d, idx holds %d indices' % (count, idx.numel()))
    if out is None:
        out = torch.empty(P + NSTAT_ACTOR, dtype=f32, device=theta.device)
    _req(out, (P + NSTAT_ACTOR,), f32, 'out')
    if workspace is None:
        workspace = torch.empty((workspace_bytes(sh, max(count, 1)) + 3) // 4, dtype=f32, device=theta.device)
    with torch.cuda.device(theta.device):
        _lib.check(_lib.load().dpenv_allocation_grad(C.byref(sh), C.byref(q), _p(theta), _p(x), _p(tau), _p(weight), _p(idx), int(count), int(n_rows),
                                                     _p(stop_flag), _p(out), _p(workspace), workspace.numel() * workspace.element_size(), _s(theta)))
    return out


def adam_step(theta, grad, m, v, step_counter, lr, beta1=0.9, beta2=0.999, eps=1e-8, gate_kl=None, kl_limit=float('inf'), stop_flag=None):
    """dpenv_adam_step: one torch.optim.Adam step of theta [P] with grad[:P] in place; step_counter int32 [1] counts the steps taken.
    gate_kl (float32 [1], e.g. the approx_kl slot of the gradient buffer) with stop_flag (int32 [1]): if the flag is set or
    gate_kl > kl_limit the flag is set and nothing else changes."""
    torch = _torch()
    P = theta.numel()
    for t, what in ((theta, 'theta'), (m, 'm'), (v, 'v')):
        _req(t, (P,), torch.float32, what)
    if grad.numel() < P:
        raise ValueError('grad has %d elements, theta %d' % (grad.numel(), P))
    _req(grad, None, torch.float32, 'grad')
    _req(step_counter, (1,), torch.int32, 'step_counter')
    _req(gate_kl, (1,), torch.float32, 'gate_kl')
    _req(stop_flag, (1,), torch.int32, 'stop_flag')
    with torch.cuda.device(theta.device):
        _lib.check(_lib.load().dpenv_adam_step(_p(theta), _p(grad), _p(m), _p(v), int(P), float(lr), float(beta1), float(beta2), float(eps),
                                               _p(step_counter), _p(gate_kl), float(kl_limit), _p(stop_flag), _s(theta)))
    return theta


# ---- host statements of the law (NumPy) --------------------------------------------------------------------------------------------
def _forward64(theta, obs, in_dim, out_dim, actor, leak):
    Ws, bs, ls = unflatten(np.asarray(theta, np.float64), in_dim, out_dim, actor)
    h, hs, zs = np.asarray(obs, np.float64), [], []
    for i in range(3):
        hs.append(h)
        z = h @ Ws[i] + bs[i]
        zs.append(z)
        h = np.maximum(z, leak * z)
    hs.append(h)
    return Ws, bs, ls, hs, zs, h @ Ws[3] + bs[3]


def _backward64(Ws, hs, zs, dout, leak, extra=None):
    """dout = dL/d(output) [count, out] -> the flat gradient (extra: the log_std part)."""
    gW, gb = [None] * 4, [None] * 4
    g = dout
    for i in (3, 2, 1, 0):
        gW[i] = hs[i].T @ g
        gb[i] = g.sum(0)
        if i > 0:
            g = (g @ Ws[i].T) * np.where(zs[i - 1] > 0, 1.0, leak)      # act'(z): 1 where z > 0, leak elsewhere (z = 0 included)
    return flatten(gW, gb, extra)


def ppo_actor_grad_ref(theta, obs, act, adv, logp_old, clip, leak=0.2, hidden_z=False):
    """The header's actor law in closed form, float64: (grad [P], stats [4] = pi_loss, approx_kl, clip_frac, mean_ratio); with hidden_z
    also the hidden pre-activations and the ratio (the tests' fixture conditions)."""
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    A, lpo = np.asarray(adv, np.float64), np.asarray(logp_old, np.float64)
    count, in_dim, out_dim = obs.shape[0], obs.shape[1], act.shape[1]
    Ws, bs, ls, hs, zs, mu = _forward64(theta, obs, in_dim, out_dim, True, leak)
    sd = np.exp(ls) + 1e-8
    q = (act - mu) / sd
    logp = (-0.5 * ((q * q + 2.0 * ls) + math.log(2.0 * math.pi))).sum(1)
    ratio = np.exp(logp - lpo)
    lo, hi = 1.0 - clip, 1.0 + clip
    s1, s2 = ratio * A, np.minimum(np.maximum(ratio, lo), hi) * A
    # THE RULE: the gradient flows where the unclipped term is the minimum; at a tie (A == 0, or lo <= ratio <= hi with the bounds included) it flows too
    gl = np.where(s1 <= s2, -A * ratio, 0.0) / count
    dmu = gl[:, None] * (q / sd)
    dls = (gl[:, None] * (q * q * (np.exp(ls) / sd) - 1.0)).sum(0)
    grad = _backward64(Ws, hs, zs, dmu, leak, dls)
    stats = np.array([(-np.minimum(s1, s2)).mean(), (lpo - logp).mean(), ((ratio > hi) | (ratio < lo)).mean(), ratio.mean()])
    if hidden_z:
        return grad, stats, zs, ratio
    return grad, stats


def imitation_grad_ref(theta, obs, act, loss, weight=None, leak=0.2):
    """The header's imitation law in closed form, float64: (grad [P], stats [4] = the chosen loss, weighted NLL, weighted MSE, 0)."""
    code = _loss_code(loss)
    if code not in (_lib.IMITATE_NLL, _lib.IMITATE_MSE):
        raise ValueError('unknown loss %r' % (loss,))
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    count, in_dim, out_dim = obs.shape[0], obs.shape[1], act.shape[1]
    w = np.ones(count) if weight is None else np.asarray(weight, np.float64)
    Ws, bs, ls, hs, zs, mu = _forward64(theta, obs, in_dim, out_dim, True, leak)
    sd = np.exp(ls) + 1e-8
    q = (act - mu) / sd
    logp = (-0.5 * ((q * q + 2.0 * ls) + math.log(2.0 * math.pi))).sum(1)
    e = mu - act
    nll, mse = (w * -logp).sum() / count, (w * (e * e).sum(1)).sum() / count
    if code == _lib.IMITATE_NLL:
        gl = -w / count
        dmu = gl[:, None] * (q / sd)
        dls = (gl[:, None] * (q * q * (np.exp(ls) / sd) - 1.0)).sum(0)
    else:
        dmu = (2.0 * w / count)[:, None] * e
        dls = np.zeros(out_dim)
    grad = _backward64(Ws, hs, zs, dmu, leak, dls)
    return grad, np.array([nll if code == _lib.IMITATE_NLL else mse, nll, mse, 0.0])


def alloc_loss_terms(p, tau, params=None):
    """The allocation loss's per-row terms at network outputs p [n, 6] for wrenches tau [n, >= 3] (include/dpenv.h, ALLOCATION LOSS), in
    float64 on the struct's float32 numbers: dict(r [n, 3] the wrench residual, Js, Jp, Jx, J [n], dp [n, 6] = dJ/dp)."""
    q = alloc_loss_params(params)
    t = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)    # the struct's f32 numbers
    ws, lx, ly, kf, kr, az = (t(q[k]) for k in ('w_slack', 'lx', 'ly', 'kf', 'kr', 'azimuth'))
    wp, wsat, ascale, mode = float(t(q['w_power'])), float(t(q['w_sat'])), float(t(q['angle_scale'])), int(q['azimuth_mode'])
    if mode not in (0, 1):
        raise ValueError('allocation loss: azimuth_mode is 0 or 1')
    p, tau = np.asarray(p, np.float64), np.asarray(tau, np.float64)
    pj = p[:, [2, 0, 1]]                                                            # env order bow, port, star
    n = 100.0 * np.clip(pj, -1.0, 1.0)
    K = np.where(n >= 0, kf, kr)
    F = (K * n) * np.abs(n)
    e = np.maximum(np.abs(pj) - 1.0, 0.0)
    dF = np.where(np.abs(pj) <= 1.0, (200.0 * K) * np.abs(n), 0.0)
    a = p[:, 3:5] * ascale if mode == 0 else np.broadcast_to(az, (p.shape[0], 2))
    s, c = np.sin(a), np.cos(a)
    b3 = lx[1:] * s - ly[1:] * c
    Fk = F[:, 1:]
    r = np.stack([(c * Fk).sum(1) - tau[:, 0], (F[:, 0] + (s * Fk).sum(1)) - tau[:, 1], (lx[0] * F[:, 0] + (b3 * Fk).sum(1)) - tau[:, 2]], 1)
    Js, Jp, Jx = (ws * (r * r)).sum(1), (np.abs(F) * (F * F)).sum(1), (e * e).sum(1)
    J = 0.5 * ((Js + wp * Jp) + wsat * Jx)
    wr = ws * r
    gF = np.empty_like(F)
    gF[:, 0] = wr[:, 1] + lx[0] * wr[:, 2]                                          # the bow thruster is pure sway: column (0, 1, lx_b)
    gF[:, 1:] = (c * wr[:, 0:1] + s * wr[:, 1:2]) + b3 * wr[:, 2:3]
    gF = gF + (1.5 * wp) * (F * np.abs(F))
    dp = np.zeros_like(p)
    dp[:, [2, 0, 1]] = gF * dF + wsat * np.copysign(e, pj)
    if mode == 0:
        d3 = lx[1:] * c + ly[1:] * s
        dp[:, 3:5] = ascale * ((-(Fk * s) * wr[:, 0:1] + (Fk * c) * wr[:, 1:2]) + (Fk * d3) * wr[:, 2:3])
    return dict(r=r, Js=Js, Jp=Jp, Jx=Jx, J=J, dp=dp)


def allocation_grad_ref(theta, x, tau, params, weight=None, leak=0.2):
    """The header's allocation loss in closed form, float64: (grad [P], stats [4] = L, weighted mean Js, Jp, Jx).  x [n, in], tau [n, 3] or
    [n, 6] (columns 3..5 are not read)."""
    x = np.asarray(x, np.float64)
    count, in_dim = x.shape
    w = np.ones(count) if weight is None else np.asarray(weight, np.float64)
    Ws, bs, _, hs, zs, p = _forward64(theta, x, in_dim, 6, True, leak)
    t = alloc_loss_terms(p, tau, params)
    grad = _backward64(Ws, hs, zs, (w / count)[:, None] * t['dp'], leak, np.zeros(6))
    return grad, np.array([(w * t[k]).sum() / count for k in ('J', 'Js', 'Jp', 'Jx')])


def value_grad_ref(theta, obs, ret, leak=0.2):
    """The critic's law in closed form, float64: (grad [P], stats [1] = v_loss)."""
    obs, ret = np.asarray(obs, np.float64), np.asarray(ret, np.float64)
    count = obs.shape[0]
    Ws, bs, _, hs, zs, out = _forward64(theta, obs, obs.shape[1], 1, False, leak)
    e = out[:, 0] - ret
    return _backward64(Ws, hs, zs, (2.0 * e / count)[:, None], leak), np.array([(e * e).mean()])


def _powi(b, e):
    p, b = 1.0, float(b)
    while e > 0:
        if e & 1:
            p *= b
        b *= b
        e >>= 1
    return p


def adam_step_ref(theta, grad, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, gate_kl=None, kl_limit=float('inf'), stop=0):
    """dpenv_adam_step in NumPy float32, operation by operation as include/dpenv.h writes it.  step: the steps taken so far.
    Returns (theta, m, v, step, stop) after the call; with the gate closed (gate_kl given and (stop or gate_kl > kl_limit)) only stop changes."""
    f = np.float32
    theta, grad, m, v = (np.asarray(x, f) for x in (theta, grad, m, v))
    if gate_kl is not None and (stop or f(gate_kl) > f(kl_limit)):
        return theta.copy(), m.copy(), v.copy(), int(step), 1
    t = int(step) + 1
    b1, b2 = f(beta1), f(beta2)
    step_size = f(lr) / f(1.0 - _powi(float(b1), t))
    bc2s = np.sqrt(f(1.0 - _powi(float(b2), t)))
    m2 = _fma32(f(1) - b1, grad - m, m)
    v2 = _fma32((f(1) - b2) * grad, grad, b2 * v)
    denom = np.sqrt(v2) / bc2s + f(eps)
    theta2 = _fma32(-step_size, m2 / denom, theta)
    return theta2, m2, v2, t, int(stop)


# ---- the supervised thrust allocator (src/sl/FFNN.py, train.py): an MSE fit on (u, alpha) labels with the imitation gradient, or a fit
# through the force map with the allocation gradient; the Adam step above either way ---------------------------------------------------
FIT_LOSSES = ('mse', 'wrench')


def _steps(iters, draw, grad, buf, adam, average=None, hist=None, stat0=0):
    """The one step loop of every fit here, `iters` times: idx = draw(k) (an int32 index tensor, or None = every row), grad(idx) writes
    the gradient and its statistics into buf, average(buf) in place if given (a multi-rank caller's all-reduce), hist[k] = buf[stat0:] if
    a history is kept (stream-ordered, device to device: the statistics are those BEFORE the step), adam() takes the step."""
    for k in range(iters):
        grad(draw(k))
        if average is not None:
            average(buf)
        if hist is not None:
            hist[k].copy_(buf[stat0:])
        adam()


class _RoundPool(object):
    """The aggregation pool of the round drivers (PPOUpdater.dagger, fit_nn_allocator_on_policy): `rounds` flights of T x n rows each, of
    which the last `keep` stay (None: all).  Checks the counts under the caller's name; round r writes slot r % keep of a preallocated
    [keep * T * n, w] block, and the first filled(r) rows of the block are then in use."""

    def __init__(self, who, rounds, T, iters, keep, n):
        rounds, T, iters = int(rounds), int(T), int(iters)
        if rounds < 1 or T < 1 or iters < 1:
            raise ValueError('%s: rounds, T and iters are >= 1' % who)
        keep = rounds if keep is None else int(keep)
        if keep < 1:
            raise ValueError('%s: keep >= 1' % who)
        self.rounds, self.T, self.iters, self.keep, self.n, self.R = rounds, T, iters, min(keep, rounds), n, T * n

    def slot(self, block, r):
        """Round r's rows of block [keep * T * n, w] as [T, n, w]."""
        s = r % self.keep
        return block[s * self.R:(s + 1) * self.R].view(self.T, self.n, -1)

    def filled(self, r):
        return min(r + 1, self.keep) * self.R


def nn_allocator_init(in_dim, seed):
    """The flat float32 start of fit_nn_allocator: glorot-uniform kernels from numpy.random.RandomState(seed), zero biases
    (tf.layers.dense's default, as policy.ActorCritic), a zero log_std tail."""
    L = layout(in_dim, 6, True)
    rng = np.random.RandomState(seed)
    Ws, bs = [], []
    for i in range(4):
        lim = math.sqrt(6.0 / (L['sizes'][i] + L['sizes'][i + 1]))
        Ws.append(rng.uniform(-lim, lim, size=(L['sizes'][i], L['sizes'][i + 1])).astype(np.float32))
        bs.append(np.zeros(L['sizes'][i + 1], np.float32))
    return flatten(Ws, bs, np.zeros(6, np.float32))


def nn_allocator_minibatches(rows, count, iters, seed):
    """fit_nn_allocator's minibatches [iters, count] (a CPU int64 tensor): the first `count` of a seeded torch.randperm per step."""
    torch = _torch()
    gen = torch.Generator(device='cpu')
    gen.manual_seed(int(seed))
    return torch.stack([torch.randperm(rows, generator=gen)[:count] for _ in range(int(iters))])


def fit_nn_allocator(dataset, in_dim=9, iters=200, lr=1e-3, minibatch=256, seed=0, leak=0.2, device='cuda:0', loss='mse', alloc_loss=None,
                     init=None):
    """Fit the neural thrust allocator (include/dpenv.h, "the neural thrust allocation") to a dataset of deploy.nn_allocator_dataset:
    FFNN.py's loss and optimiser - mean squared error, Adam - as `iters` steps of dpenv_imitation_grad(MSE) + dpenv_adam_step on
    minibatches drawn with a seeded generator, everything on the device, nothing read back inside the loop.  The network is the fused
    update's shape {in_dim, 80, 80, 80, 6} with the leaky-relu slope `leak` (0 = the reference's relu; the reference's 20-wide shape
    and every other hidden shape are flown by the allocator but not fitted here); the update sees it as an actor, whose log_std tail
    is carried and ignored.  in_dim 9: the dataset's inputs as they are; 3: its last three columns (the scaled wrench alone).
    loss: 'mse' (the above, on the labels dataset['y']) or 'wrench': the same loop, initialisation and minibatches with
    dpenv_allocation_grad on dataset['x'] and dataset['tau'] - the QP law's objective at the network's output, through the force map, no
    labels (include/dpenv.h, ALLOCATION LOSS).  alloc_loss: that loss's numbers, the dict of deploy.alloc_loss_defaults whole or in part
    (e.g. dict(w_power=0.05)); they also define the wrench figures below.
    init: a flat float32 theta [P] (an array, or a tensor on any device; P = layout(in_dim, 6, True)['P'], a fit's 'theta') to start from
    instead of nn_allocator_init(in_dim, seed); it is copied, not changed.  Adam's state starts at zero either way.  The dataset's x, y
    and tau may be float32 tensors (nn_wrench_rows' are): they are then used on the device without a host copy.
    Returns dict(W, b - views of the flat parameter tensor on the device, what env.set_nn_allocator and policy.thrust_alloc_nn read in
    place - leak, theta, loss; mse_initial, mse_final: mean_rows(sum_j (out_j - y_j)^2) over the WHOLE dataset before and after (None
    without dataset['y']); J_initial, J_final, wrench_ms_initial, wrench_ms_final: the allocation loss and its mean Js - the mean squared
    wrench residual [N^2] with the default w_slack - over the whole dataset before and after (None without dataset['tau']))."""
    torch = _torch()
    f32 = torch.float32
    if loss not in FIT_LOSSES:
        raise ValueError("fit_nn_allocator: loss must be 'mse' or 'wrench' (got %r)" % (loss,))
    is_t = lambda a: isinstance(a, torch.Tensor)
    host = lambda a: a if a is None or is_t(a) else np.asarray(a, np.float32)
    x, y, tau = host(dataset['x']), host(dataset.get('y')), host(dataset.get('tau'))
    if in_dim not in (3, 9) or len(x.shape) != 2 or x.shape[1] < in_dim:
        raise ValueError('fit_nn_allocator: in_dim is 3 or 9, the dataset has x [rows, >= in_dim]')
    if (loss == 'mse' or y is not None) and (y is None or tuple(y.shape) != (x.shape[0], 6)):
        raise ValueError("fit_nn_allocator: loss='mse' fits the labels y [rows, 6]")
    if (loss == 'wrench' or tau is not None) and (tau is None or tuple(tau.shape) != (x.shape[0], 3)):
        raise ValueError("fit_nn_allocator: loss='wrench' reads the wrenches tau [rows, 3]")
    rows = int(x.shape[0])
    if rows < 1:
        raise ValueError('fit_nn_allocator: the dataset has no rows')
    P = layout(in_dim, 6, True)['P']
    if init is not None:
        if not is_t(init):
            init = torch.as_tensor(np.asarray(init))
        if init.dim() != 1 or init.numel() != P or init.dtype != f32:
            raise ValueError('fit_nn_allocator: init is a flat float32 theta of %d entries for in_dim %d (got %s %s)'
                             % (P, in_dim, init.dtype, list(init.shape)))
    dev_of = lambda a: a.to(device=device, dtype=f32) if is_t(a) else torch.as_tensor(np.ascontiguousarray(a)).to(device)
    x = dev_of(x[:, x.shape[1] - in_dim:]).contiguous()
    if y is not None:
        y = dev_of(y).contiguous()
    if tau is not None:                                          # the kernel's [rows, 6] target rows: the wrench, then three columns nothing reads
        tau = dev_of(tau)
        tau = torch.cat([tau, torch.zeros_like(tau)], 1).contiguous()
    qp = alloc_loss_params(alloc_loss)
    theta = torch.as_tensor(nn_allocator_init(in_dim, seed)).to(device) if init is None else init.to(device).clone()
    m, v = torch.zeros(P, dtype=f32, device=device), torch.zeros(P, dtype=f32, device=device)
    step = torch.zeros(1, dtype=torch.int32, device=device)
    sh = make_shape(in_dim, 6, True, leak=leak)
    count = min(int(minibatch), rows)
    ws = torch.empty((workspace_bytes(sh, rows) + 3) // 4, dtype=f32, device=device)
    g = torch.empty(P + NSTAT_ACTOR, dtype=f32, device=device)
    idx_all = nn_allocator_minibatches(rows, count, iters, seed).to(torch.int32).to(device)

    def whole(kind):                                             # a statistic over the whole dataset; `g` is scratch here, read back at once
        if kind == 'mse':
            return None if y is None else [float(imitation_grad(theta, x, y, loss='mse', out=g, workspace=ws, leak=leak)[P])]
        return None if tau is None else [float(t) for t in allocation_grad(theta, x, tau, qp, out=g, workspace=ws, leak=leak)[P:P + 2]]

    mse0, wr0 = whole('mse'), whole('wrench')
    if loss == 'mse':
        grad = lambda idx: imitation_grad(theta, x, y, loss='mse', idx=idx, out=g, workspace=ws, leak=leak, count=count)
    else:
        grad = lambda idx: allocation_grad(theta, x, tau, qp, idx=idx, out=g, workspace=ws, leak=leak, count=count)
    _steps(int(iters), lambda k: idx_all[k], grad, g, lambda: adam_step(theta, g, m, v, step, lr))
    mse1, wr1 = whole('mse'), whole('wrench')
    tW, tb, _ = unflatten(theta, in_dim, 6, True)
    first = lambda s, k: None if s is None else s[k]
    return dict(W=list(tW), b=list(tb), leak=float(leak), theta=theta, loss=loss, mse_initial=first(mse0, 0), mse_final=first(mse1, 0),
                J_initial=first(wr0, 0), J_final=first(wr1, 0), wrench_ms_initial=first(wr0, 1), wrench_ms_final=first(wr1, 1))


def fit_nn_allocator_population(dataset, w_powers, alloc_loss=None, **fit):
    """K wrench-loss fits of one shape, one per power weight: for every w in w_powers, fit_nn_allocator(dataset, loss='wrench',
    alloc_loss=dict(alloc_loss or {}, w_power=w), **fit) - a loop over the existing fused gradient, each fit from the same
    initialisation and minibatches (fit: in_dim, iters, lr, minibatch, seed, leak, device, init).  Returns the list of the K fits'
    dicts, each with its 'w_power': what deploy.nn_population_stack, env.set_nn_allocator_population and evaluate.nn_allocator_sweep
    take."""
    ws = [float(w) for w in w_powers]
    if not ws:
        raise ValueError('fit_nn_allocator_population: w_powers is empty')
    if 'loss' in fit:
        raise ValueError("fit_nn_allocator_population: the fits are loss='wrench'")
    nets = []
    for w in ws:
        net = fit_nn_allocator(dataset, loss='wrench', alloc_loss=dict(alloc_loss or {}, w_power=w), **fit)
        net['w_power'] = w
        nets.append(net)
    return nets


def nn_wrench_rows(tau, in_dim=9, params=None):
    """Wrenches -> the rows fit_nn_allocator(loss='wrench') takes, on the device: tau, a float32 device tensor [R, 3] (N, N, Nm; a
    policy.controller_label_nn(tau=True) block viewed as rows), -> dict(x [R, in_dim], tau [R, 3]).  x[:, -3:] = tau * tau_scale, one
    float32 product per entry with tau_scale rounded to float32 first - the bits of the input the kernels form; with in_dim 9 the first
    six columns are in_const.  params: the dict of deploy.nn_allocator_defaults (None = the defaults)."""
    torch = _torch()
    from .deploy import nn_allocator_defaults
    if not isinstance(tau, torch.Tensor) or tau.dim() != 2 or tau.shape[1] != 3 or tau.dtype != torch.float32:
        raise ValueError('nn_wrench_rows: tau is a float32 tensor [R, 3]')
    if in_dim not in (3, 9):
        raise ValueError('nn_wrench_rows: in_dim is 3 or 9')
    p = nn_allocator_defaults() if params is None else params
    f32_of = lambda v: torch.as_tensor(np.asarray(v, np.float64).astype(np.float32)).to(tau.device)
    x = torch.empty((tau.shape[0], in_dim), dtype=torch.float32, device=tau.device)
    x[:, in_dim - 3:] = tau * f32_of(p['tau_scale'])
    if in_dim == 9:
        x[:, :6] = f32_of(p['in_const'])
    return dict(x=x, tau=tau)


def fit_nn_allocator_on_policy(env, rounds, T, iters, base=None, keep=None, lr=1e-3, minibatch=256, seed=0, leak=0.2, alloc_loss=None, in_dim=9):
    """Fit the neural allocator to the wrenches its own closed loop asks of it: `rounds` x (fly the PID + network chain, read the PID's
    clipped wrench on every row flown, refit through the force map).  The wrench loss needs no labels, only wrenches; the closed loop
    never writes them, the labelling scan does (policy.controller_label_nn(act=False, tau=True)).  env: an env with the baseline on
    (env.set_dp_controller) that can fly a network (no controller table, no QP allocator); its resets, currents, reference filter and
    hull randomisation are the caller's and decide which wrenches are flown.  base: an optional deploy.nn_allocator_dataset dict; it is
    fitted first - fit_nn_allocator(base, loss='wrench', seed=seed) from nn_allocator_init(in_dim, seed) - and its rows stay in the pool
    of every round.  Without base the first flight is the initial network's.  Per round r:
      1. env.set_nn_allocator(net) with the network so far (constants: the defaults, the leak `leak`)
      2. z = env.get_dp_controller_state(), then policy.controller_rollout(env, T)
      3. controller_label_nn(act=False, tau=True) on the block's obs / done from that z, written into slot `r % keep` of a preallocated
         wrench pool [keep * T * n, 3] (keep=None: every round has its own slot)
      4. fit_nn_allocator(loss='wrench', init=theta, seed=seed + 1 + r) on base's rows followed by nn_wrench_rows of the filled slots,
         rows whose wrench is not finite left out
    Adam's state starts at zero in every round (fit_nn_allocator owns it).  Returns dict(W, b, leak, theta - the last round's network, as
    fit_nn_allocator returns it -, rounds = one record per round: dict(rows, J_initial, J_final, wrench_ms_initial, wrench_ms_final) on
    that round's pool before and after its refit, base = the base fit's record (None without base), pool = the wrench pool
    [keep * T * n, 3], filled = its rows in use, T, n, keep).  The network is left set on the env; z and the env's state run on through
    the rounds."""
    torch = _torch()
    from .policy import controller_label_nn, controller_rollout
    n, dev, f32 = env.n_envs, env.device, torch.float32
    rp = _RoundPool('fit_nn_allocator_on_policy', rounds, T, iters, keep, n)
    if env.dp_controller is None:
        raise ValueError('fit_nn_allocator_on_policy: the baseline DP controller forms the wrench; env.set_dp_controller() first')
    rounds, T, iters, keep = rp.rounds, rp.T, rp.iters, rp.keep
    pool = torch.empty((keep * rp.R, 3), dtype=f32, device=dev)
    zbuf = torch.empty((3, n), dtype=f32, device=dev)
    fit_kw = dict(in_dim=in_dim, iters=iters, lr=lr, minibatch=minibatch, leak=leak, device=dev, loss='wrench', alloc_loss=alloc_loss)
    base_rec, bx, bt = None, None, None
    if base is not None:
        fit = fit_nn_allocator(base, seed=seed, **fit_kw)
        base_rec = {k: fit[k] for k in ('J_initial', 'J_final', 'wrench_ms_initial', 'wrench_ms_final')}
        base_rec['rows'] = int(np.shape(base['x'])[0])
        theta = fit['theta']
        bx = torch.as_tensor(np.ascontiguousarray(np.asarray(base['x'], np.float32)[:, -in_dim:])).to(dev)
        bt = torch.as_tensor(np.asarray(base['tau'], np.float32)).to(dev)
    else:
        theta = torch.as_tensor(nn_allocator_init(in_dim, seed)).to(dev)
    out, records = None, []
    for r in range(rounds):
        tW, tb, _ = unflatten(theta, in_dim, 6, True)
        env.set_nn_allocator(dict(W=list(tW), b=list(tb), leak=float(leak)))
        z = env.get_dp_controller_state()
        out = controller_rollout(env, T, out=out)
        controller_label_nn(env, out['obs'], out['done'], z=z, act=False, tau=True, out=(None, zbuf, rp.slot(pool, r)))
        filled = rp.filled(r)
        flown = pool[:filled]
        flown = flown[torch.isfinite(flown).all(1)]
        ds = nn_wrench_rows(flown, in_dim)
        if bx is not None:
            ds = dict(x=torch.cat([bx, ds['x']]), tau=torch.cat([bt, ds['tau']]))
        fit = fit_nn_allocator(ds, seed=seed + 1 + r, init=theta, **fit_kw)
        theta = fit['theta']
        rec = {k: fit[k] for k in ('J_initial', 'J_final', 'wrench_ms_initial', 'wrench_ms_final')}
        rec['rows'] = int(ds['x'].shape[0])
        records.append(rec)
    return dict(W=fit['W'], b=fit['b'], leak=float(leak), theta=theta, rounds=records, base=base_rec, pool=pool, filled=filled, T=T, n=n, keep=keep)


# ---- the whole update ----------------------------------------------------------------------------------------------------------------
class PPOUpdater(object):
    """The update of ppo.py:265-273 on the device for a cuda ``ActorCritic`` (9 or 6 -> 80 -> 80 -> 80 -> 7 / 1, leaky-relu or relu).

    The tensors of `ac` are re-homed as views of two flat vectors (``pi_theta`` [14 334], ``v_theta`` [13 841]), so ``ac.upload``,
    ``state_dict`` and ``forward_ref`` keep working on the values the kernels update.  Owns Adam's m and v, the step counters, the
    stop flag, the gradient buffers and the workspace."""

    def __init__(self, ac, pi_lr=3e-4, v_lr=1e-3, clip=0.2, target_kl=0.01, betas=(0.9, 0.999), eps=1e-8):
        torch = _torch()
        if ac.activation == 'tanh':
            raise ValueError('the fused update implements leaky-relu / relu networks (tanh is refused by the library)')
        if tuple(ac.hidden_sizes) != (HIDDEN,) * 3:
            raise ValueError('the fused update implements three hidden layers of 80 (got %r)' % (tuple(ac.hidden_sizes),))
        if not all(p.is_cuda for p in ac.parameters()):
            raise ValueError('the ActorCritic must live on the GPU: there is no CPU fallback')
        self.ac, self.clip, self.target_kl = ac, float(clip), float(target_kl)
        self.pi_lr, self.v_lr, self.betas, self.eps = float(pi_lr), float(v_lr), betas, float(eps)
        dev = ac.log_std.device
        self.device = dev
        with torch.no_grad():
            self.pi_theta = flatten(ac.pi_W, ac.pi_b, ac.log_std).detach().float().contiguous().clone()
            self.v_theta = flatten(ac.v_W, ac.v_b).detach().float().contiguous().clone()
        ac.pi_W, ac.pi_b, ac.log_std = unflatten(self.pi_theta, ac.obs_dim, ac.act_dim, True)
        ac.v_W, ac.v_b, _ = unflatten(self.v_theta, ac.obs_dim, 1, False)
        self.pi_shape = make_shape(ac.obs_dim, ac.act_dim, True, leak=ac.leak)
        self.v_shape = make_shape(ac.obs_dim, 1, False, leak=ac.leak)
        self.P_pi, self.P_v = param_count(self.pi_shape), param_count(self.v_shape)
        assert self.P_pi == self.pi_theta.numel() and self.P_v == self.v_theta.numel()
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
        self.pi_m, self.pi_v, self.v_m, self.v_v = z(self.P_pi), z(self.P_pi), z(self.P_v), z(self.P_v)
        self.pi_grad, self.v_grad = z(self.P_pi + NSTAT_ACTOR), z(self.P_v + NSTAT_CRITIC)
        self.pi_steps, self.v_steps, self.stop = z(1, torch.int32), z(1, torch.int32), z(1, torch.int32)
        self._pi_steps_host = 0
        self._ws, self._out = None, z(3, torch.float64)

    def _workspace(self, count):
        need = max(workspace_bytes(self.pi_shape, count), workspace_bytes(self.v_shape, count))
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = _torch().empty((need + 3) // 4, dtype=_torch().float32, device=self.device)
        return self._ws

    def _batch(self, obs, minibatch):
        """(rows N, rows per gradient step, the workspace for them)."""
        N = obs.shape[0]
        mb = N if minibatch is None else min(int(minibatch), N)
        return N, mb, self._workspace(mb)

    def _net(self, actor):
        if actor:
            return self.pi_theta, self.pi_grad, self.pi_m, self.pi_v, self.pi_steps, self.P_pi
        return self.v_theta, self.v_grad, self.v_m, self.v_v, self.v_steps, self.P_v

    def _loop(self, actor, grad, iters, N, mb, lr, average, hist=None, **gate):
        """_steps on the actor's or the critic's flat vector: indices drawn with torch.randint as the torch loop draws them (only when
        mb < N), grad(idx) into that net's gradient buffer, Adam at lr with this updater's betas and eps (gate: adam_step's gate)."""
        torch = _torch()
        theta, g, m, v, steps, P = self._net(actor)
        b1, b2 = self.betas
        _steps(iters, lambda k: torch.randint(0, N, (mb,), device=self.device).to(torch.int32) if mb < N else None, grad, g,
               lambda: adam_step(theta, g, m, v, steps, lr, b1, b2, self.eps, **gate), average, hist, P)

    def _read(self, actor, hist, iters, keep_optimizer_state):
        """A warm start's tail: the one read of its history, then that net's Adam m, v and step counter are zeroed, so PPO starts with
        a fresh optimiser - or, kept, the host's count of the actor's steps is advanced (ungated: every queued step was taken)."""
        out = hist.cpu()
        _, _, m, v, steps, _ = self._net(actor)
        if not keep_optimizer_state:
            m.zero_()
            v.zero_()
            steps.zero_()
        if actor:
            self._pi_steps_host = self._pi_steps_host + iters if keep_optimizer_state else 0
        return out

    def update(self, obs, act, adv, ret, logp_old, iters=80, minibatch=None, average=None):
        """Queue `iters` actor steps (gated on approx_kl > 1.5 target_kl, ppo.py:267-270) and `iters` critic steps, then read
        (pi_iters, kl, v_loss) back ONCE.  obs [N, od], act [N, ad], adv / ret / logp_old [N], float32 on the device.
        minibatch: rows per gradient step, drawn with torch.randint as the torch loop draws them (None or >= N: every row).
        average: callable applied in place to the flat [P + nstat] gradient-and-statistics buffer between gradient and Adam
        (a multi-rank caller's all-reduce)."""
        N, mb, ws = self._batch(obs, minibatch)
        leak = self.ac.leak
        self.stop.zero_()
        self._loop(True, lambda idx: ppo_actor_grad(self.pi_theta, obs, act, adv, logp_old, self.clip, idx=idx, out=self.pi_grad, workspace=ws,
                                                    leak=leak, stop_flag=self.stop, count=mb),
                   iters, N, mb, self.pi_lr, average, gate_kl=self.pi_grad[self.P_pi + 1:self.P_pi + 2], kl_limit=1.5 * self.target_kl,
                   stop_flag=self.stop)
        self._loop(False, lambda idx: value_grad(self.v_theta, obs, ret, idx=idx, out=self.v_grad, workspace=ws, leak=leak, count=mb),
                   iters, N, mb, self.v_lr, average)
        self._out[0] = self.pi_steps[0]
        self._out[1] = self.pi_grad[self.P_pi + 1]
        self._out[2] = self.v_grad[self.P_v]
        steps, kl, v_loss = self._out.tolist()                         # the one read
        pi_iters = int(steps) - self._pi_steps_host
        self._pi_steps_host = int(steps)
        return pi_iters, kl, v_loss

    # ---- the supervised warm start: demonstration rows (e.g. a controller_rollout of the DP baseline) before the first PPO epoch ----
    def pretrain(self, obs, act, iters, minibatch=None, loss='mse', weight=None, lr=None, average=None, keep_optimizer_state=False):
        """Queue `iters` x (imitation_grad -> adam_step, no gate) on the actor: obs [N, od], act [N, ad], weight [N] or None, float32 on
        the device; indices drawn as `update` draws them.  Returns the [iters, 4] history (chosen loss, weighted NLL, weighted MSE, 0 per
        step, each measured BEFORE that step's Adam), read back once.  Unless keep_optimizer_state, the actor's Adam m, v and step counter
        are then zeroed, so PPO starts with a fresh optimiser."""
        N, mb, ws = self._batch(obs, minibatch)
        hist = _torch().zeros((iters, NSTAT_ACTOR), dtype=_torch().float32, device=self.device)
        self._loop(True, lambda idx: imitation_grad(self.pi_theta, obs, act, loss=loss, weight=weight, idx=idx, out=self.pi_grad, workspace=ws,
                                                    leak=self.ac.leak, count=mb),
                   iters, N, mb, self.pi_lr if lr is None else float(lr), average, hist)
        return self._read(True, hist, iters, keep_optimizer_state)

    # ---- DAgger: expert labels on the states the ACTOR visits, aggregated over rounds (Ross et al. 2011) ----
    def dagger(self, env, rounds, T, iters, minibatch=None, loss='mse', keep=None, sample=False, reset_at_end=False, lr=None, average=None,
               upload=None, expert='pinv', qp_params=None, thruster_state='own', qp_table=None, nn_net=None, nn_constants=None):
        """`rounds` x (fly the actor, label its states with the baseline DP controller, aggregate, refit).  env: a float32-row env with
        the baseline on (env.set_dp_controller; a table of set_dp_controller_table in force is the one that labels).  Per round:
          1. ac.upload(env, **upload)                       (upload: keyword arguments of ActorCritic.upload, e.g. dict(precision='f32'))
          2. policy_rollout(env, T, sample=sample, reset_at_end=reset_at_end): the learner flies, T x n rows
          3. policy.controller_label on the block's obs / done: the expert's action on every state the learner saw.  The expert's
             integral z is carried along each env's rows, zeroed behind a done row, handed from round to round by this driver and zeroed
             when reset_at_end cuts every env
          4. the round's obs and labels go into slot `round % keep` of a preallocated [keep * T * n] dataset (keep=None: every round has
             its own slot); the labels are written there by the kernel
          5. pretrain(dataset[:filled], iters, minibatch, loss, lr=lr, average=average, keep_optimizer_state=True)
        Returns one record per round: dict(history=[iters, 4] imitation statistics (pretrain's), reward_per_step=the actor's mean reward
        on that round's flight, label_msd=the mean squared distance between the actor's act rows and the labels, rows=dataset rows fitted).
        The dataset stays on the updater as self.dagger_data = dict(obs [keep * T * n, od], act [.., ad], filled, T, n, keep).  The only
        host reads are pretrain's one per round and one for the flight figures after the last round.  Adam's state runs on through the
        rounds and is left as it is; the caller uploads the final actor where it wants it flown.
        A memoryless actor cannot represent ki * z: the labels depend on the integral, the actor sees o alone.  A caller who wants a target
        the actor can represent labels with a ki = 0 controller or table.
        expert: 'pinv' (the PID + pseudo-inverse law, as above) or 'qp': step 3 is policy.controller_label_qp, the same PID with the
        rate-limited QP allocation - the low-energy contender.  Its thruster state x is carried beside z: along each env's rows, from round
        to round, zeroed with z.  The QP's numbers are qp_params (the dict of deploy.qp_allocator_defaults), else the ones
        env.set_qp_allocator has in force, else the defaults of the DEFAULT hull, as evaluate.baseline_box_test takes them.  The env need
        not be able to fly the QP: per-env hulls (randomised ones too) and a controller table label like any other.  x is the expert's own
        recursion, not the thruster state the actor's actions would have left.
        thruster_state (expert='qp'): 'own' (the default: the recursion above, bit for bit the driver without this keyword) or 'flown':
        the round's out['act'] goes to controller_label_qp(flown=...), so row t is labelled from the thruster state the actor's executed
        action of row t - 1 left (dpenv_controller_label_qp_ex) - the expert's answer in the state the learner is in.  The thrust part
        of that state is a function of the observation's lagged thrust columns, which the actor sees.  x, the state the last executed
        row left, is handed from round to round and zeroed by reset_at_end.  qp_table (expert='qp'): a float32 device tensor [32, n]
        (deploy.qp_allocator_table), env i labelled with row i in qp_params['iterations'] solver steps (16 without qp_params) - one
        expert per env; the scalar numbers are then not read.
        expert='nn': step 3 is policy.controller_label_nn with the explicit network nn_net (a dict with 'W' and 'b', as
        train.fit_nn_allocator returns one; nn_constants: a dict of deploy.nn_allocator_defaults' entries to override) - the same PID
        with the neural allocation.  The network has no state: only z is carried.  The env need not fly the network: a controller table
        or a QP set label like any other.  thruster_state / qp_table are refused as for 'pinv'; nn_net goes with expert='nn' only.
        Not here: beta-mixed flights in which the expert executes some of the steps, an integral-augmented actor, bf16 rows (the gradient
        kernels take float32 rows: a bf16 env raises ValueError)."""
        torch = _torch()
        from .policy import controller_label, controller_label_nn, controller_label_qp, policy_rollout
        rp = _RoundPool('dagger', rounds, T, iters, keep, env.n_envs)
        rounds, T, iters, keep = rp.rounds, rp.T, rp.iters, rp.keep
        if expert not in ('pinv', 'qp', 'nn'):
            raise ValueError("dagger: expert is 'pinv', 'qp' or 'nn', not %r" % (expert,))
        if thruster_state not in ('own', 'flown'):
            raise ValueError("dagger: thruster_state is 'own' or 'flown', not %r" % (thruster_state,))
        if expert != 'qp' and (thruster_state != 'own' or qp_table is not None):
            raise ValueError("dagger: thruster_state and qp_table go with expert='qp' (the pseudo-inverse has no thruster state)")
        if (expert == 'nn') != (nn_net is not None) or (nn_constants is not None and expert != 'nn'):
            raise ValueError("dagger: expert='nn' labels with the network nn_net; nn_net and nn_constants go with expert='nn' only")
        if env.obs_torch_dtype != torch.float32:
            raise ValueError('dagger: the gradient kernels take float32 rows; make the env with float32 obs rows (got %s)' % (env.obs_torch_dtype,))
        if env.dp_controller is None:
            raise ValueError('dagger: the baseline DP controller labels the rows; env.set_dp_controller() first')
        n, od, ad = env.n_envs, env.num_states, env.num_actions
        dev, f32 = self.device, torch.float32
        data_obs = torch.empty((keep * rp.R, od), dtype=f32, device=dev)
        data_act = torch.empty((keep * rp.R, ad), dtype=f32, device=dev)
        self.dagger_data = dict(obs=data_obs, act=data_act, filled=0, T=T, n=n, keep=keep)
        z = torch.zeros((3, n), dtype=f32, device=dev)
        if expert == 'qp':
            from .deploy import qp_allocator_defaults
            x = torch.zeros((5, n), dtype=f32, device=dev)
            qp = qp_params if qp_params is not None else env.qp_allocator if env.qp_allocator is not None else qp_allocator_defaults()
        flight = torch.zeros((rounds, 2), dtype=torch.float64, device=dev)
        out, records = None, []
        for r in range(rounds):
            self.ac.upload(env, **(upload or {}))
            out = policy_rollout(env, T, out=out, sample=sample, reset_at_end=reset_at_end)
            labels = rp.slot(data_act, r)
            if expert == 'qp':                                         # neither flown nor a table: the call of the driver before them
                controller_label_qp(env, out['obs'], out['done'], z=z, x=x, params=qp if qp_table is None else None, out=(labels, z, x),
                                    flown=out['act'] if thruster_state == 'flown' else None, table=qp_table,
                                    iterations=int(qp['iterations']) if qp_table is not None else None)
                if reset_at_end:
                    x.zero_()
            elif expert == 'nn':
                controller_label_nn(env, out['obs'], out['done'], z=z, net=nn_net, out=(labels, z), **(nn_constants or {}))
            else:
                controller_label(env, out['obs'], out['done'], z=z, out=(labels, z))
            if reset_at_end:
                z.zero_()
            rp.slot(data_obs, r).copy_(out['obs'])
            filled = rp.filled(r)
            self.dagger_data['filled'] = filled
            flight[r, 0] = out['rew'].mean()
            flight[r, 1] = ((out['act'] - labels) ** 2).mean()
            hist = self.pretrain(data_obs[:filled], data_act[:filled], iters, minibatch=minibatch, loss=loss, lr=lr, average=average,
                                 keep_optimizer_state=True)
            records.append(dict(history=hist, rows=filled))
        for rec, (rew, msd) in zip(records, flight.tolist()):
            rec['reward_per_step'], rec['label_msd'] = rew, msd
        return records

    def pretrain_critic(self, obs, ret, iters, minibatch=None, lr=None, average=None, keep_optimizer_state=False):
        """The critic's half of the warm start: `iters` x (value_grad -> adam_step) on ret [N] (the demonstration's discounted returns).
        Returns the [iters, 1] history of v_loss, read back once; the critic's Adam state is then zeroed unless keep_optimizer_state."""
        N, mb, ws = self._batch(obs, minibatch)
        hist = _torch().zeros((iters, NSTAT_CRITIC), dtype=_torch().float32, device=self.device)
        self._loop(False, lambda idx: value_grad(self.v_theta, obs, ret, idx=idx, out=self.v_grad, workspace=ws, leak=self.ac.leak, count=mb),
                   iters, N, mb, self.v_lr if lr is None else float(lr), average, hist)
        return self._read(False, hist, iters, keep_optimizer_state)
