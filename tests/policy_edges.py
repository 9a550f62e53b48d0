"""Edge cases of the in-kernel actor-critic (plain NumPy / CPU torch, no GPU): the cases, the references and the bounds shared by
tests/test_policy_edges_cpu.py (are the cases fair, and where does the documented arithmetic itself hold its contract?) and
tests/test_gpu_policy_edges.py (the HIP kernels against float64).

Three evaluations of one network on one batch of float32 observation rows:
  ref64        oracle/policy_ref.actor_critic in float64 on the float32 parameters - the yardstick of every accuracy claim
  y32          the same forward in torch float32 on the CPU (ActorCritic.forward_ref / logp_ref) - what "an fp32 evaluation" gives
  split_model  a NumPy statement of the arithmetic include/dpenv.h and the comments of dpenv_policy_dev.h describe.  Written from
               that text, it never calls the library:
                 F32  W = Wh + Wl, x = xh + xl with hi = f16(.) (round to nearest even, subnormals kept, overflow to inf) and
                      lo = f16(. - hi); a layer is Wh xh + Wh xl + Wl xh accumulated exactly and rounded to float32 ONCE (the
                      kernel's f32 accumulation order is what the factor 2 / the K x 2^-24 floor of the GPU bound are for);
                      the first layer's bias is the weight of a constant-1 input (slot 15: split like a weight, the input's low part is
                      0), later biases are float32; activations in float32 on the accumulator, then split again.
                 F16  only Wh xh; the first layer's bias is f16.  leaky / relu: the accumulator is rounded to f16 first, then
                      max(h, h * f16(leak)) in f16 (act_pack's comment); tanh: in float32, then rounded to f16.
                 tanh is 1 - 2 / (exp2(2 log2(e) x) + 1) in float32 (dpenv_policy_dev.h: "evaluated in f32 as 1 - 2 / (exp(2x) + 1)").

Cases: the shipped shape 9-80-80-80-7 (+ 9-80-80-80-1), fixed seed, non-zero biases and distinct log_std as tests/test_gpu_policy.make_ac
draws them, N_ROWS = 97 observation rows (one full wave, then a wave with one full 32-env tile and a tile of one lane).

`in_domain(params, obs, activation, precision)` is the supported range as include/dpenv.h states it, evaluated on the actual rows and kernels: inside
it the accuracy constants C hold; `domain(case, ...)` is that of a case."""
import math

import numpy as np

F32, F16, F64 = np.float32, np.float16, np.float64
OBS_DIM, ACT_DIM, HIDDEN = 9, 7, (80, 80, 80)
N_ROWS = 97
SEED = 3
# The observation draw.  `overflow` multiplies the rows POISONED of `nominal` by 2^14, and only an INPUT can leave f16's range that way (a
# first-layer sum of in-range inputs stays below 2^15.1: |W| < 0.26).  So the draw is the first seed (of RandomState(1000 + seed)) at
# which each of those six rows holds an entry of magnitude >= 4.1 - x 2^14 that is >= 67 174, past 65 520 where f16(x) becomes inf,
# exactly and whatever the summation order.  tests/test_policy_edges_cpu.py asserts the property.
OBS_SEED = 2395
OBS_SCALE = np.array([3, 3, 0.3, 0.5, 0.2, 0.2, 0.5, 0.5, 0.5], F32)        # the scale vector of tests/test_gpu_policy*.py
ACTIVATIONS = ('leaky', 'relu', 'tanh')
PRECISIONS = ('f16', 'f32', 'f32_actor')
POISONED = (0, 31, 32, 63, 64, 96)                                           # first / last lane of every 32-env tile of the 97 rows
# name -> (log2 of the observation factor, weight factor in every layer)
CASES = {'nominal': (0, 1.0), 'zero': (None, 1.0), 'tiny': (-20, 1.0), 'far': (7, 1.0), 'far_heavy': (7, 2.0), 'heavy': (0, 4.0),
         'overflow': (0, 1.0)}
RANGE_CASES = tuple(c for c in CASES if c != 'overflow')
OVERFLOW_FACTOR = 2.0 ** 14
# the project's own accuracy numbers, relative to max(S, 1) with S = max |ref64| of the output tensor:
# F32 from include/dpenv.h ("within 1e-5 of an fp32 evaluation"), F16 from tests/test_gpu_policy.py:56
C = {'f32': 1e-5, 'f16': 2e-3}
# roundings along the fma chain to an output, counted as tests/test_gpu_ppo_update.py counts them: one fma per k of the padded input
# layer and of each 80-wide layer, + the activation
K_FORWARD = (16 + 1) + 3 * (80 + 1)
K_LOGP = K_FORWARD + 14                      # + the likelihood stage as tests/test_gpu_imitation.py counts it
F16_MAX = 65504.0
HIDDEN_LIMIT = 2.0 ** 15                     # include/dpenv.h: inputs and hidden values of a supported env stay below this
LEAK = {'leaky': 0.2, 'relu': 0.0, 'tanh': 0.2}


# ---------------------------------------------------------------- the supported domain (include/dpenv.h, ActorCritic.upload)
NOMINAL_OBS = 16.0              # |obs| below this is the training scale (the draws of `nominal` stay below 8)
# tanh: the largest growth at which C[precision] is promised.  Chosen from the CPU model (tests/test_policy_edges_cpu.py sweeps it at weights
# x 1, x 2, x 4 and at scalings that are no power of two): F32 stays below 4e-6 up to growth 2^5 and first misses 1e-5 at 2^7 (weights x 4);
# F16 stays below 1e-3 up to growth 2 and first misses 2e-3 at 2^3.
TANH_GROWTH_LIMIT = {'f32': 2.0 ** 5, 'f16': 2.0}


def weight_scale(p):
    """The largest max|W| / sqrt(6 / (fan_in + fan_out)) over the dense kernels of both networks, at least 1: how far the weights have grown
    past the bound of their glorot-uniform initialisation."""
    w = 1.0
    for name, W in p.items():
        if name.endswith('/kernel'):
            W = np.asarray(W, F64)
            w = max(w, float(np.abs(W).max()) / math.sqrt(6.0 / (W.shape[0] + W.shape[1])))
    return w


def growth_of(p, obs):
    """growth = max(1, max|obs| / 16) x weight_scale: the ONE definition, as include/dpenv.h words it"""
    return max(1.0, float(np.abs(np.asarray(obs, F64)).max()) / NOMINAL_OBS) * weight_scale(p)


def in_domain(p, obs, activation, precision):
    """True where include/dpenv.h promises C[precision] x max(S, 1) for these parameters on these observation rows:
      - every input magnitude below 2^15 (hidden magnitudes too: the CPU test asserts that for the cases);
      - leaky-relu / relu: nothing else - the output scale grows with the input's, and the error with it;
      - tanh, whose outputs stay O(1) while the rounding of its first layer's inputs grows with them: while growth_of(p, obs) is at most
        2^5 in F32 and at most 2 in F16.
    'f32_actor' is the actor of 'f32' and the critic of 'f16': in the domain where both are."""
    if precision == 'f32_actor':
        return in_domain(p, obs, activation, 'f32') and in_domain(p, obs, activation, 'f16')
    if not float(np.abs(obs).max()) < HIDDEN_LIMIT:
        return False
    if activation != 'tanh':
        return True
    return growth_of(p, obs) <= TANH_GROWTH_LIMIT[precision]


def domain(case, activation, precision):
    """in_domain of a case's own parameters and rows"""
    return in_domain(case_params(case, activation), case_obs(case), activation, precision)


# ---------------------------------------------------------------- cases
_cache = {}


def make_ac(activation, wscale=1.0, device='cpu', log_std=None):
    """ActorCritic of the shipped shape: glorot kernels (seed fixed) x wscale, biases and log_std as tests/test_gpu_policy.make_ac."""
    import torch
    from ml4ca_amd.policy import ActorCritic
    ac = ActorCritic(OBS_DIM, ACT_DIM, HIDDEN, seed=SEED, device='cpu', activation=activation)
    g = torch.Generator().manual_seed(SEED + 100)
    for b in ac.pi_b + ac.v_b:
        b.copy_((torch.rand(b.shape, generator=g) - 0.5) * 0.6)
    ac.log_std.copy_(torch.rand(ACT_DIM, generator=g) - 0.8)
    if log_std is not None:
        ac.log_std.copy_(torch.tensor(log_std, dtype=torch.float32))
    for W in ac.pi_W + ac.v_W:
        W.mul_(float(wscale))
    if str(device) != 'cpu':
        ac.pi_W, ac.pi_b = [w.to(device) for w in ac.pi_W], [b.to(device) for b in ac.pi_b]
        ac.v_W, ac.v_b = [w.to(device) for w in ac.v_W], [b.to(device) for b in ac.v_b]
        ac.log_std = ac.log_std.to(device)
        ac.device = torch.device(device)
    return ac


def nominal_obs(n=N_ROWS, seed=OBS_SEED):
    return (np.random.RandomState(1000 + seed).standard_normal((n, OBS_DIM)) * OBS_SCALE).astype(F32)


def case_obs(case, n=N_ROWS):
    """float32 [n, 9] observation rows of a case (n other than N_ROWS only for `nominal`-like cases: the small-batch tests)."""
    e, _ = CASES[case]
    if case == 'zero':
        # tile edges exactly zero; one non-zero entry per row elsewhere: +scale, -scale, an f16-subnormal and an f32-tiny value per input
        o = np.zeros((n, OBS_DIM), F32)
        for k in range(OBS_DIM):
            o[1 + k, k] = OBS_SCALE[k]
            o[33 + k, k] = -OBS_SCALE[k]
            o[65 + k, k] = OBS_SCALE[k] * F32(2.0 ** -16)
            o[80 + k, k] = -OBS_SCALE[k] * F32(2.0 ** -40)
        return o
    o = nominal_obs(n) * F32(2.0 ** e)
    if case == 'overflow':
        o[list(POISONED)] *= F32(OVERFLOW_FACTOR)
    return o


def params(activation, wscale=1.0):
    """{reference variable name: float32 array} of make_ac (cached, never changed)."""
    key = ('params', activation, float(wscale))
    if key not in _cache:
        _cache[key] = make_ac(activation, wscale).state_dict()
    return _cache[key]


def case_params(case, activation):
    return params(activation, CASES[case][1])


# ---------------------------------------------------------------- references
def net_layers(p, scope):
    Ws, bs, i = [], [], 0
    while True:
        name = '%s/dense%s' % (scope, '' if i == 0 else '_%d' % i)
        if name + '/kernel' not in p:
            return Ws, bs
        Ws.append(np.asarray(p[name + '/kernel'], F32))
        bs.append(np.asarray(p[name + '/bias'], F32))
        i += 1


def ref64(p, obs, activation):
    """(mu [n, 7], v [n]) float64: oracle/policy_ref.actor_critic on the float32 parameters, the slope the float32 value the kernel gets."""
    from oracle import policy_ref as PR
    return PR.actor_critic(p, np.asarray(obs, F64), activation=activation, leak=float(F32(LEAK[activation])))


def hidden64(p, obs, activation, scope):
    """float64 pre-activations [z1, z2, z3] ([n, 80] each) of one network."""
    Ws, bs = net_layers(p, scope)
    x, zs = np.asarray(obs, F64), []
    lk = 0.0 if activation == 'relu' else float(F32(LEAK[activation]))
    for W, b in zip(Ws[:-1], bs[:-1]):
        z = x @ W.astype(F64) + b
        zs.append(z)
        x = np.tanh(z) if activation == 'tanh' else np.where(z > 0, z, lk * z)
    return zs


def _ac_from(p, activation):
    from ml4ca_amd.policy import ActorCritic
    return ActorCritic.from_tensors(p, leak=LEAK[activation] if activation != 'relu' else 0.0, device='cpu', activation=activation)


def y32(p, obs, activation):
    """(mu, v) of torch float32 on the CPU (ActorCritic.forward_ref), as float64 arrays."""
    import torch
    with torch.no_grad():
        mu, v = _ac_from(p, activation).forward_ref(torch.from_numpy(np.ascontiguousarray(obs, F32)))
    return mu.double().numpy(), v.double().numpy()


def logp32(p, obs, act, activation):
    """ActorCritic.logp_ref(act | mu32(obs)) in torch float32, as a float64 array."""
    import torch
    with torch.no_grad():
        ac = _ac_from(p, activation)
        mu, _ = ac.forward_ref(torch.from_numpy(np.ascontiguousarray(obs, F32)))
        return ac.logp_ref(torch.from_numpy(np.ascontiguousarray(act, F32)), mu).double().numpy()


def logp64(p, obs, act, activation):
    from oracle import policy_ref as PR
    mu, _ = ref64(p, obs, activation)
    return PR.gaussian_likelihood(np.asarray(act, F64), mu, np.asarray(p['pi/log_std'], F64))


# ---------------------------------------------------------------- the documented arithmetic
def to_f16(x):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(x, F32).astype(F16)


def split(x):
    """x (float32) -> (hi, lo) as float64 arrays holding f16 values: hi = f16(x), lo = f16(x - f32(hi))"""
    x = np.asarray(x, F32)
    hi = to_f16(x)
    with np.errstate(over='ignore', invalid='ignore'):
        lo = to_f16(x - hi.astype(F32))
    return hi.astype(F64), lo.astype(F64)


def tanh32(z):
    """1 - 2 / (exp2(2 log2(e) z) + 1), every operation rounded to float32, the last two fused (fma(-2, rcp, 1))"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        e = np.exp2(np.asarray(z, F32) * F32(2.8853900817779268)).astype(F32)
        r = (F32(1.0) / (e + F32(1.0))).astype(F32)
        return (1.0 - 2.0 * r.astype(F64)).astype(F32)


def _act32(z, activation, leak):
    if activation == 'tanh':
        return tanh32(z)
    with np.errstate(invalid='ignore'):
        return np.fmax(z, (z * F32(leak)).astype(F32))          # v_max_f32 returns the operand that is a number


def _mlp_model(Ws, bs, obs, activation, leak, split_mode, hidden=None, pre=None):
    x = np.asarray(obs, F32)
    last = len(Ws) - 1
    for l, (W, b) in enumerate(zip(Ws, bs)):
        Wh, Wl = split(W)
        with np.errstate(over='ignore', invalid='ignore'):
            if split_mode:
                xh, xl = split(x)
                acc = xh @ Wh + xl @ Wh + xh @ Wl
                if l == 0:
                    bh, bl = split(b)
                    acc = acc + bh + bl
                else:
                    acc = acc + b.astype(F64)
            else:
                xh = to_f16(x).astype(F64)
                acc = xh @ Wh + (to_f16(b).astype(F64) if l == 0 else b.astype(F64))
            z = acc.astype(F32)
        if l == last:
            return z
        if pre is not None:
            pre.append(z)
        if split_mode:
            x = _act32(z, activation, leak)
        elif activation == 'tanh':
            x = to_f16(tanh32(z)).astype(F32)
        else:
            with np.errstate(over='ignore', invalid='ignore'):
                h = to_f16(z)
                hl = to_f16(h.astype(F32) * to_f16(leak).astype(F32))     # the product of two f16 values is exact in float32: one rounding
                x = np.fmax(h, hl).astype(F32)
        if hidden is not None:
            hidden.append(x)


def split_model(p, obs, activation, leak, precision, hidden=None):
    """(mu [n, 7], v [n]) float32 of the documented arithmetic.  precision: 'f16' | 'f32' | 'f32_actor'.  hidden: a dict that
    receives {'pi': [h1, h2, h3], 'v': [...]}, the activated hidden values ([n, 80] float32) that the next layer converts to f16, and
    {'pi_z': [z1, z2, z3], 'v_z': [...]}, the accumulators they are the activation of."""
    leak = 0.0 if activation == 'relu' else leak
    out = []
    for scope, sm in (('pi', precision in ('f32', 'f32_actor')), ('v', precision == 'f32')):
        Ws, bs = net_layers(p, scope)
        hs, zs = ([], []) if hidden is not None else (None, None)
        out.append(_mlp_model(Ws, bs, obs, activation, F32(leak), sm, hs, zs))
        if hidden is not None:
            hidden[scope], hidden[scope + '_z'] = hs, zs
    return out[0], out[1][:, 0]


# ---------------------------------------------------------------- errors and bounds
def scale_of(ref):
    return max(float(np.abs(ref).max()), 1.0)


def err(got, ref):
    """max |got - ref| with non-finite differences counted as inf"""
    d = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    return float('inf') if not np.isfinite(d).all() else float(d.max())


def evaluate(case, activation, n=N_ROWS):
    """Everything the tests need of one (case, activation), computed once and never changed: obs, ref64, y32 and split_model per precision."""
    key = ('eval', case, activation, n)
    if key not in _cache:
        p, obs = case_params(case, activation), case_obs(case, n)
        r = dict(obs=obs, params=p, ref=ref64(p, obs, activation), y32=y32(p, obs, activation), model={}, hidden={})
        for prec in ('f16', 'f32'):
            h = {}
            r['model'][prec] = split_model(p, obs, activation, LEAK[activation], prec, hidden=h)
            r['hidden'][prec] = h
        r['model']['f32_actor'] = (r['model']['f32'][0], r['model']['f16'][1])
        _cache[key] = r
    return _cache[key]


def tensor_precision(precision, j):
    """The arithmetic of output tensor j (0 = mu, 1 = v) in a mode: F32_ACTOR is F32's actor and F16's critic."""
    return {'f16': 'f16', 'f32': 'f32', 'f32_actor': ('f32', 'f16')[j]}[precision]


def range_bound(ev, precision, j):
    """The GPU bound of output tensor j: max(2 |split_model - ref64|_max, K 2^-24 max(S, 1)) - the kernel is pinned to its stated
    arithmetic whatever the case (2 = the allowance of tests/test_gpu_ppo_update.py for a different summation order)."""
    ref = ev['ref'][j]
    return max(2.0 * err(ev['model'][precision][j], ref), K_FORWARD * 2.0 ** -24 * scale_of(ref))


def record(path, line):
    print(line)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


# ---------------------------------------------------------------- the likelihood stage (log_std ends)
LOG_STD_ENDS = (-4.0, -4.0, -2.0, 0.0, 1.0, 1.0, -0.5)        # examples/train_ppo.py clamps log_std to [-4, 1]


def ends_noise(T, n, seed=SEED):
    """float32 [T, n, 7] standard-normal draws holding xi = 0 exactly (env 0 and a whole component), +-5, and ordinary draws."""
    xi = np.random.RandomState(2000 + seed).standard_normal((T, n, ACT_DIM)).astype(F32)
    xi[:, 1 % n, :] = 5.0
    xi[:, 2 % n, :] = -5.0
    xi[:, 0, :] = 0.0
    xi[:, :, 3] = 0.0
    xi[0, min(31, n - 1), 0], xi[0, min(32, n - 1), 1], xi[0, n - 1, 5] = 5.0, -5.0, 5.0
    return xi


def logp_scale(act, mu64, log_std):
    """S' = max_i sum_k (z_k^2 / 2 + |logp_const_k|): the sizes of the terms a row's log-likelihood is summed from"""
    ls = np.asarray(log_std, F64)
    z = (np.asarray(act, F64) - mu64) / (np.exp(ls) + 1e-8)
    const = np.abs(-ls - 0.5 * math.log(2.0 * math.pi))
    return float((0.5 * z * z + const).sum(-1).max())
