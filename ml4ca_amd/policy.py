"""Actor-critic of the reference PPO (spinup/algos/tf1/ppo/core.py:29-33,80-107) for the in-kernel rollout.

``ActorCritic`` holds the fp32 parameters in the reference's layout (dense kernels W[in][out], biases, log_std;
variable names pi/dense{,_1,_2,_3}/{kernel,bias}, pi/log_std, v/dense*) as torch tensors, offers an fp32 torch
forward pass (the numerics reference for tests and for the PPO update, which stays host-side glue), and uploads
itself to a ``BatchedRevoltEnv`` where libdpenv evaluates it on the matrix cores inside the rollout launch
(dpenv_policy.hip).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import _is_on, _torch


class ActorCritic(object):
    def __init__(self, obs_dim=9, act_dim=7, hidden_sizes=(80, 80, 80), leak=0.2, log_std_init=-0.5, seed=0, device='cpu',
                 activation='leaky'):
        """activation: the reference's --activation choices (train.py:24,31): 'leaky' (slope `leak`, default 0.2 as
        tf.nn.leaky_relu), 'relu' (= leaky with slope 0) or 'tanh'."""
        torch = _torch()
        if not (len(set(hidden_sizes)) == 1 and 1 <= len(hidden_sizes) <= 4):
            raise ValueError('equal hidden widths, 1..4 hidden layers (got %r)' % (tuple(hidden_sizes),))
        if activation not in ('leaky', 'relu', 'tanh'):
            raise ValueError("activation must be 'leaky', 'relu' or 'tanh' (got %r)" % (activation,))
        if activation == 'relu':
            leak = 0.0
        self.activation = activation
        self.obs_dim, self.act_dim, self.hidden_sizes, self.leak = obs_dim, act_dim, tuple(hidden_sizes), float(leak)
        g = torch.Generator().manual_seed(seed)
        self.device = torch.device(device)

        def net(out_dim):
            sizes = [obs_dim] + list(hidden_sizes) + [out_dim]
            Ws, bs = [], []
            for i in range(len(sizes) - 1):
                # tf.layers.dense default kernel initializer: glorot uniform, zero bias
                lim = math.sqrt(6.0 / (sizes[i] + sizes[i + 1]))
                Ws.append(((torch.rand((sizes[i], sizes[i + 1]), generator=g) * 2 - 1) * lim).to(self.device))
                bs.append(torch.zeros(sizes[i + 1], device=self.device))
            return Ws, bs

        self.pi_W, self.pi_b = net(act_dim)
        self.v_W, self.v_b = net(1)
        self.log_std = torch.full((act_dim,), float(log_std_init), device=self.device)      # core.py:83

    @classmethod
    def from_tensors(cls, tensors, leak=0.2, device='cpu', activation='leaky'):
        """Build from a {name: array} dict with the reference's variable names (core.py:103-106 scopes 'pi' and 'v',
        tf.layers.dense naming dense, dense_1, ...; pi/log_std) - e.g. the output of tf_checkpoint.read_bundle."""
        torch = _torch()

        def layers(scope):
            Ws, bs, i = [], [], 0
            while True:
                name = '%s/dense%s' % (scope, '' if i == 0 else '_%d' % i)
                if name + '/kernel' not in tensors:
                    break
                Ws.append(torch.tensor(np.asarray(tensors[name + '/kernel'], np.float32), device=device))
                bs.append(torch.tensor(np.asarray(tensors[name + '/bias'], np.float32), device=device))
                i += 1
            return Ws, bs

        pW, pb = layers('pi')
        vW, vb = layers('v')
        if not pW or not vW:
            raise ValueError("no 'pi/dense*/kernel' / 'v/dense*/kernel' variables found")
        hidden = tuple(int(w.shape[1]) for w in pW[:-1])
        ac = cls(int(pW[0].shape[0]), int(pW[-1].shape[1]), hidden, leak=leak, device=device, activation=activation)
        ac.pi_W, ac.pi_b, ac.v_W, ac.v_b = pW, pb, vW, vb
        ac.log_std = torch.tensor(np.asarray(tensors['pi/log_std'], np.float32), device=device)
        return ac

    @classmethod
    def from_tf_checkpoint(cls, prefix, leak=0.2, device='cpu', activation='leaky'):
        """Load a reference-trained model, e.g. '<model dir>/tf1_save/variables/variables' (logx.py:161-228)."""
        from .tf_checkpoint import read_bundle
        return cls.from_tensors(read_bundle(prefix), leak=leak, device=device, activation=activation)

    @classmethod
    def from_saved_model(cls, model_dir, device='cpu'):
        """Load a reference-trained model from its `tf1_save` directory (logx.py:161-228: `saved_model.pb` + `variables/`), taking the
        hidden activation and its slope from the saved GRAPH (tf_graph.py) instead of from the caller: the thesis' models are
        Maximum(0.2 x, x) (tf.nn.leaky_relu of TensorFlow 1.12), which is also how the kernels evaluate it."""
        import os
        from .tf_checkpoint import read_bundle
        from . import tf_graph
        g = tf_graph.read_saved_model(os.path.join(model_dir, 'saved_model.pb'))
        desc = tf_graph.describe_actor_critic(g)
        act, alpha = tf_graph.hidden_activation(desc)
        for net in ('pi', 'v'):                            # the shape this library evaluates: dense stacks, no activation behind the last layer
            for l in desc[net][:-1]:
                if len(l['ops']) != 3:
                    raise ValueError('unsupported saved graph: hidden layer %r is %r, expected MatMul -> BiasAdd -> activation' % (l['layer'], l['ops']))
            if desc[net][-1]['ops'] != ['MatMul', 'BiasAdd']:
                raise ValueError('unsupported saved graph: an activation (%r) follows the last layer %r' % (desc[net][-1]['ops'], desc[net][-1]['layer']))
        ac = cls.from_tensors(read_bundle(os.path.join(model_dir, 'variables', 'variables')), leak=float(np.float32(alpha)), device=device,
                              activation=act)
        ac.graph = desc
        return ac

    def state_dict(self):
        """{reference variable name: numpy array} (inverse of from_tensors)."""
        out = {}
        for scope, Ws, bs in (('pi', self.pi_W, self.pi_b), ('v', self.v_W, self.v_b)):
            for i, (W, b) in enumerate(zip(Ws, bs)):
                name = '%s/dense%s' % (scope, '' if i == 0 else '_%d' % i)
                out[name + '/kernel'] = W.detach().cpu().numpy()
                out[name + '/bias'] = b.detach().cpu().numpy()
        out['pi/log_std'] = self.log_std.detach().cpu().numpy()
        return out

    def parameters(self):
        return self.pi_W + self.pi_b + self.v_W + self.v_b + [self.log_std]

    def _mlp(self, x, Ws, bs):
        torch = _torch()
        for W, b in zip(Ws[:-1], bs[:-1]):
            x = torch.tanh(x @ W + b) if self.activation == 'tanh' else torch.nn.functional.leaky_relu(x @ W + b, self.leak)
        return x @ Ws[-1] + bs[-1]

    def forward_ref(self, obs):
        """fp32 torch reference: (mu [n, act_dim], v [n])."""
        return self._mlp(obs, self.pi_W, self.pi_b), self._mlp(obs, self.v_W, self.v_b)[:, 0]

    def logp_ref(self, act, mu):
        """gaussian_likelihood, core.py:42-46."""
        torch = _torch()
        pre = -0.5 * (((act - mu) / (torch.exp(self.log_std) + 1e-8)) ** 2 + 2 * self.log_std + math.log(2 * math.pi))
        return pre.sum(dim=1)

    def upload(self, env, precision='f16', launch_form='auto'):
        """Pack into the env's library handle (dpenv_set_policy_desc); call again after each PPO update.

        precision: 'f16' (fast mode: f16 weights / activations, f32 accumulation), 'f32' (split-f16 arithmetic within 1e-5 of an
        fp32 evaluation - the reference's networks are fp32, core.py:29-33) or 'f32_actor' (the actor - mu, action, logp - as in
        'f32', the critic as in 'f16': the PPO ratio is exact, values carry the fast mode's ~5e-4; ~1.5 x the speed of 'f32').
        launch_form: 'auto' | 'one_wave' | 'two_wave'.
        SUPPORTED RANGE of those figures (include/dpenv.h; tests/policy_edges.py domain()): observations and hidden activations pass
        through f16 in every mode, so their magnitudes must stay below 2^15.  An env outside that range gets meaningless rows
        (non-finite; finite and wrong in 'f16' with tanh) for that env alone - every other env of the launch keeps its rows bit for
        bit.  Below it, relative to S = max(largest |output|, 1): leaky / relu hold 1e-5 S ('f32') and 2e-3 S ('f16', 5e-4 S
        typical) at every observation and weight scale; tanh only while growth = max(1, max|obs| / 16) x weight scale is at most
        2^5 for 'f32' and at most 2 for 'f16', weight scale being the largest max|W| / sqrt(6 / (fan_in + fan_out)) over the dense
        kernels, at least 1.
        Parameters that live on the env's device are handed over as DEVICE pointers: one packing kernel on the current stream,
        no host copy and no synchronisation; parameters elsewhere (CPU tensors) go through a host copy."""
        torch = _torch()
        lib = env.lib
        on_dev = all(p.is_cuda and p.device == env.device and p.dtype == torch.float32 and p.is_contiguous() for p in self.parameters())
        keep = []

        def mk(Ws, bs):
            m = _lib.Mlp()
            m.n_layers = len(Ws)
            sizes = [Ws[0].shape[0]] + [w.shape[1] for w in Ws]
            for i, sz in enumerate(sizes):
                m.sizes[i] = int(sz)
            for i, (W, b) in enumerate(zip(Ws, bs)):
                if on_dev:
                    m.W[i], m.b[i] = W.data_ptr(), b.data_ptr()
                else:
                    Wn = np.ascontiguousarray(W.detach().float().cpu().numpy())
                    bn = np.ascontiguousarray(b.detach().float().cpu().numpy())
                    keep.extend([Wn, bn])
                    m.W[i], m.b[i] = Wn.ctypes.data, bn.ctypes.data
            return m

        pi, v = mk(self.pi_W, self.pi_b), mk(self.v_W, self.v_b)
        d = _lib.PolicyDesc()
        d.struct_size = C.sizeof(_lib.PolicyDesc)
        d.pi, d.v = C.pointer(pi), C.pointer(v)
        if on_dev:
            d.log_std = self.log_std.data_ptr()
        else:
            ls = np.ascontiguousarray(self.log_std.detach().float().cpu().numpy())
            keep.append(ls)
            d.log_std = ls.ctypes.data
        d.activation = _lib.ACT_TANH if self.activation == 'tanh' else _lib.ACT_LEAKY_RELU
        d.leak = float(self.leak)
        d.precision = {'f16': _lib.POLICY_F16, 'f32': _lib.POLICY_F32, 'f32_actor': _lib.POLICY_F32_ACTOR}[precision]
        d.launch_form = {'auto': _lib.LAUNCH_AUTO, 'one_wave': _lib.LAUNCH_ONE_WAVE, 'two_wave': _lib.LAUNCH_TWO_WAVE}[launch_form]
        d.device_pointers = 1 if on_dev else 0
        with torch.cuda.device(env.device):
            _lib.check(lib.dpenv_set_policy_desc(env._h, C.byref(d), env._stream()), env._h)
            if not on_dev:
                torch.cuda.current_stream(env.device).synchronize()      # the host arrays in `keep` must outlive the copies
        env._has_policy = True
        self.precision = precision
        return self


def policy_launch_form(env):
    """('two_wave' | 'one_wave', envs per workgroup) that the uploaded policy's rollouts run in (what 'auto' resolved to)."""
    tw, epw = C.c_int32(0), C.c_int32(0)
    _lib.check(env.lib.dpenv_get_policy_launch(env._h, C.byref(tw), C.byref(epw)), env._h)
    return ('two_wave' if tw.value else 'one_wave'), int(epw.value)


def policy_launch_info(env):
    """dict(two_wave, envs_per_workgroup, waves_per_64_envs, precision) of the uploaded policy as the LIBRARY resolved it
    (dpenv_get_policy_launch_ex): waves 1 = one-wave form, 2 = env + network wave, 3 = env + actor + critic wave."""
    out = (C.c_int32 * 4)()
    _lib.check(env.lib.dpenv_get_policy_launch_ex(env._h, out), env._h)
    return dict(two_wave=bool(out[0]), envs_per_workgroup=int(out[1]), waves_per_64_envs=int(out[2]),
                precision={_lib.POLICY_F16: 'f16', _lib.POLICY_F32: 'f32', _lib.POLICY_F32_ACTOR: 'f32_actor'}[int(out[3])])


def release_policy_graphs(env):
    """dpenv_release_policy_graphs: the HIP graphs that recorded closed-loop launches of this env are gone; uploads of any layout are accepted again."""
    _lib.check(env.lib.dpenv_release_policy_graphs(env._h), env._h)


def policy_forward(env, obs):
    """Deterministic actor mean and critic value for obs [n, obs_dim] on the env's device (dpenv_policy_forward)."""
    torch = _torch()
    n = obs.shape[0]
    env._chk(obs, (n, env.num_states), torch.float32, 'obs')
    mu = torch.empty((n, env.num_actions), dtype=torch.float32, device=env.device)
    v = torch.empty(n, dtype=torch.float32, device=env.device)
    _lib.check(env.lib.dpenv_policy_forward(env._h, env._ptr(obs), env._ptr(mu), env._ptr(v), n, env._stream()), env._h)
    return mu, v


def policy_rollout(env, T, noise=None, switch_steps=(), refs=None, out=None, sample=None, reset_at_end=False):
    """T steps of (actor -> sample -> env.step -> critic) in ONE launch: the rollout loop ppo.py:289-322 for every env.

    noise: float32 [T, n, act_dim] standard-normal draws (a = mu + exp(log_std) * noise, core.py:85), or None.  With noise None:
    sample=True draws the exploration noise inside the kernel (Philox keyed by the seed, the global env id and the number of
    actions the env has sampled so far - like tf.random_normal inside the reference's graph, core.py:85, but reproducible and
    independent of the rank count); sample=False / None is the deterministic policy a = mu (test_policy.py:90).  Returns a dict of blocks: obs [T,n,od] (policy inputs), act [T,n,ad],
    rew, val, logp, boot [T,n], done [T,n] uint8, last_obs [n,od], last_val [n].  GAE: rollout.gae(rew, val, end=done, boot=boot).
    reset_at_end: the reference's epoch boundary (ppo.py:305-322): every env is cut and re-drawn after step T-1 (dpenv.h).
    With the integral action on (env.set_integral_action) the launch applies it and out['integ'] [T,n,3] holds the I added to obs[t]
    (obs[..., :3] - integ is the true error).  With the reference filter on (env.set_reference_filter) the switches set the filter's
    targets, every step's new_ref is its position, and out['ref'] [T,n,3] holds the eta_d that obs[t] was formed against."""
    torch = _torch()
    n, od, ad = env.n_envs, env.num_states, env.num_actions
    f32, odt = torch.float32, env.obs_torch_dtype
    if noise is not None:
        env._chk(noise, (T, n, ad), f32, 'noise')
    io = _lib.PolicyRolloutIO()
    io.struct_size = C.sizeof(_lib.PolicyRolloutIO)
    env._schedule(io, switch_steps, refs)
    out = env._blocks((('obs', (T, n, od), odt), ('act', (T, n, ad), f32), ('rew', (T, n), f32), ('val', (T, n), f32), ('logp', (T, n), f32),
                       ('boot', (T, n), f32), ('done', (T, n), torch.uint8), ('last_obs', (n, od), odt), ('last_val', (n,), f32)), out)
    filt, integ = env.reference_filter is not None, env.integral_action is not None
    for key, on in (('ref', filt), ('integ', integ)):
        if on:
            env._blocks(((key, (T, n, 3), f32),), out, fill=True)
    io.T = int(T)
    io.noise = noise.data_ptr() if noise is not None else None
    io.obs, io.act, io.reward = out['obs'].data_ptr(), out['act'].data_ptr(), out['rew'].data_ptr()
    io.value, io.logp, io.done = out['val'].data_ptr(), out['logp'].data_ptr(), out['done'].data_ptr()
    io.boot, io.last_obs, io.last_value = out['boot'].data_ptr(), out['last_obs'].data_ptr(), out['last_val'].data_ptr()
    io.sample = 1 if (sample and noise is None) else 0
    io.reset_at_end = 1 if reset_at_end else 0
    ipt = out['integ'].data_ptr() if integ else None
    if filt:
        rc = env.lib.dpenv_policy_rollout_deployed(env._h, C.byref(io), out['ref'].data_ptr(), ipt, env._stream())
    elif integ:
        rc = env.lib.dpenv_policy_rollout_integral(env._h, C.byref(io), ipt, env._stream())
    else:
        rc = env.lib.dpenv_policy_rollout(env._h, C.byref(io), env._stream())
    _lib.check(rc, env._h)
    return out


def controller_rollout(env, T, switch_steps=(), refs=None, out=None):
    """T steps of (baseline DP controller -> env.step) in ONE launch (dpenv_controller_rollout): the PID + pseudo-inverse law of
    env.set_dp_controller evaluated in registers on each observation, the classical counterpart of policy_rollout on the same plant.
    Returns a dict of blocks with policy_rollout's keys and row conventions: obs [T,n,9] (the controller's inputs), act [T,n,7],
    rew [T,n], done [T,n] uint8, last_obs [n,9]; with the reference filter on (env.set_reference_filter) also ref [T,n,3], the eta_d
    obs[t] was formed against.  ScoreCard.add consumes the dict unchanged."""
    torch = _torch()
    n, od, ad = env.n_envs, env.num_states, env.num_actions
    f32, odt = torch.float32, env.obs_torch_dtype
    io = _lib.ControllerRolloutIO()
    io.struct_size = C.sizeof(_lib.ControllerRolloutIO)
    env._schedule(io, switch_steps, refs)
    out = env._blocks((('obs', (T, n, od), odt), ('act', (T, n, ad), f32), ('rew', (T, n), f32), ('done', (T, n), torch.uint8),
                       ('last_obs', (n, od), odt)), out)
    io.T = int(T)
    io.obs, io.act, io.reward, io.done = out['obs'].data_ptr(), out['act'].data_ptr(), out['rew'].data_ptr(), out['done'].data_ptr()
    io.last_obs = out['last_obs'].data_ptr()
    io.ref_out = None
    if env.reference_filter is not None:
        io.ref_out = env._blocks((('ref', (T, n, 3), f32),), out, fill=True)['ref'].data_ptr()
    _lib.check(env.lib.dpenv_controller_rollout(env._h, C.byref(io), env._stream()), env._h)
    return out


def controller_label(env, obs, done=None, z=None, out=None):
    """The baseline DP controller's actions on a block of rows some OTHER flight wrote (dpenv_controller_label), in one launch: expert
    labels for the states an actor visited, or the baseline's answer beside the actor's on the same states.  obs [T, n, 9] float32 or
    bfloat16 on the env's device (the block's own dtype, whatever the env writes), rows in policy_rollout's conventions; done [T, n]
    uint8 or None (no episode ends in the block); z [3, n] float32, the integral every env starts from (get_dp_controller_state's
    layout), or None = 0.  Per row: the law of env.set_dp_controller - row i of the table while set_dp_controller_table has one in
    force - on obs[t], z advanced first and zeroed behind a done row.  Returns (act [T, n, 7], z [3, n]); out = (act, z) supplies the
    buffers (z may be the input tensor itself).  Nothing of the env changes: not its state, not its own z, not a counter.  For float32
    rows of controller_rollout with auto-reset on the labels are that launch's act rows bit for bit.  deploy.label_rows is the host
    statement."""
    T, (act, z_out) = _label_front('controller_label', env, obs, done, z, out, more=())
    io = _label_io(_lib.ControllerLabelIO(), T, obs, done, z, z_out, act)
    _lib.check(env.lib.dpenv_controller_label(env._h, C.byref(io), env._stream()), env._h)
    return act, z_out


def _label_front(who, env, obs, done, z, out=None, more=None):
    """The opening of the controller_label* scans: obs is a [T, n, 9] float32 or bfloat16 block (refused under the caller's name `who`),
    done [T, n] uint8 or None, z [3, n] float32 or None.  Returns T and the float32 out buffers - act [T, n, 7], z [3, n], then one per
    shape in `more` - as a tuple: the caller's out tuple checked (_chk, named out[j]), or new tensors when out is None.  more=None
    leaves the buffers to the caller (None is returned for them)."""
    torch = _torch()
    n, f32 = env.n_envs, torch.float32
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
        raise ValueError('%s: obs is a tensor [T, n, 9]' % who)
    if obs.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('%s: obs rows are float32 or bfloat16, not %s' % (who, obs.dtype))
    T = int(obs.shape[0])
    env._chk(obs, (T, n, 9), obs.dtype, 'obs')
    env._chk(done, (T, n), torch.uint8, 'done')
    env._chk(z, (3, n), f32, 'z')
    if more is None:
        return T, None
    shapes = ((T, n, 7), (3, n)) + tuple(more)
    if out is not None and len(out) != len(shapes):
        raise ValueError('%s: out holds %d buffers' % (who, len(shapes)))
    blk = env._blocks(tuple((j, shape, f32) for j, shape in enumerate(shapes)), out)
    return T, tuple(blk[j] for j in range(len(shapes)))


def _label_io(io, T, obs, done, z, z_out, act):
    """The fields the four label io structs share, into a new one of them."""
    io.struct_size = C.sizeof(io)
    io.T = T
    io.obs = obs.data_ptr()
    io.obs_dtype = 1 if obs.dtype == _torch().bfloat16 else 0
    io.done = done.data_ptr() if done is not None else None
    io.z_in = z.data_ptr() if z is not None else None
    io.z_out = z_out.data_ptr()
    io.act = act.data_ptr() if act is not None else None
    return io


def qp_allocator_struct(params=None):
    """dpenv_qp_allocator for deploy.qp_allocator_defaults' dict; None = the library's defaults (the default hull's)."""
    q = _lib.QPAllocator()
    if params is None:
        _lib.check(_lib.load().dpenv_qp_allocator_defaults(C.byref(q)))
        return q
    q.struct_size = C.sizeof(_lib.QPAllocator)
    q.iterations = int(params['iterations'])
    q.w_power, q.w_dalpha, q.w_dforce = float(params['w_power']), float(params['w_dalpha']), float(params['w_dforce'])
    for name, count in (('w_slack', 3), ('f_max', 3), ('force_rate', 3), ('azimuth_rate', 2), ('lx', 3), ('ly', 3), ('kf', 3), ('kr', 3)):
        if len(params[name]) != count:
            raise ValueError('qp_allocator_struct: %s has %d entries, want %d' % (name, len(params[name]), count))
        for k in range(count):
            getattr(q, name)[k] = float(params[name][k])
    return q


def controller_label_qp(env, obs, done=None, z=None, x=None, params=None, out=None, cost=False, flown=None, table=None, iterations=None,
                        refused=None):
    """The PID + rate-limited QP chain's actions on a block of rows some OTHER flight wrote (dpenv_controller_label_qp), in one launch:
    controller_label with the QP law in place of the pseudo-inverse - the low-energy expert's labels for the states an actor visited.
    obs [T, n, 9] float32 or bfloat16, done [T, n] uint8 or None, z [3, n] float32 or None = 0 as controller_label takes them; x [5, n]
    float32, the thruster state every env starts from (get_qp_allocator_state's layout), or None = 0.  Per row: the PID lines of
    env.set_dp_controller (row i of the table while one is in force) on obs[t] with z advanced first, the QP law on that wrench with
    x advanced, both zeroed behind a done row.  params: the dict of deploy.qp_allocator_defaults; None = the numbers
    env.set_qp_allocator has in force (an error if none is set).  The env's hull kind does not matter: an env with per-env hulls or a
    controller table, which cannot fly the QP, labels with explicit params.  Returns (act [T, n, 7], z [3, n], x [5, n]) and, with
    cost=True, the final objective of every row's solve [T, n] as a fourth value; out = (act, z, x) supplies the buffers (z and x may
    be the input tensors themselves).  Nothing of the env changes: not its state, not its own z or thruster state, not a counter.  For
    float32 rows of controller_rollout with the QP set and auto-reset on the labels are that launch's act rows bit for bit.
    deploy.label_rows_qp is the host statement.
    flown [T, n, 7] float32 (dpenv_controller_label_qp_ex): the actions that were EXECUTED on these rows - a policy_rollout's out['act'].
    Row t is then solved from the thruster state the executed row t - 1 left (deploy.qp_state_from_action) instead of the expert's own
    recursion; the x returned is the state the last executed row left, to hand to the next block.  table: a float32 device tensor [32, n]
    (deploy.qp_allocator_table) - env i is labelled with row i, in `iterations` solver steps (None = 16); giving params too is an error.
    Each lane checks its own row: a refused one runs the rest allocator (zero thrust, azimuths held), reports a NaN objective and sets
    its byte of refused (a uint8 tensor [n], or None).  With neither flown nor table the call is dpenv_controller_label_qp itself."""
    torch = _torch()
    n, f32 = env.n_envs, torch.float32
    if table is not None and params is not None:
        raise ValueError('controller_label_qp: params or table, not both')
    if table is None and (iterations is not None or refused is not None):
        raise ValueError('controller_label_qp: iterations and refused go with table (params carries its own iterations)')
    T, (act, z_out, x_out) = _label_front('controller_label_qp', env, obs, done, z, out, more=((5, n),))
    env._chk(x, (5, n), f32, 'x')
    J = torch.empty((T, n), dtype=f32, device=env.device) if cost else None
    q = qp_allocator_struct(params) if params is not None else None
    ex = flown is not None or table is not None
    io = _label_io(_lib.ControllerLabelQpExIO() if ex else _lib.ControllerLabelQpIO(), T, obs, done, z, z_out, act)
    io.x_in = x.data_ptr() if x is not None else None
    io.x_out = x_out.data_ptr()
    io.cost = J.data_ptr() if cost else None
    io.q = C.pointer(q) if q is not None else None
    call = env.lib.dpenv_controller_label_qp
    if ex:
        env._chk(flown, (T, n, 7), f32, 'flown')
        env._chk(table, (32, n), f32, 'table')
        env._chk(refused, (n,), torch.uint8, 'refused')
        io.flown = flown.data_ptr() if flown is not None else None
        io.qp_table = table.data_ptr() if table is not None else None
        io.iterations = (16 if iterations is None else int(iterations)) if table is not None else 0
        io.refused_out = refused.data_ptr() if refused is not None else None
        call = env.lib.dpenv_controller_label_qp_ex
    _lib.check(call(env._h, C.byref(io), env._stream()), env._h)
    return (act, z_out, x_out, J) if cost else (act, z_out, x_out)


def thrust_alloc_qp(tau, state=None, params=None, dt=0.2, out=None, cost=False, table=None, iterations=None, refused=None):
    """One control step of the rate-limited QP thrust allocation on the device (dpenv_thrust_alloc_qp), one lane per env: tau float32
    [3, n] = Fx, Fy, Mz and the thruster state in force, state float32 [5, n] = F_bow, F_port, F_star, a_port, a_star (None = zeros), ->
    (action [n, 7], new state [5, n]) and, with cost=True, the final objective [n] as a third value.  params: the dict of
    deploy.qp_allocator_defaults (None = the defaults); dt the control period.  out = (action, state) supplies the buffers; the state
    buffer may be the input tensor itself.  An env whose tau is not finite keeps its state and commands it.  Handle-free: a caller with
    its own motion controller closes the loop with this between two launches.  deploy.BatchedQPAllocator is the host statement.
    table: a float32 device tensor [32, n] (deploy.qp_allocator_table) - env i is allocated with row i (dpenv_thrust_alloc_qp_table), in
    iterations solver steps (None = 16); giving params too is an error.  Each lane checks its own row: a refused one runs the rest
    allocator (zero thrust, azimuths held), reports a NaN objective and sets its byte of refused (a uint8 tensor [n], or None)."""
    torch = _torch()
    lib = _lib.load()
    f32 = torch.float32
    if not isinstance(tau, torch.Tensor) or tau.dim() != 2 or tau.shape[0] != 3 or tau.dtype != f32 or not tau.is_cuda or not tau.is_contiguous():
        raise ValueError('thrust_alloc_qp: tau is a contiguous float32 device tensor [3, n]')
    n = int(tau.shape[1])

    def chk(t, shape, what):
        if not _is_on(t, shape, f32, tau.device):
            raise ValueError('thrust_alloc_qp: %s is a contiguous float32 tensor %s on tau\'s device' % (what, list(shape)))

    if state is not None:
        chk(state, (5, n), 'state')
    if out is None:
        out = (torch.empty((n, 7), dtype=f32, device=tau.device), torch.empty((5, n), dtype=f32, device=tau.device))
    act, state_out = out
    chk(act, (n, 7), 'out[0]')
    chk(state_out, (5, n), 'out[1]')
    J = torch.empty((n,), dtype=f32, device=tau.device) if cost else None
    s = _lib._s(tau)
    if table is not None:
        if params is not None:
            raise ValueError('thrust_alloc_qp: params or table, not both')
        chk(table, (32, n), 'table')
        if refused is not None and not _is_on(refused, (n,), torch.uint8, tau.device):
            raise ValueError('thrust_alloc_qp: refused is a contiguous uint8 tensor [%d] on tau\'s device' % n)
        with torch.cuda.device(tau.device):
            _lib.check(lib.dpenv_thrust_alloc_qp_table(C.c_void_p(table.data_ptr()), 16 if iterations is None else int(iterations), float(dt),
                                                       C.c_void_p(tau.data_ptr()), C.c_void_p(state.data_ptr()) if state is not None else None,
                                                       C.c_void_p(state_out.data_ptr()), C.c_void_p(act.data_ptr()),
                                                       C.c_void_p(J.data_ptr()) if cost else None,
                                                       C.c_void_p(refused.data_ptr()) if refused is not None else None, n, s))
        return (act, state_out, J) if cost else (act, state_out)
    if iterations is not None or refused is not None:
        raise ValueError('thrust_alloc_qp: iterations and refused go with table (params carries its own iterations)')
    q = qp_allocator_struct(params)
    with torch.cuda.device(tau.device):
        _lib.check(lib.dpenv_thrust_alloc_qp(C.byref(q), float(dt), C.c_void_p(tau.data_ptr()),
                                             C.c_void_p(state.data_ptr()) if state is not None else None, C.c_void_p(state_out.data_ptr()),
                                             C.c_void_p(act.data_ptr()), C.c_void_p(J.data_ptr()) if cost else None, n, s))
    return (act, state_out, J) if cost else (act, state_out)


def _in_place(tensors, device):
    """Every entry is a contiguous float32 tensor on `device`: what the library can read where it is (device_pointers = 1)."""
    torch = _torch()
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous()
               for t in tensors)


def _nn_alloc_map(who, tau, out, raw, struct, call):
    """What thrust_alloc_nn and thrust_alloc_nn_population share: the check of tau, the allocator struct (struct(device) -> a tuple the
    call reads and that keeps the struct's arrays alive), the action and raw buffers, and the launch on tau's device and current stream:
    call(that tuple, tau, action, raw or None, n, stream) is the one library call."""
    torch = _torch()
    f32 = torch.float32
    if not isinstance(tau, torch.Tensor) or tau.dim() != 2 or tau.shape[0] != 3 or tau.dtype != f32 or not tau.is_cuda or not tau.is_contiguous():
        raise ValueError('%s: tau is a contiguous float32 device tensor [3, n]' % who)
    n = int(tau.shape[1])
    st = struct(tau.device)
    act, p = (out if raw else (out, None)) if out is not None else (None, None)
    if act is None:
        act = torch.empty((n, 7), dtype=f32, device=tau.device)
    if raw and p is None:
        p = torch.empty((n, 6), dtype=f32, device=tau.device)
    for t, shape, what in ((act, (n, 7), 'action'), (p, (n, 6), 'raw')):
        if t is not None and not _is_on(t, shape, f32, tau.device):
            raise ValueError('%s: the %s buffer is a contiguous float32 tensor %s on tau\'s device' % (who, what, list(shape)))
    s = _lib._s(tau)
    with torch.cuda.device(tau.device):
        _lib.check(call(st, C.c_void_p(tau.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(p.data_ptr()) if p is not None else None, n, s))
    return (act, p) if raw else act


def nn_allocator_struct(net, params, device):
    """(dpenv_nn_allocator, keep) for a net (deploy.nn_net_arrays' forms) and the dict of deploy.nn_allocator_defaults.  If every W and b
    is a contiguous float32 tensor on `device`, they are handed over as DEVICE pointers (device_pointers = 1: no copy - the optimiser's
    own tensors, a graph replay reads their contents of that moment); else as host arrays (device_pointers = 0).  keep holds what the
    struct points to: keep it alive until the call that takes the struct has returned."""
    from .deploy import nn_net_arrays, nn_net_sizes
    Ws, bs = (net['W'], net['b']) if isinstance(net, dict) else net
    on_dev = _in_place(list(Ws) + list(bs), device)
    sizes = nn_net_sizes(Ws, bs)
    hW, hb = (None, None) if on_dev else nn_net_arrays(net)    # (no copy of device tensors: the call stays capturable)
    m = _lib.Mlp()
    m.n_layers = len(sizes) - 1
    for i, sz in enumerate(sizes):
        m.sizes[i] = int(sz)
    for i in range(len(sizes) - 1):
        if on_dev:
            m.W[i], m.b[i] = Ws[i].data_ptr(), bs[i].data_ptr()
        else:
            m.W[i], m.b[i] = hW[i].ctypes.data, hb[i].ctypes.data
    a = _lib.NNAllocator()
    a.struct_size = C.sizeof(_lib.NNAllocator)
    a.net = C.pointer(m)
    a.leak = float(params['leak'])
    for name, count in (('in_const', 6), ('tau_scale', 3), ('azimuth', 2)):
        if len(params[name]) != count:
            raise ValueError('nn_allocator_struct: %s has %d entries, want %d' % (name, len(params[name]), count))
        for k in range(count):
            getattr(a, name)[k] = float(params[name][k])
    a.angle_scale = float(params['angle_scale'])
    a.azimuth_mode = int(params['azimuth_mode'])
    a.device_pointers = 1 if on_dev else 0
    return a, (m, hW, hb, Ws, bs)


def nn_population_struct(nets, params, device):
    """(dpenv_nn_allocator, K, keep) for a population - a list of nets or the stacked dict of deploy.nn_population_stack - and the dict
    of deploy.nn_allocator_defaults: nn_allocator_struct with W[l] [K, in, out] and b[l] [K, out] behind the pointers (sizes are one
    network's).  Stacked contiguous float32 tensors on `device` are handed over in place (device_pointers = 1), anything else as host
    arrays (device_pointers = 0)."""
    from .deploy import nn_population_stack
    st = nn_population_stack(nets)
    K = int(st['W'][0].shape[0])
    one = dict(W=[w[0] for w in st['W']], b=[b[0] for b in st['b']])
    a, keep = nn_allocator_struct(one, params, device)            # the shape, the constants (and network 0's addresses, replaced below)
    on_dev = _in_place(list(st['W']) + list(st['b']), device)
    if on_dev:
        Ws, bs = list(st['W']), list(st['b'])
        ptr = lambda t: t.data_ptr()
    else:
        cv = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t), dtype=np.float32)
        Ws, bs = [cv(w) for w in st['W']], [cv(b) for b in st['b']]
        ptr = lambda t: t.ctypes.data
    m = keep[0]
    for l in range(len(Ws)):
        m.W[l], m.b[l] = ptr(Ws[l]), ptr(bs[l])
    a.device_pointers = 1 if on_dev else 0
    return a, K, (keep, Ws, bs, st)


def nn_population_to(nets, device):
    """The population's stacked W and b as contiguous float32 tensors on `device` (tensors already there are kept as they are)."""
    from .deploy import nn_population_stack
    st = nn_population_stack(nets)
    out = nn_net_to(dict(W=st['W'], b=st['b']), device)
    out['b'] = [b.reshape(w.shape[0], -1) for w, b in zip(out['W'], out['b'])]
    if 'leak' in st:
        out['leak'] = st['leak']
    return out


def thrust_alloc_nn_population(tau, nets, envs_per_net=64, out=None, raw=False, **constants):
    """thrust_alloc_nn with K networks of one shape (dpenv_thrust_alloc_nn_population): env i of tau [3, n] takes network
    (i // envs_per_net) % K.  nets: a list of nets or the stacked dict of deploy.nn_population_stack - stacked tensors on tau's device
    are read in place, anything else is stacked and copied there first; envs_per_net: a multiple of 64; the rest is thrust_alloc_nn's.
    On network k's envs the outputs are thrust_alloc_nn's with network k, bit for bit; deploy.BatchedNNAllocatorPopulation is the host
    statement."""
    from .deploy import nn_allocator_params

    def struct(dev):
        dnet = nn_population_to(nets, dev)
        return nn_population_struct(dnet, nn_allocator_params(dnet, **constants), dev)
    return _nn_alloc_map('thrust_alloc_nn_population', tau, out, raw, struct,
                         lambda st, *io: _lib.load().dpenv_thrust_alloc_nn_population(C.byref(st[0]), st[1], int(envs_per_net), *io))


def nn_net_to(net, device):
    """The net's W and b as contiguous float32 tensors on `device` (tensors already there are kept as they are): dict(W, b[, leak])."""
    torch = _torch()
    Ws, bs = (net['W'], net['b']) if isinstance(net, dict) else net
    mv = lambda t: (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t, np.float32))).to(device=device, dtype=torch.float32).contiguous()
    out = dict(W=[mv(w) for w in Ws], b=[mv(b).reshape(-1) for b in bs])
    if isinstance(net, dict) and 'leak' in net:
        out['leak'] = net['leak']
    return out


def controller_label_nn(env, obs, done=None, z=None, net=None, out=None, raw=False, tau=False, act=True, **constants):
    """The PID + network chain's actions on a block of rows some OTHER flight wrote (dpenv_controller_label_nn), in one launch:
    controller_label with the neural allocation in place of the pseudo-inverse, and on request the PID's clipped wrench per row - the
    value the allocator is handed, which the closed loop never writes.  obs [T, n, 9] float32 or bfloat16, done [T, n] uint8 or None,
    z [3, n] float32 or None = 0 as controller_label takes them.  Per row: the PID lines of env.set_dp_controller (row i of the table
    while one is in force) on obs[t] with z advanced first, the network on that wrench, z zeroed behind a done row.  net: a dict with
    'W' and 'b' as thrust_alloc_nn takes it (tensors on the env's device are read in place, anything else is copied there first), with
    constants on top of deploy.nn_allocator_defaults; None = the network env.set_nn_allocator has in force (an error if none is set;
    constants are then an error too).  With an explicit net the env's allocation stage does not matter: an env with a controller table
    or a QP set labels with a network.  Returns (act [T, n, 7], z [3, n]), then raw [T, n, 6] (the network's six outputs) with raw=True,
    then tau [T, n, 3] with tau=True.  act=False with tau=True is the wrench-only scan: no network is needed or looked at, act is
    returned as None.  out supplies the buffers in the order of the return value (z may be the input tensor itself).  Nothing of the
    env changes.  For float32 rows of controller_rollout with a network set and auto-reset on the labels (net=None) are that launch's
    act rows bit for bit; on any block act and raw are thrust_alloc_nn on tau, row by row, bit for bit.  deploy.label_rows_nn is the
    host statement."""
    torch = _torch()
    n = env.n_envs
    dev, f32 = env.device, torch.float32
    if not act and not tau:
        raise ValueError('controller_label_nn: act=False and tau=False leave nothing to compute')
    if raw and not act:
        raise ValueError('controller_label_nn: raw goes with act')
    if not act and (net is not None or constants):
        raise ValueError('controller_label_nn: the wrench-only scan (act=False) takes no net and no constants')
    if net is None and constants:
        raise ValueError('controller_label_nn: constants go with net (net=None labels with the network and constants the env has in force)')
    T, _ = _label_front('controller_label_nn', env, obs, done, z)
    want = [('act', (T, n, 7), bool(act)), ('z', (3, n), True), ('raw', (T, n, 6), bool(raw)), ('tau', (T, n, 3), bool(tau))]
    names = [w[0] for w in want if w[2] or w[0] == 'act']
    if out is not None and len(out) != len(names):
        raise ValueError('controller_label_nn: out is (%s)' % ', '.join(names))
    buf = dict(zip(names, out)) if out is not None else {}
    for name, shape, on in want:
        if not on:
            if buf.get(name) is not None:
                raise ValueError('controller_label_nn: out has a buffer for %s, which is not asked for' % name)
            buf[name] = None
            continue
        if buf.get(name) is None:
            buf[name] = torch.empty(shape, dtype=f32, device=dev)
        env._chk(buf[name], shape, f32, "out's %s" % name)
    a, keep = None, None
    if net is not None:
        from .deploy import nn_allocator_params
        a, keep = nn_allocator_struct(nn_net_to(net, dev), nn_allocator_params(net, **constants), dev)
    io = _label_io(_lib.ControllerLabelNnIO(), T, obs, done, z, buf['z'], buf['act'])
    io.raw = buf['raw'].data_ptr() if raw else None
    io.tau_out = buf['tau'].data_ptr() if tau else None
    io.a = C.pointer(a) if a is not None else None
    _lib.check(env.lib.dpenv_controller_label_nn(env._h, C.byref(io), env._stream()), env._h)
    del keep
    return tuple(buf[k] for k in names)


def thrust_alloc_nn(tau, net, out=None, raw=False, **constants):
    """The neural thrust allocation on the device (dpenv_thrust_alloc_nn), one lane per env: tau float32 [3, n] = Fx, Fy, Mz -> the final
    variant's continuous-angle action [n, 7] and, with raw=True, the network's six outputs [n, 6] as a second value.  net: a dict with
    'W' and 'b' (W[l] [in][out]; inputs 3 or 9, 2..5 dense layers, equal hidden widths <= 96, 6 outputs) - tensors on tau's device are
    read in place, anything else is copied there first; constants: entries of deploy.nn_allocator_defaults to override (leak,
    azimuth_mode, ...).  out = the action buffer, or (action, raw) with raw=True.  An env whose tau or whose network output is not finite
    gets the rest action.  Handle-free and stateless; deploy.BatchedNNAllocator is the host statement."""
    from .deploy import nn_allocator_params
    return _nn_alloc_map('thrust_alloc_nn', tau, out, raw,
                         lambda dev: nn_allocator_struct(nn_net_to(net, dev), nn_allocator_params(net, **constants), dev),
                         lambda st, *io: _lib.load().dpenv_thrust_alloc_nn(C.byref(st[0]), *io))
