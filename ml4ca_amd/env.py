"""Gym-style host mirror of the reference environment over libdpenv.so.

Mirrors the reference's environment interface (paths relative to the reference root,
ENV = src/rl/windows_workspace/specific/customEnv.py):

  * ``BatchedRevoltEnv``  - N environments stepped by one HIP kernel launch; ``reset()`` / ``step()``
    take and return ROCm torch tensors.  This is what a vectorised PPO rollout consumes.
  * ``Revolt`` / ``RevoltSimple`` / ``RevoltLimited`` / ``RevoltFinal`` - single-env adapters with
    the reference constructors' signatures (ENV:22-32,331,355,377), NumPy in / NumPy out, and the
    attribute set the reference's PPO loop and evaluation harness read (ppo.py:202-206,
    train.py:70-73, test_policy.py:114-178) so that a Spinning-Up style loop runs unchanged.
    ``digitwin`` is accepted and ignored: the py4j/Cybersea bridge (digitwin.py) is replaced by
    the kernel's own plant.

PyTorch is plumbing here (device memory, streams); all env arithmetic runs in libdpenv.so.
"""
import ctypes as C
import math
import weakref

import numpy as np

from . import _lib
from ._lib import _torch
from .deploy import REFERENCE_FILTER_OMEGA, REFERENCE_FILTER_ZETA
from . import reset_samplers as simtools

_VARIANTS = {'full': _lib.FULL, 'simple': _lib.SIMPLE, 'limited': _lib.LIMITED, 'final': _lib.FINAL}
_NAMES = {'full': 'full', 'simple': 'revoltsimple', 'limited': 'revoltlimited', 'final': 'revoltfinal'}   # ENV:37,335,360,385


def variant_constants(variant, cont_ang=False):
    """Per-variant constants exactly as the reference constructors leave them (ENV:55-65,337-349,361-371,386-399)."""
    pi = math.pi
    if variant == 'full':
        return dict(num_actions=6, real_action_bounds=[100] * 3 + [pi] * 3,
                    real_ss_bounds=[8.0, 8.0, pi / 2, 1.4, 0.30, 0.52],
                    default_actions={0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
                    valid_action_indices=[0, 1, 2, 3, 4, 5],
                    act_2_act_map={0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5},
                    act_2_act_map_inv={0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5})
    if variant == 'simple':
        return dict(num_actions=3, real_action_bounds=[100] * 3,
                    real_ss_bounds=[8.0, 8.0, pi / 2, 1.75, 0.30, 0.51],
                    default_actions={0: 0, 1: 0, 2: 0, 3: pi / 2, 4: -3 * pi / 4, 5: 3 * pi / 4},
                    valid_action_indices=[0, 1, 2],
                    act_2_act_map={0: 0, 1: 1, 2: 2}, act_2_act_map_inv={0: 0, 1: 1, 2: 2})
    if variant in ('limited', 'final'):
        ab = pi / 2 if variant == 'limited' else pi
        return dict(num_actions=7 if (variant == 'final' and cont_ang) else 5,
                    real_action_bounds=[100] * 3 + [ab] * 2,
                    real_ss_bounds=[8.0, 8.0, 45 * pi / 180, 1.4, 0.30, 0.52],
                    default_actions={0: 0, 1: 0, 2: 0, 3: pi / 2, 4: 0, 5: 0},
                    valid_action_indices=[0, 1, 2, 4, 5],
                    act_2_act_map={0: 0, 1: 1, 2: 2, 4: 3, 5: 4},
                    act_2_act_map_inv={0: 0, 1: 1, 2: 2, 3: 4, 4: 5})
    raise ValueError('unknown variant %r' % (variant,))


class Box(object):
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency): what ppo.py:202-206 reads."""

    def __init__(self, low, high, dtype=np.float64):
        self.low, self.high, self.shape, self.dtype = low, high, low.shape, dtype

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)


_OUT_NAMES = {}                          # 'out[%r]' % key, formatted once per key: the block checks run on every launch


class BatchedRevoltEnv(object):
    """N independent ReVolt DP environments on one MI355X (one wavefront lane per environment).

    step()/reset() semantics per environment are Revolt.step / Revolt.reset (ENV:92-194).
    Differences forced by batching, all explicit:
      * ``done`` is a uint8 tensor of DPENV_DONE_* bits (1 terminal = the reference's ``d``,
        2 time limit = ppo.py:304's ``traj_len == max_ep_len``, 4 non-finite state).
      * with ``auto_reset=True`` finished envs are re-sampled inside the same launch (the batched
        form of ppo.py:305-322) and ``obs`` holds the new episode's first observation; the terminal
        observation is available through ``final_obs``.
      * reset() takes explicit per-env init / ref tensors instead of **init dicts.
    """

    def __init__(self, n_envs, variant='final', extended_state=True, cont_ang=True, device='cuda:0',
                 testing=False, realtime=False, max_ep_len=800, auto_reset=False, terminate=True,
                 wrap_mode='reference', seed=0, env_id_base=0, obs_dtype='float32', current=False,
                 vessel_params=None, layout='aos', reset_fraction=0.8, time_limit=True, hold_plant=False,
                 current_drift=False, current_tau=100.0, current_sigma_v=0.02, current_sigma_beta=5.0 * math.pi / 180.0,
                 n_steps=None, reset_acts=False, step_one_wave=False, per_env_lds=False):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError('BatchedRevoltEnv needs a ROCm device: the env.step path is a HIP kernel and has no CPU fallback')
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.variant = variant
        k = variant_constants(variant, cont_ang)
        self.name = _NAMES[variant]
        self.extended_state = bool(extended_state)
        self.cont_ang = bool(cont_ang) and variant == 'final'
        self.testing = bool(testing)
        self.reset_actions = bool(reset_acts)                        # ENV:30,179-188
        self.n_envs = int(n_envs)
        self.num_actions = k['num_actions']
        self.num_states = 9 if extended_state else 6                 # ENV:44
        self.real_action_bounds = k['real_action_bounds']
        self.real_ss_bounds = k['real_ss_bounds']
        self.default_actions = k['default_actions']
        self.valid_action_indices = k['valid_action_indices']
        self.act_2_act_map = k['act_2_act_map']
        self.act_2_act_map_inv = k['act_2_act_map_inv']
        self.n_steps = 1 if (testing and realtime) else 20           # ENV:79-80
        if n_steps is not None:                                      # any other agent rate: n_steps plant sub-steps of 10 ms
            self.n_steps = int(n_steps)
        self.dt = 0.01 * self.n_steps                                # ENV:81
        self.max_ep_len = int(max_ep_len * 10.0 / self.n_steps)      # ENV:83
        self.vel_rew_coeffs = [0.5, 0.5, 1.0]                        # ENV:78
        self.covar = np.array([[1.0, 0.0], [0.0, 25.0]])             # ENV:86-87
        self.observation_space = Box(-np.ones(self.num_states), np.ones(self.num_states))   # ENV:55-64
        self.action_space = Box(-np.ones(self.num_actions), np.ones(self.num_actions))

        cfg = _lib.default_config()
        cfg.n_envs = self.n_envs
        cfg.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg.variant = _VARIANTS[variant]
        cfg.extended_state = int(self.extended_state)
        cfg.cont_ang = int(self.cont_ang)
        cfg.n_substeps = self.n_steps
        cfg.substep_dt = 0.01
        cfg.wrap_mode = {'reference': _lib.WRAP_REFERENCE, 'radians': _lib.WRAP_RADIANS}[wrap_mode]
        cfg.terminate = int(bool(terminate))
        cfg.max_ep_len = self.max_ep_len if time_limit else 0
        cfg.auto_reset = int(bool(auto_reset))
        lay = {'aos': _lib.AOS, 'soa': _lib.SOA}[layout]
        cfg.action_layout = lay
        cfg.obs_layout = lay
        self.obs_torch_dtype = {'float32': torch.float32, 'bfloat16': torch.bfloat16}[str(obs_dtype).replace('torch.', '')]
        cfg.obs_dtype = _lib.BF16 if self.obs_torch_dtype == torch.bfloat16 else _lib.F32
        cfg.current_enabled = int(bool(current))
        cfg.seed = int(seed)
        cfg.env_id_base = int(env_id_base)
        cfg.reset_fraction = float(reset_fraction)
        cfg.hold_plant = int(bool(hold_plant))
        cfg.current_drift = int(bool(current_drift))
        cfg.current_tau = float(current_tau)
        cfg.current_sigma_v = float(current_sigma_v)
        cfg.current_sigma_beta = float(current_sigma_beta)
        cfg.reset_acts = int(self.reset_actions)                     # drawn inside the reset kernels, ENV:179-188
        cfg.step_one_wave = int(bool(step_one_wave))                 # A/B switch: dpenv_step's re-draw on the env wave (dpenv.h)
        cfg.per_env_lds = int(bool(per_env_lds))                     # A/B switch: per-env blocks through an LDS image in dpenv_step (dpenv.h)
        self.cfg = cfg
        self.layout = layout
        self.auto_reset = bool(auto_reset)

        n_classes = 1
        vp = None
        if vessel_params is not None:
            vp_np = np.ascontiguousarray(np.asarray(vessel_params, dtype=np.float32).reshape(-1, _lib.NPARAM))
            n_classes = vp_np.shape[0]
            vp = vp_np.ctypes.data_as(C.POINTER(C.c_float))
        self.n_classes = n_classes
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dpenv_create(C.byref(cfg), vp, n_classes, C.byref(h)))
        self._h = h
        n, od = self.n_envs, self.num_states
        oshape = (n, od) if layout == 'aos' else (od, n)
        self._obs = [torch.empty(oshape, dtype=self.obs_torch_dtype, device=self.device) for _ in range(2)]
        self._flip = 0
        self._f32, self._u8, self._i32 = torch.float32, torch.uint8, torch.int32
        self._rew = torch.empty(n, dtype=torch.float32, device=self.device)
        self._done = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._final_obs = None
        self._io = _lib.StepIO()
        self._io.struct_size = C.sizeof(_lib.StepIO)
        self._io_ref = C.byref(self._io)
        self._ok = {}
        self._dev_index = cfg.device
        self._raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
        self._ashape, self._oshape = tuple(self.action_shape), tuple(self.obs_shape)
        self._n1, self._r3, self._p4 = (n,), (3, n), (4, n)
        self._step_ex = self.lib.dpenv_step_ex
        self.integral_action = None          # dict of the parameters while set_integral_action() has it on
        self.reference_filter = None         # dict of the parameters while set_reference_filter() has it on
        self.dp_controller = None            # dict of the parameters while set_dp_controller() has it on
        self.dp_controller_table = None      # the [32, n] tensor while set_dp_controller_table() has per-env numbers in force
        self.qp_allocator = None             # dict of the parameters while set_qp_allocator() has the QP allocation in the closed loop
        self.nn_allocator = None             # dict of the constants (and 'net') while set_nn_allocator() has the network in the closed loop
        self.qp_allocator_table = None       # the [32, n] tensor while set_qp_allocator_table() has per-env QP numbers in force
        self._qp_table_iterations = 0

    # -- plumbing -----------------------------------------------------------------------------
    # What a Python `for` over step() pays per call besides the launch is this plumbing (bench.py `eager_loop`): the stream handle and
    # the argument checks.  Both are kept cheap: the raw stream of the CURRENT stream context comes from torch's C binding where it
    # has one (a graph capture's side stream included), and a tensor object that passed the checks once is recognised by identity (a
    # weak reference, so a recycled id() cannot alias another tensor) and not checked again - shape, dtype, device and contiguity of a
    # live tensor object do not change short of resize_() / set_().
    def _stream(self):
        raw = self._raw_stream
        if raw is not None:
            return C.c_void_p(raw(self._dev_index))
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _chk(self, t, shape, dtype, what):
        """Argument check of a tensor handed to the C ABI: type, device, dtype, shape, contiguity - ONCE per tensor object (a weak reference keyed by
        id()): a tensor that passed is not looked at again, which is what keeps a Python `for` over step() at the GPU's rate (bench_side.json
        eager_loop: the full check costs ~0.4 us per tensor, four tensors per call, against a 4.9 us kernel).  The price: a tensor that
        is CHANGED IN PLACE between calls - t_(), transpose_(), resize_(), as_strided_(), set_(), `.data = ...` - is not re-checked, and the kernels
        would then read or write through a pointer whose extent no longer matches.  Do not reshape tensors you pass to reset / step / rollout in
        place; make a new tensor (a new object is checked)."""
        if t is None:
            return None
        ok = self._ok.get(id(t))
        if ok is not None and ok[0]() is t and ok[1] == shape and ok[2] is dtype:
            return t
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dtype
                and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise ValueError('%s must be a contiguous %s tensor of shape %s on %s (got %s)' % (
                what, dtype, tuple(shape), self.device,
                (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)))
        if len(self._ok) > 512:
            self._ok.clear()
        self._ok[id(t)] = (weakref.ref(t), tuple(shape), dtype)
        return t

    @staticmethod
    def _ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _get(self, fn, *specs, or_none=False):
        """A getter of the C ABI: one new tensor per (shape, dtype), fn(handle, their pointers..., stream), the tensors (one: itself).
        or_none: a refusal returns None instead of raising."""
        torch = _torch()
        ts = [torch.empty(shape, dtype=dtype, device=self.device) for shape, dtype in specs]
        rc = fn(self._h, *[self._ptr(t) for t in ts], self._stream())
        if or_none and rc != _lib.OK:
            return None
        _lib.check(rc, self._h)
        return ts[0] if len(ts) == 1 else tuple(ts)

    def _set(self, fn, *args):
        """A setter of the C ABI: _chk of every (tensor, shape, dtype, what) - None passes, and reaches the library as NULL - then
        fn(handle, their pointers..., stream)."""
        _lib.check(fn(self._h, *[self._ptr(self._chk(*a)) for a in args], self._stream()), self._h)

    def _blocks(self, spec, out=None, fill=False):
        """The blocks a launch writes, spec = (key, shape, dtype) each: out None makes them (a dict by key); else out[key] - a dict's or
        a tuple's - is checked (_chk, named out[key]), a block the dict lacks being made first if fill."""
        torch = _torch()
        if out is None:
            return {key: torch.empty(shape, dtype=dtype, device=self.device) for key, shape, dtype in spec}
        for key, shape, dtype in spec:
            if fill and out.get(key) is None:
                out[key] = torch.empty(shape, dtype=dtype, device=self.device)
            self._chk(out[key], shape, dtype, _OUT_NAMES.get(key) or _OUT_NAMES.setdefault(key, 'out[%r]' % (key,)))
        return out

    def _schedule(self, io, switch_steps, refs):
        """The setpoint schedule of a rollout launch into its io struct (n_switch, switch_step[], refs): refs[k] float32 [3, n] is the
        new_ref of step switch_steps[k]."""
        k = len(switch_steps)
        if k > 8:
            raise ValueError('at most 8 setpoint switches per rollout launch')
        if k:
            self._chk(refs, (k, 3, self.n_envs), self._f32, 'refs')
        io.n_switch = k
        for j, st in enumerate(switch_steps):
            io.switch_step[j] = int(st)
        io.refs = refs.data_ptr() if k else None

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.dpenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def action_shape(self):
        return (self.n_envs, self.num_actions) if self.layout == 'aos' else (self.num_actions, self.n_envs)

    @property
    def obs_shape(self):
        return (self.n_envs, self.num_states) if self.layout == 'aos' else (self.num_states, self.n_envs)

    # -- Gym-style API ------------------------------------------------------------------------
    def reset(self, mask=None, init=None, new_ref=None, fraction=None, out=None):
        """Revolt.reset (ENV:135-194) for the envs in ``mask`` (uint8 [n], None = all).

        init: float32 [6, n] rows N, E, psi, u, v, r (the reference's **init, ENV:141,152); None draws the
        training sample (ENV:143-145).  new_ref: float32 [3, n] setpoints (ENV:155-156); fraction: ENV:135.
        Returns the observation of every env."""
        torch = _torch()
        n = self.n_envs
        if fraction is not None:
            _lib.check(self.lib.dpenv_set_reset_fraction(self._h, float(fraction)), self._h)
        mask = self._chk(mask, (n,), torch.uint8, 'mask')
        init = self._chk(init, (6, n), torch.float32, 'init')
        new_ref = self._chk(new_ref, (3, n), torch.float32, 'new_ref')
        obs = out if out is not None else self._next_obs()
        self._chk(obs, self.obs_shape, self.obs_torch_dtype, 'out')
        _lib.check(self.lib.dpenv_reset(self._h, self._ptr(mask), self._ptr(init), self._ptr(new_ref), self._ptr(obs),
                                        self._stream()), self._h)
        return obs

    def _next_obs(self):
        self._flip ^= 1
        return self._obs[self._flip]

    def step(self, action, new_ref=None, out=None, reward_parts=None, final_obs=None):
        """Revolt.step (ENV:92-133) for all envs: returns (obs, reward, done_bits, info).

        action: float32 [n, act_dim] (or [act_dim, n] with layout='soa'); new_ref: float32 [3, n], visible from
        the NEXT observation (ENV:131).  out: optional (obs, reward, done) tensors to write into (e.g. rows of a
        [T, n, .] rollout buffer); otherwise internal buffers are reused (obs is double-buffered).
        Tensors are checked (device, dtype, shape, contiguity) the first time the OBJECT is seen, not on every call: do not change the shape or
        strides of a tensor in place (t_(), resize_(), set_() ...) between calls - pass a new tensor instead (_chk)."""
        f32, chk = self._f32, self._chk
        chk(action, self._ashape, f32, 'action')
        if out is None:
            obs, rew, done = self._next_obs(), self._rew, self._done
        else:
            obs, rew, done = out
            chk(obs, self._oshape, self.obs_torch_dtype, 'out[0]')
            chk(rew, self._n1, f32, 'out[1]')
            chk(done, self._n1, self._u8, 'out[2]')
        io = self._io
        io.action = action.data_ptr()
        io.new_ref = chk(new_ref, self._r3, f32, 'new_ref').data_ptr() if new_ref is not None else None
        io.obs = obs.data_ptr()
        io.reward = rew.data_ptr()
        io.done = done.data_ptr()
        io.reward_parts = chk(reward_parts, self._p4, f32, 'reward_parts').data_ptr() if reward_parts is not None else None
        io.final_obs = chk(final_obs, self._oshape, self.obs_torch_dtype, 'final_obs').data_ptr() if final_obs is not None else None
        rc = self._step_ex(self._h, self._io_ref, self._stream())
        if rc:
            self._refuse_open_loop('step')
            _lib.check(rc, self._h)
        return obs, rew, done, {'None': 0}

    def _refuse_open_loop(self, what):
        if self.integral_action is not None:
            raise ValueError('%s(): the integral action is on (set_integral_action) and this launch\'s observations would lack I; fly the closed '
                             'loop (policy.policy_rollout), compose step() with deploy.BatchedBodyFrameIntegrator after set_integral_action(None), '
                             'or turn it off' % what)
        if self.reference_filter is not None:
            raise ValueError('%s(): the reference filter is on (set_reference_filter) and would not see this launch; fly the closed loop '
                             '(policy.policy_rollout), compose step() with deploy.BatchedReferenceFilter (its position as new_ref) after '
                             'set_reference_filter(None), or turn it off' % what)

    def rollout(self, actions, switch_steps=(), refs=None, out=None):
        """T env steps in one launch (dpenv_rollout): exactly T successive step() calls with actions[t], passing
        refs[k] as new_ref at step switch_steps[k] (setpoint sequences, test_policy.py:127,148-153), but with the
        state kept in registers between steps.  actions: float32 [T, n, act_dim] (or [T, act_dim, n] for 'soa').
        Returns (obs [T, n, obs_dim], reward [T, n], done_bits [T, n]); obs[t] is what step t returned."""
        torch = _torch()
        self._refuse_open_loop('rollout')
        T = int(actions.shape[0])
        n = self.n_envs
        self._chk(actions, (T,) + self.action_shape, torch.float32, 'actions')
        io = _lib.RolloutIO()
        io.struct_size = C.sizeof(_lib.RolloutIO)
        self._schedule(io, switch_steps, refs)
        blk = self._blocks(((0, (T,) + self.obs_shape, self.obs_torch_dtype), (1, (T, n), torch.float32), (2, (T, n), torch.uint8)), out)
        obs, rew, done = blk[0], blk[1], blk[2]
        io.T = T
        io.actions = actions.data_ptr()
        io.obs = obs.data_ptr()
        io.reward = rew.data_ptr()
        io.done = done.data_ptr()
        _lib.check(self.lib.dpenv_rollout(self._h, C.byref(io), self._stream()), self._h)
        return obs, rew, done

    # -- state access (parity tests, checkpoints) ----------------------------------------------
    def get_state(self):
        return self._get(self.lib.dpenv_get_state, ((_lib.NSTATE, self.n_envs), self._f32), ((2, self.n_envs), self._i32))

    def set_state(self, state=None, counters=None):
        self._set(self.lib.dpenv_set_state, (state, (_lib.NSTATE, self.n_envs), self._f32, 'state'),
                  (counters, (2, self.n_envs), self._i32, 'counters'))

    # -- the deployed controller's integral action (dpenv.h dpenv_set_integral_action) ----------------------------------------------
    @property
    def control_period(self):
        """The env's control period n_steps * 0.01 s in float32, as the library computes it (the integral action's default step_s)."""
        return float(np.float32(self.cfg.substep_dt) * np.float32(self.cfg.n_substeps))

    def set_integral_action(self, gain=(0.05, 0.05, 0.05), bound=(0.5, 1.0, math.pi / 32), box=(5.0, 5.0, 140.0 * math.pi / 180.0),
                            dwell_s=5.0, step_s=None):
        """The RL node's body-frame integral action (rl_allocator.py:252-273) in the closed-loop launches: the policy input becomes
        o[0:3] = e + I (dpenv.h has the law).  Defaults are the node's.  step_s None = the control period.  off=True (or
        turns it off.  Turning it on zeroes the integrator of every env.  While it is on, step() and rollout()
        raise ValueError."""
        if gain is None:
            _lib.check(self.lib.dpenv_set_integral_action(self._h, None, self._stream()), self._h)
            self.integral_action = None
            return
        ia = _lib.IntegralAction()
        ia.struct_size = C.sizeof(_lib.IntegralAction)
        for j in range(3):
            ia.gain[j], ia.bound[j], ia.box[j] = float(gain[j]), float(bound[j]), float(box[j])
        ia.dwell_s = float(dwell_s)
        ia.step_s = 0.0 if step_s is None else float(step_s)
        if step_s is not None and not step_s > 0:
            raise ValueError('step_s must be > 0 (None = the control period)')
        _lib.check(self.lib.dpenv_set_integral_action(self._h, C.byref(ia), self._stream()), self._h)
        self.integral_action = dict(gain=tuple(ia.gain), bound=tuple(ia.bound), box=tuple(ia.box), dwell_s=ia.dwell_s,
                                    step_s=self.control_period if step_s is None else float(np.float32(step_s)))

    def get_integral_state(self):
        """(I float32 [3, n], count int32 [n]): the integrator and the control steps since the last (re)arrival.  Checkpoint with
        get_state() / get_rng_counters()."""
        return self._get(self.lib.dpenv_get_integral_state, (self._r3, self._f32), (self._n1, self._i32))

    def set_integral_state(self, I=None, count=None):
        self._set(self.lib.dpenv_set_integral_state, (I, self._r3, self._f32, 'I'), (count, self._n1, self._i32, 'count'))

    # -- the deployed controller's setpoint reference filter (dpenv.h dpenv_set_reference_filter) ------------------------------------
    def set_reference_filter(self, omega=REFERENCE_FILTER_OMEGA, zeta=REFERENCE_FILTER_ZETA):
        """The setpoint reference filter the RL node took its reference from (include/dpenv.h has the law) in the closed-loop launches:
        a setpoint switch sets the filter's target, and every step's new_ref is the filter's position.  omega [rad/s] / zeta: per axis
        (N, E, psi); the defaults are the recorded fit (deploy.REFERENCE_FILTER_OMEGA / _ZETA).  omega=None turns it off.  Turning it on
        puts every env's filter at rest on its reference.  While it is on, step() and rollout() raise ValueError."""
        if omega is None:
            _lib.check(self.lib.dpenv_set_reference_filter(self._h, None, self._stream()), self._h)
            self.reference_filter = None
            return
        rf = _lib.ReferenceFilter()
        rf.struct_size = C.sizeof(_lib.ReferenceFilter)
        for j in range(3):
            rf.omega[j], rf.zeta[j] = float(omega[j]), float(zeta[j])
        _lib.check(self.lib.dpenv_set_reference_filter(self._h, C.byref(rf), self._stream()), self._h)
        self.reference_filter = dict(omega=tuple(rf.omega), zeta=tuple(rf.zeta), dt=self.control_period)

    def get_reference_filter_state(self):
        """(x float32 [9, n], r float32 [3, n]): row 3 k + j of x is (pos, vel, acc)[k] of axis (N, E, psi)[j]; r the targets.  Checkpoint
        with get_state() / get_rng_counters()."""
        return self._get(self.lib.dpenv_get_reference_filter_state, ((9, self.n_envs), self._f32), (self._r3, self._f32))

    def set_reference_filter_state(self, x=None, r=None):
        self._set(self.lib.dpenv_set_reference_filter_state, (x, (9, self.n_envs), self._f32, 'x'), (r, self._r3, self._f32, 'r'))

    # -- the classical baseline: PID + pseudo-inverse allocation in the closed loop (dpenv.h dpenv_set_dp_controller) ------------------
    def set_dp_controller(self, params=None, off=False):
        """The baseline DP controller for policy.controller_rollout (include/dpenv.h has the law): params is the dict of
        deploy.dp_controller_defaults (None = the defaults of the default hull); off=True turns it off.  Turning it on zeroes the error
        integral z of every env.  step(), rollout() and policy_rollout() keep working while it is on."""
        if off:
            _lib.check(self.lib.dpenv_set_dp_controller(self._h, None, self._stream()), self._h)
            self.dp_controller = self.dp_controller_table = self.qp_allocator = self.qp_allocator_table = None
            self.nn_allocator = None
            return
        p, c = _dp_controller_struct(params)
        _lib.check(self.lib.dpenv_set_dp_controller(self._h, C.byref(c), self._stream()), self._h)
        self.dp_controller = dict(p)
        self.dp_controller_table = None      # the scalar law again: the library dropped a table in force
        self.qp_allocator = self.qp_allocator_table = None   # ... and a QP allocator, scalar or per-env
        self.nn_allocator = None                             # ... and a neural allocator

    def set_dp_controller_table(self, table, check=True):
        """Per-env numbers for the baseline (dpenv_set_dp_controller_table): table is a float32 tensor [32, n] on the env's device in
        the slot order of include/dpenv.h (deploy.dp_controller_table builds it), and controller_rollout then flies row i on env i; None
        returns to the numbers of set_dp_controller, which has to be on.  The library computes every env's allocation matrix from the row's
        lever arms and weights, and packs a row it refuses as the zero controller.  check=True passes a mask, reads it back and, if any row
        was refused, removes the table again and raises ValueError naming the first refused envs.  check=False reads nothing back: the
        form to record into a graph (a replay packs the tensor's contents of that moment).  z is left alone."""
        torch = _torch()
        if table is None:
            _lib.check(self.lib.dpenv_set_dp_controller_table(self._h, None, None, self._stream()), self._h)
            self.dp_controller_table = None
            return
        self._chk(table, (32, self.n_envs), torch.float32, 'table')
        mask = torch.empty(self.n_envs, dtype=torch.uint8, device=self.device) if check else None
        _lib.check(self.lib.dpenv_set_dp_controller_table(self._h, self._ptr(table), self._ptr(mask), self._stream()), self._h)
        self.dp_controller_table = table
        if check and bool(mask.any()):
            bad = torch.nonzero(mask).flatten()
            self.set_dp_controller_table(None)
            raise ValueError('set_dp_controller_table: %d row(s) refused (envs %s%s): non-finite gains, a negative bound, kf or a weight '
                             '<= 0, or lever arms with a singular allocation - the scalar law stays in force'
                             % (bad.numel(), bad[:8].tolist(), ', ...' if bad.numel() > 8 else ''))

    def get_dp_controller_state(self):
        """z float32 [3, n]: the baseline's error integral.  Checkpoint with get_state()."""
        return self._get(self.lib.dpenv_get_dp_controller_state, (self._r3, self._f32))

    def set_dp_controller_state(self, z):
        self._set(self.lib.dpenv_set_dp_controller_state, (z, self._r3, self._f32, 'z'))

    def set_nn_allocator(self, net=None, off=False, **constants):
        """The neural thrust allocation as the allocation stage of policy.controller_rollout (dpenv_set_nn_allocator; include/dpenv.h has
        the law): the baseline's PID forms the wrench, the network allocates it in place of the pseudo-inverse.  net: a dict with 'W' and
        'b' (W[l] [in][out]; inputs 3 or 9, 2..5 dense layers, equal hidden widths <= 96, 6 outputs; train.fit_nn_allocator returns one).
        Tensors on the env's device are handed over as device pointers - one packing launch on the current stream, capturable in a
        graph, which then re-packs the tensors' contents at every replay; anything else goes through a host copy and a synchronisation.
        constants: entries of deploy.nn_allocator_defaults to override (leak, azimuth_mode, azimuth, ...); a net that carries 'leak'
        supplies it.  off=True (or net=None) returns to the pseudo-inverse.  Needs set_dp_controller on (which drops it again), no per-env
        controller table and no QP allocator; it flies on every hull the baseline flies, per-env and randomised hulls included."""
        if off or net is None:
            _lib.check(self.lib.dpenv_set_nn_allocator(self._h, None, self._stream()), self._h)
            self.nn_allocator = None
            return
        from .deploy import nn_allocator_params
        from .policy import nn_allocator_struct
        p = nn_allocator_params(net, **constants)
        a, keep = nn_allocator_struct(net, p, self.device)
        with _torch().cuda.device(self.device):
            _lib.check(self.lib.dpenv_set_nn_allocator(self._h, C.byref(a), self._stream()), self._h)
        del keep
        self.nn_allocator = dict(p, net=net)

    def set_nn_allocator_population(self, nets=None, envs_per_net=64, off=False, **constants):
        """K neural allocators of one shape in one flight (dpenv_set_nn_allocator_population): env i flies network
        ((env_id_base + i) // envs_per_net) % K behind the baseline's PID, everything else as set_nn_allocator.  nets: a list of K net
        dicts, or the stacked dict of deploy.nn_population_stack (W[l] [K, in, out], b[l] [K, out]); stacked tensors on the env's device
        are handed over as device pointers - one packing launch, capturable once an image of that shape and K exists - anything else
        goes through a host copy.  envs_per_net: a multiple of 64, as is the env's env_id_base (a wave flies one network).  constants:
        shared by the K networks.  off=True (or nets=None) returns to the pseudo-inverse; set_nn_allocator replaces the population by
        one network.  While set, self.nn_allocator carries 'net' (the stacked dict), 'K' and 'envs_per_net'."""
        if off or nets is None:
            _lib.check(self.lib.dpenv_set_nn_allocator_population(self._h, None, 0, 0, self._stream()), self._h)
            self.nn_allocator = None
            return
        from .deploy import nn_allocator_params, nn_population_stack
        from .policy import nn_population_struct
        st = nn_population_stack(nets)
        p = nn_allocator_params(st, **constants)
        a, K, keep = nn_population_struct(st, p, self.device)
        with _torch().cuda.device(self.device):
            _lib.check(self.lib.dpenv_set_nn_allocator_population(self._h, C.byref(a), K, int(envs_per_net), self._stream()), self._h)
        del keep
        self.nn_allocator = dict(p, net=st, K=K, envs_per_net=int(envs_per_net))

    def set_qp_allocator(self, params=None, off=False):
        """The rate-limited QP thrust allocation as the allocation stage of policy.controller_rollout (dpenv_set_qp_allocator; include/dpenv.h
        has the law): the baseline's PID forms the wrench, the QP allocates it in place of the pseudo-inverse.  params is the dict of
        deploy.qp_allocator_defaults (None = the defaults of the DEFAULT hull, whatever hull the env flies: for another hull, the thrust-loss
        preset included, pass deploy.qp_allocator_defaults(its parameter vector) - its lever arms and thrust constants); off=True returns to
        the pseudo-inverse.  Needs
        set_dp_controller on (set_dp_controller drops it again), the shared hull or the thrust-loss preset and no per-env controller table.
        Turning it on puts every env's thrusters at rest; resets do the same for the envs they re-draw."""
        if off:
            _lib.check(self.lib.dpenv_set_qp_allocator(self._h, None, self._stream()), self._h)
            self.qp_allocator = self.qp_allocator_table = None
            return
        from .deploy import qp_allocator_defaults
        from .policy import qp_allocator_struct
        p = qp_allocator_defaults() if params is None else params
        q = qp_allocator_struct(p)
        _lib.check(self.lib.dpenv_set_qp_allocator(self._h, C.byref(q), self._stream()), self._h)
        self.qp_allocator = dict(p)
        self.qp_allocator_table = None       # the scalar numbers replace a table in force

    def set_qp_allocator_table(self, table, iterations=16, check=True):
        """One QP allocator per env (dpenv_set_qp_allocator_table): table is a float32 tensor [32, n] on the env's device in the slot order
        of include/dpenv.h (deploy.qp_allocator_table builds it), and controller_rollout then allocates env i's wrench with row i;
        iterations (1..32) is one count for every env.  Needs what set_qp_allocator needs, and like it puts every env's thrusters at rest.
        None returns to the numbers of set_qp_allocator - or to the pseudo-inverse if none were set - and leaves z and the thruster state
        alone.  The library packs a row it refuses as the rest allocator (zero thrust, azimuths held).  check=True passes a mask, reads it
        back and, if any row was refused, puts the previous allocator back in force - a previous table is packed again, the thruster
        state restored - and raises ValueError naming the first refused envs.  check=False reads nothing back: the form to record into a
        graph (a replay packs the tensor's contents of that moment)."""
        torch = _torch()
        if table is None:
            _lib.check(self.lib.dpenv_set_qp_allocator_table(self._h, None, 0, None, self._stream()), self._h)
            self.qp_allocator_table = None
            return
        self._chk(table, (32, self.n_envs), torch.float32, 'table')
        qp_was_on = self.qp_allocator is not None or self.qp_allocator_table is not None
        mask = torch.empty(self.n_envs, dtype=torch.uint8, device=self.device) if check else None
        x = self.get_qp_allocator_state() if check and qp_was_on else None
        _lib.check(self.lib.dpenv_set_qp_allocator_table(self._h, self._ptr(table), int(iterations), self._ptr(mask), self._stream()), self._h)
        prev, prev_iters = self.qp_allocator_table, self._qp_table_iterations
        self.qp_allocator_table, self._qp_table_iterations = table, int(iterations)
        if check and bool(mask.any()):
            bad = torch.nonzero(mask).flatten()
            if prev is not None:
                self.set_qp_allocator_table(prev, prev_iters, check=False)
            else:
                self.set_qp_allocator_table(None)
            if x is not None:
                self.set_qp_allocator_state(x)
            raise ValueError('set_qp_allocator_table: %d row(s) refused (envs %s%s): a number that is not finite, a negative weight, bound '
                             'or rate, w_dalpha or w_dforce <= 0, kf or kr <= 0 - the previous allocator stays in force'
                             % (bad.numel(), bad[:8].tolist(), ', ...' if bad.numel() > 8 else ''))

    def get_qp_allocator_state(self):
        """float32 [5, n]: the QP allocator's thruster state F_bow, F_port, F_star, a_port, a_star.  Checkpoint with get_dp_controller_state()."""
        return self._get(self.lib.dpenv_get_qp_allocator_state, ((5, self.n_envs), self._f32))

    def set_qp_allocator_state(self, x):
        self._set(self.lib.dpenv_set_qp_allocator_state, (x, (5, self.n_envs), self._f32, 'x'))

    def get_rng_counters(self):
        """(noise_ctr, drift_ctr): int32 [n] draws made so far of the in-kernel exploration noise and of the current drift (uint32
        bits).  With get_state() and get_current() a complete checkpoint: restoring all of them reproduces sampled rollouts."""
        return self._get(self.lib.dpenv_get_rng_counters, (self._n1, self._i32), (self._n1, self._i32))

    def set_rng_counters(self, noise_ctr=None, drift_ctr=None):
        self._set(self.lib.dpenv_set_rng_counters, (noise_ctr, self._n1, self._i32, 'noise_ctr'), (drift_ctr, self._n1, self._i32, 'drift_ctr'))

    def get_obs_thrust(self):
        """float32 [n, 4]: thrust columns of the observation the last closed-loop launch ended with (a mid-episode checkpoint needs
        them: the observation lags the stored thrust command by one step, customEnv.py:196-205,126).  Every call that changes the state
        keeps them: rollouts leave those of the last observation they returned, set_state those of an observation rebuilt from the state
        (previous thrust / 100), a reset those of the envs it re-draws, step() those of the observation it returns while a policy is in
        force.  None only while they are stale: after a step() WITHOUT a policy uploaded, or after a masked reset of a handle whose
        columns were already stale - the next closed-loop launch then starts from the state block alone."""
        return self._get(self.lib.dpenv_get_obs_thrust, ((self.n_envs, 4), self._f32), or_none=True)

    def set_obs_thrust(self, t):
        self._set(self.lib.dpenv_set_obs_thrust, (t, (self.n_envs, 4), self._f32, 'obs_thrust'))

    def set_current(self, vc, beta, present_only=False):
        """Per-env constant current: speed [m/s] and NED direction [rad] (results/.../current_box_test/plot_pos.py:78).  They are
        both the present value and the mean a drifting current reverts to; present_only=True restores only the present values
        (what get_current returned: checkpoints of a drifting current)."""
        self._set(self.lib.dpenv_set_current_present if present_only else self.lib.dpenv_set_current,
                  (vc, self._n1, self._f32, 'vc'), (beta, self._n1, self._f32, 'beta'))

    def get_current(self):
        """Present (vc, beta) of every env; differs from what set_current gave only with current_drift."""
        return self._get(self.lib.dpenv_get_current, (self._n1, self._f32), (self._n1, self._f32))

    def get_current_mean(self):
        """(vc, beta) the drift reverts to: what set_current gave, or what the last randomised reset drew (set_current_randomisation)."""
        return self._get(self.lib.dpenv_get_current_mean, (self._n1, self._f32), (self._n1, self._f32))

    def set_current_randomisation(self, vc_range, beta_range, vc_nominal=None, beta_nominal=None):
        """Per-episode randomisation of the current through the reset path (dpenv_set_current_randomisation): every reset starts its
        episode in V_c = max(0, vc_nominal + vc_range u1), beta_c = beta_nominal + beta_range u2, u ~ U[-1, 1), keyed (seed; global env
        id, episode).  Nominals: float32 [n] device tensors, default the means in force (set_current).  Both ranges 0: off."""
        torch = _torch()
        for t, what in ((vc_nominal, 'vc_nominal'), (beta_nominal, 'beta_nominal')):
            if t is not None:
                self._chk(t, (self.n_envs,), torch.float32, what)
        _lib.check(self.lib.dpenv_set_current_randomisation(self._h, self._ptr(vc_nominal), self._ptr(beta_nominal), float(vc_range),
                                                            float(beta_range), self._stream()), self._h)

    def set_vessel_class(self, class_id):
        torch = _torch()
        self._chk(class_id, (self.n_envs,), torch.int32, 'class_id')
        if int(class_id.min()) < 0 or int(class_id.max()) >= self.n_classes:
            raise ValueError('class ids must be in [0, %d)' % self.n_classes)
        _lib.check(self.lib.dpenv_set_vessel_class(self._h, self._ptr(class_id), self._stream()), self._h)

    def set_vessel_params(self, params, keep_randomisation=False):
        """Per-env hull / thruster parameters (dpenv_set_vessel_params_ex): float32 [NPARAM, n] device tensor, row p = parameter
        _lib.P[...] of every env - the constants the reference hard-codes for its one vessel (qp_allocator.py:51-55,69-70;
        SupervisedTau.py:35-36,69-71), the build-owned plant's mass / damping terms and (rows 26..31) the thrusters' inflow-loss
        coefficients.  A single length-NPARAM vector is given to every env.  None returns to the vessel classes / the single class given
        to the constructor.  Stream-ordered (no read-back; may be recorded into a graph).  keep_randomisation=True installs the table
        while set_vessel_randomisation stays in force: the restore path of a checkpoint (get_state + get_vessel_params) taken mid-episode."""
        torch = _torch()
        if params is not None and not (hasattr(params, 'dim') and params.dim() == 2):
            one = torch.as_tensor(np.asarray(params.cpu() if hasattr(params, 'cpu') else params, np.float32).reshape(_lib.NPARAM), device=self.device)
            params = one[:, None].expand(_lib.NPARAM, self.n_envs).contiguous()
        self._chk(params, (_lib.NPARAM, self.n_envs), torch.float32, 'params')
        flags = _lib.VESSEL_KEEP_RANDOMISATION if keep_randomisation else 0
        _lib.check(self.lib.dpenv_set_vessel_params_ex(self._h, self._ptr(params), flags, self._stream()), self._h)

    def get_vessel_params(self):
        """float32 [NPARAM, n]: the per-env parameter vectors in force (set explicitly, or drawn by the randomisation)."""
        return self._get(self.lib.dpenv_get_vessel_params, ((_lib.NPARAM, self.n_envs), self._f32))

    def set_vessel_randomisation(self, rel_range, nominal=None):
        """Domain randomisation through the reset path (dpenv_set_vessel_randomisation): every reset starts its episode on a hull with
        parameter p = nominal[p] * (1 + rel_range[p] * u), u ~ U[-1, 1), keyed (seed; global env id, episode).  rel_range: a float (the
        same relative half-range for every parameter), a length-NPARAM sequence, or None to stop re-drawing; nominal: a parameter
        vector, default class 0."""
        if rel_range is None:
            _lib.check(self.lib.dpenv_set_vessel_randomisation(self._h, None, None, self._stream()), self._h)
            return
        rr = np.zeros(_lib.NPARAM, np.float32)
        if np.isscalar(rel_range):
            rr[:_lib.NPARAM_USED] = float(rel_range)
        else:
            rr[:] = np.asarray(rel_range, np.float32).reshape(_lib.NPARAM)
        nom = None
        if nominal is not None:
            nom_np = np.ascontiguousarray(np.asarray(nominal, np.float32).reshape(_lib.NPARAM))
            nom = nom_np.ctypes.data_as(C.POINTER(C.c_float))
        _lib.check(self.lib.dpenv_set_vessel_randomisation(self._h, nom, rr.ctypes.data_as(C.POINTER(C.c_float)), self._stream()), self._h)

    def render(self):
        pass   # ENV:246-247


def thrust_map(n_pct, alpha, params=None):
    """tau = B(alpha) F(n) on device (SupervisedTau.py:42-83): n_pct, alpha float32 [3, n] in env order
    (bow, port, star); returns float32 [3, n] = Fx, Fy, Mz."""
    torch = _torch()
    lib = _lib.load()
    assert n_pct.shape == alpha.shape and n_pct.shape[0] == 3 and n_pct.is_contiguous() and alpha.is_contiguous()
    assert n_pct.dtype == torch.float32 and alpha.dtype == torch.float32 and n_pct.is_cuda
    tau = torch.empty_like(n_pct)
    p = None
    if params is not None:
        pa = np.ascontiguousarray(params, dtype=np.float32)
        assert pa.shape == (_lib.NPARAM,)
        p = pa.ctypes.data_as(C.POINTER(C.c_float))
    with torch.cuda.device(n_pct.device):
        _lib.check(lib.dpenv_thrust_map(p, _lib._p(n_pct), _lib._p(alpha), _lib._p(tau), n_pct.shape[1], _lib._s(n_pct)))
    return tau


def _dp_controller_struct(params):
    """(params dict, dpenv_dp_controller) for deploy.dp_controller_defaults' dict; None = the defaults of the default hull."""
    from .deploy import dp_controller_defaults
    p = dp_controller_defaults() if params is None else params
    c = _lib.DPController()
    c.struct_size = C.sizeof(_lib.DPController)
    for j in range(3):
        c.kp[j], c.kd[j], c.ki[j] = float(p['kp'][j]), float(p['kd'][j]), float(p['ki'][j])
        c.z_bound[j], c.tau_max[j], c.kf[j] = float(p['z_bound'][j]), float(p['tau_max'][j]), float(p['kf'][j])
    for m in range(5):
        for j in range(3):
            c.G[m][j] = float(p['G'][m][j])
    c.kr_bow, c.f_eps = float(p['kr_bow']), float(p['f_eps'])
    return p, c


def thrust_alloc(tau, params=None):
    """The baseline's stateless allocation on device (dpenv_thrust_alloc): tau float32 [3, n] = Fx, Fy, Mz -> the final variant's
    continuous-angle action float32 [n, 7]; params: the dict of deploy.dp_controller_defaults (None = the default hull's)."""
    torch = _torch()
    lib = _lib.load()
    assert tau.dim() == 2 and tau.shape[0] == 3 and tau.is_contiguous() and tau.dtype == torch.float32 and tau.is_cuda
    _, c = _dp_controller_struct(params)
    act = torch.empty((tau.shape[1], 7), dtype=torch.float32, device=tau.device)
    with torch.cuda.device(tau.device):
        _lib.check(lib.dpenv_thrust_alloc(C.byref(c), _lib._p(tau), _lib._p(act), tau.shape[1], _lib._s(tau)))
    return act


class _ErrorFrameView(object):
    """What test_policy.py:117-121 reads from env.EF (errorFrame.py:15-23), backed by the device state."""

    def __init__(self, env):
        self._env = env

    def _row(self, a, b):
        st, _ = self._env._benv.get_state()
        return [float(x) for x in st[a:b, 0].cpu().numpy()]

    def get_NED_pos(self):
        return self._row(_lib.S['N'], _lib.S['N'] + 3)

    def get_NED_ref(self):
        return self._row(_lib.S['REF_N'], _lib.S['REF_N'] + 3)

    def get_pose(self):
        return [float(x) for x in self._env.state()[:3]]

    def update(self, pos=None, ref=None):
        st, _ = self._env._benv.get_state()
        torch = _torch()
        if pos:
            st[_lib.S['N']:_lib.S['N'] + 3, 0] = torch.tensor(pos, dtype=torch.float32)
        if ref:
            st[_lib.S['REF_N']:_lib.S['REF_N'] + 3, 0] = torch.tensor(ref, dtype=torch.float32)
        self._env._benv.set_state(st.contiguous(), None)


class Revolt(object):
    """Single-environment adapter with the reference's constructor and Gym API (ENV:11-325)."""

    _variant = 'full'

    def __init__(self, digitwin=None, num_actions=None, num_states=6, real_ss_bounds=None, testing=False,
                 realtime=False, max_ep_len=800, extended_state=False, reset_acts=False, cont_ang=False,
                 device='cuda:0', seed=0, wrap_mode='reference'):
        torch = _torch()
        self.dTwin = digitwin   # kept for attribute compatibility; never called
        self._benv = BatchedRevoltEnv(1, variant=self._variant, extended_state=extended_state, cont_ang=cont_ang,
                                      device=device, testing=testing, realtime=realtime, max_ep_len=max_ep_len,
                                      auto_reset=False, terminate=True, wrap_mode=wrap_mode, seed=seed,
                                      time_limit=False)
        b = self._benv
        for k in ('name', 'extended_state', 'cont_ang', 'testing', 'num_actions', 'num_states', 'real_action_bounds',
                  'real_ss_bounds', 'default_actions', 'valid_action_indices', 'act_2_act_map', 'act_2_act_map_inv',
                  'n_steps', 'dt', 'max_ep_len', 'vel_rew_coeffs', 'covar', 'observation_space', 'action_space'):
            setattr(self, k, getattr(b, k))
        self.reset_actions = reset_acts
        self.covar_inv = np.linalg.inv(self.covar)
        self.EF = _ErrorFrameView(self)
        self.metadata = {'render.modes': ['human']}
        self._act = torch.zeros(b.action_shape, dtype=torch.float32, device=b.device)
        self._ref = torch.zeros((3, 1), dtype=torch.float32, device=b.device)
        self._init = torch.zeros((6, 1), dtype=torch.float32, device=b.device)
        self._rng = np.random
        # step() I/O in PINNED HOST memory that the kernel reads and writes directly (hipHostMalloc memory is mapped into the device's
        # address space at the same address): one launch and one stream synchronisation per step instead of an H2D copy, a launch and
        # three D2H copies with a synchronisation each.  The C ABI wants device-ACCESSIBLE pointers, which these are.
        self._h_act = torch.zeros(b.action_shape, dtype=torch.float32).pin_memory()
        self._h_ref = torch.zeros((3, 1), dtype=torch.float32).pin_memory()
        self._h_obs = torch.zeros(b.obs_shape, dtype=torch.float32).pin_memory()
        self._h_rew = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._h_done = torch.zeros(1, dtype=torch.uint8).pin_memory()
        self._np_act, self._np_ref = self._h_act.numpy(), self._h_ref.numpy()
        self._np_obs, self._np_rew, self._np_done = self._h_obs.numpy(), self._h_rew.numpy(), self._h_done.numpy()
        self._sio = _lib.StepIO()
        self._sio.struct_size = C.sizeof(_lib.StepIO)
        self._sio.action = self._h_act.data_ptr()
        self._sio.obs = self._h_obs.data_ptr()
        self._sio.reward = self._h_rew.data_ptr()
        self._sio.done = self._h_done.data_ptr()

    # ENV:92-133
    def step(self, action, new_ref=None):
        torch = _torch()
        b = self._benv
        if b.obs_torch_dtype != torch.float32:
            raise ValueError('the single-env adapter returns float64 observations made from float32 rows')
        a = np.asarray(action, dtype=np.float32)
        if a.size != b.num_actions:
            raise ValueError('action must have %d elements for the %s env (got shape %s)' % (b.num_actions, b.name, a.shape))
        self._np_act[...] = a.reshape(b.action_shape)
        self._sio.new_ref = None
        if new_ref is not None:
            self._np_ref[...] = np.asarray(new_ref, dtype=np.float32).reshape(3, 1)
            self._sio.new_ref = self._h_ref.data_ptr()
        stream = torch.cuda.current_stream(b.device)
        _lib.check(b.lib.dpenv_step_ex(b._h, C.byref(self._sio), C.c_void_p(stream.cuda_stream)), b._h)
        stream.synchronize()                     # the kernel's stores to the pinned rows are visible to the host from here
        o = self._np_obs.reshape(-1).astype(np.float64)
        r = float(self._np_rew[0])
        d = bool(int(self._np_done[0]) & (_lib.DONE_TERMINAL | _lib.DONE_FAULT))
        return o, r, d, {'None': 0}

    # ENV:135-194
    def reset(self, new_ref=None, fraction=0.8, fixed_point=None, **init):
        torch = _torch()
        if not init:
            N, E, Y, u, v, r = 0, 0, 0, 0, 0, 0
            if not self.testing:
                N, E, Y = simtools.get_pose_on_state_space(self.real_ss_bounds[0:3], fraction=fraction)
                u, v, r = simtools.get_vel_on_state_space(self.real_ss_bounds[3:], fraction=0.30 * fraction)
            elif fixed_point is None:
                N, E, Y = simtools.get_random_pose_on_radius()
            else:
                N, E, Y = simtools.get_fixed_pose_on_radius(n=fixed_point)
        else:
            # the reference forwards 'Module.Feature' keys to the plant (ENV:152,159-161)
            N, E = init.get('Hull.PosNED', [0, 0])[:2]
            Y = init.get('Hull.PosAttitude', [0, 0, 0])[2]
            nu6 = init.get('Hull.VelocityNu', [0] * 6)
            u, v, r = nu6[0], nu6[1], nu6[5]
        self._init.copy_(torch.tensor([N, E, Y, u, v, r], dtype=torch.float32).reshape(6, 1))
        nr = None
        if self.testing and new_ref is not None:   # ENV:155-156
            self._ref.copy_(torch.tensor(new_ref, dtype=torch.float32).reshape(3, 1))
            nr = self._ref
        obs = self._benv.reset(init=self._init, new_ref=nr)
        if self.reset_actions:
            # ENV:179-188: previous thrust ~ clip(N(0, 0.1) * 100)
            a = np.clip(self._rng.normal(loc=0.0, scale=0.1, size=3) * 100.0, -100.0, 100.0)
            st, _ = self._benv.get_state()
            st[_lib.S['PT_BOW']:_lib.S['PT_BOW'] + 3, 0] = torch.tensor(a, dtype=torch.float32)
            self._benv.set_state(st.contiguous(), None)
            return self.state_extended() if self.extended_state else self.state()
        return obs.float().cpu().numpy().reshape(-1).astype(np.float64)

    # ENV:196-213 (host-side views of the device state; not on the hot path)
    def _state9(self):
        st, _ = self._benv.get_state()
        s = st[:, 0].cpu().numpy().astype(np.float64)
        eN, eE = s[0] - s[6], s[1] - s[7]
        deg = self._benv.cfg.wrap_mode == _lib.WRAP_REFERENCE
        ref = 180.0 if deg else math.pi
        wrap = lambda x: np.mod(x + ref, 2 * ref) - ref
        rot = wrap(s[2])
        x = math.cos(rot) * eN + math.sin(rot) * eE
        y = -math.sin(rot) * eN + math.cos(rot) * eE
        return np.array([x, y, wrap(s[2] - s[8]), s[3], s[4], s[5], s[9] / 100.0, s[10] / 100.0, s[11] / 100.0])

    def state(self):
        return self._state9()[:6]

    def state_extended(self):
        return self._state9()

    def is_terminal(self):
        return bool(np.any(np.abs(self.state()) > np.array(self.real_ss_bounds)))

    # ENV:215-244 (pure host helpers used by the evaluation harness, test_policy.py:160)
    def scale_and_clip(self, action):
        bnds = np.array(self.real_action_bounds)
        return np.clip(np.multiply(action, bnds), -bnds, bnds).tolist()

    def handle_continuous_angles(self, action):
        assert self.name.lower() == 'revoltfinal' and self.cont_ang is True
        a_port = np.arctan2(action[3], action[4]) / self.real_action_bounds[3]
        a_star = np.arctan2(action[5], action[6]) / self.real_action_bounds[3]
        return np.hstack((action[0:3], np.array([a_port, a_star])))

    def wrap_stern_angles(self, action):
        assert self.name.lower() == 'revoltfinal' and self.cont_ang is False
        b = self.real_action_bounds[3]
        w = lambda x: (np.mod(x * b + math.pi, 2 * math.pi) - math.pi) / b
        return np.hstack((action[0:3], np.array([w(action[3]), w(action[4])])))

    def render(self):
        pass

    def close(self):
        self._benv.close()


class RevoltSimple(Revolt):
    _variant = 'simple'

    def __init__(self, digitwin=None, testing=False, realtime=False, max_ep_len=800, extended_state=False,
                 reset_acts=False, cont_ang=False, **kw):
        super().__init__(digitwin=digitwin, testing=testing, realtime=realtime, max_ep_len=max_ep_len,
                         extended_state=extended_state, reset_acts=reset_acts, cont_ang=False, **kw)


class RevoltLimited(Revolt):
    _variant = 'limited'

    def __init__(self, digitwin=None, testing=False, realtime=False, max_ep_len=800, extended_state=False,
                 reset_acts=False, cont_ang=False, **kw):
        super().__init__(digitwin=digitwin, testing=testing, realtime=realtime, max_ep_len=max_ep_len,
                         extended_state=extended_state, reset_acts=reset_acts, cont_ang=False, **kw)


class RevoltFinal(Revolt):
    _variant = 'final'

    def __init__(self, digitwin=None, testing=False, realtime=False, max_ep_len=800, extended_state=False,
                 reset_acts=False, cont_ang=False, **kw):
        super().__init__(digitwin=digitwin, testing=testing, realtime=realtime, max_ep_len=max_ep_len,
                         extended_state=extended_state, reset_acts=reset_acts, cont_ang=cont_ang, **kw)


ENVIRONMENTS = {'simple': RevoltSimple, 'limited': RevoltLimited, 'final': RevoltFinal, 'full': Revolt}   # trainer.py:15
