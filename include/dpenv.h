/*
 * dpenv.h - C ABI of libdpenv.so: the MI355X-native batched ReVolt dynamic-positioning
 * environment (env.step hot path of simensov/ml4ca as one HIP kernel for gfx950).
 *
 * This is the drop-in boundary.  The reference is pure Python with no FFI of its own; the
 * interface this library replaces is (paths relative to the reference root,
 * WW = src/rl/windows_workspace):
 *   - upper boundary, what the PPO loop calls: Revolt.reset / Revolt.step
 *       WW/specific/customEnv.py:135-194, :92-133  (consumed at WW/spinup/algos/tf1/ppo/ppo.py:286-322)
 *   - lower boundary, the plant plug-in seam it swallows: DigiTwin.val / DigiTwin.step
 *       WW/specific/digitwin.py:50-114, :213-219   (py4j RPC into the Cybersea simulator)
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain C: opaque handle, raw pointers and sizes, int status codes.  No torch types.
 *   - Every bulk-data pointer is a DEVICE pointer owned by the caller (e.g. tensor.data_ptr());
 *     config structs and vessel parameter vectors are HOST memory.  A NULL optional pointer
 *     means "not requested".
 *   - The library owns the per-env state block in HBM behind the handle.  No allocation,
 *     no host synchronisation inside reset/step: calls are ordered on the hipStream_t passed in
 *     and are graph-capturable.
 *   - One handle per (process, GPU).  A handle is not thread-safe; different handles are independent.
 *   - Thruster order everywhere: 0 = bow (THR1), 1 = stern port (THR2), 2 = stern starboard (THR3)
 *     (customEnv.py:48-50).  The ROS/QP code uses port, star, bow (qp_allocator.py:69-70).
 *   - Return value: DPENV_OK or a negative DPENV_E*; dpenv_last_error() gives the message.
 *     There is NO CPU fallback: without a usable gfx950 device dpenv_create fails with DPENV_ENODEV.
 */
#ifndef DPENV_H
#define DPENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPENV_ABI_VERSION 6

typedef struct dpenv_s* dpenv_handle;
typedef void* dpenv_stream; /* hipStream_t; NULL = the null stream */

enum {
    DPENV_OK = 0,
    DPENV_EINVAL = -1,  /* bad argument / unsupported combination */
    DPENV_ENODEV = -2,  /* no usable HIP device */
    DPENV_ENOMEM = -3,  /* device allocation failed */
    DPENV_EHIP = -4,    /* HIP runtime error (launch, copy) */
};

/* env variants, customEnv.py:11 (Revolt, name 'full'), :327 RevoltSimple, :351 RevoltLimited, :373 RevoltFinal */
enum { DPENV_FULL = 0, DPENV_SIMPLE = 1, DPENV_LIMITED = 2, DPENV_FINAL = 3 };
/* memory layout of action / observation batches */
enum { DPENV_AOS = 0 /* [n_envs][dim] row-major (torch-native) */, DPENV_SOA = 1 /* [dim][n_envs] */ };
/* yaw wrap in the error frame: REFERENCE replicates errorFrame.py:29,31 calling wrap_angle with its
 * default deg=True on radians (mathematics.py:14); RADIANS wraps to [-pi,pi) like the ROS node. */
enum { DPENV_WRAP_REFERENCE = 0, DPENV_WRAP_RADIANS = 1 };
enum { DPENV_F32 = 0, DPENV_BF16 = 1 };
/* bits of the per-env done byte */
enum { DPENV_DONE_TERMINAL = 1 /* is_terminal, customEnv.py:207-213 */,
       DPENV_DONE_TIMELIMIT = 2 /* traj_len == max_ep_len, ppo.py:304 */,
       DPENV_DONE_FAULT = 4 /* non-finite state or action (also sets TERMINAL) */ };

/* canonical state exchange format for get/set_state: float state[DPENV_NSTATE][n_envs] */
enum {
    DPENV_S_N = 0, DPENV_S_E, DPENV_S_PSI, DPENV_S_U, DPENV_S_V, DPENV_S_R,
    DPENV_S_REF_N, DPENV_S_REF_E, DPENV_S_REF_PSI,
    DPENV_S_PT_BOW, DPENV_S_PT_PORT, DPENV_S_PT_STAR, /* previous thrust command, percent (customEnv.py:126) */
    DPENV_S_A_BOW, DPENV_S_A_PORT, DPENV_S_A_STAR,    /* azimuth command in force, rad (customEnv.py:122) */
    DPENV_NSTATE
};
/* int32 counters[2][n_envs]: [0] steps taken in the running episode, [1] episodes sampled so far */

/* vessel parameter vector: float[DPENV_NPARAM] per vessel class.  Hull terms are BUILD-OWNED (the
 * reference's plant is the closed Cybersea simulator); thruster terms come from the reference
 * (K: qp_allocator.py:51-55 / SupervisedTau.py:69-71, lever arms: qp_allocator.py:69-70). */
enum {
    DPENV_P_M11 = 0, DPENV_P_M22, DPENV_P_M23, DPENV_P_M33, /* rigid-body + added mass, symmetric */
    DPENV_P_XU, DPENV_P_XUU, DPENV_P_YV, DPENV_P_YVV, DPENV_P_YR, DPENV_P_NV, DPENV_P_NR, DPENV_P_NRR, /* damping >= 0 */
    DPENV_P_KF_BOW, DPENV_P_KF_PORT, DPENV_P_KF_STAR, /* F = K n|n|, n >= 0 */
    DPENV_P_KR_BOW, DPENV_P_KR_PORT, DPENV_P_KR_STAR, /* n < 0 */
    DPENV_P_LX_BOW, DPENV_P_LX_PORT, DPENV_P_LX_STAR,
    DPENV_P_LY_BOW, DPENV_P_LY_PORT, DPENV_P_LY_STAR,
    DPENV_P_NUV, DPENV_P_YUR, /* speed-proportional cross-flow terms: yaw moment -N_uv u v (adds to the Munk moment -(m22-m11) u v; N_uv < -(m22-m11) would make the hull weathervane-stable), sway force -Y_ur u r */
    /* BUILD-OWNED inflow thrust loss (the linear open-water characteristic, Fossen 2011 eq. 9.7): F = K n|n| - Kl |n| u_a, u_a = the speed through
     * the water of the thruster's position along its axis at the start of the env step, never past zero thrust; [N per percent per m/s], >= 0.
     * 0 (the default hull) is the reference's law F = K n|n| (SupervisedTau.py:42-83) exactly.  Non-zero coefficients are carried by the SINGLE
     * class of dpenv_create (kernel arguments: the shared training form, the default's cost) or by per-env blocks (the general per-env kernels);
     * vessel CLASSES (n_classes > 1) may not have them. */
    DPENV_P_KLF_BOW, DPENV_P_KLF_PORT, DPENV_P_KLF_STAR, /* n >= 0 */
    DPENV_P_KLR_BOW, DPENV_P_KLR_PORT, DPENV_P_KLR_STAR, /* n < 0 */
    DPENV_NPARAM = 32,
    DPENV_NPARAM_USED = 32
};
#define DPENV_MAX_CLASSES 64   /* classes share LDS-staged tables; for more distinct hulls than that - one per env - see dpenv_set_vessel_params */

typedef struct dpenv_config {
    uint32_t struct_size;    /* sizeof(dpenv_config), ABI check */
    int32_t n_envs;
    int32_t device;          /* HIP device ordinal, -1 = current */
    int32_t variant;         /* DPENV_FULL .. DPENV_FINAL */
    int32_t extended_state;  /* obs dim 9 (1) or 6 (0), customEnv.py:44,201-205 */
    int32_t cont_ang;        /* FINAL only: 7 actions with sin/cos azimuth heads, customEnv.py:227-235.  Supported head magnitudes:
                                2^-60 <= max(|sin head|, |cos head|) <= 2^60 per pair, or both heads zero (then, like numpy.arctan2,
                                the sign of the zero cos head decides: +0 -> azimuth +-0, -0 -> azimuth +-pi, force and bookkeeping
                                alike).  Outside that range a step stays finite and raises no fault bit, but the force no longer
                                follows the azimuth: a pair with sin^2 + cos^2 below the smallest normal float pushes as a zero
                                pair, one whose sum overflows (heads above about 2^63) gives no force. */
    int32_t n_substeps;      /* plant sub-steps per env step, 20 (customEnv.py:79-80) */
    float substep_dt;        /* 0.01 s (customEnv.py:81) */
    int32_t wrap_mode;       /* DPENV_WRAP_* */
    int32_t terminate;       /* 1: evaluate is_terminal bounds; 0: never terminal */
    int32_t max_ep_len;      /* time limit in env steps (train.py:70-73 -> 400); 0 = none */
    int32_t auto_reset;      /* re-sample finished envs inside step (ppo.py:305-322 batched) */
    int32_t action_layout;   /* DPENV_AOS / DPENV_SOA */
    int32_t obs_layout;
    int32_t obs_dtype;       /* DPENV_F32 / DPENV_BF16 */
    int32_t current_enabled; /* per-env constant irrotational current, see dpenv_set_current */
    uint64_t seed;           /* Philox key of the reset sampler */
    int64_t env_id_base;     /* global id of local env 0: results do not depend on the rank count */
    float reset_fraction;    /* 0.8 (customEnv.py:135; curriculum hook ppo.py:286,319) */
    int32_t hold_plant;      /* 1: hull state is held while the step runs, like Hull.StateResetOn=1
                                (customEnv.py:164-167); lets parity tests replay the reference's scripted-plant
                                fixtures through the kernel.  0 in production. */
    int32_t current_drift;   /* 1: V_c and beta_c follow a first-order Gauss-Markov process around the values given to
                                dpenv_set_current (config 5's slowly varying disturbance; build-defined) */
    float current_tau;       /* correlation time [s], 100 */
    float current_sigma_v;   /* stationary std of V_c [m/s], 0.02 */
    float current_sigma_beta;/* stationary std of beta_c [rad], 5 deg */
    int32_t reset_acts;      /* 1: an episode starts with previous thrust clip(100 * N(0, 0.1)) instead of zero (the reference's
                                reset_acts constructor flag, customEnv.py:30,179-188); drawn in the kernel by every kind of reset,
                                Philox keyed (seed; global env id, episode) like the pose sample */
    int32_t step_one_wave;   /* 0 (default): dpenv_step with auto_reset on launches a second wave per 64 envs that prepares the re-draw of
                                finished envs beside the plant loop (up to 256 envs per CU), and dpenv_rollout runs an env wave and a row
                                wave per 64 envs (up to 384 envs per CU) - same rows bit for bit, the one-wave kernels above those sizes
                                (DESIGN.md section 4).  1: the one-wave kernels at every size - the A/B switch of tools/ and tests;
                                was `reserved` (0) before round 4 */
    int32_t per_env_lds;     /* per-env parameter blocks in dpenv_step: 0 (default) a lane loads its block straight into registers; 1: by
                                LDS-DMA (global_load_lds_dwordx4) into a [group][lane] LDS image that the step reads back - the A/B SURVEY
                                section 7 asks for ("LDS [matrix_elem][lane] vs plain VGPRs"); same rows bit for bit, slower (DESIGN.md
                                section 4).  The T-step kernels load the block once per launch into registers either way. */
} dpenv_config;

/* Optional outputs / inputs of one step beyond the Gym tuple.  All device pointers, any may be NULL. */
typedef struct dpenv_step_io {
    uint32_t struct_size;
    const float* action;     /* [n][act_dim] or [act_dim][n] per action_layout */
    const float* new_ref;    /* [3][n]: applied AFTER obs/reward/done of this step (customEnv.py:131) */
    void* obs;               /* [n][obs_dim] or [obs_dim][n], f32 or bf16 */
    float* reward;           /* [n] */
    uint8_t* done;           /* [n], DPENV_DONE_* bits */
    float* reward_parts;     /* [4][n]: vel, pose gaussian, thrust penalty, derivative penalty */
    void* final_obs;         /* same layout as obs: terminal observation of envs that auto-reset */
} dpenv_step_io;

/* Fill *cfg with the shipped training configuration (RevoltFinal, extended state, continuous
 * angles, 20 x 0.01 s, T = 400, train.py:47-54).  n_envs is left 0. */
int dpenv_default_config(dpenv_config* cfg);
/* Default ReVolt parameter vector. */
int dpenv_default_vessel(float params[DPENV_NPARAM]);
/* The presets of the build-owned plant, one per set of steady full-thrust speeds the reference records (customEnv.py:13-18):
 * NO_LOSS = dpenv_default_vessel (+2.20 m/s ahead, 0.60 rad/s: "no thrust losses activated"); THRUST_LOSS = the same hull with stern
 * thrusters that meet BOTH sets: their reverse gain from -1.60 m/s astern without losses, their inflow-loss coefficients (DPENV_P_KLF_* /
 * DPENV_P_KLR_*) from +1.4 / -1.1 m/s ahead / astern "with thrust losses" (the velocity bounds the reference trains with, customEnv.py:26);
 * yaw then comes out at 0.505 rad/s against the recorded 0.52 (tests/calibration/fit_thrust_loss_preset.py).  Pass the vector to
 * dpenv_create (one class), in a dpenv_set_vessel_params block, or as `nominal` to dpenv_set_vessel_randomisation. */
enum { DPENV_VESSEL_NO_LOSS = 0, DPENV_VESSEL_THRUST_LOSS = 1,
       /* round 6, a FLAG (combine with THRUST_LOSS: 3): the sway-yaw part of the hull (m22, Yv, Yvv, Yr, Nv, Nr, Nrr, Yur) refitted jointly to
        * what the default hull is fitted to AND to the reference's 32 recorded Cybersea station-keeping runs in a current from 16 directions
        * (results/all_plots/dyn_pos/) AND to the recorded steady sway speed: sway 0.350 m/s (recorded 0.35; default hull 0.29), yaw 0.605, the
        * station-keeping yaw-moment residual halved, at 0.01-0.02 m on the free-drift / box-test / replay rows
        * (tests/calibration/fit_dynpos_preset.py).  Not the default: every row the default hull has produced stays. */
       DPENV_VESSEL_DYNPOS_FIT = 2 };
int dpenv_default_vessel_ex(int32_t kind, float params[DPENV_NPARAM]);
/* Derived sizes for a config. */
int dpenv_act_dim(const dpenv_config* cfg);
int dpenv_obs_dim(const dpenv_config* cfg);

/* Create an environment batch.  vessel_params: host float[n_classes][DPENV_NPARAM], NULL = one
 * default class.  With n_classes > 1 call dpenv_set_vessel_class to assign envs to classes.
 * A single class with thrust-loss coefficients (dpenv_default_vessel_ex(DPENV_VESSEL_THRUST_LOSS, ...)) runs on kernels that take hull AND
 * coefficients from their arguments - dpenv_step, dpenv_rollout, and dpenv_policy_rollout's two-wave form in the shipped configuration (final
 * variant, continuous angles, extended state, leaky-relu): the traffic of the default hull; the other closed-loop forms read that hull from a
 * per-env image (every env the same block).  dpenv_get_vessel_params works; dpenv_set_vessel_params(h, NULL, s) returns to this class WITH
 * its loss.  Classes (n_classes > 1) with coefficients are refused. */
int dpenv_create(const dpenv_config* cfg, const float* vessel_params, int32_t n_classes, dpenv_handle* out);
int dpenv_destroy(dpenv_handle h);
/* Message of the last failure on this handle (h == NULL: last failure of dpenv_create in this thread). */
const char* dpenv_last_error(dpenv_handle h);

/* Change the pose/velocity fraction of the training reset sampler (curriculum hook, ppo.py:286,319-322). */
int dpenv_set_reset_fraction(dpenv_handle h, float fraction);
/* class_id: device int32[n_envs], values in [0, n_classes).  Copied. */
int dpenv_set_vessel_class(dpenv_handle h, const int32_t* class_id, dpenv_stream s);

/* ---- per-env vessel parameter blocks (north_star: "per-env 3x3 mass / Coriolis / damping blocks"; SURVEY appendix D: "M, D as per-env
 * SoA parameter arrays (domain randomisation) with a shared-default fast path") -----------------------------------------------------
 * Every env gets its OWN hull and thruster parameters - the constants the reference hard-codes once for its one vessel
 * (qp_allocator.py:51-55,69-70 K and lever arms, SupervisedTau.py:35-36,69-71) and the build-owned mass / damping terms of the plant
 * that stands in for customEnv.py:124.  params: DEVICE float[DPENV_NPARAM][n_envs] (structure of arrays: row p = parameter DPENV_P_p of
 * every env), copied on the stream: one kernel derives each env's mass-matrix inverse (the same float operations
 * as for a class, so an env given its class's numbers reproduces the class path bit for bit) and packs the block as eight float4
 * streams (+ two for the thrust-loss coefficients).  dpenv_step then reads 128 B more per env-step (SURVEY 8d accounts 108 B: 285 B per
 * env-step); the T-step kernels (dpenv_rollout, dpenv_policy_rollout) load the block once per launch.  A block that is not a vessel (mass
 * matrix not positive definite, non-finite entry, negative loss coefficient) is not rejected here: that env reports DPENV_DONE_FAULT at
 * its first step.  If ANY env has a thrust-loss coefficient the general per-env kernels apply it (they read 32 B more per env-step; envs
 * without a coefficient get the rows of the plain per-env kernels bit for bit).  Whether any env has one is a word the packing kernel leaves
 * behind the table: the setter does NOT wait for it - it is stream-ordered and may be recorded into a HIP graph.  Outside a capture the word
 * travels to the host behind an event and the next launch on this handle takes it from there (waiting for that one event if need be); a
 * launch that is itself being recorded, and every launch after a RECORDED setter, runs the general kernels with the coefficients applied -
 * zeros where there are none, which change no row.  A refused call (bad flags, a HIP error) leaves the handle's switches - per-env blocks,
 * randomisation, thrust loss - as they were.
 * params == NULL: back to the vessel classes / the single class of dpenv_create (the shared-default fast path: parameters in SGPRs).
 * Switching between the paths voids HIP graphs captured before (the table's address is a kernel argument).
 * flags (dpenv_set_vessel_params_ex): DPENV_VESSEL_KEEP_RANDOMISATION - the table is installed while the domain randomisation STAYS in force
 * (dpenv_set_vessel_randomisation must have been called): the restore path of a checkpoint taken mid-episode - fresh handle, same config;
 * dpenv_set_vessel_randomisation(nominal, range); dpenv_set_vessel_params_ex(saved table, KEEP); dpenv_set_state(saved state, counters) - the
 * run continues bit for bit, hulls re-drawn at every later reset.  dpenv_set_vessel_params(h, p, s) = _ex(h, p, 0, s): ends the re-draws. */
enum { DPENV_VESSEL_KEEP_RANDOMISATION = 1 };
int dpenv_set_vessel_params_ex(dpenv_handle h, const float* params, uint32_t flags, dpenv_stream s);
int dpenv_set_vessel_params(dpenv_handle h, const float* params, dpenv_stream s);
/* The parameter vectors in force: DEVICE float[DPENV_NPARAM][n_envs] - the per-env blocks, or, with ONE class and none in force, that class's
 * vector in every column.  Refused with vessel classes (n_classes > 1) and no per-env blocks. */
int dpenv_get_vessel_params(dpenv_handle h, float* params_out, dpenv_stream s);
/* Domain randomisation through the reset path: from this call on EVERY reset of an env - dpenv_reset (also with explicit init),
 * auto-reset inside dpenv_step / dpenv_rollout / dpenv_policy_rollout, reset_at_end - starts the new episode on a freshly drawn hull:
 *   parameter p = nominal[p] * (1 + rel_range[p] * u),  u uniform in [-1, 1) (16 bits),
 * Philox4x32-10 keyed by config.seed with counter (global env id, episode counter, tag 0x48000000 | block) - parameter p takes the
 * 16-bit half (q & 1) of word (q & 7) >> 1 of block q >> 3, q = its slot in the order m11 m22 m23 m33 Xu (0..4) | Xuu Yv Yvv Yr Nv Nr Nrr
 * Nuv (8..15) | Yur Kf[3] Kr[3] lx_bow (16..23) | lx_port lx_star ly[3] Klf[3] (24..31), Klr[3] (5..7); u = h / 32768 - 1: a function of the env and of
 * its episode like the pose sample, so hulls do not depend on the rank count or on the launch form, and a checkpoint (dpenv_get_state
 * counters + dpenv_get_vessel_params) restores them through dpenv_set_vessel_params_ex(..., DPENV_VESSEL_KEEP_RANDOMISATION).  nominal: HOST float[DPENV_NPARAM], NULL = class 0 of dpenv_create; rel_range:
 * HOST float[DPENV_NPARAM], entries in [0, 1), 0 = that parameter is not randomised; every hull of the range must have a positive
 * definite mass matrix (checked).  Until its first reset an env runs on the nominal hull.  Implies per-env blocks;
 * rel_range == NULL stops the re-draws (the hulls in force stay); dpenv_set_vessel_params(h, NULL / table, s) ends it as well.
 * With the randomisation on, a dpenv_reset with explicit init advances the episode counter too (it consumes random numbers). */
int dpenv_set_vessel_randomisation(dpenv_handle h, const float* nominal, const float* rel_range, dpenv_stream s);
/* vc, beta: device float[n_envs] current speed [m/s] and NED direction [rad].  Copied; they are both the
 * present value and the mean the drift process reverts to. */
int dpenv_set_current(dpenv_handle h, const float* vc, const float* beta, dpenv_stream s);
/* Only the PRESENT values (the drift's state), leaving the means alone: restores what dpenv_get_current returned (checkpoints). */
int dpenv_set_current_present(dpenv_handle h, const float* vc, const float* beta, dpenv_stream s);
/* present current of every env (differs from the set values only with current_drift / the per-episode randomisation) */
int dpenv_get_current(dpenv_handle h, float* vc_out, float* beta_out, dpenv_stream s);
/* the means the drift reverts to (= the values given to dpenv_set_current until a randomised reset re-draws them): with dpenv_get_current the
 * current's part of a checkpoint - restore with dpenv_set_current(means) followed by dpenv_set_current_present(present values) */
int dpenv_get_current_mean(dpenv_handle h, float* vc_out, float* beta_out, dpenv_stream s);
/* Per-episode randomisation of the current through the reset path (config 5 widened; the reference's one operating point is 0.2 m/s towards
 * 135 deg, results/all_plots/current_box_test/plot_pos.py:78): from this call on EVERY reset of an env - dpenv_reset (also with explicit
 * init), auto-reset inside dpenv_step / dpenv_rollout / dpenv_policy_rollout, reset_at_end - starts the new episode in a freshly drawn current
 *   V_c = max(0, vc_nominal[i] + vc_range * u1),   beta_c = beta_nominal[i] + beta_range * u2,   u1, u2 uniform in [-1, 1) (24 bits),
 * words 0 and 1 of Philox4x32-10 keyed by config.seed with counter (global env id, episode counter, tag 3): a function of the env and of
 * its episode like the pose sample and the hull draw - independent of the rank count and of the launch form.  The drawn values become the
 * present current AND the mean the drift (config.current_drift) reverts to.  vc_nominal, beta_nominal: DEVICE float[n_envs], copied; NULL =
 * the means in force (what dpenv_set_current gave; a checkpoint restore passes the ORIGINAL nominals explicitly: by then the means are drawn
 * values).  Until its first reset an env keeps the current it has.  Needs config.current_enabled.
 * The re-draw lives in the kernels that carry re-draws: with ONE class, the shared training form (hull and thrust-loss coefficients - zero for
 * a hull without a loss - as kernel arguments: the default's memory traffic, the default's rows until a reset draws); with per-env blocks in
 * force, the general per-env kernels; vessel classes (n_classes > 1 without per-env blocks) are refused, and so is returning to them with
 * dpenv_set_vessel_params(h, NULL, s) while it is on.  Both ranges 0: off (currents stay as they are).  Like the hull randomisation, a dpenv_reset
 * with explicit init then advances the episode counter too.  Stream-ordered, may be recorded into a graph. */
int dpenv_set_current_randomisation(dpenv_handle h, const float* vc_nominal, const float* beta_nominal, float vc_range, float beta_range,
                                    dpenv_stream s);

/* Revolt.reset (customEnv.py:135-194) for the envs selected by mask (device uint8[n], NULL = all).
 * init: device float[6][n] = N, E, psi, u, v, r (the **init override, customEnv.py:141,152), NULL =
 * training sample (simtools.py:109-123).  ref: device float[3][n] new setpoints, NULL = keep.
 * obs_out (optional) receives the observation of EVERY env. */
int dpenv_reset(dpenv_handle h, const uint8_t* mask, const float* init, const float* ref, void* obs_out,
                dpenv_stream s);

/* Revolt.step (customEnv.py:92-133) for all envs. */
int dpenv_step(dpenv_handle h, const float* action, const float* new_ref, void* obs_out, float* rew_out,
               uint8_t* done_out, dpenv_stream s);
int dpenv_step_ex(dpenv_handle h, const dpenv_step_io* io, dpenv_stream s);

/* Fused rollout: T env steps in ONE launch with the state resident in registers.  Exactly the semantics of T
 * successive dpenv_step calls with actions[t] as the action and, at t == switch_step[k], refs[k] as new_ref
 * (the setpoint-sequence form of test_policy.py:127,148-153 / results/all_plots/box_test/plot_pos.py:55-59).
 * obs[t] is the observation returned by step t.  Open loop: the action block must exist before the launch
 * (recorded command sequences, pre-sampled exploration noise, benchmark input). */
#define DPENV_MAX_SWITCH 8
typedef struct dpenv_rollout_io {
    uint32_t struct_size;
    int32_t T;
    const float* actions;    /* [T][n][act_dim] (AOS) or [T][act_dim][n] (SOA) */
    void* obs;               /* [T][n][obs_dim] or [T][obs_dim][n]; f32 or bf16 */
    float* reward;           /* [T][n] */
    uint8_t* done;           /* [T][n], DPENV_DONE_* bits */
    int32_t n_switch;        /* 0..DPENV_MAX_SWITCH, switch_step strictly increasing */
    int32_t switch_step[DPENV_MAX_SWITCH];
    const float* refs;       /* [n_switch][3][n] */
} dpenv_rollout_io;
int dpenv_rollout(dpenv_handle h, const dpenv_rollout_io* io, dpenv_stream s);

/* ---- actor-critic in the loop -------------------------------------------------
 * The PPO actor-critic of the reference (mlp_gaussian_policy / mlp_actor_critic, spinup/algos/tf1/ppo/core.py:29-33,
 * 80-107; shipped model 9-80-80-80-7 + 9-80-80-80-1, leaky_relu 0.2, config.json) evaluated inside the rollout
 * launch on the matrix cores (f16 weights/activations, f32 accumulate), so that one launch produces T rows of the
 * trajectory buffer (o, a, r, v, logp) of ppo.py:298 for every env. */
enum { DPENV_ACT_LEAKY_RELU = 0, DPENV_ACT_TANH = 1 };
typedef struct dpenv_mlp {
    int32_t n_layers;        /* dense layers = hidden layers + 1, in [2, 5] */
    int32_t sizes[6];        /* n_layers + 1 widths, e.g. {9, 80, 80, 80, 7}; hidden widths equal and <= 96 */
    const float* W[5];       /* W[l][in][out] row-major (tf.layers.dense kernel layout); host or device, see dpenv_policy_desc */
    const float* b[5];       /* b[l][out] */
} dpenv_mlp;
/* Arithmetic of the in-kernel networks.  F16: f16 weights and activations, f32 accumulation - the fast mode, within ~5e-4 of
 * the output scale of an fp32 evaluation.  F32: "fp32-faithful" split-f16 arithmetic (W = Wh + Wl, x = xh + xl, three MFMAs per
 * product, activations in f32): mu, v, logp within 1e-5 of an fp32 evaluation of core.py:29-33,80-107 - the mode parity with
 * the reference's fp32 TF1 networks is claimed on; three times the matrix work of F16.
 * F32_ACTOR: the actor (mu, and with it the sampled action and logp) in the F32 arithmetic, the critic in the F16 arithmetic: what a
 * PPO update needs exactly is the log-likelihood (the ratio exp(logp_new - logp_old) then starts at 1); values carry the F16 mode's
 * ~5e-4 and are bit-identical to the F16 mode's.  Two thirds of the matrix work of F32.
 * SUPPORTED RANGE of these figures (tests/policy_edges.py domain(), measured in DESIGN.md section 4).  Every mode passes the
 * observation and every hidden activation through f16: their magnitudes must stay below 2^15 (f16 ends at 65 504).  An env whose
 * observation or hidden value leaves f16's range gets meaningless rows - non-finite mu, v, action and logp in every mode, except F16
 * with tanh, where the infinite pre-activation saturates to +-1 and the rows are finite and wrong - for that env alone: every other
 * env of the launch, the other columns of its MFMA tile and the other wave of its pair included, keeps its rows bit for bit.  An fp32
 * network is finite there; the library neither rescales nor clamps.  Below 2^15, with S = the largest |output| and never less than 1:
 *   leaky-relu / relu: F32 within 1e-5 S, F16 within 2e-3 S (5e-4 S is typical, 1e-3 S the largest measured) at every observation and
 *     weight scale - the output scale grows with the input's, and the error with it; exact zeros and f16-subnormal inputs included.
 *   tanh: its outputs stay O(1) while the rounding of the first layer's inputs grows with them, so the figures hold only while
 *     growth = max(1, max|obs| / 16) x weight scale  is at most 2^5 in F32 and at most 2 in F16, with weight scale = the largest
 *     max|W| / sqrt(6 / (fan_in + fan_out)) over the dense kernels of both networks and never less than 1 (it is 1 at the
 *     glorot-uniform initialisation).  The limits are conservative and come from a CPU model of this arithmetic, swept at weights
 *     x 1, x 2, x 4: F32 stays below 4e-6 S up to growth 2^5 and first misses 1e-5 S at 2^7; F16 stays below 1e-3 S up to growth 2
 *     and first misses 2e-3 S at 2^3.  Measured on the device beyond them: F16 off by 5.9e-3 S at growth 57 (max|obs| 909) and by
 *     1.5e-2 S at growth 114; at growth 4 (weights x 4, |obs| < 16) F16 is at 1.1e-3 S - still within 2e-3 S, but not promised.
 * At log_std = -4 (std = e^-4, the lower clamp of examples/train_ppo.py) an error of mu is 55 x as large in z.  Measured with noise
 * up to +-5 (summed terms of logp up to 87): F32 / F32_ACTOR are within 9e-5 in logp and the first PPO ratio of dpenv_ppo_actor_grad on
 * those rows within 4e-7 of 1; F16's logp is off by 0.2 and a fresh update clips some of its rows. */
enum { DPENV_POLICY_F16 = 0, DPENV_POLICY_F32 = 1, DPENV_POLICY_F32_ACTOR = 2 };
/* Launch form of dpenv_policy_rollout.  TWO_WAVE: every 64 envs get an env wave and a network wave (pair-level LDS hand-over;
 * 256-env workgroups with both waves of a pair on one SIMD, or - while one round of them fits the chip, n_envs <= 128 x CUs -
 * 128-env workgroups with a SIMD per wave); ONE_WAVE: one wave does both.  Both write identical rows.  AUTO picks TWO_WAVE where
 * it exists (every arithmetic with leaky-relu / relu, F16 also with tanh) and its LDS footprint (the weight images its network wave
 * reads + 40-50 KiB of mailboxes) fits the 160 KiB, else ONE_WAVE. */
enum { DPENV_LAUNCH_AUTO = 0, DPENV_LAUNCH_ONE_WAVE = 1, DPENV_LAUNCH_TWO_WAVE = 2 };
typedef struct dpenv_policy_desc {
    uint32_t struct_size;
    const dpenv_mlp* pi;     /* obs_dim -> act_dim */
    const dpenv_mlp* v;      /* obs_dim -> 1, same hidden shape */
    const float* log_std;    /* float[act_dim] (core.py:83) */
    int32_t activation;      /* DPENV_ACT_* */
    float leak;              /* leaky-relu slope in [0, 1] */
    int32_t precision;       /* DPENV_POLICY_* */
    int32_t launch_form;     /* DPENV_LAUNCH_* */
    int32_t device_pointers; /* 0: W, b, log_std are HOST pointers (copied on the stream, then packed on the device);
                                1: they are DEVICE pointers (e.g. the optimiser's own parameter tensors): packed by one kernel
                                on the stream - no host copy, no synchronisation, graph-capturable.  Re-upload after every
                                PPO update (ppo.py:260-280) costs one small launch. */
    int32_t reserved;
} dpenv_policy_desc;
/* Pack the networks into the image the rollout kernels stage into LDS.  Launches issued (on any stream) before this call keep
 * the weights they were given: the library holds two images and writes them alternately, and the packing waits (on `s`, by event)
 * for the last launch that read the image it reuses.  Launches issued afterwards read the new image; they are ordered behind the
 * packing if they are issued on `s` (or on a stream the caller orders behind `s`).  device_pointers = 1: stream-ordered, no host
 * synchronisation, graph-capturable.  device_pointers = 0 (host arrays): the call synchronises `s` before it returns, so the
 * arrays may be freed or changed at once.  Fails with DPENV_EINVAL if the requested launch form cannot hold the networks in the
 * 160 KiB LDS; after a failed DPENV_ENOMEM no policy is in force.
 * Graphs: a dpenv_policy_rollout / dpenv_policy_forward RECORDED INTO A HIP GRAPH has the address of the image that was current at
 * capture time baked into its kernel node.  From that capture on, every eager upload is written IN PLACE into that image (no more
 * alternation), so a replay always runs the weights of the latest upload - the usual PPO pattern "upload each epoch, replay the rollout
 * graph" works with any number of uploads between replays.  Ordering of an in-place upload: behind eager readers of the image by their
 * event (any stream), behind graph replays by STREAM ORDER - replay and upload on one stream, or order the two streams yourself.  An
 * upload recorded into the graph itself (device pointers) re-packs from the weight tensors at every replay.  Growing the network shape
 * (a larger image) voids graphs captured before. */
int dpenv_set_policy_desc(dpenv_handle h, const dpenv_policy_desc* d, dpenv_stream s);
/* What DPENV_LAUNCH_AUTO resolved to for the policy in force: *two_wave_out = 1 for the two-wave form, *envs_per_workgroup_out = 256 or
 * 128 (host ints, either may be NULL). */
int dpenv_get_policy_launch(dpenv_handle h, int32_t* two_wave_out, int32_t* envs_per_workgroup_out);
/* The same and more, as the library resolved it: out[0] two-wave form (0 / 1), out[1] envs per workgroup, out[2] waves per 64 envs (1 one-wave
 * form, 2 env + network wave, 3 env + actor + critic wave), out[3] the arithmetic (DPENV_POLICY_*). */
int dpenv_get_policy_launch_ex(dpenv_handle h, int32_t out[4]);
/* Ends the pinning described above: call it when every HIP graph that recorded a dpenv_policy_rollout / dpenv_policy_forward of this handle
 * has been destroyed (or will not be replayed again).  Until then an upload whose image LAYOUT differs from the one the graphs were captured
 * with - another hidden shape, precision, activation, leak or launch form; the kernel nodes hold those by value next to the image's address -
 * is refused with DPENV_EINVAL (it would be read with the old layout: wrong weights, no error); new weights of the same layout are what the
 * in-place upload is for.  After the call uploads alternate between the two images again and any layout is accepted. */
int dpenv_release_policy_graphs(dpenv_handle h);
/* Convenience forms (host pointers, F16, AUTO, null stream):
 * pi: obs_dim -> act_dim, v: obs_dim -> 1 (same hidden shape); log_std: host float[act_dim]; leak: hidden
 * leaky-relu slope (0.2 = tf.nn.leaky_relu default; 0 = relu).  Packs and uploads; may be called again after
 * every PPO update. */
int dpenv_set_policy(dpenv_handle h, const dpenv_mlp* pi, const dpenv_mlp* v, const float* log_std, float leak);
/* The same with the hidden activation named: the reference's --activation {leaky, relu, tanh} (train.py:24,31;
 * spinup core.py:29-33 takes any activation, tanh being Spinning Up's default).  relu = DPENV_ACT_LEAKY_RELU with
 * leak 0; leak is ignored for DPENV_ACT_TANH. */
int dpenv_set_policy_ex(dpenv_handle h, const dpenv_mlp* pi, const dpenv_mlp* v, const float* log_std, int32_t activation,
                        float leak);
/* mu_out [n][act_dim], v_out [n] for obs [n][obs_dim] (all device, row-major): the deterministic policy of
 * test_policy.py:90 and the critic. */
int dpenv_policy_forward(dpenv_handle h, const float* obs, float* mu_out, float* v_out, int32_t n, dpenv_stream s);

typedef struct dpenv_policy_rollout_io {
    uint32_t struct_size;
    int32_t T;
    const float* noise;      /* [T][n][act_dim] N(0,1) draws (a = mu + exp(log_std) * noise, core.py:85); NULL: see `sample` */
    void* obs;               /* [T][n][obs_dim]  policy input of step t; f32 or bf16 per config.obs_dtype (the actor
                                always sees the full-precision observation, only the stored row is rounded) */
    float* act;              /* [T][n][act_dim] */
    float* reward;           /* [T][n] */
    float* value;            /* [T][n]  V(obs[t]) */
    float* logp;             /* [T][n]  log-likelihood of act[t] (core.py:42-46) */
    uint8_t* done;           /* [T][n]  DPENV_DONE_* bits */
    float* boot;             /* [T][n]  value appended at a path end (ppo.py:311): 0 if terminal, V(next obs) if only the
                                time limit or the end of the launch cut the path; 0 elsewhere.  Feed to dpenv_gae. */
    void* last_obs;          /* [n][obs_dim] policy input of the next launch; f32 or bf16 */
    float* last_value;       /* [n] */
    int32_t n_switch;
    int32_t switch_step[DPENV_MAX_SWITCH];
    const float* refs;       /* [n_switch][3][n] */
    int32_t sample;          /* with noise == NULL: 0 = deterministic policy a = mu (test_policy.py:90); 1 = the exploration noise is
                                drawn INSIDE the kernel like the reference's tf.random_normal (core.py:85): Philox4x32-10 +
                                Box-Muller keyed (config.seed; global env id, number of actions that env has sampled so far), so a
                                trajectory does not depend on the rank count or launch geometry and no [T][n][act_dim] noise block
                                is generated, stored or read (28 B per env-step).  Ignored when noise != NULL. */
    int32_t reset_at_end;    /* 1: the reference's epoch boundary (ppo.py:305-322, `t == local_steps_per_epoch - 1`): after step T-1
                                EVERY env is cut - boot[T-1] = V(its last observation), or 0 if it terminated at that step
                                (ppo.py:311) - and re-drawn with the training sampler (episode counter + 1, step counter 0), so the
                                next launch starts T-step-aligned fresh episodes like the reference's next epoch; last_obs /
                                last_value are those of the NEW episodes.  Needs config.auto_reset.  0: episodes continue across
                                launches (the block still ends with a bootstrap value, like a cut-off path). */
} dpenv_policy_rollout_io;
/* Requires AOS layouts.  Vessel classes, drifting current, auto-reset (with reset_acts) and bf16 observation rows all work
 * here as in dpenv_step.  Launch form and arithmetic: dpenv_policy_desc. */
int dpenv_policy_rollout(dpenv_handle h, const dpenv_policy_rollout_io* io, dpenv_stream s);

/* Parity/test access to the library-owned state in the canonical format above. */
int dpenv_get_state(dpenv_handle h, float* state_out, int32_t* counters_out, dpenv_stream s);
int dpenv_set_state(dpenv_handle h, const float* state_in, const int32_t* counters_in, dpenv_stream s);
/* The two per-env draw counters that key the streams drawn every env step: exploration noise (sample = 1 rollouts) and the
 * Gauss-Markov current drift; device uint32[n_envs] each, either pointer may be NULL.  get_state + get_current + these =
 * everything a checkpoint needs: restoring them reproduces the sampled rollouts that followed the checkpoint, bit for bit. */
int dpenv_get_rng_counters(dpenv_handle h, uint32_t* noise_ctr_out, uint32_t* drift_ctr_out, dpenv_stream s);
int dpenv_set_rng_counters(dpenv_handle h, const uint32_t* noise_ctr_in, const uint32_t* drift_ctr_in, dpenv_stream s);
/* The observation of step t carries the thrust command of step t-1 (customEnv.py:196-205 fills state_ext before :126 updates
 * prev_thrust); the state block holds the command of step t.  A closed-loop launch that CONTINUES an episode therefore starts from
 * the observation its predecessor ended with: the library keeps that observation's thrust columns (device float[n_envs][4]: o[6], o[7],
 * o[8], unused).  Every call that changes the state keeps them (round 4): dpenv_policy_rollout and dpenv_rollout leave the columns of the
 * last observation they returned, dpenv_set_state those of an observation rebuilt from the state (previous thrust / 100), dpenv_reset
 * those of the envs it re-draws (a masked reset leaves the other envs' columns alone), and dpenv_step those of the observation it returns -
 * but only while a policy is in force (16 bytes per env-step that the plain step path does not pay): after a dpenv_step WITHOUT a policy
 * the columns are stale, and a closed-loop launch that follows an upload rebuilds its first observation from the state block (its thrust
 * columns are then the command of the last step, not of the one before).  get fails with DPENV_EINVAL while they are stale; set is for
 * restoring a mid-episode checkpoint (after dpenv_set_state).  Whether a launch continues or rebuilds is decided on the host when
 * dpenv_policy_rollout is CALLED: inside a captured graph the first closed-loop launch keeps the decision made at capture time on
 * every replay (capture a graph that starts with a continuing launch after one such launch has run).  Likewise a dpenv_step RECORDED INTO A
 * GRAPH before the first policy upload has "no policy in force" baked in (it does not write the columns): re-capture step graphs after the
 * first upload if closed-loop launches are to continue from their observations. */
int dpenv_get_obs_thrust(dpenv_handle h, float* out, dpenv_stream s);
int dpenv_set_obs_thrust(dpenv_handle h, const float* in, dpenv_stream s);

/* Stateless thruster force map tau = B(alpha) F(n) (SupervisedTau.py:42-83) for n items:
 * n_pct, alpha, tau_out are device float[3][n] (bow, port, star / Fx, Fy, Mz); params host float[DPENV_NPARAM]. */
int dpenv_thrust_map(const float* params, const float* n_pct, const float* alpha, float* tau_out, int32_t n,
                     dpenv_stream s);

/* GAE-lambda over a [T][n] rollout (TrajectoryBuffer.finish_path, ppo.py:65-91, batched): a path ends
 * after step t of env i where end[t][i] != 0 and always after T-1.  Bootstrap value at a path end:
 * boot[t][i] if boot != NULL, else 0 at inner ends and last_val[i] (NULL = 0) at the final row. */
int dpenv_gae(const float* rew, const float* val, const uint8_t* end, const float* boot, const float* last_val,
              int32_t T, int32_t n, float gamma, float lam, float* adv_out, float* ret_out, dpenv_stream s);
/* The same scan, and in the same pass the statistics the normalisation needs: stats_out[0] = sum of adv, stats_out[1] = sum of
 * adv^2 over the block (device doubles; accumulated in double in a fixed order, so two runs give the same bits).  workspace:
 * dpenv_gae_workspace_bytes(n) bytes of device memory (per-workgroup partials), needed when stats_out is given.
 * A lane owns two adjacent env columns when n % 2 == 0 and the blocks are 8-byte aligned (8-byte row accesses), and rows
 * are fetched two 8-row groups ahead of the recurrence: the scan is bound by HBM (17 B per env-step, 21 B with boot). */
int64_t dpenv_gae_workspace_bytes(int32_t n);
int dpenv_gae_stats(const float* rew, const float* val, const uint8_t* end, const float* boot, const float* last_val,
                    int32_t T, int32_t n, float gamma, float lam, float* adv_out, float* ret_out, void* workspace,
                    double* stats_out, dpenv_stream s);
/* Advantage normalisation (TrajectoryBuffer.get, ppo.py:99-103 + mpi_tools.py:71-92):
 * adv = (adv - mean) / (std + 1e-8), mean and population std over ALL ranks' samples.
 * One-pass form: all-reduce (sum) the two doubles of dpenv_gae_stats and the sample count over the ranks, then
 *   dpenv_adv_apply_stats(adv, count, stats, total_count): mean = stats[0] / total_count, std = sqrt(stats[1] / total_count - mean^2).
 * Three-pass form (the reference's own order, two all-reduces): sum -> [mean = sum/count] -> sum of squared deviations ->
 * [std = sqrt(sumsq/count)] -> apply; sum_out, sumsq_out, mean, std are device float scalars.  The two reductions are
 * deterministic (double partials added in a fixed order) and share one scratch buffer per device: do not run them
 * concurrently on two streams of one device. */
int dpenv_adv_apply_stats(float* adv, int64_t count, const double* stats, double total_count, dpenv_stream s);
int dpenv_adv_sum(const float* adv, int64_t count, float* sum_out, dpenv_stream s);
int dpenv_adv_sumsq(const float* adv, int64_t count, const float* mean, float* sumsq_out, dpenv_stream s);
int dpenv_adv_apply(float* adv, int64_t count, const float* mean, const float* std, dpenv_stream s);

/* ---- the deployed controller: the trained actor plus the ROS node's body-frame integral action ---------------------------------
 * (rl_allocator.py:252-273 of the reference).  While it is on, the closed-loop launches apply it once per env step to the pose-error
 * components e = obs[0:3] as the env forms them (make_obs, whatever wrap_mode the handle uses), with two per-env items of state, the
 * integrator value I[3] and an int32 count c of control steps since the last (re)arrival, in this f32 order:
 *     outside = |e0| > box0 || |e1| > box1 || |e2| > box2        (strict >: an error of exactly box is inside, as in the node)
 *     if outside: I = 0, c = 0
 *     else:       c = min(c + 1, D); if c >= D: I_j = fminf(fmaxf(I_j + step_s * (gain_j * e_j), -bound_j), bound_j)
 *     policy input o[0:3] = e + I                                 (o[3:] unchanged)
 * D is the smallest integer with D * dt > dwell_s (dt = n_substeps * substep_dt, computed in f64): the node's (now - time_arrival) > dwell
 * test in control steps.  The update happens when the observation after a step is formed - a step that ends an episode updates on its
 * last observation (what V of that observation, the bootstrap value, sees) and the reset then zeroes I and c: a new episode's first
 * observation carries I = 0.  A launch's first policy input is rebuilt from the stored state and the stored I with NO update, so two
 * launches of T/2 write the rows of one launch of T.  Reward, termination and the plant see the true state; only the policy input changes
 * (the obs rows, last_obs, and the observations val and boot are computed from).
 * Every reset zeroes I and c: dpenv_reset (for the envs it re-draws), auto-reset and reset_at_end.
 * Supported: final variant with continuous angles (every arithmetic and launch form; shared hull, classes, per-env hulls, randomisation,
 * the thrust-loss preset, randomised and drifting current, auto-reset, reset_at_end), limited and full variants (one-wave form); all with
 * extended_state and a leaky-relu / relu network of hidden width <= 80.  Anything else: DPENV_EINVAL, with the set named.
 * While it is on, dpenv_step, dpenv_step_ex and dpenv_rollout return DPENV_EINVAL (their observations would lack I): an eager deployment
 * composes dpenv_step with the law on the host (ml4ca_amd.deploy.BatchedBodyFrameIntegrator). */
typedef struct dpenv_integral_action {
    uint32_t struct_size;
    float gain[3];           /* (0.05, 0.05, 0.05) in the node */
    float bound[3];          /* |I_j| <= bound_j: (0.5 m, 1.0 m, pi / 32) */
    float box[3];            /* |e_j| > box_j on any axis resets I and c: (5 m, 5 m, 140 deg in rad) */
    float dwell_s;           /* 5.0 s: I integrates once c * dt > dwell_s */
    float step_s;            /* integration step; <= 0 = the control period n_substeps * substep_dt */
} dpenv_integral_action;
/* ia = NULL turns the action off (the closed loop runs its original kernels again).  Turning it on zeroes I and c of every env.  Refused:
 * NaN, negative bounds or box, a negative dwell, and the simple variant (the node refuses it too, rl_allocator.py:126). */
int dpenv_set_integral_action(dpenv_handle h, const dpenv_integral_action* ia, dpenv_stream s);
/* The checkpoint path of the action's state, next to dpenv_get_state / dpenv_get_rng_counters: I_out / I_in device float[3][n_envs],
 * count device int32[n_envs]; either pointer may be NULL.  DPENV_EINVAL while the action is off.  The library produces counts in
 * [0, D] only; count_in is copied as it is (a device block: nothing is read back to check it), and the law's c = min(c + 1, D) then
 * does this: a count above D acts as D from the next update on; a negative count -k waits k updates longer before I integrates (the
 * dwell is D + k); I_in is taken as it is and clipped to the bound at the next integrating update.  count_in must not be INT32_MAX:
 * c + 1 would overflow, which C leaves undefined.  tests/test_gpu_control_edges.py pins -3, D + 1, 1000 and INT32_MAX - 1. */
int dpenv_get_integral_state(dpenv_handle h, float* I_out, int32_t* count_out, dpenv_stream s);
int dpenv_set_integral_state(dpenv_handle h, const float* I_in, const int32_t* count_in, dpenv_stream s);
/* dpenv_policy_rollout with the action on (required), plus integ_out: device float[T][n][3], the I added to obs[t] (NULL = not written),
 * so that obs[t][0:3] - integ_out[t] is the true error.  Plain dpenv_policy_rollout applies the action as well while it is on. */
int dpenv_policy_rollout_integral(dpenv_handle h, const dpenv_policy_rollout_io* io, float* integ_out, dpenv_stream s);

/* ---- the setpoint reference filter of the deployed controller (additive to ABI 6) ----------------------------------------------------
 * The RL node never saw raw setpoint steps: it took its reference from the smoothing filter between the operator's setpoint and the
 * policy (reference_filter/state_desired, rl_allocator.py:160,187-195 of the reference), and the thesis scores IAE against that filtered
 * reference (box_test/plot_pos.py:31,174).  The law, per env and per axis j in {N, E, psi}, is the linear third-order reference model
 * (Fossen 2011) with no rate limits:
 *     x''' + (2 zeta_j + 1) omega_j x'' + (2 zeta_j + 1) omega_j^2 x' + omega_j^3 x = omega_j^3 r_j
 * State per env: x_j = (pos, vel, acc) and the target r_j, 12 floats; heading in rad, unwrapped.  Discretisation: exact zero-order hold
 * over the control period dt = n_substeps * substep_dt (f32, as the integral action's step):  x_j <- Phi_j x_j + Gamma_j r_j, with Phi_j
 * (3x3) and Gamma_j (3x1) computed on the host in f64 from (omega_j, zeta_j, dt) - the matrix exponential of the 4x4 augmented system
 * [[A_j, B_j], [0, 0]] dt, by scaling and squaring of its degree-18 Taylor polynomial - and rounded to f32 (dpenv_reference_filter_coeffs
 * returns them).  Each row m of the update is, in f32 (the build has -ffp-contract=off):
 *     x'_m = ((Phi[m][0] * pos + Phi[m][1] * vel) + Phi[m][2] * acc) + Gamma[m] * r
 * Per control step t of the closed loop, while the filter is on:
 *   1. a switch of the schedule (io->switch_step / io->refs) that falls on step t sets the target instead of the env's reference;
 *      heading is taken the short way: r_psi = psi_d + wrapf(r_new - psi_d), wrapf(d) = d - 2pi_f * rintf(d * (1 / 2pi)_f);
 *   2. the filter advances one dt;
 *   3. its position eta_d = (N_d, E_d, psi_d) is that step's new_ref (has_ref), visible from the next step (Q4) as always.
 * The fused launch therefore equals the eager composition env.step(a_t, new_ref = F.advance()), row for row: observation, reward,
 * termination and the integral action all see eta_d.  One difference in the state a launch leaves: the new_ref of its LAST step stays
 * pending in the filter's position, and the env's stored reference is the one its last observation was formed against; the next launch
 * puts the filter's position in force before its first step (so two launches of T/2 write the rows of one launch of T).  An env re-drawn
 * at the last step takes the pending reference, as in the eager composition.  Every reset puts the filter at rest on the env's new reference (pos = ref, vel = acc = 0, r = ref):
 * dpenv_reset (for the envs it re-draws), auto-reset, reset_at_end, and turning the filter on (every env).
 * Defaults (what ml4ca_amd uses): omega = (0.619, 0.619, 1.51) rad/s, zeta = (1, 1, 1) - the least-squares fit to the recorded filter
 * output (tools/gen_golden_reffilter.py, tests/golden/reference_filter.npz).
 * Supported: the integral action's set (above), with or without the integral action - the final variant with continuous angles in every
 * arithmetic and launch form, limited and full (one-wave form); extended_state; a leaky-relu / relu network of hidden width <= 80.  Anything
 * else: DPENV_EINVAL with the set named.  While it is on, dpenv_step, dpenv_step_ex and dpenv_rollout return DPENV_EINVAL: an eager user
 * composes dpenv_step with the filter on the host (ml4ca_amd.deploy.BatchedReferenceFilter) and passes its position as new_ref. */
typedef struct dpenv_reference_filter {
    uint32_t struct_size;
    float omega[3];          /* natural frequency per axis N, E, psi [rad/s], > 0 */
    float zeta[3];           /* relative damping per axis, > 0 */
} dpenv_reference_filter;
/* rf = NULL turns the filter off (the closed loop runs its existing kernels again).  Turning it on puts every env's filter at rest on its
 * reference.  Refused: NaN or non-finite values, omega <= 0, zeta <= 0, and a variant / state outside the supported set. */
int dpenv_set_reference_filter(dpenv_handle h, const dpenv_reference_filter* rf, dpenv_stream s);
/* The checkpoint path of the filter: x device float[9][n_envs], row 3 k + j = (pos, vel, acc)[k] of axis (N, E, psi)[j]; r device
 * float[3][n_envs], the targets.  Either pointer may be NULL.  DPENV_EINVAL while the filter is off. */
int dpenv_get_reference_filter_state(dpenv_handle h, float* x_out, float* r_out, dpenv_stream s);
int dpenv_set_reference_filter_state(dpenv_handle h, const float* x_in, const float* r_in, dpenv_stream s);
/* Pure host function: the f32 coefficients the kernels use for control period dt: phi_out[j] = Phi_j row-major, gam_out[j] = Gamma_j.
 * No upper limit is put on omega.  Each coefficient is within 2^-24 |c| + a of the exact matrix exponential, a the f64 recipe's own
 * absolute error (tests/control_edges.py measures it against 60 digits: below 3e-14 for omega <= 1.51, 2e-12 at omega = 10, 2e-9 at
 * omega = 50 with zeta = 1e-3, dt = 0.2).  From omega dt of about 40 on, the entries that decay like exp(-omega dt) are smaller than a:
 * they carry an absolute meaning only, and only that form is tested there. */
int dpenv_reference_filter_coeffs(const dpenv_reference_filter* rf, float dt, float phi_out[3][9], float gam_out[3][3]);
/* dpenv_policy_rollout with the filter on (required), plus ref_out: device float[T][n][3], the eta_d that obs[t] was formed against (the
 * env's reference when obs[t] was formed), and integ_out as in dpenv_policy_rollout_integral (needs the integral action on).  Either may
 * be NULL.  Plain dpenv_policy_rollout / dpenv_policy_rollout_integral apply the filter as well while it is on. */
int dpenv_policy_rollout_deployed(dpenv_handle h, const dpenv_policy_rollout_io* io, float* ref_out, float* integ_out, dpenv_stream s);

/* ---- streaming score card: box-test IAE, thruster work and returns accumulated on the device (additive to ABI 6) -----------------------
 * evaluate.iae / evaluate.work / deployment_box_test need every row of a flight resident (105 B per env-step with the integral action and
 * the filter on: 8.6 GB for a 250 s box test of 65 536 envs).  Closed-loop launches continue one another bit for bit, so a flight can be
 * flown in short chunks through ONE re-used set of row blocks; these calls consume each chunk and carry the trapezoid across chunk and
 * episode boundaries: O(n) memory, and per-episode return / length (spinup's EpRet / EpLen) for runs that auto-reset.  Handle-free, like
 * dpenv_gae: every bulk pointer is a device pointer, the io struct is host memory, calls are stream-ordered and graph-capturable.
 *
 * State.  One opaque state per env, caller-owned, dpenv_score_state_bytes(n) bytes, 16-byte aligned.  All-zero bytes mean "fresh": the
 * caller resets it with a memset (no allocation, no host sync, stream-ordered and capturable).  It holds, per env: an OPEN episode - sums
 * iae, work[3], ret in f64; len as a count; the previous sample (q_prev, P_prev[3]) in f32; a has_prev flag - and CLOSED-episode totals -
 * episodes as a count; sums of iae, work[3], ret in f64; the sum of len.
 *
 * Per-row update.  One call consumes a block of T rows, in order t = 0 ... T-1, for every env i.  Per-sample terms are f32 in exactly
 * this order (the build uses -ffp-contract=off; sqrt is the hardware's correctly rounded one):
 *     e_k  = f32(obs[t][i][k]) - (integ ? integ[t][i][k] : 0)          k = 0,1,2   (bf16 obs widened first)
 *     q    = sqrtf( (e_0/norm_0)^2 + (e_1/norm_1)^2 + ((e_2*R2D)/norm_2)^2 )          R2D = (float)(180/pi), sum left to right
 *     n_j  = fminf(fmaxf(act[t][i][j]*100, -100), 100)                 j = 0,1,2   (evaluate.commanded_thrust)
 *     x_j  = n_j/100 * rps_j ;   P_j = sgn(n_j) * c_j * (x_j*x_j*x_j)              (evaluate.thruster_power)
 *     if has_prev:  iae += (double)(0.5f*(q + q_prev)*dt) ;  work_j += (double)(0.5f*(P_j + P_prev_j)*dt)
 *     ret += (double)rew[t][i] ;  len += 1 ;  (q_prev, P_prev) = (q, P) ;  has_prev = 1
 *     if done[t][i] != 0  or  (cut_at_end and t == T-1):
 *           closed += open ; episodes += 1 ; open = 0 ; has_prev = 0
 * The first sample of an episode contributes no segment (like the reference's integrals[0] = 0, common.py:60-74); the trapezoid never
 * bridges an episode end; ANY non-zero done byte ends the episode (the rule dpenv_gae's `end` uses); cut_at_end serves reset_at_end
 * launches, whose cut envs may carry done[T-1] == 0.
 *
 * Inputs: row-major [T][n][stride] blocks, as dpenv_policy_rollout* and the AOS form of dpenv_rollout write them ([dim][n] layouts are not
 * supported: there is no way to ask for them).  obs: f32 or bf16, obs_stride >= 3 elements, only columns 0..2 are read (the pose error).
 * act: f32, act_stride >= 3, only columns 0..2 are read - the three thrust commands, which is what evaluate.commanded_thrust assumes of
 * every variant's action vector.  rew: [T][n] f32.  done: [T][n] u8, NULL = never ends.  integ: [T][n][3] f32 (dpenv_policy_rollout_integral's
 * integ_out) or NULL; needs obs.  Any of obs / act / rew may be NULL: the sums it feeds then stay untouched (len and episodes always count).
 * Everything is validated on the host before any device call: DPENV_EINVAL, the field named by dpenv_last_error(NULL). */
enum { DPENV_SCORE_IAE = 0, DPENV_SCORE_WORK = 1 /* 1..3: bow, port, star */, DPENV_SCORE_RET = 4, DPENV_SCORE_LEN = 5,   /* the open episode */
       DPENV_SCORE_EPISODES = 6, DPENV_SCORE_EP_IAE = 7, DPENV_SCORE_EP_WORK = 8 /* 8..10 */, DPENV_SCORE_EP_RET = 11,
       DPENV_SCORE_EP_LEN = 12,                                                                                         /* closed episodes, summed */
       DPENV_SCORE_NOUT = 13 };
typedef struct dpenv_score_io {
    uint32_t struct_size;    /* sizeof(dpenv_score_io), ABI check */
    int32_t T;               /* rows in this block, >= 1 */
    int32_t n;               /* envs, >= 1 */
    const void* obs;         /* [T][n][obs_stride] f32 / bf16, or NULL */
    const float* act;        /* [T][n][act_stride], or NULL */
    const float* rew;        /* [T][n], or NULL */
    const uint8_t* done;     /* [T][n], or NULL = never ends */
    const float* integ;      /* [T][n][3], or NULL; needs obs */
    int32_t obs_dtype;       /* DPENV_F32 / DPENV_BF16 */
    int32_t obs_stride;      /* elements per obs row, >= 3 (default 9) */
    int32_t act_stride;      /* floats per act row, >= 3 (default 7) */
    float dt;                /* sample period [s], 0.2 */
    float norm[3];           /* IAE normalisation (5 m, 5 m, 25 deg), box_test/plot_pos.py:174 */
    float power_coeff[3];    /* c_j = (float)(KQ0_j * 2 pi * 1025 * D_j^5): KQ0 0.02 / 0.036 / 0.036, D 0.06 / 0.15 / 0.15 (plot_act.py:124-135), computed in double, rounded once */
    float rps_max[3];        /* (33, 11, 11) revolutions per second at 100 % */
    int32_t cut_at_end;      /* 1: every env's episode is closed after row T-1 */
} dpenv_score_io;
int64_t dpenv_score_state_bytes(int32_t n);          /* 0 for n < 1 */
/* Fill *io with the constants above; T, n and the block pointers are left 0 / NULL. */
int dpenv_score_default_io(dpenv_score_io* io);
int dpenv_score_accumulate(void* state, const dpenv_score_io* io, dpenv_stream s);
/* out: device double[DPENV_SCORE_NOUT][n], slot DPENV_SCORE_* of every env (counts as doubles). */
int dpenv_score_read(const void* state, int32_t n, double* out, dpenv_stream s);
/* out: device double[DPENV_SCORE_NOUT][3] = sum, min, max over the envs of each read slot.  Two stages with a fixed pairing (a wave per 64
 * envs, then one workgroup over the partials in index order): the sums are the same bits every run.  workspace:
 * dpenv_score_summary_workspace_bytes(n) bytes of device memory. */
int64_t dpenv_score_summary_workspace_bytes(int32_t n);
int dpenv_score_summary(const void* state, int32_t n, double* out, void* workspace, dpenv_stream s);

/* ---- the score card's wear axis: IADC, the integral absolute derivative of the commands (additive to ABI 6) -----------------------------
 * The thesis' third axis beside IAE and W* (results/all_plots/box_test/plot_act.py:320-391): how much the thrust and azimuth commands
 * move.  dpenv_score_accumulate_wear is dpenv_score_accumulate - the score state ends up the same, bit for bit - with a second
 * caller-owned state beside it, in ONE pass over the rows: a scored flight reads its act rows once.
 *
 * The commands.  Per env i and row t, the commands the env itself decodes from the action row:
 *     n_j, j = bow, port, star, in percent:  fminf(fmaxf(act[t][i][j]*100, -100), 100)                  (the score card's own expression)
 *     alpha_k, k = port, star, in radians:  the variant's command decode (customEnv.py:104-122, 215-244; the step kernels' own function):
 *         FULL                    act[4], act[5] times pi_f, clipped to +-pi_f                           (pi_f = (float)pi)
 *         LIMITED                 act[3], act[4] times pi_f/2, clipped to +-pi_f/2
 *         FINAL without cont_ang  w = a - 2 floorf((a + 1) * 0.5f) for a = act[3], act[4]; w * pi_f, clipped to +-pi_f     (the wrap form)
 *         FINAL with cont_ang     atan2(act[3], act[4]), atan2(act[5], act[6]), clipped to +-pi_f; atan2 is the kernels' own, max abs
 *                                 error 2.6e-7, signed zeros kept ((+-0, -x) gives +-pi)
 *         SIMPLE                  commands no azimuth: alpha_k = 0, its angle term is 0
 *     The bow azimuth is not counted, as in the reference (plot_act.py:334, "no action from the angle of the bow thruster").
 *
 * Per-row update.  With a previous sample (n', alpha') of the same episode, in f32, in exactly this order (the build has -ffp-contract=off;
 * / is correctly rounded):
 *     d_n = ((|n_0 - n_0'| + |n_1 - n_1'|) + |n_2 - n_2'|) / 100
 *     w_k = fminf(|alpha_k - alpha_k'|, 2pi_f - |alpha_k - alpha_k'|)      (2pi_f = 2 * (float)pi; both angles are clipped to +-pi_f, so w_k >= 0)
 *     d_a = (w_1 + w_2) / pi_f
 *     iadc_rps += (double)d_n ;  iadc_angle += (double)d_a
 * then (n', alpha') = (n, alpha), has_prev = 1, and behind a row that ends the episode (dpenv_score_accumulate's rule: any non-zero done
 * byte, or cut_at_end on row T-1) closed += open, open = 0, has_prev = 0.  IADC = iadc_rps + iadc_angle, added in f64 at read time.
 * The first sample of an episode contributes nothing - the reset's own command is not a previous sample - and nothing bridges an episode
 * end.  On the env's uniform grid the reference's (|delta|/dt/scale)*dt is |delta|/scale: the law has no dt.  The reference's per-interval
 * clip to [0, 400] (plot_act.py:385) cannot act - an interval is at most 3*2 + 2*1 = 8 - and is not built; its re-use of the previous entry
 * for intervals under 0.1 s (:336-339, :358-363) never fires on a 0.2 s grid and lives in the host's series function only
 * (evaluate.iadc_series).
 *
 * Non-finite actions.  The law is stated for finite actions.  fmaxf / fminf return their other operand when one is NaN, so every clip above
 * returns a bound for a NaN: a NaN thrust entry reads as -100 %, +-Inf as +-100 %; a NaN or Inf azimuth entry (or head: atan2 of a NaN or
 * of two infinities is a NaN or some finite angle) reads as some angle within the clip, -pi_f (-pi_f/2 for LIMITED) where the decode's
 * result is a NaN.  The commands, and so both sums, stay finite whatever the row holds; lanes never read one another's rows, so a
 * non-finite row changes nothing of any other env.
 *
 * Wear state.  One per env, caller-owned, dpenv_score_wear_state_bytes(n) bytes (64 per env; 0 for n < 1), 16-byte aligned, all-zero bytes
 * = fresh (a memset resets it, like the score state): open and closed iadc_rps / iadc_angle in f64, the previous n[3] and alpha[2] in f32,
 * and a has_prev flag of its own - a fresh wear state joined to a score state in mid-episode counts nothing for its first row instead of
 * differencing against zeros.  dpenv_score_state_bytes and the 128-byte score state are what they were. */
enum { DPENV_SCORE_WEAR_RPS = 0, DPENV_SCORE_WEAR_ANGLE = 1,             /* the open episode */
       DPENV_SCORE_WEAR_EP_RPS = 2, DPENV_SCORE_WEAR_EP_ANGLE = 3,       /* closed episodes, summed */
       DPENV_SCORE_WEAR_NOUT = 4 };
typedef struct dpenv_score_wear_io {
    uint32_t struct_size;    /* sizeof(dpenv_score_wear_io), ABI check */
    int32_t variant;         /* DPENV_FULL .. DPENV_FINAL: whose command decode the azimuths take */
    int32_t cont_ang;        /* FINAL only: the rows carry sin / cos heads (7 columns) */
} dpenv_score_wear_io;
int64_t dpenv_score_wear_state_bytes(int32_t n);     /* 0 for n < 1 */
/* One pass over the block: the score state as dpenv_score_accumulate leaves it, the wear state by the law above.  Refused on the host,
 * before any device call, with the field named: everything dpenv_score_accumulate refuses; wear NULL or not 16-byte aligned; wio NULL or
 * of another struct_size; a variant outside the enum; cont_ang on a variant other than FINAL; io->act NULL; io->act_stride below the
 * variant's dpenv_act_dim (6 / 3 / 5 / 5, 7 with cont_ang). */
int dpenv_score_accumulate_wear(void* state, void* wear, const dpenv_score_io* io, const dpenv_score_wear_io* wio, dpenv_stream s);
/* out: device double[DPENV_SCORE_WEAR_NOUT][n], slot DPENV_SCORE_WEAR_* of every env. */
int dpenv_score_wear_read(const void* wear, int32_t n, double* out, dpenv_stream s);
/* out: device double[DPENV_SCORE_WEAR_NOUT][3] = sum, min, max over the envs of each wear slot, with dpenv_score_summary's fixed two-stage
 * pairing.  workspace: dpenv_score_wear_summary_workspace_bytes(n) bytes of device memory. */
int64_t dpenv_score_wear_summary_workspace_bytes(int32_t n);
int dpenv_score_wear_summary(const void* wear, int32_t n, double* out, void* workspace, dpenv_stream s);

/* ---- the classical baseline in the closed loop: a PID motion controller feeding a pseudo-inverse thrust allocation (additive to ABI 6) --
 * The thesis compares the RL allocator with the classical chain; the reference tree has neither its PID nor its pseudo-inverse node, so the
 * law is build-defined, like the plant.  While it is on, dpenv_controller_rollout flies it per env and per control step on the observation
 * o as the env forms it (make_obs, whatever wrap_mode the handle uses): e = o[0:3] the body-frame pose error, nu = o[3:6].  State per env:
 * z[3], the error integral.  In f32, in exactly this order (the build has -ffp-contract=off; sqrtf and / are correctly rounded):
 *     z_j   = fminf(fmaxf(z_j + dt * e_j, -z_bound_j), z_bound_j)                    j = 0,1,2   (dt = n_substeps * substep_dt in f32)
 *     tau_j = -((kp_j * e_j + kd_j * nu_j) + ki_j * z_j);   tau_j = fminf(fmaxf(tau_j, -tau_max_j), tau_max_j)
 *     f_m   = (G[m][0] * tau_0 + G[m][1] * tau_1) + G[m][2] * tau_2                  m = 0..4: Fy_bow, Fx_port, Fy_port, Fx_star, Fy_star
 *     bow:      Kb = f_0 >= 0 ? kf[0] : kr_bow;   n_b = copysignf(sqrtf(fabsf(f_0) / Kb), f_0)
 *     stern i:  F = sqrtf(Fx * Fx + Fy * Fy);     n_i = sqrtf(F / kf[i])             (port: m = 1, 2, kf[1]; star: m = 3, 4, kf[2])
 *               (sin_i, cos_i) = F > f_eps ? (Fy / F, Fx / F) : (0, 1)
 *     action = [ fminf(fmaxf(n_b / 100, -1), 1), fminf(n_port / 100, 1), fminf(n_star / 100, 1), sin_port, cos_port, sin_star, cos_star ]
 * - the final variant's continuous-angle action (customEnv.py:227-235): the bow tunnel thruster fixed at pi / 2, the stern pods free with
 * thrust >= 0; a saturated command is not redistributed.  G is the weighted pseudo-inverse W^-1 T' (T W^-1 T')^-1 of the extended-thrust
 * matrix T = [[0, 1, 0, 1, 0], [1, 0, 1, 0, 1], [lx_bow, -ly_port, lx_port, -ly_star, lx_star]], W = diag(weight), computed in f64 and
 * rounded once to f32 (dpenv_dp_allocation_matrix) - from the controller's NOMINAL lever arms: a randomised hull is flown by a controller
 * that does not know it (dpenv_set_dp_controller_table below gives every env its own numbers, lever arms included).  z is zeroed by every reset: dpenv_reset (for the envs it re-draws), auto-reset (an env that ends an episode has
 * z = 0 before its new episode's first action) and turning the controller on (every env).  A launch's first input is rebuilt from the stored
 * state, its thrust columns continued as dpenv_policy_rollout's, and z is updated at every action: two launches of T/2 write the rows of
 * one launch of T.
 * Supported: the final variant with continuous angles and extended_state, AOS rows, f32 or bf16 obs rows (the law sees the f32 observation);
 * the shared hull, the thrust-loss preset, per-env hulls and their randomisation, constant, drifting and per-episode currents, auto-reset,
 * with or without the reference filter.  Vessel classes (n_classes > 1), any other variant and a handle with the integral action on:
 * DPENV_EINVAL with the set named.  The controller is a launch form, not a mode: dpenv_step, dpenv_rollout and dpenv_policy_rollout keep
 * working while it is on (they leave z alone).  ml4ca_amd.deploy.BatchedDPController is the host statement of the law.
 * AT THE EDGES of the numbers (tests/control_edges.py flies them).  The allocation's domain: every f_m finite and, per stern pod,
 * Fx Fx + Fy Fy inside f32's normal range or exactly 0 - |f| below about 1.3e19 and, unless both components are 0, above 2^-63 = 1.1e-19.
 * Inside it the action is the float64 law's to a few roundings (the bounds are derived in tests/control_edges.py).  Outside it the law
 * is the f32 text above and nothing more: from |f| = 1.3e19 on the sum of squares overflows, F = inf, n_i saturates at 1 and the heads
 * are (+-0, +-0) - not a unit vector - or NaN where a component is itself inf; below 2^-63 the squares round as subnormals and from
 * 2^-75 = 2.6e-23 down to 0, F = 0 and the heads are (0, 1) whatever f_eps is (with f_eps = 0 a force that small keeps the direction
 * ahead).  At tau = 0 and f_eps = 0, F = 0 is not > f_eps: the heads are (0, 1), never 0 / 0.  tau_max_j = +inf is accepted (only NaN
 * and negative bounds are refused): that axis is not clipped, and dpenv_thrust_alloc takes any tau, so the domain is the caller's to
 * keep.  Every clip is fminf(fmaxf(v, -b), b), which DROPS a NaN: an observation with a NaN in e_j gives z_j = -z_bound_j and
 * tau_j = -tau_max_j on that row, a NaN in nu_j gives tau_j = -tau_max_j and leaves z_j alone, and the rows behind it are finite again;
 * a NaN wrench handed to the allocation commands [-1, 1, 1, 0, 1, 0, 1].  e_j = +-inf puts z_j on +-z_bound_j and, for kp_j > 0, tau_j
 * on -+tau_max_j (kp_j < 0: the other sign; kp_j = 0: 0 * inf is NaN and tau_j = -tau_max_j).  The integral action's counts outside
 * [0, D] and the reference filter's omega are treated at dpenv_set_integral_state and dpenv_reference_filter_coeffs.
 * No row of the law's own flights is non-finite; these are the answers for rows some other flight wrote.  With a bound of exactly 0
 * the clip returns a zero whose sign is not defined (fminf and fmaxf may return either of two equal zeros): z_j and tau_j are 0 in value.
 * The host statement clips with fmin / fmax in the same nesting and agrees with the device on all of this bit for bit, such a zero's
 * sign apart. */
typedef struct dpenv_dp_controller {
    uint32_t struct_size;
    float kp[3], kd[3], ki[3];   /* finite */
    float z_bound[3];            /* |z_j| <= z_bound_j, >= 0 */
    float tau_max[3];            /* |tau_j| <= tau_max_j, >= 0: (69 N, 30 N, 80 Nm) in SupervisedTau.py:37 */
    float G[5][3];               /* dpenv_dp_allocation_matrix of the nominal lever arms, finite */
    float kf[3];                 /* thrust constants ahead: bow, port, star, > 0 */
    float kr_bow;                /* bow astern, > 0 */
    float f_eps;                 /* a stern force at or below it keeps the direction (sin, cos) = (0, 1); >= 0 [N] */
} dpenv_dp_controller;
/* Pure host function, f64 inside: lx, ly the lever arms of bow, port, star [m] (ly[0] is not used: the tunnel thruster pushes sideways
 * only); weight[5] > 0 per column of T.  DPENV_EINVAL if T W^-1 T' is singular. */
int dpenv_dp_allocation_matrix(const float lx[3], const float ly[3], const float weight[5], float G_out[5][3]);
/* c = NULL turns the controller off.  Turning it on zeroes z of every env.  Refused, before any state changes: NaN or non-finite gains and
 * G, NaN or negative bounds and f_eps, kf <= 0, kr_bow <= 0, and a handle outside the supported set. */
int dpenv_set_dp_controller(dpenv_handle h, const dpenv_dp_controller* c, dpenv_stream s);
/* The checkpoint path of z, next to dpenv_get_state: device float[3][n_envs].  DPENV_EINVAL while the controller is off. */
int dpenv_get_dp_controller_state(dpenv_handle h, float* z_out, dpenv_stream s);
int dpenv_set_dp_controller_state(dpenv_handle h, const float* z_in, dpenv_stream s);

/* Per-env numbers for the law (additive to ABI 6): one controller per env, for a gain sweep in one launch or a baseline that knows each
 * env's hull.  The public table is a DEVICE float[DPENV_CTRL_NPARAM][n_envs], laid out like the vessel table (row p = slot p of every env);
 * the caller owns it.  Slots: */
#define DPENV_CTRL_NPARAM 32
#define DPENV_CTRL_KP 0       /* 0-2  kp, finite */
#define DPENV_CTRL_KD 3       /* 3-5  kd, finite */
#define DPENV_CTRL_KI 6       /* 6-8  ki, finite */
#define DPENV_CTRL_ZB 9       /* 9-11 z_bound, >= 0 */
#define DPENV_CTRL_TMAX 12    /* 12-14 tau_max, >= 0 */
#define DPENV_CTRL_WEIGHT 15  /* 15-19 the five allocation weights (columns of T), finite and > 0 */
#define DPENV_CTRL_LX 20      /* 20-22 lever arms lx: bow, port, star, finite */
#define DPENV_CTRL_LY 23      /* 23-25 lever arms ly: bow (not used by T), port, star, finite */
#define DPENV_CTRL_KF 26      /* 26-28 thrust constants ahead: bow, port, star, finite and > 0 */
#define DPENV_CTRL_KR_BOW 29  /* bow astern, finite and > 0 */
#define DPENV_CTRL_F_EPS 30   /* direction threshold, >= 0 */
                              /* 31 reserved, 0 */
/* The call needs the controller on (dpenv_set_dp_controller first: it supplies dt, the z block and the supported-set check), else
 * DPENV_EINVAL.  A packing kernel, one lane per env, computes every env's G from its lever arms and weights with the recipe and the
 * operation order of dpenv_dp_allocation_matrix (V = W^-1 T', M = T V with the sums started at 0.0 in index order, the adjugate,
 * det = (M00 adj00 + M01 adj10) + M02 adj20, G = V adj / det), in f64, rounded once to f32, and writes the env's 36 numbers into a
 * library-owned block (allocated by the first call, released with the handle): every later call is stream-ordered without allocation and
 * graph-capturable, and a captured launch flies whatever the last packing wrote.
 * Refused rows: a row is refused if it breaks any condition dpenv_set_dp_controller refuses (non-finite gains, NaN or negative bounds and
 * f_eps, kf <= 0, kr_bow <= 0), has a weight <= 0 or non-finite, a non-finite lever arm, a det that is non-finite or zero, or a non-finite
 * G.  A refused row is packed as the ZERO CONTROLLER - gains, bounds and G all 0, kf = kr_bow = 1, f_eps = 0 - with which the law commands
 * the action [0, 0, 0, 0, 1, 0, 1] at every step, whatever the observation holds, non-finite entries included (equal in VALUE: the
 * law forms tau = -(0 + 0), so n_bow may be -0.0); the other rows are not affected.  refused_out: NULL, or a device uint8[n_envs] that
 * gets 1 for a refused env and 0 for the others.  The library reads nothing back, does not synchronise and uses no atomics: the caller
 * decides whether to look.
 * While a table is in force dpenv_controller_rollout flies row i on env i: the law above, read with per-env operands (dt stays the
 * handle's).  Rows, resets, the reference filter, currents and hull sources are what they are without it.  The call leaves z alone: gains can
 * change between the launches of one flight, and a checkpoint restores as table + dpenv_set_dp_controller_state.  table = NULL returns to
 * the numbers of dpenv_set_dp_controller; dpenv_set_dp_controller(h, c) with c != NULL installs that scalar law again and drops the
 * table, NULL turns everything off.  dpenv_thrust_alloc takes no table. */
int dpenv_set_dp_controller_table(dpenv_handle h, const float* table, uint8_t* refused_out, dpenv_stream s);

typedef struct dpenv_controller_rollout_io {
    uint32_t struct_size;    /* sizeof(dpenv_controller_rollout_io), ABI check */
    int32_t T;
    void* obs;               /* [T][n][9]  the controller's input at step t; f32 or bf16 */
    float* act;              /* [T][n][7]  its action */
    float* reward;           /* [T][n] */
    uint8_t* done;           /* [T][n]  DPENV_DONE_* bits */
    void* last_obs;          /* [n][9]  the controller's input of the next launch */
    float* ref_out;          /* [T][n][3] the eta_d obs[t] was formed against, or NULL; needs the reference filter on */
    int32_t n_switch;
    int32_t switch_step[DPENV_MAX_SWITCH];
    const float* refs;       /* [n_switch][3][n] */
} dpenv_controller_rollout_io;
/* T steps of (law -> env.step) in one launch: the row conventions of dpenv_policy_rollout, so dpenv_score_accumulate consumes the blocks
 * unchanged.  With the reference filter on (dpenv_set_reference_filter) the switches set its targets and every step's new_ref is its
 * position, exactly as in dpenv_policy_rollout_deployed.  Stream-ordered, no allocation and no host synchronisation: graph-capturable. */
int dpenv_controller_rollout(dpenv_handle h, const dpenv_controller_rollout_io* io, dpenv_stream s);
/* The law on rows some other flight wrote (additive to ABI 6): expert labels for the states an actor visited (DAgger-style relabelling),
 * or the baseline's answer beside an actor's on the same states.  A forward scan in one launch, one lane per env; per row t and env i
 *     act[t][i][0:7] = the law above on o = obs[t][i][0:6] with the env's z_i (z_i is advanced first, exactly as in the closed loop)
 *     if (done && done[t][i] != 0) z_i = 0                         -- the next row is a new episode's first
 * z_i starts from z_in[:, i] (NULL = 0) and is written to z_out[:, i] at the end (NULL = not wanted; z_out may be z_in), so a block
 * labelled in pieces with z handed over gives the rows of one call.  The numbers are the handle's controller in force: the table of
 * dpenv_set_dp_controller_table when there is one (row i on env i), else dpenv_set_dp_controller's; dt is the handle's.  obs rows are
 * f32 or bf16 as obs_dtype says, whatever the handle's config says; a bf16 value is widened exactly and the law runs in f32.  The thrust
 * columns obs[..][6:9] are not read.
 * For f32 rows written by dpenv_controller_rollout with auto-reset on, labelled with that launch's done block, the z the launch started
 * from and the same controller, the labels are that launch's act rows bit for bit and z_out is its final z.  (Without auto-reset the
 * closed loop keeps z across a done row; pass done = NULL to label such a block.)
 * The call reads and writes nothing of the handle's env state, its own z, the lagged thrust columns or the RNG counters: a labelled block
 * changes no later row of any launch.  Stream-ordered, no allocation, no host synchronisation; one kernel node when captured into a
 * graph (a captured call flies whatever table the last packing wrote; the scalar numbers are those at capture).
 * DPENV_EINVAL with the reason in dpenv_last_error, before anything is launched or written: the controller off, a wrong struct_size,
 * T <= 0, NULL obs or act, an obs_dtype that is neither DPENV_F32 nor DPENV_BF16.  ml4ca_amd.deploy.label_rows is the host statement.
 * The labels are always the pseudo-inverse law's, also while dpenv_set_qp_allocator has the QP allocation in the closed loop. */
typedef struct dpenv_controller_label_io {
    uint32_t struct_size;    /* sizeof(dpenv_controller_label_io), ABI check */
    int32_t T;
    const void* obs;         /* [T][n][9] rows in dpenv_policy_rollout's conventions; f32 or bf16 */
    int32_t obs_dtype;       /* DPENV_F32 / DPENV_BF16: the block's, independent of the handle's config */
    const uint8_t* done;     /* [T][n] DPENV_DONE_* bits, or NULL = no episode ends in the block */
    const float* z_in;       /* [3][n] (dpenv_get_dp_controller_state's layout) or NULL = 0 */
    float* z_out;            /* [3][n] or NULL; may be z_in */
    float* act;              /* [T][n][7] the law's action on obs[t] */
} dpenv_controller_label_io;
int dpenv_controller_label(dpenv_handle h, const dpenv_controller_label_io* io, dpenv_stream s);
/* The stateless allocation of the law (its f_m, bow and stern lines) for n wrenches: tau device float[3][n] -> action_out device
 * float[n][7].  Handle-free, like dpenv_thrust_map; of c only G, kf, kr_bow and f_eps are read, the whole struct is validated. */
int dpenv_thrust_alloc(const dpenv_dp_controller* c, const float* tau, float* action_out, int32_t n, dpenv_stream s);

/* ---- the rate-limited QP thrust allocation: the thesis' third allocator (additive to ABI 6) ---------------------------------------------
 * The reference's nonlinear "QP" allocator (src/qp/ROS/qp_allocator/src/qp_allocator.py:108-234) as a handle-free, STATEFUL map on the
 * device: per env and control step a wrench tau and the thruster state in force go in, the new state and the final variant's
 * continuous-angle action come out.  The formulation is the reference's; the solver is build-defined.  SLSQP is not ported, and neither
 * are the +-s_bnd bound on the slack and the node's retry loop that widens it (:209-226): the slack is eliminated, which is the problem
 * that loop converges to, so the solve cannot fail on an infeasible wrench - the wrench is followed as far as the rate limits allow.
 *
 * Unknowns x = (F_bow, F_port, F_star, a_port, a_star) in env order; the bow tunnel thruster's azimuth is fixed at pi / 2, so its column
 * of B is (0, 1, lx_bow).  With x^- the state in force (F^-, a^-):
 *     r(x) = B(a) F - tau                  B column i: (cos a_i, sin a_i, lx_i sin a_i - ly_i cos a_i)
 *     J(x) = 1/2 sum_j w_slack_j r_j^2 + 1/2 w_power sum_i |F_i|^3 + 1/2 w_dalpha sum_i (a_i - a_i^-)^2 + 1/2 w_dforce sum_i (F_i - F_i^-)^2
 *     lo_i = fmaxf(-f_max_i, F_i^- - dF_i)   hi_i = fminf(f_max_i, F_i^- + dF_i)      dF_i = force_rate_i * dt      (forces, i = 0..2)
 *     lo_k = a_k^- - da_k                    hi_k = a_k^- + da_k                      da_k = azimuth_rate_k * dt    (azimuths, k = 0, 1)
 * dF and da are one f32 product each, formed on the host.  Defaults (dpenv_qp_allocator_defaults; :52-58,116-150): w_slack (1, 1, 1),
 * w_power 1, w_dalpha = w_dforce = 0.25, f_max (9, 20.5, 20.5) N, force_rate (10, 25, 25) N/s and azimuth_rate 5 pi / 12 rad/s - with
 * dt = 0.2 s the reference's (2, 5, 5) N and pi / 12 per step - and the default hull's lever arms and thrust constants.
 *
 * SOLVER: `iterations` (K, 1..32, default 16) projected Levenberg-Marquardt steps with accept / reject from x = clip(x^-, lo, hi) (x^-
 * itself wherever |F^-| <= f_max) and lambda = 0.  In f32, in exactly this order (-ffp-contract=off: no product below is fused into a
 * sum; sqrtf and / are correctly rounded; clip(v, lo, hi) = fminf(fmaxf(v, lo), hi); sin / cos are the library's call-free polynomial,
 * max abs error 9.2e-8):
 *   evaluate(x):   (s_k, c_k) = sincos(a_k);   b3_k = lx_k * s_k - ly_k * c_k                         k = port, star
 *     r_0 = (c_p * F_p + c_s * F_s) - tau_0
 *     r_1 = ((F_b + s_p * F_p) + s_s * F_s) - tau_1
 *     r_2 = ((lx_b * F_b + b3_p * F_p) + b3_s * F_s) - tau_2
 *     Js = (w_slack_0 * (r_0 * r_0) + w_slack_1 * (r_1 * r_1)) + w_slack_2 * (r_2 * r_2)
 *     Jp = (|F_b| * (F_b * F_b) + |F_p| * (F_p * F_p)) + |F_s| * (F_s * F_s)
 *     e_i = x_i - x_i^-;   Ja = e_3 * e_3 + e_4 * e_4;   Jf = (e_0 * e_0 + e_1 * e_1) + e_2 * e_2
 *     J = 0.5 * (((Js + w_power * Jp) + w_dalpha * Ja) + w_dforce * Jf)
 *   per iteration, at the current x with its s, c, b3, r, J:
 *   1. Jm [3][5], the Jacobian of r: column F_b = (0, 1, lx_b); column F_k = (c_k, s_k, b3_k);
 *      column a_k = (-(F_k * s_k), F_k * c_k, F_k * (lx_k * c_k + ly_k * s_k))
 *   2. wr_j = w_slack_j * r_j;  WJ[j][l] = w_slack_j * Jm[j][l];  g_l = (Jm[0][l] * wr_0 + Jm[1][l] * wr_1) + Jm[2][l] * wr_2, then
 *      g_i = g_i + ((1.5 * w_power) * (F_i * |F_i|) + w_dforce * (F_i - F_i^-))  for the forces,  g_k = g_k + w_dalpha * (a_k - a_k^-)
 *   3. H[k][l] = (Jm[0][k] * WJ[0][l] + Jm[1][k] * WJ[1][l]) + Jm[2][k] * WJ[2][l]  for l <= k (the lower triangle is H), then
 *      H[i][i] = H[i][i] + ((3 * w_power) * |F_i| + w_dforce),  H[k][k] = H[k][k] + w_dalpha: Gauss-Newton, definite by its diagonal
 *   4. H[k][k] = H[k][k] + lambda * H[k][k]
 *   5. frozen_k = (x_k <= lo_k and g_k > 0) or (x_k >= hi_k and g_k < 0), with the g of step 2 and the H[k][k] of step 4; a frozen k
 *      has g_k = 0, H[k][k] = 1 and zeros in the rest of its row and column
 *   6. H = L D L' without pivoting, for j = 0..4:  v_m = L[j][m] * D_m (m < j);  D_j = H[j][j] - L[j][0] * v_0 - ... in order of m;
 *      iD_j = 1 / D_j;  L[i][j] = (H[i][j] - L[i][0] * v_0 - ...) * iD_j (i > j).  y_i = -g_i - L[i][0] * y_0 - ... (m < i, in order);
 *      d_i = y_i * iD_i - L[i+1][i] * d_{i+1} - ... (m > i, ascending), i = 4..0
 *   7. x_t = clip(x + d, lo, hi);  evaluate(x_t)
 *   8. J(x_t) < J(x): x = x_t, lambda = 0.25 * lambda;  else x stays, lambda = 8 * fmaxf(lambda, 0.125)
 * J never increases, and x stays in [lo, hi].  PRECONDITION on the state a caller supplies (state_in, dpenv_set_qp_allocator_state): finite,
 * and |F_i^-| <= f_max_i.  The law's own outputs meet it.  Then lo <= x^- <= hi and the start is x^- itself; a state with
 * |F_i^-| > f_max_i + dF_i has lo_i > hi_i, clip then returns hi_i and "inside [lo, hi]" no longer holds for that force; a state that
 * is not finite gives an action that is not finite.  Neither is checked: the state lives on the device.  A plain projected Gauss-Newton without step 8 does not converge on rate-infeasible jumps.
 * After the last iteration F^- = F and a^- = a wrapped to [-pi, pi) (k = floorf((a + pi) * (0.5 / pi)), a^- = fmaf(-k, 2 pi, a); mapToPi
 * :101-106,277), and
 *     action = [ n_b, n_p, n_s, sin a_p, cos a_p, sin a_s, cos a_s ],   n_i = clip(copysignf(sqrtf(|F_i| / K_i), F_i) / 100, -1, 1)
 * with K_i = F_i >= 0 ? kf_i : kr_i (:287-288) and the heads taken once more, of the un-wrapped a.  If any component of tau is not finite
 * the env's state is left bit for bit what it was and the action is that state's - the node's rule for a failed solve (:267-269); no
 * other env is affected.  cost_out gets the final J (NaN for such an env).
 * AT THE EDGES of the numbers (tests/qp_edges.py flies them).  A finite tau so large that the f32 J of the start is not finite (|tau_j|
 * from about 1e19 / sqrt(w_slack_j); +inf, or NaN = 0 * inf where w_slack_j = 0): every trial's J is not finite either, J(x_t) < J(x) is
 * false each time, so the env holds its clipped start - state_out is that start with the azimuths wrapped, the action is finite - and
 * cost_out gets that J, which is NOT finite although tau is.  Azimuths beyond 3e4 rad in magnitude, where sincos folds in f32 first: the
 * heads are a valid rotation of about that angle, not one within 9.2e-8 of it.  A thruster with f_max_i = 0 or dF_i = 0 whose F_i^- is
 * -0.0 has lo_i = -0.0 and hi_i = +0.0: the sign of the zero that clip returns there is not specified; everywhere else a force of -0.0
 * that stays is -0.0 and commands n_i = -0.0.  With every f_max_i = 0 the forces stay 0 and with every rate 0 nothing moves, whatever tau.
 * ml4ca_amd.deploy.BatchedQPAllocator is the host statement of the law. */
typedef struct dpenv_qp_allocator {
    uint32_t struct_size;
    int32_t iterations;          /* K, 1..32 */
    float w_slack[3];            /* >= 0 */
    float w_power;               /* >= 0 */
    float w_dalpha, w_dforce;    /* > 0: they keep H definite */
    float f_max[3];              /* >= 0 [N]: bow, port, star */
    float force_rate[3];         /* >= 0 [N/s] */
    float azimuth_rate[2];       /* >= 0 [rad/s]: port, star */
    float lx[3], ly[3];          /* lever arms [m]: bow, port, star, finite (ly[0] is not used) */
    float kf[3], kr[3];          /* thrust constants ahead / astern, > 0 */
} dpenv_qp_allocator;
int dpenv_qp_allocator_defaults(dpenv_qp_allocator* q);
/* One control step for n envs, one lane per env.  Device pointers: tau float[3][n]; state_in float[5][n] = F_bow, F_port, F_star, a_port,
 * a_star (NULL = zeros); state_out float[5][n] (NULL = not wanted; may be state_in); action_out float[n][7]; cost_out float[n] or NULL.
 * dt [s] > 0 is the control period.  Refused with DPENV_EINVAL before anything is launched: a wrong struct_size, a number that is not
 * finite, a weight < 0, w_dalpha or w_dforce <= 0, a bound or rate < 0, kf or kr <= 0, iterations outside 1..32, dt <= 0, n <= 0, NULL
 * tau or action_out.  Stream-ordered, no allocation, no host synchronisation: graph-capturable, one kernel node.
 * A caller with its own motion controller closes the loop with this call between two launches. */
int dpenv_thrust_alloc_qp(const dpenv_qp_allocator* q, float dt, const float* tau, const float* state_in, float* state_out,
                          float* action_out, float* cost_out, int32_t n, dpenv_stream s);
/* The QP law as the allocation stage of the baseline's closed loop: while one is set, dpenv_controller_rollout (signature and rows
 * unchanged) forms tau with the PID lines of the DP controller's law - z advanced, the wrench clipped to tau_max, bit for bit what they
 * are without it - and allocates it with the law above in place of the f_m / bow / stern lines; dt is the handle's.  Per env the
 * thruster state x^- [5] travels beside z: loaded with it, stored with it, and zeroed wherever z is zeroed - auto-reset (the new
 * episode's first action starts from thrusters at rest), dpenv_reset for the envs it re-draws, and this call (every env).  So the act
 * rows of a launch are dpenv_thrust_alloc_qp applied row by row to the PID's tau, bit for bit, and two launches of T/2 write the rows of
 * one launch of T.
 * Needs the DP controller on (it supplies tau, z and dt), else DPENV_EINVAL.  q = NULL returns the handle to the pseudo-inverse.
 * dpenv_set_dp_controller (on or off) drops the QP, as it drops the table.  Supported: the shared hull and the thrust-loss preset (one
 * class, hull as kernel arguments), constant, drifting and per-episode currents, auto-reset, with or without the reference filter.
 * Per-env hull blocks and their randomisation, a per-env controller table in force (and dpenv_set_dp_controller_table while a QP is set),
 * and whatever dpenv_set_dp_controller refuses: DPENV_EINVAL with the set named, at this call or - if the handle changed since - at the
 * launch.  Every refusal of a q that dpenv_thrust_alloc_qp refuses happens before any state changes.  The first call allocates the state
 * block (released with the handle); every later call is stream-ordered without allocation and graph-capturable.
 * dpenv_controller_label keeps labelling with the pseudo-inverse law whatever is set here; dpenv_controller_label_qp (below) labels with
 * this one. */
int dpenv_set_qp_allocator(dpenv_handle h, const dpenv_qp_allocator* q, dpenv_stream s);
/* The checkpoint path of the thruster state, beside z's: device float[5][n_envs] = F_bow, F_port, F_star, a_port, a_star.  DPENV_EINVAL
 * while no QP allocator is set. */
int dpenv_get_qp_allocator_state(dpenv_handle h, float* state_out, dpenv_stream s);
int dpenv_set_qp_allocator_state(dpenv_handle h, const float* state_in, dpenv_stream s);
/* One QP allocator PER ENV (additive to ABI 6): the tool that turns the QP's one point on the tracking-error / energy plane into a curve -
 * K weight sets x D current directions in ONE flight (ml4ca_amd.evaluate.qp_weight_sweep), as dpenv_set_dp_controller_table does for the
 * pseudo-inverse baseline.  The table is a DEVICE float[DPENV_QP_NPARAM][n_envs], laid out like the controller table - row p = slot p of
 * every env - and owned by the caller.  Slots, in the order of dpenv_qp_allocator's fields and with its conditions: */
#define DPENV_QP_NPARAM 32
#define DPENV_QP_WSLACK 0     /* 0-2  w_slack, finite and >= 0 */
#define DPENV_QP_WPOWER 3     /* w_power, finite and >= 0 */
#define DPENV_QP_WDALPHA 4    /* w_dalpha, finite and > 0 */
#define DPENV_QP_WDFORCE 5    /* w_dforce, finite and > 0 */
#define DPENV_QP_FMAX 6       /* 6-8  f_max: bow, port, star, finite and >= 0 */
#define DPENV_QP_FRATE 9      /* 9-11 force_rate [N/s], finite and >= 0 */
#define DPENV_QP_ARATE 12     /* 12-13 azimuth_rate [rad/s]: port, star, finite and >= 0 */
#define DPENV_QP_LX 14        /* 14-16 lever arms lx: bow, port, star, finite */
#define DPENV_QP_LY 17        /* 17-19 lever arms ly: bow (not used), port, star, finite */
#define DPENV_QP_KF 20        /* 20-22 thrust constants ahead, finite and > 0 */
#define DPENV_QP_KR 23        /* 23-25 thrust constants astern, finite and > 0 */
                              /* 26-31 reserved, not read */
/* The iteration count is NOT in the table: it is one number per call (1..32), so the solver's loop stays uniform across a wave.
 * dpenv_set_qp_allocator_table is dpenv_set_qp_allocator with row i flown on env i: the same preconditions and refusals with the same
 * messages (the DP controller on, no per-env hull blocks, no controller table in force, iterations in 1..32), the same law, the same
 * zeroing of every env's thruster state by a valid call.  A packing kernel, one lane per env, copies the table into a library-owned block
 * (allocated by the first call, released with the handle; 112 B per env) - the caller's buffer is free after the call, on the stream - and
 * forms dF = force_rate * dt and da = azimuth_rate * dt as one f32 product each with the handle's dt: exactly what the host forms for the
 * scalar call, so a table of equal rows flies the scalar call's rows bit for bit.  Later calls are stream-ordered without allocation and
 * graph-capturable; a captured launch flies whatever the last packing wrote.
 * Refused rows: dpenv_thrust_alloc_qp's checks, row by row (a number that is not finite, a weight < 0, w_dalpha or w_dforce <= 0, a bound
 * or rate < 0, kf or kr <= 0, a dF or da that is not finite).  A refused row is packed as the REST ALLOCATOR - f_max = force_rate =
 * azimuth_rate = 0, w_slack = w_power = 0, w_dalpha = w_dforce = 1, lx = ly = 0, kf = kr = 1 - with which the law commands zero thrust
 * and holds the azimuths, every output finite (from forces at rest, which is the law's precondition |F^-| <= f_max with f_max = 0: a
 * valid call leaves every env there); the other rows are not affected.  refused_out: NULL, or a device uint8[n_envs] that gets 1
 * for a refused env and 0 for the others.  The library reads nothing back and does not synchronise.
 * table = NULL returns to the scalar numbers dpenv_set_qp_allocator last set, or to the pseudo-inverse if none were set, and leaves z and
 * the thruster state alone (as dpenv_set_dp_controller_table(NULL) leaves z).  dpenv_set_qp_allocator(h, q) replaces the table by scalar
 * numbers (q = NULL: the pseudo-inverse again, nothing to return to); dpenv_set_dp_controller drops both; dpenv_set_dp_controller_table is
 * refused while a table is set, as it is while a scalar QP is set.  dpenv_get / dpenv_set_qp_allocator_state work unchanged.
 * dpenv_controller_label_qp with q = NULL is refused while a TABLE is in force (the scan takes one set of numbers: pass q);
 * dpenv_controller_label_qp_ex labels with a table of its own. */
int dpenv_set_qp_allocator_table(dpenv_handle h, const float* table, int32_t iterations, uint8_t* refused_out, dpenv_stream s);
/* dpenv_thrust_alloc_qp with row i of the PUBLIC table (device float[DPENV_QP_NPARAM][n]) on env i; the other arguments are that call's.
 * There is no packing launch: each lane reads its 26 numbers and checks them itself, with the device function the packing kernel uses, so
 * the two never disagree.  A refused lane runs the rest allocator above, reports NaN in cost_out and sets its byte of refused_out (device
 * uint8[n] or NULL; 0 for the others).  DPENV_EINVAL before anything is launched: NULL table, tau or action_out, n <= 0, iterations
 * outside 1..32, dt not finite or <= 0.  Stream-ordered, no allocation, no host synchronisation: graph-capturable, one kernel node. */
int dpenv_thrust_alloc_qp_table(const float* table, int32_t iterations, float dt, const float* tau, const float* state_in,
                                float* state_out, float* action_out, float* cost_out, uint8_t* refused_out, int32_t n, dpenv_stream s);
/* ---- the neural thrust allocation: the supervised contender (additive to ABI 6) ---------------------------------------------------------
 * The reference's first allocator, the supervised feed-forward network of src/sl (FFNN.py / train.py fit a 9-20-20-20-20-6 relu network
 * to SupervisedTau.py's dataset tau = B(alpha) F(u); ROS/neural_allocator/src/neural_allocator.py flies it behind the DP controller's
 * wrench), as a handle-free, STATELESS map on the device and as the allocation stage of the baseline's closed loop.  The network is a
 * dpenv_mlp: sizes[0] inputs (9: the node's six lever-arm constants and the scaled wrench; 3: the scaled wrench alone), n_layers - 1
 * hidden layers of one width, six outputs.  Per env and control step, in f32, in exactly this order (-ffp-contract=off; the only fused
 * operations are the fmaf written below):
 *     input       x_{6+j} = tau_j * tau_scale_j, j = 0..2 (one product each), behind x_0..5 = in_const when sizes[0] == 9; x_j = tau_j *
 *                 tau_scale_j alone when sizes[0] == 3                                                      (neural_allocator.py:117-126)
 *     dense layer y_j = b_j, then for k ascending y_j = fmaf(W[k][j], h_k, y_j)           (h = x for the first layer; W[l][in][out])
 *     activation  h_j = y_j > 0 ? y_j : leak * y_j for a hidden layer (leak = 0: relu, src/sl/train.py:111); the last layer is linear
 *     output      p = (u_port, u_star, u_bow, a_port, a_star, a_bow), the node's order (:137)
 *     thrust      n_i = fminf(fmaxf(p_i, -1), 1), i = 0..2: the node's * 100, its saturation at +-100 % (:178-192) and the env's / 100,
 *                 stated once
 *     stern angle ang_k = p_{3+k} * angle_scale, k = port, star (azimuth_mode 0, the node's `rotating`), or ang_k = azimuth[k]
 *                 (azimuth_mode 1: the node's fixed pods, :225)
 *     heads       (sin_k, cos_k) = the library's call-free sincos of ang_k (max abs error 9.2e-8)
 *     action      [ n_bow, n_port, n_star, sin_port, cos_port, sin_star, cos_star ]
 * a_bow is not used: the env's tunnel thruster is fixed.  REST RULE: if any tau_j or any of the six p is not finite, that env's action is
 * the rest action [0, 0, 0, 0, 1, 0, 1]; no other env is affected.  (With leak = 0 a hidden pre-activation of -inf gives 0 * -inf = NaN
 * and so the rest action.)  The law has no state and reads no hull.  ml4ca_amd.deploy.BatchedNNAllocator is its host statement.
 * dpenv_controller_label_nn (below) scans the PID + network chain over rows some other flight wrote.
 * NOT HERE: a reader for the reference's .h5 models (weights arrive as arrays), one network per single env (the weights reach the
 * fmaf through scalar loads because every lane of a wave reads the same ones; a network per lane would take them out of the scalar path -
 * one network per 64 envs is dpenv_set_nn_allocator_population below), and an evaluation on the matrix cores - the network is evaluated
 * on the VALU, one fmaf per weight and env. */
typedef struct dpenv_nn_allocator {
    uint32_t struct_size;
    const dpenv_mlp* net;     /* sizes[0] in {3, 9}; sizes[n_layers] == 6; n_layers 2..5; hidden widths equal, 1..96 */
    float leak;               /* hidden activation y > 0 ? y : leak * y; 0 <= leak <= 1, 0 = relu (src/sl/train.py:111) */
    float in_const[6];        /* inputs 0..5 when sizes[0] == 9: lx_port, ly_port, lx_star, ly_star, lx_bow, ly_bow (neural_allocator.py:74-79) */
    float tau_scale[3];       /* (1/54, 1/69.2, 1/76.9), formed in f64, rounded once (:60) */
    float angle_scale;        /* pi (:50,61) */
    int32_t azimuth_mode;     /* 0: the network's stern angles (the node's `rotating`); 1: fixed at azimuth[2] (:225: -3pi/4, 3pi/4) */
    float azimuth[2];         /* port, star [rad], read in mode 1 */
    int32_t device_pointers;  /* as dpenv_policy_desc's */
} dpenv_nn_allocator;
/* Fills the constants above (leak 0, azimuth_mode 0, device_pointers 1) and leaves net NULL. */
int dpenv_nn_allocator_defaults(dpenv_nn_allocator* a);
/* One control step for n envs, one lane per env.  Device pointers: tau float[3][n]; action_out float[n][7]; raw_out float[n][6] = the six
 * p, or NULL.  The network's W and b must be DEVICE pointers (device_pointers = 1) and are read in place: no packing launch, no
 * allocation, no synchronisation - graph-capturable, one kernel node.  Refused with DPENV_EINVAL before anything is launched, the field
 * named in dpenv_last_error(NULL): a wrong struct_size, a NULL net, a shape outside the set above, a NULL W / b / tau / action_out, a leak
 * outside [0, 1], an in_const, tau_scale, angle_scale or azimuth that is not finite, an azimuth_mode other than 0 and 1, n <= 0,
 * device_pointers other than 1. */
int dpenv_thrust_alloc_nn(const dpenv_nn_allocator* a, const float* tau, float* action_out, float* raw_out, int32_t n, dpenv_stream s);
/* The network as the allocation stage of the baseline's closed loop: while one is set, dpenv_controller_rollout (signature and rows
 * unchanged) forms tau with the PID lines of the DP controller's law - z advanced, the wrench clipped to tau_max, bit for bit what they
 * are without it - and allocates it with the law above in place of the f_m / bow / stern lines.  So the act rows of a launch are
 * dpenv_thrust_alloc_nn applied row by row to the PID's tau, bit for bit, and two launches of T/2 write the rows of one launch of T.
 * The weights are copied into a library-owned, zero-padded image (allocated by the first call at the size of the largest shape, released
 * with the handle), so the caller's arrays are free after the call, on the stream.  device_pointers = 1: one packing launch on s -
 * stream-ordered, no allocation after the first call, graph-capturable; the image of a shape always lies at the same addresses, so a
 * captured launch flies whatever the last upload of that shape wrote (an upload of another shape voids graphs captured before).
 * device_pointers = 0 (host arrays): the call synchronises s before it returns, as dpenv_set_policy_desc does.  An upload is ordered
 * behind earlier launches by stream order alone: issue it on the stream the launches use.
 * Needs the DP controller on (it supplies tau, z and dt), else DPENV_EINVAL.  a = NULL returns the handle to the pseudo-inverse.
 * dpenv_set_dp_controller (on or off) drops the network, as it drops the QP.  The law touches no hull, so it is supported wherever
 * dpenv_set_dp_controller is: the shared hull, the thrust-loss preset, per-env hull blocks and their randomisation, every current,
 * auto-reset, with or without the reference filter.  Refused with DPENV_EINVAL and the reason named: a per-env controller table in force,
 * a QP allocator (scalar or table) set, and whatever dpenv_set_dp_controller refuses (the integral action on, ...); in the other
 * direction dpenv_set_qp_allocator, dpenv_set_qp_allocator_table and dpenv_set_dp_controller_table are refused while a network is set.
 * dpenv_controller_label, dpenv_controller_label_qp and dpenv_controller_label_qp_ex are untouched: they label with the pseudo-inverse
 * and the QP law whatever is set here. */
int dpenv_set_nn_allocator(dpenv_handle h, const dpenv_nn_allocator* a, dpenv_stream s);
/* ---- a population of neural allocators: one network per envs_per_net envs (additive to ABI 6) -------------------------------------------
 * K networks of ONE shape and ONE set of constants (leak, in_const, tau_scale, angle_scale, azimuth_mode, azimuth) in one flight: what
 * dpenv_set_dp_controller_table is to the PID's gains and dpenv_set_qp_allocator_table to the QP's numbers.  a is a dpenv_nn_allocator
 * whose net arrays carry a leading axis K: W[l] is [K][in][out], b[l] is [K][out] (sizes[] is one network's).  The law:
 *     net(j) = (j / envs_per_net) % K                   (integer division; j a global env id)
 *     env i of the handle flies network net(env_id_base + i), with the law above - the REST RULE per env included.
 * envs_per_net is a multiple of 64 and so is env_id_base: the closed loop runs 64 envs per wave, a wave never straddles two networks, and
 * the wave's weights stay wave-uniform (scalar loads).  The % K wraps: more envs than K * envs_per_net fly network 0 again behind K - 1,
 * fewer leave the trailing networks unused.  While a population is set, dpenv_controller_rollout (signature and rows unchanged) allocates
 * env i's PID wrench with its network; everything else is dpenv_set_nn_allocator's flight, so with K = 1 the rows are that call's bit for
 * bit, and the rows of env i are those of dpenv_set_nn_allocator with network net(env_id_base + i) on an identically configured handle.
 * The weights go into a library-owned zero-padded image of K networks (per layer [K][in][pad16(out)], then [K][pad16(out)]), released
 * with the handle.  device_pointers = 1: ONE packing launch on s with the network index on a grid axis; an upload with the shape and K of
 * the image in place is stream-ordered, allocation-free and graph-capturable, and a captured launch flies whatever the last such upload
 * wrote.  An upload with ANOTHER shape or K RE-ALLOCATES the image (hipMalloc, then hipFree of the old one, which synchronises the
 * device): not capturable, and graphs captured before are void.  device_pointers = 0 (host arrays): the call synchronises s before it
 * returns.  If the allocation fails the call returns DPENV_ENOMEM and the handle is as it was - the old image, the stage in force.
 * DPENV_EINVAL with the field named, before anything is launched or allocated: K < 1; envs_per_net < 64 or not a multiple of 64;
 * K * (envs_per_net / 64) >= 2^31; the handle's env_id_base negative or not a multiple of 64; and everything dpenv_set_nn_allocator
 * refuses (the controller off, a per-env controller table in force, a QP allocator set, a bad shape, constant or device_pointers).
 * a = NULL returns the handle to the pseudo-inverse (K and envs_per_net are not looked at).  dpenv_set_nn_allocator replaces a population
 * by one network, and this call replaces one network by a population; dpenv_set_dp_controller drops it; dpenv_set_qp_allocator,
 * dpenv_set_qp_allocator_table and dpenv_set_dp_controller_table are refused while it is set, as they are under one network.
 * dpenv_controller_label_nn under a population: with a = NULL and act wanted the call is refused (the scan takes ONE network: pass a -
 * the precedent is dpenv_controller_label_qp under a QP table); the wrench-only scan (act = NULL) and the scan with an explicit a work as
 * on any handle.  A population form of the scan is NOT HERE: dpenv_thrust_alloc_nn_population on the scan's tau_out is that scan's act,
 * bit for bit. */
int dpenv_set_nn_allocator_population(dpenv_handle h, const dpenv_nn_allocator* a, int32_t K, int32_t envs_per_net, dpenv_stream s);
/* dpenv_thrust_alloc_nn with K stacked networks: env i of the call takes network (i / envs_per_net) % K.  a's W[l] [K][in][out] and b[l]
 * [K][out] are DEVICE arrays (device_pointers = 1) read in place: no packing launch, no allocation, no synchronisation - graph-capturable,
 * one kernel node.  On network k's lanes the outputs are dpenv_thrust_alloc_nn's with network k, bit for bit.  DPENV_EINVAL before
 * anything is launched: what dpenv_thrust_alloc_nn refuses, K < 1, envs_per_net < 64 or not a multiple of 64. */
int dpenv_thrust_alloc_nn_population(const dpenv_nn_allocator* a, int32_t K, int32_t envs_per_net, const float* tau, float* action_out,
                                     float* raw_out, int32_t n, dpenv_stream s);
/* The PID + network chain on rows some other flight wrote (additive to ABI 6): dpenv_controller_label's scan with the neural allocation
 * in place of the f_m / bow / stern lines, and the PID's clipped wrench per row beside it - the network's labels for the states an actor
 * visited, and the wrenches a flight asked of its allocator, which the closed loop never writes.  One launch, one lane per env; per row t
 * and env i, in the order of the closed loop with a network set:
 *     o   = obs[t][i][0:6]                              (a bf16 value widened exactly)
 *     tau = the PID lines of the DP controller's law on o with the env's z_i: z_i advanced first, the wrench clipped to tau_max
 *     tau_j = NaN if o_j or o_{3+j} is NaN              (the law's fminf / fmaxf clip drops a NaN: a closed loop would fly -tau_max on such
 *                                                        a row, which no flight writes; the scan answers it with the REST RULE, as the host
 *                                                        statement does, and z_i stays the law's)
 *     tau_out[t][i][0:3] = tau                          (if tau_out is not NULL: the exact value the allocator is handed)
 *     act[t][i][0:7], p = the neural law above on tau   (if act is not NULL; the REST RULE included)
 *     raw[t][i][0:6] = p                                (if raw is not NULL)
 *     if (done && done[t][i] != 0) z_i = 0              -- the next row is a new episode's first
 * z_i starts from z_in[:, i] (NULL = 0) and is written to z_out at the end (NULL = not wanted; may be z_in), so a block labelled in pieces
 * with z handed over gives the rows of one call.  The network has no state: nothing else travels.  The PID's numbers are the handle's
 * controller in force: row i of dpenv_set_dp_controller_table's table on env i when there is one, else dpenv_set_dp_controller's; dt is
 * the handle's.  a: the network and its constants, validated with the checks of dpenv_thrust_alloc_nn (device_pointers = 1: W and b are
 * DEVICE arrays read in place, no packing launch, no allocation); NULL = the network dpenv_set_nn_allocator has in force on h, its image
 * and its constants.
 * (A) For f32 rows written by dpenv_controller_rollout with a network set and auto-reset on, labelled with that launch's done block, the z
 *     it started from and a = NULL, act is that launch's act rows bit for bit and z_out is its final z.
 * (B) On any block, act and raw are dpenv_thrust_alloc_nn applied row by row to tau_out, bit for bit - with an explicit a and with
 *     a = NULL alike.
 * With an explicit a the handle's allocation stage does not matter: a handle with a per-env controller table, a QP allocator or nothing
 * set is labelled with a network.  dpenv_set_nn_allocator refuses a controller table; the scan does not, and env i takes row i of the
 * PID's table.  With act = NULL no network is needed at all and a is not looked at: the call is a scan of the PID lines alone, bound by
 * its row traffic (tau_out and z_out are those of the full scan, bit for bit).
 * The call reads and writes nothing of the handle's env state, its z, its network image, the lagged thrust columns or the RNG counters.
 * Stream-ordered, no allocation, no host synchronisation; one kernel node when captured into a graph (a captured call with a = NULL flies
 * whatever the last upload of that shape wrote, and the constants of capture time).  The scan is serial in T per env.
 * DPENV_EINVAL with the reason in dpenv_last_error, before anything is launched or written: the controller off, a wrong struct_size,
 * T <= 0, NULL obs, act and tau_out both NULL, raw without act, an obs_dtype that is neither DPENV_F32 nor DPENV_BF16, act wanted with
 * a NULL and no network set, act wanted with a NULL while a POPULATION is in force (dpenv_set_nn_allocator_population: pass a), and
 * whatever dpenv_thrust_alloc_nn refuses of a.  ml4ca_amd.deploy.label_rows_nn is the host statement. */
typedef struct dpenv_controller_label_nn_io {
    uint32_t struct_size;    /* sizeof(dpenv_controller_label_nn_io), ABI check */
    int32_t T;
    const void* obs;         /* [T][n][9] rows in dpenv_policy_rollout's conventions; f32 or bf16; columns 0..5 read */
    int32_t obs_dtype;       /* DPENV_F32 / DPENV_BF16: the block's, independent of the handle's config */
    const uint8_t* done;     /* [T][n] DPENV_DONE_* bits, or NULL = no episode ends in the block */
    const float* z_in;       /* [3][n] (dpenv_get_dp_controller_state's layout) or NULL = 0 */
    float* z_out;            /* [3][n] or NULL; may be z_in */
    float* act;              /* [T][n][7] the chain's action on obs[t], or NULL = the wrench-only scan */
    float* raw;              /* [T][n][6] the network's six outputs p, or NULL; needs act */
    float* tau_out;          /* [T][n][3] the PID's clipped wrench, or NULL */
    const dpenv_nn_allocator* a;   /* the network; NULL = the one dpenv_set_nn_allocator has in force on h */
} dpenv_controller_label_nn_io;
int dpenv_controller_label_nn(dpenv_handle h, const dpenv_controller_label_nn_io* io, dpenv_stream s);
/* The PID + QP chain on rows some other flight wrote (additive to ABI 6): dpenv_controller_label's scan with the QP law in place of the
 * f_m / bow / stern lines - the low-energy expert's labels for the states an actor visited.  One launch, one lane per env; per row t and
 * env i, in the order of the closed loop with a QP set:
 *     o   = obs[t][i][0:6]                              (a bf16 value widened exactly)
 *     tau = the PID lines of the DP controller's law on o with the env's z_i: z_i advanced first, the wrench clipped to tau_max
 *     act[t][i][0:7], J = the QP law above on tau and the env's thruster state x_i, which it advances (the rule for a tau that is not
 *                         finite and the wrap of the azimuths included)
 *     cost[t][i] = J                                    (if cost is not NULL)
 *     if (done && done[t][i] != 0) z_i = 0, x_i = 0     -- the next row is a new episode's first, from thrusters at rest
 * z_i starts from z_in[:, i] and x_i from x_in[:, i] (NULL = 0); they are written to z_out / x_out at the end (NULL = not wanted; each
 * may be its input), so a block labelled in pieces with z and x handed over gives the rows of one call.  x is the EXPERT'S OWN recursion
 * along the rows, as z is: not the thruster state the flown actions would have left (dpenv_controller_label_qp_ex, below, takes that one).
 * The PID's numbers are the handle's controller in force: row i of dpenv_set_dp_controller_table's table on env i when there is one (G
 * is not read), else dpenv_set_dp_controller's.  dt is the handle's, for z and for dF = force_rate * dt and da = azimuth_rate * dt, one
 * f32 product each formed on the host.  q: the QP's numbers, validated with the checks of dpenv_thrust_alloc_qp; NULL = the ones
 * dpenv_set_qp_allocator has in force on h.  The handle's hull kind does not matter - no hull is touched - so a handle with per-env hull
 * blocks or a controller table, on which dpenv_set_qp_allocator is refused, labels with an explicit q.
 * (A) For f32 rows written by dpenv_controller_rollout with a QP set and auto-reset on, labelled with that launch's done block, the z and
 *     the thruster state it started from, the same controller and the same q, the labels are that launch's act rows bit for bit, z_out is
 *     its final z and x_out its final dpenv_get_qp_allocator_state.
 * (B) On any block the labels are dpenv_thrust_alloc_qp applied row by row to the PID's tau, with the state zeroed behind done rows, bit
 *     for bit, cost included.
 * The call reads and writes nothing of the handle's env state, its z, its own QP thruster state, the lagged thrust columns or the RNG
 * counters.  Stream-ordered, no allocation, no host synchronisation; one kernel node when captured into a graph (a captured call flies
 * the scalar numbers and the q of capture time, and whatever table the last packing wrote).  The scan is serial in T per env: at small n
 * its cost is the closed loop's latency per row.
 * DPENV_EINVAL with the reason in dpenv_last_error, before anything is launched or written: the controller off, a wrong struct_size,
 * T <= 0, NULL obs or act, an obs_dtype that is neither DPENV_F32 nor DPENV_BF16, q NULL with no QP allocator set, and whatever
 * dpenv_thrust_alloc_qp refuses of q.  ml4ca_amd.deploy.label_rows_qp is the host statement. */
typedef struct dpenv_controller_label_qp_io {
    uint32_t struct_size;    /* sizeof(dpenv_controller_label_qp_io), ABI check */
    int32_t T;
    const void* obs;         /* [T][n][9] rows in dpenv_policy_rollout's conventions; f32 or bf16; columns 0..5 read */
    int32_t obs_dtype;       /* DPENV_F32 / DPENV_BF16: the block's, independent of the handle's config */
    const uint8_t* done;     /* [T][n] DPENV_DONE_* bits, or NULL = no episode ends in the block */
    const float* z_in;       /* [3][n] (dpenv_get_dp_controller_state's layout) or NULL = 0 */
    float* z_out;            /* [3][n] or NULL; may be z_in */
    const float* x_in;       /* [5][n] thruster state (dpenv_get_qp_allocator_state's layout) or NULL = 0 */
    float* x_out;            /* [5][n] or NULL; may be x_in */
    float* act;              /* [T][n][7] the chain's action on obs[t] */
    float* cost;             /* [T][n] the final J of each row's solve, or NULL */
    const dpenv_qp_allocator* q;   /* the QP's numbers; NULL = the ones dpenv_set_qp_allocator has in force on h */
} dpenv_controller_label_qp_io;
int dpenv_controller_label_qp(dpenv_handle h, const dpenv_controller_label_qp_io* io, dpenv_stream s);
/* The same scan with the thruster state taken from the FLOWN actions and / or one QP allocator per env (additive to ABI 6).  The DAgger
 * label is the expert's answer in the state the learner is in, and the actuators are part of that state: with `flown`, row t is solved
 * from the thruster state the EXECUTED action of row t - 1 left, not from the expert's own recursion.
 * S(q, a[7]) -> x[5], the thruster state an executed action row of the final variant's continuous-angle form leaves: the env's own command
 * decode followed by the QP's thrust law, f32, in this order (clip(v, b) = fminf(fmaxf(v, -b), b)):
 *     thr_k = clip(a[k] * 100, 100)                                        k = bow, port, star
 *     K     = thr_k >= 0 ? kf_k : kr_k
 *     F_k   = (K * thr_k) * |thr_k|
 *     F_k   = clip(F_k, f_max_k)                       -- the law's precondition |F^-| <= f_max
 *     x_k   = F_k, or 0 if a[k] or F_k is not finite
 *     al_i  = clip(atan2(a[3 + 2 i], a[4 + 2 i]), pi)                      i = port, star; the library's call-free atan2, max abs error 2.6e-7
 *     al_i  = al_i - 2 pi floorf((al_i + pi) * (0.5 / pi))                 -- the wrap of the law's own state, the last step one fmaf
 *     x_{3+i} = al_i, or 0 if either head or al_i is not finite
 * kf, kr and f_max are the QP's numbers: row i's when a table labels.  A component fed by an entry that is not finite is AT REST (the env
 * itself flies a NaN thrust entry as -100 %: such a row has no meaning and the scan does not follow it).
 * Per row t and env i, everything else as dpenv_controller_label_qp:
 *     x_used = x_i                                       (x_in[:, i] at t = 0; NULL = 0)
 *     tau    = the PID lines on obs[t][i] with z_i       (unchanged)
 *     act[t][i], J = the QP law on tau from x_used       (the law's own advance of x is dropped)
 *     x_i    = S(q_i, flown[t][i])
 *     if (done && done[t][i] != 0) z_i = 0, x_i = 0
 * x_out is the last x_i, so a block labelled in pieces with z and x handed over equals one call; the label of row t does not depend on
 * flown[t:].  Behind a done row the flown form keeps the convention "thrusters at rest": the thrust the reset drew for the new episode is
 * not known to the scan.  There is NO float32 bit-for-bit identity against the QP closed loop's own rows for the flown form - S of the law's
 * own action returns its state to within 2 ulp of the forces and 1e-6 rad, and the solver's accept / reject turns amplify that (a few 1e-2
 * in an action entry at 16 iterations); the identity that holds is by parts: act[t][i] and cost[t][i] are dpenv_thrust_alloc_qp on the PID's
 * tau and the x_used above, bit for bit.
 * qp_table: a DEVICE float[DPENV_QP_NPARAM][n_envs], the public table of dpenv_set_qp_allocator_table, env i labelled with row i in
 * `iterations` (1..32) solver steps: K weight sets label one block of states in one launch.  There is no packing launch: each lane reads
 * and checks its row itself, as in dpenv_thrust_alloc_qp_table; a refused row runs the rest allocator, reports NaN in cost and sets its
 * byte of refused_out (device uint8[n_envs] or NULL; 0 for the others).  dF and da are formed with the handle's dt.
 * q and qp_table both given: DPENV_EINVAL.  refused_out without qp_table: DPENV_EINVAL.  With neither q nor qp_table the rules of
 * dpenv_controller_label_qp apply (the handle's scalar numbers; refused while a table is in force: pass q or qp_table).  With flown = NULL
 * and no qp_table the call IS dpenv_controller_label_qp.  All other refusals are that call's, before anything is launched, and so are its
 * guarantees: the handle untouched, no allocation, no synchronisation, one kernel node under capture.
 * ml4ca_amd.deploy.label_rows_qp(flown=...) and deploy.qp_state_from_action are the host statements. */
typedef struct dpenv_controller_label_qp_ex_io {
    uint32_t struct_size;    /* sizeof(dpenv_controller_label_qp_ex_io), ABI check */
    int32_t T;
    const void* obs;         /* as dpenv_controller_label_qp_io, field by field ... */
    int32_t obs_dtype;
    const uint8_t* done;
    const float* z_in;
    float* z_out;
    const float* x_in;
    float* x_out;
    float* act;
    float* cost;
    const dpenv_qp_allocator* q;
    const float* flown;      /* ... then: [T][n][7] f32 the executed actions, or NULL = the expert's own recursion */
    const float* qp_table;   /* device float[DPENV_QP_NPARAM][n], or NULL */
    int32_t iterations;      /* read with qp_table: 1..32 */
    uint8_t* refused_out;    /* [n] or NULL; with qp_table */
} dpenv_controller_label_qp_ex_io;
int dpenv_controller_label_qp_ex(dpenv_handle h, const dpenv_controller_label_qp_ex_io* io, dpenv_stream s);

/* ---- The PPO update: actor and critic gradients and a device-gated Adam step --------------------------------------------------------
 * Handle-free like dpenv_gae / dpenv_adv_*: device pointers and a stream; no call allocates or synchronises, so a whole update (80
 * actor steps, 80 critic steps) queues without a host round trip and every call can be captured into a graph (each call is a chain of
 * kernels, no parallel branches).  Everything is validated on the host before any device call; a refused call launches nothing.
 *
 * PARAMETERS.  One flat float theta[P] per network: W0 row-major [in][out] (the x @ W orientation), b0, W1, b1, ..., and for the actor
 * log_std[out] at the end.  9 -> 80 -> 80 -> 80 -> 7 with log_std: P = 14 334; 9 -> 80 -> 80 -> 80 -> 1: P = 13 841
 * (dpenv_train_param_count).  Hidden activation h = max(z, leak z), 0 <= leak <= 1 (0 = relu); its derivative is 1 where z > 0 and
 * leak elsewhere (z = 0 included).
 *
 * ROWS.  f32: obs [n_rows][in], act [n_rows][out], adv, ret, logp_old [n_rows].  idx: `count` row indices in [0, n_rows), repeats
 * allowed, or NULL = rows 0 .. count-1 (then n_rows >= count).  The indices are the CALLER'S CONTRACT: they live on the device and are
 * not checked there; an index outside [0, n_rows) reads outside the blocks.
 *
 * ACTOR LOSS (ppo.py:238-240), per row, sums over the out action components j:
 *     sd_j  = exp(log_std_j) + 1e-8
 *     q_j   = (act_j - mu_j) / sd_j
 *     logp  = sum_j -0.5 ((q_j^2 + 2 log_std_j) + log(2 pi))                          (gaussian_likelihood, core.py:42-46)
 *     ratio = exp(logp - logp_old)
 *     s1 = ratio A,   s2 = min(max(ratio, 1 - clip), 1 + clip) A,   L = -mean(min(s1, s2))
 * GRADIENT RULE.  dL/dlogp = -A ratio / count  if  s1 <= s2,  else 0.  s1 < s2 is the unclipped term being the minimum (also with the
 * ratio outside the bounds, when the advantage pulls it back); s1 == s2 happens where A == 0 or 1 - clip <= ratio <= 1 + clip, bounds
 * INCLUDED, and there torch.minimum's half-and-half tie split and torch.clamp's inclusive bounds add up to the same -A ratio / count.
 * A ratio outside float32's range is taken as float32 forms it: exp underflows to 0 (the row's gradient is zero for either sign of A)
 * or overflows to +inf, where A > 0 is cut (zero gradient, the row's loss -(1 + clip) A, mean_ratio +inf) and A < 0 is non-finite by
 * the law itself, as it is in torch float32 - such rows are the caller's to keep out.
 *     dlogp/dmu_j = q_j / sd_j        dlogp/dlog_std_j = q_j^2 exp(log_std_j) / sd_j - 1
 * STATISTICS behind the gradient, grad_out[P .. P+3] (so a multi-rank caller averages gradient and KL in the one all-reduce):
 *     pi_loss = L,  approx_kl = mean(logp_old - logp),  clip_frac = mean(ratio > 1 + clip or ratio < 1 - clip),  mean_ratio = mean(ratio).
 * CRITIC.  L = mean((ret - v)^2), dL/dv = 2 (v - ret) / count;  grad_out[P] = v_loss = L.
 *
 * ARITHMETIC.  Every product of the forward pass, the backward pass and the weight gradients is an exact-f32 matrix instruction (a
 * k-ordered fmaf chain); rows are summed unscaled and 1/count is applied once, by the final reduction.  DETERMINISM.  The grid is a
 * function of count alone (ceil(count / 64) workgroups, at most 256); each workgroup writes one partial to the workspace and the
 * partials are summed in workgroup order (in f64, rounded once).  No floating-point atomics: equal inputs give equal bits.
 *
 * WHAT IS IMPLEMENTED, everything else being refused with DPENV_EINVAL and the reason in dpenv_last_error(NULL):
 *     n_layers == 4 with sizes = {in, 80, 80, 80, out}, 1 <= in <= 16;  actor (log_std = 1): 1 <= out <= 7;  critic (log_std = 0): out == 1;
 *     activation DPENV_ACT_LEAKY_RELU with 0 <= leak <= 1;  row_dtype DPENV_F32.
 *     Refused: DPENV_ACT_TANH, any other depth or width, bf16 rows. */
typedef struct dpenv_train_shape {
    uint32_t struct_size;
    int32_t n_layers;        /* dense layers */
    int32_t sizes[6];        /* in, hidden ..., out */
    int32_t activation;      /* DPENV_ACT_* */
    float leak;
    int32_t row_dtype;       /* DPENV_F32 */
    int32_t log_std;         /* 1: actor, theta ends with log_std[out];  0: critic */
} dpenv_train_shape;
/* P of the shape, or DPENV_EINVAL. */
int64_t dpenv_train_param_count(const dpenv_train_shape* shape);
/* Bytes of device workspace a gradient call on up to max_count rows needs (the per-workgroup partials).  The caller allocates;
 * a gradient call whose workspace_bytes is smaller than its count needs is refused. */
int dpenv_train_workspace_bytes(const dpenv_train_shape* shape, int32_t max_count, int64_t* bytes_out);
/* count <= 2^30.  The first gradient call of a process on a device raises the kernel's LDS limit (a function attribute, not a stream
 * operation): make that call outside a stream capture; every later call can be captured.
 * grad_out: device float[P + 4].  stop_flag: device int32 or NULL; a launch that finds it set returns at once and leaves grad_out
 * as it is (the gate of dpenv_adam_step has closed: the rest of a queued update falls through). */
int dpenv_ppo_actor_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* act, const float* adv,
                         const float* logp_old, const int32_t* idx, int32_t count, int32_t n_rows, float clip, const int32_t* stop_flag,
                         float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s);
/* grad_out: device float[P + 1]. */
int dpenv_value_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* ret, const int32_t* idx,
                     int32_t count, int32_t n_rows, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s);
/* IMITATION LOSS: the supervised gradient of the actor on demonstration rows (obs [n_rows][in], act [n_rows][out]), e.g. the obs / act
 * blocks of dpenv_controller_rollout, with an optional weight per row.  weight: device float[n_rows] or NULL = 1; w_i = weight ?
 * weight[row_i] : 1.  weight = advantage is the vanilla policy gradient, 0 masks a row, exp(A / beta) is advantage-weighted regression.
 * shape must be an actor's (log_std = 1); idx, count, n_rows, stop_flag, the workspace (dpenv_train_workspace_bytes) and the first-call
 * rule are dpenv_ppo_actor_grad's, and so are ARITHMETIC and DETERMINISM above: the same kernel body with another per-row stage.
 * Per row, with sd_j, q_j and logp as in ACTOR LOSS and sums over the out action components in j order:
 *     e_j = mu_j - act_j          se = sum_j e_j^2
 * DPENV_IMITATE_NLL.  L = -(1/count) sum_i w_i logp_i
 *     dL/dmu_j      = -w_i (q_j / sd_j) / count
 *     dL/dlog_std_j = -w_i (q_j^2 exp(log_std_j) / sd_j - 1) / count
 * DPENV_IMITATE_MSE.  L = (1/count) sum_i w_i se_i
 *     dL/dmu_j      = (2 w_i) e_j / count
 *     the log_std part of the gradient is +0.0, as bits
 * STATISTICS, grad_out[P .. P+3]:  the chosen L,  the weighted NLL (1/count) sum_i w_i (-logp_i),  the weighted MSE (1/count) sum_i w_i se_i
 * (both whichever loss is chosen),  +0.0 (reserved).  The buffer is the actor's float[P + 4].
 * The divisor is count, not sum(w).  A zero-weight row contributes exactly zero; its obs and act must still be finite.
 * Refused with DPENV_EINVAL, launching and touching nothing: an unknown loss, a critic shape, and everything dpenv_ppo_actor_grad
 * refuses for the corresponding arguments. */
#define DPENV_IMITATE_NLL 0
#define DPENV_IMITATE_MSE 1
int dpenv_imitation_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* act, const float* weight,
                         const int32_t* idx, int32_t count, int32_t n_rows, int32_t loss, const int32_t* stop_flag, float* grad_out,
                         void* workspace, int64_t workspace_bytes, dpenv_stream s);
/* ALLOCATION LOSS (additive to ABI 6): the gradient that trains the neural thrust allocator THROUGH THE FORCE MAP instead of on (u, alpha)
 * labels.  The inverse map tau -> (u, alpha) is one-to-many, so a regression on labels averages over solutions; the wrench a command
 * produces is a single-valued, differentiable function of the network's output, and the loss is the QP law's own objective evaluated
 * there: the weighted wrench residual, |F|^3 power and a penalty for thrust commands outside +-1.  It needs no labels, and its w_power is
 * the knob that turns the QP's point into a front.  No rate terms: the network has no memory of x^-.
 * The network is the fused update's actor shape {in, 80, 80, 80, 6} with in = 3 or 9 (dpenv_nn_allocator's inputs); its log_std tail is
 * carried and gets the gradient +0.0, as bits.  Rows: x [n_rows][in] the network's inputs; tau_rows [n_rows][6], columns 0..2 the demanded
 * wrench tau in N, N, Nm - UNSCALED, the scaled wrench is among the inputs - and columns 3..5 fetched but never entering a result (they
 * may hold anything, NaN included); weight [n_rows] or NULL = 1.  idx, count, n_rows, stop_flag, the workspace, the first-call rule,
 * ARITHMETIC and DETERMINISM are dpenv_imitation_grad's: the same kernel body with a fifth per-row stage.
 * Per row, in f32, in exactly this order (-ffp-contract=off: no product below is fused into a sum; the only fused operations are inside
 * sincos, which is the library's call-free polynomial sincos_lean - max abs error 9.2e-8 - as in the QP law and the neural allocation;
 * clip(v, lo, hi) = fminf(fmaxf(v, lo), hi)), with the network's output p = (u_port, u_star, u_bow, a_port, a_star, a_bow), the
 * allocator's own order, and the env order i = bow, port, star <-> j(i) = 2, 0, 1:
 *     n_i = 100 * clip(p_j, -1, 1);   K_i = n_i >= 0 ? kf_i : kr_i;   F_i = (K_i * n_i) * |n_i|          (the env's thrust law)
 *     e_i = fmaxf(|p_j| - 1, 0);      dF_i = |p_j| <= 1 ? (200 * K_i) * |n_i| : 0                          (dF_i/dp_j; 0 outside the clip)
 *     a_k = azimuth_mode == 0 ? p_{3+k} * angle_scale : azimuth[k]                                         k = port, star
 *     (s_k, c_k) = sincos(a_k);  b3_k, r_0, r_1, r_2, Js, Jp: the lines of "evaluate(x)" of the QP law above, x = (F_b, F_p, F_s, a_p, a_s) -
 *                                the bow thruster is pure sway there, column (0, 1, lx_b)
 *     Jx = (e_b * e_b + e_p * e_p) + e_s * e_s
 *     J  = 0.5 * ((Js + w_power * Jp) + w_sat * Jx)
 *     L  = (1/count) sum_rows w_row * J_row
 * Output gradient, with wr_m = w_slack_m * r_m and Jm the QP law's Jacobian (its step 1):
 *     gF_i       = ((Jm[0][i] * wr_0 + Jm[1][i] * wr_1) + Jm[2][i] * wr_2) + (1.5 * w_power) * (F_i * |F_i|)
 *     dL/dp_j(i) = w_row * (gF_i * dF_i + w_sat * copysignf(e_i, p_j)) / count
 *     ga_k       = (Jm[0][a_k] * wr_0 + Jm[1][a_k] * wr_1) + Jm[2][a_k] * wr_2,   Jm[.][a_k] = (-(F_k * s_k), F_k * c_k, F_k * (lx_k * c_k + ly_k * s_k))
 *     dL/dp_3+k  = azimuth_mode == 0 ? w_row * (angle_scale * ga_k) / count : +0.0
 *     dL/dp_5    = +0.0   (a_bow is not used: the tunnel thruster is fixed)
 * At |p_j| = 1 exactly the thrust's slope is taken (|p_j| <= 1) and e_i = 0.  1/count stays with the reduction, as for the other stages.
 * STATISTICS, grad_out[P .. P+3]:  L,  (1/count) sum w Js,  (1/count) sum w Jp,  (1/count) sum w Jx.  The buffer is the actor's float[P + 4].
 * The divisor is count, not sum(w).  A zero-weight row contributes exactly zero; its x and tau must still be finite.
 * The loss means what the deployed law does: for the p of dpenv_thrust_alloc_nn (raw_out) and azimuth_mode 0, r is the wrench
 * dpenv_thrust_map's law without inflow loss gives that call's action, minus tau.  ml4ca_amd.train.allocation_grad_ref is the host statement.
 * Refused with DPENV_EINVAL, launching and touching nothing, the field named in dpenv_last_error(NULL): a wrong struct_size, a critic
 * shape, sizes[0] outside {3, 9}, an output width other than 6, a number that is not finite, a weight (w_slack, w_power, w_sat) < 0, kf or
 * kr <= 0, an azimuth_mode other than 0 and 1, and everything dpenv_imitation_grad refuses for the arguments they share. */
typedef struct dpenv_alloc_loss {
    uint32_t struct_size;
    float w_slack[3];        /* >= 0 */
    float w_power;           /* >= 0 */
    float w_sat;             /* >= 0: the weight of the commands' excess over +-1 */
    float lx[3], ly[3];      /* lever arms [m]: bow, port, star, finite (ly[0] is not used) */
    float kf[3], kr[3];      /* thrust constants ahead / astern, > 0 */
    float angle_scale;       /* dpenv_nn_allocator's */
    int32_t azimuth_mode;    /* 0: the network's stern angles; 1: fixed at azimuth[2] (then the angle outputs get no gradient) */
    float azimuth[2];        /* port, star [rad], read in mode 1 */
} dpenv_alloc_loss;
/* The QP's default w_slack (1, 1, 1) and w_power 1, w_sat = 100, the default hull's lever arms and thrust constants
 * (dpenv_qp_allocator_defaults) and the neural allocator's angle_scale, azimuth_mode and azimuth (dpenv_nn_allocator_defaults). */
int dpenv_alloc_loss_defaults(dpenv_alloc_loss* q);
int dpenv_allocation_grad(const dpenv_train_shape* shape, const dpenv_alloc_loss* loss, const float* theta, const float* x,
                          const float* tau_rows, const float* weight, const int32_t* idx, int32_t count, int32_t n_rows,
                          const int32_t* stop_flag, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s);
/* ADAM, torch.optim.Adam's update (bias correction and eps placement included; not TF's variant).  theta, grad, m, v: device float[P],
 * 16-byte aligned.  step_counter: device int32, the steps taken so far.  With t = *step_counter + 1, every operation in f32 and
 * correctly rounded unless marked f64:
 *     pow(b, t): f64, p = 1; while t: { if (t & 1) p *= b; b *= b; t >>= 1; }
 *     step_size = lr / (float)(1 - pow(beta1, t))        bc2s = sqrt((float)(1 - pow(beta2, t)))
 *     m     = fmaf(1 - beta1, g - m, m)
 *     v     = fmaf((1 - beta2) g, g, beta2 v)
 *     denom = sqrt(v) / bc2s + eps
 *     theta = fmaf(-step_size, m / denom, theta)
 * THE GATE replaces the host's float(kl) + break (ppo.py:267-270).  gate_kl: device float or NULL; stop_flag: device int32, required
 * with gate_kl.  If gate_kl != NULL and (*stop_flag != 0 or *gate_kl > kl_limit): *stop_flag = 1 and nothing else changes.  Otherwise
 * the step is taken and *step_counter incremented.  gate_kl == NULL: no gate, stop_flag is not read. */
int dpenv_adam_step(float* theta, const float* grad, float* m, float* v, int32_t P, float lr, float beta1, float beta2, float eps,
                    int32_t* step_counter, const float* gate_kl, float kl_limit, int32_t* stop_flag, dpenv_stream s);

int dpenv_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DPENV_H */
