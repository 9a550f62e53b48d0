// dpenv_dev.h - internal contract between the host API (dpenv_api.hip, dpenv_api_free.hip) and the kernels
// (dpenv_kernels.hip) of libdpenv.so.  Not part of the public ABI (that is include/dpenv.h).
#ifndef DPENV_DEV_H
#define DPENV_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace dpenv {

constexpr int BLOCK = 64;         // threads per workgroup = one wave64; one lane per environment; LDS staging is wave-private
constexpr int RBLOCK = 64;        // rollout kernel: one wave per workgroup (wave-private LDS transposes)
constexpr int MAX_SWITCH = 8;
// slots of the public per-env controller table float[CTRL_NPARAM][n] = DPENV_CTRL_* of include/dpenv.h (dpenv_api.hip asserts it)
constexpr int CTRL_NPARAM = 32, CTRL_KP = 0, CTRL_KD = 3, CTRL_KI = 6, CTRL_ZB = 9, CTRL_TMAX = 12, CTRL_WEIGHT = 15, CTRL_LX = 20,
              CTRL_LY = 23, CTRL_KF = 26, CTRL_KR_BOW = 29, CTRL_F_EPS = 30;
constexpr int CTRL_TAB_STREAMS = 9;   // float4 streams of the packed per-env block (dpenv_control_law.h has its layout)
constexpr int64_t ctrl_tab_float4s(int n) { return ((int64_t)n + 63) / 64 * 64 * CTRL_TAB_STREAMS; }   // whole waves of 64 envs
constexpr int MAX_CLASSES = 64;

// kernel specialisations: variant x azimuth-head style (customEnv.py:11,327,351,373 + cont_ang :90)
enum { MODE_FULL = 0, MODE_SIMPLE = 1, MODE_LIMITED = 2, MODE_FINAL_WRAP = 3, MODE_FINAL_CONT = 4 };
enum { LAYOUT_AOS = 0, LAYOUT_SOA = 1 };
enum { WRAP_REFERENCE = 0, WRAP_RADIANS = 1 };
enum { DONE_TERMINAL = 1u, DONE_TIMELIMIT = 2u, DONE_FAULT = 4u };

// derived per-class parameter block (host precomputes the mass-matrix inverse)
enum {
    VD_M11 = 0, VD_M22, VD_M23, VD_INV11, VD_I22, VD_I23, VD_I33,
    VD_XU, VD_XUU, VD_YV, VD_YVV, VD_YR, VD_NV, VD_NR, VD_NRR, VD_NUV, VD_YUR,
    VD_KF, VD_KR = VD_KF + 3, VD_LX = VD_KR + 3, VD_LY = VD_LX + 3,
    VD_COUNT = VD_LY + 3
};

struct VesselDev {
    float p[VD_COUNT];
};

// Per-ENV parameter blocks (dpenv_set_vessel_params / dpenv_set_vessel_randomisation; north_star: "per-env 3x3 mass / Coriolis /
// damping blocks", SURVEY appendix D: domain randomisation).  One block = the VD_COUNT derived floats above + the raw m33 (so that the
// public parameter vector can be read back) + 2 pad = ENV_GROUPS float4.  HBM layout float4 ET[ENV_GROUPS][stride] - group g of env i at
// ET[g * stride + i], the same structure-of-float4-streams form as the state (S0..S3): a wave-level access is one coalesced 1 KiB
// dwordx4 transaction.  128 B per env-step read by dpenv_step (SURVEY 8d accounts 3 x 9 x 4 = 108 B for it: 285 B per env-step).
constexpr int VD_M33 = VD_COUNT;          // slot of the raw m33 in a per-env block
constexpr int ENV_GROUPS = 8;
constexpr int ENV_BLOCK_FLOATS = 4 * ENV_GROUPS;
static_assert(VD_COUNT + 1 <= ENV_BLOCK_FLOATS, "per-env block: derived parameters + m33 must fit eight float4");
constexpr int RAND_NPARAM = 32;           // public parameters DPENV_P_M11 .. DPENV_P_KLR_STAR (include/dpenv.h): the whole vector
// The six inflow thrust-loss coefficients (DPENV_P_KLF_* / DPENV_P_KLR_*) are NOT part of the Vessel the kernels carry in registers: they
// are two more rows of the per-env table, ET[ENV_GROUPS] = (Klf bow, port, star, Klr bow) and ET[ENV_GROUPS + 1] = (Klr port, star, -, -),
// read at the force map of an env step ONLY by the GENERAL per-env kernels (VES_ENV_RND below; the closed loop's RND instantiations and its
// one-wave forms) and only while StepArgs.loss_on says some env has one.  Every other kernel passes a compile-time "no table" and is, to
// the instruction, what it was before the loss existed: built both ways (round 5) - with the coefficients inside the Vessel the 256-env f16
// closed loop went from 76 to 100 B of scratch, behind a run-time flag in every kernel from 76 to 92 B and the headline step kernel from
// 63 to 66 VGPRs (one wave per SIMD less).  In the randomisation's draw they are groups 8 and 9.
constexpr int LOSS_GROUPS = 2;
constexpr int DRAW_GROUPS = ENV_GROUPS + LOSS_GROUPS;
constexpr int RAND_TAB_FLOATS = 64;       // device table of the randomisation: [0..31] nominal public parameters, [32..63] relative half-ranges

// where step_kernel takes a lane's vessel from (template argument VES)
enum { VES_ARGS = 0,      // one class: kernel arguments (SGPRs)
       VES_CLASS_LDS = 1, // vessel classes: [class][param] table staged into LDS as [param][class]
       VES_ENV_VGPR = 2,  // per-env blocks: eight coalesced float4 loads per lane straight into registers
       VES_ENV_LDS = 3,   // per-env blocks: LDS-DMA (global_load_lds_dwordx4) into a [group][lane] image, read back when needed (the A/B of SURVEY 7)
       VES_ENV_RND = 4,   // the GENERAL per-env form: VES_ENV_VGPR + the domain randomisation's hull re-draw in the reset paths (while StepArgs.rand_tab)
                          //   + the inflow thrust loss (while StepArgs.loss_on).  Its own instantiation: the draw's four Philox blocks cost the register
                          //   allocation of the other forms 15-70 VGPRs when they share the code, the loss 10-16
       VES_ARGS_LOSS = 5 }; // the SHARED training form (round 6): one class, hull AND the six thrust-loss coefficients as kernel arguments (StepArgs.v0,
                          //   StepArgs.kl; SGPRs; zeros = no loss: the default's rows bit for bit) + the per-episode current re-draw in the reset
                          //   paths (while StepArgs.cur_nom) - the regime the reference trains in (customEnv.py:17,26) and a randomised current at
                          //   the default's memory traffic, not at 160 B per env-step of identical per-env blocks
// StepArgs.loss_on
enum { LOSS_NONE = 0,     // no thrust loss anywhere
       LOSS_TABLE = 1,    // the per-env table's coefficients are applied: some env has one - or the host does not know yet (a setter recorded into a
                          //   graph, an answer still on its way): zero coefficients are neutral bit for bit, so assuming a loss is always right
       LOSS_SHARED = 3 }; // the single class's coefficients in StepArgs.kl (possibly all zero): only kernels instantiated for it are launched with this value

struct StepArgs {
    // library-owned state streams (see dpenv_kernels.hip header)
    float4* S0;
    float4* S1;
    float4* S2;
    float4* RF;
    int32_t* episode;
    // per-call I/O (caller-owned device memory)
    const float* action;
    const float* new_ref;
    void* obs;
    float* rew;
    uint8_t* done;
    float* parts;
    void* final_obs;
    // optional per-env inputs owned by the library
    float* cur_vc;            // present current speed / direction (read-write with drift)
    float* cur_beta;
    float* cur_vc0;           // means the drift reverts to (written by a reset when the current is randomised per episode)
    float* cur_beta0;
    uint32_t* drift_ctr;      // per-env draw counter of the drift noise
    int32_t current_drift;
    float drift_a;            // dt / tau
    float drift_sv;           // sigma_v * sqrt(2 dt / tau)
    float drift_sb;           // sigma_beta * sqrt(2 dt / tau)
    const int32_t* class_id;
    const float* class_tab;   // [n_classes][VD_COUNT]
    int32_t n_classes;
    VesselDev v0;             // class 0 by value -> SGPRs on the single-class path
    int32_t n;
    int32_t n_substeps;
    float h;
    float inv_dt;             // 1 / (n_substeps * h)
    int32_t max_ep_len;
    int32_t terminate;
    int32_t auto_reset;
    int32_t wrap_mode;
    int32_t action_layout;
    int32_t obs_layout;
    int32_t obs_bf16;
    int32_t hold_plant;
    uint32_t seed_lo, seed_hi;
    int64_t env_id_base;
    float reset_fraction;
    int32_t reset_acts;       // customEnv.py:179-188: previous thrust drawn at reset
    uint32_t* noise_ctr;      // per-env count of exploration-noise draws made so far (in-kernel sampling)
    float4* S3;               // thrust columns (o[6..8]) of the observation the LAST closed-loop launch ended with, see PolicyArgs.use_lag
    float4* env_tab;          // per-env parameter blocks ET[ENV_GROUPS][env_stride], NULL = classes / the single class (written by the kernels only
                              //   when the randomisation re-draws a hull)
    int32_t env_stride;
    int32_t loss_on;          // LOSS_* below the VES_ enum: whether / where from the kernels that carry the inflow thrust loss apply it
    const float* rand_tab;    // domain randomisation on: device float[RAND_TAB_FLOATS] (nominal | relative half-range); every reset - explicit,
                              //   auto, reset_at_end - re-draws the env's hull for the new episode, Philox keyed (seed; global env id, episode)
    // ---- round 6 (appended: the fields above keep their offsets) ----
    float kl[8];              // LOSS_SHARED: Klf bow, port, star | Klr bow, port, star of the single class (two pad)
    const float* cur_nom;     // per-episode randomisation of the current on (dpenv_set_current_randomisation): device float[2][cur_nom_stride], the
                              //   nominal V_c | beta_c of every env; every reset draws the new episode's current around them (current_redraw)
    int32_t cur_nom_stride;
    float cur_range_v;        // half-ranges of the draw: V_c [m/s], beta_c [rad]
    float cur_range_b;
};

// fused T-step rollout (dpenv_rollout)
struct RolloutArgs {
    int32_t T;
    const float* actions;     // [T][n][A] or [T][A][n]
    void* obs;                // [T][n][OD] or [T][OD][n]
    float* rew;               // [T][n]
    uint8_t* done;            // [T][n]
    int32_t n_switch;
    int32_t switch_step[MAX_SWITCH];
    const float* refs;        // [n_switch][3][n]
};

// actor-critic evaluated in-kernel (dpenv_policy.hip, dpenv_policy_x.hip)
struct PolicyArgs {
    const uint4* frags;       // LDS image, first part: [2 nets][nent] x 16 B MFMA A-operand fragment entries (f16), actor then critic;
                              // split arithmetic: followed by the same for the LOW parts of the weights (W = hi + lo)
    const float* bias;        // [2][nblk][32] f32: bias tiles of the row-blocks after the first layer, accumulator layout
    const float* consts;      // [24] f32 written by the packing kernel: exp(log_std) (core.py:84) | 1 / (exp(log_std) + 1e-8)
                              // (core.py:45) | -log_std - 0.5 log(2 pi) (core.py:45), 8 slots each
    int32_t nent;             // 16-byte entries of one weight image of one network (compact fragment layout, FragAddr in dpenv_policy_dev.h)
    int32_t nblk;             // bias blocks per net = 3 (n_hidden - 1) + 1
    int32_t ks;               // k-steps of 16 hidden features: 5 (width <= 80) or 6 (width <= 96)
    int32_t act;              // hidden activation: 0 leaky-relu(leak), 1 tanh
    int32_t ws;               // rollout launch form: 0 = one wave per 64 envs, 1 = an env wave and a network wave per 64 envs (policy_rollout_ws_kernel)
    int32_t split;            // 1 = split-f16 arithmetic (DPENV_POLICY_F32): weights and activations as hi + lo f16 pairs
    int32_t critic_f16;       // with split: the critic is evaluated in f16 arithmetic on the high image (DPENV_POLICY_F32_ACTOR)
    int32_t n_hidden;
    float leak;               // leaky-relu slope (0.2)
    int32_t sample;           // 1: noise == NULL means "draw the exploration noise in the kernel" (policy_noise), not "a = mu"
    int32_t reset_at_end;     // 1: every env is cut and re-drawn after step T-1 (ppo.py:305-322), boot = V(last obs) unless terminal
    int32_t use_lag;          // 1: the state was last touched by a closed-loop launch: its first policy input takes the thrust columns
                              // from S3.  The observation of step t carries the thrust command of step t-1 (customEnv.py:196-205: state_ext is
                              // filled BEFORE prev_thrust is updated, :126), the state block only the command of step t; without the lagged
                              // copy a launch that continues an episode would start from an observation the reference never shows its policy.
    int32_t ws_groups;        // two-wave form: 4 = 512-thread workgroups of 256 envs, 2 = 256-thread workgroups of 128 envs (a SIMD per wave)
    // rollout I/O
    int32_t T;
    const float* noise;       // [T][n][A] standard normal draws, NULL = deterministic (a = mu)
    void* obs_out;            // [T][n][OD]  policy input of step t   (ppo.py:298 'o'); f32 or bf16
    float* act_out;           // [T][n][A]   action taken             ('a')
    float* rew;               // [T][n]
    float* val;               // [T][n]      V(o_t)                   ('v_t')
    float* logp;              // [T][n]                               ('logp_t')
    uint8_t* done;            // [T][n]
    float* boot;              // [T][n]      bootstrap value where a path ends (ppo.py:311), else 0
    void* last_obs;           // [n][OD]     policy input of the next launch; f32 or bf16
    float* last_val;          // [n]
    int32_t n_switch;
    int32_t switch_step[MAX_SWITCH];
    const float* refs;
};

// the deployed RL node's body-frame integral action in the closed loop (dpenv_set_integral_action; rl_allocator.py:252-273 of the
// reference): a separate argument of the *_integ kernels only, so the kernels without it keep their argument block
struct IntegArgs {
    float4* state;            // [n] I[0..2] | count of control steps since the last (re)arrival (int32 bits)
    float* out;               // [T][n][3] the I added to obs[t], or NULL
    float gain[3], bound[3], box[3];
    float step_s;
    int32_t dwell;            // D: the smallest count with D * dt > dwell_s
};

// the setpoint reference filter of the deployed controller in the closed loop (dpenv_set_reference_filter; include/dpenv.h has the law): a
// separate argument of the *_reff kernels only, like IntegArgs
struct FilterArgs {
    float4* state;            // [3][n]: axis j (N, E, psi) of env i at state[j * n + i] = (pos, vel, acc, target)
    float* out;               // [T][n][3] the eta_d obs[t] was formed against, or NULL
    float phi[3][9];          // Phi_j row-major, f32 from the f64 zero-order hold (dpenv_reference_filter_coeffs)
    float gam[3][3];          // Gamma_j
};

// the baseline DP controller in the closed loop (dpenv_set_dp_controller / dpenv_controller_rollout; include/dpenv.h has the law,
// dpenv_control.hip the kernels): the law's numbers, its per-env state and the I/O of one launch
struct ControlArgs {
    float4* z;                // [n] the error integral z[0..2] (one pad)
    float kp[3], kd[3], ki[3], zb[3], tmax[3];
    float G[5][3];            // weighted pseudo-inverse of the extended-thrust matrix, rows Fy_bow, Fx_port, Fy_port, Fx_star, Fy_star
    float kf[3], kr_bow;      // bow, port, star ahead; bow astern
    float f_eps;
    float dt;                 // n_substeps * substep_dt in f32
    int32_t use_lag;          // as PolicyArgs.use_lag: the first observation takes its thrust columns from S3
    // rollout I/O
    int32_t T;
    void* obs;                // [T][n][9]  controller input of step t; f32 or bf16
    float* act;               // [T][n][7]  its action
    float* rew;               // [T][n]
    uint8_t* done;            // [T][n]
    void* last_obs;           // [n][9]     controller input of the next launch
    int32_t n_switch;
    int32_t switch_step[MAX_SWITCH];
    const float* refs;        // [n_switch][3][n]
};

// the rate-limited QP thrust allocation (dpenv_thrust_alloc_qp; include/dpenv.h has the law, dpenv_qp_law.h its device text, dpenv_control.hip
// the kernel): the law's numbers in env order bow, port, star, and the I/O of one call
struct QpArgs {
    float ws[3], wp, wda, wdf;  // slack, power, azimuth-change and force-change weights
    float fmax[3];
    float dF[3], da[2];         // per control step: force_rate * dt, azimuth_rate * dt, each one f32 product formed on the host
    float lx[3], ly[3], kf[3], kr[3];
    int32_t iters;              // 1 .. QP_MAX_ITERS
};
constexpr int QP_MAX_ITERS = 32;
// The numbers of ONE env, in registers: what the *_qp_tab kernels fly instead of QpArgs' shared set while a per-env QP table is in force
// (dpenv_set_qp_allocator_table, dpenv_thrust_alloc_qp_table).  QpArgs' members under QpArgs' names, so qp_allocate reads either; iters
// is the call's (wave-uniform).
struct QpLane {
    float ws[3], wp, wda, wdf;
    float fmax[3];
    float dF[3], da[2];
    float lx[3], ly[3], kf[3], kr[3];
    int32_t iters;
};
// slots of the public per-env QP table float[QP_NPARAM][n] = DPENV_QP_* of include/dpenv.h (dpenv_api.hip asserts it), in the order of
// dpenv_qp_allocator's fields; QP_NREAD of them are read
constexpr int QP_NPARAM = 32, QP_WSLACK = 0, QP_WPOWER = 3, QP_WDALPHA = 4, QP_WDFORCE = 5, QP_FMAX = 6, QP_FRATE = 9, QP_ARATE = 12,
              QP_LX = 14, QP_LY = 17, QP_KF = 20, QP_KR = 23, QP_NREAD = 26;
constexpr int QP_TAB_STREAMS = 7;     // float4 streams of the packed per-env QP block (dpenv_qp_law.h has its layout): 112 B per env
constexpr int64_t qp_tab_float4s(int n) { return ((int64_t)n + 63) / 64 * 64 * QP_TAB_STREAMS; }   // whole waves of 64 envs
// the allocation as the allocation stage of the baseline's closed loop (dpenv_set_qp_allocator): the numbers and the per-env thruster
// state, a separate argument of controller_rollout_qp_kernel only
struct QpRollout {
    QpArgs q;
    float* state;               // [5][n], dpenv_get_qp_allocator_state's layout
};
struct QpAllocIO {
    const float* tau;           // [3][n]
    const float* state_in;      // [5][n] F_bow, F_port, F_star, a_port, a_star, or NULL = 0
    float* state_out;           // [5][n] or NULL; may be state_in
    float* act;                 // [n][7]
    float* cost;                // [n] the final objective, or NULL
    int32_t n;
};

// the neural thrust allocation (dpenv_thrust_alloc_nn / dpenv_set_nn_allocator; include/dpenv.h has the law, dpenv_nn_law.h its device
// text, dpenv_control_nn.hip the kernels): a dense network in -> H -> ... -> H -> 6 and the constants around it.  W[l] is [in_l][ld_l]
// row-major: the caller's arrays in place (ld_l = the layer's width) or the library's zero-padded image (ld_l = the width rounded up to
// NN_CHUNK, b[l] padded likewise); every pointer is a DEVICE pointer.
constexpr int NN_MAX_H = 96, NN_CHUNK = 16, NN_MAX_LAYERS = 5;
constexpr int nn_pad(int w) { return (w + NN_CHUNK - 1) / NN_CHUNK * NN_CHUNK; }
constexpr int NN_IMAGE_FLOATS = NN_MAX_LAYERS * (NN_MAX_H * NN_MAX_H + NN_MAX_H);   // the largest image: what a handle allocates once
struct NnArgs {
    const float* W[NN_MAX_LAYERS];
    const float* b[NN_MAX_LAYERS];
    int32_t n_layers, in_dim, H;    // dense layers 2..5, inputs 3 or 9, hidden width 1..NN_MAX_H; the last layer has 6 outputs
    float leak;
    float in_const[6], tau_scale[3], angle_scale;
    int32_t azimuth_mode;
    float azimuth[2];
};
// what the launchers of the units that evaluate the network (dpenv_control_nn.hip, dpenv_label_nn.hip) refuse of a shape
inline bool nn_shape_ok(int n_layers, int in_dim, int H)
{
    return n_layers >= 2 && n_layers <= NN_MAX_LAYERS && (in_dim == 3 || in_dim == 9) && H >= 1 && H <= NN_MAX_H;
}
// ... and of its arrays: every launcher that is handed an NnArgs (or an NnPack, whose source side has the same members) asks this, once
template <typename A> bool nn_args_ok(const A& a)
{
    if (!nn_shape_ok(a.n_layers, a.in_dim, a.H)) return false;
    for (int l = 0; l < a.n_layers; ++l)
        if (!a.W[l] || !a.b[l]) return false;
    return true;
}
// the allocation as the allocation stage of the baseline's closed loop (dpenv_set_nn_allocator): a separate argument of
// controller_rollout_nn_kernel only; the weights are the handle's padded image
struct NnRollout {
    NnArgs a;
};
// the packing of the zero-padded image of K networks from DEVICE arrays (dpenv_set_nn_allocator, K = 1, and
// dpenv_set_nn_allocator_population with device_pointers = 1): network k of src layer l at W[l] + k in out and b[l] + k out, in place; of
// dst at dW[l] + k in ld and db[l] + k ld, the image's layers
struct NnPack {
    const float* W[NN_MAX_LAYERS];
    const float* b[NN_MAX_LAYERS];
    float* dW[NN_MAX_LAYERS];
    float* db[NN_MAX_LAYERS];
    int32_t n_layers, in_dim, H;
    int32_t K;
};
// K networks of one shape, one per run of waves (dpenv_set_nn_allocator_population / dpenv_thrust_alloc_nn_population;
// dpenv_control_nn_pop.hip): a.W[l] is [K][in_l][ld_l] and a.b[l] [K][ld_l] - network 0's addresses, the others behind it layer by layer -
// and wave w of the launch (workgroup w: 64 envs) takes network ((wave_base + w) / waves_per_net) % K.  The index is a function of
// blockIdx alone, so the wave's addresses stay wave-uniform and the weights keep arriving by scalar loads.
struct NnPop {
    NnArgs a;
    int32_t K, waves_per_net;       // K >= 1; envs_per_net / 64 >= 1
    uint32_t wave_base;             // (env_id_base / 64) mod (K waves_per_net), which the host keeps below 2^31; 0 for the handle-free map
};

// device-side weight packing (pack_policy_kernel): one dense network, DEVICE pointers
struct PackNet {
    const float* W[5];        // W[l][in][out] row-major (tf.layers.dense kernel layout)
    const float* b[5];
    int32_t n_layers, in_dim, H, out_dim;
};

constexpr int POLICY_WS_MAILBOX_BYTES = 4 * (64 * 9 * 5 + 64 * 4 + 64) * 4;   // two-wave form: four groups of mailboxes
constexpr int POLICY_WS_MAILBOX_X_BYTES = 4 * (64 * 9 * 4 + 64 * 4 + 64) * 4; // the same for the split arithmetics (no row staging area)
constexpr int PREC_F16 = 0, PREC_F32 = 1, PREC_F32_ACTOR = 2;                 // = DPENV_POLICY_* of include/dpenv.h
constexpr int POLICY_STAGING_BYTES = 4 * 64 * 9 * 4;                           // one-wave form: four wave-private row areas

// =============================================================================================
//  launch layer: run-time axes -> template instantiations
// =============================================================================================
// Each with_* helper calls f with a std::integral_constant of the run-time value; an unknown value is hipErrorInvalidValue.
// -DDPENV_DEV_FAST (development builds only, never shipped) narrows the axes here and nowhere else: each helper then admits the
// shipped value alone - final variant / continuous angles, extended state, hidden width <= 80 leaky-relu, obs 9 / act 7.
template <int V> using Int = std::integral_constant<int, V>;

template <typename F> hipError_t with_mode(int mode, F&& f)
{
    switch (mode) {
#ifndef DPENV_DEV_FAST
    case MODE_FULL: return f(Int<MODE_FULL>{});
    case MODE_SIMPLE: return f(Int<MODE_SIMPLE>{});
    case MODE_LIMITED: return f(Int<MODE_LIMITED>{});
    case MODE_FINAL_WRAP: return f(Int<MODE_FINAL_WRAP>{});
#endif
    case MODE_FINAL_CONT: return f(Int<MODE_FINAL_CONT>{});
    }
    return hipErrorInvalidValue;
}

template <typename F> hipError_t with_ext(int ext, F&& f)
{
    if (ext) return f(std::true_type{});
#ifndef DPENV_DEV_FAST
    return f(std::false_type{});
#else
    return hipErrorInvalidValue;
#endif
}

template <typename F> hipError_t with_mode_ext(int mode, int ext, F&& f)
{
    return with_mode(mode, [&](auto M) { return with_ext(ext, [&](auto E) { return f(M, E); }); });
}

// KA = ks + 16 act: hidden width <= 80 (ks 5) or <= 96 (ks 6) x leaky-relu / relu (act 0) or tanh (act 1)
template <typename F> hipError_t with_ka(const PolicyArgs& pa, F&& f)
{
    if ((pa.ks != 5 && pa.ks != 6) || (pa.act != 0 && pa.act != 1)) return hipErrorInvalidValue;
    switch (pa.ks + 16 * pa.act) {
    case 5: return f(Int<5>{});
#ifndef DPENV_DEV_FAST
    case 6: return f(Int<6>{});
    case 21: return f(Int<21>{});
    case 22: return f(Int<22>{});
#endif
    }
    return hipErrorInvalidValue;
}

template <typename F> hipError_t with_mode_ext_ka(int mode, int ext, const PolicyArgs& pa, F&& f)
{
    return with_mode_ext(mode, ext, [&](auto M, auto E) { return with_ka(pa, [&](auto K) { return f(M, E, K); }); });
}

// the (obs dim, act dim) pairs of the env variants (dpenv_obs_dim / dpenv_act_dim): the standalone forward kernels' shapes
template <typename F> hipError_t with_obs_act(int od, int adim, F&& f)
{
    if (od == 9 && adim == 7) return f(Int<9>{}, Int<7>{});
#ifndef DPENV_DEV_FAST
    if (od == 9 && adim == 5) return f(Int<9>{}, Int<5>{});
    if (od == 9 && adim == 6) return f(Int<9>{}, Int<6>{});
    if (od == 6 && adim == 7) return f(Int<6>{}, Int<7>{});
    if (od == 6 && adim == 5) return f(Int<6>{}, Int<5>{});
    if (od == 6 && adim == 6) return f(Int<6>{}, Int<6>{});
    if (od == 6 && adim == 3) return f(Int<6>{}, Int<3>{});
#endif
    return hipErrorInvalidValue;
}

template <typename F> hipError_t with_ves(int ves, F&& f)
{
    switch (ves) {
    case VES_ARGS: return f(Int<VES_ARGS>{});
    case VES_CLASS_LDS: return f(Int<VES_CLASS_LDS>{});
    case VES_ENV_VGPR: return f(Int<VES_ENV_VGPR>{});
    case VES_ENV_LDS: return f(Int<VES_ENV_LDS>{});
    case VES_ENV_RND: return f(Int<VES_ENV_RND>{});
    case VES_ARGS_LOSS: return f(Int<VES_ARGS_LOSS>{});
    }
    return hipErrorInvalidValue;
}

// a launch with dynamic LDS above the default limit: raise the kernel's limit, then launch
template <typename... P, typename... A>
hipError_t launch_with_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args)
{
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

// ---- the instantiation set of each kernel family, stated once: its launcher instantiates what these admit, and the host routes by them ----
// step_kernel, rollout_kernel / rollout_ws_kernel, reset_kernel: every MODE x EXT (x VES), the T-step kernels' vessel source mapped as follows
constexpr int rollout_ves(int ves) { return ves == VES_ENV_LDS ? VES_ENV_VGPR : ves; }   // a T-step kernel's staging area is the register file
// one-wave closed loop (f16 and split arithmetics), standalone forward: every MODE x EXT x KA; with the integral action:
constexpr bool integ_one_wave(int mode, bool ext, int ka)
{
    return (mode == MODE_FINAL_CONT || mode == MODE_LIMITED || mode == MODE_FULL) && ext && ka == 5;
}
// two-wave closed loop (every MODE x EXT): leaky-relu / relu in every arithmetic and geometry, tanh in f16 with four groups only
constexpr bool ws_has(int ka, int prec, int groups) { return ka < 16 || (prec == PREC_F16 && groups == 4); }
// its general per-env (RND) and shared training (SLOSS) forms: the shipped training configuration (train.py:47-54) with leaky-relu / relu
constexpr bool ws_general(int mode, bool ext, int ka) { return mode == MODE_FINAL_CONT && ext && ka < 16; }
// its integral action: the final variant / continuous angles, extended state, leaky-relu / relu of width <= 80
constexpr bool ws_integ(int mode, bool ext, int ka) { return mode == MODE_FINAL_CONT && ext && ka == 5; }
// the setpoint reference filter (FilterArgs): the integral action's set in both families, instantiated for the filter alone and for the
// filter with the integral action
constexpr bool reff_one_wave(int mode, bool ext, int ka) { return integ_one_wave(mode, ext, ka); }
constexpr bool ws_reff(int mode, bool ext, int ka) { return ws_integ(mode, ext, ka); }
// the baseline controller's closed loop (controller_rollout_kernel): the final variant with continuous angles and the extended state, with
// and without the reference filter, one instantiation per vessel source below - vessel classes have none
constexpr bool control_has(int mode, bool ext) { return mode == MODE_FINAL_CONT && ext; }
template <typename F> hipError_t with_control_ves(int ves, F&& f)
{
    switch (ves) {
    case VES_ARGS: return f(Int<VES_ARGS>{});
#ifndef DPENV_DEV_FAST
    case VES_ARGS_LOSS: return f(Int<VES_ARGS_LOSS>{});
    case VES_ENV_VGPR: return f(Int<VES_ENV_VGPR>{});
    case VES_ENV_RND: return f(Int<VES_ENV_RND>{});
#endif
    }
    return hipErrorInvalidValue;
}
// the vessel source must match the arguments (as launch_rollout's): a per-env form needs the table, VES_ARGS_LOSS and only it reads
// StepArgs.kl.  What every launcher of that closed loop (dpenv_control.hip, dpenv_control_nn.hip, dpenv_control_nn_pop.hip) asks first.
inline bool control_ves_ok(int ves, const StepArgs* a)
{
    if ((ves == VES_ENV_VGPR || ves == VES_ENV_RND) && !a->env_tab) return false;
    if ((ves == VES_ARGS_LOSS) != (a->loss_on == LOSS_SHARED)) return false;
    return true;
}
// waves per 64 envs of the two-wave form: an env and a network wave, plus a critic wave of its own (ROLES = 3) in the 128-env geometry
// for the two split arithmetics, all exact and exact actor - not f16 (dpenv_policy_ws.h has the measurements)
constexpr int ws_roles(int prec, int groups) { return (groups == 2 && prec != PREC_F16) ? 3 : 2; }

// ---- the streaming score card (dpenv_score_*; kernels in dpenv_score_dev.h and dpenv_score_wear.hip): the arguments of one accumulate call ----
struct ScoreArgs {
    uint4* state;
    const void* obs;            // [T][n][obs_stride] f32 or bf16, columns 0..2 read
    const float* act;           // [T][n][act_stride], columns 0..2 read
    const float* rew;           // [T][n]
    const uint8_t* done;        // [T][n]
    const float* integ;         // [T][n][3]
    int T, n, obs_stride, act_stride, cut_at_end;
    float dt;
    float norm[3], coeff[3], rps[3];
};

// ---- the baseline controller's law on rows some other flight wrote (dpenv_controller_label; the kernel is dpenv_label.hip's): the I/O of
// one labelling scan.  The law's numbers travel as ControlArgs (its z and rollout I/O are not read) or as the packed per-env table.
struct LabelArgs {
    const void* obs;            // [T][n][9] f32 or bf16, columns 0..5 read
    const uint8_t* done;        // [T][n] or NULL
    const float* z_in;          // [3][n] or NULL = 0
    float* z_out;               // [3][n] or NULL; may be z_in
    float* act;                 // [T][n][7]
    int T, n;
};
// the same scan with the rate-limited QP allocation behind the PID lines (dpenv_controller_label_qp): the thruster state x travels beside
// z.  The QP's numbers travel as QpArgs, the PID's as ControlArgs (G and the thrust constants are not read) or as the packed table.
struct LabelQpArgs {
    const void* obs;            // [T][n][9] f32 or bf16, columns 0..5 read
    const uint8_t* done;        // [T][n] or NULL
    const float* z_in;          // [3][n] or NULL = 0
    float* z_out;               // [3][n] or NULL; may be z_in
    const float* x_in;          // [5][n] (QpRollout.state's layout) or NULL = 0
    float* x_out;               // [5][n] or NULL; may be x_in
    float* act;                 // [T][n][7]
    float* cost;                // [T][n] the final objective of each row's solve, or NULL
    int T, n;
};
// what dpenv_controller_label_qp_ex adds to that scan: the thruster state taken from the FLOWN action rows, and one QP allocator per env
// read from the public table by the lane itself (qp_lane_from_row)
struct LabelQpExArgs {
    const float* flown;         // [T][n][7] the executed actions, or NULL = the expert's own recursion
    const float* qp_table;      // PUBLIC table float[QP_NPARAM][n], or NULL = QpArgs' shared numbers
    uint8_t* refused;           // [n] or NULL; with qp_table
    int32_t iters;              // with qp_table: 1 .. QP_MAX_ITERS
};
// the scan with the neural allocation behind the PID lines (dpenv_controller_label_nn; the kernel is dpenv_label_nn.hip's): the law has no
// state, so only z travels.  The network's numbers travel as NnArgs (not read when act is NULL), the PID's as ControlArgs or the table.
struct LabelNnArgs {
    const void* obs;            // [T][n][9] f32 or bf16, columns 0..5 read
    const uint8_t* done;        // [T][n] or NULL
    const float* z_in;          // [3][n] or NULL = 0
    float* z_out;               // [3][n] or NULL; may be z_in
    float* act;                 // [T][n][7], or NULL = the wrench-only scan: the network is not evaluated
    float* raw;                 // [T][n][6] the network's six outputs, or NULL; with act
    float* tau;                 // [T][n][3] the PID's clipped wrench, or NULL
    int T, n;
};

// ---- launchers: called by the host units (dpenv_api.hip, dpenv_api_free.hip), defined by the translation unit that owns the kernels; not exported from libdpenv.so ----
namespace __attribute__((visibility("hidden"))) dev {
// dpenv_kernels.hip.  ves: VES_* (where the vessel of a lane comes from)
hipError_t launch_step(const StepArgs* a, int mode, int ext, int ves, int reset_wave, hipStream_t s);
hipError_t launch_rollout(const StepArgs* a, const RolloutArgs* ra, int mode, int ext, int ves, int two_wave, hipStream_t s);
hipError_t launch_reset(const StepArgs* a, int mode, int ext, const uint8_t* mask, const float* init, const float* ref, hipStream_t s);
hipError_t launch_get_state(const StepArgs* a, float* st, int32_t* ctr, hipStream_t s);
hipError_t launch_set_state(const StepArgs* a, const float* st, const int32_t* ctr, hipStream_t s);
// raw public parameters -> per-env blocks: raw[p * p_stride + i * i_stride] (SoA block: p_stride = n, i_stride = 1; one vector for every env:
// p_stride = 1, i_stride = 0); and back (out[p * n + i])
// tab: ET[DRAW_GROUPS][stride] (vessel block + thrust-loss rows); loss_flag (device word, may be NULL) is OR-ed with 1 if any env's
// thrust-loss coefficient is non-zero
hipError_t launch_pack_env_vessels(const float* raw, int64_t p_stride, int64_t i_stride, float4* tab, uint32_t* loss_flag, int stride, int n,
                                   hipStream_t s);
hipError_t launch_unpack_env_vessels(const float4* tab, int stride, float* out, int n, hipStream_t s);
hipError_t launch_thrust_map(const VesselDev* vd, const float* n_pct, const float* alpha, float* tau, int n, hipStream_t s);
int64_t gae_workspace_bytes(int n);
hipError_t launch_gae(const float* rew, const float* val, const uint8_t* end, const float* boot, const float* last_val, int T, int n,
                      float gamma, float lam, float* adv, float* ret, double* workspace, double* stats, hipStream_t s);
// the score card: state / workspace sizes, the block scan (obs_bf16: the obs rows are bf16), the [13][n] read-out and the two-stage summary
int64_t score_state_bytes(int n);
int64_t score_summary_workspace_bytes(int n);
hipError_t launch_score(const ScoreArgs* a, int obs_bf16, hipStream_t s);
hipError_t launch_score_read(const void* state, int n, double* out, hipStream_t s);
hipError_t launch_score_summary(const void* state, int n, double* out, double* workspace, hipStream_t s);
// dpenv_score_wear.hip: the score scan with the wear state (IADC) beside the score state, one pass over the rows (mode: MODE_* of the
// variant whose command decode the azimuths take; a->act must not be NULL), the [4][n] read-out and the two-stage summary of the wear slots
int64_t score_wear_state_bytes(int n);
int64_t score_wear_summary_workspace_bytes(int n);
hipError_t launch_score_wear(const ScoreArgs* a, void* wear, int obs_bf16, int mode, hipStream_t s);
hipError_t launch_score_wear_read(const void* wear, int n, double* out, hipStream_t s);
hipError_t launch_score_wear_summary(const void* wear, int n, double* out, double* workspace, hipStream_t s);
hipError_t launch_sum(const float* x, int64_t count, const float* mean, float* out, hipStream_t s);
hipError_t launch_adv_apply(float* x, int64_t count, const float* mean, const float* std, const double* stats, double total_count,
                            hipStream_t s);
// dpenv_policy.hip (f16) and dpenv_policy_x.hip (split arithmetics): weight packing, standalone forward, one-wave closed loop;
// ia != NULL: the closed loop with the integral action; fa != NULL: with the reference filter (and ia, if not NULL)
hipError_t launch_pack_policy(const PackNet* pi, const PackNet* v, const float* log_std, int adim, int ks, int nent, int nblk, int split,
                              void* frags, float* bias, float* consts, hipStream_t s);
hipError_t launch_policy_forward(const PolicyArgs* pa, int od, int adim, const float* obs, float* mu, float* v, int n, hipStream_t s);
hipError_t launch_policy_forward_x(const PolicyArgs* pa, int od, int adim, const float* obs, float* mu, float* v, int n, hipStream_t s);
hipError_t launch_policy_rollout(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                 hipStream_t s);
hipError_t launch_policy_rollout_x(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                   hipStream_t s);
hipError_t launch_integ_clear(float4* state, const uint8_t* mask, int n, hipStream_t s);
hipError_t launch_integ_state_io(float4* state, float* I, int32_t* c, int n, int write, hipStream_t s);
// the reference filter's state: at rest on the env's reference RF[i].xyz (mask NULL = every env); and the checkpoint path
// (x float[9][n] | r float[3][n], either may be NULL)
hipError_t launch_reff_rest(const float4* RF, float4* state, const uint8_t* mask, int n, hipStream_t s);
hipError_t launch_reff_state_io(float4* state, float* x, float* r, int n, int write, hipStream_t s);
// dpenv_control.hip: the baseline controller's closed loop (fa != NULL: with the reference filter; ves as
// launch_rollout's, classes excluded), its state (op 0 read into ext float[3][n], 1 write from it, 2 zero the envs of mask) and the
// stateless allocation tau [3][n] -> action [n][7]
// tab: the packed per-env block launch_pack_controllers wrote (every env flies its own row: the *_tab kernels), or NULL (ca's shared numbers)
// qr: the QP allocation in place of the pseudo-inverse (tab NULL; VES_ARGS and VES_ARGS_LOSS only), or NULL
// qtab (with qr): the packed per-env QP block launch_pack_qp_table wrote - every env flies its own row (the *_qp_tab kernels) and of qr->q
// only iters is read - or NULL (qr->q's shared numbers)
hipError_t launch_controller_rollout(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const float4* tab, const QpRollout* qr,
                                     const float4* qtab, int ves, hipStream_t s);
// the public table float[CTRL_NPARAM][n] -> the packed block of ctrl_tab_float4s(n) float4; refused: uint8 [n] or NULL (dpenv_set_dp_controller_table)
hipError_t launch_pack_controllers(const float* table, float4* tab, uint8_t* refused, int n, hipStream_t s);
hipError_t launch_control_state(float4* z, float* ext, const uint8_t* mask, int n, int op, hipStream_t s);
hipError_t launch_thrust_alloc(const ControlArgs* ca, const float* tau, float* action, int n, hipStream_t s);
// dpenv_label.hip: the law scanned over the T rows of a block, one lane per env (tab as launch_controller_rollout's; obs_bf16: the obs rows
// are bf16); reads ca's numbers and dt only
hipError_t launch_controller_label(const ControlArgs* ca, const LabelArgs* la, const float4* tab, int obs_bf16, hipStream_t s);
// ... with the QP allocation of qa in place of the pseudo-inverse; of ca (or tab) the PID's numbers and dt only
hipError_t launch_controller_label_qp(const ControlArgs* ca, const QpArgs* qa, const LabelQpArgs* la, const float4* tab, int obs_bf16, hipStream_t s);
// ... with xa's flown rows and / or per-env QP table (at least one of the two; qa is not read with a table)
hipError_t launch_controller_label_qp_ex(const ControlArgs* ca, const QpArgs* qa, const LabelQpArgs* la, const LabelQpExArgs* xa, const float4* tab,
                                         int obs_bf16, hipStream_t s);
// dpenv_control.hip: one control step of the QP allocation for n envs, one lane per env
hipError_t launch_qp_alloc(const QpArgs* qa, const QpAllocIO* io, hipStream_t s);
// the zeroing of the closed loop's QP thruster state for the envs of mask (NULL = every env)
hipError_t launch_qp_state_clear(float* state, const uint8_t* mask, int n, hipStream_t s);
// the public QP table float[QP_NPARAM][n] -> the packed block of qp_tab_float4s(n) float4, dF and da formed with dt; refused: uint8 [n] or
// NULL (dpenv_set_qp_allocator_table)
hipError_t launch_pack_qp_table(const float* table, float4* qtab, uint8_t* refused, float dt, int n, hipStream_t s);
// launch_qp_alloc with row i of the PUBLIC table on env i, checked by the lane itself (dpenv_thrust_alloc_qp_table)
hipError_t launch_qp_alloc_tab(const float* table, int iters, float dt, const QpAllocIO* io, uint8_t* refused, hipStream_t s);
// dpenv_control_nn.hip: the neural allocation for n envs, one lane per env, weights read in place (raw: [n][6] the network's outputs, or NULL)
hipError_t launch_nn_alloc(const NnArgs* na, const float* tau, float* action, float* raw, int n, hipStream_t s);
// the baseline's closed loop with the neural allocation behind the PID lines (launch_controller_rollout's a, ca, fa and ves; every
// vessel source of with_control_ves); nr->a points into the padded image launch_nn_pack or the host wrote
hipError_t launch_controller_rollout_nn(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const NnRollout* nr, int ves, hipStream_t s);
// dpenv_control_nn_pop.hip: launch_nn_alloc and launch_controller_rollout_nn with K networks of one shape, one per waves_per_net waves (NnPop)
hipError_t launch_nn_alloc_pop(const NnPop* np, const float* tau, float* action, float* raw, int n, hipStream_t s);
hipError_t launch_controller_rollout_nn_pop(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const NnPop* np, int ves, hipStream_t s);
// the caller's DEVICE arrays -> the zero-padded image of np->K networks (one network: K = 1), one launch
hipError_t launch_nn_pack(const NnPack* np, hipStream_t s);
// dpenv_label_nn.hip: launch_controller_label's scan with the neural allocation in place of the pseudo-inverse and, if la->tau, the PID's
// wrench per row; na: NULL exactly when la->act is NULL; padded: na's W and b are the zero-padded image, else arrays read in place
hipError_t launch_controller_label_nn(const ControlArgs* ca, const NnArgs* na, const LabelNnArgs* la, const float4* tab, int obs_bf16, int padded,
                                      hipStream_t s);
// two-wave closed loop, dpenv_policy_ws.h; one arithmetic per translation unit: dpenv_policy_ws.hip PREC_F16, dpenv_policy_xws1.hip
// PREC_F32, dpenv_policy_xws2.hip PREC_F32_ACTOR
template <int PREC>
hipError_t launch_policy_rollout_ws(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                    hipStream_t s);
}  // namespace dev

}  // namespace dpenv

#endif
