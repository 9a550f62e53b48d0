// dpenv_train_dev.h - the training family (include/dpenv.h: dpenv_ppo_actor_grad, dpenv_value_grad, dpenv_adam_step): the shapes the
// gradient kernel is built for, the layout of a flat parameter vector, the argument blocks and the launchers of dpenv_train.hip.
// Shared by dpenv_train.hip (the kernels) and dpenv_api_free.hip (the entry points); hidden like the launchers of dpenv_dev.h.
#ifndef DPENV_TRAIN_DEV_H
#define DPENV_TRAIN_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dpenv {

// ---- the one family of shapes the kernel implements: in -> 80 -> 80 -> 80 -> out, in <= 16, out <= 7 (actor) or 1 (critic) ----
constexpr int TR_H = 80;           // hidden width
constexpr int TR_PAD = 16;         // the input and the output layer are padded to one 16-wide MFMA tile
constexpr int TR_ROWS = 64;        // rows per tile: four waves x 16 rows in the forward / backward phase, K = 64 in the dW phase
constexpr int TR_MAX_WG = 256;     // workgroups at most (one per CU of an MI355X); the grid is min(tiles, TR_MAX_WG): a function of count alone
constexpr int TR_NSTAT_ACTOR = 4;  // pi_loss, approx_kl, clip_frac, mean_ratio; the imitation loss: L, weighted NLL, weighted MSE, 0
constexpr int TR_NSTAT_CRITIC = 1; // v_loss

// flat theta: W0 [in][80] | b0 [80] | W1 [80][80] | b1 | W2 [80][80] | b2 | W3 [80][out] | b3 [out] | (actor) log_std [out]
struct TrainLayout {
    int in_dim, out_dim, actor;
    int w[4], b[4], ls, P;
};
inline TrainLayout train_layout(int in_dim, int out_dim, int actor)
{
    TrainLayout L;
    L.in_dim = in_dim; L.out_dim = out_dim; L.actor = actor;
    int o = 0;
    L.w[0] = o; o += in_dim * TR_H; L.b[0] = o; o += TR_H;
    L.w[1] = o; o += TR_H * TR_H;   L.b[1] = o; o += TR_H;
    L.w[2] = o; o += TR_H * TR_H;   L.b[2] = o; o += TR_H;
    L.w[3] = o; o += TR_H * out_dim; L.b[3] = o; o += out_dim;
    L.ls = o;
    if (actor) o += out_dim;
    L.P = o;
    return L;
}
constexpr int TR_MAX_COUNT = 1 << 30;   // rows per gradient call at most (keeps every 32-bit tile and row index of the kernel in range)
inline int train_grid(int count)
{
    const int64_t tiles = ((int64_t)count + TR_ROWS - 1) / TR_ROWS;
    return tiles < TR_MAX_WG ? (int)tiles : TR_MAX_WG;
}

// the per-row output stage of the gradient kernel, a template parameter of its body (dpenv_train.hip)
constexpr int TR_STAGE_VALUE = 0, TR_STAGE_PPO = 1, TR_STAGE_IMIT_NLL = 2, TR_STAGE_IMIT_MSE = 3, TR_NSTAGE = 4;
// the fifth stage, the allocation loss (dpenv_allocation_grad), has a kernel signature and a launcher of its own: its numbers travel in
// AllocLossArgs beside GradArgs, so the four stages above keep their argument block and with it their instruction streams
constexpr int TR_STAGE_ALLOC = 4;

struct GradArgs {
    TrainLayout L;
    const float* theta;
    const float* obs;        // [n_rows][in_dim]
    const float* act;        // [n_rows][out_dim]   (actor)
    const float* adv;        // [n_rows] advantage (actor), return (critic) or row weight (imitation; NULL = 1)
    const float* logp_old;   // [n_rows]            (actor)
    const int32_t* idx;      // [count] or NULL
    const int32_t* stop_flag;// or NULL
    float* partial;          // workspace: [grid][P + nstat]
    float* grad_out;         // [P + nstat]
    int count;
    float leak, clip;
};

// the allocation loss's numbers (dpenv_alloc_loss, validated by the entry point), env order bow, port, star
struct AllocLossArgs {
    float ws[3], wp, wsat;
    float lx[3], ly[3], kf[3], kr[3];
    float angle_scale;
    int azimuth_mode;
    float azimuth[2];        // port, star
};

struct AdamArgs {
    float* theta; const float* grad; float* m; float* v;
    int P;
    float lr, beta1, beta2, eps;
    int32_t* step_counter;
    const float* gate_kl;    // or NULL: no gate
    float kl_limit;
    int32_t* stop_flag;      // or NULL
};

namespace __attribute__((visibility("hidden"))) dev {
// dpenv_train.hip: the gradient (mlp_grad_kernel or imitation_grad_kernel + grad_reduce_kernel) and the gated Adam step (adam_step_kernel + adam_commit_kernel)
hipError_t launch_mlp_grad(const GradArgs* a, int stage, hipStream_t s);   // stage: TR_STAGE_*
// allocation_grad_kernel + grad_reduce_kernel: a->act holds the tau rows [n_rows][6], a->adv the row weight or NULL, a->logp_old and a->clip are not read
hipError_t launch_alloc_grad(const GradArgs* a, const AllocLossArgs* q, hipStream_t s);
hipError_t launch_adam_step(const AdamArgs* a, hipStream_t s);
}  // namespace dev

}  // namespace dpenv

#endif
