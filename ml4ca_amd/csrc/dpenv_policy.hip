// dpenv_policy.hip - the PPO actor-critic evaluated INSIDE the rollout launch.
//
// Reference: mlp_gaussian_policy / mlp_actor_critic, src/rl/windows_workspace/spinup/algos/tf1/ppo/core.py:29-33,
// 80-107 (dense layers y = x W + b with W[in][out], hidden activation leaky_relu(0.2) for the shipped model -
// train.py:24,31, config.json - linear output, log_std parameter, pi = mu + N(0,1) exp(log_std),
// gaussian_likelihood core.py:42-46), consumed by the rollout loop ppo.py:289-322 which stores
// (o, a, r, v, logp) per step (ppo.py:298).
//
// Mapping to CDNA4.  A wave owns 64 environments (one per lane) and evaluates the MLP for all of them at
// once on the matrix cores in the TRANSPOSED orientation  H_next^T [features x envs] = W^T [out x in] . H^T:
//   * A operand  = weights, pre-permuted on the host into MFMA fragments, read from LDS (one 16-byte
//                  ds_read_b128 per lane per fragment); one LDS copy per 256-thread workgroup.
//   * B operand  = activations.  The f32 accumulator tile of v_mfma_f32_32x32x16_f16 has the env on the lane and
//                  the feature in the register index, which is exactly what the next layer's B operand wants:
//                  leaky-relu + convert to f16 in place, no lane movement, no LDS (cdna_hip_programming.md
//                  section 3, "an accumulator tile as the next MFMA's operand"; the k-order permutation that
//                  comes with it is folded into the host-side weight packing).
//   * biases     = first layer: a constant-1 input (slot 15) whose weight column holds the bias; later layers: the
//                  accumulator's INITIAL value (srcC of the first MFMA of a row-block is a bias tile read from LDS,
//                  one 64-byte broadcast read per lane half), so hidden width 80 needs K = 80 = 5 k-steps, not 96.
//   * in/out     = the env-per-lane <-> (32-env tile, lane-half) exchange at both ends is one
//                  v_permlane32_swap per register.
// Precision: f16 weights and activations, f32 accumulation.  This is the only MFMA use in the library; the
// environment itself stays scalar fp32 physics.
#include "dpenv_policy_dev.h"

namespace dpenv {

// =============================================================================================
//  standalone forward pass: mu [n][A], v [n] for obs [n][OD]   (deterministic policy / validation)
// =============================================================================================
template <int OD, int A, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_forward_kernel(const PolicyArgs pa, const float* obs, float* mu_out,
                                                                 float* v_out, int n)
{
    extern __shared__ uint4 lds_dyn[];
    uint4* lds_w = lds_dyn;                                                     // [2][nent] fragment entries
    const float* lds_b = (const float*)(lds_dyn + 2 * pa.nent);                       // [2][nblk][32] bias floats
    float* lds_io = (float*)lds_dyn + policy_lds_io_offset_floats(pa) + (threadIdx.x >> 6) * (64 * 9);   // wave-private staging
    stage_weights(lds_w, pa);
    const int lane = threadIdx.x & 63;
    const int wave0 = blockIdx.x * PBLOCK + (threadIdx.x & ~63);               // first env of this wave
    if (wave0 >= n) return;
    const int i = wave0 + lane;
    const bool live = i < n;
    float pre[OD], o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    load_rows<OD, 64>(obs + (int64_t)wave0 * OD, (int64_t)(n - wave0) * OD, lane, pre);
    wave_rows_from_regs<OD>(lds_io, pre, o, lane);
    half8 in0, in1;
    obs_to_frags<OD>(o, in0, in1);
    float mu[8], vv[8];
    mlp_eval2<KA>(lds_w, lds_w + pa.nent, lds_b, lds_b + pa.nblk * 32, pa.n_hidden, in0, in1, (_Float16)pa.leak, mu, vv);
    wave_store_rows<A>(lds_io, mu_out, (int64_t)wave0 * A, (int64_t)(n - wave0) * A, mu, lane);
    if (live) v_out[i] = vv[0];
}

// =============================================================================================
//  policy-in-the-loop rollout: T steps of (policy -> sample -> env.step -> value) per launch,
//  writing the PPO trajectory rows (ppo.py:298) straight into [T][n][.] blocks.
// =============================================================================================
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_kernel(const StepArgs a, const PolicyArgs pa)
{
    constexpr bool INTEG = false, REFF = false, SPLIT = false;
    const IntegArgs ia{};
    const FilterArgs fa{};
#include "dpenv_policy_rollout_body.inc"
}

// INTEG: the deployed node's integral action (IntegArgs, dpenv_set_integral_action)
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_integ_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia)
{
    constexpr bool INTEG = true, REFF = false, SPLIT = false;
    const FilterArgs fa{};
#include "dpenv_policy_rollout_body.inc"
}

// REFF: the setpoint reference filter (FilterArgs, dpenv_set_reference_filter), with the integral action if INTEG_
template <int MODE, bool EXT, int KA, bool INTEG_>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_reff_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia, const FilterArgs fa)
{
    constexpr bool INTEG = INTEG_, REFF = true, SPLIT = false;
#include "dpenv_policy_rollout_body.inc"
}

// the reference filter at rest on the env's reference RF[i].xyz: turning it on (mask NULL) and dpenv_reset (the envs it re-draws)
__global__ __launch_bounds__(256) void reff_rest_kernel(const float4* RF, float4* state, const uint8_t* mask, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (mask != nullptr && mask[i] == 0)) return;
    const float4 rf = RF[i];
    const float ref[3] = {rf.x, rf.y, rf.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) state[(int64_t)j * n + i] = make_float4(ref[j], 0.0f, 0.0f, ref[j]);
}

// the checkpoint path (dpenv_get_reference_filter_state / dpenv_set_reference_filter_state): float4 [3][n] <-> x float[9][n] (row 3 k + j:
// pos, vel, acc of axis j) | r float[3][n]; either may be NULL
__global__ __launch_bounds__(256) void reff_state_io_kernel(float4* state, float* x, float* r, int n, int write)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float4 q = state[(int64_t)j * n + i];
        if (write) {
            if (x) { q.x = x[(int64_t)j * n + i]; q.y = x[(int64_t)(3 + j) * n + i]; q.z = x[(int64_t)(6 + j) * n + i]; }
            if (r) q.w = r[(int64_t)j * n + i];
            state[(int64_t)j * n + i] = q;
        } else {
            if (x) { x[(int64_t)j * n + i] = q.x; x[(int64_t)(3 + j) * n + i] = q.y; x[(int64_t)(6 + j) * n + i] = q.z; }
            if (r) r[(int64_t)j * n + i] = q.w;
        }
    }
}

// the explicit reset's side of the integral action (dpenv_reset): I = 0, count = 0 for the envs it re-draws
__global__ __launch_bounds__(256) void integ_clear_kernel(float4* state, const uint8_t* mask, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && (mask == nullptr || mask[i] != 0)) state[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// the checkpoint path (dpenv_get_integral_state / dpenv_set_integral_state): float4 [n] <-> I float[3][n] | count int32[n]; either may be NULL
__global__ __launch_bounds__(256) void integ_state_io_kernel(float4* state, float* I, int32_t* c, int n, int write)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 q = state[i];
    if (write) {
        if (I) { q.x = I[i]; q.y = I[(int64_t)n + i]; q.z = I[2 * (int64_t)n + i]; }
        if (c) q.w = __int_as_float(c[i]);
        state[i] = q;
    } else {
        if (I) { I[i] = q.x; I[(int64_t)n + i] = q.y; I[2 * (int64_t)n + i] = q.z; }
        if (c) c[i] = __float_as_int(q.w);
    }
}

// =============================================================================================
//  Weight packing ON THE DEVICE: fp32 dense kernels W[l][in][out] / biases (the reference's variable layout, core.py:29-33)
//  -> the LDS image the evaluation kernels stage (MFMA A-operand fragments, bias tiles, std / logp constants).
//  One thread per f16 element of the COMPACT image (FragAddr: block-2 fragments of an 80-wide layer and the output layer's fragments
//  keep only the rows anybody reads).  Logical fragment f, lane l = (r = l & 31, h = l >> 5), element j holds
//  W^T[out row 32 mo + r][input slot k(f, h, j)]:
//    first layer : k = 8 h + j                                   (slots 0..in-1 = inputs, slot 15 = the layer's bias)
//    later layers: k = 32 mt + 16 s + 8 (j >> 2) + 4 h + (j & 3)  (the accumulator-as-operand order), ks = 2 mt + s;
//                  their biases go into `bias` as accumulator-layout tiles: block b, half h, register r16
//                  -> b[out row 32 mo + 8 (r16 >> 2) + 4 h + (r16 & 3)]
//  split: a second image of the LOW parts, lo = f16(w - f32(f16(w))), behind the first (dpenv_policy_dev.h, mlp_eval_x).
//  Stream-ordered, no host round trip: a PPO loop re-packs after every update without synchronising (ppo.py:260-280).
// =============================================================================================
__device__ __forceinline__ float pack_weight(const PackNet& m, int ks_n, int f, int lane, int j)
{
    const int r = lane & 31, hh = lane >> 5, H = m.H, nh = m.n_layers - 1;
    if (f < 3) {                                                        // first layer
        const int k = 8 * hh + j, row = 32 * f + r;
        if (row >= H) return 0.0f;
        return k < m.in_dim ? m.W[0][(size_t)k * H + row] : (k == 15 ? m.b[0][row] : 0.0f);
    }
    const int idx = f - 3, per_layer = 3 * ks_n;
    if (idx < per_layer * (nh - 1)) {                                   // hidden -> hidden
        const int l = 1 + idx / per_layer, rem = idx % per_layer, mo = rem / ks_n, ks = rem % ks_n;
        const int fk = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hh + (j & 3), row = 32 * mo + r;
        return (row < H && fk < H) ? m.W[l][(size_t)fk * H + row] : 0.0f;
    }
    const int ks = idx - per_layer * (nh - 1);                          // output layer
    const int fk = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hh + (j & 3);
    return (r < m.out_dim && fk < H) ? m.W[m.n_layers - 1][(size_t)fk * m.out_dim + r] : 0.0f;
}

__global__ __launch_bounds__(256) void pack_policy_kernel(const PackNet pi, const PackNet v, const float* log_std, int adim, int ks_n,
                                                          int nent, int nblk, int split, _Float16* frags, float* bias, float* consts)
{
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const int per_net = nent * 8;
    if (tid < 2 * per_net) {
        const int net = tid / per_net, el = tid % per_net, j = el & 7;
        int e = el >> 3;
        const PackNet& m = net ? v : pi;
        // entry of the compact image (FragAddr, dpenv_policy_dev.h) -> logical fragment f and a lane that reads this entry
        const int nh = m.n_layers - 1, B2 = ks_n == 5 ? 32 : 64, L0 = 128 + B2, LH = ks_n * (128 + B2);
        auto lane_of = [](int k, int per_half) { return (k / per_half) * 32 + (k % per_half); };      // entry k of a 2 x per_half fragment
        int f, lane;
        if (e < L0) {
            if (e < 128) { f = e >> 6; lane = e & 63; }
            else { f = 2; lane = lane_of(e - 128, B2 / 2); }
        } else if (e < L0 + (nh - 1) * LH) {
            e -= L0;
            const int l = e / LH, r = e % LH;
            if (r < 2 * ks_n * 64) { f = 3 + l * 3 * ks_n + (r >> 6); lane = r & 63; }
            else { const int r2 = r - 2 * ks_n * 64; f = 3 + l * 3 * ks_n + 2 * ks_n + r2 / B2; lane = lane_of(r2 % B2, B2 / 2); }
        } else {
            e -= L0 + (nh - 1) * LH;
            f = 3 + (nh - 1) * 3 * ks_n + (e >> 4);
            lane = lane_of(e & 15, 8);
        }
        const float w = pack_weight(m, ks_n, f, lane, j);
        const _Float16 hi = (_Float16)w;                                // round to nearest even
        frags[tid] = hi;
        if (split) frags[2 * per_net + tid] = (_Float16)(w - (float)hi);
    }
    if (tid < 2 * nblk * 32) {
        const int net = tid / (nblk * 32), e = tid % (nblk * 32), blk = e / 32, hh = (e >> 4) & 1, r16 = e & 15;
        const PackNet& m = net ? v : pi;
        const int nh = m.n_layers - 1, rr = 8 * (r16 >> 2) + 4 * hh + (r16 & 3);
        float b;
        if (blk < 3 * (nh - 1)) {
            const int l = 1 + blk / 3, row = 32 * (blk % 3) + rr;
            b = row < m.H ? m.b[l][row] : 0.0f;
        } else {
            b = rr < m.out_dim ? m.b[m.n_layers - 1][rr] : 0.0f;
        }
        bias[tid] = b;
    }
    if (tid < 8) {
        const float ls = tid < adim ? log_std[tid] : 0.0f;
        const float sd = expf(ls);
        consts[tid] = sd;                                               // core.py:84
        consts[8 + tid] = 1.0f / (sd + 1e-8f);                          // core.py:45, EPS = 1e-8
        consts[16 + tid] = tid < adim ? (-ls - 0.5f * logf(2.0f * 3.14159265358979323846f)) : 0.0f;
    }
}

}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_pack_policy(const PackNet* pi, const PackNet* v, const float* log_std, int adim, int ks, int nent, int nblk, int split,
                                  void* frags, float* bias, float* consts, hipStream_t s)
{
    const int total = 2 * nent * 8;
    hipLaunchKernelGGL(pack_policy_kernel, dim3((total + 255) / 256), dim3(256), 0, s, *pi, *v, log_std, adim, ks, nent, nblk, split,
                       (_Float16*)frags, bias, consts);
    return hipGetLastError();
}

static size_t policy_lds_bytes(const PolicyArgs& pa)
{
    return (size_t)2 * pa.nent * 16 + (size_t)2 * pa.nblk * 32 * 4 + (size_t)PWAVES * 64 * 9 * 4;
}

hipError_t dev::launch_policy_forward(const PolicyArgs* pa, int od, int adim, const float* obs, float* mu, float* v, int n, hipStream_t s)
{
    const dim3 grid((n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    return with_obs_act(od, adim, [&](auto OD, auto A) { return with_ka(*pa, [&](auto K) {
        return launch_with_lds(policy_forward_kernel<OD, A, K>, grid, block, policy_lds_bytes(*pa), s, *pa, obs, mu, v, n);
    }); });
}

// the one-wave closed loop in f16; with the integral action (ia) the set integ_one_wave admits, with the reference filter (fa) the set
// reff_one_wave admits
hipError_t dev::launch_policy_rollout(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                      hipStream_t s)
{
    const dim3 grid((a->n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    const size_t lds = policy_lds_bytes(*pa);
    return with_mode_ext_ka(mode, ext, *pa, [&](auto M, auto E, auto K) -> hipError_t {
        if (fa) {
            if constexpr (reff_one_wave(M, E, K)) {
                if (ia) return launch_with_lds(policy_rollout_reff_kernel<M, E, K, true>, grid, block, lds, s, *a, *pa, *ia, *fa);
                return launch_with_lds(policy_rollout_reff_kernel<M, E, K, false>, grid, block, lds, s, *a, *pa, IntegArgs{}, *fa);
            }
            return hipErrorInvalidValue;
        }
        if (!ia) return launch_with_lds(policy_rollout_kernel<M, E, K>, grid, block, lds, s, *a, *pa);
        if constexpr (integ_one_wave(M, E, K)) return launch_with_lds(policy_rollout_integ_kernel<M, E, K>, grid, block, lds, s, *a, *pa, *ia);
        return hipErrorInvalidValue;
    });
}

hipError_t dev::launch_integ_clear(float4* state, const uint8_t* mask, int n, hipStream_t s)
{
    hipLaunchKernelGGL(integ_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, s, state, mask, n);
    return hipGetLastError();
}

hipError_t dev::launch_reff_rest(const float4* RF, float4* state, const uint8_t* mask, int n, hipStream_t s)
{
    hipLaunchKernelGGL(reff_rest_kernel, dim3((n + 255) / 256), dim3(256), 0, s, RF, state, mask, n);
    return hipGetLastError();
}

hipError_t dev::launch_reff_state_io(float4* state, float* x, float* r, int n, int write, hipStream_t s)
{
    hipLaunchKernelGGL(reff_state_io_kernel, dim3((n + 255) / 256), dim3(256), 0, s, state, x, r, n, write);
    return hipGetLastError();
}

hipError_t dev::launch_integ_state_io(float4* state, float* I, int32_t* c, int n, int write, hipStream_t s)
{
    hipLaunchKernelGGL(integ_state_io_kernel, dim3((n + 255) / 256), dim3(256), 0, s, state, I, c, n, write);
    return hipGetLastError();
}
