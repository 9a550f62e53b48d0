// dpenv_train.hip - the PPO update on the device (include/dpenv.h: "The PPO update"): mlp_grad_kernel<ACTOR> (forward, output gradient,
// backward and the weight gradients of one in -> 80 -> 80 -> 80 -> out network on the matrix cores, one partial per workgroup),
// grad_reduce_kernel (the partials summed in a fixed order) and the gated Adam step (adam_step_kernel + adam_commit_kernel).
// imitation_grad_kernel<LOSS> (dpenv_imitation_grad) is the same body with a third per-row output stage: dpenv_train_grad_body.inc is
// the one text of all four kernels, the stage chosen at compile time.  allocation_grad_kernel (dpenv_allocation_grad) is the same text
// with a fifth stage - the QP law's objective at the network's output - and a second argument for that stage's numbers.
//
// Arithmetic: the exact-f32 MFMA v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain).  80 = 5 x 16, so the hidden layers tile
// without padding; the 9- or 6-wide input and the 7- or 1-wide output are padded to one 16-wide tile with zeros.  No operand split, no
// range care: 1/count is applied by the reduction, after every sum (DESIGN.md section 4 for why not the split-f16 form).
//
// One workgroup = 256 threads = 4 waves works on tiles of TR_ROWS = 64 rows.  Everything a tile needs lives in LDS: the weights
// (loaded once per workgroup), the tile's inputs X and its activations H1..H3 as [row][feature].  An f32 MFMA takes ONE float per
// lane and operand and runs 32 cycles, so feeding both operands from LDS (two ds_read_b32 per MFMA at worst, 6 per 5 in the row
// phase) leaves the matrix pipe the bound, and [row][feature] serves all three products without a transposition:
//   forward   Z = H W       A[i = row][k = feature] = H[row][k]      B[k][j] = W[k][j]
//   backward  G = dZ W'     A[i = row][k = feature] = dZ[row][k]     B[k][j] = W[j][k]
//   weights   dW = H' dZ    A[i = feature][k = row] = H[row][i]      B[k = row][j] = dZ[row][j]
// Row phase (forward, output gradient, backward): wave w owns rows 16 w .. 16 w + 15 of the tile.  dW phase: the 60 16x16 tiles of
// dW0..dW3 are dealt round-robin to the four waves (15 each = 60 accumulator registers), every tile consuming all 64 rows; the
// accumulators live across ALL tiles of the workgroup.  The backward pass overwrites H(l+1) with dZ(l) in place once dW(l+1) has read
// it, so the tile's LDS footprint is X + three activation blocks + the output block.  Biases (and the actor's log_std) are column sums
// of the same blocks, taken by one thread per column in row order.
#include <mutex>

#include "dpenv_env_dev.h"    // sincos_lean, the allocation stage's sin / cos (the QP law's and the neural allocator's)
#include "dpenv_train_dev.h"

namespace dpenv {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// row strides (floats), chosen so that the 64 lanes of an operand read fall on distinct banks (or nearly): see the reads in gemm_rows / dw_step
constexpr int LDX = 20, LDH = 84, LDW = 81, LDW3 = 17, LDD = 20;
// LDS map (floats)
constexpr int O_W0 = 0;                              // [16][80], rows >= in_dim zero
constexpr int O_W1 = O_W0 + TR_PAD * TR_H;           // [80][LDW]
constexpr int O_W2 = O_W1 + TR_H * LDW;
constexpr int O_W3 = O_W2 + TR_H * LDW;              // [80][LDW3], columns >= out_dim zero
constexpr int O_B = O_W3 + TR_H * LDW3;              // b0 | b1 | b2 [80] each, b3 [16]
constexpr int O_LS = O_B + 3 * TR_H + TR_PAD;        // log_std [16] | exp(log_std) + 1e-8 [16] | exp(log_std) [16]
constexpr int O_X = O_LS + 3 * TR_PAD;               // [64][LDX]
constexpr int O_H1 = O_X + TR_ROWS * LDX;            // [64][LDH]
constexpr int O_H2 = O_H1 + TR_ROWS * LDH;
constexpr int O_H3 = O_H2 + TR_ROWS * LDH;
constexpr int O_D = O_H3 + TR_ROWS * LDH;            // [64][LDD]: the network's output, then its gradient (actor: d/dmu | d/dlog_std)
constexpr int O_ST = O_D + TR_ROWS * LDD;            // [64][4] per-row statistics
constexpr int O_A = O_ST + TR_ROWS * 4;              // [64][8] the rows' actions (actor)
constexpr int O_AUX = O_A + TR_ROWS * 8;             // [64][2] advantage | logp_old (actor), return (critic), weight (imitation)
constexpr int LDS_FLOATS = O_AUX + TR_ROWS * 2;
static_assert(LDS_FLOATS * 4 <= 160 * 1024, "the tile does not fit the CU's LDS");

// acc[nt] (16 rows x 16 columns each) += A[16 rows][4 KSTEPS] * B: A row-major with stride lda; B[k][j] at B[k * ldb + j], or with TB
// its transpose, B[j * ldb + k]
template <int KSTEPS, int NT, bool TB>
__device__ __forceinline__ void gemm_rows(const float* A, int lda, const float* B, int ldb, f4 (&acc)[NT], int lane)
{
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
        const int k = 4 * kk + lk;
        const float a = A[lr * lda + k];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float b = TB ? B[(nt * 16 + lr) * ldb + k] : B[k * ldb + nt * 16 + lr];
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[nt], 0, 0, 0);
        }
    }
}

// one hidden layer forward for the wave's 16 rows: H_out = act(H_in W + b); act(z) = max(z, leak z)
template <int KSTEPS>
__device__ __forceinline__ void layer_forward(const float* Hin, int ldin, const float* W, int ldw, const float* bias, float* Hout, float leak, int lane)
{
    const int lr = lane & 15, lk = lane >> 4;
    f4 acc[5];
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
        const float b = bias[nt * 16 + lr];
        acc[nt] = f4{b, b, b, b};
    }
    gemm_rows<KSTEPS, 5, false>(Hin, ldin, W, ldw, acc, lane);
#pragma unroll
    for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float z = acc[nt][r];
            Hout[(4 * lk + r) * LDH + nt * 16 + lr] = fmaxf(z, leak * z);
        }
}

// one layer backward for the wave's 16 rows: dZ = (G W') * act'(z), written over the layer's activations H (act' is read off h: h > 0
// exactly where z > 0 for leak in [0, 1], and z <= 0 takes the slope `leak`, as torch's leaky_relu backward does at z = 0)
template <int KSTEPS>
__device__ __forceinline__ void layer_backward(const float* G, int ldg, const float* W, int ldw, float* H, float leak, int lane)
{
    const int lr = lane & 15, lk = lane >> 4;
    f4 acc[5];
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) acc[nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    gemm_rows<KSTEPS, 5, true>(G, ldg, W, ldw, acc, lane);
#pragma unroll
    for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* p = H + (4 * lk + r) * LDH + nt * 16 + lr;
            const float g = acc[nt][r];
            *p = *p > 0.0f ? g : leak * g;
        }
}

// the 60 tiles of dW, in the order they are dealt: layer 3 (5 tiles: 80 x 16), layer 2 (25), layer 1 (25), layer 0 (5: 16 x 80)
template <int LAYER> struct DwRange { };
template <> struct DwRange<3> { static constexpr int lo = 0, hi = 5; };
template <> struct DwRange<2> { static constexpr int lo = 5, hi = 30; };
template <> struct DwRange<1> { static constexpr int lo = 30, hi = 55; };
template <> struct DwRange<0> { static constexpr int lo = 55, hi = 60; };

// dW(LAYER) += H' dZ over the tile's 64 rows, for the tiles this wave owns (tile t belongs to wave t % 4, slot t / 4)
template <int LAYER>
__device__ __forceinline__ void dw_step(f4 (&dw)[15], const float* lds, int wave, int lane)
{
    constexpr int lo = DwRange<LAYER>::lo, hi = DwRange<LAYER>::hi;
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int s = 0; s < 15; ++s) {
        if (4 * s + 3 < lo || 4 * s >= hi) continue;          // compile time: no tile of this layer in the slot
        const int t = 4 * s + wave;
        if (t >= lo && t < hi) {
            const int u = t - lo;
            const float *pa, *pb;
            int lda, ldb;
            if (LAYER == 3) { pa = lds + O_H3 + u * 16; lda = LDH; pb = lds + O_D; ldb = LDD; }
            else if (LAYER == 0) { pa = lds + O_X; lda = LDX; pb = lds + O_H1 + u * 16; ldb = LDH; }
            else {
                const int it = u / 5, jt = u - 5 * it;
                pa = lds + (LAYER == 2 ? O_H2 : O_H1) + it * 16; lda = LDH;
                pb = lds + (LAYER == 2 ? O_H3 : O_H2) + jt * 16; ldb = LDH;
            }
            f4 c = dw[s];
#pragma unroll
            for (int kk = 0; kk < TR_ROWS / 4; ++kk) {
                const int k = 4 * kk + lk;
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k * lda + lr], pb[k * ldb + lr], c, 0, 0, 0);
            }
            dw[s] = c;
        }
    }
}

__device__ __forceinline__ float column_sum(const float* p, int ld)
{
    float s = 0.0f;
#pragma unroll 16                                              // the loads of 16 rows in flight; the additions stay in row order
    for (int row = 0; row < TR_ROWS; ++row) s += p[row * ld];
    return s;
}

template <bool ACTOR_NET>
__global__ __launch_bounds__(256) void mlp_grad_kernel(GradArgs a)
{
    constexpr int STAGE = ACTOR_NET ? TR_STAGE_PPO : TR_STAGE_VALUE;
#include "dpenv_train_grad_body.inc"
}

// the imitation loss (dpenv_imitation_grad): the same body with the third per-row stage.  LOSS: DPENV_IMITATE_NLL (0) or DPENV_IMITATE_MSE (1)
template <int LOSS>
__global__ __launch_bounds__(256) void imitation_grad_kernel(GradArgs a)
{
    constexpr int STAGE = LOSS == 0 ? TR_STAGE_IMIT_NLL : TR_STAGE_IMIT_MSE;
#include "dpenv_train_grad_body.inc"
}

// the allocation loss (dpenv_allocation_grad): the same body with the fifth per-row stage, whose numbers arrive in an argument of its
// own - the other kernels' argument block, and with it their instruction streams, are what they were without it
__global__ __launch_bounds__(256) void allocation_grad_kernel(GradArgs a, AllocLossArgs q)
{
    constexpr int STAGE = TR_STAGE_ALLOC;
#define TR_BODY_ALLOC
#include "dpenv_train_grad_body.inc"
#undef TR_BODY_ALLOC
}

// grad_out[p] = (sum over the workgroups' partials, in workgroup order) / count
__global__ __launch_bounds__(256) void grad_reduce_kernel(const float* partial, int nwg, int total, int count, const int32_t* stop_flag,
                                                          float* grad_out)
{
    if (stop_flag && *stop_flag) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += (double)partial[(size_t)w * total + p];
    grad_out[p] = (float)(s / (double)count);
}

// ---- Adam (dpenv.h: the operations in this order) ----
__device__ __forceinline__ double powi(double b, int e)
{
    double p = 1.0;
    while (e > 0) {
        if (e & 1) p *= b;
        b *= b;
        e >>= 1;
    }
    return p;
}

__device__ __forceinline__ bool gate_closed(const AdamArgs& a) { return a.gate_kl && (*a.stop_flag != 0 || *a.gate_kl > a.kl_limit); }

struct AdamScalars { float c1, c2, step_size, bc2s; };

__device__ __forceinline__ void adam_one(const AdamArgs& a, const AdamScalars& k, float g, float& th, float& m, float& v)
{
    m = fmaf(k.c1, g - m, m);
    v = fmaf(k.c2 * g, g, a.beta2 * v);
    const float denom = sqrtf(v) / k.bc2s + a.eps;
    th = fmaf(-k.step_size, m / denom, th);
}

__global__ __launch_bounds__(256) void adam_step_kernel(AdamArgs a)
{
    if (gate_closed(a)) return;                               // adam_commit_kernel, behind this one, sets the flag
    const int t = *a.step_counter + 1;
    AdamScalars k;
    k.c1 = 1.0f - a.beta1;
    k.c2 = 1.0f - a.beta2;
    k.step_size = a.lr / (float)(1.0 - powi((double)a.beta1, t));
    k.bc2s = sqrtf((float)(1.0 - powi((double)a.beta2, t)));
    const int n4 = a.P >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(a.grad);
    float4* th4 = reinterpret_cast<float4*>(a.theta);
    float4* m4 = reinterpret_cast<float4*>(a.m);
    float4* v4 = reinterpret_cast<float4*>(a.v);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const float4 g = g4[i];
        float4 th = th4[i], m = m4[i], v = v4[i];
        adam_one(a, k, g.x, th.x, m.x, v.x);
        adam_one(a, k, g.y, th.y, m.y, v.y);
        adam_one(a, k, g.z, th.z, m.z, v.z);
        adam_one(a, k, g.w, th.w, m.w, v.w);
        th4[i] = th; m4[i] = m; v4[i] = v;
    }
    const int i = 4 * n4 + threadIdx.x;                        // the scalar tail
    if (blockIdx.x == 0 && threadIdx.x < 4 && i < a.P) adam_one(a, k, a.grad[i], a.theta[i], a.m[i], a.v[i]);
}

// one thread, behind adam_step_kernel on the stream (which reads the counter and the flag but writes neither): closes the gate or counts the step
__global__ void adam_commit_kernel(AdamArgs a)
{
    if (gate_closed(a)) *a.stop_flag = 1;
    else *a.step_counter = *a.step_counter + 1;
}

}  // namespace

hipError_t dev::launch_mlp_grad(const GradArgs* a, int stage, hipStream_t s)
{
    const int grid = train_grid(a->count);
    const int nstat = a->L.actor ? TR_NSTAT_ACTOR : TR_NSTAT_CRITIC;
    const int total = a->L.P + nstat;
    const size_t lds_bytes = (size_t)LDS_FLOATS * sizeof(float);
    const void* fn;
    switch (stage) {
    case TR_STAGE_VALUE: fn = reinterpret_cast<const void*>(&mlp_grad_kernel<false>); break;
    case TR_STAGE_PPO: fn = reinterpret_cast<const void*>(&mlp_grad_kernel<true>); break;
    case TR_STAGE_IMIT_NLL: fn = reinterpret_cast<const void*>(&imitation_grad_kernel<0>); break;
    case TR_STAGE_IMIT_MSE: fn = reinterpret_cast<const void*>(&imitation_grad_kernel<1>); break;
    default: return hipErrorInvalidValue;
    }
    // the tile needs more LDS than a kernel gets by default: the limit is raised once per kernel and device, by whichever call comes first
    // (a function attribute, not a stream operation; dpenv.h asks for that first call to be made outside a stream capture)
    static std::once_flag once[TR_NSTAGE][64];
    int devid = 0;
    hipError_t e = hipGetDevice(&devid);
    if (e != hipSuccess) return e;
    if (devid >= 0 && devid < 64) {
        hipError_t first = hipSuccess;
        std::call_once(once[stage][devid], [&] { first = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); });
        if (first != hipSuccess) return first;
    } else {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    switch (stage) {
    case TR_STAGE_VALUE: hipLaunchKernelGGL(mlp_grad_kernel<false>, dim3(grid), dim3(256), lds_bytes, s, *a); break;
    case TR_STAGE_PPO: hipLaunchKernelGGL(mlp_grad_kernel<true>, dim3(grid), dim3(256), lds_bytes, s, *a); break;
    case TR_STAGE_IMIT_NLL: hipLaunchKernelGGL(imitation_grad_kernel<0>, dim3(grid), dim3(256), lds_bytes, s, *a); break;
    default: hipLaunchKernelGGL(imitation_grad_kernel<1>, dim3(grid), dim3(256), lds_bytes, s, *a); break;
    }
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const float*)a->partial, grid, total, a->count, a->stop_flag,
                       a->grad_out);
    return hipGetLastError();
}

// the fifth stage: launch_mlp_grad's steps for the kernel with the second argument (the same grid, LDS size, first-call rule and reduction)
hipError_t dev::launch_alloc_grad(const GradArgs* a, const AllocLossArgs* q, hipStream_t s)
{
    const int grid = train_grid(a->count);
    const int total = a->L.P + TR_NSTAT_ACTOR;
    const size_t lds_bytes = (size_t)LDS_FLOATS * sizeof(float);
    const void* fn = reinterpret_cast<const void*>(&allocation_grad_kernel);
    static std::once_flag once[64];
    int devid = 0;
    hipError_t e = hipGetDevice(&devid);
    if (e != hipSuccess) return e;
    if (devid >= 0 && devid < 64) {
        hipError_t first = hipSuccess;
        std::call_once(once[devid], [&] { first = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); });
        if (first != hipSuccess) return first;
    } else {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(allocation_grad_kernel, dim3(grid), dim3(256), lds_bytes, s, *a, *q);
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const float*)a->partial, grid, total, a->count, a->stop_flag,
                       a->grad_out);
    return hipGetLastError();
}

hipError_t dev::launch_adam_step(const AdamArgs* a, hipStream_t s)
{
    const int n4 = a->P >> 2;
    int grid = (n4 + 255) / 256;
    grid = grid < 1 ? 1 : (grid > 1024 ? 1024 : grid);
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(adam_commit_kernel, dim3(1), dim3(1), 0, s, *a);
    return hipGetLastError();
}

}  // namespace dpenv
