// dpenv_train.hip - the PPO update on the device (include/dpenv.h: "The PPO update"): mlp_grad_kernel<ACTOR> (forward, output gradient,
// backward and the weight gradients of one in -> 80 -> 80 -> 80 -> out network on the matrix cores, one partial per workgroup),
// grad_reduce_kernel (the partials summed in a fixed order) and the gated Adam step (adam_step_kernel + adam_commit_kernel).
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
constexpr int O_AUX = O_A + TR_ROWS * 8;             // [64][2] advantage | logp_old (actor), return (critic)
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

template <bool ACTOR>
__global__ __launch_bounds__(256) void mlp_grad_kernel(GradArgs a)
{
    extern __shared__ float lds[];
    if (a.stop_flag && *a.stop_flag) return;                  // the gate has closed: the update is over (uniform over the grid)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const TrainLayout& L = a.L;
    const int in = L.in_dim, od = L.out_dim;
    constexpr int NSTAT = ACTOR ? TR_NSTAT_ACTOR : TR_NSTAT_CRITIC;

    // ---- the parameters, once per workgroup ----
    for (int e = tid; e < TR_PAD * TR_H; e += 256) {
        const int k = e / TR_H;
        lds[O_W0 + e] = k < in ? a.theta[L.w[0] + e] : 0.0f;
    }
    for (int e = tid; e < TR_H * TR_H; e += 256) {
        const int k = e / TR_H, j = e - k * TR_H;
        lds[O_W1 + k * LDW + j] = a.theta[L.w[1] + e];
        lds[O_W2 + k * LDW + j] = a.theta[L.w[2] + e];
    }
    for (int e = tid; e < TR_H * TR_PAD; e += 256) {
        const int k = e >> 4, j = e & 15;
        lds[O_W3 + k * LDW3 + j] = j < od ? a.theta[L.w[3] + k * od + j] : 0.0f;
    }
    if (tid < TR_H) {
        lds[O_B + tid] = a.theta[L.b[0] + tid];
        lds[O_B + TR_H + tid] = a.theta[L.b[1] + tid];
        lds[O_B + 2 * TR_H + tid] = a.theta[L.b[2] + tid];
    }
    if (tid < TR_PAD) {
        lds[O_B + 3 * TR_H + tid] = tid < od ? a.theta[L.b[3] + tid] : 0.0f;
        if (ACTOR) {
            const float ls = tid < od ? a.theta[L.ls + tid] : 0.0f;
            const float es = expf(ls);
            lds[O_LS + tid] = ls;
            lds[O_LS + TR_PAD + tid] = es + 1e-8f;
            lds[O_LS + 2 * TR_PAD + tid] = es;
        }
    }

    f4 dw[15];
#pragma unroll
    for (int s = 0; s < 15; ++s) dw[s] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    float db0 = 0.0f, db1 = 0.0f, db2 = 0.0f, db3 = 0.0f;
    double stat = 0.0;
    const float lo = (float)(1.0 - (double)a.clip), hi = (float)(1.0 + (double)a.clip);
    const int tiles = (a.count + TR_ROWS - 1) / TR_ROWS;
    const int r0 = wave * 16;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int base = tile * TR_ROWS;
        __syncthreads();                                       // the previous tile's last readers are done (and the parameters are in)
        {   // the tile's inputs, gathered; rows past count and columns past in_dim are zero
            const int row = tid >> 2, part = tid & 3, g = base + row;
            const bool ok = g < a.count;
            const int64_t src = ok ? (a.idx ? (int64_t)a.idx[g] : (int64_t)g) : 0;
#pragma unroll
            for (int c = part; c < TR_PAD; c += 4) lds[O_X + row * LDX + c] = (ok && c < in) ? a.obs[src * in + c] : 0.0f;
            // what the output gradient needs of the row, fetched in the same burst
            if (ACTOR) {
#pragma unroll
                for (int c = part; c < 8; c += 4) lds[O_A + row * 8 + c] = (ok && c < od) ? a.act[src * od + c] : 0.0f;
                if (part == 1) lds[O_AUX + row * 2 + 1] = ok ? a.logp_old[src] : 0.0f;
            }
            if (part == 0) lds[O_AUX + row * 2] = ok ? a.adv[src] : 0.0f;
        }
        __syncthreads();
        // ---- forward: the wave's 16 rows ----
        layer_forward<TR_PAD / 4>(lds + O_X + r0 * LDX, LDX, lds + O_W0, TR_H, lds + O_B, lds + O_H1 + r0 * LDH, a.leak, lane);
        __syncthreads();
        layer_forward<TR_H / 4>(lds + O_H1 + r0 * LDH, LDH, lds + O_W1, LDW, lds + O_B + TR_H, lds + O_H2 + r0 * LDH, a.leak, lane);
        __syncthreads();
        layer_forward<TR_H / 4>(lds + O_H2 + r0 * LDH, LDH, lds + O_W2, LDW, lds + O_B + 2 * TR_H, lds + O_H3 + r0 * LDH, a.leak, lane);
        __syncthreads();
        {
            const float b = lds[O_B + 3 * TR_H + lr];
            f4 o[1] = {f4{b, b, b, b}};
            gemm_rows<TR_H / 4, 1, false>(lds + O_H3 + r0 * LDH, LDH, lds + O_W3, LDW3, o, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[O_D + (r0 + 4 * lk + r) * LDD + lr] = o[0][r];
        }
        __syncthreads();
        // ---- the output gradient, one lane per row, times count (the reduction divides) ----
        if (lane < 16) {
            const int row = r0 + lane, g = base + row;
            float* d = lds + O_D + row * LDD;
            float* st = lds + O_ST + row * 4;
            if (g < a.count) {
                const float* ra = lds + O_A + row * 8;
                if (ACTOR) {
                    float logp = 0.0f;
                    for (int j = 0; j < od; ++j) {
                        const float q = (ra[j] - d[j]) / lds[O_LS + TR_PAD + j];
                        logp += -0.5f * ((q * q + 2.0f * lds[O_LS + j]) + 1.8378770664093453f);
                    }
                    const float lpo = lds[O_AUX + row * 2 + 1], A = lds[O_AUX + row * 2];
                    const float ratio = expf(logp - lpo);
                    const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, lo), hi) * A;
                    const float gl = s1 <= s2 ? -(A * ratio) : 0.0f;       // dL/dlogp x count: the unclipped term is the minimum (ties included)
                    for (int j = 0; j < od; ++j) {
                        const float sd = lds[O_LS + TR_PAD + j];
                        const float q = (ra[j] - d[j]) / sd;
                        d[j] = gl * (q / sd);                                                    // dlogp/dmu = (a - mu) / sd^2
                        d[od + j] = gl * (q * q * (lds[O_LS + 2 * TR_PAD + j] / sd) - 1.0f);     // dlogp/dlog_std = q^2 e^ls / sd - 1
                    }
                    for (int j = 2 * od; j < TR_PAD; ++j) d[j] = 0.0f;
                    st[0] = -fminf(s1, s2);
                    st[1] = lpo - logp;
                    st[2] = (ratio > hi || ratio < lo) ? 1.0f : 0.0f;
                    st[3] = ratio;
                } else {
                    const float e = d[0] - lds[O_AUX + row * 2];           // v - ret
                    d[0] = 2.0f * e;
                    for (int j = 1; j < TR_PAD; ++j) d[j] = 0.0f;
                    st[0] = e * e;
                }
            } else {
                for (int j = 0; j < TR_PAD; ++j) d[j] = 0.0f;
                st[0] = st[1] = st[2] = st[3] = 0.0f;
            }
        }
        __syncthreads();
        if (tid < NSTAT) {
#pragma unroll 16
            for (int row = 0; row < TR_ROWS; ++row) stat += (double)lds[O_ST + row * 4 + tid];
        }
        // ---- backward and the weight gradients, layer by layer ----
        dw_step<3>(dw, lds, wave, lane);
        if (tid < TR_PAD) db3 += column_sum(lds + O_D + tid, LDD);
        __syncthreads();
        layer_backward<TR_PAD / 4>(lds + O_D + r0 * LDD, LDD, lds + O_W3, LDW3, lds + O_H3 + r0 * LDH, a.leak, lane);
        __syncthreads();
        dw_step<2>(dw, lds, wave, lane);
        if (tid < TR_H) db2 += column_sum(lds + O_H3 + tid, LDH);
        __syncthreads();
        layer_backward<TR_H / 4>(lds + O_H3 + r0 * LDH, LDH, lds + O_W2, LDW, lds + O_H2 + r0 * LDH, a.leak, lane);
        __syncthreads();
        dw_step<1>(dw, lds, wave, lane);
        if (tid < TR_H) db1 += column_sum(lds + O_H2 + tid, LDH);
        __syncthreads();
        layer_backward<TR_H / 4>(lds + O_H2 + r0 * LDH, LDH, lds + O_W1, LDW, lds + O_H1 + r0 * LDH, a.leak, lane);
        __syncthreads();
        dw_step<0>(dw, lds, wave, lane);
        if (tid < TR_H) db0 += column_sum(lds + O_H1 + tid, LDH);
    }

    // ---- one partial per workgroup, in theta's layout, the statistics behind it ----
    float* out = a.partial + (size_t)blockIdx.x * (size_t)(L.P + NSTAT);
#pragma unroll
    for (int s = 0; s < 15; ++s) {
        const int t = 4 * s + wave;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ti = 4 * lk + r;                         // row / column inside the 16 x 16 tile
            const float val = dw[s][r];
            if (t < 5) {
                if (lr < od) out[L.w[3] + (t * 16 + ti) * od + lr] = val;
            } else if (t < 55) {
                const int u = t < 30 ? t - 5 : t - 30, it = u / 5, jt = u - 5 * it;
                out[L.w[t < 30 ? 2 : 1] + (it * 16 + ti) * TR_H + jt * 16 + lr] = val;
            } else {
                if (ti < in) out[L.w[0] + ti * TR_H + (t - 55) * 16 + lr] = val;
            }
        }
    }
    if (tid < TR_H) {
        out[L.b[0] + tid] = db0;
        out[L.b[1] + tid] = db1;
        out[L.b[2] + tid] = db2;
    }
    if (tid < od) out[L.b[3] + tid] = db3;
    if (ACTOR && tid >= od && tid < 2 * od) out[L.ls + tid - od] = db3;
    if (tid < NSTAT) out[L.P + tid] = (float)stat;
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

hipError_t dev::launch_mlp_grad(const GradArgs* a, hipStream_t s)
{
    const int grid = train_grid(a->count);
    const int nstat = a->L.actor ? TR_NSTAT_ACTOR : TR_NSTAT_CRITIC;
    const int total = a->L.P + nstat;
    const size_t lds_bytes = (size_t)LDS_FLOATS * sizeof(float);
    // the tile needs more LDS than a kernel gets by default: the limit is raised once per kernel and device, by whichever call comes first
    // (a function attribute, not a stream operation; dpenv.h asks for that first call to be made outside a stream capture)
    static std::once_flag once[2][64];
    int devid = 0;
    hipError_t e = hipGetDevice(&devid);
    if (e != hipSuccess) return e;
    const int act = a->L.actor ? 1 : 0;
    const void* fn = act ? reinterpret_cast<const void*>(&mlp_grad_kernel<true>) : reinterpret_cast<const void*>(&mlp_grad_kernel<false>);
    if (devid >= 0 && devid < 64) {
        hipError_t first = hipSuccess;
        std::call_once(once[act][devid], [&] { first = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); });
        if (first != hipSuccess) return first;
    } else {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    if (act) hipLaunchKernelGGL(mlp_grad_kernel<true>, dim3(grid), dim3(256), lds_bytes, s, *a);
    else hipLaunchKernelGGL(mlp_grad_kernel<false>, dim3(grid), dim3(256), lds_bytes, s, *a);
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
