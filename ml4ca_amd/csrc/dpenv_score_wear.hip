// dpenv_score_wear.hip - the score card's third axis (dpenv_score_accumulate_wear and dpenv_score_wear_* in dpenv.h): IADC, the integral
// absolute derivative of the commands, accumulated in the same pass over a block's rows that updates the score state.  A scored flight
// reads its act rows once: the scan is score_kernel's (dpenv_score_dev.h) with the act fetch widened to the variant's azimuth columns,
// the score update is the one function of dpenv_score_lane.h both kernels call, and the commands are the env's own decode
// (env_decode_cmd of dpenv_env_dev.h), so IADC is taken on what the plant was actually told.
//
// A unit of its own with the library's CXXFLAGS, for the reason dpenv_label.hip is: no other unit's kernels see a new instantiation.
//
// Wear state, caller-owned, all-zero = fresh: WEAR_STREAMS 16-byte streams st[s][n] beside the score state's eight:
//   0  (open iadc_rps, open iadc_angle)      f64 x 2      2  (n_prev0, n_prev1, n_prev2, alpha_prev_port)      f32 x 4
//   1  (closed iadc_rps, closed iadc_angle)  f64 x 2      3  (alpha_prev_star, has_prev, 0, 0)                 f32, u32 x 3
// 64 B per env.  has_prev is the wear state's own: a fresh wear state joined to a score state in mid-episode counts nothing for its first row.
// A row is up to 15 loads per lane (score_kernel: 11), 97 B instead of 81 B with seven action columns.
//
// Registers and instructions (f32 obs / bf16 obs; score_kernel: 85 VGPR, 1258 / 1297 instructions), no scratch in any of the ten:
//   full 114 / 106 VGPR, 1518 / 1555      simple 106 / 98, 1457 / 1493      limited 106 / 106, 1501 / 1542
//   final 106 / 106, 1541 / 1581          final cont_ang 122 / 116, 1718 / 1758 (the two atan2 per row)
// The measured cost beside score_kernel is profiles/score_wear_timing.txt.
#include "dpenv_env_dev.h"

namespace dpenv {

#include "dpenv_score_lane.h"

namespace {

constexpr int WEAR_STREAMS = 4;
constexpr int WEAR_NOUT = 4;            // DPENV_SCORE_WEAR_NOUT

// the action columns behind the three thrusts that the variant's azimuth commands read (the bow azimuth of FULL, column 3, is not counted)
constexpr int wear_col0(int mode) { return mode == MODE_FULL ? 4 : 3; }
constexpr int wear_ncol(int mode) { return mode == MODE_SIMPLE ? 0 : (mode == MODE_FINAL_CONT ? 4 : 2); }

template <int MODE>
struct WearRow {
    ScoreRow r;
    float x[wear_ncol(MODE) ? wear_ncol(MODE) : 1];
};

struct WearState {
    double rps, ang, c_rps, c_ang;
    float np[3], ap[2];
    uint32_t has_prev;
};

__device__ __forceinline__ void wear_load(const uint4* __restrict__ st, int n, int i, WearState& w)
{
    uint4 q[WEAR_STREAMS];
#pragma unroll
    for (int k = 0; k < WEAR_STREAMS; ++k) q[k] = st[(int64_t)k * n + i];
    double2 d;
    d = score_d2(q[0]); w.rps = d.x; w.ang = d.y;
    d = score_d2(q[1]); w.c_rps = d.x; w.c_ang = d.y;
    w.np[0] = __uint_as_float(q[2].x); w.np[1] = __uint_as_float(q[2].y); w.np[2] = __uint_as_float(q[2].z);
    w.ap[0] = __uint_as_float(q[2].w); w.ap[1] = __uint_as_float(q[3].x);
    w.has_prev = q[3].y;
}

__device__ __forceinline__ void wear_store(uint4* __restrict__ st, int n, int i, const WearState& w)
{
    st[i] = score_u4(w.rps, w.ang);
    st[(int64_t)n + i] = score_u4(w.c_rps, w.c_ang);
    st[2 * (int64_t)n + i] = make_uint4(__float_as_uint(w.np[0]), __float_as_uint(w.np[1]), __float_as_uint(w.np[2]), __float_as_uint(w.ap[0]));
    st[3 * (int64_t)n + i] = make_uint4(__float_as_uint(w.ap[1]), w.has_prev, 0u, 0u);
}

// the wear law of dpenv.h for one row: f32 in the stated order, sums f64; end: the row ended the episode (score_row_update's verdict)
template <int MODE>
__device__ __forceinline__ void wear_row_update(WearState& w, const WearRow<MODE>& row, bool end)
{
    float act[7] = {row.r.a[0], row.r.a[1], row.r.a[2], 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < wear_ncol(MODE); ++c) act[wear_col0(MODE) + c] = row.x[c];
    float ang[3] = {0.0f, 0.0f, 0.0f}, thr[3];          // SIMPLE commands no azimuth: its angle term stays 0
    env_decode_cmd<MODE, false>(ang, act, thr);
    if (w.has_prev) {
        const float dn = ((fabsf(thr[0] - w.np[0]) + fabsf(thr[1] - w.np[1])) + fabsf(thr[2] - w.np[2])) / 100.0f;
        const float d1 = fabsf(ang[1] - w.ap[0]), d2 = fabsf(ang[2] - w.ap[1]);
        const float w1 = fminf(d1, 2.0f * kPi - d1), w2 = fminf(d2, 2.0f * kPi - d2);
        const float da = (w1 + w2) / kPi;
        w.rps += (double)dn;
        w.ang += (double)da;
    }
    w.np[0] = thr[0]; w.np[1] = thr[1]; w.np[2] = thr[2];
    w.ap[0] = ang[1]; w.ap[1] = ang[2];
    w.has_prev = 1u;
    if (end) {
        w.c_rps += w.rps; w.c_ang += w.ang;
        w.rps = 0.0; w.ang = 0.0; w.has_prev = 0u;
        w.np[0] = 0.0f; w.np[1] = 0.0f; w.np[2] = 0.0f; w.ap[0] = 0.0f; w.ap[1] = 0.0f;
    }
}

// score_kernel's scan - one lane per env, rows fetched SCORE_U ahead into two register banks, dead lanes shadowing the last env - with the
// wear state travelling beside the score state.  a.act is never NULL here (the host refuses it).
template <bool BF16, int MODE>
__global__ __launch_bounds__(64) void score_wear_kernel(const ScoreArgs a, uint4* __restrict__ wear)
{
    const int n = a.n, T = a.T;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const int il = live ? i : n - 1;                    // dead lanes shadow the last env and never store
    ScoreState s;
    WearState w;
    score_load(a.state, n, il, s);
    wear_load(wear, n, il, w);

    WearRow<MODE> A[SCORE_U], B[SCORE_U];
    auto load = [&](WearRow<MODE> (&buf)[SCORE_U], int j) {
#pragma unroll
        for (int u = 0; u < SCORE_U; ++u) {
            ScoreRow& r = buf[u].r;
            int t = j * SCORE_U + u;
            t = t < T ? t : T - 1;                      // past the end: re-read the last row (never consumed)
            const int64_t k = (int64_t)t * n + il;
#pragma unroll
            for (int c = 0; c < 3; ++c) { r.e[c] = 0.0f; r.g[c] = 0.0f; }
            if (a.obs) {
                if (BF16) {
                    const uint16_t* p = (const uint16_t*)a.obs + k * a.obs_stride;
#pragma unroll
                    for (int c = 0; c < 3; ++c) r.e[c] = __uint_as_float((uint32_t)p[c] << 16);
                } else {
                    const float* p = (const float*)a.obs + k * a.obs_stride;
#pragma unroll
                    for (int c = 0; c < 3; ++c) r.e[c] = p[c];
                }
            }
            if (a.integ) {
                const float* p = a.integ + k * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) r.g[c] = p[c];
            }
            const float* p = a.act + k * a.act_stride;  // the thrusts and, behind them, the variant's azimuth columns
#pragma unroll
            for (int c = 0; c < 3; ++c) r.a[c] = p[c];
#pragma unroll
            for (int c = 0; c < wear_ncol(MODE); ++c) buf[u].x[c] = p[wear_col0(MODE) + c];
            r.r = a.rew ? a.rew[k] : 0.0f;
            r.d = a.done ? (uint32_t)a.done[k] : 0u;
        }
    };
    auto consume = [&](const WearRow<MODE> (&buf)[SCORE_U], int j) {
#pragma unroll
        for (int u = 0; u < SCORE_U; ++u) {
            const int t = j * SCORE_U + u;
            if (t >= T) break;
            const bool end = score_row_update(a, s, buf[u].r, t);
            wear_row_update<MODE>(w, buf[u], end);
        }
    };
    const int nb = (T + SCORE_U - 1) / SCORE_U;
    load(A, 0);
    for (int j = 0; j < nb; j += 2) {
        load(B, j + 1);
        consume(A, j);
        load(A, j + 2);
        consume(B, j + 1);
    }
    if (live) {
        score_store(a.state, n, i, s);
        wear_store(wear, n, i, w);
    }
}

// the 4 read slots of one env (dpenv.h DPENV_SCORE_WEAR_*)
__device__ __forceinline__ void wear_slots(const WearState& w, double (&v)[WEAR_NOUT])
{
    v[0] = w.rps; v[1] = w.ang; v[2] = w.c_rps; v[3] = w.c_ang;
}

// out[slot][n] doubles
__global__ __launch_bounds__(64) void score_wear_read_kernel(const uint4* __restrict__ st, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    WearState w;
    wear_load(st, n, live ? i : n - 1, w);
    double v[WEAR_NOUT];
    wear_slots(w, v);
    if (live) {
#pragma unroll
        for (int k = 0; k < WEAR_NOUT; ++k) out[(int64_t)k * n + i] = v[k];
    }
}

// dpenv_kernels.hip's wave_sum_fixed (that unit's own): the same pairing every run
__device__ __forceinline__ double wear_wave_sum_fixed(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

// the score summary's two stages on the wear slots.  Stage 1: one wave per 64 envs leaves partials[block][slot][sum, min, max]
__global__ __launch_bounds__(64) void score_wear_summary_partial_kernel(const uint4* __restrict__ st, int n, double* __restrict__ partials)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    WearState w;
    wear_load(st, n, live ? i : n - 1, w);
    double v[WEAR_NOUT];
    wear_slots(w, v);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int k = 0; k < WEAR_NOUT; ++k) {
        const double sum = wear_wave_sum_fixed(live ? v[k] : 0.0);
        const double mn = wave_min_fixed(live ? v[k] : inf);
        const double mx = wave_max_fixed(live ? v[k] : -inf);
        if (threadIdx.x == 0) {
            double* p = partials + ((int64_t)blockIdx.x * WEAR_NOUT + k) * 3;
            p[0] = sum; p[1] = mn; p[2] = mx;
        }
    }
}

// stage 2: thread k folds partials k, k + 256, ... in index order, then a fixed tree over LDS: the same bits every run
__global__ __launch_bounds__(256) void score_wear_summary_final_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ out)
{
    __shared__ double red[3][256];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int slot = 0; slot < WEAR_NOUT; ++slot) {
        double sum = 0.0, mn = inf, mx = -inf;
        for (int k = threadIdx.x; k < nparts; k += 256) {
            const double* p = partials + ((int64_t)k * WEAR_NOUT + slot) * 3;
            sum += p[0]; mn = fmin(mn, p[1]); mx = fmax(mx, p[2]);
        }
        red[0][threadIdx.x] = sum; red[1][threadIdx.x] = mn; red[2][threadIdx.x] = mx;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) {
                red[0][threadIdx.x] += red[0][threadIdx.x + h];
                red[1][threadIdx.x] = fmin(red[1][threadIdx.x], red[1][threadIdx.x + h]);
                red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + h]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { out[slot * 3] = red[0][0]; out[slot * 3 + 1] = red[1][0]; out[slot * 3 + 2] = red[2][0]; }
        __syncthreads();
    }
}

template <bool BF16>
hipError_t launch_wear_mode(const ScoreArgs& a, uint4* wear, int mode, hipStream_t s)
{
    const dim3 grid((a.n + 63) / 64);
    switch (mode) {
    case MODE_FULL: hipLaunchKernelGGL((score_wear_kernel<BF16, MODE_FULL>), grid, dim3(64), 0, s, a, wear); break;
    case MODE_SIMPLE: hipLaunchKernelGGL((score_wear_kernel<BF16, MODE_SIMPLE>), grid, dim3(64), 0, s, a, wear); break;
    case MODE_LIMITED: hipLaunchKernelGGL((score_wear_kernel<BF16, MODE_LIMITED>), grid, dim3(64), 0, s, a, wear); break;
    case MODE_FINAL_WRAP: hipLaunchKernelGGL((score_wear_kernel<BF16, MODE_FINAL_WRAP>), grid, dim3(64), 0, s, a, wear); break;
    case MODE_FINAL_CONT: hipLaunchKernelGGL((score_wear_kernel<BF16, MODE_FINAL_CONT>), grid, dim3(64), 0, s, a, wear); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace dpenv

using namespace dpenv;

int64_t dev::score_wear_state_bytes(int n) { return (int64_t)n * WEAR_STREAMS * 16; }

int64_t dev::score_wear_summary_workspace_bytes(int n) { return (((int64_t)n + 63) / 64) * WEAR_NOUT * 3 * (int64_t)sizeof(double); }

hipError_t dev::launch_score_wear(const ScoreArgs* a, void* wear, int obs_bf16, int mode, hipStream_t s)
{
    if (!a->act) return hipErrorInvalidValue;
    return obs_bf16 ? launch_wear_mode<true>(*a, (uint4*)wear, mode, s) : launch_wear_mode<false>(*a, (uint4*)wear, mode, s);
}

hipError_t dev::launch_score_wear_read(const void* wear, int n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(score_wear_read_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const uint4*)wear, n, out);
    return hipGetLastError();
}

hipError_t dev::launch_score_wear_summary(const void* wear, int n, double* out, double* workspace, hipStream_t s)
{
    const int grid = (n + 63) / 64;
    hipLaunchKernelGGL(score_wear_summary_partial_kernel, dim3(grid), dim3(64), 0, s, (const uint4*)wear, n, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_wear_summary_final_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, grid, out);
    return hipGetLastError();
}
