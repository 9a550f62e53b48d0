// dpenv_score_dev.h - the streaming score card (dpenv_score_* in dpenv.h): box-test IAE, thruster work and returns accumulated on the
// device from the [T][n][.] row blocks the closed-loop launches write, one block at a time, so that scoring a flight needs O(n) memory
// instead of the O(T n) rows.  Included by dpenv_kernels.hip inside namespace dpenv (it owns the kernels and their launchers).
//
// The state of one env, its stream I/O and the per-row update are dpenv_score_lane.h's, shared with the one-pass score + wear scan of
// dpenv_score_wear.hip.  The row fetch stands here and, widened, there: as a shared __forceinline__ function it re-scheduled score_kernel
// (tools/isa_diff.py against the kernel before; with the update alone shared both instantiations are the same instruction stream).
#ifndef DPENV_SCORE_DEV_H
#define DPENV_SCORE_DEV_H

#include "dpenv_score_lane.h"

// the 13 read slots of one env (dpenv.h DPENV_SCORE_*)
__device__ __forceinline__ void score_slots(const ScoreState& s, double (&v)[SCORE_NOUT])
{
    v[0] = s.iae; v[1] = s.w[0]; v[2] = s.w[1]; v[3] = s.w[2]; v[4] = s.ret; v[5] = (double)s.len; v[6] = (double)s.episodes;
    v[7] = s.c_iae; v[8] = s.c_w[0]; v[9] = s.c_w[1]; v[10] = s.c_w[2]; v[11] = s.c_ret; v[12] = (double)s.c_len;
}

// Forward scan over the T rows of a block, one lane per env.  The update is serial in t, but no load depends on it: rows are fetched
// SCORE_U at a time into one of two register banks while the other is consumed (gae_kernel's scheme, forwards).  Per-sample terms are
// f32 in the order dpenv.h states; the sums are f64.  Missing blocks (NULL) are wave-uniform branches.
template <bool BF16>
__global__ __launch_bounds__(64) void score_kernel(const ScoreArgs a)
{
    const int n = a.n, T = a.T;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const int il = live ? i : n - 1;                    // dead lanes shadow the last env and never store
    ScoreState s;
    score_load(a.state, n, il, s);

    ScoreRow A[SCORE_U], B[SCORE_U];
    auto load = [&](ScoreRow (&buf)[SCORE_U], int j) {
#pragma unroll
        for (int u = 0; u < SCORE_U; ++u) {
            int t = j * SCORE_U + u;
            t = t < T ? t : T - 1;                      // past the end: re-read the last row (never consumed)
            const int64_t k = (int64_t)t * n + il;
#pragma unroll
            for (int c = 0; c < 3; ++c) { buf[u].e[c] = 0.0f; buf[u].a[c] = 0.0f; buf[u].g[c] = 0.0f; }
            if (a.obs) {
                if (BF16) {
                    const uint16_t* p = (const uint16_t*)a.obs + k * a.obs_stride;
#pragma unroll
                    for (int c = 0; c < 3; ++c) buf[u].e[c] = __uint_as_float((uint32_t)p[c] << 16);
                } else {
                    const float* p = (const float*)a.obs + k * a.obs_stride;
#pragma unroll
                    for (int c = 0; c < 3; ++c) buf[u].e[c] = p[c];
                }
            }
            if (a.integ) {
                const float* p = a.integ + k * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) buf[u].g[c] = p[c];
            }
            if (a.act) {
                const float* p = a.act + k * a.act_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) buf[u].a[c] = p[c];
            }
            buf[u].r = a.rew ? a.rew[k] : 0.0f;
            buf[u].d = a.done ? (uint32_t)a.done[k] : 0u;
        }
    };
    auto consume = [&](const ScoreRow (&buf)[SCORE_U], int j) {
#pragma unroll
        for (int u = 0; u < SCORE_U; ++u) {
            const int t = j * SCORE_U + u;
            if (t >= T) break;
            score_row_update(a, s, buf[u], t);
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
    if (live) score_store(a.state, n, i, s);
}

// out[slot][n] doubles
__global__ __launch_bounds__(64) void score_read_kernel(const uint4* __restrict__ st, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    ScoreState s;
    score_load(st, n, live ? i : n - 1, s);
    double v[SCORE_NOUT];
    score_slots(s, v);
    if (live) {
#pragma unroll
        for (int k = 0; k < SCORE_NOUT; ++k) out[(int64_t)k * n + i] = v[k];
    }
}

// stage 1: one wave per 64 envs leaves partials[block][slot][sum, min, max]; dead lanes carry the neutral elements
__global__ __launch_bounds__(64) void score_summary_partial_kernel(const uint4* __restrict__ st, int n, double* __restrict__ partials)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    ScoreState s;
    score_load(st, n, live ? i : n - 1, s);
    double v[SCORE_NOUT];
    score_slots(s, v);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int k = 0; k < SCORE_NOUT; ++k) {
        const double sum = wave_sum_fixed(live ? v[k] : 0.0);
        const double mn = wave_min_fixed(live ? v[k] : inf);
        const double mx = wave_max_fixed(live ? v[k] : -inf);
        if (threadIdx.x == 0) {
            double* p = partials + ((int64_t)blockIdx.x * SCORE_NOUT + k) * 3;
            p[0] = sum; p[1] = mn; p[2] = mx;
        }
    }
}

// stage 2: thread k folds partials k, k + 256, ... in index order, then a fixed tree over LDS: the same bits every run
__global__ __launch_bounds__(256) void score_summary_final_kernel(const double* __restrict__ partials, int nparts, double* __restrict__ out)
{
    __shared__ double red[3][256];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int slot = 0; slot < SCORE_NOUT; ++slot) {
        double sum = 0.0, mn = inf, mx = -inf;
        for (int k = threadIdx.x; k < nparts; k += 256) {
            const double* p = partials + ((int64_t)k * SCORE_NOUT + slot) * 3;
            sum += p[0]; mn = fmin(mn, p[1]); mx = fmax(mx, p[2]);
        }
        red[0][threadIdx.x] = sum; red[1][threadIdx.x] = mn; red[2][threadIdx.x] = mx;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                red[0][threadIdx.x] += red[0][threadIdx.x + w];
                red[1][threadIdx.x] = fmin(red[1][threadIdx.x], red[1][threadIdx.x + w]);
                red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + w]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { out[slot * 3] = red[0][0]; out[slot * 3 + 1] = red[1][0]; out[slot * 3 + 2] = red[2][0]; }
        __syncthreads();
    }
}

#endif
