// dpenv_score_dev.h - the streaming score card (dpenv_score_* in dpenv.h): box-test IAE, thruster work and returns accumulated on the
// device from the [T][n][.] row blocks the closed-loop launches write, one block at a time, so that scoring a flight needs O(n) memory
// instead of the O(T n) rows.  Included by dpenv_kernels.hip inside namespace dpenv (it owns the kernels and their launchers).
//
// State, caller-owned, all-zero = fresh: SCORE_STREAMS 16-byte streams st[s][n], every wave-level access one coalesced 1 KiB dwordx4:
//   0  (open iae, open work0)        f64 x 2        5  (q_prev, P_prev0, P_prev1, P_prev2)      f32 x 4
//   1  (open work1, open work2)                     6  (open len, has_prev, episodes, 0)        u32 x 4
//   2  (open ret, closed iae)                       7  (closed len, 0)                          u64 x 2
//   3  (closed work0, closed work1)
//   4  (closed work2, closed ret)
// 128 B per env, loaded once and stored once per call; a 50-row block moves 50 x 81 B of rows per env beside them.
#ifndef DPENV_SCORE_DEV_H
#define DPENV_SCORE_DEV_H

constexpr int SCORE_STREAMS = 8;
constexpr int SCORE_NOUT = 13;          // DPENV_SCORE_NOUT
// rows fetched ahead per register bank (two banks: one is consumed while the other lands).  A row is up to 11 loads per lane; measured at
// 65 536 envs x 50 rows (profiles/LAB_NOTES.md): 2 rows per bank 77 us, 4 rows 81 us, 8 rows 91 us - the lone wave per SIMD is bound by
// instruction issue as much as by the rows, and the shorter banks keep the loop small (85 VGPR).
constexpr int SCORE_U = 2;

struct ScoreRow {
    float e[3], a[3], g[3], r;
    uint32_t d;
};

struct ScoreState {
    double iae, w[3], ret, c_iae, c_w[3], c_ret;
    float qp, pp[3];
    uint32_t len, has_prev, episodes;
    uint64_t c_len;
};

__device__ __forceinline__ double2 score_d2(const uint4& q)
{
    double2 d;
    d.x = __hiloint2double((int)q.y, (int)q.x);
    d.y = __hiloint2double((int)q.w, (int)q.z);
    return d;
}
__device__ __forceinline__ uint4 score_u4(double x, double y)
{
    return make_uint4((uint32_t)__double2loint(x), (uint32_t)__double2hiint(x), (uint32_t)__double2loint(y), (uint32_t)__double2hiint(y));
}

// i must be a live index (dead lanes pass a clamped one)
__device__ __forceinline__ void score_load(const uint4* __restrict__ st, int n, int i, ScoreState& s)
{
    uint4 q[SCORE_STREAMS];
#pragma unroll
    for (int k = 0; k < SCORE_STREAMS; ++k) q[k] = st[(int64_t)k * n + i];
    double2 d;
    d = score_d2(q[0]); s.iae = d.x; s.w[0] = d.y;
    d = score_d2(q[1]); s.w[1] = d.x; s.w[2] = d.y;
    d = score_d2(q[2]); s.ret = d.x; s.c_iae = d.y;
    d = score_d2(q[3]); s.c_w[0] = d.x; s.c_w[1] = d.y;
    d = score_d2(q[4]); s.c_w[2] = d.x; s.c_ret = d.y;
    s.qp = __uint_as_float(q[5].x); s.pp[0] = __uint_as_float(q[5].y); s.pp[1] = __uint_as_float(q[5].z); s.pp[2] = __uint_as_float(q[5].w);
    s.len = q[6].x; s.has_prev = q[6].y; s.episodes = q[6].z;
    s.c_len = ((uint64_t)q[7].y << 32) | q[7].x;
}

__device__ __forceinline__ void score_store(uint4* __restrict__ st, int n, int i, const ScoreState& s)
{
    st[i] = score_u4(s.iae, s.w[0]);
    st[(int64_t)n + i] = score_u4(s.w[1], s.w[2]);
    st[2 * (int64_t)n + i] = score_u4(s.ret, s.c_iae);
    st[3 * (int64_t)n + i] = score_u4(s.c_w[0], s.c_w[1]);
    st[4 * (int64_t)n + i] = score_u4(s.c_w[2], s.c_ret);
    st[5 * (int64_t)n + i] = make_uint4(__float_as_uint(s.qp), __float_as_uint(s.pp[0]), __float_as_uint(s.pp[1]), __float_as_uint(s.pp[2]));
    st[6 * (int64_t)n + i] = make_uint4(s.len, s.has_prev, s.episodes, 0u);
    st[7 * (int64_t)n + i] = make_uint4((uint32_t)s.c_len, (uint32_t)(s.c_len >> 32), 0u, 0u);
}

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
            const ScoreRow& r = buf[u];
            float q = 0.0f, P[3] = {0.0f, 0.0f, 0.0f};
            if (a.obs) {
                const float e0 = (r.e[0] - r.g[0]) / a.norm[0];
                const float e1 = (r.e[1] - r.g[1]) / a.norm[1];
                const float e2 = ((r.e[2] - r.g[2]) * 57.295779513082323f) / a.norm[2];
                q = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
            }
            if (a.act) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float nn = fminf(fmaxf(r.a[c] * 100.0f, -100.0f), 100.0f);
                    const float x = (nn / 100.0f) * a.rps[c];
                    const float sg = nn > 0.0f ? 1.0f : (nn < 0.0f ? -1.0f : 0.0f);
                    P[c] = (sg * a.coeff[c]) * ((x * x) * x);
                }
            }
            if (s.has_prev) {
                if (a.obs) s.iae += (double)((0.5f * (q + s.qp)) * a.dt);
                if (a.act) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) s.w[c] += (double)((0.5f * (P[c] + s.pp[c])) * a.dt);
                }
            }
            if (a.rew) s.ret += (double)r.r;
            s.len += 1u;
            s.qp = q; s.pp[0] = P[0]; s.pp[1] = P[1]; s.pp[2] = P[2];
            s.has_prev = 1u;
            if (r.d != 0u || (a.cut_at_end && t == T - 1)) {
                s.c_iae += s.iae; s.c_ret += s.ret; s.c_len += s.len; s.episodes += 1u;
#pragma unroll
                for (int c = 0; c < 3; ++c) { s.c_w[c] += s.w[c]; s.w[c] = 0.0; }
                s.iae = 0.0; s.ret = 0.0; s.len = 0u; s.has_prev = 0u;
                s.qp = 0.0f; s.pp[0] = 0.0f; s.pp[1] = 0.0f; s.pp[2] = 0.0f;
            }
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

__device__ __forceinline__ double wave_min_fixed(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_down(x, off, 64));
    return x;
}
__device__ __forceinline__ double wave_max_fixed(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
    return x;
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
