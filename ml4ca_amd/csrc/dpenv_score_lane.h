// dpenv_score_lane.h - what one lane of the streaming score card holds and does per row: the state of one env, its 16-byte stream I/O and
// the per-row update dpenv.h states.  Shared by score_kernel (dpenv_score_dev.h, in dpenv_kernels.hip) and the one-pass score + wear scan
// (dpenv_score_wear.hip), so that the law stands once and the two leave the same score bytes.  Included inside namespace dpenv; no kernels.
//
// State, caller-owned, all-zero = fresh: SCORE_STREAMS 16-byte streams st[s][n], every wave-level access one coalesced 1 KiB dwordx4:
//   0  (open iae, open work0)        f64 x 2        5  (q_prev, P_prev0, P_prev1, P_prev2)      f32 x 4
//   1  (open work1, open work2)                     6  (open len, has_prev, episodes, 0)        u32 x 4
//   2  (open ret, closed iae)                       7  (closed len, 0)                          u64 x 2
//   3  (closed work0, closed work1)
//   4  (closed work2, closed ret)
// 128 B per env, loaded once and stored once per call; a 50-row block moves 50 x 81 B of rows per env beside them.
#ifndef DPENV_SCORE_LANE_H
#define DPENV_SCORE_LANE_H

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

// The per-row update of dpenv.h for row t of a T-row block: per-sample terms f32 in the stated order, sums f64.  Returns whether the row
// ended the env's episode (a non-zero done byte, or cut_at_end on the last row).
__device__ __forceinline__ bool score_row_update(const ScoreArgs& a, ScoreState& s, const ScoreRow& r, int t)
{
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
    const bool end = r.d != 0u || (a.cut_at_end && t == a.T - 1);
    if (end) {
        s.c_iae += s.iae; s.c_ret += s.ret; s.c_len += s.len; s.episodes += 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s.c_w[c] += s.w[c]; s.w[c] = 0.0; }
        s.iae = 0.0; s.ret = 0.0; s.len = 0u; s.has_prev = 0u;
        s.qp = 0.0f; s.pp[0] = 0.0f; s.pp[1] = 0.0f; s.pp[2] = 0.0f;
    }
    return end;
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

#endif
