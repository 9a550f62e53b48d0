// dpenv_qp_law.h - the rate-limited QP thrust allocation (dpenv_thrust_alloc_qp in include/dpenv.h, which states the law operation by
// operation): the reference's nonlinear "QP" allocator (qp_allocator.py:108-234) with the slack eliminated, solved by a fixed number of
// projected Levenberg-Marquardt steps with accept / reject.  The ONE text of the law on the device: included inside namespace dpenv by
// dpenv_control.hip, after dpenv_env_dev.h (sincos_lean, wrap_angle).  deploy.BatchedQPAllocator is the host statement.
//
// Everything is plain f32 in the stated order (the build has -ffp-contract=off; `/` and sqrtf are the compiler's correctly rounded forms),
// branch-free per lane apart from the iteration loop, whose count is wave-uniform.  Five unknowns per env: every array below is indexed
// by compile-time constants once the loops are unrolled, so the 5 x 5 factorisation lives in registers - a run-time index into one of
// them would send it to scratch.  No LDS, no calls.
#ifndef DPENV_QP_LAW_H
#define DPENV_QP_LAW_H

// x = (F_bow, F_port, F_star, a_port, a_star) and what the objective needs of it: sin / cos of the two azimuths, the pods' moment arms
// b3_i = lx_i sin a_i - ly_i cos a_i, the residual r = B(a) F - tau and J
struct QpPoint {
    float x[5];
    float s[2], c[2], b3[2];
    float r[3];
    float J;
};

template <class Q>
__device__ __forceinline__ void qp_evaluate(const Q& q, const float tau[3], const float prev[5], QpPoint& p)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sincos_lean(p.x[3 + i], p.s[i], p.c[i]);
        p.b3[i] = q.lx[1 + i] * p.s[i] - q.ly[1 + i] * p.c[i];
    }
    const float* F = p.x;
    p.r[0] = (p.c[0] * F[1] + p.c[1] * F[2]) - tau[0];
    p.r[1] = ((F[0] + p.s[0] * F[1]) + p.s[1] * F[2]) - tau[1];
    p.r[2] = ((q.lx[0] * F[0] + p.b3[0] * F[1]) + p.b3[1] * F[2]) - tau[2];
    const float Js = (q.ws[0] * (p.r[0] * p.r[0]) + q.ws[1] * (p.r[1] * p.r[1])) + q.ws[2] * (p.r[2] * p.r[2]);
    const float Jp = (fabsf(F[0]) * (F[0] * F[0]) + fabsf(F[1]) * (F[1] * F[1])) + fabsf(F[2]) * (F[2] * F[2]);
    float e2[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float e = p.x[k] - prev[k];
        e2[k] = e * e;
    }
    const float Ja = e2[3] + e2[4];
    const float Jf = (e2[0] + e2[1]) + e2[2];
    p.J = 0.5f * (((Js + q.wp * Jp) + q.wda * Ja) + q.wdf * Jf);
}

// One control step: state[5] (the thruster state in force) and tau[3] in; state[5] (azimuths wrapped to [-pi, pi)), the final variant's
// continuous-angle action act[7] and the final objective J out.  A tau that is not finite changes nothing: the env keeps its state and
// commands it.
template <class Q>
__device__ __forceinline__ void qp_allocate(const Q& q, const float tau[3], float state[5], float act[7], float& J_out)
{
    float prev[5], lo[5], hi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) prev[k] = state[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fmaxf(-q.fmax[k], prev[k] - q.dF[k]);
        hi[k] = fminf(q.fmax[k], prev[k] + q.dF[k]);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        lo[3 + k] = prev[3 + k] - q.da[k];
        hi[3 + k] = prev[3 + k] + q.da[k];
    }
    QpPoint p;
#pragma unroll
    for (int k = 0; k < 5; ++k) p.x[k] = fminf(fmaxf(prev[k], lo[k]), hi[k]);      // the state itself wherever |F| <= f_max
    qp_evaluate(q, tau, prev, p);
    float lam = 0.0f;

#pragma nounroll
    for (int it = 0; it < q.iters; ++it) {
        const float* F = p.x;
        // the 3 x 5 Jacobian of r: force columns b_i (the bow's is (0, 1, lx_bow)), angle columns F_i b_i'
        float Jm[3][5];
        Jm[0][0] = 0.0f; Jm[1][0] = 1.0f; Jm[2][0] = q.lx[0];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float d3 = q.lx[1 + i] * p.c[i] + q.ly[1 + i] * p.s[i];
            Jm[0][1 + i] = p.c[i];             Jm[1][1 + i] = p.s[i];             Jm[2][1 + i] = p.b3[i];
            Jm[0][3 + i] = -(F[1 + i] * p.s[i]); Jm[1][3 + i] = F[1 + i] * p.c[i]; Jm[2][3 + i] = F[1 + i] * d3;
        }
        float wr[3], WJ[3][5];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            wr[j] = q.ws[j] * p.r[j];
#pragma unroll
            for (int k = 0; k < 5; ++k) WJ[j][k] = q.ws[j] * Jm[j][k];
        }
        float g[5], H[5][5];                                     // H: the lower triangle only
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            g[k] = (Jm[0][k] * wr[0] + Jm[1][k] * wr[1]) + Jm[2][k] * wr[2];
#pragma unroll
            for (int l = 0; l <= k; ++l) H[k][l] = (Jm[0][k] * WJ[0][l] + Jm[1][k] * WJ[1][l]) + Jm[2][k] * WJ[2][l];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g[k] = g[k] + ((1.5f * q.wp) * (F[k] * fabsf(F[k])) + q.wdf * (F[k] - prev[k]));
            H[k][k] = H[k][k] + ((3.0f * q.wp) * fabsf(F[k]) + q.wdf);
        }
#pragma unroll
        for (int k = 3; k < 5; ++k) {
            g[k] = g[k] + q.wda * (p.x[k] - prev[k]);
            H[k][k] = H[k][k] + q.wda;
        }
        bool fr[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            H[k][k] = H[k][k] + lam * H[k][k];
            fr[k] = (p.x[k] <= lo[k] && g[k] > 0.0f) || (p.x[k] >= hi[k] && g[k] < 0.0f);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            g[k] = fr[k] ? 0.0f : g[k];
            H[k][k] = fr[k] ? 1.0f : H[k][k];
#pragma unroll
            for (int l = 0; l < k; ++l) H[k][l] = (fr[k] || fr[l]) ? 0.0f : H[k][l];
        }
        // H = L D L' without pivoting, L unit lower triangular; one division per pivot
        float L[5][5], D[5], iD[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float v[5];
#pragma unroll
            for (int m = 0; m < j; ++m) v[m] = L[j][m] * D[m];
            D[j] = H[j][j];
#pragma unroll
            for (int m = 0; m < j; ++m) D[j] = D[j] - L[j][m] * v[m];
            iD[j] = 1.0f / D[j];
#pragma unroll
            for (int i = j + 1; i < 5; ++i) {
                float t = H[i][j];
#pragma unroll
                for (int m = 0; m < j; ++m) t = t - L[i][m] * v[m];
                L[i][j] = t * iD[j];
            }
        }
        float y[5], d[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            float t = -g[i];
#pragma unroll
            for (int m = 0; m < i; ++m) t = t - L[i][m] * y[m];
            y[i] = t;
        }
#pragma unroll
        for (int i = 4; i >= 0; --i) {
            float t = y[i] * iD[i];
#pragma unroll
            for (int m = i + 1; m < 5; ++m) t = t - L[m][i] * d[m];
            d[i] = t;
        }
        QpPoint pt;
#pragma unroll
        for (int k = 0; k < 5; ++k) pt.x[k] = fminf(fmaxf(p.x[k] + d[k], lo[k]), hi[k]);
        qp_evaluate(q, tau, prev, pt);
        const bool acc = pt.J < p.J;                             // false for a NaN on either side
#pragma unroll
        for (int k = 0; k < 5; ++k) p.x[k] = acc ? pt.x[k] : p.x[k];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            p.s[i] = acc ? pt.s[i] : p.s[i];
            p.c[i] = acc ? pt.c[i] : p.c[i];
            p.b3[i] = acc ? pt.b3[i] : p.b3[i];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) p.r[j] = acc ? pt.r[j] : p.r[j];
        p.J = acc ? pt.J : p.J;
        lam = acc ? 0.25f * lam : 8.0f * fmaxf(lam, 0.125f);
    }

    const bool ok = isfinite(tau[0]) && isfinite(tau[1]) && isfinite(tau[2]);
    float xf[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) xf[k] = ok ? p.x[k] : prev[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        state[k] = xf[k];
        const float K = xf[k] >= 0.0f ? q.kf[k] : q.kr[k];
        const float nk = copysignf(sqrtf(fabsf(xf[k]) / K), xf[k]);
        act[k] = fminf(fmaxf(nk / 100.0f, -1.0f), 1.0f);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        state[3 + i] = ok ? wrap_angle(xf[3 + i], false) : prev[3 + i];
        sincos_lean(xf[3 + i], act[3 + 2 * i], act[4 + 2 * i]);
    }
    J_out = p.J;
}

// S(q, a) of include/dpenv.h (dpenv_controller_label_qp_ex): the thruster state an EXECUTED action row of the final variant's
// continuous-angle form leaves - the env's own command decode (env_decode_cmd<MODE_FINAL_CONT>: thrust percent, clipped azimuths), then
// the QP's thrust law F = K n |n| brought inside the law's precondition |F| <= f_max, the azimuths wrapped as qp_allocate wraps its state.
// A component fed by an action entry that is not finite (or that comes out not finite) is 0: thrusters at rest.  The ONLY statement of S
// on the device; deploy.qp_state_from_action is the host statement.
template <class Q>
__device__ __forceinline__ void qp_state_from_action(const Q& q, const float a[7], float x[5])
{
    float ang[3], thr[3];
    env_decode_cmd<MODE_FINAL_CONT>(ang, a, thr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float K = thr[k] >= 0.0f ? q.kf[k] : q.kr[k];
        float F = (K * thr[k]) * fabsf(thr[k]);
        F = fminf(fmaxf(F, -q.fmax[k]), q.fmax[k]);
        x[k] = (isfinite(a[k]) && isfinite(F)) ? F : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float al = wrap_angle(ang[1 + i], false);
        x[3 + i] = (isfinite(a[3 + 2 * i]) && isfinite(a[4 + 2 * i]) && isfinite(al)) ? al : 0.0f;
    }
}

// ---- one QP allocator per env (dpenv_set_qp_allocator_table, dpenv_thrust_alloc_qp_table): QpLane (dpenv_dev.h) holds an env's numbers in
// registers and qp_allocate<QpLane> above is the law, unedited ----

// The packed per-env block pack_qp_table_kernel writes, ctrl_tab_index's layout with QP_TAB_STREAMS streams: per wave of 64 envs seven
// float4 streams of 64 lanes, stream k of env i at qp_tab_index(i, k).  Flat slot q = 4 k + component:
// ws 0-2 | wp 3 | wda 4 | wdf 5 | fmax 6-8 | dF 9-11 | da 12-13 | lx 14-16 | ly 17-19 | kf 20-22 | kr 23-25 | 26, 27 pad
__host__ __device__ __forceinline__ int64_t qp_tab_index(int i, int k) { return ((int64_t)(i >> 6) * QP_TAB_STREAMS + k) * 64 + (i & 63); }

__device__ __forceinline__ void qp_lane_flatten(const QpLane& q, float f[4 * QP_TAB_STREAMS])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[k] = q.ws[k]; f[6 + k] = q.fmax[k]; f[9 + k] = q.dF[k]; f[14 + k] = q.lx[k]; f[17 + k] = q.ly[k]; f[20 + k] = q.kf[k];
        f[23 + k] = q.kr[k];
    }
    f[3] = q.wp; f[4] = q.wda; f[5] = q.wdf;
    f[12] = q.da[0]; f[13] = q.da[1];
    f[26] = f[27] = 0.0f;
}

// the env's numbers out of the packed block: seven 16-byte loads, checked and with dF / da formed when the block was packed
__device__ __forceinline__ void load_qp_lane(const float4* __restrict__ qtab, int il, int iters, QpLane& q)
{
    float f[4 * QP_TAB_STREAMS];
#pragma unroll
    for (int k = 0; k < QP_TAB_STREAMS; ++k) {
        const float4 v = qtab[qp_tab_index(il, k)];
        f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q.ws[k] = f[k]; q.fmax[k] = f[6 + k]; q.dF[k] = f[9 + k]; q.lx[k] = f[14 + k]; q.ly[k] = f[17 + k]; q.kf[k] = f[20 + k];
        q.kr[k] = f[23 + k];
    }
    q.wp = f[3]; q.wda = f[4]; q.wdf = f[5];
    q.da[0] = f[12]; q.da[1] = f[13];
    q.iters = iters;
}

// Row i of the PUBLIC table float[QP_NPARAM][n] -> the lane's numbers: dF = force_rate * dt and da = azimuth_rate * dt as one f32 product
// each (what the host forms for dpenv_set_qp_allocator), then dpenv_thrust_alloc_qp's checks.  A row that breaks one is replaced by the
// REST allocator - f_max = dF = da = 0, w_slack = w_power = 0, w_dalpha = w_dforce = 1, lx = ly = 0, kf = kr = 1: zero thrust, azimuths
// held, every output finite - and false is returned.  The ONLY statement of the per-row checks on the device: the packing kernel and the
// handle-free kernel both call it.
__device__ __forceinline__ bool qp_lane_from_row(const float* __restrict__ pub, int n, int i, float dt, int iters, QpLane& q)
{
    float p[QP_NREAD];
#pragma unroll
    for (int k = 0; k < QP_NREAD; ++k) p[k] = pub[(int64_t)k * n + i];
    float dF[3], da[2];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dF[k] = p[QP_FRATE + k] * dt;
        ok = ok && isfinite(p[QP_WSLACK + k]) && p[QP_WSLACK + k] >= 0.0f;
        ok = ok && isfinite(p[QP_FMAX + k]) && p[QP_FMAX + k] >= 0.0f;
        ok = ok && isfinite(p[QP_FRATE + k]) && p[QP_FRATE + k] >= 0.0f && isfinite(dF[k]);
        ok = ok && isfinite(p[QP_LX + k]) && isfinite(p[QP_LY + k]);
        ok = ok && isfinite(p[QP_KF + k]) && p[QP_KF + k] > 0.0f;
        ok = ok && isfinite(p[QP_KR + k]) && p[QP_KR + k] > 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        da[k] = p[QP_ARATE + k] * dt;
        ok = ok && isfinite(p[QP_ARATE + k]) && p[QP_ARATE + k] >= 0.0f && isfinite(da[k]);
    }
    ok = ok && isfinite(p[QP_WPOWER]) && p[QP_WPOWER] >= 0.0f;
    ok = ok && isfinite(p[QP_WDALPHA]) && p[QP_WDALPHA] > 0.0f;
    ok = ok && isfinite(p[QP_WDFORCE]) && p[QP_WDFORCE] > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q.ws[k] = ok ? p[QP_WSLACK + k] : 0.0f;
        q.fmax[k] = ok ? p[QP_FMAX + k] : 0.0f;
        q.dF[k] = ok ? dF[k] : 0.0f;
        q.lx[k] = ok ? p[QP_LX + k] : 0.0f;
        q.ly[k] = ok ? p[QP_LY + k] : 0.0f;
        q.kf[k] = ok ? p[QP_KF + k] : 1.0f;
        q.kr[k] = ok ? p[QP_KR + k] : 1.0f;
    }
    q.da[0] = ok ? da[0] : 0.0f;
    q.da[1] = ok ? da[1] : 0.0f;
    q.wp = ok ? p[QP_WPOWER] : 0.0f;
    q.wda = ok ? p[QP_WDALPHA] : 1.0f;
    q.wdf = ok ? p[QP_WDFORCE] : 1.0f;
    q.iters = iters;
    return ok;
}

#endif
