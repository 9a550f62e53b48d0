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

#endif
