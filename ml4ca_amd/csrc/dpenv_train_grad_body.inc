// dpenv_train_grad_body.inc - the body of the gradient kernels of dpenv_train.hip, included once per __global__ function so that every
// kernel holds the same text directly (a shared device function, even a forced-inline one, changes how the argument block is fetched
// and with it the schedule of the existing kernels).  Expects in scope: the kernel's argument `GradArgs a` and `constexpr int STAGE`
// (TR_STAGE_*), which selects the per-row output stage and what it fetches of a row at compile time.
// The fifth stage, TR_STAGE_ALLOC (dpenv.h, ALLOCATION LOSS), reads numbers of its own, `AllocLossArgs q`, which only its kernel has:
// everything it adds stands between #ifdef TR_BODY_ALLOC and #endif, so the text the other four kernels compile is the text without it.
    extern __shared__ float lds[];
    constexpr bool ACTOR = STAGE != TR_STAGE_VALUE;           // a policy network: actions and log_std
#ifdef TR_BODY_ALLOC
    constexpr bool IMIT = true;                               // a row is fetched as the imitation stages fetch it: the act slot (tau) and the weight or 1
#else
    constexpr bool IMIT = STAGE == TR_STAGE_IMIT_NLL || STAGE == TR_STAGE_IMIT_MSE;
#endif
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
                if constexpr (!IMIT) {
                    if (part == 1) lds[O_AUX + row * 2 + 1] = ok ? a.logp_old[src] : 0.0f;
                }
            }
            if constexpr (IMIT) {                               // the row's weight in the advantage's slot; no weights = 1
                if (part == 0) lds[O_AUX + row * 2] = ok ? (a.adv ? a.adv[src] : 1.0f) : 0.0f;
            } else {
                if (part == 0) lds[O_AUX + row * 2] = ok ? a.adv[src] : 0.0f;
            }
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
#ifdef TR_BODY_ALLOC
                if constexpr (STAGE == TR_STAGE_ALLOC) {
                    // dpenv.h, ALLOCATION LOSS: the QP law's objective at the network's output p = d[0..5], tau = ra[0..2]; env order i = bow,
                    // port, star reads p_j with j = 2, 0, 1.  Every index below is a compile-time constant once unrolled: no scratch.
                    const float w = lds[O_AUX + row * 2];
                    float F[3], e[3], dFdp[3], pj[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        pj[i] = d[i == 0 ? 2 : i - 1];
                        const float n = 100.0f * fminf(fmaxf(pj[i], -1.0f), 1.0f);
                        const float K = n >= 0.0f ? q.kf[i] : q.kr[i];
                        F[i] = (K * n) * fabsf(n);
                        e[i] = fmaxf(fabsf(pj[i]) - 1.0f, 0.0f);
                        dFdp[i] = fabsf(pj[i]) <= 1.0f ? (200.0f * K) * fabsf(n) : 0.0f;
                    }
                    float sn[2], cs[2], b3[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float ang = q.azimuth_mode == 0 ? d[3 + k] * q.angle_scale : q.azimuth[k];
                        sincos_lean(ang, sn[k], cs[k]);
                        b3[k] = q.lx[1 + k] * sn[k] - q.ly[1 + k] * cs[k];
                    }
                    float r[3];
                    r[0] = (cs[0] * F[1] + cs[1] * F[2]) - ra[0];
                    r[1] = ((F[0] + sn[0] * F[1]) + sn[1] * F[2]) - ra[1];
                    r[2] = ((q.lx[0] * F[0] + b3[0] * F[1]) + b3[1] * F[2]) - ra[2];
                    const float Js = (q.ws[0] * (r[0] * r[0]) + q.ws[1] * (r[1] * r[1])) + q.ws[2] * (r[2] * r[2]);
                    const float Jp = (fabsf(F[0]) * (F[0] * F[0]) + fabsf(F[1]) * (F[1] * F[1])) + fabsf(F[2]) * (F[2] * F[2]);
                    const float Jx = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                    const float J = 0.5f * ((Js + q.wp * Jp) + q.wsat * Jx);
                    const float wr[3] = {q.ws[0] * r[0], q.ws[1] * r[1], q.ws[2] * r[2]};
                    // the Jacobian's force columns: bow (0, 1, lx_b), pods (c_k, s_k, b3_k); its angle columns F_k (-s_k, c_k, lx_k c_k + ly_k s_k)
                    const float Jf[3][3] = {{0.0f, cs[0], cs[1]}, {1.0f, sn[0], sn[1]}, {q.lx[0], b3[0], b3[1]}};
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float gF = ((Jf[0][i] * wr[0] + Jf[1][i] * wr[1]) + Jf[2][i] * wr[2]) + (1.5f * q.wp) * (F[i] * fabsf(F[i]));
                        d[i == 0 ? 2 : i - 1] = w * (gF * dFdp[i] + q.wsat * copysignf(e[i], pj[i]));
                    }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float d3 = q.lx[1 + k] * cs[k] + q.ly[1 + k] * sn[k];
                        const float ga = (-(F[1 + k] * sn[k]) * wr[0] + (F[1 + k] * cs[k]) * wr[1]) + (F[1 + k] * d3) * wr[2];
                        d[3 + k] = q.azimuth_mode == 0 ? w * (q.angle_scale * ga) : 0.0f;
                    }
                    for (int j = 5; j < TR_PAD; ++j) d[j] = 0.0f;       // a_bow is not used; the log_std part is +0.0
                    st[0] = w * J;
                    st[1] = w * Js;
                    st[2] = w * Jp;
                    st[3] = w * Jx;
                } else
#endif
                if constexpr (IMIT) {
                    // dpenv.h, IMITATION LOSS: both losses' row statistics, the gradient of the chosen one
                    const float w = lds[O_AUX + row * 2];
                    float logp = 0.0f, se = 0.0f;
                    for (int j = 0; j < od; ++j) {
                        const float q = (ra[j] - d[j]) / lds[O_LS + TR_PAD + j];
                        logp += -0.5f * ((q * q + 2.0f * lds[O_LS + j]) + 1.8378770664093453f);
                        const float e = d[j] - ra[j];
                        se += e * e;
                    }
                    if constexpr (STAGE == TR_STAGE_IMIT_NLL) {
                        const float gl = -w;                                                     // dL/dlogp x count
                        for (int j = 0; j < od; ++j) {
                            const float sd = lds[O_LS + TR_PAD + j];
                            const float q = (ra[j] - d[j]) / sd;
                            d[j] = gl * (q / sd);
                            d[od + j] = gl * (q * q * (lds[O_LS + 2 * TR_PAD + j] / sd) - 1.0f);
                        }
                    } else {
                        const float w2 = 2.0f * w;
                        for (int j = 0; j < od; ++j) {
                            d[j] = w2 * (d[j] - ra[j]);
                            d[od + j] = 0.0f;
                        }
                    }
                    for (int j = 2 * od; j < TR_PAD; ++j) d[j] = 0.0f;
                    const float nll = w * -logp, mse = w * se;
                    st[0] = STAGE == TR_STAGE_IMIT_NLL ? nll : mse;
                    st[1] = nll;
                    st[2] = mse;
                    st[3] = 0.0f;
                } else if (ACTOR) {
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
