// dpenv_label_qp_body.inc - the body of controller_label_qp_kernel and controller_label_qp_ex_kernel (dpenv_label.hip), included into each
// (see dpenv_policy_rollout_body.inc for why it is spliced, not called).  In scope: ca (ControlArgs), qa (QpArgs), la (LabelQpArgs), xa
// (LabelQpExArgs), tab (the packed per-env controller block) and the compile-time TAB, QTAB, FLOWN and BF16.  controller_label_qp_kernel
// is the body with QTAB = FLOWN = false and an empty xa, which the compiler folds away.
//
// controller_label_kernel's scan with the rate-limited QP allocation behind the PID lines (dpenv_controller_label_qp): per row the closed
// loop's QP branch (dpenv_control_rollout_body.inc) - dp_wrench on the env's z, qp_allocate on its thruster state x - and both zeroed
// behind a done row.  z[3] and x[5] come in with the opening burst and go out once at the end.  About 620 VALU instructions per LM
// iteration stand against 7 loads per row, so the fetch is one row ahead and no deeper: row t + 1 is in flight under the solve of row t.
// The iteration count is a kernel argument, the loop wave-uniform; dead lanes solve env n - 1's rows again and store nothing.
//
// The two things dpenv_controller_label_qp_ex adds, same scheme (one wave per workgroup, one lane per env, row t + 1 in flight under the
// solve of row t, a wave-uniform iteration loop):
// FLOWN: the thruster state row t + 1 is solved from is S (qp_state_from_action) of the action row t that was EXECUTED, not the law's own
//   advance of x, which is dropped.  The flown row t is fetched with obs row t - 28 more bytes per lane at the act rows' 28-byte stride (one
//   16-byte and one 12-byte load), straight into registers like the 36-byte obs rows beside them: they land under the ~620 K VALU
//   instructions of the previous row's solve, so staging them coalesced through the LDS area would buy nothing the scan can see and cost
//   a wait the loads do not have (measured: 1.016 x the own recursion at 65 536 envs x 50 rows, DESIGN.md section 7).
// QTAB: the lane's own row of the PUBLIC QP table, 26 loads in the opening burst, checked by qp_lane_from_row; QpLane goes through
//   qp_allocate<QpLane> unedited.  A refused row runs the rest allocator, reports NaN in cost and sets its byte of refused.  qa is not read.
// Dead lanes shadow env n - 1 and store nothing, refused included.
    constexpr int A = 7, OD = 9;
    __shared__ float lds_row[64 * A];

    const int n = la.n, T = la.T;
    const LabelLane L = label_lane(n);
    const int lane = L.lane, wave0 = L.wave0, i = L.i, il = L.il;
    const bool live = L.live;

    ControlLane cl;
    if constexpr (TAB) load_control_lane(tab, il, ca.dt, cl);
    QpLane ql;
    bool row_ok = true;
    if constexpr (QTAB) {
        row_ok = qp_lane_from_row(xa.qp_table, n, il, ca.dt, xa.iters, ql);
        if (live && xa.refused) xa.refused[i] = row_ok ? 0 : 1;
    }
    float z[3] = {0.0f, 0.0f, 0.0f};
    if (la.z_in) {
        z[0] = la.z_in[il]; z[1] = la.z_in[(int64_t)n + il]; z[2] = la.z_in[2 * (int64_t)n + il];
    }
    float x[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (la.x_in) {
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = la.x_in[(int64_t)k * n + il];
    }

    const int64_t stride_a = (int64_t)n * A;
    const int64_t w_a = (int64_t)wave0 * A;                      // the wave's slice of the [T][n][7] block
    const int64_t rem_a = stride_a - w_a;

    auto load = [&](LabelRowEx<FLOWN>& row, int t) {
        t = t < T ? t : T - 1;                                   // past the end: re-read the last row (never consumed)
        const int64_t k = (int64_t)t * n + il;
        if (BF16) {
            const uint16_t* p = (const uint16_t*)la.obs + k * OD;
#pragma unroll
            for (int c = 0; c < 6; ++c) row.o[c] = __uint_as_float((uint32_t)p[c] << 16);
        } else {
            const float* p = (const float*)la.obs + k * OD;
#pragma unroll
            for (int c = 0; c < 6; ++c) row.o[c] = p[c];
        }
        row.d = la.done ? (uint32_t)la.done[k] : 0u;
        if constexpr (FLOWN) {
            const float* f = xa.flown + k * A;
#pragma unroll
            for (int c = 0; c < A; ++c) row.f[c] = f[c];
        }
    };
    LabelRowEx<FLOWN> cur, nxt;
    load(cur, 0);
    for (int t = 0; t < T; ++t) {
        load(nxt, t + 1);
        float o[OD], tau[3], act[A], J;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = cur.o[c];
        o[6] = o[7] = o[8] = 0.0f;                               // the thrust columns: the law does not read them
        if constexpr (TAB) dp_wrench(cl, o, z, tau);
        else dp_wrench(ca, o, z, tau);
        if constexpr (QTAB) qp_allocate(ql, tau, x, act, J);
        else qp_allocate(qa, tau, x, act, J);
        if constexpr (FLOWN) {                                   // the law's own advance of x is dropped: the executed row's state
            if constexpr (QTAB) qp_state_from_action(ql, cur.f, x);
            else qp_state_from_action(qa, cur.f, x);
        }
        control_store_rows<A>(lds_row, la.act, (int64_t)t * stride_a + w_a, rem_a, act, lane, false);
        if (live && la.cost) (la.cost + (int64_t)t * n)[(unsigned)i] = row_ok ? J : __builtin_nanf("");
        if (cur.d != 0u) {                                       // the next row is a new episode's first: thrusters at rest
            z[0] = z[1] = z[2] = 0.0f;
#pragma unroll
            for (int k = 0; k < 5; ++k) x[k] = 0.0f;
        }
        cur = nxt;
    }
    if (live && la.z_out) {
        la.z_out[i] = z[0]; la.z_out[(int64_t)n + i] = z[1]; la.z_out[2 * (int64_t)n + i] = z[2];
    }
    if (live && la.x_out) {
#pragma unroll
        for (int k = 0; k < 5; ++k) la.x_out[(int64_t)k * n + i] = x[k];
    }
