// dpenv_control_rollout_body.inc - the body of controller_rollout_kernel, controller_rollout_tab_kernel and controller_rollout_qp_kernel
// (dpenv_control.hip), included into each (see dpenv_policy_rollout_body.inc for why it is spliced, not called).  In scope: a (StepArgs), ca (ControlArgs), fa
// (FilterArgs), the compile-time TAB and, if TAB, tab (the packed per-env controller block, ctrl_tab_index), the compile-time QP and, if QP,
// qr (QpRollout: the rate-limited QP allocation of dpenv_qp_law.h in place of dp_allocate, its thruster state carried beside z), the
// compile-time QTAB (with QP) and, if QTAB, qtab (the packed per-env QP block, qp_tab_index: the env's own numbers in place of qr.q's,
// of which only iters is read); the compile-time NN and, if NN, nr (NnRollout: the neural allocation of dpenv_nn_law.h in place of
// dp_allocate; it has no state); the rest are the kernel's template arguments.
    constexpr int MODE = MODE_FINAL_CONT;
    constexpr bool EXT = true;
    constexpr int A = 7, OD = 9;
    constexpr bool RND = VES == VES_ENV_RND, PER_ENV = VES == VES_ENV_VGPR || RND;
    constexpr int IL = VES == VES_ARGS_LOSS ? IL_SHARED : IL_NONE;
    constexpr bool CURR = RND || VES == VES_ARGS_LOSS;
    __shared__ float lds_row[RBLOCK * 9];

    const int tid = threadIdx.x;
    const int n = a.n;
    const int wave0 = blockIdx.x * RBLOCK;
    const int i = wave0 + tid;
    const bool live = i < n;
    const int il = live ? i : n - 1;

    Env s;
    load_env(a, il, s);
    ControlLane cl;                                              // TAB: the env's own numbers, read once, in the opening burst
    if constexpr (TAB) load_control_lane(tab, il, ca.dt, cl);
    QpLane ql;                                                   // QTAB: the env's own QP numbers, likewise
    if constexpr (QTAB) load_qp_lane(qtab, il, qr.q.iters, ql);
    sincos_lean(s.psi, s.sn, s.cs);
    Current cur = {0.0f, 0.0f, 0.0f, 0.0f, 0u};
    float vc0 = 0.0f, beta0 = 0.0f;
    if (a.cur_vc) {
        cur.vc = a.cur_vc[il]; cur.beta = a.cur_beta[il];
        if (a.current_drift) { vc0 = a.cur_vc0[il]; beta0 = a.cur_beta0[il]; cur.ctr = a.drift_ctr[il]; }
        current_components(cur);
    }
    Vessel ve = PER_ENV ? vessel_from_env(a.env_tab, a.env_stride, il) : vessel_from_args(a.v0);
    if (!PER_ENV) pin_vessel_in_vgprs(ve);
    uint32_t episode = a.auto_reset ? (uint32_t)a.episode[il] : 0u;
    bool ep_dirty = false, rf_dirty = false, cur_dirty = false;

    const int64_t stride_a = (int64_t)n * A, stride_o = (int64_t)n * OD;
    const int64_t w_a = (int64_t)wave0 * A, w_o = (int64_t)wave0 * OD;       // the wave's slice of a [T][n][.] block
    const int64_t rem_a = stride_a - w_a, rem_o = stride_o - w_o;

    // observation of the current state = controller input of step 0 (ENV:196-205)
    float o[9];
    {
        float sr_, cr_;
        bool same_;
        make_obs(s.N, s.E, s.psi, s.u, s.v, s.r, s.refN, s.refE, s.refPsi, s.pt, a.wrap_mode == WRAP_REFERENCE, o, sr_, cr_, same_);
    }
    if (ca.use_lag) {                                            // continue the episode with the observation the last launch ended with
        const float4 lg = a.S3[il];
        o[6] = lg.x; o[7] = lg.y; o[8] = lg.z;
    }
    float z[3];
    {
        const float4 q = ca.z[il];
        z[0] = q.x; z[1] = q.y; z[2] = q.z;
    }
    float xq[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};                // QP: the thruster state in force
    if constexpr (QP) {
#pragma unroll
        for (int k = 0; k < 5; ++k) xq[k] = qr.state[(int64_t)k * n + il];
    }
    ReffState fs{};
    if constexpr (REFF) {
        fs = reff_load(fa, il, n);
        reff_row(fa, 0, n, i, live, s.refN, s.refE, s.refPsi);  // the reference o_0 was formed against
        s.refN = fs.x[0][0]; s.refE = fs.x[1][0]; s.refPsi = fs.x[2][0];   // the last launch's pending new_ref is in force from step 0
    }

    int next_switch = 0;
    for (int t = 0; t < ca.T; ++t) {
        control_store_rows<OD>(lds_row, ca.obs, (int64_t)t * stride_o + w_o, rem_o, o, tid, a.obs_bf16 != 0);
        float act[A];
        if constexpr (NN) {                                      // the PID's wrench, allocated by the network
            float tau[3], p[6];
            dp_wrench(ca, o, z, tau);
            nn_allocate<true>(nr.a, nn_lds() + tid, tau, act, p);
        } else if constexpr (QP) {                               // the PID's wrench, allocated by the QP law
            float tau[3], J;
            dp_wrench(ca, o, z, tau);
            if constexpr (QTAB) qp_allocate(ql, tau, xq, act, J);
            else qp_allocate(qr.q, tau, xq, act, J);
        } else if constexpr (TAB) dp_control(cl, o, z, act);
        else dp_control(ca, o, z, act);
        control_store_rows<A>(lds_row, ca.act, (int64_t)t * stride_a + w_a, rem_a, act, tid, false);

        bool has_ref = false;
        float nrN = 0.0f, nrE = 0.0f, nrP = 0.0f;
        if (next_switch < ca.n_switch && ca.switch_step[next_switch] == t) {   // wave-uniform
            const float* rp = ca.refs + (int64_t)next_switch * 3 * n;
            nrN = rp[il]; nrE = rp[(int64_t)n + il]; nrP = rp[2 * (int64_t)n + il];
            has_ref = true; rf_dirty = true;
            ++next_switch;
        }
        if constexpr (REFF) {                                    // a switch sets the filter's target; its position is the step's new_ref
            if (has_ref) reff_target(fs, nrN, nrE, nrP);
            reff_advance(fa, fs);
            nrN = fs.x[0][0]; nrE = fs.x[1][0]; nrP = fs.x[2][0];
            has_ref = t + 1 < ca.T; rf_dirty = true;             // the last step's stays pending in the filter
            if (t + 1 < ca.T) reff_row(fa, t + 1, n, i, live, s.refN, s.refE, s.refPsi);
        }
        StepOut out;
        env_step<MODE, EXT>(a, ve, s, act, has_ref, nrN, nrE, nrP, a.cur_vc != nullptr, cur.vcN, cur.vcE, out, RND ? il : IL);
        if (a.current_drift) current_drift_step(a, cur, vc0, beta0, a.env_id_base + i);
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = out.o[k];
        if (a.auto_reset && out.d != 0u && live) {
            if constexpr (REFF) {                                // the last step's pending new_ref: a re-drawn env keeps it as its reference
                if (t == ca.T - 1) { s.refN = fs.x[0][0]; s.refE = fs.x[1][0]; s.refPsi = fs.x[2][0]; }
            }
            env_auto_reset<MODE>(a, s, a.env_id_base + i, episode, o);
            if (RND && a.rand_tab) redraw_vessel(a, i, episode, ve);   // domain randomisation: the new episode runs on a new hull
            if (CURR && a.cur_nom) { current_redraw_inline(a, i, episode, cur, vc0, beta0); cur_dirty = true; }  // ... in a new current
            ++episode; ep_dirty = true; rf_dirty = true;
            z[0] = z[1] = z[2] = 0.0f;                           // the new episode's first action is the law at z = 0
            if constexpr (QP) {                                  // ... and from thrusters at rest
#pragma unroll
                for (int k = 0; k < 5; ++k) xq[k] = 0.0f;
            }
            if constexpr (REFF) {                                // ... and the filter at rest on its reference
                reff_rest(fs, s.refN, s.refE, s.refPsi);
                if (t + 1 < ca.T) reff_row(fa, t + 1, n, i, live, s.refN, s.refE, s.refPsi);
            }
        }
        if (live) {
            (ca.rew + (int64_t)t * n)[(unsigned)i] = out.reward;
            (ca.done + (int64_t)t * n)[(unsigned)i] = (uint8_t)out.d;
        }
    }
    // observation after the last step (controller input of the next launch) and final state
    control_store_rows<OD>(lds_row, ca.last_obs, w_o, rem_o, o, tid, a.obs_bf16 != 0);
    if (live) {
        store_env(a, i, s, rf_dirty);
        a.S3[i] = make_float4(o[6], o[7], o[8], 0.0f);
        ca.z[i] = make_float4(z[0], z[1], z[2], 0.0f);
        if constexpr (QP) {
#pragma unroll
            for (int k = 0; k < 5; ++k) qr.state[(int64_t)k * n + i] = xq[k];
        }
        if (ep_dirty) a.episode[i] = (int)episode;
        if (a.current_drift) { a.cur_vc[i] = cur.vc; a.cur_beta[i] = cur.beta; a.drift_ctr[i] = cur.ctr; }
        if (CURR && cur_dirty) store_current(a, i, cur, vc0, beta0, true);
        if constexpr (REFF) reff_store(fa, i, n, fs);
    }
