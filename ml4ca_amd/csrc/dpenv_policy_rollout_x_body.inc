// dpenv_policy_rollout_x_body.inc - the body of policy_rollout_x_kernel, policy_rollout_x_integ_kernel and policy_rollout_x_reff_kernel
// (dpenv_policy_x.hip), included into each (see dpenv_policy_rollout_body.inc for why it is spliced, not called).  In scope: a, pa, ia, fa
// and the compile-time INTEG and REFF.
    constexpr int A = ModeTraits<MODE>::A;
    constexpr int OD = EXT ? 9 : 6;
    extern __shared__ uint4 lds_dyn[];
    stage_weights(lds_dyn, pa);
    const SplitNets nets = split_nets(lds_dyn, pa);
    const float leak = pa.leak;
    const int n = a.n;
    const int wave0 = blockIdx.x * PBLOCK + (threadIdx.x & ~63);
    if (wave0 >= n) return;
    const int i = blockIdx.x * PBLOCK + threadIdx.x;
    const bool live = i < n;
    const int il = live ? i : n - 1;

    Env s;
    load_env(a, il, s);
    sincos_lean(s.psi, s.sn, s.cs);
    Current cur = {0.0f, 0.0f, 0.0f, 0.0f, 0u};
    float vc0 = 0.0f, beta0 = 0.0f;
    if (a.cur_vc) {
        cur.vc = a.cur_vc[il]; cur.beta = a.cur_beta[il];
        if (a.current_drift) { vc0 = a.cur_vc0[il]; beta0 = a.cur_beta0[il]; cur.ctr = a.drift_ctr[il]; }
        current_components(cur);
    }
    Vessel ve = launch_vessel_plain(a, il);                      // re-drawn with the episode when the randomisation is on
    uint32_t episode = a.auto_reset ? (uint32_t)a.episode[il] : 0u;
    bool ep_dirty = false, rf_dirty = (MODE == MODE_FULL);
    const PolicyConsts<A> pc = load_policy_consts<A>(pa);
    const bool draw = pa.noise == nullptr && pa.sample != 0;
    uint32_t nctr = draw ? a.noise_ctr[il] : 0u;

    float o[9];
    {
        float sr_, cr_;
        bool same_;
        make_obs(s.N, s.E, s.psi, s.u, s.v, s.r, s.refN, s.refE, s.refPsi, s.pt, a.wrap_mode == WRAP_REFERENCE, o, sr_, cr_, same_);
    }
    if (EXT && pa.use_lag) {                                     // continue the episode with the observation the last launch ended with
        const float4 lg = a.S3[il];
        o[6] = lg.x; o[7] = lg.y; o[8] = lg.z;
    }
    IntegState ig{};
    if constexpr (INTEG) {                                       // the first policy input: the stored I, no update
        ig = integ_load(ia, il);
        integ_apply(ig, o);
    }
    ReffState fs{};
    if constexpr (REFF) {
        fs = reff_load(fa, il, n);
        reff_row(fa, 0, n, i, live, s.refN, s.refE, s.refPsi);  // the reference o_0 was formed against
        s.refN = fs.x[0][0]; s.refE = fs.x[1][0]; s.refPsi = fs.x[2][0];   // the last launch's pending new_ref is in force from step 0
    }
    SplitIn in;
    float vout[8], mu[8];
    obs_to_frags_x<OD>(o, in);
    mlp_eval_x<KA>(nets.Wpi_h, nets.Wpi_l, nets.Bpi, pa.n_hidden, in, leak, mu);
    critic_eval<KA>(nets, pa, in, leak, vout);
    float v_t = vout[0];

    int next_switch = 0;
    for (int t = 0; t < pa.T; ++t) {
        const int64_t row = (int64_t)t * n + i;
        if (live) store_row_direct<OD>(pa.obs_out, row, o, a.obs_bf16 != 0);
        if constexpr (INTEG) integ_row(ia, t, n, i, live, ig);
        float act[A];
        float logp;
        if (pa.noise || draw) {
            float xi[A];
            if (pa.noise) {
#pragma unroll
                for (int k = 0; k < A; ++k) xi[k] = pa.noise[((int64_t)t * n + il) * A + k];
            } else {
                policy_noise<A>(a, a.env_id_base + i, nctr, xi);
                ++nctr;
            }
            logp = sample_action<A>(pc, mu, xi, act);
        } else {
            logp = mean_action<A>(pc, mu, act);
        }
        if (live) store_row_direct<A>(pa.act_out, row, act, false);

        bool has_ref = false;
        float nrN = 0.0f, nrE = 0.0f, nrP = 0.0f;
        if (next_switch < pa.n_switch && pa.switch_step[next_switch] == t) {
            const float* rp = pa.refs + (int64_t)next_switch * 3 * n;
            nrN = rp[il]; nrE = rp[(int64_t)n + il]; nrP = rp[2 * (int64_t)n + il];
            has_ref = true; rf_dirty = true;
            ++next_switch;
        }
        if constexpr (REFF) {                                    // a switch sets the filter's target; its position is the step's new_ref
            if (has_ref) reff_target(fs, nrN, nrE, nrP);
            reff_advance(fa, fs);
            nrN = fs.x[0][0]; nrE = fs.x[1][0]; nrP = fs.x[2][0];
            has_ref = t + 1 < pa.T; rf_dirty = true;             // the last step's stays pending in the filter: the state keeps the
                                                                 // reference its last observation was formed against
            // o_t+1 is formed before new_ref applies (Q4): against the reference in force now (a reset below overwrites the row)
            if (t + 1 < pa.T) reff_row(fa, t + 1, n, i, live, s.refN, s.refE, s.refPsi);
        }
        StepOut out;
        env_step<MODE, EXT>(a, ve, s, act, has_ref, nrN, nrE, nrP, a.cur_vc != nullptr, cur.vcN, cur.vcE, out, il);
        if (a.current_drift) current_drift_step(a, cur, vc0, beta0, a.env_id_base + i);
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = out.o[k];
        if constexpr (INTEG) {                                   // the step's update; a cut episode's pre-reset input carries it too
            integ_update(ia, ig, o);
            integ_apply(ig, o);
        }
        // ppo.py:305-322 with reset_at_end: after the LAST step of the block every env is cut and re-drawn, ended or not
        const bool do_reset = ((a.auto_reset && out.d != 0u) || (pa.reset_at_end && t == pa.T - 1)) && live;
        float v_pre = 0.0f;
        if (__ballot(do_reset) != 0ull) {                       // wave-uniform
            // the critic once more, on the pre-reset observation - only if an env of the wave was CUT (time limit): a terminated
            // env bootstraps with 0 (ppo.py:311), and with termination on most finished envs are terminated ones
            if (__ballot(do_reset && (out.d & DONE_TERMINAL) == 0u) != 0ull) {
                obs_to_frags_x<OD>(o, in);
                critic_eval<KA>(nets, pa, in, leak, vout);
                v_pre = vout[0];
            }
            if (do_reset) {
                if constexpr (REFF) {                             // the last step's pending new_ref: a re-drawn env keeps it as its reference
                    if (t == pa.T - 1) { s.refN = fs.x[0][0]; s.refE = fs.x[1][0]; s.refPsi = fs.x[2][0]; }
                }
                env_auto_reset<MODE>(a, s, a.env_id_base + i, episode, o);
                if (a.rand_tab) redraw_vessel_cold(a, i, episode, ve);    // domain randomisation: the new episode runs on a new hull
                if (a.cur_nom) current_redraw(a, i, episode, cur, vc0, beta0);    // ... in a new current (stored with the final state)
                ++episode; ep_dirty = true; rf_dirty = true;
                if constexpr (INTEG) integ_clear(ig);             // the new episode starts with I = 0
                if constexpr (REFF) {                             // ... and the filter at rest on its reference
                    reff_rest(fs, s.refN, s.refE, s.refPsi);
                    if (t + 1 < pa.T) reff_row(fa, t + 1, n, i, live, s.refN, s.refE, s.refPsi);
                }
            }
        }
        obs_to_frags_x<OD>(o, in);
        mlp_eval_x<KA>(nets.Wpi_h, nets.Wpi_l, nets.Bpi, pa.n_hidden, in, leak, mu);
        critic_eval<KA>(nets, pa, in, leak, vout);
        const float v_next = do_reset ? v_pre : vout[0];
        const float v_new = vout[0];
        const bool terminal = (out.d & DONE_TERMINAL) != 0u;
        const bool ended = (out.d != 0u) || (t == pa.T - 1);
        const float boot = (ended && !terminal) ? v_next : 0.0f;          // ppo.py:311
        if (live) {
            pa.rew[row] = out.reward;
            pa.done[row] = (uint8_t)out.d;
            pa.val[row] = v_t;
            pa.logp[row] = logp;
            pa.boot[row] = boot;
        }
        v_t = v_new;
    }
    if (live) {
        store_row_direct<OD>(pa.last_obs, i, o, a.obs_bf16 != 0);
        pa.last_val[i] = v_t;
        store_env(a, i, s, rf_dirty);
        if (EXT) a.S3[i] = make_float4(o[6], o[7], o[8], 0.0f);
        if (ep_dirty) a.episode[i] = (int)episode;
        if (a.current_drift) { a.cur_vc[i] = cur.vc; a.cur_beta[i] = cur.beta; a.drift_ctr[i] = cur.ctr; }
        if (a.cur_nom && ep_dirty) store_current(a, i, cur, vc0, beta0, true);
        if (draw) a.noise_ctr[i] = nctr;
        if constexpr (INTEG) integ_store(ia, i, ig);
        if constexpr (REFF) reff_store(fa, i, n, fs);
    }
