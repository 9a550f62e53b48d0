// dpenv_policy_rollout_body.inc - the body of the one-wave closed loop, included into policy_rollout_kernel, policy_rollout_integ_kernel
// and policy_rollout_reff_kernel (dpenv_policy.hip: f16, SPLIT = false) and their policy_rollout_x* twins (dpenv_policy_x.hip: split-f16,
// SPLIT = true).  In scope: a (StepArgs), pa (PolicyArgs), ia (IntegArgs), fa (FilterArgs) and the compile-time INTEG, REFF and SPLIT.
// The body is spliced into each __global__ function rather than called as a device function: inlined through a device function the
// INTEG = false kernel came out as another instruction stream than the kernel had before the integral action existed.  Lambdas for the
// arithmetic-dependent parts changed every kernel's instruction stream too, so those are `if constexpr (SPLIT)` blocks: the network
// evaluation, and the rows - staged through the wave's LDS area in f16; per lane in split, whose network image leaves no room for that.
// Even dead address arithmetic changed it: neither form computes the other's lds_io, row-block strides or row.
    constexpr int A = ModeTraits<MODE>::A;
    constexpr int OD = EXT ? 9 : 6;
    extern __shared__ uint4 lds_dyn[];
    uint4* lds_w = lds_dyn;
    float* lds_io = SPLIT ? nullptr : (float*)lds_dyn + policy_lds_io_offset_floats(pa) + (threadIdx.x >> 6) * (64 * 9);
    stage_weights(lds_w, pa);
    const uint4 *Wpi = lds_w, *Wv = lds_w + pa.nent;            // the f16 image: Wpi, Wv, then the biases
    const float *Bpi = (const float*)(lds_dyn + 2 * pa.nent), *Bv = Bpi + pa.nblk * 32;
    const SplitNets nets = split_nets(lds_dyn, pa);              // the split image
    const float leak = pa.leak;

    const int lane = threadIdx.x & 63;
    const int n = a.n;
    const int wave0 = blockIdx.x * PBLOCK + (threadIdx.x & ~63);
    if (wave0 >= n) return;                                      // whole wave out of range (uniform)
    const int i = SPLIT ? (int)(blockIdx.x * PBLOCK + threadIdx.x) : wave0 + lane;
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
    // single class: SGPR-resident (the VGPRs are needed by the MLP); classes: per lane from the table, once per launch
    Vessel ve = launch_vessel_plain(a, il);                      // re-drawn with the episode when the randomisation is on
    uint32_t episode = a.auto_reset ? (uint32_t)a.episode[il] : 0u;
    bool ep_dirty = false, rf_dirty = (MODE == MODE_FULL);
    const PolicyConsts<A> pc = load_policy_consts<A>(pa);
    const bool draw = pa.noise == nullptr && pa.sample != 0;
    uint32_t nctr = draw ? a.noise_ctr[il] : 0u;

    const int64_t stride_a = SPLIT ? 0 : (int64_t)n * A, stride_o = SPLIT ? 0 : (int64_t)n * OD;
    const int64_t w_a = SPLIT ? 0 : (int64_t)wave0 * A, w_o = SPLIT ? 0 : (int64_t)wave0 * OD;     // f16: the wave's slice of a [T][n][.] block
    const int64_t rem_a = stride_a - w_a, rem_o = stride_o - w_o;

    // observation of the current state = policy input of step 0 (ENV:196-205), and its value
    float o[9];
    {
        float sr_, cr_;
        bool same_;
        make_obs(s.N, s.E, s.psi, s.u, s.v, s.r, s.refN, s.refE, s.refPsi, s.pt, a.wrap_mode == WRAP_REFERENCE, o, sr_, cr_,
                 same_);
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
    half8 in0, in1;                                              // f16 network input
    SplitIn in;                                                  // split network input
    float vout[8], mu[8];
    if constexpr (SPLIT) {                                       // actor and critic of o_0
        obs_to_frags_x<OD>(o, in);
        mlp_eval_x<KA>(nets.Wpi_h, nets.Wpi_l, nets.Bpi, pa.n_hidden, in, leak, mu);
        critic_eval<KA>(nets, pa, in, leak, vout);
    } else {
        obs_to_frags<OD>(o, in0, in1);
        mlp_eval2<KA>(Wpi, Wv, Bpi, Bv, pa.n_hidden, in0, in1, (_Float16)leak, mu, vout);
    }
    float v_t = vout[0];

    float pre[A];                                                // f16: the given noise row of the next step
    if (!SPLIT && pa.noise) load_rows<A, 64>(pa.noise + w_a, rem_a, lane, pre);
    int next_switch = 0;
    for (int t = 0; t < pa.T; ++t) {
        const int64_t row = SPLIT ? (int64_t)t * n + i : 0;      // split: this lane's row of a [T][n][.] block
        // ---- store the policy input row; the actor's mean for it is already there (joint evaluation) -------------
        if constexpr (SPLIT) { if (live) store_row_direct<OD>(pa.obs_out, row, o, a.obs_bf16 != 0); }
        else wave_store_rows<OD>(lds_io, pa.obs_out, (int64_t)t * stride_o + w_o, rem_o, o, lane, a.obs_bf16 != 0);
        if constexpr (INTEG) integ_row(ia, t, n, i, live, ig);
        // ---- sample: a = mu + std * xi (core.py:85), log-likelihood (core.py:42-46) -----------
        float act[A], logp;
        if constexpr (SPLIT) {                                   // split: the given noise row per lane
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
        } else if (pa.noise) {                                   // f16: the given noise row through the staging, the next one fetched
            float xi[A];
            wave_rows_from_regs<A>(lds_io, pre, xi, lane);
            if (t + 1 < pa.T) load_rows<A, 64>(pa.noise + (int64_t)(t + 1) * stride_a + w_a, rem_a, lane, pre);
            logp = sample_action<A>(pc, mu, xi, act);
        } else if (draw) {
            float xi[A];
            policy_noise<A>(a, a.env_id_base + i, nctr, xi);
            ++nctr;
            logp = sample_action<A>(pc, mu, xi, act);
        } else {
            logp = mean_action<A>(pc, mu, act);
        }
        if constexpr (SPLIT) { if (live) store_row_direct<A>(pa.act_out, row, act, false); }
        else wave_store_rows<A>(lds_io, pa.act_out, (int64_t)t * stride_a + w_a, rem_a, act, lane);

        // ---- env.step ------------------------------------------------------------------------
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
        // ---- value of the observation this step produced, and the next policy input ------------------------------
        // No env of the wave finished (the common case): the next policy input IS that observation, so one joint
        // evaluation gives V(o') for the bootstrap and the actor's mean for the next step.  Otherwise the critic is
        // run once more on the pre-reset observation of the wave before the finished envs are re-drawn.
        float v_pre = 0.0f;
        if (__ballot(do_reset) != 0ull) {                       // wave-uniform
            // only if an env of the wave was CUT (time limit): a terminated one bootstraps with 0 (ppo.py:311), as most do with termination on
            if (__ballot(do_reset && (out.d & DONE_TERMINAL) == 0u) != 0ull) {
                if constexpr (SPLIT) {
                    obs_to_frags_x<OD>(o, in);
                    critic_eval<KA>(nets, pa, in, leak, vout);
                } else {
                    obs_to_frags<OD>(o, in0, in1);
                    mlp_eval<KA>(Wv, Bv, pa.n_hidden, in0, in1, (_Float16)leak, vout);
                }
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
        if constexpr (SPLIT) {
            obs_to_frags_x<OD>(o, in);
            mlp_eval_x<KA>(nets.Wpi_h, nets.Wpi_l, nets.Bpi, pa.n_hidden, in, leak, mu);
            critic_eval<KA>(nets, pa, in, leak, vout);
        } else {
            obs_to_frags<OD>(o, in0, in1);
            mlp_eval2<KA>(Wpi, Wv, Bpi, Bv, pa.n_hidden, in0, in1, (_Float16)leak, mu, vout);
        }
        const float v_next = do_reset ? v_pre : vout[0];
        const float v_new = vout[0];
        // bootstrap value at a path end (ppo.py:311): 0 if the env terminated, V(o) if only the time limit or the
        // end of this launch cut the path
        const bool terminal = (out.d & DONE_TERMINAL) != 0u;
        const bool ended = (out.d != 0u) || (t == pa.T - 1);
        const float boot = (ended && !terminal) ? v_next : 0.0f;

        if (live) {
            if constexpr (SPLIT) {
                pa.rew[row] = out.reward;
                pa.done[row] = (uint8_t)out.d;
                pa.val[row] = v_t;
                pa.logp[row] = logp;
                pa.boot[row] = boot;
            } else {
                (pa.rew + (int64_t)t * n)[(unsigned)i] = out.reward;
                (pa.done + (int64_t)t * n)[(unsigned)i] = (uint8_t)out.d;
                (pa.val + (int64_t)t * n)[(unsigned)i] = v_t;
                (pa.logp + (int64_t)t * n)[(unsigned)i] = logp;
                (pa.boot + (int64_t)t * n)[(unsigned)i] = boot;
            }
        }
        v_t = v_new;
    }
    // observation after the last step (policy input of the next launch) and final state
    if constexpr (!SPLIT) wave_store_rows<OD>(lds_io, pa.last_obs, w_o, rem_o, o, lane, a.obs_bf16 != 0);    // the whole wave
    if (live) {
        if constexpr (SPLIT) store_row_direct<OD>(pa.last_obs, i, o, a.obs_bf16 != 0);
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
