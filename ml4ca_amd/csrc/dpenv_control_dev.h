// dpenv_control_dev.h - the classical baseline in the closed loop (dpenv_set_dp_controller / dpenv_controller_rollout in dpenv.h): a PID
// motion controller feeding a weighted pseudo-inverse thrust allocation, evaluated in registers inside a T-step launch.  Included by
// dpenv_policy.hip inside namespace dpenv (after dpenv_policy_dev.h: the env's device functions, the reference filter's, the wave-private
// row staging); that unit owns the kernels and their launchers.
//
// The law is build-defined (the reference has no PID and no pseudo-inverse node in its tree) and stated operation by operation in
// include/dpenv.h; deploy.BatchedDPController is its host statement.  Everything here is plain f32 in that order: the build has
// -ffp-contract=off, `/` and sqrtf are the compiler's correctly rounded forms.
#ifndef DPENV_CONTROL_DEV_H
#define DPENV_CONTROL_DEV_H

// tau[3] -> the final variant's continuous-angle action [n_bow, n_port, n_star, sin_port, cos_port, sin_star, cos_star] / 100 %
__device__ __forceinline__ void dp_allocate(const ControlArgs& c, const float tau[3], float act[7])
{
    float f[5];                                                  // Fy_bow, Fx_port, Fy_port, Fx_star, Fy_star
#pragma unroll
    for (int m = 0; m < 5; ++m) f[m] = (c.G[m][0] * tau[0] + c.G[m][1] * tau[1]) + c.G[m][2] * tau[2];
    const float Kb = f[0] >= 0.0f ? c.kf[0] : c.kr_bow;
    const float nb = copysignf(sqrtf(fabsf(f[0]) / Kb), f[0]);
    act[0] = fminf(fmaxf(nb / 100.0f, -1.0f), 1.0f);
#pragma unroll
    for (int k = 0; k < 2; ++k) {                                // stern pods: thrust >= 0, free azimuth
        const float Fx = f[1 + 2 * k], Fy = f[2 + 2 * k];
        const float F = sqrtf(Fx * Fx + Fy * Fy);
        const float ns = sqrtf(F / c.kf[1 + k]);
        act[1 + k] = fminf(ns / 100.0f, 1.0f);
        const bool dir = F > c.f_eps;
        act[3 + 2 * k] = dir ? Fy / F : 0.0f;
        act[4 + 2 * k] = dir ? Fx / F : 1.0f;
    }
}

// one control step of the law on the observation o (e = o[0:3], nu = o[3:6]): the integral first, then the wrench, then the allocation
__device__ __forceinline__ void dp_control(const ControlArgs& c, const float o[9], float z[3], float act[7])
{
    float tau[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        z[j] = fminf(fmaxf(z[j] + c.dt * o[j], -c.zb[j]), c.zb[j]);
        const float t = -((c.kp[j] * o[j] + c.kd[j] * o[3 + j]) + c.ki[j] * z[j]);
        tau[j] = fminf(fmaxf(t, -c.tmax[j]), c.tmax[j]);
    }
    dp_allocate(c, tau, act);
}

// A wave's 64 rows of W floats to a [.][n][W] block: staged through the wave-private LDS area, stored coalesced - wave_store_rows /
// store_rows (dpenv_policy_dev.h, dpenv_env_dev.h) restated.  A copy on purpose: instantiating those two templates for W = 9 and 7 a second
// time in this translation unit changed the instruction schedule of the policy closed-loop kernels that instantiate them too (the
// final variant with the extended state: 8 kernels, 2 to 36 instructions each), and every existing kernel has to stay what it was.
template <int W>
__device__ __forceinline__ void control_store_rows(float* lds, void* dst, int64_t base, int64_t rem, const float* v, int lane, bool bf16)
{
    lds_order<64>();
#pragma unroll
    for (int k = 0; k < W; ++k) lds[lane * W + k] = v[k];
    lds_order<64>();
    const bool full = rem >= (int64_t)64 * W;                    // uniform; the last wave's dead lanes hold no row
    if (bf16) {
        uint16_t* p = (uint16_t*)dst + base;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (full || j * 64 + lane < rem) p[(unsigned)(j * 64 + lane)] = f2bf(lds[j * 64 + lane]);
    } else {
        float* p = (float*)dst + base;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (full || j * 64 + lane < rem) p[(unsigned)(j * 64 + lane)] = lds[j * 64 + lane];
    }
}

// =============================================================================================
//  closed loop with the baseline controller: rollout_kernel's state-in-registers T-step loop (dpenv_kernels.hip) with the action
//  computed from the previous observation instead of fetched - per env-step a 36-byte observation row, a 28-byte action row, reward
//  and done go out and nothing comes in.  One wave per workgroup, the final variant with continuous angles and the extended state.
//  Row conventions of the policy's closed loop (dpenv_policy_rollout_body.inc): obs[t] is the controller's input of step t, the first
//  one rebuilt from the state with the thrust columns of S3; REFF carries the setpoint reference filter with the same calls in the
//  same places, the last step's new_ref pending.
// =============================================================================================
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa)
{
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
        dp_control(ca, o, z, act);
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
        if (ep_dirty) a.episode[i] = (int)episode;
        if (a.current_drift) { a.cur_vc[i] = cur.vc; a.cur_beta[i] = cur.beta; a.drift_ctr[i] = cur.ctr; }
        if (CURR && cur_dirty) store_current(a, i, cur, vc0, beta0, true);
        if constexpr (REFF) reff_store(fa, i, n, fs);
    }
}

// the controller's state z, float4 [n] <-> float [3][n]: op 0 reads it out (dpenv_get_dp_controller_state), 1 writes it
// (dpenv_set_dp_controller_state), 2 zeroes it for the envs of mask (NULL = every env: turning the controller on, dpenv_reset)
__global__ __launch_bounds__(256) void control_state_kernel(float4* z, float* ext, const uint8_t* mask, int n, int op)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (op == 0) {
        const float4 q = z[i];
        ext[i] = q.x; ext[(int64_t)n + i] = q.y; ext[2 * (int64_t)n + i] = q.z;
    } else if (op == 1) {
        z[i] = make_float4(ext[i], ext[(int64_t)n + i], ext[2 * (int64_t)n + i], 0.0f);
    } else if (mask == nullptr || mask[i] != 0) {
        z[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// the stateless allocation (dpenv_thrust_alloc): tau [3][n] -> action [n][7], the closed loop's device function
__global__ __launch_bounds__(256) void alloc_kernel(const ControlArgs ca, const float* tau, float* action, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float t[3] = {tau[i], tau[(int64_t)n + i], tau[2 * (int64_t)n + i]};
    float act[7];
    dp_allocate(ca, t, act);
    store_row_direct<7>(action, i, act, false);
}

#endif
