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

// the law itself - ControlLane, ctrl_tab_index, load_control_lane, dp_allocate, dp_control - shared with the labelling scan (dpenv_label.hip)
#include "dpenv_control_law.h"
// the QP allocation, the other allocation stage the closed loop's body can be compiled with (controller_rollout_qp_kernel, dpenv_qp.hip)
#include "dpenv_qp_law.h"

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
    constexpr bool TAB = false, QP = false;
    const float4* const tab = nullptr;
    const QpRollout qr = {};
#include "dpenv_control_rollout_body.inc"
}

// TAB: every env flies its own row of the packed controller block (dpenv_set_dp_controller_table) - nine 16-byte loads per env and launch
// behind the state loads, the numbers held in VGPRs for the launch, read only.  The law, the rows and everything else are the kernel above.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_tab_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                         const float4* __restrict__ tab)
{
    constexpr bool TAB = true, QP = false;
    const QpRollout qr = {};
#include "dpenv_control_rollout_body.inc"
}

// The public controller table float[DPENV_CTRL_NPARAM][n] -> the packed block, one lane per env (dpenv_set_dp_controller_table).  G is
// dpenv_dp_allocation_matrix's recipe in its operation order (dpenv_api_free.hip), in f64, rounded once.  A row that breaks a condition of
// include/dpenv.h is packed as the zero controller and marked in refused (uint8 [n], or NULL).
__global__ __launch_bounds__(256) void pack_controllers_kernel(const float* __restrict__ pub, float4* __restrict__ tab,
                                                                uint8_t* __restrict__ refused, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float p[CTRL_NPARAM];
#pragma unroll
    for (int k = 0; k < CTRL_NPARAM; ++k) p[k] = pub[(int64_t)k * n + i];
    const float *kp = p + CTRL_KP, *kd = p + CTRL_KD, *ki = p + CTRL_KI, *zb = p + CTRL_ZB, *tmax = p + CTRL_TMAX, *w = p + CTRL_WEIGHT;
    const float *lx = p + CTRL_LX, *ly = p + CTRL_LY, *kf = p + CTRL_KF;
    const float kr_bow = p[CTRL_KR_BOW], f_eps = p[CTRL_F_EPS];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ok = ok && isfinite(kp[j]) && isfinite(kd[j]) && isfinite(ki[j]);
        ok = ok && zb[j] >= 0.0f && tmax[j] >= 0.0f;             // (false for a NaN)
        ok = ok && isfinite(kf[j]) && kf[j] > 0.0f;
        ok = ok && isfinite(lx[j]) && isfinite(ly[j]);
    }
    ok = ok && isfinite(kr_bow) && kr_bow > 0.0f && f_eps >= 0.0f;
#pragma unroll
    for (int m = 0; m < 5; ++m) ok = ok && isfinite(w[m]) && w[m] > 0.0f;

    const double T[3][5] = {{0.0, 1.0, 0.0, 1.0, 0.0},
                            {1.0, 0.0, 1.0, 0.0, 1.0},
                            {(double)lx[0], -(double)ly[1], (double)lx[1], -(double)ly[2], (double)lx[2]}};
    double V[5][3], M[3][3], adj[3][3];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[m][j] = T[j][m] / (double)w[m];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 5; ++m) acc += T[r][m] * V[m][c];
            M[r][c] = acc;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {                            // adj[r][c] = cofactor of M[c][r]
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            adj[r][c] = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1];
        }
    const double det = (M[0][0] * adj[0][0] + M[0][1] * adj[1][0]) + M[0][2] * adj[2][0];
    ok = ok && isfinite(det) && det != 0.0;
    float G[5][3];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc += V[m][j] * adj[j][c];
            G[m][c] = (float)(acc / det);
            ok = ok && isfinite(G[m][c]);
        }

    float q[4 * CTRL_TAB_STREAMS];
#pragma unroll
    for (int k = 0; k < 4 * CTRL_TAB_STREAMS; ++k) q[k] = 0.0f;
    if (ok) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            q[j] = kp[j]; q[3 + j] = kd[j]; q[6 + j] = ki[j]; q[9 + j] = zb[j]; q[12 + j] = tmax[j]; q[30 + j] = kf[j];
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int j = 0; j < 3; ++j) q[15 + 3 * m + j] = G[m][j];
        q[33] = kr_bow;
        q[34] = f_eps;
    } else {                                                     // the zero controller: the action [0, 0, 0, 0, 1, 0, 1] whatever the observation
        q[30] = q[31] = q[32] = q[33] = 1.0f;
    }
#pragma unroll
    for (int k = 0; k < CTRL_TAB_STREAMS; ++k) tab[ctrl_tab_index(i, k)] = make_float4(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]);
    if (refused) refused[i] = ok ? 0 : 1;
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
