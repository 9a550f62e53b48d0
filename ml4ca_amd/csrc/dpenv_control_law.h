// dpenv_control_law.h - the baseline DP controller's law (include/dpenv.h states it operation by operation): the numbers of one env, the
// packed per-env table's index and load, the allocation and one control step.  The ONE text of the law on the device: included inside
// namespace dpenv by dpenv_control.hip and dpenv_control_nn.hip (the closed-loop kernels) and by dpenv_label.hip and dpenv_label_nn.hip
// (the labelling scans), after dpenv_dev.h.  Everything here is plain f32 in the stated order: the build has -ffp-contract=off, `/` and sqrtf are the compiler's
// correctly rounded forms.
#ifndef DPENV_CONTROL_LAW_H
#define DPENV_CONTROL_LAW_H

// The law's numbers of ONE env, in registers: what controller_rollout_tab_kernel flies instead of ControlArgs' shared set while a
// per-env table is in force (dpenv_set_dp_controller_table).  Same member names, so dp_control / dp_allocate read either.
struct ControlLane {
    float kp[3], kd[3], ki[3], zb[3], tmax[3];
    float G[5][3];
    float kf[3], kr_bow;
    float f_eps;
    float dt;                                                    // the handle's (wave-uniform)
};

// The packed per-env block pack_controllers_kernel writes: per wave of 64 envs CTRL_TAB_STREAMS float4 streams of 64 lanes, stream k of
// env i at ctrl_tab_index(i, k) - a wave's load is 1 KiB contiguous, and the nine addresses of a lane differ by constants (with
// [k][n] streams the nine wave-uniform bases cost the randomised-hull form with the filter 36 B of scratch).  ctrl_tab_float4s(n) is
// the block's size.  Flat slot q = 4 k + component:
// kp 0-2 | kd 3-5 | ki 6-8 | zb 9-11 | tmax 12-14 | G row-major 15-29 | kf 30-32 | kr_bow 33 | f_eps 34 | 35 pad
__host__ __device__ __forceinline__ int64_t ctrl_tab_index(int i, int k) { return ((int64_t)(i >> 6) * CTRL_TAB_STREAMS + k) * 64 + (i & 63); }

__device__ __forceinline__ void load_control_lane(const float4* __restrict__ tab, int il, float dt, ControlLane& c)
{
    float q[4 * CTRL_TAB_STREAMS];
#pragma unroll
    for (int k = 0; k < CTRL_TAB_STREAMS; ++k) {
        const float4 v = tab[ctrl_tab_index(il, k)];
        q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c.kp[j] = q[j]; c.kd[j] = q[3 + j]; c.ki[j] = q[6 + j]; c.zb[j] = q[9 + j]; c.tmax[j] = q[12 + j]; c.kf[j] = q[30 + j];
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.G[m][j] = q[15 + 3 * m + j];
    c.kr_bow = q[33];
    c.f_eps = q[34];
    c.dt = dt;
}

// tau[3] -> the final variant's continuous-angle action [n_bow, n_port, n_star, sin_port, cos_port, sin_star, cos_star] / 100 %
// (C: ControlArgs, the shared numbers as kernel arguments, or ControlLane)
template <class C>
__device__ __forceinline__ void dp_allocate(const C& c, const float tau[3], float act[7])
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

// the PID lines of one control step on the observation o (e = o[0:3], nu = o[3:6]): the integral first, then the clipped wrench
template <class C>
__device__ __forceinline__ void dp_wrench(const C& c, const float o[9], float z[3], float tau[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        z[j] = fminf(fmaxf(z[j] + c.dt * o[j], -c.zb[j]), c.zb[j]);
        const float t = -((c.kp[j] * o[j] + c.kd[j] * o[3 + j]) + c.ki[j] * z[j]);
        tau[j] = fminf(fmaxf(t, -c.tmax[j]), c.tmax[j]);
    }
}

// one control step of the law: the integral, the wrench, then the pseudo-inverse allocation
template <class C>
__device__ __forceinline__ void dp_control(const C& c, const float o[9], float z[3], float act[7])
{
    float tau[3];
    dp_wrench(c, o, z, tau);
    dp_allocate(c, tau, act);
}

#endif
