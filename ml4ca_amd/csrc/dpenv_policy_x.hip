// dpenv_policy_x.hip - the PPO actor-critic inside the rollout launch in split-f16 ("fp32-faithful") arithmetic:
// DPENV_POLICY_F32.  Reference: mlp_gaussian_policy / mlp_actor_critic, spinup/algos/tf1/ppo/core.py:29-33,80-107 (fp32 TF1
// dense layers), gaussian_likelihood core.py:42-46, rollout loop ppo.py:289-322.  This is the mode parity with the reference's
// fp32 networks is claimed on (mu, v and logp within 1e-5 of an fp32 evaluation; tests/test_gpu_policy.py); dpenv_policy.hip
// holds the f16 fast mode.  See dpenv_policy_dev.h (mlp_eval_x) for the arithmetic.
//
// Launch form: one wave per 64 envs, 256-thread workgroups.  The LDS image of both networks is twice the f16 one (high and
// low fragments: 152 KiB for the shipped 9-80-80-80 shape), which leaves no room for the two-wave form's mailboxes nor for row
// staging: observation / action / noise rows are accessed per lane (36 / 28-byte rows; slower stores, same bytes).
#include "dpenv_policy_dev.h"

namespace dpenv {

struct SplitNets {
    const uint4 *Wpi_h, *Wv_h, *Wpi_l, *Wv_l;
    const float *Bpi, *Bv;
};

__device__ __forceinline__ SplitNets split_nets(const uint4* lds_w, const PolicyArgs& pa)
{
    SplitNets s;
    s.Wpi_h = lds_w;
    s.Wv_h = lds_w + pa.nent;
    s.Wpi_l = lds_w + 2 * pa.nent;
    s.Wv_l = lds_w + 3 * pa.nent;
    s.Bpi = (const float*)(lds_w + 4 * pa.nent);
    s.Bv = s.Bpi + pa.nblk * 32;
    return s;
}

// the critic in the arithmetic the descriptor asked for: split-f16 like the actor (DPENV_POLICY_F32), or plain f16 on the HIGH
// image and the high parts of the input - exactly the F16 mode's critic, bit for bit (DPENV_POLICY_F32_ACTOR)
template <int KA>
__device__ __forceinline__ void critic_eval(const SplitNets& nets, const PolicyArgs& pa, const SplitIn& in, float leak, float out[8])
{
    if (pa.critic_f16) mlp_eval<KA>(nets.Wv_h, nets.Bv, pa.n_hidden, in.h0, in.h1, (_Float16)leak, out);
    else mlp_eval_x<KA>(nets.Wv_h, nets.Wv_l, nets.Bv, pa.n_hidden, in, leak, out);
}

template <int OD, int A, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_forward_x_kernel(const PolicyArgs pa, const float* obs, float* mu_out, float* v_out, int n)
{
    extern __shared__ uint4 lds_dyn[];
    stage_weights(lds_dyn, pa);
    const SplitNets nets = split_nets(lds_dyn, pa);
    const int i = blockIdx.x * PBLOCK + threadIdx.x;
    if ((int)(blockIdx.x * PBLOCK + (threadIdx.x & ~63)) >= n) return;          // whole wave out of range (uniform)
    const bool live = i < n;
    const int il = live ? i : n - 1;
    float o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < OD; ++k) o[k] = obs[(int64_t)il * OD + k];
    SplitIn in;
    obs_to_frags_x<OD>(o, in);
    float mu[8], vv[8];
    mlp_eval_x<KA>(nets.Wpi_h, nets.Wpi_l, nets.Bpi, pa.n_hidden, in, pa.leak, mu);
    critic_eval<KA>(nets, pa, in, pa.leak, vv);
    if (live) {
        store_row_direct<A>(mu_out, i, mu, false);
        v_out[i] = vv[0];
    }
}

// the rollout loop of policy_rollout_kernel (dpenv_policy.hip) with the exact network evaluation; rows, bootstrap values and
// auto-reset handling are identical
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_x_kernel(const StepArgs a, const PolicyArgs pa)
{
    constexpr bool INTEG = false;
    const IntegArgs ia{};
#include "dpenv_policy_rollout_x_body.inc"
}

// INTEG: the deployed node's integral action (IntegArgs, dpenv_set_integral_action)
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_x_integ_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia)
{
    constexpr bool INTEG = true;
#include "dpenv_policy_rollout_x_body.inc"
}

}  // namespace dpenv

using namespace dpenv;

static size_t lds_bytes_x(const PolicyArgs& pa) { return (size_t)4 * pa.nent * 16 + (size_t)2 * pa.nblk * 32 * 4; }

extern "C" hipError_t dpenv_dev_launch_policy_forward_x(const PolicyArgs* pa, int od, int adim, const float* obs, float* mu, float* v,
                                                        int n, hipStream_t s)
{
    const dim3 grid((n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    const size_t lds = lds_bytes_x(*pa);
#define FWD_K(OD_, A_, KS_)                                                                                              \
    do {                                                                                                                 \
        hipError_t e = hipFuncSetAttribute((const void*)policy_forward_x_kernel<OD_, A_, KS_>,                            \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
        if (e != hipSuccess) return e;                                                                                   \
        hipLaunchKernelGGL((policy_forward_x_kernel<OD_, A_, KS_>), grid, block, lds, s, *pa, obs, mu, v, n);             \
        return hipGetLastError();                                                                                        \
    } while (0)
#define FWD(OD_, A_)                                                                                                     \
    do {                                                                                                                 \
        if (ka == 5) FWD_K(OD_, A_, 5);                                                                                  \
        if (ka == 6) FWD_K(OD_, A_, 6);                                                                                  \
        if (ka == 21) FWD_K(OD_, A_, 21);                                                                                \
        FWD_K(OD_, A_, 22);                                                                                              \
    } while (0)
    if ((pa->ks != 5 && pa->ks != 6) || (pa->act != 0 && pa->act != 1) || !pa->split) return hipErrorInvalidValue;
    const int ka = pa->ks + 16 * pa->act;
#ifdef DPENV_DEV_FAST
    if (od == 9 && adim == 7 && ka == 5) FWD_K(9, 7, 5);
#else
    if (od == 9 && adim == 7) FWD(9, 7);
    if (od == 9 && adim == 5) FWD(9, 5);
    if (od == 9 && adim == 6) FWD(9, 6);
    if (od == 6 && adim == 7) FWD(6, 7);
    if (od == 6 && adim == 5) FWD(6, 5);
    if (od == 6 && adim == 6) FWD(6, 6);
    if (od == 6 && adim == 3) FWD(6, 3);
#endif
#undef FWD_K
#undef FWD
    return hipErrorInvalidValue;
}

template <int MODE, bool EXT, int KA>
static hipError_t launch_x_one(const StepArgs& a, const PolicyArgs& pa, hipStream_t s)
{
    const dim3 grid((a.n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    const size_t lds = lds_bytes_x(pa);
    hipError_t e = hipFuncSetAttribute((const void*)policy_rollout_x_kernel<MODE, EXT, KA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((policy_rollout_x_kernel<MODE, EXT, KA>), grid, block, lds, s, a, pa);
    return hipGetLastError();
}

template <int MODE>
static hipError_t launch_x_mode(const StepArgs& a, const PolicyArgs& pa, bool ext, hipStream_t s)
{
    if ((pa.ks != 5 && pa.ks != 6) || (pa.act != 0 && pa.act != 1) || !pa.split) return hipErrorInvalidValue;
#ifdef DPENV_DEV_FAST
    if (pa.ks != 5 || pa.act != 0 || !ext) return hipErrorInvalidValue;
    return launch_x_one<MODE, true, 5>(a, pa, s);
#else
    switch (pa.ks + 16 * pa.act) {
    case 5: return ext ? launch_x_one<MODE, true, 5>(a, pa, s) : launch_x_one<MODE, false, 5>(a, pa, s);
    case 6: return ext ? launch_x_one<MODE, true, 6>(a, pa, s) : launch_x_one<MODE, false, 6>(a, pa, s);
    case 21: return ext ? launch_x_one<MODE, true, 21>(a, pa, s) : launch_x_one<MODE, false, 21>(a, pa, s);
    default: return ext ? launch_x_one<MODE, true, 22>(a, pa, s) : launch_x_one<MODE, false, 22>(a, pa, s);
    }
#endif
}

extern "C" hipError_t dpenv_dev_launch_policy_rollout_x(const StepArgs* a, const PolicyArgs* pa, int mode, int ext, hipStream_t s)
{
    if (pa->ws) return pa->critic_f16 ? dpenv_dev_launch_policy_rollout_xws_f32_actor(a, pa, mode, ext, s)
                                      : dpenv_dev_launch_policy_rollout_xws_f32(a, pa, mode, ext, s);
#ifdef DPENV_DEV_FAST
    return mode == MODE_FINAL_CONT ? launch_x_mode<MODE_FINAL_CONT>(*a, *pa, ext, s) : hipErrorInvalidValue;
#else
    switch (mode) {
    case MODE_FULL: return launch_x_mode<MODE_FULL>(*a, *pa, ext, s);
    case MODE_SIMPLE: return launch_x_mode<MODE_SIMPLE>(*a, *pa, ext, s);
    case MODE_LIMITED: return launch_x_mode<MODE_LIMITED>(*a, *pa, ext, s);
    case MODE_FINAL_WRAP: return launch_x_mode<MODE_FINAL_WRAP>(*a, *pa, ext, s);
    case MODE_FINAL_CONT: return launch_x_mode<MODE_FINAL_CONT>(*a, *pa, ext, s);
    }
    return hipErrorInvalidValue;
#endif
}

// the closed loop with the integral action in the split arithmetics (dpenv_policy.hip: dpenv_dev_launch_policy_rollout_integ has the supported set)
template <int MODE>
static hipError_t launch_x_integ_one(const StepArgs& a, const PolicyArgs& pa, const IntegArgs& ia, hipStream_t s)
{
    const dim3 grid((a.n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    const size_t lds = lds_bytes_x(pa);
    hipError_t e = hipFuncSetAttribute((const void*)policy_rollout_x_integ_kernel<MODE, true, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((policy_rollout_x_integ_kernel<MODE, true, 5>), grid, block, lds, s, a, pa, ia);
    return hipGetLastError();
}

extern "C" hipError_t dpenv_dev_launch_policy_rollout_x_integ(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, int mode, int ext,
                                                              hipStream_t s)
{
    if (!ext || pa->ks != 5 || pa->act != 0 || !pa->split) return hipErrorInvalidValue;
    if (pa->ws) return pa->critic_f16 ? dpenv_dev_launch_policy_rollout_xws_f32_actor_integ(a, pa, ia, mode, ext, s)
                                      : dpenv_dev_launch_policy_rollout_xws_f32_integ(a, pa, ia, mode, ext, s);
    switch (mode) {
    case MODE_FINAL_CONT: return launch_x_integ_one<MODE_FINAL_CONT>(*a, *pa, *ia, s);
#ifndef DPENV_DEV_FAST
    case MODE_LIMITED: return launch_x_integ_one<MODE_LIMITED>(*a, *pa, *ia, s);
    case MODE_FULL: return launch_x_integ_one<MODE_FULL>(*a, *pa, *ia, s);
#endif
    }
    return hipErrorInvalidValue;
}
