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

// the one-wave closed loop of dpenv_policy.hip with the exact network evaluation (dpenv_policy_rollout_body.inc, SPLIT = true)
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_x_kernel(const StepArgs a, const PolicyArgs pa)
{
    constexpr bool INTEG = false, REFF = false, SPLIT = true;
    const IntegArgs ia{};
    const FilterArgs fa{};
#include "dpenv_policy_rollout_body.inc"
}

// INTEG: the deployed node's integral action (IntegArgs, dpenv_set_integral_action)
template <int MODE, bool EXT, int KA>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_x_integ_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia)
{
    constexpr bool INTEG = true, REFF = false, SPLIT = true;
    const FilterArgs fa{};
#include "dpenv_policy_rollout_body.inc"
}

// REFF: the setpoint reference filter (FilterArgs, dpenv_set_reference_filter), with the integral action if INTEG_
template <int MODE, bool EXT, int KA, bool INTEG_>
__global__ __launch_bounds__(PBLOCK) void policy_rollout_x_reff_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia, const FilterArgs fa)
{
    constexpr bool INTEG = INTEG_, REFF = true, SPLIT = true;
#include "dpenv_policy_rollout_body.inc"
}

}  // namespace dpenv

using namespace dpenv;

static size_t lds_bytes_x(const PolicyArgs& pa) { return (size_t)4 * pa.nent * 16 + (size_t)2 * pa.nblk * 32 * 4; }

hipError_t dev::launch_policy_forward_x(const PolicyArgs* pa, int od, int adim, const float* obs, float* mu, float* v, int n, hipStream_t s)
{
    if (!pa->split) return hipErrorInvalidValue;
    const dim3 grid((n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    return with_obs_act(od, adim, [&](auto OD, auto A) { return with_ka(*pa, [&](auto K) {
        return launch_with_lds(policy_forward_x_kernel<OD, A, K>, grid, block, lds_bytes_x(*pa), s, *pa, obs, mu, v, n);
    }); });
}

// the one-wave closed loop in the split arithmetics; with the integral action (ia) the set integ_one_wave admits, with the reference
// filter (fa) the set reff_one_wave admits
hipError_t dev::launch_policy_rollout_x(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                        hipStream_t s)
{
    if (!pa->split) return hipErrorInvalidValue;
    const dim3 grid((a->n + PBLOCK - 1) / PBLOCK), block(PBLOCK);
    const size_t lds = lds_bytes_x(*pa);
    return with_mode_ext_ka(mode, ext, *pa, [&](auto M, auto E, auto K) -> hipError_t {
        if (fa) {
            if constexpr (reff_one_wave(M, E, K)) {
                if (ia) return launch_with_lds(policy_rollout_x_reff_kernel<M, E, K, true>, grid, block, lds, s, *a, *pa, *ia, *fa);
                return launch_with_lds(policy_rollout_x_reff_kernel<M, E, K, false>, grid, block, lds, s, *a, *pa, IntegArgs{}, *fa);
            }
            return hipErrorInvalidValue;
        }
        if (!ia) return launch_with_lds(policy_rollout_x_kernel<M, E, K>, grid, block, lds, s, *a, *pa);
        if constexpr (integ_one_wave(M, E, K)) return launch_with_lds(policy_rollout_x_integ_kernel<M, E, K>, grid, block, lds, s, *a, *pa, *ia);
        return hipErrorInvalidValue;
    });
}
