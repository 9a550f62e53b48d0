// dpenv_policy_ws.h - the closed-loop rollout with the work of every 64 envs split over two waves (an env wave and a network
// wave per SIMD), for all three network arithmetics.  Included by dpenv_policy_ws.hip (PREC_F16) and dpenv_policy_xws*.hip
// (PREC_F32, PREC_F32_ACTOR): one translation unit each, they take minutes to compile.
#ifndef DPENV_POLICY_WS_H
#define DPENV_POLICY_WS_H
#include <type_traits>
#include "dpenv_policy_dev.h"

namespace dpenv {

// =============================================================================================
//  The same rollout with the work of every 64 envs split over TWO waves (wave specialisation).
//
//  At 65 536 envs policy_rollout_kernel puts one wave on each SIMD, and one wave alone issues an instruction every
//  ~2.3 ns however idle the SIMD is (tools/issue_rate.hip).  Here a 512-thread workgroup owns 256 envs with eight waves:
//  E-wave g (0..3) carries the environments of group g, M-wave 4+g their networks, so every SIMD holds an E and an M
//  wave.  The pair hands over through LDS mailboxes and sequence words (no workgroup barrier in the loop).  Per step t:
//      network wave                                          env wave
//      wait o_t; fragments; xi_t -> mailbox                  (rows of step t-1, drift of step t)
//      actor(o_t) -> mu_t, post                              wait mu_t
//      critic(o_t) (+ critic of the pre-reset observation    a_t = mu_t + std xi_t; env.step; reset of finished envs;
//         where step t-1 cut an episode), post V             o_t+1 -> mailbox, post            <- the serial chain ends here
//      draw xi_t+1 (Philox + Box-Muller) while waiting       logp, action / reward / done / observation rows; wait V; val, boot rows
//  The chain actor(o_t) -> env.step(t) -> actor(o_t+1) stays serial; the critic - half of the network work - and the exploration
//  noise run beside the env step, the row bookkeeping beside the actor.  Same mlp_eval chains and same env_step as
//  policy_rollout_kernel: every row is bit-identical.  (ROLES = 2: an env wave and a network wave.  Two three-wave forms - a critic wave
//  of its own; the network wave split by env tile - were built and measured in round 2, were slower, and are gone: DESIGN.md section 4.)
// =============================================================================================
//  Arithmetic (PREC): PREC_F16 - the fast mode; PREC_F32 - actor and critic in the split-f16 arithmetic of mlp_eval_x (the network
//  wave reads a second, LOW image of the weights); PREC_F32_ACTOR - actor split, critic plain f16 on the high image.  The split
//  modes have no LDS left for the env wave's row staging: their rows go out per lane (store_row_direct), the mailbox group is
//  2 304 bytes smaller.  Rows are bit-identical to the one-wave kernels of the same arithmetic (tests).
//  Geometry (GROUPS): 4 - a 512-thread workgroup of 256 envs, an env and a network wave on every SIMD (65 536 envs fill the chip);
//  2 - a 256-thread workgroup of 128 envs, ONE wave per SIMD: for batches that leave SIMDs free (n <= 128 x CUs, e.g. config 4's
//  32 768 envs per GPU) neither wave shares its issue port.
constexpr int WSBLOCK = 512;
constexpr int WS_GROUP_FLOATS = 64 * 9 * 5 + 64 * 4 + 64;       // io | obs | pre[2] | mu | v[2] | vpre[2] | sequence words (+ pad)
constexpr int WS_GROUP_FLOATS_X = 64 * 9 * 4 + 64 * 4 + 64;     // the same without the io area
static_assert(4 * WS_GROUP_FLOATS * 4 == POLICY_WS_MAILBOX_BYTES, "dpenv_dev.h: POLICY_WS_MAILBOX_BYTES out of step with the mailbox layout");
static_assert(4 * WS_GROUP_FLOATS_X * 4 == POLICY_WS_MAILBOX_X_BYTES, "dpenv_dev.h: POLICY_WS_MAILBOX_X_BYTES out of step with the mailbox layout");
__host__ __device__ constexpr int ws_images(int prec) { return prec == PREC_F16 ? 2 : (prec == PREC_F32_ACTOR ? 3 : 4); }

// pair-level hand-over inside a workgroup: a sequence word in LDS, released by one wave and acquired by its partner.
// Both waves of a pair belong to the same workgroup, so they are always co-resident; the waiter sleeps between polls.
// Every lane's mailbox rows are released by a workgroup-scope fence that ALL lanes execute (the sequence word is stored by lane 0 alone);
// the waiter acquires with a fence after its poll loop.  On gfx950 (waves of a workgroup share a CU, no tgsplit) the release fence is the
// s_waitcnt lgkmcnt(0) that used to sit inside the lane-0 branch, the acquire fence emits nothing: same instructions, but ordered by the
// memory model instead of by in-order LDS issue and the compiler's good will.
__device__ __forceinline__ void ws_post(int* p, int v, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ws_wait(int* p, int v)
{
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < v)
        __builtin_amdgcn_s_sleep(2);       // x 64 cycles between polls (A/B'd in round 3: 0 / 1 / 2 / 4 within noise in both geometries)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define WS_EVAL(W_, B_, f0_, f1_) mlp_eval<KA>(W_, B_, pa.n_hidden, f0_, f1_, leak, outv)
//  RND: the domain randomisation's hull re-draw compiled into the reset branch (instantiated for the shipped training configuration only -
//  final variant, continuous angles, extended state, leaky-relu - see ws_general in dpenv_dev.h and dpenv_env_dev.h redraw_vessel_cold).
//  SLOSS (round 6): the SHARED training form - the single class's thrust-loss coefficients from the kernel arguments (StepArgs.kl, LOSS_SHARED;
//  zeros for a hull without a loss: the rows of the default kernels bit for bit) and the per-episode current re-draw: the thrust-loss preset and /
//  or dpenv_set_current_randomisation on the shared hull, without per-env blocks; same configurations as RND.
template <int MODE, bool EXT, int KA, int ROLES, int PREC = PREC_F16, int GROUPS = 4, bool RND = false, bool SLOSS = false>
__global__ __launch_bounds__(64 * GROUPS * ROLES) void policy_rollout_ws_kernel(const StepArgs a, const PolicyArgs pa)
{
    constexpr bool INTEG = false, REFF = false;
    const IntegArgs ia{};
    const FilterArgs fa{};
#include "dpenv_policy_ws_body.inc"
}

//  INTEG: the deployed node's integral action (IntegArgs, dpenv_set_integral_action) on the env wave; the network waves see it through the
//  observation mailbox alone
template <int MODE, bool EXT, int KA, int ROLES, int PREC, int GROUPS, bool RND, bool SLOSS>
__global__ __launch_bounds__(64 * GROUPS * ROLES) void policy_rollout_ws_integ_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia)
{
    constexpr bool INTEG = true, REFF = false;
    const FilterArgs fa{};
#include "dpenv_policy_ws_body.inc"
}

//  REFF: the setpoint reference filter (FilterArgs, dpenv_set_reference_filter) on the env wave, with the integral action if INTEG_
template <int MODE, bool EXT, int KA, int ROLES, int PREC, int GROUPS, bool RND, bool SLOSS, bool INTEG_>
__global__ __launch_bounds__(64 * GROUPS * ROLES) void policy_rollout_ws_reff_kernel(const StepArgs a, const PolicyArgs pa, const IntegArgs ia,
                                                                                      const FilterArgs fa)
{
    constexpr bool INTEG = INTEG_, REFF = true;
#include "dpenv_policy_ws_body.inc"
}


}  // namespace dpenv

// ---- host side: one launcher per arithmetic, explicitly instantiated by the translation unit that owns it -------------------------
// Which arithmetics get the critic wave (ws_roles in dpenv_dev.h) in the 128-env geometry: measured (same call,
// bit-identical rows, profiles/r04_critic_wave.txt; 32 768 / 8 192 envs): all exact 9.43 -> 7.85 / 9.24 -> 7.30 us per step, exact actor
// 7.4-7.7 -> 7.3-7.45 / 7.23 -> 7.01; f16 5.20 -> 5.50 / 4.76 -> 5.03 with row staging (116 B of scratch at the 256 registers two waves on a
// SIMD leave), 5.27 -> 5.33 / 4.79 -> 4.92 without it (no scratch): the f16 step is its chain already - so the two split arithmetics get the
// critic wave, f16 keeps two roles.
namespace dpenv {

template <int MODE, bool EXT, int KA, int PREC, int GROUPS, bool RND, bool SLOSS>
static hipError_t ws_go(const StepArgs& a, const PolicyArgs& pa, const IntegArgs* ia, const FilterArgs* fa, hipStream_t s)
{
    constexpr int ROLES = ws_roles(PREC, GROUPS);
    const dim3 grid((a.n + 64 * GROUPS - 1) / (64 * GROUPS)), block(64 * GROUPS * ROLES);
    const size_t lds = (size_t)ws_images(PREC) * pa.nent * 16 + (size_t)2 * pa.nblk * 32 * 4 +
                       (size_t)GROUPS * ((((PREC == PREC_F16 && ROLES == 2)) ? WS_GROUP_FLOATS : WS_GROUP_FLOATS_X) +
                                         (ROLES == 3 ? 64 * 9 : 0)) * 4;
    if (fa) {
        if constexpr (ws_reff(MODE, EXT, KA)) {
            if (ia)
                return launch_with_lds(policy_rollout_ws_reff_kernel<MODE, EXT, KA, ROLES, PREC, GROUPS, RND, SLOSS, true>, grid, block, lds, s, a, pa,
                                       *ia, *fa);
            return launch_with_lds(policy_rollout_ws_reff_kernel<MODE, EXT, KA, ROLES, PREC, GROUPS, RND, SLOSS, false>, grid, block, lds, s, a, pa,
                                   IntegArgs{}, *fa);
        }
        return hipErrorInvalidValue;
    }
    if (!ia) return launch_with_lds(policy_rollout_ws_kernel<MODE, EXT, KA, ROLES, PREC, GROUPS, RND, SLOSS>, grid, block, lds, s, a, pa);
    if constexpr (ws_integ(MODE, EXT, KA))
        return launch_with_lds(policy_rollout_ws_integ_kernel<MODE, EXT, KA, ROLES, PREC, GROUPS, RND, SLOSS>, grid, block, lds, s, a, pa, *ia);
    return hipErrorInvalidValue;
}

// the set the ws_* predicates of dpenv_dev.h admit; dpenv_api.hip routes everything else to the one-wave kernels
template <int PREC>
hipError_t dev::launch_policy_rollout_ws(const StepArgs* a, const PolicyArgs* pa, const IntegArgs* ia, const FilterArgs* fa, int mode, int ext,
                                         hipStream_t s)
{
    if (pa->ws_groups != 2 && pa->ws_groups != 4) return hipErrorInvalidValue;
    const bool sloss = a->loss_on == LOSS_SHARED;                    // the single class's coefficients as kernel arguments
    if (sloss && a->env_tab) return hipErrorInvalidValue;
    const bool rnd = !sloss && (a->rand_tab || a->loss_on != LOSS_NONE || a->cur_nom);   // hull / current re-draws, the table's thrust loss
    return with_mode_ext_ka(mode, ext, *pa, [&](auto M, auto E, auto K) {
        auto groups = [&](auto G) -> hipError_t {
            if constexpr (ws_has(K, PREC, G)) {
                if constexpr (ws_general(M, E, K)) {
                    if (sloss) return ws_go<M, E, K, PREC, G, false, true>(*a, *pa, ia, fa, s);
                    if (rnd) return ws_go<M, E, K, PREC, G, true, false>(*a, *pa, ia, fa, s);
                }
                if (!sloss && !rnd) return ws_go<M, E, K, PREC, G, false, false>(*a, *pa, ia, fa, s);
            }
            return hipErrorInvalidValue;
        };
        return pa->ws_groups == 2 ? groups(Int<2>{}) : groups(Int<4>{});
    });
}

}  // namespace dpenv

#endif
