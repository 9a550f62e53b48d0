// dpenv_qp.hip - the rate-limited QP thrust allocation on the device (dpenv_thrust_alloc_qp in dpenv.h): the thesis' third allocator beside
// the RL actor and the PID + pseudo-inverse chain, as a handle-free, stateful map tau -> action for n envs.
//
// And the same law as the allocation stage of the baseline's closed loop (dpenv_set_qp_allocator): controller_rollout_qp_kernel is the body
// of controller_rollout_kernel (dpenv_control_rollout_body.inc) compiled with QP = true - the PID's lines form tau, qp_allocate takes
// dp_allocate's place, the thruster state travels beside z.
//
// The law exists once, in dpenv_qp_law.h.  A unit of its own with the library's CXXFLAGS, like dpenv_label.hip: no other unit's kernels see
// a new instantiation.  The handle-free call: per env 12 B of wrench and 20 B of thruster state come in; 20 B of state, 28 B of action and
// (optionally) 4 B of objective go out; everything between is registers.
#include "dpenv_policy_dev.h"

namespace dpenv {

#include "dpenv_control_law.h"
#include "dpenv_qp_law.h"

namespace {

// control_store_rows of dpenv_control_dev.h, which the closed-loop body calls: a wave's 64 rows of W floats staged through the wave-private
// LDS area, stored coalesced.  A copy for the reason given there (that header also defines kernels this unit must not define again).
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

// The baseline's closed loop with the QP allocation: VES 0 (the shared hull) and VES 5 (the thrust-loss preset, currents re-drawn), with
// and without the reference filter.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_qp_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                        const QpRollout qr)
{
    constexpr bool TAB = false, QP = true;
    const float4* const tab = nullptr;
#include "dpenv_control_rollout_body.inc"
}

// zeroes the thruster state [5][n] of the envs of mask (NULL = every env): dpenv_reset, turning the allocator on
__global__ __launch_bounds__(256) void qp_state_clear_kernel(float* state, const uint8_t* mask, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (mask != nullptr && mask[i] == 0)) return;
#pragma unroll
    for (int k = 0; k < 5; ++k) state[(int64_t)k * n + i] = 0.0f;
}

// One lane per env.  The [5][n] state is read whole before anything is written, and only by the env's own lane: state_out may be state_in.
__global__ __launch_bounds__(256) void qp_alloc_kernel(const QpArgs qa, const QpAllocIO io)
{
    const int n = io.n;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float tau[3] = {io.tau[i], io.tau[(int64_t)n + i], io.tau[2 * (int64_t)n + i]};
    float x[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (io.state_in) {
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = io.state_in[(int64_t)k * n + i];
    }
    float act[7], J;
    qp_allocate(qa, tau, x, act, J);
    if (io.state_out) {
#pragma unroll
        for (int k = 0; k < 5; ++k) io.state_out[(int64_t)k * n + i] = x[k];
    }
    float* p = io.act + (int64_t)i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = act[k];
    if (io.cost) io.cost[i] = J;
}

}  // namespace
}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_qp_alloc(const QpArgs* qa, const QpAllocIO* io, hipStream_t s)
{
    if (io->n <= 0 || !io->tau || !io->act || qa->iters < 1 || qa->iters > QP_MAX_ITERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qp_alloc_kernel, dim3((io->n + 255) / 256), dim3(256), 0, s, *qa, *io);
    return hipGetLastError();
}

hipError_t dev::launch_controller_rollout_qp(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const QpRollout* qr, int ves,
                                             hipStream_t s)
{
    if (!qr->state || qr->q.iters < 1 || qr->q.iters > QP_MAX_ITERS) return hipErrorInvalidValue;
    if ((ves == VES_ARGS_LOSS) != (a->loss_on == LOSS_SHARED)) return hipErrorInvalidValue;   // as launch_controller_rollout's
    const dim3 grid((a->n + RBLOCK - 1) / RBLOCK), block(RBLOCK);
    if (ves == VES_ARGS) {
        if (fa) hipLaunchKernelGGL((controller_rollout_qp_kernel<VES_ARGS, true>), grid, block, 0, s, *a, *ca, *fa, *qr);
        else hipLaunchKernelGGL((controller_rollout_qp_kernel<VES_ARGS, false>), grid, block, 0, s, *a, *ca, FilterArgs{}, *qr);
    } else if (ves == VES_ARGS_LOSS) {
        if (fa) hipLaunchKernelGGL((controller_rollout_qp_kernel<VES_ARGS_LOSS, true>), grid, block, 0, s, *a, *ca, *fa, *qr);
        else hipLaunchKernelGGL((controller_rollout_qp_kernel<VES_ARGS_LOSS, false>), grid, block, 0, s, *a, *ca, FilterArgs{}, *qr);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dev::launch_qp_state_clear(float* state, const uint8_t* mask, int n, hipStream_t s)
{
    if (!state || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qp_state_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, s, state, mask, n);
    return hipGetLastError();
}
