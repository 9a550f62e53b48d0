// dpenv_control_nn.hip - the neural thrust allocation on the device (dpenv_thrust_alloc_nn / dpenv_set_nn_allocator in dpenv.h): the
// reference's supervised feed-forward allocator (src/sl: FFNN.py, ROS/neural_allocator) as a handle-free map tau -> action for n envs,
// and as the allocation stage of the baseline's closed loop - dpenv_control_rollout_body.inc compiled with NN: the PID's lines form tau,
// nn_allocate takes dp_allocate's place.  The law has no state and touches no hull, so the closed loop exists for every vessel source the
// pseudo-inverse flies (the shared hull, the thrust-loss preset, per-env hulls and their randomisation), with and without the reference
// filter.  The law exists once, in dpenv_nn_law.h, which also says how it is evaluated (scalar loads of the weights, a wave-private
// LDS column block for the activations, accumulators in VGPRs).  The handle's zero-padded image is the K = 1 case of the population's:
// its one packing kernel is in dpenv_control_nn_pop.hip (launch_nn_pack).
//
// A unit of its own with the library's CXXFLAGS, for the reason dpenv_label.hip is one: compiled into dpenv_control.hip, new
// instantiations of the shared body re-schedule the kernels that are there.
#include "dpenv_policy_dev.h"

namespace dpenv {

#include "dpenv_control_law.h"
// (the shared body names the QP law in the branches this unit discards)
#include "dpenv_qp_law.h"
#include "dpenv_nn_law.h"
#include "dpenv_control_rows.h"

namespace {

// The baseline's closed loop with the neural allocation: one wave per workgroup, the wave's activation block (dynamic LDS, nn_lds_bytes)
// beside the row staging area.  The weights are the handle's zero-padded image.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_nn_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                        const NnRollout nr)
{
    constexpr bool TAB = false, QP = false, QTAB = false, NN = true;
    const float4* const tab = nullptr;
    const float4* const qtab = nullptr;
    const QpRollout qr = {};
#include "dpenv_control_rollout_body.inc"
}

// the handle-free map (dpenv_thrust_alloc_nn): the caller's one network on every wave (nn_alloc_lane, dpenv_nn_law.h)
__global__ __launch_bounds__(64) void nn_alloc_kernel(const NnArgs na, const float* __restrict__ tau, float* __restrict__ action,
                                                       float* __restrict__ raw, int n)
{
    nn_alloc_lane(na, tau, action, raw, n);
}

}  // namespace
}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_nn_alloc(const NnArgs* na, const float* tau, float* action, float* raw, int n, hipStream_t s)
{
    if (!nn_args_ok(*na) || !tau || !action || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_alloc_kernel, dim3((n + 63) / 64), dim3(64), nn_lds_bytes(na->H), s, *na, tau, action, raw, n);
    return hipGetLastError();
}

hipError_t dev::launch_controller_rollout_nn(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const NnRollout* nr, int ves,
                                             hipStream_t s)
{
    if (!control_ves_ok(ves, a) || !nn_args_ok(nr->a)) return hipErrorInvalidValue;
    const dim3 grid((a->n + RBLOCK - 1) / RBLOCK), block(RBLOCK);
    const int lds = nn_lds_bytes(nr->a.H);
    return with_control_ves(ves, [&](auto V) {
        if (fa) hipLaunchKernelGGL((controller_rollout_nn_kernel<V, true>), grid, block, lds, s, *a, *ca, *fa, *nr);
        else hipLaunchKernelGGL((controller_rollout_nn_kernel<V, false>), grid, block, lds, s, *a, *ca, FilterArgs{}, *nr);
        return hipGetLastError();
    });
}
