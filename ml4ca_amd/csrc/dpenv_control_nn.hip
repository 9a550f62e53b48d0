// dpenv_control_nn.hip - the neural thrust allocation on the device (dpenv_thrust_alloc_nn / dpenv_set_nn_allocator in dpenv.h): the
// reference's supervised feed-forward allocator (src/sl: FFNN.py, ROS/neural_allocator) as a handle-free map tau -> action for n envs,
// and as the allocation stage of the baseline's closed loop - dpenv_control_rollout_body.inc compiled with NN: the PID's lines form tau,
// nn_allocate takes dp_allocate's place.  The law has no state and touches no hull, so the closed loop exists for every vessel source the
// pseudo-inverse flies (the shared hull, the thrust-loss preset, per-env hulls and their randomisation), with and without the reference
// filter.  The law exists once, in dpenv_nn_law.h, which also says how it is evaluated (scalar loads of the weights, a wave-private
// LDS column block for the activations, accumulators in VGPRs).
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

// the handle-free map (dpenv_thrust_alloc_nn): tau [3][n] -> action [n][7] and, if raw, the network's outputs [n][6]; one lane per env,
// one wave per workgroup, the caller's weights read in place.  Dead lanes shadow env n - 1 and store nothing.
__global__ __launch_bounds__(64) void nn_alloc_kernel(const NnArgs na, const float* __restrict__ tau, float* __restrict__ action,
                                                       float* __restrict__ raw, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const int il = live ? i : n - 1;
    const float t[3] = {tau[il], tau[(int64_t)n + il], tau[2 * (int64_t)n + il]};
    float act[7], p[6];
    nn_allocate<false>(na, nn_lds() + threadIdx.x, t, act, p);
    if (!live) return;
    float* q = action + (int64_t)i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) q[k] = act[k];
    if (raw) {
        float* r = raw + (int64_t)i * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = p[k];
    }
}

// The caller's arrays -> the zero-padded image: block (k, l) copies row k of layer l (row in_l: the bias), thread j column j.
__global__ __launch_bounds__(NN_MAX_H) void nn_pack_kernel(const NnPack np)
{
    const int l = blockIdx.y, k = blockIdx.x, j = threadIdx.x;
    const float *W = np.W[0], *b = np.b[0];
    float *dW = np.dW[0], *db = np.db[0];
#pragma unroll
    for (int q = 1; q < NN_MAX_LAYERS; ++q)
        if (l == q) { W = np.W[q]; b = np.b[q]; dW = np.dW[q]; db = np.db[q]; }
    const int in = l == 0 ? np.in_dim : np.H;
    const int out = l == np.n_layers - 1 ? 6 : np.H;
    const int ld = nn_pad(out);
    if (k > in || j >= ld) return;
    if (k < in) dW[k * ld + j] = j < out ? W[k * out + j] : 0.0f;
    else db[j] = j < out ? b[j] : 0.0f;
}

}  // namespace
}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_nn_alloc(const NnArgs* na, const float* tau, float* action, float* raw, int n, hipStream_t s)
{
    if (!nn_shape_ok(na->n_layers, na->in_dim, na->H) || !tau || !action || n <= 0) return hipErrorInvalidValue;
    for (int l = 0; l < na->n_layers; ++l)
        if (!na->W[l] || !na->b[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_alloc_kernel, dim3((n + 63) / 64), dim3(64), nn_lds_bytes(na->H), s, *na, tau, action, raw, n);
    return hipGetLastError();
}

hipError_t dev::launch_controller_rollout_nn(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const NnRollout* nr, int ves,
                                             hipStream_t s)
{
    if ((ves == VES_ENV_VGPR || ves == VES_ENV_RND) && !a->env_tab) return hipErrorInvalidValue;
    if ((ves == VES_ARGS_LOSS) != (a->loss_on == LOSS_SHARED)) return hipErrorInvalidValue;
    if (!nn_shape_ok(nr->a.n_layers, nr->a.in_dim, nr->a.H)) return hipErrorInvalidValue;
    for (int l = 0; l < nr->a.n_layers; ++l)
        if (!nr->a.W[l] || !nr->a.b[l]) return hipErrorInvalidValue;
    const dim3 grid((a->n + RBLOCK - 1) / RBLOCK), block(RBLOCK);
    const int lds = nn_lds_bytes(nr->a.H);
    return with_control_ves(ves, [&](auto V) {
        if (fa) hipLaunchKernelGGL((controller_rollout_nn_kernel<V, true>), grid, block, lds, s, *a, *ca, *fa, *nr);
        else hipLaunchKernelGGL((controller_rollout_nn_kernel<V, false>), grid, block, lds, s, *a, *ca, FilterArgs{}, *nr);
        return hipGetLastError();
    });
}

hipError_t dev::launch_nn_pack(const NnPack* np, hipStream_t s)
{
    if (!nn_shape_ok(np->n_layers, np->in_dim, np->H)) return hipErrorInvalidValue;
    for (int l = 0; l < np->n_layers; ++l)
        if (!np->W[l] || !np->b[l] || !np->dW[l] || !np->db[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_pack_kernel, dim3(NN_MAX_H + 1, np->n_layers), dim3(NN_MAX_H), 0, s, *np);
    return hipGetLastError();
}
