// dpenv_control_nn_pop.hip - a POPULATION of neural thrust allocators on the device (dpenv_set_nn_allocator_population /
// dpenv_thrust_alloc_nn_population in dpenv.h): K networks of one shape and one set of constants, one network per run of whole waves.
// The closed loop and the handle-free map run one wave per workgroup, so "the wave's network" is a function of blockIdx.x alone:
//     net = ((wave_base + blockIdx.x) / waves_per_net) % K
// is wave-uniform by construction, and so are the wave's per-layer addresses W[l] + net * in_l * ld_l and b[l] + net * ld_l.  They are
// formed ONCE per launch, in 64-bit scalar arithmetic, into an NnArgs of the wave's own; from there on the kernel is the scalar
// network's: dpenv_nn_law.h and dpenv_control_rollout_body.inc are included as they are, not copied and not changed (the body's NN branch
// flies the `nr` it finds in scope, which here is the wave's), the weights arrive by scalar loads and enter v_fmac_f32 as SGPR operands.
// The % K keeps every address inside the K networks whatever n and env_id_base are.  A network per single ENV is not here and cannot
// be had this way: its addresses would differ between lanes, and the weights would leave the scalar path for one vector load per fmaf.
// The handle-free map's lane after the addresses is dpenv_nn_law.h's nn_alloc_lane, the scalar map's.  The library's ONE packing kernel
// is here too: the one network of dpenv_set_nn_allocator is packed as a population of K = 1, whose image is the same bytes.
//
// A unit of its own with the library's CXXFLAGS, for the reason dpenv_control_nn.hip is one: no kernel of another unit is re-scheduled.
#include "dpenv_policy_dev.h"

namespace dpenv {

#include "dpenv_control_law.h"
// (the shared body names the QP law in the branches this unit discards)
#include "dpenv_qp_law.h"
#include "dpenv_nn_law.h"
#include "dpenv_control_rows.h"

namespace {

// network `net` of the stacked arrays; PAD: the library's zero-padded image (rows of nn_pad(width) floats), else the caller's arrays in
// place (per-layer strides in * out and out).  Layers past n_layers get addresses nothing reads.
template <bool PAD>
__device__ __forceinline__ NnArgs nn_pop_network(const NnPop& p, uint32_t wave)
{
    const uint32_t net = (wave / (uint32_t)p.waves_per_net) % (uint32_t)p.K;     // < K
    NnArgs w = p.a;
#pragma unroll
    for (int l = 0; l < NN_MAX_LAYERS; ++l) {
        const int in = l == 0 ? p.a.in_dim : p.a.H;
        const int out = l == p.a.n_layers - 1 ? 6 : p.a.H;
        const int ld = PAD ? nn_pad(out) : out;
        w.W[l] = p.a.W[l] + (int64_t)net * (int64_t)(in * ld);
        w.b[l] = p.a.b[l] + (int64_t)net * (int64_t)ld;
    }
    return w;
}

// controller_rollout_nn_kernel with the wave's network out of the handle's image of K
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_nn_pop_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                            const NnPop pop)
{
    constexpr bool TAB = false, QP = false, QTAB = false, NN = true;
    const float4* const tab = nullptr;
    const float4* const qtab = nullptr;
    const QpRollout qr = {};
    const NnRollout nr = {nn_pop_network<true>(pop, pop.wave_base + blockIdx.x)};
#include "dpenv_control_rollout_body.inc"
}

// nn_alloc_kernel with the wave's network out of the caller's stacked arrays, read in place
__global__ __launch_bounds__(64) void nn_alloc_pop_kernel(const NnPop pop, const float* __restrict__ tau, float* __restrict__ action,
                                                           float* __restrict__ raw, int n)
{
    nn_alloc_lane(nn_pop_network<false>(pop, pop.wave_base + blockIdx.x), tau, action, raw, n);
}

// The caller's arrays -> the zero-padded image of K networks (the one network of dpenv_set_nn_allocator: K = 1): block (net, l, k) copies
// row k of layer l of network net (row in_l: the bias), thread j column j
__global__ __launch_bounds__(NN_MAX_H) void nn_pack_pop_kernel(const NnPack np)
{
    const int net = blockIdx.x, l = blockIdx.y, k = blockIdx.z, j = threadIdx.x;
    const float *W = np.W[0], *b = np.b[0];
    float *dW = np.dW[0], *db = np.db[0];
#pragma unroll
    for (int q = 1; q < NN_MAX_LAYERS; ++q)
        if (l == q) { W = np.W[q]; b = np.b[q]; dW = np.dW[q]; db = np.db[q]; }
    const int in = l == 0 ? np.in_dim : np.H;
    const int out = l == np.n_layers - 1 ? 6 : np.H;
    const int ld = nn_pad(out);
    if (net >= np.K || k > in || j >= ld) return;
    W += (int64_t)net * (in * out); b += (int64_t)net * out;
    dW += (int64_t)net * (in * ld); db += (int64_t)net * ld;
    if (k < in) dW[k * ld + j] = j < out ? W[k * out + j] : 0.0f;
    else db[j] = j < out ? b[j] : 0.0f;
}

bool pop_ok(const NnPop* np) { return nn_args_ok(np->a) && np->K >= 1 && np->waves_per_net >= 1; }

}  // namespace
}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_nn_alloc_pop(const NnPop* np, const float* tau, float* action, float* raw, int n, hipStream_t s)
{
    if (!pop_ok(np) || !tau || !action || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_alloc_pop_kernel, dim3((n + 63) / 64), dim3(64), nn_lds_bytes(np->a.H), s, *np, tau, action, raw, n);
    return hipGetLastError();
}

hipError_t dev::launch_controller_rollout_nn_pop(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const NnPop* np, int ves,
                                                 hipStream_t s)
{
    if (!control_ves_ok(ves, a) || !pop_ok(np)) return hipErrorInvalidValue;
    const dim3 grid((a->n + RBLOCK - 1) / RBLOCK), block(RBLOCK);
    const int lds = nn_lds_bytes(np->a.H);
    return with_control_ves(ves, [&](auto V) {
        if (fa) hipLaunchKernelGGL((controller_rollout_nn_pop_kernel<V, true>), grid, block, lds, s, *a, *ca, *fa, *np);
        else hipLaunchKernelGGL((controller_rollout_nn_pop_kernel<V, false>), grid, block, lds, s, *a, *ca, FilterArgs{}, *np);
        return hipGetLastError();
    });
}

hipError_t dev::launch_nn_pack(const NnPack* np, hipStream_t s)
{
    if (!nn_args_ok(*np) || np->K < 1) return hipErrorInvalidValue;
    for (int l = 0; l < np->n_layers; ++l)
        if (!np->dW[l] || !np->db[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_pack_pop_kernel, dim3(np->K, np->n_layers, NN_MAX_H + 1), dim3(NN_MAX_H), 0, s, *np);
    return hipGetLastError();
}
