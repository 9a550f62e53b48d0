// dpenv_control.hip - the classical baseline on the device: its closed loop and its allocators.
//
// The closed loop (dpenv_set_dp_controller / dpenv_controller_rollout in dpenv.h): a PID motion controller feeding a thrust allocation,
// evaluated in registers inside a T-step launch.  One body, dpenv_control_rollout_body.inc, compiled with the weighted pseudo-inverse
// on the shared numbers (controller_rollout_kernel), on every env's own row of the packed table (controller_rollout_tab_kernel), and
// with the rate-limited QP allocation (controller_rollout_qp_kernel, dpenv_set_qp_allocator): the PID's lines form tau, qp_allocate
// takes dp_allocate's place, the thruster state travels beside z - and the same with every env's own QP numbers held per lane
// (controller_rollout_qp_tab_kernel, dpenv_set_qp_allocator_table; pack_qp_table_kernel packs them, dpenv_thrust_alloc_qp_table is
// the handle-free form).  Beside it the table's packing, the controller's state, and the two
// allocations as handle-free maps tau -> action for n envs (dpenv_thrust_alloc, dpenv_thrust_alloc_qp: the thesis' third allocator
// beside the RL actor and the PID + pseudo-inverse chain).  The handle-free QP call: per env 12 B of wrench and 20 B of thruster state
// come in; 20 B of state, 28 B of action and (optionally) 4 B of objective go out; everything between is registers.
//
// The laws are build-defined (the reference has no PID and no pseudo-inverse node in its tree) and stated operation by operation in
// include/dpenv.h; deploy.BatchedDPController and deploy.BatchedQPAllocator are their host statements.  Each exists once on the device,
// in dpenv_control_law.h and dpenv_qp_law.h.  Everything here is plain f32 in that order: the build has -ffp-contract=off, `/` and sqrtf
// are the compiler's correctly rounded forms.
//
// A unit of its own with the library's CXXFLAGS: it needs the env's and the reference filter's device functions and the wave-private row
// staging (dpenv_policy_dev.h), nothing of the actor-critic.  The labelling scan (dpenv_label.hip) scans the same law and is NOT in this
// unit: compiled here, it re-schedules all four controller_rollout_qp_kernel instantiations.
#include "dpenv_policy_dev.h"

namespace dpenv {

// the law itself - ControlLane, ctrl_tab_index, load_control_lane, dp_allocate, dp_control - shared with the labelling scan (dpenv_label.hip)
#include "dpenv_control_law.h"
// the QP allocation, the other allocation stage the closed loop's body can be compiled with (controller_rollout_qp_kernel)
#include "dpenv_qp_law.h"
// the neural allocation, the third stage the body can be compiled with - in dpenv_control_nn.hip, not here: only the names its NN branch mentions
#include "dpenv_nn_law.h"
// control_store_rows, which the closed-loop body calls
#include "dpenv_control_rows.h"

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
    constexpr bool TAB = false, QP = false, QTAB = false, NN = false;
    const NnRollout nr = {};
    const float4* const tab = nullptr;
    const float4* const qtab = nullptr;
    const QpRollout qr = {};
#include "dpenv_control_rollout_body.inc"
}

// TAB: every env flies its own row of the packed controller block (dpenv_set_dp_controller_table) - nine 16-byte loads per env and launch
// behind the state loads, the numbers held in VGPRs for the launch, read only.  The law, the rows and everything else are the kernel above.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_tab_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                         const float4* __restrict__ tab)
{
    constexpr bool TAB = true, QP = false, QTAB = false, NN = false;
    const NnRollout nr = {};
    const float4* const qtab = nullptr;
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

namespace {

// The baseline's closed loop with the QP allocation: VES 0 (the shared hull) and VES 5 (the thrust-loss preset, currents re-drawn), with
// and without the reference filter.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_qp_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                        const QpRollout qr)
{
    constexpr bool TAB = false, QP = true, QTAB = false, NN = false;
    const NnRollout nr = {};
    const float4* const tab = nullptr;
    const float4* const qtab = nullptr;
#include "dpenv_control_rollout_body.inc"
}

// QTAB: every env flies its own row of the packed QP block (dpenv_set_qp_allocator_table) - seven 16-byte loads per env and launch in the
// opening burst, the numbers held in VGPRs for the launch, read only; of qr.q only iters is read (one count per launch: the iteration
// loop stays wave-uniform).  The law, the rows and everything else are the kernel above.  A kernel of its own name, as
// controller_rollout_tab_kernel is, so that the four scalar instantiations keep their symbols.
template <int VES, bool REFF>
__global__ __launch_bounds__(RBLOCK) void controller_rollout_qp_tab_kernel(const StepArgs a, const ControlArgs ca, const FilterArgs fa,
                                                                            const QpRollout qr, const float4* __restrict__ qtab)
{
    constexpr bool TAB = false, QP = true, QTAB = true, NN = false;
    const NnRollout nr = {};
    const float4* const tab = nullptr;
#include "dpenv_control_rollout_body.inc"
}

// The public QP table float[DPENV_QP_NPARAM][n] -> the packed block, one lane per env (dpenv_set_qp_allocator_table): qp_lane_from_row
// forms dF / da with the handle's dt, checks the row and packs a refused one as the rest allocator; refused: uint8 [n] or NULL.
__global__ __launch_bounds__(256) void pack_qp_table_kernel(const float* __restrict__ pub, float4* __restrict__ qtab,
                                                             uint8_t* __restrict__ refused, float dt, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    QpLane q;
    const bool ok = qp_lane_from_row(pub, n, i, dt, 0, q);
    float f[4 * QP_TAB_STREAMS];
    qp_lane_flatten(q, f);
#pragma unroll
    for (int k = 0; k < QP_TAB_STREAMS; ++k) qtab[qp_tab_index(i, k)] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    if (refused) refused[i] = ok ? 0 : 1;
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

// qp_alloc_kernel with row i of the PUBLIC table on env i (dpenv_thrust_alloc_qp_table): the lane reads its 26 numbers (lane-contiguous
// rows) and checks them itself, with the packing kernel's device function.  A refused lane runs the rest allocator, reports a NaN
// objective and sets its byte of refused (uint8 [n] or NULL).
__global__ __launch_bounds__(256) void qp_alloc_tab_kernel(const float* __restrict__ pub, const int iters, const float dt, const QpAllocIO io,
                                                            uint8_t* __restrict__ refused)
{
    const int n = io.n;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    QpLane q;
    const bool ok = qp_lane_from_row(pub, n, i, dt, iters, q);
    const float tau[3] = {io.tau[i], io.tau[(int64_t)n + i], io.tau[2 * (int64_t)n + i]};
    float x[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (io.state_in) {
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = io.state_in[(int64_t)k * n + i];
    }
    float act[7], J;
    qp_allocate(q, tau, x, act, J);
    if (io.state_out) {
#pragma unroll
        for (int k = 0; k < 5; ++k) io.state_out[(int64_t)k * n + i] = x[k];
    }
    float* p = io.act + (int64_t)i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = act[k];
    if (io.cost) io.cost[i] = ok ? J : __builtin_nanf("");
    if (refused) refused[i] = ok ? 0 : 1;
}

}  // namespace
}  // namespace dpenv

using namespace dpenv;

// The order of the launchers below is the order the compiler emits their kernels in, and the kernels' schedules have been seen to depend
// on it: the QP instantiations are named before the pseudo-inverse ones.

hipError_t dev::launch_qp_alloc(const QpArgs* qa, const QpAllocIO* io, hipStream_t s)
{
    if (io->n <= 0 || !io->tau || !io->act || qa->iters < 1 || qa->iters > QP_MAX_ITERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qp_alloc_kernel, dim3((io->n + 255) / 256), dim3(256), 0, s, *qa, *io);
    return hipGetLastError();
}

hipError_t dev::launch_controller_rollout(const StepArgs* a, const ControlArgs* ca, const FilterArgs* fa, const float4* tab, const QpRollout* qr,
                                          const float4* qtab, int ves, hipStream_t s)
{
    if (!control_ves_ok(ves, a)) return hipErrorInvalidValue;
    const dim3 grid((a->n + RBLOCK - 1) / RBLOCK), block(RBLOCK);
    if (!qr && qtab) return hipErrorInvalidValue;
    if (qr) {                                                    // the QP allocation: a shared hull only
        if (tab || !qr->state || qr->q.iters < 1 || qr->q.iters > QP_MAX_ITERS) return hipErrorInvalidValue;
        if (qtab) {                                              // every env on its own row of the packed QP block
            if (ves == VES_ARGS) {
                if (fa) hipLaunchKernelGGL((controller_rollout_qp_tab_kernel<VES_ARGS, true>), grid, block, 0, s, *a, *ca, *fa, *qr, qtab);
                else hipLaunchKernelGGL((controller_rollout_qp_tab_kernel<VES_ARGS, false>), grid, block, 0, s, *a, *ca, FilterArgs{}, *qr, qtab);
            } else if (ves == VES_ARGS_LOSS) {
                if (fa) hipLaunchKernelGGL((controller_rollout_qp_tab_kernel<VES_ARGS_LOSS, true>), grid, block, 0, s, *a, *ca, *fa, *qr, qtab);
                else hipLaunchKernelGGL((controller_rollout_qp_tab_kernel<VES_ARGS_LOSS, false>), grid, block, 0, s, *a, *ca, FilterArgs{}, *qr, qtab);
            } else {
                return hipErrorInvalidValue;
            }
            return hipGetLastError();
        }
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
    return with_control_ves(ves, [&](auto V) {
        if (tab) {
            if (fa) hipLaunchKernelGGL((controller_rollout_tab_kernel<V, true>), grid, block, 0, s, *a, *ca, *fa, tab);
            else hipLaunchKernelGGL((controller_rollout_tab_kernel<V, false>), grid, block, 0, s, *a, *ca, FilterArgs{}, tab);
            return hipGetLastError();
        }
        if (fa) hipLaunchKernelGGL((controller_rollout_kernel<V, true>), grid, block, 0, s, *a, *ca, *fa);
        else hipLaunchKernelGGL((controller_rollout_kernel<V, false>), grid, block, 0, s, *a, *ca, FilterArgs{});
        return hipGetLastError();
    });
}

hipError_t dev::launch_qp_state_clear(float* state, const uint8_t* mask, int n, hipStream_t s)
{
    if (!state || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qp_state_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, s, state, mask, n);
    return hipGetLastError();
}

hipError_t dev::launch_pack_controllers(const float* table, float4* tab, uint8_t* refused, int n, hipStream_t s)
{
    hipLaunchKernelGGL(pack_controllers_kernel, dim3((n + 255) / 256), dim3(256), 0, s, table, tab, refused, n);
    return hipGetLastError();
}

hipError_t dev::launch_control_state(float4* z, float* ext, const uint8_t* mask, int n, int op, hipStream_t s)
{
    hipLaunchKernelGGL(control_state_kernel, dim3((n + 255) / 256), dim3(256), 0, s, z, ext, mask, n, op);
    return hipGetLastError();
}

hipError_t dev::launch_thrust_alloc(const ControlArgs* ca, const float* tau, float* action, int n, hipStream_t s)
{
    hipLaunchKernelGGL(alloc_kernel, dim3((n + 255) / 256), dim3(256), 0, s, *ca, tau, action, n);
    return hipGetLastError();
}

hipError_t dev::launch_pack_qp_table(const float* table, float4* qtab, uint8_t* refused, float dt, int n, hipStream_t s)
{
    if (!table || !qtab || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_qp_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, table, qtab, refused, dt, n);
    return hipGetLastError();
}

hipError_t dev::launch_qp_alloc_tab(const float* table, int iters, float dt, const QpAllocIO* io, uint8_t* refused, hipStream_t s)
{
    if (!table || io->n <= 0 || !io->tau || !io->act || iters < 1 || iters > QP_MAX_ITERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qp_alloc_tab_kernel, dim3((io->n + 255) / 256), dim3(256), 0, s, table, iters, dt, *io, refused);
    return hipGetLastError();
}
