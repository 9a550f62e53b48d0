// dpenv_label.hip - the baseline DP controller's law evaluated on rows some other flight wrote (dpenv_controller_label in dpenv.h): expert
// labels for the states an actor visited (DAgger), or the distance between an actor's actions and the baseline's on those states.
//
// The law exists once, in dpenv_control_law.h; the closed-loop kernels (dpenv_control.hip) weld it to env_step, this unit scans it over a
// [T][n][9] observation block.  The integral z is carried along each env's row sequence and zeroed behind every done row, so the label
// of row t depends on every row before it: a scan, one lane per env, not a map over rows.
//
// A unit of its own with the library's CXXFLAGS: no other unit's kernels see a new instantiation (dpenv_control_rows.h records what a
// second instantiation of a shared template does to its neighbours' schedules).  Not merged into dpenv_control.hip: that re-schedules
// the QP closed loop (all four controller_rollout_qp_kernel instantiations).  Per env-row 36 B of observation (18 B as bf16) and a
// done byte come in, 28 B of action go out; the handle's state is neither read nor written.
//
// Two scans: controller_label_kernel allocates the PID's wrench with the pseudo-inverse (dp_control), controller_label_qp_kernel with the
// rate-limited QP law of dpenv_qp_law.h (dpenv_controller_label_qp), whose thruster state travels beside z and whose objective can go
// out beside the action (4 B per env-row).  The first is bound by its row traffic, the second by VALU issue.  controller_label_qp_ex_kernel
// is the second with the thruster state taken from the flown action rows and / or one QP allocator per env (dpenv_controller_label_qp_ex):
// the two are one body, dpenv_label_qp_body.inc.  A lane's place in the wave is label_lane for all three.  The rest of the lane prologue
// (z and x in and out, a row's six columns and done byte) stands once in that body and once in controller_label_kernel, not in shared
// device functions: tried as __forceinline__ helpers, the z load, the row decode and the z store each re-scheduled controller_label_kernel,
// and a store helper instantiated for both argument blocks re-scheduled all twenty kernels of the unit (tools/isa_diff.py against the
// unit before; profiles/controller_family_isa_diff.txt is the record of what stands).
#include <type_traits>

#include "dpenv_env_dev.h"

namespace dpenv {

#include "dpenv_control_law.h"
// the QP allocation the second scan (controller_label_qp_kernel) puts behind the PID lines
#include "dpenv_qp_law.h"
// control_store_rows: a wave's 64 action rows staged through the wave-private LDS area, stored coalesced
#include "dpenv_control_rows.h"
// LABEL_U and label_lane, shared with the network's scan (dpenv_label_nn.hip)
#include "dpenv_label_lane.h"

namespace {

struct LabelRow {
    float o[6];
    uint32_t d;
};
// ... and, FLOWN, the action row that was executed on it
template <bool FLOWN>
struct LabelRowEx {
    float o[6];
    uint32_t d;
    float f[FLOWN ? 7 : 1];
};

// Forward scan over the T rows of a block, one lane per env, one wave per workgroup.  The law is serial in t, but no load depends on it:
// rows are fetched LABEL_U at a time into one of two register banks while the other is consumed.  TAB: the env's own row of the packed
// controller table, nine 16-byte loads in the opening burst; else the shared numbers of ca (SGPRs).  Dead lanes shadow env n - 1 and
// store nothing.
template <bool TAB, bool BF16>
__global__ __launch_bounds__(64) void controller_label_kernel(const ControlArgs ca, const LabelArgs la, const float4* __restrict__ tab)
{
    constexpr int A = 7, OD = 9;
    __shared__ float lds_row[64 * A];

    const int n = la.n, T = la.T;
    const LabelLane L = label_lane(n);
    const int lane = L.lane, wave0 = L.wave0, i = L.i, il = L.il;
    const bool live = L.live;

    ControlLane cl;
    if constexpr (TAB) load_control_lane(tab, il, ca.dt, cl);
    float z[3] = {0.0f, 0.0f, 0.0f};
    if (la.z_in) {
        z[0] = la.z_in[il]; z[1] = la.z_in[(int64_t)n + il]; z[2] = la.z_in[2 * (int64_t)n + il];
    }

    const int64_t stride_a = (int64_t)n * A;
    const int64_t w_a = (int64_t)wave0 * A;                      // the wave's slice of the [T][n][7] block
    const int64_t rem_a = stride_a - w_a;

    LabelRow RA[LABEL_U], RB[LABEL_U];
    auto load = [&](LabelRow (&buf)[LABEL_U], int j) {
#pragma unroll
        for (int u = 0; u < LABEL_U; ++u) {
            int t = j * LABEL_U + u;
            t = t < T ? t : T - 1;                               // past the end: re-read the last row (never consumed)
            const int64_t k = (int64_t)t * n + il;
            if (BF16) {
                const uint16_t* p = (const uint16_t*)la.obs + k * OD;
#pragma unroll
                for (int c = 0; c < 6; ++c) buf[u].o[c] = __uint_as_float((uint32_t)p[c] << 16);
            } else {
                const float* p = (const float*)la.obs + k * OD;
#pragma unroll
                for (int c = 0; c < 6; ++c) buf[u].o[c] = p[c];
            }
            buf[u].d = la.done ? (uint32_t)la.done[k] : 0u;
        }
    };
    auto consume = [&](const LabelRow (&buf)[LABEL_U], int j) {
#pragma unroll
        for (int u = 0; u < LABEL_U; ++u) {
            const int t = j * LABEL_U + u;
            if (t >= T) break;
            float o[OD], act[A];
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = buf[u].o[c];
            o[6] = o[7] = o[8] = 0.0f;                           // the thrust columns: the law does not read them
            if constexpr (TAB) dp_control(cl, o, z, act);
            else dp_control(ca, o, z, act);
            control_store_rows<A>(lds_row, la.act, (int64_t)t * stride_a + w_a, rem_a, act, lane, false);
            if (buf[u].d != 0u) z[0] = z[1] = z[2] = 0.0f;       // the next row is a new episode's first
        }
    };
    const int nb = (T + LABEL_U - 1) / LABEL_U;
    load(RA, 0);
    for (int j = 0; j < nb; j += 2) {
        load(RB, j + 1);
        consume(RA, j);
        load(RA, j + 2);
        consume(RB, j + 1);
    }
    if (live && la.z_out) {
        la.z_out[i] = z[0]; la.z_out[(int64_t)n + i] = z[1]; la.z_out[2 * (int64_t)n + i] = z[2];
    }
}

// dpenv_label_qp_body.inc without the flown rows and the per-env QP table
template <bool TAB, bool BF16>
__global__ __launch_bounds__(64) void controller_label_qp_kernel(const ControlArgs ca, const QpArgs qa, const LabelQpArgs la,
                                                                  const float4* __restrict__ tab)
{
    constexpr bool QTAB = false, FLOWN = false;
    const LabelQpExArgs xa = {};
#include "dpenv_label_qp_body.inc"
}

template <bool TAB, bool QTAB, bool FLOWN, bool BF16>
__global__ __launch_bounds__(64) void controller_label_qp_ex_kernel(const ControlArgs ca, const QpArgs qa, const LabelQpArgs la,
                                                                     const LabelQpExArgs xa, const float4* __restrict__ tab)
{
#include "dpenv_label_qp_body.inc"
}

}  // namespace
}  // namespace dpenv

using namespace dpenv;

// the four instantiations of a scan over (controller table, bf16 rows): launch(tab_c, bf16_c) launches the one its two constants name
namespace {
template <class F>
void label_dispatch(const float4* tab, int obs_bf16, F launch)
{
    using std::true_type;
    using std::false_type;
    if (tab) {
        if (obs_bf16) launch(true_type(), true_type());
        else launch(true_type(), false_type());
    } else {
        if (obs_bf16) launch(false_type(), true_type());
        else launch(false_type(), false_type());
    }
}
}  // namespace

hipError_t dev::launch_controller_label(const ControlArgs* ca, const LabelArgs* la, const float4* tab, int obs_bf16, hipStream_t s)
{
    if (la->n <= 0 || la->T <= 0 || !la->obs || !la->act) return hipErrorInvalidValue;
    const dim3 grid((la->n + 63) / 64), block(64);
    label_dispatch(tab, obs_bf16, [&](auto t, auto b) {
        hipLaunchKernelGGL((controller_label_kernel<decltype(t)::value, decltype(b)::value>), grid, block, 0, s, *ca, *la, tab);
    });
    return hipGetLastError();
}

hipError_t dev::launch_controller_label_qp(const ControlArgs* ca, const QpArgs* qa, const LabelQpArgs* la, const float4* tab, int obs_bf16,
                                           hipStream_t s)
{
    if (la->n <= 0 || la->T <= 0 || !la->obs || !la->act || qa->iters < 1 || qa->iters > QP_MAX_ITERS) return hipErrorInvalidValue;
    const dim3 grid((la->n + 63) / 64), block(64);
    label_dispatch(tab, obs_bf16, [&](auto t, auto b) {
        hipLaunchKernelGGL((controller_label_qp_kernel<decltype(t)::value, decltype(b)::value>), grid, block, 0, s, *ca, *qa, *la, tab);
    });
    return hipGetLastError();
}

// Named after the launchers above: the compiler emits the kernels in the order of their launchers, and the parent's kernels keep their place.
namespace {
template <bool QTAB, bool FLOWN>
void launch_label_qp_ex(const ControlArgs* ca, const QpArgs* qa, const LabelQpArgs* la, const LabelQpExArgs* xa, const float4* tab, int obs_bf16,
                        hipStream_t s)
{
    const dim3 grid((la->n + 63) / 64), block(64);
    label_dispatch(tab, obs_bf16, [&](auto t, auto b) {
        hipLaunchKernelGGL((controller_label_qp_ex_kernel<decltype(t)::value, QTAB, FLOWN, decltype(b)::value>), grid, block, 0, s, *ca, *qa, *la, *xa, tab);
    });
}
}  // namespace

hipError_t dev::launch_controller_label_qp_ex(const ControlArgs* ca, const QpArgs* qa, const LabelQpArgs* la, const LabelQpExArgs* xa,
                                              const float4* tab, int obs_bf16, hipStream_t s)
{
    if (la->n <= 0 || la->T <= 0 || !la->obs || !la->act || (!xa->flown && !xa->qp_table)) return hipErrorInvalidValue;
    const int iters = xa->qp_table ? xa->iters : qa->iters;
    if (iters < 1 || iters > QP_MAX_ITERS || (xa->refused && !xa->qp_table)) return hipErrorInvalidValue;
    if (xa->qp_table) {
        if (xa->flown) launch_label_qp_ex<true, true>(ca, qa, la, xa, tab, obs_bf16, s);
        else launch_label_qp_ex<true, false>(ca, qa, la, xa, tab, obs_bf16, s);
    } else {
        launch_label_qp_ex<false, true>(ca, qa, la, xa, tab, obs_bf16, s);
    }
    return hipGetLastError();
}
