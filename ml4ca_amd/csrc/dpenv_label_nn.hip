// dpenv_label_nn.hip - the PID + network chain evaluated on rows some other flight wrote (dpenv_controller_label_nn in dpenv.h): the
// neural allocator's labels for the states an actor visited, and the PID's clipped wrench per row - the wrench the allocator is handed in
// the closed loop, which that loop never writes.  controller_label_kernel's scan (dpenv_label.hip) with nn_allocate in dp_allocate's place:
// z is carried along each env's row sequence and zeroed behind every done row; the network has no state.
//
// The laws exist once, in dpenv_control_law.h and dpenv_nn_law.h, which also says how the network is evaluated (scalar loads of the
// weights through the constant address space, a wave-private LDS column block for the activations, accumulators in VGPRs).  A unit of its
// own with the library's CXXFLAGS, for the reason dpenv_label.hip and dpenv_control_nn.hip are: no other unit's kernels see a new
// instantiation.  Per env-row 36 B of observation (18 B as bf16) and a done byte come in; 28 B of action, 24 B of raw outputs and 12 B of
// wrench go out, each only if wanted.  With act == NULL (a launch constant) the network is skipped altogether: a wrench scan bound by its
// row traffic, which needs no network.
#include <type_traits>

#include "dpenv_env_dev.h"

namespace dpenv {

#include "dpenv_control_law.h"
#include "dpenv_nn_law.h"
// control_store_rows: a wave's 64 rows staged through the wave-private LDS area, stored coalesced
#include "dpenv_control_rows.h"
#include "dpenv_label_lane.h"

namespace {

struct LabelNnRow {
    float o[6];
    uint32_t d;
};

// Forward scan over the T rows of a block, one lane per env, one wave per workgroup; rows are fetched LABEL_U at a time into one of two
// register banks while the other is consumed.  TAB: the env's own row of the packed controller table, else the shared numbers of ca.
// PAD: na's weights are the handle's zero-padded image, else the caller's arrays in place.  The wave's activation block is the dynamic
// LDS (nn_lds_bytes(H), none when act is NULL) behind the static row staging area.
template <bool TAB, bool BF16, bool PAD>
__global__ __launch_bounds__(64) void controller_label_nn_kernel(const ControlArgs ca, const NnArgs na, const LabelNnArgs la,
                                                                  const float4* __restrict__ tab)
{
    constexpr int A = 7, OD = 9, R = 6, W3 = 3;
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
    float* const hcol = nn_lds() + lane;

    // the wave's slice of a [T][n][W] block: row t starts at t * n * W + wave0 * W, and n * W - wave0 * W floats of it are the block's
    const int64_t stride_a = (int64_t)n * A, w_a = (int64_t)wave0 * A, rem_a = stride_a - w_a;
    const int64_t stride_r = (int64_t)n * R, w_r = (int64_t)wave0 * R, rem_r = stride_r - w_r;
    const int64_t stride_t = (int64_t)n * W3, w_t = (int64_t)wave0 * W3, rem_t = stride_t - w_t;

    LabelNnRow RA[LABEL_U], RB[LABEL_U];
    auto load = [&](LabelNnRow (&buf)[LABEL_U], int j) {
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
    auto consume = [&](const LabelNnRow (&buf)[LABEL_U], int j) {
#pragma unroll
        for (int u = 0; u < LABEL_U; ++u) {
            const int t = j * LABEL_U + u;
            if (t >= T) break;
            float o[OD], tau[3];
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = buf[u].o[c];
            o[6] = o[7] = o[8] = 0.0f;                           // the thrust columns: the law does not read them
            if constexpr (TAB) dp_wrench(cl, o, z, tau);
            else dp_wrench(ca, o, z, tau);
            // a NaN entry in a row some other flight wrote: the law's fminf / fmaxf clip drops it (a closed loop would fly -tau_max), the
            // host statement keeps it.  The scan keeps it too - the component it fed is NaN, so the rest rule answers such a row
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (o[c] != o[c] || o[3 + c] != o[3 + c]) tau[c] = __builtin_nanf("");
            if (la.tau) control_store_rows<W3>(lds_row, la.tau, (int64_t)t * stride_t + w_t, rem_t, tau, lane, false);
            if (la.act) {                                        // a launch constant: the wrench-only scan never enters
                float act[A], p[R];
                nn_allocate<PAD>(na, hcol, tau, act, p);
                control_store_rows<A>(lds_row, la.act, (int64_t)t * stride_a + w_a, rem_a, act, lane, false);
                if (la.raw) control_store_rows<R>(lds_row, la.raw, (int64_t)t * stride_r + w_r, rem_r, p, lane, false);
            }
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

}  // namespace
}  // namespace dpenv

using namespace dpenv;

hipError_t dev::launch_controller_label_nn(const ControlArgs* ca, const NnArgs* na, const LabelNnArgs* la, const float4* tab, int obs_bf16,
                                           int padded, hipStream_t s)
{
    if (la->n <= 0 || la->T <= 0 || !la->obs || (!la->act && !la->tau) || (la->raw && !la->act) || (la->act != nullptr) != (na != nullptr))
        return hipErrorInvalidValue;
    NnArgs g = {};
    int lds = 0;
    if (na) {
        if (!nn_args_ok(*na)) return hipErrorInvalidValue;
        g = *na;
        lds = nn_lds_bytes(na->H);
    }
    const dim3 grid((la->n + 63) / 64), block(64);
    auto launch = [&](auto t, auto b, auto p) {
        hipLaunchKernelGGL((controller_label_nn_kernel<decltype(t)::value, decltype(b)::value, decltype(p)::value>), grid, block, lds, s, *ca, g,
                           *la, tab);
    };
    auto by_rows = [&](auto t, auto p) {
        if (obs_bf16) launch(t, std::true_type(), p);
        else launch(t, std::false_type(), p);
    };
    auto by_tab = [&](auto p) {
        if (tab) by_rows(std::true_type(), p);
        else by_rows(std::false_type(), p);
    };
    if (padded) by_tab(std::true_type());
    else by_tab(std::false_type());
    return hipGetLastError();
}
