// dpenv_nn_law.h - the neural thrust allocation's law (include/dpenv.h states it operation by operation): a small dense network from the
// scaled wrench to the thruster command, evaluated per env by the env's own lane.  The ONE text of the law on the device: included inside
// namespace dpenv after dpenv_env_dev.h by dpenv_control_nn.hip (the handle-free map and the closed-loop kernels), by
// dpenv_control_nn_pop.hip (the same with a population of networks: it hands nn_allocate the wave's own NnArgs), by dpenv_label_nn.hip
// (the labelling scan) and by dpenv_control.hip (which only needs the names the shared closed-loop body mentions in its NN branch: nothing
// of this header is instantiated there).
// Everything is plain f32 in the stated order: every product-sum of a layer is an explicit fmaf, the build has -ffp-contract=off.
//
// Form.  The weights are the same for every lane, so they never enter a VGPR: W and b are read through the constant address space with
// wave-uniform indices (scalar loads, NN_CHUNK consecutive dwords of one row at a time) and go into v_fmac as SGPR operands.  The
// activations of a layer live in a wave-private LDS column block h[k][lane] (one wave per workgroup; dynamic LDS, nn_lds_bytes(H): 8 KiB
// for the reference's 20-wide shape, 24 KiB at the largest width, so the block does not limit the waves per CU below what the
// registers allow); a lane reads and writes its own column only, so no barrier is needed.  A layer is evaluated NN_CHUNK
// outputs at a time: the chunk's accumulators start at the bias, a run-time loop over the input index k reads h_k once (one ds_read) and
// issues NN_CHUNK fmaf, and the next chunk re-reads the column.  Every chunk's accumulators are distinct elements of ONE statically
// indexed array (the chunk loop is unrolled and guarded by wave-uniform tests), so all outputs of a layer are complete before the first
// of them overwrites an input in LDS - one buffer serves, not two.  Chunks past the layer's width are skipped: a 20-wide layer costs
// two chunks per input, not six.  No element of the array is indexed at run time: nothing goes to scratch.
// PAD: W[l] is the library's zero-padded image (rows of nn_pad(width) floats, so a chunk is NN_CHUNK contiguous dwords); else the
// caller's arrays in place (rows of `width` floats; the chunk's column indices are clamped to width - 1, and the duplicates computed
// past the width are never read).
#ifndef DPENV_NN_LAW_H
#define DPENV_NN_LAW_H

typedef const __attribute__((address_space(4))) float* nn_cptr;

// the wave's activation block: rows 0 .. nn_pad(H) - 1 (the nine inputs fit the first sixteen; a hidden layer's write-back fills whole
// chunks), the dynamic LDS of a launch whose kernel calls nn_allocate
constexpr int nn_lds_bytes(int H) { return nn_pad(H) * 64 * (int)sizeof(float); }

// the lane's column starts at nn_lds() + lane, element k of it at [k * 64]
__device__ __forceinline__ float* nn_lds()
{
    extern __shared__ float nn_h[];
    return nn_h;
}

// y_j = b_j, then for k ascending y_j = fmaf(W[k][j], h_k, y_j), for every j < out; acc[j] = y_j
template <bool PAD>
__device__ __forceinline__ void nn_dense(const float* Wg, const float* bg, int in, int out, const float* hcol, float (&acc)[NN_MAX_H])
{
    const nn_cptr W = (nn_cptr)Wg;
    const nn_cptr b = (nn_cptr)bg;
    const int ld = PAD ? nn_pad(out) : out;
#pragma unroll
    for (int c0 = 0; c0 < NN_MAX_H; c0 += NN_CHUNK) {
        if (c0 < out) {                                          // wave-uniform
            int cj[NN_CHUNK];
#pragma unroll
            for (int c = 0; c < NN_CHUNK; ++c) cj[c] = PAD ? c0 + c : min(c0 + c, out - 1);
#pragma unroll
            for (int c = 0; c < NN_CHUNK; ++c) acc[c0 + c] = b[cj[c]];
#pragma unroll 4
            for (int k = 0; k < in; ++k) {
                const float h = hcol[k * 64];
                const nn_cptr row = W + k * ld;
#pragma unroll
                for (int c = 0; c < NN_CHUNK; ++c) acc[c0 + c] = fmaf(row[cj[c]], h, acc[c0 + c]);
            }
        }
    }
}

// tau[3] -> the final variant's continuous-angle action [n_bow, n_port, n_star, sin_port, cos_port, sin_star, cos_star] and the
// network's six outputs p = (u_port, u_star, u_bow, a_port, a_star, a_bow); hcol: the lane's column of the wave's activation block
template <bool PAD>
__device__ __forceinline__ void nn_allocate(const NnArgs& na, float* hcol, const float tau[3], float act[7], float p[6])
{
    const int L = na.n_layers, H = na.H;
    if (na.in_dim == 9) {                                        // wave-uniform
#pragma unroll
        for (int q = 0; q < 6; ++q) hcol[q * 64] = na.in_const[q];
#pragma unroll
        for (int j = 0; j < 3; ++j) hcol[(6 + j) * 64] = tau[j] * na.tau_scale[j];
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) hcol[j * 64] = tau[j] * na.tau_scale[j];
    }
    float acc[NN_MAX_H];
#pragma unroll
    for (int j = 0; j < NN_MAX_H; ++j) acc[j] = 0.0f;
    for (int l = 0; l < L; ++l) {
        const float* Wl = na.W[0];                               // (static indices: a kernel argument indexed at run time would be copied to scratch)
        const float* bl = na.b[0];
#pragma unroll
        for (int q = 1; q < NN_MAX_LAYERS; ++q)
            if (l == q) { Wl = na.W[q]; bl = na.b[q]; }
        const int in = l == 0 ? na.in_dim : H;
        const bool last = l == L - 1;
        const int out = last ? 6 : H;
        nn_dense<PAD>(Wl, bl, in, out, hcol, acc);
        if (!last) {
#pragma unroll
            for (int c0 = 0; c0 < NN_MAX_H; c0 += NN_CHUNK) {
                if (c0 < out) {
#pragma unroll
                    for (int c = 0; c < NN_CHUNK; ++c) {
                        const float y = acc[c0 + c];
                        hcol[(c0 + c) * 64] = y > 0.0f ? y : na.leak * y;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) p[j] = acc[j];
    bool ok = isfinite(tau[0]) && isfinite(tau[1]) && isfinite(tau[2]);
#pragma unroll
    for (int j = 0; j < 6; ++j) ok = ok && isfinite(p[j]);
    float sn[2], cs[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ang = na.azimuth_mode == 1 ? na.azimuth[k] : p[3 + k] * na.angle_scale;
        sincos_lean(ang, sn[k], cs[k]);
    }
    act[0] = ok ? fminf(fmaxf(p[2], -1.0f), 1.0f) : 0.0f;
    act[1] = ok ? fminf(fmaxf(p[0], -1.0f), 1.0f) : 0.0f;
    act[2] = ok ? fminf(fmaxf(p[1], -1.0f), 1.0f) : 0.0f;
    act[3] = ok ? sn[0] : 0.0f;
    act[4] = ok ? cs[0] : 1.0f;
    act[5] = ok ? sn[1] : 0.0f;
    act[6] = ok ? cs[1] : 1.0f;
}

// The handle-free map's lane (nn_alloc_kernel, nn_alloc_pop_kernel) from "which NnArgs" on: tau [3][n] -> action [n][7] and, if raw, the
// network's outputs [n][6]; one lane per env, one wave per workgroup, the weights read in place.  Dead lanes shadow env n - 1 and store
// nothing.  (The kernels' parameters carry __restrict__, these do not: repeated here it re-schedules both kernels.)
__device__ __forceinline__ void nn_alloc_lane(const NnArgs& na, const float* tau, float* action, float* raw, int n)
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

#endif
