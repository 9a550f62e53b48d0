// dpenv_control_rows.h - the baseline's row store: what the closed-loop body (dpenv_control_rollout_body.inc, dpenv_control.hip) and the
// labelling scan (dpenv_label.hip) write their [.][n][W] rows with.  Defines no kernel; included inside namespace dpenv, after
// dpenv_env_dev.h (lds_order, f2bf).
#ifndef DPENV_CONTROL_ROWS_H
#define DPENV_CONTROL_ROWS_H

// A wave's 64 rows of W floats to a [.][n][W] block: staged through the wave-private LDS area, stored coalesced - wave_store_rows /
// store_rows (dpenv_policy_dev.h, dpenv_env_dev.h) restated.  A copy on purpose: instantiating those two templates for W = 9 and 7 a second
// time in the translation unit of the policy closed-loop kernels changed the instruction schedule of those kernels, which instantiate
// them too (the final variant with the extended state: 8 kernels, 2 to 36 instructions each), and every existing kernel has to stay
// what it was.  The one definition of the copy: the label scan calls it with bf16 = false.
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

#endif
