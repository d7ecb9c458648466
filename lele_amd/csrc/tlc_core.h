// tlc_core.h -- the time-major depthwise stencil of ONE (channel, time tile), shared by dwconv1d_tlc_kernel (conv.hip: tiles of a dense
// [B, T, P] tensor) and dwconv1d_tlc_seg_kernel (segments.hip: tiles of a packed batch's segments), so that a segment is the dense
// call on it alone by construction.
#pragma once
#include "simd_math.h"

namespace lele {

// Workgroup b runs on XCD b % 8: the logical item index under which every XCD walks one contiguous range of the grid's items
__device__ __forceinline__ unsigned tlc_xcd_index(unsigned total) {
    const unsigned G = gridDim.x, xcd = blockIdx.x & 7u, gbase = G >> 3, grem = G & 7u;
    const unsigned logical = xcd * gbase + (xcd < grem ? xcd : grem) + (blockIdx.x >> 3);
    return logical * 256u + threadIdx.x;
}

// xp / op: channel ch of time step 0 of the sequence (t_in steps of `pitch` elements in, t_out steps of `c` elements out).  A lane
// produces TT consecutive time steps from t0 from a sliding register window.  Per output: taps in ascending order, taps outside
// [0, t_in) skipped (not multiplied by zero), FMA chain, bias added afterwards.
template <int KW, int TT>
__device__ __forceinline__ void tlc_tile(const float* __restrict__ xp, const float* __restrict__ w, const float* __restrict__ bias,
                                         float* __restrict__ op, unsigned ch, int t0, int t_in, int t_out, int c, int pitch, int pl, int relu,
                                         int add_input) {
    float xs[KW + TT - 1], wv[KW];
#pragma unroll
    for (int j = 0; j < KW + TT - 1; ++j) {
        const int t = t0 - pl + j;
        xs[j] = xp[(size_t)min(max(t, 0), t_in - 1) * pitch];
    }
#pragma unroll
    for (int j = 0; j < KW; ++j) wv[j] = w[ch * KW + j];
    const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
    for (int q = 0; q < TT; ++q) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            const int t = t0 + q - pl + j;
            const float f = fmaf_(xs[q + j], wv[j], acc);
            acc = (t >= 0 && t < t_in) ? f : acc;
        }
        if (bias) acc = acc + bv;
        if (relu) acc = acc > 0.0f ? acc : 0.0f;
        // the FSMN residual (memory + input): x[t0 + q] sits at window index q + pl (the host checks pl <= KW - 1);
        // a separate unrolled select keeps the index a compile-time constant per (q, pl) pair
        if (add_input) {
            float xv = 0.0f;
#pragma unroll
            for (int j = 0; j < KW; ++j) xv = (j == pl) ? xs[q + j] : xv;
            acc = acc + xv;
        }
        if (t0 + q < t_out) op[(size_t)(t0 + q) * c] = acc;
    }
}

}  // namespace lele
