// quant.hip -- lele's dynamic-quantised u8 linear path on gfx950 (i8 MFMA, v_mfma_i32_32x32x32_i8).
//
//   lele_hip_fused_quantized_linear     <- /root/reference/src/kernels/quantization.rs:77-169 (x86 branch) +
//                                          src/kernels/avx/quantization.rs:102-417 (DynQuant + u8 GEMM + epilogue)
//   lele_hip_dynamic_quantize_linear    <- quantization.rs:1628-1657 + avx/quantization.rs:832-927
//   lele_hip_mat_mul_integer_with_scale_bias (zero points, scale, bias, ReLU all optional)
//                                       <- quantization.rs:8-72, 927-992 + avx/quantization.rs:642-830
//
// Bit-exact with the reference: the integer part is exact, every rounding step is reproduced
// (round-half-even(fma(x,1/scale,zp)) in the 8-wide body, f32::round(x*inv+zp) in the per-row scalar tail; epilogue
// (float)acc * (dyn_scale*w_scale[j]) then + bias then max(.,0), mul and add NOT fused).
//
// Pipeline per call (all on the ctx stream):
//   1. qminmax_kernel + qparams_kernel : min/max of each batch slice -> {scale, zp, 1/scale}   (one range per slice!)
//   2. qrows_kernel                    : f32 rows -> i8 (q - 128) rows padded to 16, + exact i32 row sums
//   3. igemm_kernel                    : sum (q-128)(w-128) on the matrix cores; zero-point algebra + f32 epilogue
// Weights (f32-encoded u8 [K,N], as lele's TensorView::from_bytes_u8 carries them) are transposed once to i8
// [N, Kpad] (w - 128) with column sums and cached per (pointer, bytes) -- the analogue of B_WEIGHT_CACHE
// (avx/quantization.rs:12-95).
#include "common.h"
#include "lane_ops.h"
#include "gemm_small.h"
#include "norm_core.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>

using namespace lele;

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

struct QParams {  // per batch slice
    float scale, zp, inv_scale;
    int zp_i;
};

// ------------------------------------------------------------------------------------------ 1. range
__global__ __launch_bounds__(256) void qminmax_kernel(const float* __restrict__ x, int64_t slice_len,
                                                      float* __restrict__ partial /*[slices][blocks][2]*/) {
    const float* p = x + (int64_t)blockIdx.y * slice_len;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    auto upd = [&](float v) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    };
    // scalar head up to the first 16-byte boundary, float4 body, scalar tail (min/max are order-independent: exact)
    const int64_t head = std::min<int64_t>(slice_len, (int64_t)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    const int64_t nvec = (slice_len - head) / 4;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    if (gtid < head) upd(p[gtid]);
    const float4* pv = reinterpret_cast<const float4*>(p + head);
    for (int64_t i = gtid; i < nvec; i += gstride) {
        const float4 v = pv[i];
        upd(v.x);
        upd(v.y);
        upd(v.z);
        upd(v.w);
    }
    for (int64_t i = head + nvec * 4 + gtid; i < slice_len; i += gstride) upd(p[i]);
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    __shared__ float smn[4], smx[4];
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = smn[w] < mn ? smn[w] : mn;
            mx = smx[w] > mx ? smx[w] : mx;
        }
        float* o = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = mn;
        o[1] = mx;
    }
}

// The same for a packed batch: grid.y = segment, whose slice is the rows off[y] .. off[y + 1] of x [R, k] (an empty segment leaves
// the neutral pair, which nobody reads).  min / max are order-independent, so a segment's pair is qminmax_kernel's on it alone.
__global__ __launch_bounds__(256) void qminmax_seg_kernel(const float* __restrict__ x, const int64_t* __restrict__ off, int64_t k,
                                                          float* __restrict__ partial /*[segments][blocks][2]*/) {
    const int64_t r0 = off[blockIdx.y], slice_len = (off[blockIdx.y + 1] - r0) * k;
    const float* p = x + r0 * k;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    auto upd = [&](float v) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    };
    // as qminmax_kernel: scalar head up to the segment's first 16-byte boundary, float4 body, scalar tail
    const int64_t head = std::min<int64_t>(slice_len, (int64_t)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    const int64_t nvec = (slice_len - head) / 4;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    if (gtid < head) upd(p[gtid]);
    const float4* pv = reinterpret_cast<const float4*>(p + head);
    for (int64_t i = gtid; i < nvec; i += gstride) {
        const float4 v = pv[i];
        upd(v.x);
        upd(v.y);
        upd(v.z);
        upd(v.w);
    }
    for (int64_t i = head + nvec * 4 + gtid; i < slice_len; i += gstride) upd(p[i]);
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    __shared__ float smn[4], smx[4];
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = smn[w] < mn ? smn[w] : mn;
            mx = smx[w] > mx ? smx[w] : mx;
        }
        float* o = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = mn;
        o[1] = mx;
    }
}

// Two instructions that do on their own what the reference spells out in several (probed on gfx950: profiles/r05_cvt_pk_u8_probe.txt):
//   * v_cvt_pk_u8_f32 rounds to nearest EVEN and saturates to [0, 255] (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, 255.5 and
//     +inf -> 255, negative values and NaN -> 0): _mm256_round_ps(.., NEAREST) + the clamp + the pack in one -- no rintf in front;
//   * v_max_f32(x, +0) returns +0 for x = -0, for negative x and for NaN: `if x > 0 { x } else { 0 }` (ReLU) bit for bit.
__device__ __forceinline__ float relu0(float v) { return __builtin_fmaxf(v, 0.0f); }

// avx/quantization.rs:134-140: range -> {scale, zero point, 1/scale}
__device__ __forceinline__ QParams make_qparams(float mn, float mx) {
    const float adjusted_max = mx > 0.0f ? mx : 0.0f;
    const float adjusted_min = mn < 0.0f ? mn : 0.0f;
    float range = adjusted_max - adjusted_min;
    if (!(range > 1e-5f)) range = 1e-5f;
    const float scale = range / 255.0f;
    float z = roundf(-adjusted_min / scale);  // f32::round (half away from zero)
    z = z < 0.0f ? 0.0f : (z > 255.0f ? 255.0f : z);
    QParams q;
    q.scale = scale;
    q.zp = z;
    q.inv_scale = 1.0f / scale;
    q.zp_i = (int)z;
    return q;
}

__global__ void qparams_kernel(const float* __restrict__ partial, int nblocks, QParams* __restrict__ prm,
                               float* __restrict__ scale_out, float* __restrict__ zp_out, unsigned* __restrict__ zero_slice = nullptr) {
    const int s = blockIdx.x;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    for (int i = threadIdx.x; i < nblocks; i += 64) {
        const float a = partial[((int64_t)s * nblocks + i) * 2], b = partial[((int64_t)s * nblocks + i) * 2 + 1];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (threadIdx.x == 0) {
        const QParams q = make_qparams(mn, mx);
        prm[s] = q;
        if (scale_out) scale_out[s] = q.scale;
        if (zp_out) zp_out[s] = q.zp;
        if (zero_slice) zero_slice[s] = 0u;  // the per-slice maxima a feed-forward block's range pass adds into
    }
}

__device__ __forceinline__ float quant_one(float v, const QParams& q, bool simd_body) {
    float r = simd_body ? rintf(__builtin_fmaf(v, q.inv_scale, q.zp))  // _mm256_fmadd_ps + round-to-nearest-even
                        : roundf(v * q.inv_scale + q.zp);               // scalar remainder: two roundings, half away
    return r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
}

// ------------------------------------------------------------------------------------------ 2. rows -> i8
// MODE 0: dynamic quantisation with prm[row / m] -- prm[row_seg[row]] for a packed batch of unequal segments, whose parameters the
//         pairs are partial[row_seg[row]][nblk] -- (fused linear: SIMD body = first k&~7 elements of EACH ROW)
// MODE 1: the input already holds u8 values as f32 (mat_mul_integer): q = sat_u8(round-nearest-even(x))
// One wave per row; writes q-128 as i8 into [rows][kp] (zero padded = contributes 0) and the exact sum of (q-128).
// MODE 0 with `partial` != NULL: the slice's {scale, zp} are derived here from the min/max partials (every wave
// repeats the same few-hundred-element reduction, which is cheaper than a separate launch) and the first row of each
// slice publishes them to prm[] for the GEMM epilogue.
template <int MODE, bool PREFETCH = false>
__global__ __launch_bounds__(256) void qrows_kernel(const float* __restrict__ x, int64_t rows, int k, int kp, int m,
                                                    QParams* __restrict__ prm, int8_t* __restrict__ aq,
                                                    int* __restrict__ row_sums, const float* __restrict__ partial,
                                                    int nblk, unsigned* __restrict__ zero_slice = nullptr,
                                                    int* __restrict__ zero_rows = nullptr,
                                                    const int* __restrict__ row_seg = nullptr /* packed batch: row -> segment (= slice) */) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    // side job for the fused two-layer form (lele_hip_fused_ffn_quantized): clear the accumulators its GEMM passes add into --
    // one per slice (the hidden layer's maximum) and one per row (the hidden layer's i8 row sums)
    if (lane == 0) {
        if (zero_rows) zero_rows[row] = 0;
        if (zero_slice && row % m == 0) zero_slice[row / m] = 0u;
    }
    // PREFETCH (few rows: the launch is latency-bound): the row's elements are requested FIRST (up to 8 x 16 bytes per lane,
    // K <= 2048), so that they travel while the range partials are fetched and reduced below -- two dependent round trips
    // become one.  With many rows the streaming loop is better (more waves in flight per SIMD): +3 % on the batched case.
    constexpr int MAXC = 8;
    const float* xrow = x + row * k;
    const bool fast = PREFETCH && (k & 3) == 0 && k >= 4 && (((uintptr_t)x & 15) == 0) && kp <= 256 * MAXC;
    const int nch = (kp + 255) / 256;
    float4 pre[MAXC];
    if (fast) {
#pragma unroll
        for (int u = 0; u < MAXC; ++u)
            if (u < nch) {  // uniform
                const int c = lane * 4 + 256 * u;
                pre[u] = *reinterpret_cast<const float4*>(xrow + (c < k ? c : k - 4));
            }
    }
    QParams q;
    if (MODE == 0) {
        const int64_t slice = row_seg ? row_seg[row] : row / m;
        if (partial) {
            float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
            // {min, max} pairs as 8-byte loads, all of a trip's loads in flight together (clamped index: a repeated pair changes
            // nothing); a one-pair-per-trip loop exposed one L2 round trip per 64 pairs -- 4 us for the 504 row pairs of a LayerNorm
            const float2* pp = reinterpret_cast<const float2*>(partial) + slice * nblk;
            auto sweep = [&](int i0, auto unroll) {
                constexpr int U = decltype(unroll)::value;
                float2 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = i0 + lane + 64 * u;
                    v[u] = pp[idx < nblk ? idx : nblk - 1];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    mn = v[u].x < mn ? v[u].x : mn;
                    mx = v[u].y > mx ? v[u].y : mx;
                }
            };
            if (nblk <= 256) {
                sweep(0, std::integral_constant<int, 4>());
            } else {  // up to 1024 pairs (a GEMM's per-workgroup pairs, a LayerNorm's rows) per trip: one round trip, not four
                for (int i0 = 0; i0 < nblk; i0 += 1024) sweep(i0, std::integral_constant<int, 16>());
            }
            // min / max over the wave on the DPP / permlane network (lane_ops.h; order-independent, exact)
            mn = wave_allreduce64(mn, [](float cur, float a) { return a < cur ? a : cur; });
            mx = wave_allreduce64(mx, [](float cur, float a) { return a > cur ? a : cur; });
            q = make_qparams(mn, mx);
            // the slice's first row publishes (a packed batch: the first row of its segment)
            const bool first = row_seg ? (row == 0 || row_seg[row - 1] != (int)slice) : row == slice * m;
            if (lane == 0 && first) prm[slice] = q;
        } else {
            q = prm[slice];
        }
    }
    const float* xr = x + row * k;
    int8_t* dst = aq + row * kp;
    const int simd_k = k & ~7;
    const bool vec4 = (k & 3) == 0 && (((uintptr_t)x & 15) == 0);  // every row start is then 16-byte aligned
    int sum = 0;
    if (fast) {
        unsigned usum = 0;  // sum of q over the chunks quantised the short way
        int nfast = 0;
#pragma unroll
        for (int u = 0; u < MAXC; ++u)
            if (u < nch) {
                const int c = lane * 4 + 256 * u;
                if (MODE == 0 && c + 3 < simd_k) {
                    // four elements inside the SIMD body: fma, v_cvt_pk_u8_f32 (rounds to nearest even, saturates to [0, 255] = the
                    // clamp, and packs); per four elements one xor 0x80808080 (q - 128 as i8) and one v_sad_u8 (their sum)
                    unsigned pk = 0;
                    pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(pre[u].x, q.inv_scale, q.zp), 0, pk);
                    pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(pre[u].y, q.inv_scale, q.zp), 1, pk);
                    pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(pre[u].z, q.inv_scale, q.zp), 2, pk);
                    pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(pre[u].w, q.inv_scale, q.zp), 3, pk);
                    usum = __builtin_amdgcn_sad_u8(pk, 0u, usum);
                    nfast += 4;
                    *reinterpret_cast<unsigned*>(dst + c) = pk ^ 0x80808080u;
                } else if (c < kp) {
                    const float xv[4] = {pre[u].x, pre[u].y, pre[u].z, pre[u].w};
                    int packed = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kk = c + e;
                        int v = 0;
                        if (kk < k) {
                            float qf;
                            if (MODE == 0)
                                qf = quant_one(xv[e], q, kk < simd_k);
                            else {
                                const float r = rintf(xv[e]);
                                qf = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
                            }
                            v = (int)qf - 128;
                            sum += v;
                        }
                        packed |= (v & 0xff) << (8 * e);
                    }
                    *reinterpret_cast<int*>(dst + c) = packed;
                }
            }
        sum += (int)usum - 128 * nfast;
    } else
    for (int c = lane * 4; c < kp; c += 256) {
        float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec4 && c + 3 < k) {
            const float4 v = *reinterpret_cast<const float4*>(xr + c);
            xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = xr[c + e < k ? c + e : k - 1];
        }
        int packed = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = c + e;
            int v = 0;
            if (kk < k) {
                float qf;
                if (MODE == 0)
                    qf = quant_one(xv[e], q, kk < simd_k);
                else {
                    const float r = rintf(xv[e]);
                    qf = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
                }
                v = (int)qf - 128;
                sum += v;
            }
            packed |= (v & 0xff) << (8 * e);
        }
        *reinterpret_cast<int*>(dst + c) = packed;
    }
    sum = wave_sum_i32(sum);
    if (lane == 0) row_sums[row] = sum;
}

// unfused DynamicQuantizeLinear: y (u8 values as f32), body = first len&~7 elements of the FLAT tensor
__global__ void dq_apply_kernel(const float* __restrict__ x, int64_t len, const QParams* __restrict__ prm,
                                float* __restrict__ y) {
    const QParams q = prm[0];
    const int64_t simd_end = (len / 8) * 8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = quant_one(x[i], q, i < simd_end);
}

// ------------------------------------------------------------------------------------------ weights -> i8 [N][Kp]
// grid (64-column groups, 64-byte chunks of kp), 256 threads: a 64 x 64 tile is read coalesced along n (16 rows per thread, all
// loads in flight), centred, turned in LDS and written as 16-byte pieces of the [N][Kp] rows; column sums by atomicAdd on zeroed
// sums (a thread per column walking all of k took 240-410 us per matrix: ~100 ms of a SenseVoice-shaped model's first forward)
__global__ __launch_bounds__(256) void wpack_kernel(const float* __restrict__ w /*[K][N]*/, int k, int n, int kp, int8_t* __restrict__ wt,
                                                    int* __restrict__ col_sums) {
    __shared__ __attribute__((aligned(16))) int8_t s_t[64][80];  // [column][k], 16 bytes of padding per row
    __shared__ int s_part[4][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int j = j0 + c, jc = j < n ? j : n - 1;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int kk = k0 + q * 16 + e;
        v[e] = w[(int64_t)(kk < k ? kk : k - 1) * n + jc];
    }
    int sum = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        int val = 0;
        if (k0 + q * 16 + e < k) {
            const float r = rintf(v[e]);  // cvtps + saturating packs (transpose_b_from_f32_avx2)
            val = (r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r)) - 128;  // == u8 ^ 0x80 read as i8
            sum += val;
        }
        s_t[c][q * 16 + e] = (int8_t)val;
    }
    s_part[q][c] = sum;
    __syncthreads();
    if (q == 0 && j < n) atomicAdd(&col_sums[j], s_part[0][c] + s_part[1][c] + s_part[2][c] + s_part[3][c]);
    const int cc = threadIdx.x >> 2, seg = threadIdx.x & 3;
    if (j0 + cc < n && k0 + 16 * seg < kp)  // kp is a multiple of 16: a piece is whole or absent
        *reinterpret_cast<v4i*>(wt + (int64_t)(j0 + cc) * kp + k0 + 16 * seg) = *reinterpret_cast<const v4i*>(&s_t[cc][16 * seg]);
}

// ------------------------------------------------------------------------------------------ 3. i8 GEMM
// C[row][col] = sum_k A'[row][k] * B'[col][k]   (A' = q-128, B' = w-128, both [rows][kp] with k contiguous)
// Tile BM x BN, K step 64 bytes; LDS rows of 64 B + 16 B pad (same bank argument as the f32 core: 5*row mod 16).
// Lane l feeds the two MFMA steps of a K tile with bytes [32*(l>>5), +16) and [32*(l>>5)+16, +16) of its row, for A
// and B alike, so the hardware's internal k order is irrelevant (it pairs like with like).
struct IgemmEpi {
    float* out;
    int64_t rows, n;
    int m;  // rows per batch slice
    int k;
    const int* row_sums;  // sum_k (q-128) per row
    const int* col_sums;  // sum_k (w-128) per column
    const QParams* prm;   // per slice (dynamic) or NULL
    int zp_a_fixed, zp_b;
    const float* wscale;  // may be NULL
    int wscale_len;
    const float* bias;  // may be NULL
    int relu;
    // residual operands [rows][n] added after bias / ReLU, in this order: ((lin + res1) + res2) -- the Add nodes that follow
    // a projection in a transformer block, folded into its store (lele_hip_fused_quantized_linear_residual)
    const float* res1 = nullptr;
    const float* res2 = nullptr;
    float* blockstat = nullptr;  // small-problem kernel: one {min, max} pair per workgroup (common.h, LeleBuf::rowstat)
    int flags = 0;               // developer A/B switches (LELE_HIP_IGEMM_FLAGS): 1 = column terms after the K loop, 2 = previous epilogue
    // the fused two-layer form (igemm_kernel's EM = 1 / 2 passes, see lele_hip_fused_ffn_quantized)
    unsigned* slice_max = nullptr;  // per slice: bits of max(result) (ReLU results are >= 0: unsigned order = float order)
    int8_t* q_out = nullptr;        // EM 2: the result quantised with its slice's range, as q - 128, [rows][n]
    int* q_rowsum = nullptr;        // EM 2: sum over the row of (q - 128), accumulated over column blocks
    QParams* q_prm = nullptr;       // EM 2: the slices' parameters, published for the next GEMM's epilogue
    const int* row_seg = nullptr;   // packed batch (lele_hip_fused_quantized_linear_segments): row -> segment, the slice of prm[]
    unsigned long long* arg_keys = nullptr;  // EM 3 / 4: [column tiles][rows], a tile's best argmax_key(value, column) per row (plain stores)
    float* arg_sums = nullptr;  // EM 4: [column tiles][rows], sum over the tile's columns of exp(value - the tile's maximum) (plain stores)
    int topk = 0;               // EM 5: keys kept per (row, column tile), 1 .. 8; arg_keys is [column tiles][topk][rows] then
    // EM 6 (the listed columns' values, igemm_head.h) adds no field: it reads three that no head uses, so that the kernel's argument
    // block -- and with it the code of every other mode -- stays what it was.  `out`: [rows][topk] values (plain stores, one lane a
    // (row, slot)); `topk`: the listed columns a row; `q_rowsum`: [n], a column's slot or -1.
    __device__ __forceinline__ float* at_out() const { return out; }
    __device__ __forceinline__ const int* at_slot() const { return q_rowsum; }
    __device__ __forceinline__ int at_ncols() const { return topk; }
    // Everything that depends only on the row (slice parameters, row-sum term, output row pointer) or only on the
    // column (column sum, weight scale, bias) is computed once per row / column of a thread's tile, not per element.
    struct RowCtx {
        int ca, rterm;
        float dyn_scale;
        float* orow;
    };
    struct ColCtx {
        int colsum;
        float ws, bias;
    };
    __device__ __forceinline__ RowCtx row_ctx(int64_t row) const {
        int zp_a = zp_a_fixed;
        float ds = 1.0f;
        if (prm) {
            const QParams q = prm[row_seg ? (unsigned)row_seg[row] : (rows == m ? 0u : (unsigned)row / (unsigned)m)];
            zp_a = q.zp_i;
            ds = q.scale;
        }
        // sum (q - zp_a)(w - zp_b) with q = q'+128, w = w'+128  (exact in i32, as the reference's wrapping algebra)
        const int ca = 128 - zp_a, cb = 128 - zp_b;
        return RowCtx{ca, cb * row_sums[row] + k * ca * cb, ds, out + row * n};
    }
    __device__ __forceinline__ ColCtx col_ctx(int col) const {
        ColCtx c{0, 1.0f, 0.0f};
        col = col < n ? col : (int)n - 1;  // clamped: loads stay unconditional, out-of-range columns are never stored
        c.colsum = col_sums[col];
        if (wscale) c.ws = wscale_len <= 1 ? wscale[0] : wscale[col];
        if (bias) c.bias = bias[col];
        return c;
    }
    __device__ __forceinline__ float value(const RowCtx& r, const ColCtx& c, int acc) const {
        const int total = acc + r.rterm + r.ca * c.colsum;
        float vf = (float)total;  // _mm256_cvtepi32_ps
        // combined_scale[j] = dyn_scale * weight_scale[j], then one mul (dyn_scale is 1.0 when there is no dynamic range)
        if (wscale) vf = vf * (r.dyn_scale * c.ws);
        if (bias) vf = vf + c.bias;
        if (relu) vf = relu0(vf);
        return vf;
    }
    // the same value with the zero-point product on the 24-bit multiplier (full rate): |128 - zp_a| <= 128 and a column sum of
    // at most 2^23 (K <= 65536) are exact there
    __device__ __forceinline__ float value24(const RowCtx& r, const ColCtx& c, int acc) const {
        const int total = acc + r.rterm + __mul24(r.ca, c.colsum);
        float vf = (float)total;
        if (wscale) vf = vf * (r.dyn_scale * c.ws);
        if (bias) vf = vf + c.bias;
        if (relu) vf = relu0(vf);
        return vf;
    }
    __device__ __forceinline__ void store(const RowCtx& r, const ColCtx& c, int col, int acc) const { r.orow[col] = value(r, c, acc); }
    // with residuals: the caller has loaded them (unconditionally, from clamped coordinates) before any store
    __device__ __forceinline__ float value_res(const RowCtx& r, const ColCtx& c, int acc, float r1, float r2) const {
        float vf = value(r, c, acc) + r1;
        if (res2) vf = vf + r2;
        return vf;
    }
    __device__ __forceinline__ void store_res(const RowCtx& r, const ColCtx& c, int col, int acc, float r1, float r2) const {
        r.orow[col] = value_res(r, c, acc, r1, r2);
    }
};

}  // namespace
#include "igemm_head.h"
namespace {

// EM (epilogue mode) 0: the result as f32.  EM 1 / 2 are the two passes of the fused two-layer form, where the f32 result (the
// hidden layer of a feed-forward block, 45 MB per configs[3] shard) never exists in HBM -- recomputing the product costs ~5 us of
// matrix-core time against ~30 us of traffic for writing it and reading it twice:
//   EM 1: only the per-slice maximum of the (ReLU) result, by atomic max into epi.slice_max;
//   EM 2: the result again, quantised with the slice's now-known range exactly as qrows_kernel would quantise the stored f32
//         (SIMD body: rint(fma(v, 1/scale, zp)), saturated), written as i8 with its row sums -- what the next GEMM consumes.
// EM 3 / 4 / 5 / 6 are the decode heads (ids, ids with log-probabilities, the k best, listed columns): head_epilogue, igemm_head.h, where the kernel is
// declared with its default arguments (OCC = 1, EM = 0).
template <int BM, int BN, int WM, int WN, int BKB /* bytes of K per LDS tile: 64 or 128 */, int OCC, int EM>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(OCC))) void igemm_kernel(const int8_t* __restrict__ a, const int8_t* __restrict__ b,
                                                            int64_t rows, int n, int kp, int64_t b_batch_stride,
                                                            int m_per_batch, IgemmEpi epi) {
    constexpr int NT = WM * WN * 64;
    constexpr int PITCH = BKB + 16;  // bytes (80 / 144: 16-B aligned rows, 16 distinct bank slots per 16-lane group)
    constexpr int CQ = BKB / 16;     // 16-B chunks per tile row
    constexpr int TMT = BM / WM / 32, TNT = BN / WN / 32;
    constexpr int ASLOTS = (BM * CQ + NT - 1) / NT, BSLOTS = (BN * CQ + NT - 1) / NT;  // 16-B chunks per thread
    extern __shared__ __attribute__((aligned(16))) char igemm_lds[];  // As[2][BM*PITCH] then Bs[2][BN*PITCH]
    char(*As)[BM * PITCH] = reinterpret_cast<char(*)[BM * PITCH]>(igemm_lds);
    char(*Bs)[BN * PITCH] = reinterpret_cast<char(*)[BN * PITCH]>(igemm_lds + 2 * BM * PITCH);
    __shared__ int s_ca[BM], s_rterm[BM];
    __shared__ float s_ds[BM];
    __shared__ unsigned s_mx[2];
    __shared__ QParams s_q[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    unsigned tx, ty, tz;
    gemm::tile_coords(tx, ty, tz);  // XCD-aware order (gemm_core.h)
    const int64_t m0 = (int64_t)ty * BM;
    // EM 1 / 2 (m >= BM): the tile's rows below `split` belong to slice s0, the rest to slice s0 + 1
    const int s0 = (EM == 1 || EM == 2) ? (int)(m0 / epi.m) : 0;
    const int split = (EM == 1 || EM == 2) ? (int)(((int64_t)s0 + 1) * epi.m - m0) : 0;
    if (EM == 1 && tid < 2) s_mx[tid] = 0u;
    if (EM == 2 && tid < 2) {
        const int64_t nslices = epi.rows / epi.m;
        const int64_t sl = s0 + tid < nslices ? s0 + tid : nslices - 1;
        s_q[tid] = make_qparams(0.0f, __uint_as_float(epi.slice_max[sl]));
    }
    // per-row epilogue terms: fetched once per block up front (clamped, unconditional -- their latency hides behind
    // the K loop) instead of per element behind a bounds branch, which serialises one global load per row
    for (int t = tid; t < BM; t += NT) {
        const int64_t r = m0 + t < rows ? m0 + t : rows - 1;
        const IgemmEpi::RowCtx rc = epi.row_ctx(r);
        s_ca[t] = rc.ca;
        s_rterm[t] = rc.rterm;
        s_ds[t] = rc.dyn_scale;
    }
    const int n0 = tx * BN;
    const int hv = lane >> 5, l31 = lane & 31;
    // un-batched weights: b_batch_stride == 0; batched B (mat_mul_integer with batch_b > 1): slice = row block / m
    const int8_t* bb = b + (b_batch_stride ? (m0 / m_per_batch) * b_batch_stride : 0);

    v4i ra[ASLOTS], rb[BSLOTS];
    const v4i zero4 = {0, 0, 0, 0};
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < ASLOTS; ++i) {
            const int s = tid + i * NT, row = s / CQ, kq = s % CQ;
            if (s < BM * CQ) {
                const int64_t r = m0 + row;
                const int kb = k0 + 16 * kq;
                ra[i] = (r < rows && kb < kp) ? *reinterpret_cast<const v4i*>(a + r * kp + kb) : zero4;
            }
        }
#pragma unroll
        for (int i = 0; i < BSLOTS; ++i) {
            const int s = tid + i * NT, row = s / CQ, kq = s % CQ;
            if (s < BN * CQ) {
                const int c = n0 + row;
                const int kb = k0 + 16 * kq;
                rb[i] = (c < n && kb < kp) ? *reinterpret_cast<const v4i*>(bb + (int64_t)c * kp + kb) : zero4;
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < ASLOTS; ++i) {
            const int s = tid + i * NT;
            if (s < BM * CQ) *reinterpret_cast<v4i*>(&As[buf][(s / CQ) * PITCH + 16 * (s % CQ)]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BSLOTS; ++i) {
            const int s = tid + i * NT;
            if (s < BN * CQ) *reinterpret_cast<v4i*>(&Bs[buf][(s / CQ) * PITCH + 16 * (s % CQ)]) = rb[i];
        }
    };
    v16i acc[TMT][TNT];
#pragma unroll
    for (int i = 0; i < TMT; ++i)
#pragma unroll
        for (int j = 0; j < TNT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    // the tiles' column terms (column sum, weight scale, bias): requested before the K loop and pinned there -- fetched after it
    // every block would wait one full memory round trip with nothing else to do
    IgemmEpi::ColCtx cc[TNT];
    int cols[TNT];
#pragma unroll
    for (int j = 0; j < TNT; ++j) cols[j] = n0 + wn * TNT * 32 + j * 32 + l31;
    if (!(epi.flags & 1)) {
#pragma unroll
        for (int j = 0; j < TNT; ++j) cc[j] = epi.col_ctx(cols[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
    const int nk = (kp + BKB - 1) / BKB;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gload((kt + 1) * BKB);
#pragma unroll
        for (int sub = 0; sub < BKB / 64; ++sub) {  // 64 bytes of K per sub-step (two MFMA steps)
            v4i fa[TMT][2], fb[TNT][2];
#pragma unroll
            for (int i = 0; i < TMT; ++i) {
                const char* src = &As[cur][(wm * TMT * 32 + i * 32 + l31) * PITCH + sub * 64 + 32 * hv];
                fa[i][0] = *reinterpret_cast<const v4i*>(src);
                fa[i][1] = *reinterpret_cast<const v4i*>(src + 16);
            }
#pragma unroll
            for (int j = 0; j < TNT; ++j) {
                const char* src = &Bs[cur][(wn * TNT * 32 + j * 32 + l31) * PITCH + sub * 64 + 32 * hv];
                fb[j][0] = *reinterpret_cast<const v4i*>(src);
                fb[j][1] = *reinterpret_cast<const v4i*>(src + 16);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < TMT; ++i)
#pragma unroll
                    for (int j = 0; j < TNT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
    }
    if (epi.flags & 1) {
#pragma unroll
        for (int j = 0; j < TNT; ++j) cc[j] = epi.col_ctx(cols[j]);
    }
    if constexpr (EM == 1) {
        const int rows_here = (int)(rows - m0 < BM ? rows - m0 : BM);
        float mx0 = 0.0f, mx1 = 0.0f;  // ReLU: every value is >= 0, NaN becomes 0
#pragma unroll
        for (int i = 0; i < TMT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wm * TMT * 32 + i * 32 + 4 * hv + (r & 3) + 8 * (r >> 2);
                const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], nullptr};
#pragma unroll
                for (int j = 0; j < TNT; ++j) {
                    float v = epi.value24(rc, cc[j], acc[i][j][r]);
                    v = (lr < rows_here && cols[j] < n) ? v : 0.0f;
                    if (lr < split) mx0 = fmaxf(mx0, v);
                    else mx1 = fmaxf(mx1, v);
                }
            }
        for (int off = 32; off > 0; off >>= 1) {
            mx0 = fmaxf(mx0, __shfl_xor(mx0, off));
            mx1 = fmaxf(mx1, __shfl_xor(mx1, off));
        }
        if (lane == 0) {
            if (mx0 > 0.0f) atomicMax(&s_mx[0], __float_as_uint(mx0));
            if (mx1 > 0.0f) atomicMax(&s_mx[1], __float_as_uint(mx1));
        }
        __syncthreads();
        if (tid < 2 && s_mx[tid]) atomicMax(&epi.slice_max[s0 + tid], s_mx[tid]);
        return;
    }
    if constexpr (EM == 2) {
        static_assert(EM != 2 || BN % 16 == 0, "i8 tile rows are stored in 16-byte chunks");
        const int rows_here = (int)(rows - m0 < BM ? rows - m0 : BM);
        constexpr int QP = BN + 16;   // i8 tile [BM][BN] in the K loop's LDS (its last barrier has passed), rows padded
        char* const qt = igemm_lds;
#pragma unroll
        for (int i = 0; i < TMT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wm * TMT * 32 + i * 32 + 4 * hv + (r & 3) + 8 * (r >> 2);
                const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], nullptr};
                const int which = lr < split ? 0 : 1;
                const float inv = s_q[which].inv_scale, zp = s_q[which].zp;
#pragma unroll
                for (int j = 0; j < TNT; ++j) {
                    const float v = epi.value24(rc, cc[j], acc[i][j][r]);
                    const unsigned q = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(v, inv, zp), 0, 0u);
                    qt[lr * QP + wn * TNT * 32 + j * 32 + l31] = (char)(q ^ 0x80u);
                }
            }
        __syncthreads();
        constexpr int CH = BN / 16;  // 16-byte chunks per tile row: CH consecutive lanes hold one row
        static_assert(EM != 2 || (CH == 8 || CH == 4 || CH == 16), "row-sum reduction over CH lanes");
        for (int c = tid; c < BM * CH; c += NT) {
            const int row = c / CH, c16 = c % CH;
            const v4i w = *reinterpret_cast<const v4i*>(qt + row * QP + 16 * c16);
            unsigned us = __builtin_amdgcn_sad_u8((unsigned)w[0] ^ 0x80808080u, 0u, 0u);
            us = __builtin_amdgcn_sad_u8((unsigned)w[1] ^ 0x80808080u, 0u, us);
            us = __builtin_amdgcn_sad_u8((unsigned)w[2] ^ 0x80808080u, 0u, us);
            us = __builtin_amdgcn_sad_u8((unsigned)w[3] ^ 0x80808080u, 0u, us);
            int part = (int)us - 128 * 16;  // sum of (q - 128) over the chunk
            for (int off = CH / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if (row < rows_here) {
                *reinterpret_cast<v4i*>(epi.q_out + (m0 + row) * (int64_t)n + n0 + 16 * c16) = w;
                if (c16 == 0) atomicAdd(&epi.q_rowsum[m0 + row], part);
            }
        }
        if (tx == 0 && tid < 2 && (tid == 0 || split < rows_here)) epi.q_prm[s0 + tid] = s_q[tid];
        return;
    }
    if constexpr (EM >= 3) {
        head_epilogue<EM, BM, WM, WN, TMT, TNT>(epi, acc, cc, cols, s_ca, s_rterm, s_ds, igemm_lds, tid, wm, wn, tx, m0, rows, n);
        return;
    }
    if (epi.flags & 2) {
    if (epi.res1) {  // residual operands: four rows at a time, their loads issued together before the stores
#pragma unroll
        for (int i = 0; i < TMT; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                float r1[4][TNT], r2[4][TNT];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t row = m0 + wm * TMT * 32 + i * 32 + q + 8 * g4 + 4 * hv;
                    const int64_t rowc = row < rows ? row : rows - 1;
#pragma unroll
                    for (int j = 0; j < TNT; ++j) {
                        const int64_t at = rowc * epi.n + (cols[j] < n ? cols[j] : n - 1);
                        r1[q][j] = epi.res1[at];
                        r2[q][j] = epi.res2 ? epi.res2[at] : 0.0f;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int lr = wm * TMT * 32 + i * 32 + q + 8 * g4 + 4 * hv;
                    const int64_t row = m0 + lr;
                    const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], epi.out + (row < rows ? row : 0) * epi.n};
#pragma unroll
                    for (int j = 0; j < TNT; ++j)
                        if (row < rows && cols[j] < n) epi.store_res(rc, cc[j], cols[j], acc[i][j][q + 4 * g4], r1[q][j], r2[q][j]);
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TMT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = wm * TMT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hv;
            const int64_t row = m0 + lr;
            if (row >= rows) continue;
            const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], epi.out + row * epi.n};
#pragma unroll
            for (int j = 0; j < TNT; ++j)
                if (cols[j] < n) epi.store(rc, cc[j], cols[j], acc[i][j][r]);
        }
        return;
    }
    // epilogue: straight-line per tile -- one uniform 64-bit base + 32-bit element offsets, the zero-point product on the 24-bit
    // multiplier, every residual operand of a tile requested before its first store (loads and stores retire through ONE
    // in-order counter: a load issued after a store cannot be waited for without waiting for the store)
    const int rows_here = (int)(rows - m0 < BM ? rows - m0 : BM);
    float* const obase = epi.out + m0 * (int64_t)n;
    const unsigned nu = (unsigned)n;
    auto epilogue = [&](auto nres_c) {
        constexpr int NRES = decltype(nres_c)::value;
        const float* const r1base = NRES > 0 ? epi.res1 + m0 * (int64_t)n : nullptr;
        const float* const r2base = NRES > 1 ? epi.res2 + m0 * (int64_t)n : nullptr;
#pragma unroll
        for (int i = 0; i < TMT; ++i) {
            const int rbase = wm * TMT * 32 + i * 32 + 4 * hv;
            float r1[NRES > 0 ? 16 : 1][TNT], r2[NRES > 1 ? 16 : 1][TNT];
            if (NRES > 0) {
                const int last = rows_here - 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = rbase + (r & 3) + 8 * (r >> 2);
                    const unsigned rowoff = (unsigned)(lr < last ? lr : last) * nu;
#pragma unroll
                    for (int j = 0; j < TNT; ++j) {
                        const unsigned at = rowoff + (unsigned)(cols[j] < n ? cols[j] : n - 1);
                        r1[r][j] = r1base[at];
                        if (NRES > 1) r2[r][j] = r2base[at];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = rbase + (r & 3) + 8 * (r >> 2);
                const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], nullptr};
                const bool rok = lr < rows_here;
                const unsigned rowoff = (unsigned)lr * nu;
#pragma unroll
                for (int j = 0; j < TNT; ++j) {
                    float v = epi.value24(rc, cc[j], acc[i][j][r]);
                    if (NRES > 0) v = v + r1[r][j];
                    if (NRES > 1) v = v + r2[r][j];
                    if (rok && cols[j] < n) obase[rowoff + (unsigned)cols[j]] = v;
                }
            }
        }
    };
    if (!epi.res1) epilogue(std::integral_constant<int, 0>());
    else if (!epi.res2) epilogue(std::integral_constant<int, 1>());
    else epilogue(std::integral_constant<int, 2>());
}


}  // namespace
#include "igemm_rs.h"
#include "igemm_big.h"
namespace {

// ------------------------------------------------------------------------------------------ fragment-major weights (igemm_rs.h)
// weights [K][N] (u8 values as f32) -> fragment-major i8: block (ct, ks) = columns [32ct, +32) x k [32ks, +32), lane l of the
// block holds column 32ct + (l & 31), k = 32ks + 16(l >> 5) + [0, 16).  One thread per (column, 16-k chunk).
__global__ void wpack_frag_kernel(const float* __restrict__ w, int k, int n, int ks, int nt, int8_t* __restrict__ wf) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(t % (nt * 32));          // column (fast: the reads of a wave are one coalesced row segment)
    const int kc = (int)(t / (nt * 32));         // 16-k chunk
    if (kc >= ks * 2) return;
    int packed[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int kk = kc * 16 + e;
        int v = 0;
        if (kk < k && j < n) {
            const float r = rintf(w[(int64_t)kk * n + j]);  // cvtps + saturating packs (transpose_b_from_f32_avx2)
            const int u = r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r);
            v = u - 128;
        }
        packed[e >> 2] |= (v & 0xff) << (8 * (e & 3));
    }
    const int64_t blk = (int64_t)(j >> 5) * ks + (kc >> 1);
    const int lane = (j & 31) + 32 * (kc & 1);
    v4i o = {packed[0], packed[1], packed[2], packed[3]};
    *reinterpret_cast<v4i*>(wf + (blk * 64 + lane) * 16) = o;
}
// column sums of the centred weights (exact i32): grid (64-column groups, 64-row chunks of k), 256 threads = 4 k-quarters x 64
// columns, 16 rows each with every load in flight at once; the quarters meet in LDS, the chunks by atomicAdd on zeroed sums
// (a thread per column walking all of k took 260 us per weight matrix: 54 ms of a SenseVoice-shaped model's first forward)
__global__ __launch_bounds__(256) void wcolsum_kernel(const float* __restrict__ w, int k, int n, int* __restrict__ col_sums) {
    __shared__ int s_part[4][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c, jc = j < n ? j : n - 1;
    const int k0 = blockIdx.y * 64 + q * 16;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int kk = k0 + e;
        v[e] = w[(int64_t)(kk < k ? kk : k - 1) * n + jc];
    }
    int sum = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float r = rintf(v[e]);
        sum += k0 + e < k ? (r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r)) - 128 : 0;
    }
    s_part[q][c] = sum;
    __syncthreads();
    if (q == 0 && j < n) atomicAdd(&col_sums[j], s_part[0][c] + s_part[1][c] + s_part[2][c] + s_part[3][c]);
}
int launch_wcolsum(LeleCtx* ctx, const float* dw, int k, int n, int* dcs) {
    LELE_HIP_CHECK(hipMemsetAsync(dcs, 0, (size_t)n * 4, ctx->stream));
    hipLaunchKernelGGL(wcolsum_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((k + 63) / 64)), dim3(256), 0, ctx->stream, dw, k, n, dcs);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ host helpers
struct PackedW {
    int8_t* wt;
    int* col_sums;
};

// weights as i8 [N][Kp] | column sums, of `nbatch` matrices: one cached form for declared-immutable weights, packed into the arena per
// call otherwise.  dw is the f32-encoded source on the device; NULL has it uploaded when (and only when) the form is packed.
int packed_weights_of(LeleCtx* ctx, const LeleTensor* w, const float* dw, int64_t nbatch, int k, int n, int kp, PackedW* out) {
    const size_t sums_at = weight_second((size_t)nbatch * n * kp);
    void* d = nullptr;
    LELE_TRY(ctx->weight_form(w, WeightForm::I8Packed, {}, sums_at + (size_t)nbatch * n * 4, &d, [&](void* p) {
        const void* src = dw;
        if (!src) LELE_TRY(ctx->dev_ptr(w, &src));
        int* dcs = (int*)((char*)p + sums_at);
        LELE_HIP_CHECK(hipMemsetAsync(dcs, 0, (size_t)nbatch * n * 4, ctx->stream));
        for (int64_t b = 0; b < nbatch; ++b)
            hipLaunchKernelGGL(wpack_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((kp + 63) / 64)), dim3(256), 0, ctx->stream,
                               (const float*)src + b * (int64_t)k * n, k, n, kp, (int8_t*)p + b * (int64_t)n * kp, dcs + b * n);
        LELE_HIP_CHECK(hipGetLastError());
        return 0;
    }));
    out->wt = (int8_t*)d;
    out->col_sums = (int*)((char*)d + sums_at);
    return 0;
}

// fragment-major packed weights | column sums for the one-pass kernel (cached like PackedW)
struct FragW {
    int8_t* wf;
    int* col_sums;
};
int frag_weights_of(LeleCtx* ctx, const LeleTensor* w, int k, int n, int kp, FragW* out) {
    const int ks = kp / 32, nt = (n + 31) / 32;
    const size_t sums_at = weight_second((size_t)nt * ks * 1024);
    void* d = nullptr;
    LELE_TRY(ctx->weight_form(w, WeightForm::I8Frag, {}, sums_at + (size_t)n * 4, &d, [&](void* p) {
        const void* dw = nullptr;
        LELE_TRY(ctx->dev_ptr(w, &dw));  // the f32-encoded matrix (an immutable one is uploaded and cached as WeightForm::Raw)
        const int64_t threads = (int64_t)nt * 32 * ks * 2;
        hipLaunchKernelGGL(wpack_frag_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const float*)dw, k, n, ks,
                           nt, (int8_t*)p);
        LELE_TRY(launch_wcolsum(ctx, (const float*)dw, k, n, (int*)((char*)p + sums_at)));
        LELE_HIP_CHECK(hipGetLastError());
        return 0;
    }));
    out->wf = (int8_t*)d;
    out->col_sums = (int*)((char*)d + sums_at);
    return 0;
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
// developer switches exist in the lab build only (LELE_HIP_LAB=1 python -m lele_amd.build); the product reads the documented ones
int lab_int(const char* name, int dflt) {
#ifdef LELE_HIP_LAB
    return env_int(name, dflt);
#else
    (void)name;
    return dflt;
#endif
}

// stage stopwatch of the quantised linear (lele_hip_quant_set_profiling): stage = 0 start, 1 after the range pass, 2 after the
// row quantisation, 3 after the GEMM
int qprof_mark(LeleCtx* ctx, int stage) {
    if (!ctx->qprof.on || ctx->capturing) return 0;
    auto& p = ctx->qprof;
    if (stage == 0) {
        if (p.used + 4 > p.ev.size()) {
            for (int i = 0; i < 4; ++i) {
                hipEvent_t e;
                LELE_HIP_CHECK(hipEventCreate(&e));
                p.ev.push_back(e);
            }
        }
        p.used += 4;
    }
    LELE_HIP_CHECK(hipEventRecord(p.ev[p.used - 4 + stage], ctx->stream));
    return 0;
}

// fused != NULL: only the min/max partials are produced (at most 256 per slice); *fused / *fused_nblk receive them and the
// caller's qrows_kernel<0> turns them into parameters -- one launch fewer on the latency-bound path.
int launch_range(LeleCtx* ctx, const float* dx, int64_t slices, int64_t slice_len, QParams* prm, float* scale_out,
                 float* zp_out, const float** fused = nullptr, int* fused_nblk = nullptr) {
    // enough blocks to fill 256 CUs x 4 even for one slice; every thread then streams >= 4 float4
    const int64_t want = (slice_len + 4095) / 4096;
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(1, 1024 / slices), want));  // <= 1024 partial pairs in total; a fused reader scans its slice's (<= 1024) pairs
    void* partial = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)slices * nblk * 8, &partial));
    hipLaunchKernelGGL(qminmax_kernel, dim3(nblk, (unsigned)slices), dim3(256), 0, ctx->stream, dx, slice_len,
                       (float*)partial);
    if (fused) {
        *fused = (const float*)partial;
        *fused_nblk = nblk;
    } else {
        hipLaunchKernelGGL(qparams_kernel, dim3((unsigned)slices), dim3(64), 0, ctx->stream, (const float*)partial, nblk,
                           prm, scale_out, zp_out);
    }
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// *name: what was launched, as lele_hip_last_route reports it (NULL when nothing was, or a lab build's forced tile)
int launch_igemm(LeleCtx* ctx, const int8_t* aq, const int8_t* wt, int64_t rows, int n, int kp, int m_per_batch, const IgemmEpi& epi_in,
                 const char** name) {
    *name = nullptr;
    if (rows == 0 || n == 0) return 0;
    IgemmEpi epi = epi_in;
    epi.flags = lab_int("LELE_HIP_IGEMM_FLAGS", 0);
    LELE_REQUIRE(rows < (int64_t(1) << 31), "quantized GEMM: more than 2^31 rows");
    const int64_t b128 = ((rows + 127) / 128) * ((n + 127) / 128);
    // (the kernels' b_stride stays 0: a batched B is one launch per slice, issued by the caller with rows == m)
#define IGEMM_LAUNCH(BM_, BN_, WM_, WN_, BKB_, OCC_)                                                                         \
    do {                                                                                                                  \
        constexpr size_t lds = (size_t)2 * ((BM_) + (BN_)) * ((BKB_) + 16);                                               \
        auto kern = igemm_kernel<BM_, BN_, WM_, WN_, BKB_, OCC_>;                                                          \
        if (lds > 64 * 1024) LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), (int)lds));               \
        dim3 grid((n + (BN_)-1) / (BN_), (unsigned)((rows + (BM_)-1) / (BM_)));                                           \
        hipLaunchKernelGGL(kern, grid, dim3((WM_) * (WN_) * 64), lds, ctx->stream, aq, wt, rows, n, kp, (int64_t)0,        \
                           m_per_batch, epi);                                                                             \
    } while (0)
    const int64_t b64 = ((rows + 63) / 64) * ((n + 63) / 64);
#ifdef LELE_HIP_LAB
    const int force = lab_int("LELE_HIP_IGEMM_TILE", 0);  // developer override for tile-shape experiments (tools/qlinear_bench.py)
    if (force == 1) IGEMM_LAUNCH(128, 128, 2, 4, 64, 4);
    else if (force == 2) IGEMM_LAUNCH(128, 128, 2, 4, 128, 1);
    else if (force == 3) IGEMM_LAUNCH(256, 128, 4, 2, 64, 2);
    else if (force == 4) IGEMM_LAUNCH(128, 256, 2, 4, 64, 2);
    else if (force == 5) IGEMM_LAUNCH(64, 64, 2, 2, 64, 1);
    else if (force == 6) IGEMM_LAUNCH(128, 128, 2, 2, 64, 2);
    else if (force == 7) IGEMM_LAUNCH(64, 128, 2, 2, 64, 2);
    else if (force == 8) IGEMM_LAUNCH(256, 128, 4, 2, 128, 2);
    else if (force == 9) IGEMM_LAUNCH(128, 128, 2, 4, 64, 6);
    else if (force == 10) IGEMM_LAUNCH(128, 64, 2, 2, 64, 5);
    else if (force == 11) IGEMM_LAUNCH(64, 128, 2, 2, 64, 5);
    else if (force == 12) IGEMM_LAUNCH(128, 128, 2, 2, 64, 4);
    else if (force == 13) IGEMM_LAUNCH(128, 64, 4, 2, 64, 4);
    else if (force == 14) IGEMM_LAUNCH(128, 64, 4, 2, 128, 4);
    else
#endif
    // compute-bound shapes (igemm_big.h): long K in whole 128-byte steps, at least half a chip of 256 x 256 results, 16-byte rows
    if (kp % 128 == 0 && kp >= 1024 && n % 4 == 0 && lab_int("LELE_HIP_IGEMM_BIG", 1) != 0 &&
        rows * kp < (int64_t(1) << 32) && (int64_t)n * kp < (int64_t(1) << 32) &&
        ((rows + 255) / 256) * (((int64_t)n + 255) / 256) * 2 >= (int64_t)ctx->num_cus && ((((uintptr_t)epi.out) | ((uintptr_t)epi.res1) | ((uintptr_t)epi.res2)) & 15) == 0 &&
        !epi.blockstat) {
        dim3 grid((unsigned)((n + 255) / 256), (unsigned)((rows + 255) / 256));
        *name = "igemm.big";
#ifdef LELE_HIP_LAB
        if (lab_int("LELE_HIP_IGEMM_BIG", 1) == 2) {   // (lab) four waves of 128 x 128
            auto kern = igemm_big_kernel<2>;
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), BG_LDS));
            hipLaunchKernelGGL(kern, grid, dim3(256), BG_LDS, ctx->stream, aq, wt, rows, n, kp, epi);
        } else if (lab_int("LELE_HIP_IGEMM_BIG", 1) == 3) {   // (lab) eight waves of 128 x 64, operands through staging registers
            auto kern = igemm_big_kernel<4>;
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), BG_LDS));
            hipLaunchKernelGGL(kern, grid, dim3(512), BG_LDS, ctx->stream, aq, wt, rows, n, kp, epi);
        } else
#endif
        {
            auto kern = igemm_big_kernel<4, true>;
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), BG_LDS));
            hipLaunchKernelGGL(kern, grid, dim3(512), BG_LDS, ctx->stream, aq, wt, rows, n, kp, epi);
        }
    } else if (b64 < 2 * (int64_t)ctx->num_cus) {
        // small problem (SenseVoice at M = 504): 32x32 tiles, K split over the four waves, operands straight from L2
        dim3 grid((unsigned)((n + 31) / 32), (unsigned)((rows + 31) / 32));
        *name = kp <= 512 ? "igemm.small_k4" : "igemm.small_k16";
        if (kp <= 512)
            hipLaunchKernelGGL((gemm::igemm_small_kernel<IgemmEpi, 4>), grid, dim3(256), 0, ctx->stream, aq, wt, rows, n, kp, (int64_t)0,
                               m_per_batch, epi);
        else
            hipLaunchKernelGGL((gemm::igemm_small_kernel<IgemmEpi, 16>), grid, dim3(256), 0, ctx->stream, aq, wt, rows, n, kp, (int64_t)0,
                               m_per_batch, epi);
    } else if (b128 >= 2 * ctx->num_cus) {
        // 128-byte K tiles (74 KB of LDS, 2 workgroups per CU): half as many barriers and twice the bytes in flight per K step.
        // Measured on the configs[3] shard shapes (profiles/r02_qlinear_variants.json): 29.3 / 30.0 / 41.1 us for qkv / ffn1 / ffn2
        // against 32.5 / 32.9 / 48.7 us with 64-byte tiles -- the second, nearly empty round of workgroups costs less than that.
        IGEMM_LAUNCH(128, 128, 2, 4, 128, 1);
        *name = "igemm.t128x128";
    } else if (rows <= 32) {
        IGEMM_LAUNCH(32, 128, 1, 4, 64, 1);
        *name = "igemm.t32x128";
    } else {
        // narrow results over many rows (out projection, second feed-forward layer: N = 512 over a batch of utterances): 128 x 64
        // tiles, eight waves, 128-byte K tiles -- 40.0 us against 45.9 us with 64 x 64 tiles at K = 2048, 16.3 against 16.8 at K = 512.
        // (They always cover the chip here: b64 >= 2 CUs and ceil(rows / 64) <= 2 ceil(rows / 128) give ceil(rows / 128) * ceil(n / 64)
        // >= CUs, so the 64 x 64 tile that once stood behind this one is the lab's LELE_HIP_IGEMM_TILE=5 only.)
        IGEMM_LAUNCH(128, 64, 4, 2, 128, 4);
        *name = "igemm.t128x64";
    }
#undef IGEMM_LAUNCH
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// the two passes of the fused two-layer form over the hidden layer's product (128 x 128 tiles, the big-shape configuration)
int launch_igemm_hidden(LeleCtx* ctx, int em, const int8_t* aq, const int8_t* wt, int64_t rows, int n, int kp, int m, const IgemmEpi& epi) {
    constexpr size_t lds = (size_t)2 * (128 + 128) * (128 + 16);
    const dim3 grid((n + 127) / 128, (unsigned)((rows + 127) / 128));
    auto kern = em == 1 ? igemm_kernel<128, 128, 2, 4, 128, 1, 1> : igemm_kernel<128, 128, 2, 4, 128, 1, 2>;
    LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, ctx->stream, aq, wt, rows, n, kp, (int64_t)0, m, epi);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- register-stationary route (igemm_rs.h): K padded to exactly 512 bytes (2048 inside the feed-forward block), enough 32 x 32 tiles to fill the chip
bool pads_to_512(int64_t k) { return ((k + 31) & ~int64_t(31)) == 512; }
// enough 32 x 32 tiles, 16-byte stores, 32-bit byte offsets into the result.  (Round 3 asked for 8 tiles per CU: below that the
// quantising pass + small-problem GEMM were faster.  With the rows quantised inside the kernel the route needs no pass in front, and
// one 30 s utterance -- 16 row tiles x 48-64 column tiles -- gains 7 % per forward on it: 2 tiles per CU.)
bool rs_enabled(LeleCtx* ctx, int64_t rows, int64_t n, int per_cu = 2) {
    if (env_int("LELE_HIP_IGEMM_RS", 1) == 0) return false;  // documented switch: 0 = the tiled kernels everywhere
    if (n % 4 || rows * n >= (int64_t(1) << 30)) return false;
    const int64_t units = ((rows + 31) / 32) * ((n + 31) / 32);
    return units >= (int64_t)lab_int("LELE_HIP_IGEMM_RS_MIN", per_cu * ctx->num_cus);
}
// the stand-alone linear.  Measured on one configs[3] shard (tools/rs_bench.py, whole op incl. the row quantisation): N = 1536
// 24.9 us against 28.7 us tiled, N = 2048 27.2 against 29.5 -- but N = 512 23.0 against 18.7 (few column tiles: the
// weights-in-registers prologue is not amortised), and a stand-alone K = 2048 linear 54.9 against 41.3 (the fused feed-forward
// block calls the K-split kernel itself, on a hidden layer that is already in fragment order)
// the quantising loaders (igemm_rs.h, FQ): whole 512-element rows read as float4s.  LELE_HIP_IGEMM_RS_FQ=0 (lab build) keeps the
// separate qrows_frag_kernel pass for A/B timing; both give the same bits.
bool rs_fq(int64_t k, const void* dx) { return k == 512 && (((uintptr_t)dx) & 15) == 0 && lab_int("LELE_HIP_IGEMM_RS_FQ", 1) != 0; }
bool rs_fits(LeleCtx* ctx, int64_t rows, int64_t n, int64_t k) { return pads_to_512(k) && n >= lab_int("LELE_HIP_IGEMM_RS_MIN_N", 1024) && rs_enabled(ctx, rows, n); }
// the register-stationary kernels read residuals and write results 16 bytes at a time: a device tensor that does not start on a
// 16-byte boundary (a view into a larger buffer) takes the tiled route instead (host tensors are staged into the aligned arena)
bool rs_aligned(const LeleTensor* t) { return !t || t->mem != LELE_MEM_DEVICE || (((uintptr_t)t->data) & 15) == 0; }
// f32 rows, K <= 512 -> fragment-major i8 [ceil(rows / 32)][16][1024] in the arena (+ row sums unless rs == NULL)
int launch_qrows_frag(LeleCtx* ctx, const float* dx, int64_t rows, int k, int m, QParams* prm, int8_t* af, int* rs, const float* partial,
                      int nblk, unsigned* zero_slice) {
    const int64_t nrt = (rows + 31) / 32;
    // a wave per two rows: 4 tiles' worth of workgroups per tile
    hipLaunchKernelGGL((qrows_frag_kernel<32, 1>), dim3((unsigned)(4 * nrt)), dim3(256), 0, ctx->stream, dx, (unsigned)rows, k, m, prm, af, rs,
                       partial, nblk, zero_slice);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}
// the grid of igemm_rs_kernel: column blocks of 8 tiles x row ranges, one 640 / 768-thread workgroup per CU, all resident at once
void rs_grid(LeleCtx* ctx, int64_t rows, int64_t n, int* ncb, int* nrr) {
    const int nrt = (int)((rows + 31) / 32), nct = (int)((n + 31) / 32);
    *ncb = (nct + 7) / 8;
    *nrr = std::max(1, std::min(nrt, ctx->num_cus / *ncb));
}
// the most slices of m rows a workgroup's row range can touch (FQ: the loaders keep their parameters in a table of RS_MAXSL entries;
// the fused feed-forward block's range pass keeps four maxima a workgroup)
int64_t rs_max_slices(LeleCtx* ctx, int64_t rows, int64_t n, int64_t m) {
    int ncb, nrr;
    rs_grid(ctx, rows, n, &ncb, &nrr);
    const int64_t nrt = (rows + 31) / 32, tiles = (nrt + nrr - 1) / nrr;
    return rows == m ? 1 : (tiles * 32 + m - 2) / m + 1;
}
struct RsFq {  // what the quantising loaders need besides the epilogue's arguments
    const float* x = nullptr;
    const float* partial = nullptr;
    int nblk = 0;
    unsigned* hpart = nullptr;
    unsigned* sync = nullptr;  // EM 3: the row ranges' arrival counters (rs_sync_counters)
};
// EM 3 (igemm_rs.h: both passes of the feed-forward block's first product in one launch, workgroups waiting for their neighbours):
// only where every workgroup of the launch is resident and nothing else of this library can be waiting beside it -- lane 0 of the ONLY
// live context of the device, no side lane in flight, a grid of at most one workgroup per CU, at most RS_NS_BOTH tiles a workgroup --
// and only with counters that exist already or can be made now (not while capturing).  LELE_HIP_FFN_ONE_LAUNCH=0 keeps the two launches.
unsigned* rs_sync_counters(LeleCtx* ctx, int64_t rows, int64_t n) {
    if (env_int("LELE_HIP_FFN_ONE_LAUNCH", 1) == 0) return nullptr;
    int ncb = 0, nrr = 0;
    rs_grid(ctx, rows, n, &ncb, &nrr);
    const int64_t nrt = (rows + 31) / 32, tiles = (nrt + nrr - 1) / nrr;
    if (tiles > RS_NS_BOTH || nrr > 64 || ncb * nrr > ctx->num_cus || n % 256 != 0) return nullptr;
    if (ctx->lane != 0 || ctx->side_lanes || lele::live_contexts(ctx->device) != 1) return nullptr;
    auto it = ctx->rs_sync.find({ncb, nrr});
    if (it != ctx->rs_sync.end()) return it->second;
    if (ctx->capturing) return nullptr;
    void* p = nullptr;
    // 64 counters, then one 8-byte word {launch tag, maximum} per workgroup and slice (4 a workgroup): cleared once, never again
    const size_t bytes = 256 + (size_t)ncb * nrr * 32;
    // cleared ON THE CONTEXT'S STREAM: the stream does not synchronise with the null stream, and the first launch follows at once
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemsetAsync(p, 0, bytes, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        return nullptr;
    }
    ctx->rs_sync[{ncb, nrr}] = (unsigned*)p;
    return (unsigned*)p;
}
int launch_rs(LeleCtx* ctx, int em, const int8_t* af, const int8_t* wf, int64_t rows, int n, int8_t* hid, const IgemmEpi& epi,
              const RsFq& fq = RsFq()) {
    const float* x_f32 = fq.x;
    RsArgs g{af, wf, (unsigned)rows, n, (int)((rows + 31) / 32), (n + 31) / 32, 0, 0, hid, x_f32, fq.partial, fq.nblk, fq.hpart};
    g.sync = fq.sync;
    g.deverr = ctx->deverr_dev;
#ifdef LELE_HIP_LAB
    g.dbg = nullptr;
    g.ablate = lab_int("LELE_HIP_RS_ABLATE", 0);
    if (const char* e = lab_env("LELE_HIP_RS_STAMPS"))  // a device address (tools/rs_stamps.py), optionally for one mode only
        if (lab_int("LELE_HIP_RS_STAMPS_EM", em) == em) g.dbg = (long long*)(uintptr_t)strtoull(e, nullptr, 0);
#endif
    rs_grid(ctx, rows, n, &g.ncb, &g.nrr);
    const dim3 grid((unsigned)(g.ncb * g.nrr));
    const int nres = epi.res1 ? (epi.res2 ? 2 : 1) : 0;
#define LELE_RS(EM_, NRES_, RELU_)                                                                   \
    do {                                                                                             \
        if (x_f32) {                                                                                 \
            auto kern = igemm_rs_kernel<EM_, NRES_, RELU_, true>;                                     \
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), RS_LDS));              \
            hipLaunchKernelGGL(kern, grid, dim3(768), RS_LDS, ctx->stream, g, epi);                   \
        } else {                                                                                     \
            auto kern = igemm_rs_kernel<EM_, NRES_, RELU_>;                                           \
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), RS_LDS));              \
            hipLaunchKernelGGL(kern, grid, dim3(640), RS_LDS, ctx->stream, g, epi);                   \
        }                                                                                            \
    } while (0)
    if (em == 3) {
        LELE_REQUIRE(x_f32 && fq.sync && fq.hpart, "launch_rs: the one-launch form needs the quantising loaders and its counters");
        auto kern = igemm_rs_kernel<3, 0, true, true>;
        LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), RS_LDS_BOTH));
        hipLaunchKernelGGL(kern, grid, dim3(768), RS_LDS_BOTH, ctx->stream, g, epi);
    } else if (em == 1) LELE_RS(1, 0, true);
    else if (em == 2) LELE_RS(2, 0, true);
    else if (epi.relu) {
        if (nres == 0) LELE_RS(0, 0, true);
        else if (nres == 1) LELE_RS(0, 1, true);
        else LELE_RS(0, 2, true);
    } else {
        if (nres == 0) LELE_RS(0, 0, false);
        else if (nres == 1) LELE_RS(0, 1, false);
        else LELE_RS(0, 2, false);
    }
#undef LELE_RS
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}
// K = 512, N <= 512: one workgroup a row tile, all columns (igemm_as_kernel)
bool as_fits(LeleCtx* ctx, int64_t rows, int64_t n, int64_t k, const void* dx) {
    if (env_int("LELE_HIP_IGEMM_RS", 1) == 0 || lab_int("LELE_HIP_IGEMM_AS", 1) == 0) return false;
    return k == 512 && n <= 512 && n % 4 == 0 && n >= 4 && rows * n < (int64_t(1) << 30) && (((uintptr_t)dx) & 15) == 0 &&
           rows >= (int64_t)lab_int("LELE_HIP_IGEMM_AS_MIN_ROWS", 256);
}
// a batch: one workgroup a row tile, all (up to 16) column tiles, two a wave; few row tiles (one utterance: 16): 8 or 4 column
// tiles a workgroup, one a wave, so that the grid still covers a good part of the chip
bool as_two(LeleCtx* ctx, int64_t rows, int n) {
    const int64_t nrt = (rows + 31) / 32;
    return nrt * 3 >= (int64_t)ctx->num_cus || (n + 31) / 32 <= 4 || lab_int("LELE_HIP_IGEMM_AS_TPW", 0) == 16;
}
struct AsLn {  // the LayerNorm behind the projection, in the same launch (n == 512, whole rows in a workgroup)
    const float* g = nullptr;
    const float* b = nullptr;
    float eps = 0.0f;
    float* out = nullptr;
    float* rowstat = nullptr;
    // + the FSMN memory block as res1, computed in the kernel (k = 11)
    const float* fs_x = nullptr;
    int fs_pitch = 0;
    const float* fs_w = nullptr;
    const float* fs_b = nullptr;
    int fs_pl = 0;
};
int launch_as(LeleCtx* ctx, const float* x, const int8_t* wf, int64_t rows, int n, const float* partial, int nblk, QParams* prm,
              const IgemmEpi& epi, const AsLn* ln, const char** name) {
    AsArgs g{x, wf, (unsigned)rows, n, (n + 31) / 32, partial, nblk, prm, 16};
    const int64_t nrt = (rows + 31) / 32;
    const bool two = as_two(ctx, rows, n);
    if (!two) g.tpw = lab_int("LELE_HIP_IGEMM_AS_TPW", nrt * 6 >= (int64_t)ctx->num_cus ? 8 : 4);
    *name = two ? "as.two" : g.tpw == 8 ? "as.tpw8" : g.tpw == 4 ? "as.tpw4" : nullptr;  // (no name: a lab build's LELE_HIP_IGEMM_AS_TPW)
    const dim3 grid((unsigned)nrt, two ? 1u : (unsigned)((g.nct + g.tpw - 1) / g.tpw));
    const int nres = epi.res1 ? (epi.res2 ? 2 : 1) : 0;
    if (ln) {
        LELE_REQUIRE(two && n == 512 && !epi.relu, "launch_as: the LayerNorm epilogue needs whole 512-wide rows in a workgroup");
        g.ln_g = ln->g, g.ln_b = ln->b, g.ln_eps = ln->eps, g.ln_out = ln->out, g.ln_rowstat = ln->rowstat;
#define LELE_AS_LN(NRES_)                                                                              \
    do {                                                                                               \
        auto kern = igemm_as_kernel<NRES_, false, true, true>;                                          \
        LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), AS_LN_LDS));                 \
        hipLaunchKernelGGL(kern, grid, dim3(512), AS_LN_LDS, ctx->stream, g, epi);                      \
    } while (0)
        if (ln->fs_x) {   // res1 is the memory block of ln->fs_x (epi.res1 is not read), epi.res2 the optional second residual
            g.fs_x = ln->fs_x, g.fs_pitch = ln->fs_pitch, g.fs_w = ln->fs_w, g.fs_b = ln->fs_b;
#define LELE_AS_FS(NRES_)                                                                              \
    do {                                                                                               \
        auto kern = igemm_as_kernel<NRES_, false, true, true, 11>;                                      \
        LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), as_fs_lds(11)));             \
        hipLaunchKernelGGL(kern, grid, dim3(512), as_fs_lds(11), ctx->stream, g, epi);                  \
    } while (0)
            if (epi.res2) LELE_AS_FS(2);
            else LELE_AS_FS(1);
#undef LELE_AS_FS
            LELE_HIP_CHECK(hipGetLastError());
            return 0;
        }
        if (nres == 0) LELE_AS_LN(0);
        else if (nres == 1) LELE_AS_LN(1);
        else LELE_AS_LN(2);
#undef LELE_AS_LN
        LELE_HIP_CHECK(hipGetLastError());
        return 0;
    }
#define LELE_AS(NRES_, RELU_)                                                                                     \
    do {                                                                                                          \
        if (two) hipLaunchKernelGGL((igemm_as_kernel<NRES_, RELU_, true>), grid, dim3(512), 0, ctx->stream, g, epi);   \
        else hipLaunchKernelGGL((igemm_as_kernel<NRES_, RELU_, false>), grid, dim3(512), 0, ctx->stream, g, epi);     \
    } while (0)
    if (epi.relu) {
        if (nres == 0) LELE_AS(0, true);
        else if (nres == 1) LELE_AS(1, true);
        else LELE_AS(2, true);
    } else {
        if (nres == 0) LELE_AS(0, false);
        else if (nres == 1) LELE_AS(1, false);
        else LELE_AS(2, false);
    }
#undef LELE_AS
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_rs_ks4(LeleCtx* ctx, const int8_t* af, const int8_t* wf, int64_t rows, int n, const IgemmEpi& epi, const char** name) {
    *name = "rs.ks4";
    RsArgs g{af, wf, (unsigned)rows, n, (int)((rows + 31) / 32), (n + 31) / 32, 0, 0, nullptr};
#ifdef LELE_HIP_LAB
    g.dbg = nullptr;
    g.ablate = 0;
#endif
    g.nrr = std::max(1, std::min(g.nrt, 2 * ctx->num_cus / g.nct));  // two 256-thread workgroups per CU
    const dim3 grid((unsigned)(g.nct * g.nrr));
    const int nres = epi.res1 ? (epi.res2 ? 2 : 1) : 0;
    if (nres == 0) hipLaunchKernelGGL(igemm_rs_ks4_kernel<0>, grid, dim3(256), 0, ctx->stream, g, epi);
    else if (nres == 1) hipLaunchKernelGGL(igemm_rs_ks4_kernel<1>, grid, dim3(256), 0, ctx->stream, g, epi);
    else hipLaunchKernelGGL(igemm_rs_ks4_kernel<2>, grid, dim3(256), 0, ctx->stream, g, epi);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// K = 2048, N = 512 over a batch: one workgroup a row tile, all columns, weights streamed (igemm_ask_kernel), optionally + LayerNorm
bool ask_fits(LeleCtx* ctx, int64_t rows, int64_t n, int64_t k) {
    return env_int("LELE_HIP_IGEMM_RS", 1) != 0 && env_int("LELE_HIP_IGEMM_ASK", 1) != 0 && k == 2048 && n == 512 && rows * n < (int64_t(1) << 30) &&
           as_two(ctx, rows, (int)n);
}
int launch_ask(LeleCtx* ctx, const int8_t* af, const int8_t* wf, int64_t rows, const IgemmEpi& epi, const AsLn* ln, const char** name) {
    *name = ln ? "rs.ask_ln" : "rs.ask";
    AskArgs g{af, wf, (unsigned)rows};
    if (ln) g.ln_g = ln->g, g.ln_b = ln->b, g.ln_eps = ln->eps, g.ln_out = ln->out, g.ln_rowstat = ln->rowstat;
    const dim3 grid((unsigned)((rows + 31) / 32));
    const int nres = epi.res1 ? (epi.res2 ? 2 : 1) : 0;
#define LELE_ASK(NRES_, LN_)                                                                            \
    do {                                                                                                \
        auto kern = igemm_ask_kernel<NRES_, LN_>;                                                        \
        LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), (LN_) ? ASK_LDS : ASK_TILE)); \
        hipLaunchKernelGGL(kern, grid, dim3(512), (LN_) ? ASK_LDS : ASK_TILE, ctx->stream, g, epi);      \
    } while (0)
    if (ln) {
        if (nres == 0) LELE_ASK(0, true);
        else if (nres == 1) LELE_ASK(1, true);
        else LELE_ASK(2, true);
    } else {
#ifdef LELE_HIP_LAB
        if (nres == 0) LELE_ASK(0, false);
        else if (nres == 1) LELE_ASK(1, false);
        else LELE_ASK(2, false);
#else
        LELE_REQUIRE(false, "launch_ask: the form without a LayerNorm is built into the lab library only");
#endif
    }
#undef LELE_ASK
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

namespace lele {
// {scale, zp, 1/scale, (int)zp} of the joint range of several device arrays (DynamicQuantizeLinear's rule,
// avx/quantization.rs:134-140 == conv2d.rs:2329-2333); prm_dev receives 16 bytes laid out as QParamsDev (common.h)
int quant_params_of(LeleCtx* ctx, const float* const* srcs, const int64_t* lens, int nsrc, void* prm_dev) {
    int64_t total_blocks = 0;
    std::vector<int> nb(nsrc);
    for (int i = 0; i < nsrc; ++i) {
        nb[i] = (int)std::max<int64_t>(1, std::min<int64_t>(256, (lens[i] + 4095) / 4096));
        total_blocks += nb[i];
    }
    void* partial = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)total_blocks * 8, &partial));
    int64_t off = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (lens[i] > 0)
            hipLaunchKernelGGL(qminmax_kernel, dim3(nb[i], 1), dim3(256), 0, ctx->stream, srcs[i], lens[i],
                               (float*)partial + 2 * off);
        else
            nb[i] = 0;
        off += nb[i];
    }
    hipLaunchKernelGGL(qparams_kernel, dim3(1), dim3(64), 0, ctx->stream, (const float*)partial, (int)off, (QParams*)prm_dev,
                       (float*)nullptr, (float*)nullptr);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // namespace lele

namespace {
// the producer's {min, max} pairs, if it left any next to this tensor (LayerNorm: one pair per row; the one-launch kernels: a fixed
// number per slice; a small-problem GEMM: one per workgroup, single slice only): slice s then owns `nblk` consecutive pairs and the
// separate range pass over the activation is skipped
void find_partials(LeleCtx* ctx, const LeleTensor* input, int64_t batch, int64_t m, int64_t k, const float** partial, int* nblk) {
    const int64_t rows = batch * m;
    *partial = nullptr;
    *nblk = 0;
    if (input->mem != LELE_MEM_DEVICE || m > 2048) return;
    auto it = ctx->buf_of_data.find(input->data);
    if (it == ctx->buf_of_data.end() || !it->second->rowstat_valid) return;
    const LeleBuf* src = it->second;
    if (src->rowstat_kind == 0 && src->rowstat_len == k && src->rowstat_rows == rows) {
        *partial = src->rowstat;  // one pair per row
        *nblk = (int)m;
    } else if (src->rowstat_kind == 2 && src->rowstat_len == k && src->rowstat_m == m && src->rowstat_batch == batch && src->rowstat_rows % batch == 0) {
        *partial = src->rowstat;  // a fixed number of pairs per slice of m rows (igemm_rs_kernel, the attention kernels)
        *nblk = (int)(src->rowstat_rows / batch);
    } else if (src->rowstat_kind == 1 && batch == 1 && src->rowstat_len == rows * k && src->rowstat_rows <= 4096) {
        *partial = src->rowstat;  // per-workgroup pairs of the GEMM that produced the tensor: one slice, all pairs
        *nblk = (int)src->rowstat_rows;
    }
}

// `.data.first()` of a zero point (quantization.rs:100), 0 where absent or empty, fetched on the host; callers take it `as i32`
int first_scalar_of(LeleCtx* ctx, const LeleTensor* t, float* v) {
    *v = 0.0f;
    if (!t || numel(t) == 0) return 0;
    if (t->mem != LELE_MEM_DEVICE) {
        *v = *(const float*)t->data;
        return 0;
    }
    LELE_HIP_CHECK(hipMemcpyAsync(v, t->data, 4, hipMemcpyDeviceToHost, ctx->stream));
    LELE_REQUIRE(!ctx->capturing, "graph capture: this op must run once eagerly first (it allocates or synchronises)");
    LELE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------ one quantised linear, described
struct QW {  // a layer's weight tensors as the C ABI passes them
    const LeleTensor *w, *scale, *zero, *bias;
};
// input [.., m, k] x weight [.., kw, n]: `batch` slices of m rows, each quantised with its own range
struct QCall {
    int64_t batch = 1, m = 0, k = 0, kw = 0, n = 0, rows = 0, ws_len = 0, blen = 0;
    std::vector<int64_t> shp;  // the result: the input's shape with n as its last extent
    // weight_scale: one value or one per column; bias: none or one per column
    bool lens_ok() const { return ws_len >= 1 && (ws_len <= 1 || ws_len >= n) && (blen == 0 || blen >= n); }
};
// the extents as the tensors give them, nothing judged (ranks >= 2)
QCall call_dims(const LeleTensor* input, const QW& w) {
    QCall c;
    c.m = input->shape[input->rank - 2], c.k = input->shape[input->rank - 1];
    c.kw = w.w->shape[w.w->rank - 2], c.n = w.w->shape[w.w->rank - 1];
    for (int i = 0; i + 2 < input->rank; ++i) c.batch *= input->shape[i];
    c.rows = c.batch * c.m;
    c.ws_len = w.scale ? numel(w.scale) : 0, c.blen = w.bias ? numel(w.bias) : 0;
    c.shp.assign(input->shape, input->shape + input->rank - 1);
    c.shp.push_back(c.n);
    return c;
}
// ... and judged: `who` names the operator in the messages
int describe_call(const char* who, const LeleTensor* input, const QW& w, QCall* c) {
    LELE_REQUIRE(input->rank >= 2 && w.w->rank >= 2, "%s: rank >= 2 required", who);
    *c = call_dims(input, w);
    LELE_REQUIRE(c->k == c->kw, "%s: K mismatch (%lld vs %lld)", who, (long long)c->k, (long long)c->kw);
    LELE_REQUIRE(c->ws_len >= 1, "%s: empty weight_scale", who);
    LELE_REQUIRE(c->ws_len <= 1 || c->ws_len >= c->n, "%s: weight_scale has %lld entries for N=%lld", who, (long long)c->ws_len, (long long)c->n);
    LELE_REQUIRE(c->blen == 0 || c->blen >= c->n, "%s: bias has %lld entries for N=%lld", who, (long long)c->blen, (long long)c->n);
    return 0;
}
// an f32 residual of the result's shape [.., m, n] (leading unit dimensions aside): folded into the GEMM's store
bool res_same_shape(const LeleTensor* input, int64_t n, const LeleTensor* t) {
    int64_t on = n;
    for (int i = 0; i + 1 < input->rank; ++i) on *= input->shape[i];
    if (t->dtype != LELE_F32 || numel(t) != on || t->rank > input->rank) return false;
    for (int d = 0; d < t->rank; ++d)
        if (t->shape[t->rank - 1 - d] != (d == 0 ? n : input->shape[input->rank - 1 - d])) return false;
    return true;
}
bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// where dev_ptr will put a tensor, as far as alignment goes: a device tensor stays, anything else is staged on a 256-byte boundary
const void* staged_addr(const LeleTensor* t) { return t->mem == LELE_MEM_DEVICE ? t->data : nullptr; }

// a LayerNorm over the last axis that the caller wants behind the linear: done in the GEMM's launch where a workgroup holds whole
// rows of the result (`done` says whether it was; the caller runs lele_hip_layer_norm otherwise)
struct LnReq {
    const LeleTensor* g;
    const LeleTensor* b;
    float eps;
    LeleBuf* out;  // never the linear's own `out` (every entry point that takes a LayerNorm requires two buffers)
    bool done = false;
    // optionally the FSMN memory block as the first residual, COMPUTED IN THE KERNEL (lele_hip_sanm_out_block): the request then
    // carries no res1, and is only made where fql_route answers AsLnFsmn
    const LeleTensor *fs_x = nullptr, *fs_w = nullptr, *fs_b = nullptr;  // [B, T, P], [512, 1, 11], 512 or none
    int64_t fs_pl = 0, fs_off = 0;
};
struct QReq {  // what the caller wants around the product
    int relu = 0;
    const LeleTensor *res1 = nullptr, *res2 = nullptr;  // same-shape residuals (res_same_shape), added in this order
    LnReq* ln = nullptr;
    HeadReq head;  // a decode head in place of the product (igemm_head.h)
};
// the entry point a request came through, as its messages name it
const char* fql_who(const HeadReq& head, bool packed) {
    switch (head.mode) {
        case Head::Ids: return packed ? "fused_quantized_linear_argmax_segments" : "fused_quantized_linear_argmax";
        case Head::Scored: return packed ? "fused_quantized_linear_argmax_logprob_segments" : "fused_quantized_linear_argmax_logprob";
        case Head::TopK: return packed ? "fused_quantized_linear_topk_segments" : "fused_quantized_linear_topk";
        case Head::At: return packed ? "fused_quantized_linear_logprob_at_segments" : "fused_quantized_linear_logprob_at";
        case Head::None: break;
    }
    return packed ? "fused_quantized_linear_segments" : "fused_quantized_linear";
}
// a head's result: the input's shape without its last axis, one i32 a row -- or k a row
int head_shape(const char* who, const HeadReq& head, QCall* c) {
    if (!head) return 0;
    LELE_REQUIRE(c->n >= 1 && c->k >= 1, "%s: empty K or N (K = %lld, N = %lld)", who, (long long)c->k, (long long)c->n);
    c->shp.pop_back();
    if (head.topk()) c->shp.push_back(head.k);
    if (head.listed()) {  // the caller's columns: strictly ascending inside [0, N)
        LELE_REQUIRE(head.cols && head.ncols >= 1 && head.ncols <= c->n, "%s: %lld columns listed, 1 .. N = %lld required", who, (long long)head.ncols,
                     (long long)c->n);
        LELE_REQUIRE(head.ncols < (int64_t(1) << 27), "%s: more than 2^27 listed columns", who);  // (the finish kernel counts 16 rows of them in an int)
        for (int64_t u = 0; u < head.ncols; ++u) {
            LELE_REQUIRE(head.cols[u] >= 0 && head.cols[u] < c->n, "%s: cols[%lld] = %d outside [0, N = %lld)", who, (long long)u, (int)head.cols[u],
                         (long long)c->n);
            LELE_REQUIRE(u == 0 || head.cols[u] > head.cols[u - 1], "%s: cols[%lld] = %d is not greater than cols[%lld] = %d (strictly ascending required)",
                         who, (long long)u, (int)head.cols[u], (long long)(u - 1), (int)head.cols[u - 1]);
        }
    }
    return 0;
}
// Head::At: the call's one table.  Behind what the packed call keeps there anyway (offsets and the row -> segment map; the dense call:
// nothing) the column -> slot map, int [N] with -1 for a column that is not listed: 4 N bytes.  The key is the layout AND the columns
// (as int64 behind the offsets), so that a captured graph's table is the one of its own columns.
struct AtTableArg {
    const int64_t* off;  // NULL: dense
    int64_t count;
    const int32_t* cols;
    int64_t ncols, n;
};
void build_rowseg(const void* arg, std::vector<char>& blob);
void build_at_table(const void* arg, std::vector<char>& blob) {
    const AtTableArg& a = *(const AtTableArg*)arg;
    size_t head = 0;
    if (a.off) {
        const std::pair<const int64_t*, int64_t> rs{a.off, a.count};
        build_rowseg(&rs, blob);
        head = blob.size();
    }
    blob.resize(head + (size_t)a.n * 4);
    int* slot = (int*)(blob.data() + head);
    for (int64_t j = 0; j < a.n; ++j) slot[j] = -1;
    for (int64_t u = 0; u < a.ncols; ++u) slot[a.cols[u]] = (int)u;
}
int at_table(LeleCtx* ctx, const HeadReq& head, const int64_t* off, int64_t count, int64_t n, const void** tab) {
    std::vector<int64_t> key;
    if (off) key.assign(off, off + count + 1);
    key.insert(key.end(), head.cols, head.cols + head.ncols);
    const AtTableArg arg{off, count, head.cols, head.ncols, n};
    return layout_table(ctx, "qsat", off ? count : -1, n, key.data(), (int64_t)key.size() - 1, build_at_table, &arg, tab);
}
// one layer, validated and staged: what a route's body reads
struct QLayer {
    QCall c;
    const LeleTensor* weight = nullptr;
    const float *x = nullptr, *ws = nullptr, *bias = nullptr;  // x NULL: the layer's operand exists in i8 only; bias NULL: none
    const float *res1 = nullptr, *res2 = nullptr;
    float wz = 0.0f;
    int relu = 0;
    QParams* prm = nullptr;          // per slice, filled by whichever kernel reduces the range partials first
    const float* partial = nullptr;  // {min, max} pairs of x, nblk a slice
    int nblk = 0;
    LeleBuf* out = nullptr;
    HeadReq head;  // QReq::head
};
IgemmEpi make_epi(const QLayer& l, float* out, const int* row_sums, const int* col_sums) {
    return IgemmEpi{out, l.c.rows, l.c.n, (int)l.c.m, (int)l.c.k, row_sums, col_sums, l.prm, 0, (int)l.wz, l.ws, (int)l.c.ws_len, l.bias, l.relu,
                    l.res1, l.res2};
}

// {min, max} of every 32 x 32 tile of the result, left next to it for a single-slice consumer (LeleBuf::rowstat kind 1, at most 4096
// pairs): attached before the launch, published after it
int64_t tiles32(const QCall& c) { return ((c.rows + 31) / 32) * ((c.n + 31) / 32); }
int attach_blockstat(LeleBuf* out, const QCall& c, IgemmEpi* epi) {
    const int64_t nstat = tiles32(c);
    if (nstat > 4096) return 0;
    LELE_TRY(out->reserve_rowstat(nstat));
    if ((size_t)nstat <= out->rowstat_cap) epi->blockstat = out->rowstat;
    return 0;
}
void publish_blockstat(LeleBuf* out, const QCall& c, const IgemmEpi& epi) {
    if (!epi.blockstat) return;
    out->rowstat_rows = tiles32(c), out->rowstat_len = c.rows * c.n;
    out->rowstat_kind = 1, out->rowstat_valid = true;
}

// the LayerNorm epilogue of igemm_as_kernel / igemm_ask_kernel: whole 512-wide rows in a workgroup, no ReLU, f32 scale / bias of >= 512
bool as_ln_ok(LeleCtx* ctx, int64_t rows, int64_t n, int apply_relu, const LeleTensor* g, const LeleTensor* b) {
    return env_int("LELE_HIP_LN_FUSED", 1) != 0 && n == 512 && !apply_relu && as_two(ctx, rows, (int)n) && g->dtype == LELE_F32 &&
           b->dtype == LELE_F32 && numel(g) >= 512 && numel(b) >= 512;
}
// the request as the kernel takes it: scale and bias staged, ln->out sized, room for its row statistics
int attach_ln(LeleCtx* ctx, const LnReq* ln, const QCall& c, AsLn* aln) {
    const void *dg = nullptr, *dbeta = nullptr;
    LELE_TRY(ctx->dev_ptr(ln->g, &dg));
    LELE_TRY(ctx->dev_ptr(ln->b, &dbeta));
    LELE_TRY(ln->out->reserve((size_t)c.rows * c.n * 4));
    LELE_TRY(ln->out->reserve_rowstat(c.rows));
    aln->g = (const float*)dg, aln->b = (const float*)dbeta, aln->eps = ln->eps, aln->out = (float*)ln->out->data;
    aln->rowstat = (size_t)c.rows <= ln->out->rowstat_cap ? ln->out->rowstat : nullptr;
    return 0;
}
// ... and after the launch: as lele_hip_layer_norm leaves them, one {min, max} pair per row
void publish_ln(LnReq* ln, const QCall& c, const AsLn& aln) {
    ln->done = true;
    if (!aln.rowstat) return;
    ln->out->rowstat_rows = c.rows, ln->out->rowstat_len = c.n;
    ln->out->rowstat_kind = 0, ln->out->rowstat_valid = true;
}
// an entry point issued the calls it stands for instead of a fused form: "q.calls" in front of the (last) quantised linear's route
void calls_family(LeleCtx* ctx) {
    if (ctx->route[1]) ctx->set_route_family("q.calls");
}
// ... and where no kernel took it: the call it stands for, on the sum in `out`
// (lele_hip_last_route keeps the linear's route, "q.calls" in front of it)
int finish_ln(LeleCtx* ctx, const LnReq& ln, LeleBuf* out, const int64_t* sh, int32_t r) {
    if (ln.done) return 0;
    const LeleTensor x1{out->data, sh, r, LELE_F32, LELE_MEM_DEVICE};
    int64_t sh2[LELE_MAX_RANK];
    int32_t r2 = 0;
    const char *const op = ctx->route[1], *const core = ctx->route[2];
    LELE_TRY(lele_hip_layer_norm(ctx, &x1, ln.g, ln.b, -1, ln.eps, ln.out, sh2, &r2));
    ctx->set_route(op, core);
    calls_family(ctx);
    return 0;
}

// rows -> i8 [rows][kp] + row sums in HBM, for the tiled kernels.  prefetch: the whole row in flight at once (8 x 16 bytes per lane)
int launch_qrows(LeleCtx* ctx, bool prefetch, const float* x, int64_t rows, int k, int kp, int m, QParams* prm, int8_t* aq, int* rs,
                 const float* partial, int nblk, unsigned* zero_slice, int* zero_rows, const int* row_seg) {
    auto kern = prefetch ? qrows_kernel<0, true> : qrows_kernel<0, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ctx->stream, x, rows, k, kp, m, prm, aq, rs, partial, nblk, zero_slice,
                       zero_rows, row_seg);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ the dense linear: route, then body
enum class QRoute {
    RsFq,      // register-stationary (igemm_rs_kernel), its loader waves quantise the f32 rows: one launch
    RsFrag,    // register-stationary behind qrows_frag_kernel (K < 512 padded, or rows not 16-byte aligned)
    As,        // activation-stationary (igemm_as_kernel): quantise and multiply in one kernel
    AsLn,      // ... with the requested LayerNorm in its epilogue
    AsLnFsmn,  // ... and the FSMN memory block computed in the kernel as the first residual
    Tiled,     // rows -> i8 in HBM (qrows_kernel), then the tiled i8 GEMM (launch_igemm)
    TiledHead,  // ... with a head's epilogue (igemm_kernel EM 3 / 4 / 5): the only route of a QReq::head request
};
// The one place that chooses.  dx: the staged input; dout: out->data after its reserve (the one-pass kernels move 16 bytes at a
// time).  A LayerNorm that the chosen kernel cannot take is left to the caller (LnReq::done stays false).
QRoute fql_route(LeleCtx* ctx, const QCall& c, const QReq& rq, const void* dx, const void* dout) {
    if (rq.head) return QRoute::TiledHead;
    const bool aligned = rs_aligned(rq.res1) && rs_aligned(rq.res2) && aligned16(dout);
    if (aligned && rs_fits(ctx, c.rows, c.n, c.k))
        // K = 512 exactly, 16-byte aligned rows: the loaders reduce their parameters from the {min, max} partials, nothing runs in front
        return rs_fq(c.k, dx) && rs_max_slices(ctx, c.rows, c.n, c.m) <= RS_MAXSL ? QRoute::RsFq : QRoute::RsFrag;
    if (aligned && as_fits(ctx, c.rows, c.n, c.k, dx)) {
        if (!rq.ln || !as_ln_ok(ctx, c.rows, c.n, rq.relu, rq.ln->g, rq.ln->b)) return QRoute::As;
        return rq.ln->fs_x ? QRoute::AsLnFsmn : QRoute::AsLn;
    }
    return QRoute::Tiled;
}

// rows -> i8 in fragment order (unless the loaders do it), then the barrier-free GEMM (igemm_rs.h)
int run_rs(LeleCtx* ctx, const QLayer& l, bool fq) {
    const QCall& c = l.c;
    FragW fw;
    LELE_TRY(frag_weights_of(ctx, l.weight, (int)c.k, (int)c.n, 512, &fw));
    void *af = nullptr, *rs = nullptr;
    RsFq fqa;
    if (fq) {
        fqa.x = l.x, fqa.partial = l.partial, fqa.nblk = l.nblk;
    } else {
        LELE_TRY(ctx->arena_alloc((size_t)((c.rows + 31) / 32) * 512 * 32, &af));
        LELE_TRY(ctx->arena_alloc((size_t)c.rows * 4, &rs));
        LELE_TRY(launch_qrows_frag(ctx, l.x, c.rows, (int)c.k, (int)c.m, l.prm, (int8_t*)af, (int*)rs, l.partial, l.nblk, nullptr));
    }
    LELE_TRY(qprof_mark(ctx, 2));
    IgemmEpi epi = make_epi(l, (float*)l.out->data, (const int*)rs, fw.col_sums);
    if (c.batch == 1) LELE_TRY(attach_blockstat(l.out, c, &epi));
    LELE_TRY(launch_rs(ctx, 0, (const int8_t*)af, fw.wf, c.rows, (int)c.n, nullptr, epi, fqa));
    LELE_TRY(qprof_mark(ctx, 3));
    publish_blockstat(l.out, c, epi);
    return 0;
}

// few column tiles, K = 512: quantise and multiply in one kernel, with the LayerNorm (and the memory block) where the route says so
int run_as(LeleCtx* ctx, const QLayer& l, QRoute route, LnReq* ln, const char** core) {
    const QCall& c = l.c;
    FragW fw;
    LELE_TRY(frag_weights_of(ctx, l.weight, (int)c.k, (int)c.n, 512, &fw));
    LELE_TRY(qprof_mark(ctx, 2));
    IgemmEpi epi = make_epi(l, (float*)l.out->data, nullptr, fw.col_sums);
    if (c.batch == 1) LELE_TRY(attach_blockstat(l.out, c, &epi));
    AsLn aln;
    if (route == QRoute::AsLnFsmn) {  // the kernel's res1 is the memory block of fs_x (epi.res1 is not read), epi.res2 the caller's residual
        const void *fx = nullptr, *fwp = nullptr, *fbp = nullptr;
        LELE_TRY(ctx->dev_ptr(ln->fs_x, &fx));
        LELE_TRY(ctx->dev_ptr(ln->fs_w, &fwp));
        if (ln->fs_b) LELE_TRY(ctx->dev_ptr(ln->fs_b, &fbp));
        aln.fs_x = (const float*)fx + ln->fs_off, aln.fs_pitch = (int)ln->fs_x->shape[2], aln.fs_w = (const float*)fwp;
        aln.fs_b = (const float*)fbp, aln.fs_pl = (int)ln->fs_pl;
    }
    const bool fuse_ln = route != QRoute::As;
    if (fuse_ln) LELE_TRY(attach_ln(ctx, ln, c, &aln));  // (a first reserve of ln->out cannot move `out`: they are different buffers)
    LELE_TRY(launch_as(ctx, l.x, fw.wf, c.rows, (int)c.n, l.partial, l.nblk, l.prm, epi, fuse_ln ? &aln : nullptr, core));
    if (fuse_ln) publish_ln(ln, c, aln);
    LELE_TRY(qprof_mark(ctx, 3));
    publish_blockstat(l.out, c, epi);
    return 0;
}

// three-kernel chain: rows -> i8 (+ row sums) in HBM, then the tiled i8 GEMM (a head: l.out receives the ids)
int run_tiled(LeleCtx* ctx, const QLayer& l, const char** op, const char** core) {
    const QCall& c = l.c;
    const int kp = (int)((c.k + 15) & ~int64_t(15));
    PackedW pw;
    LELE_TRY(packed_weights_of(ctx, l.weight, nullptr, 1, (int)c.k, (int)c.n, kp, &pw));
    void *aq = nullptr, *rs = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)c.rows * kp, &aq));
    LELE_TRY(ctx->arena_alloc((size_t)c.rows * 4, &rs));
    const bool prefetch = c.rows <= 2048 || (kp <= 2048 && !lab_int("LELE_HIP_QROWS_STREAM", 0));
    *op = l.head ? "q.head" : prefetch ? "q.tiled" : "q.tiled_stream";
    LELE_TRY(launch_qrows(ctx, prefetch, l.x, c.rows, (int)c.k, kp, (int)c.m, l.prm,
                          (int8_t*)aq, (int*)rs, l.partial, l.nblk, nullptr, nullptr, nullptr));
    LELE_TRY(qprof_mark(ctx, 2));
    if (l.head) {
        HeadOut o;
        LELE_TRY(head_workspace(ctx, l.head, c.rows, c.n, &o));
        o.results(l.out, l.head);
        LELE_TRY(launch_igemm_head(ctx, (const int8_t*)aq, pw.wt, c.rows, (int)c.n, kp, (int)c.m, make_epi(l, nullptr, (const int*)rs, pw.col_sums), l.head, o, core));
        return qprof_mark(ctx, 3);
    }
    IgemmEpi epi = make_epi(l, (float*)l.out->data, (const int*)rs, pw.col_sums);
    // small-problem kernel: publish one {min, max} pair per workgroup next to the result (for the linear that may follow)
    if (((c.rows + 63) / 64) * ((c.n + 63) / 64) < 2 * (int64_t)ctx->num_cus) LELE_TRY(attach_blockstat(l.out, c, &epi));
    LELE_TRY(launch_igemm(ctx, (const int8_t*)aq, pw.wt, c.rows, (int)c.n, kp, (int)c.m, epi, core));
    LELE_TRY(qprof_mark(ctx, 3));
    publish_blockstat(l.out, c, epi);
    return 0;
}

// validate, reserve, stage, range pass, then the route's body.  The order is observable: the reserve clears the statistics `out`
// published (it may be the producer of `input`'s) before find_partials looks for them.
int fql_impl(LeleCtx* ctx, const LeleTensor* input, const QW& w, const QReq& rq, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && w.w && w.scale && out, "fused_quantized_linear: NULL argument");
    QLayer l;
    const char* const who = fql_who(rq.head, false);
    LELE_TRY(describe_call(who, input, w, &l.c));
    QCall& c = l.c;
    LELE_TRY(head_shape(who, rq.head, &c));
    const size_t out_bytes = (size_t)c.rows * (rq.head ? rq.head.k : c.n) * 4;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* at_tab = nullptr;
    if (rq.head.listed() && c.rows > 0) LELE_TRY(at_table(ctx, rq.head, nullptr, 0, c.n, &at_tab));
    LELE_TRY(out->reserve(out_bytes));
    if (rq.head.scored()) LELE_TRY(rq.head.logprob->reserve(out_bytes));
    if (rq.head.listed()) LELE_TRY(rq.head.at->reserve((size_t)c.rows * rq.head.ncols * 4));
    ctx->set_route(nullptr);  // lele_hip_last_route: "" for a call that launches nothing
    if (c.rows == 0 || c.n == 0) return set_shape_v(out_shape, out_rank, c.shp);
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dws = nullptr, *db = nullptr, *dr1 = nullptr, *dr2 = nullptr;
    LELE_TRY(ctx->dev_ptr(input, &dx));
    LELE_TRY(ctx->dev_ptr(w.scale, &dws));
    if (c.blen) LELE_TRY(ctx->dev_ptr(w.bias, &db));
    if (rq.res1) LELE_TRY(ctx->dev_ptr(rq.res1, &dr1));
    if (rq.res2) LELE_TRY(ctx->dev_ptr(rq.res2, &dr2));
    LELE_TRY(first_scalar_of(ctx, w.zero, &l.wz));
    find_partials(ctx, input, c.batch, c.m, c.k, &l.partial, &l.nblk);
    void* prm = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)c.batch * sizeof(QParams), &prm));
    l.weight = w.w, l.x = (const float*)dx, l.ws = (const float*)dws, l.bias = (const float*)db, l.relu = rq.relu;
    l.res1 = (const float*)dr1, l.res2 = (const float*)dr2, l.prm = (QParams*)prm, l.out = out, l.head = rq.head;
    l.head.at_slot = (const int*)at_tab;
    LELE_TRY(qprof_mark(ctx, 0));
    if (!l.partial) LELE_TRY(launch_range(ctx, l.x, c.batch, c.m * c.k, l.prm, nullptr, nullptr, &l.partial, &l.nblk));
    LELE_TRY(qprof_mark(ctx, 1));
    const QRoute route = fql_route(ctx, c, rq, dx, out->data);
    const char *op = nullptr, *core = nullptr;  // (the register-stationary kernel has no second level)
    switch (route) {
        case QRoute::RsFq:
        case QRoute::RsFrag:
            op = route == QRoute::RsFq ? "q.rs_fq" : "q.rs_frag";
            LELE_TRY(run_rs(ctx, l, route == QRoute::RsFq));
            break;
        case QRoute::As:
        case QRoute::AsLn:
        case QRoute::AsLnFsmn:
            op = route == QRoute::As ? "q.as" : route == QRoute::AsLn ? "q.as_ln" : "q.as_ln_fsmn";
            LELE_TRY(run_as(ctx, l, route, rq.ln, &core));
            break;
        case QRoute::Tiled:
        case QRoute::TiledHead: LELE_TRY(run_tiled(ctx, l, &op, &core)); break;
    }
    ctx->set_route(op, core);
    return set_shape_v(out_shape, out_rank, c.shp);
}

// row -> segment map behind the offsets, in one table: [int64 off[count + 1]][int row_seg[R]]
void build_rowseg(const void* arg, std::vector<char>& blob) {
    const auto& a = *(const std::pair<const int64_t*, int64_t>*)arg;
    const int64_t* off = a.first;
    const int64_t count = a.second, r = off[count];
    blob.resize((size_t)(count + 1) * 8 + (size_t)r * 4);
    memcpy(blob.data(), off, (size_t)(count + 1) * 8);
    int* rs = (int*)(blob.data() + (size_t)(count + 1) * 8);
    for (int64_t i = 0; i < count; ++i)
        for (int64_t row = off[i]; row < off[i + 1]; ++row) rs[row] = (int)i;
}

// can igemm_as_kernel compute depthwise_conv1d_tlc(v_src, .., add_input = 1) of the projection's rows itself: v_src [B, T, P] with B * T
// the projection's rows and T its slice length, 512 channels from a 16-byte aligned offset, k = 11 with the output as long as the input
bool fsmn_fits(const QCall& c, const LeleTensor* v_src, const LeleTensor* fsmn_w, const LeleTensor* fsmn_bias, int64_t x_offset,
               int64_t pad_left, int64_t pad_right) {
    return v_src->rank == 3 && v_src->dtype == LELE_F32 && fsmn_w->rank == 3 && fsmn_w->dtype == LELE_F32 && fsmn_w->shape[0] == 512 &&
           fsmn_w->shape[1] == 1 && fsmn_w->shape[2] == 11 && v_src->shape[0] * v_src->shape[1] == c.rows && v_src->shape[1] == c.m && c.m >= 32 &&
           x_offset >= 0 && x_offset % 4 == 0 && x_offset + 512 <= v_src->shape[2] && v_src->shape[2] % 4 == 0 && rs_aligned(v_src) &&
           pad_left == 5 && pad_right == 5 && (!fsmn_bias || (fsmn_bias->dtype == LELE_F32 && numel(fsmn_bias) >= 512)) &&
           v_src->shape[2] * c.rows < (int64_t(1) << 30);
}

// ------------------------------------------------------------------------------------------ the feed-forward block: route, then body
enum class FfnRoute {
    Unfused,  // the two calls it stands for, an f32 hidden layer between them
    Rs,       // register-stationary: K = 512 into exactly 2048 hidden columns, written as i8 in the second product's fragment order
    Tiled,    // the hidden layer's product twice on the tiled kernel (range, then quantise), the second GEMM on its i8 rows
};
// c1: the first layer as call_dims gives it (nothing validated yet: what does not fit the fused forms runs the two calls, which raise)
FfnRoute ffn_route(LeleCtx* ctx, const LeleTensor* input, const QCall& c1, int64_t k2, int64_t n2, const LeleTensor* res1, const LeleTensor* res2) {
    const int64_t rows = c1.rows, n1 = c1.n;
    if (env_int("LELE_HIP_FFN_FUSED", 1) == 0 || c1.kw != c1.k || k2 != n1 || rows >= (int64_t(1) << 31) || !c1.lens_ok() || n2 < 1)
        return FfnRoute::Unfused;
    // (the second product's threshold is ONE tile per CU: at one 30 s utterance -- 16 x 16 tiles -- the fused block replaces ffn1 with an f32
    // hidden layer | row quantisation | small-problem GEMM: a configs[2] forward 5.33 -> 5.05 ms, round 6)
    const bool rs = pads_to_512(c1.k) && n1 == 2048 && rs_enabled(ctx, rows, n1) && rs_enabled(ctx, rows, n2, 1) && rs_aligned(res1) && rs_aligned(res2);
    // tiled: a hidden layer of whole 128-column tiles (= whole SIMD bodies of its quantiser), slices of at least one tile of rows,
    // enough tiles to fill the chip
    const bool tiled = n1 % 128 == 0 && c1.m >= 128 && ((rows + 127) / 128) * (n1 / 128) >= 2 * (int64_t)ctx->num_cus;
    if (!rs && !tiled) return FfnRoute::Unfused;
    if (res1 && !(res_same_shape(input, n2, res1) && (!res2 || res_same_shape(input, n2, res2)))) return FfnRoute::Unfused;
    return rs ? FfnRoute::Rs : FfnRoute::Tiled;
}

// the second product of the register-stationary form
enum class FfnSecond {
    Ks4,    // one column tile a workgroup over a range of row tiles (igemm_rs_ks4_kernel)
    Ask,    // one row tile a workgroup with all 512 columns (igemm_ask_kernel): lab only
    AskLn,  // ... and the requested LayerNorm in its epilogue
};
FfnSecond ffn_second(LeleCtx* ctx, const QCall& c2, int relu2, const LnReq* ln, const void* dout) {
    if (!ask_fits(ctx, c2.rows, c2.n, c2.k) || !aligned16(dout)) return FfnSecond::Ks4;
    if (ln && as_ln_ok(ctx, c2.rows, c2.n, relu2, ln->g, ln->b)) return FfnSecond::AskLn;
#ifdef LELE_HIP_LAB
    if (lab_int("LELE_HIP_IGEMM_ASK_ALWAYS", 0) != 0) return FfnSecond::Ask;
#endif
    return FfnSecond::Ks4;
}

int ffn_unfused(LeleCtx* ctx, const LeleTensor* input, const QW& w1, const QW& w2, const QReq& rq, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LeleBuf* hid = nullptr;
    LELE_TRY(ctx->tmp_buf(2, &hid));
    int64_t sh[LELE_MAX_RANK];
    int32_t r = 0;
    LELE_TRY(fql_impl(ctx, input, w1, QReq{1}, hid, sh, &r));
    LeleTensor h{hid->data, sh, r, LELE_F32, LELE_MEM_DEVICE};
    if (rq.res1) LELE_TRY(lele_hip_fused_quantized_linear_residual(ctx, &h, w2.w, w2.scale, w2.zero, w2.bias, rq.relu, rq.res1, rq.res2, out, out_shape, out_rank));
    else LELE_TRY(fql_impl(ctx, &h, w2, QReq{rq.relu}, out, out_shape, out_rank));
    calls_family(ctx);  // in front of the second linear's route
    return 0;
}

// l1.partial: the {min, max} pairs of the input; both layers' parameters are reduced inside the kernels
int ffn_rs(LeleCtx* ctx, const QLayer& l1, const QLayer& l2, LnReq* ln, const char** op, const char** core) {
    const QCall &c1 = l1.c, &c2 = l2.c;
    const int64_t rows = c1.rows, nrt = (rows + 31) / 32;
    FragW fw1, fw2;
    LELE_TRY(frag_weights_of(ctx, l1.weight, (int)c1.k, (int)c1.n, 512, &fw1));
    LELE_TRY(frag_weights_of(ctx, l2.weight, (int)c2.k, (int)c2.n, 2048, &fw2));
    void *af1 = nullptr, *rs1 = nullptr, *hid = nullptr, *hmax = nullptr;
    // both passes of the first product quantise the f32 rows in their loader waves, with parameters reduced inside the kernels; the
    // range pass leaves four maxima a workgroup (plain stores: nothing to clear) which the quantise pass's loaders reduce
    const bool fq = rs_fq(c1.k, l1.x) && rs_max_slices(ctx, rows, c1.n, c1.m) <= 4;
    LELE_TRY(ctx->arena_alloc((size_t)nrt * 2048 * 32, &hid));
    LELE_TRY(ctx->arena_alloc((size_t)c1.batch * 4, &hmax));
    RsFq fqa;
    if (fq) {
        int ncb = 0, nrr = 0;
        rs_grid(ctx, rows, c1.n, &ncb, &nrr);
        void* hpart = nullptr;
        LELE_TRY(ctx->arena_alloc((size_t)ncb * nrr * 16, &hpart));
        fqa.x = l1.x, fqa.partial = l1.partial, fqa.nblk = l1.nblk, fqa.hpart = (unsigned*)hpart;
        fqa.sync = rs_sync_counters(ctx, rows, c1.n);
    } else {
        LELE_TRY(ctx->arena_alloc((size_t)nrt * 512 * 32, &af1));
        LELE_TRY(ctx->arena_alloc((size_t)rows * 4, &rs1));
        // rows -> i8 for the first product; the same launch clears the per-slice maxima the range pass adds into
        LELE_TRY(launch_qrows_frag(ctx, l1.x, rows, (int)c1.k, (int)c1.m, l1.prm, (int8_t*)af1, (int*)rs1, l1.partial, l1.nblk, (unsigned*)hmax));
    }
    LELE_TRY(qprof_mark(ctx, 2));
    // (tests) LELE_HIP_FFN_ONE_LAUNCH=2: fail instead of falling back to the two launches, so that a test of the one-launch form tests it
    LELE_REQUIRE(env_int("LELE_HIP_FFN_ONE_LAUNCH", 1) != 2 || fqa.sync,
                 "fused_ffn_quantized: LELE_HIP_FFN_ONE_LAUNCH=2, but this call cannot take the one-launch form (K = 512 exactly, 16-byte aligned "
                 "rows, at most 4 slices and %d row tiles a workgroup, lane 0 of the only context of the device, counters made before a capture)",
                 RS_NS_BOTH);
    IgemmEpi e1 = make_epi(l1, nullptr, (const int*)rs1, fw1.col_sums);
    e1.slice_max = (unsigned*)hmax;
    *op = fqa.sync ? "qffn.rs_one" : "qffn.rs_two";
    if (fqa.sync) {  // both passes in one launch (igemm_rs.h, EM 3)
        e1.q_prm = l2.prm;
        LELE_TRY(launch_rs(ctx, 3, nullptr, fw1.wf, rows, (int)c1.n, (int8_t*)hid, e1, fqa));
    } else {
        LELE_TRY(launch_rs(ctx, 1, (const int8_t*)af1, fw1.wf, rows, (int)c1.n, nullptr, e1, fqa));   // range of the ReLU result per slice
        e1.q_prm = l2.prm;
        LELE_TRY(launch_rs(ctx, 2, (const int8_t*)af1, fw1.wf, rows, (int)c1.n, (int8_t*)hid, e1, fqa));  // the result again, as the next operand
    }
    const IgemmEpi e2 = make_epi(l2, (float*)l2.out->data, nullptr, fw2.col_sums);
    const FfnSecond second = ffn_second(ctx, c2, l2.relu, ln, l2.out->data);
    if (second == FfnSecond::Ks4) {
        LELE_TRY(launch_rs_ks4(ctx, (const int8_t*)hid, fw2.wf, rows, (int)c2.n, e2, core));
    } else {
        AsLn aln;
        if (second == FfnSecond::AskLn) LELE_TRY(attach_ln(ctx, ln, c2, &aln));
        LELE_TRY(launch_ask(ctx, (const int8_t*)hid, fw2.wf, rows, e2, second == FfnSecond::AskLn ? &aln : nullptr, core));
        if (second == FfnSecond::AskLn) publish_ln(ln, c2, aln);
    }
    return qprof_mark(ctx, 3);
}

int ffn_tiled(LeleCtx* ctx, const QLayer& l1, const QLayer& l2, const char** op, const char** core) {
    const QCall &c1 = l1.c, &c2 = l2.c;
    const int64_t rows = c1.rows;
    const int kp1 = (int)((c1.k + 15) & ~int64_t(15)), kp2 = (int)c1.n;
    PackedW pw1, pw2;
    LELE_TRY(packed_weights_of(ctx, l1.weight, nullptr, 1, (int)c1.k, (int)c1.n, kp1, &pw1));
    LELE_TRY(packed_weights_of(ctx, l2.weight, nullptr, 1, (int)c2.k, (int)c2.n, kp2, &pw2));
    void *aq1 = nullptr, *rs1 = nullptr, *aq2 = nullptr, *rs2 = nullptr, *hmax = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)rows * kp1, &aq1));
    LELE_TRY(ctx->arena_alloc((size_t)rows * 4, &rs1));
    LELE_TRY(ctx->arena_alloc((size_t)rows * kp2, &aq2));
    LELE_TRY(ctx->arena_alloc((size_t)rows * 4, &rs2));
    LELE_TRY(ctx->arena_alloc((size_t)c1.batch * 4, &hmax));
    // rows -> i8 for the first GEMM; the same launch clears the accumulators of the two hidden-layer passes
    const bool prefetch = kp1 <= 2048 && !lab_int("LELE_HIP_QROWS_STREAM", 0);
    *op = prefetch ? "qffn.tiled" : "qffn.tiled_stream";
    LELE_TRY(launch_qrows(ctx, prefetch, l1.x, rows, (int)c1.k, kp1, (int)c1.m, l1.prm, (int8_t*)aq1,
                          (int*)rs1, l1.partial, l1.nblk, (unsigned*)hmax, (int*)rs2, nullptr));
    LELE_TRY(qprof_mark(ctx, 2));
    IgemmEpi e1 = make_epi(l1, nullptr, (const int*)rs1, pw1.col_sums);
    e1.slice_max = (unsigned*)hmax;
    LELE_TRY(launch_igemm_hidden(ctx, 1, (const int8_t*)aq1, pw1.wt, rows, (int)c1.n, kp1, (int)c1.m, e1));
    e1.q_out = (int8_t*)aq2;
    e1.q_rowsum = (int*)rs2;
    e1.q_prm = l2.prm;
    LELE_TRY(launch_igemm_hidden(ctx, 2, (const int8_t*)aq1, pw1.wt, rows, (int)c1.n, kp1, (int)c1.m, e1));
    const IgemmEpi e2 = make_epi(l2, (float*)l2.out->data, (const int*)rs2, pw2.col_sums);
    LELE_TRY(launch_igemm(ctx, (const int8_t*)aq2, pw2.wt, rows, (int)c2.n, kp2, (int)c1.m, e2, core));
    return qprof_mark(ctx, 3);
}

/* Two quantised linears with a ReLU between them (the feed-forward block of a transformer layer):
 *     out = fused_quantized_linear[_residual](fused_quantized_linear(input, W1.., relu = 1), W2.., relu2, res1, res2)
 * bit for bit.  When the hidden layer is large the f32 hidden tensor is never stored: its product runs twice on the matrix cores
 * (igemm_kernel EM 1: range only; EM 2: quantise with that range, i8 + row sums), then the second GEMM consumes the i8 rows. */
int ffn_impl(LeleCtx* ctx, const LeleTensor* input, const QW& w1, const QW& w2, const QReq& rq, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && w1.w && w1.scale && w2.w && w2.scale && out, "fused_ffn_quantized: NULL argument");
    LELE_REQUIRE(input->rank >= 2 && w1.w->rank >= 2 && w2.w->rank >= 2, "fused_ffn_quantized: rank >= 2 required");
    LELE_REQUIRE(!rq.res2 || rq.res1, "fused_ffn_quantized: res2 without res1");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    QLayer l1, l2;
    l1.c = call_dims(input, w1);
    const FfnRoute route = ffn_route(ctx, input, l1.c, w2.w->shape[w2.w->rank - 2], w2.w->shape[w2.w->rank - 1], rq.res1, rq.res2);
    if (route == FfnRoute::Unfused) return ffn_unfused(ctx, input, w1, w2, rq, out, out_shape, out_rank);
    // the second layer reads the hidden tensor [.., m, n1], which exists in i8 only
    std::vector<int64_t> hshape(l1.c.shp);
    const LeleTensor hidden{nullptr, hshape.data(), input->rank, LELE_F32, LELE_MEM_DEVICE};
    LELE_TRY(describe_call("fused_ffn_quantized", &hidden, w2, &l2.c));
    const QCall &c1 = l1.c, &c2 = l2.c;
    LELE_TRY(out->reserve((size_t)c2.rows * c2.n * 4));
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dws1 = nullptr, *db1 = nullptr, *dws2 = nullptr, *db2 = nullptr, *dr1 = nullptr, *dr2 = nullptr;
    LELE_TRY(ctx->dev_ptr(input, &dx));
    LELE_TRY(ctx->dev_ptr(w1.scale, &dws1));
    LELE_TRY(ctx->dev_ptr(w2.scale, &dws2));
    if (c1.blen) LELE_TRY(ctx->dev_ptr(w1.bias, &db1));
    if (c2.blen) LELE_TRY(ctx->dev_ptr(w2.bias, &db2));
    if (rq.res1) LELE_TRY(ctx->dev_ptr(rq.res1, &dr1));
    if (rq.res2) LELE_TRY(ctx->dev_ptr(rq.res2, &dr2));
    LELE_TRY(first_scalar_of(ctx, w1.zero, &l1.wz));
    LELE_TRY(first_scalar_of(ctx, w2.zero, &l2.wz));
    find_partials(ctx, input, c1.batch, c1.m, c1.k, &l1.partial, &l1.nblk);
    void *prm1 = nullptr, *prm2 = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)c1.batch * sizeof(QParams), &prm1));
    LELE_TRY(ctx->arena_alloc((size_t)c1.batch * sizeof(QParams), &prm2));
    l1.weight = w1.w, l1.x = (const float*)dx, l1.ws = (const float*)dws1, l1.bias = (const float*)db1, l1.relu = 1, l1.prm = (QParams*)prm1;
    l2.weight = w2.w, l2.ws = (const float*)dws2, l2.bias = (const float*)db2, l2.relu = rq.relu, l2.prm = (QParams*)prm2;
    l2.res1 = (const float*)dr1, l2.res2 = (const float*)dr2, l2.out = out;
    LELE_TRY(qprof_mark(ctx, 0));
    if (!l1.partial) LELE_TRY(launch_range(ctx, l1.x, c1.batch, c1.m * c1.k, l1.prm, nullptr, nullptr, &l1.partial, &l1.nblk));
    LELE_TRY(qprof_mark(ctx, 1));
    const char *op = nullptr, *core = nullptr;
    if (route == FfnRoute::Rs) LELE_TRY(ffn_rs(ctx, l1, l2, rq.ln, &op, &core));
    else LELE_TRY(ffn_tiled(ctx, l1, l2, &op, &core));
    ctx->set_route(op, core);
    return set_shape_v(out_shape, out_rank, c2.shp);
}

/* Packed batch: every segment of input [R, K] is a batch slice of its own (quantization.rs:104-128).  Three things know about
 * segments -- the range pass (one {min, max} per segment), the row quantiser's parameter lookup and the epilogue's row_ctx, the last
 * two through a row -> segment map -- and the integer sums are exact, so a segment's rows are the dense entry point's on it alone. */
int fql_segments_impl(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count, const QW& w, const QReq& rq, LeleBuf* out,
                      int64_t* out_shape, int32_t* out_rank) {
    const char* const who = fql_who(rq.head, true);
    LeleBuf* const logprob = rq.head.scored() ? rq.head.logprob : nullptr;
    LELE_REQUIRE(ctx && input && w.w && w.scale && out, "%s: NULL argument", who);
    int64_t rows = 0, k = 0, tmax = 0;
    LELE_TRY(seg_offsets(input, row_offsets, count, &rows, &k, &tmax, who));
    QLayer l;  // input [R, K]: one "slice" of R rows, whose rows find their segment's parameters through row_seg
    LELE_TRY(describe_call(rq.head ? who : fql_who(rq.head, false), input, w, &l.c));  // (without a head it names the dense call)
    QCall& c = l.c;
    const int64_t n = c.n;
    LELE_REQUIRE(rows < (int64_t(1) << 31) && count < (int64_t(1) << 31), "%s: more than 2^31 rows or segments", who);
    LELE_TRY(head_shape(who, rq.head, &c));
    const size_t out_bytes = (size_t)rows * (rq.head ? rq.head.k : n) * 4;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* tab = nullptr;
    if (rows > 0 && n > 0 && k > 0) {
        const std::pair<const int64_t*, int64_t> arg{row_offsets, count};
        if (rq.head.listed()) LELE_TRY(at_table(ctx, rq.head, row_offsets, count, n, &tab));
        else LELE_TRY(layout_table(ctx, "qseg", 0, 0, row_offsets, count, build_rowseg, &arg, &tab));
    }
    const size_t at_bytes = rq.head.listed() ? (size_t)rows * rq.head.ncols * 4 : 0;
    ctx->set_route(nullptr);  // lele_hip_last_route: "" for a call that launches nothing
    if (rows == 0 || n == 0 || k == 0) {
        LELE_TRY(out->reserve(out_bytes));
        if (logprob) LELE_TRY(logprob->reserve(out_bytes));
        if (rq.head.listed()) LELE_TRY(rq.head.at->reserve(at_bytes));
        return set_shape_v(out_shape, out_rank, c.shp);
    }
    const int64_t* doff = (const int64_t*)tab;
    const int* drowseg = (const int*)((const char*)tab + (size_t)(count + 1) * 8);
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dws = nullptr, *db = nullptr;
    LELE_TRY(ctx->dev_ptr(input, &dx));
    LELE_TRY(ctx->dev_ptr(w.scale, &dws));
    if (c.blen) LELE_TRY(ctx->dev_ptr(w.bias, &db));
    LELE_TRY(first_scalar_of(ctx, w.zero, &l.wz));
    // 1. one range per segment: {min, max} partials only, which the row quantiser's waves reduce themselves (as in the dense chain: one
    // launch fewer).  Enough blocks for every thread of the LONGEST segment to stream ~4 float4, at most 128 pairs a segment (a row's
    // wave reads its segment's pairs in one trip); the surplus blocks of a shorter segment leave the neutral pair.
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(128, (tmax * k + 4095) / 4096));
    void *prm = nullptr, *partial = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)count * sizeof(QParams), &prm));
    LELE_TRY(ctx->arena_alloc((size_t)count * nblk * 8, &partial));
    l.x = (const float*)dx, l.ws = (const float*)dws, l.bias = (const float*)db, l.relu = rq.relu, l.prm = (QParams*)prm;
    LELE_TRY(qprof_mark(ctx, 0));
    for (int64_t c0 = 0; c0 < count; c0 += 65535) {  // grid.y limit
        const int64_t nc = std::min<int64_t>(65535, count - c0);
        hipLaunchKernelGGL(qminmax_seg_kernel, dim3(nblk, (unsigned)nc), dim3(256), 0, ctx->stream, l.x, doff + c0, k,
                           (float*)partial + c0 * nblk * 2);
    }
    LELE_TRY(qprof_mark(ctx, 1));
    // 2. rows -> i8 with their segment's parameters, 3. the tiled i8 GEMM whose epilogue looks the segment up per row
    const int kp = (int)((k + 15) & ~int64_t(15));
    PackedW pw;
    LELE_TRY(packed_weights_of(ctx, w.w, nullptr, 1, (int)k, (int)n, kp, &pw));
    void *aq = nullptr, *rs = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)rows * kp, &aq));
    LELE_TRY(ctx->arena_alloc((size_t)rows * 4, &rs));
    HeadOut ho;
    if (rq.head) LELE_TRY(head_workspace(ctx, rq.head, rows, n, &ho));
    // every fallible step is behind us: `out` is as it was until here (reserve clears any producer-side statistics of `out`;
    // those of `input` describe equal slices and are not read)
    LELE_TRY(out->reserve(out_bytes));
    if (logprob) LELE_TRY(logprob->reserve(out_bytes));
    if (rq.head.listed()) LELE_TRY(rq.head.at->reserve(at_bytes));
    const bool prefetch = rows <= 2048 || kp <= 2048;
    const char* core = nullptr;
    LELE_TRY(launch_qrows(ctx, prefetch, l.x, rows, (int)k, kp, (int)rows, l.prm, (int8_t*)aq, (int*)rs, (const float*)partial,
                          nblk, nullptr, nullptr, drowseg));
    LELE_TRY(qprof_mark(ctx, 2));
    IgemmEpi epi = make_epi(l, rq.head ? nullptr : (float*)out->data, (const int*)rs, pw.col_sums);
    epi.row_seg = drowseg;
    if (rq.head) {
        HeadReq head = rq.head;
        head.at_slot = (const int*)((const char*)tab + (size_t)(count + 1) * 8 + (size_t)rows * 4);  // (Head::At; read by no other head)
        ho.results(out, head);
        LELE_TRY(launch_igemm_head(ctx, (const int8_t*)aq, pw.wt, rows, (int)n, kp, (int)rows, epi, head, ho, &core));
    } else {
        LELE_TRY(launch_igemm(ctx, (const int8_t*)aq, pw.wt, rows, (int)n, kp, (int)rows, epi, &core));
    }
    ctx->set_route(rq.head ? "q.seg_head" : prefetch ? "q.seg" : "q.seg_stream", core);
    LELE_TRY(qprof_mark(ctx, 3));
    return set_shape_v(out_shape, out_rank, c.shp);
}

// the eight head entry points: what they require of k and of their outputs, then the dense or the packed linear (row_offsets / count)
int fql_head(LeleCtx* ctx, Head mode, int32_t k, bool packed, const LeleTensor* input, const int64_t* row_offsets, int64_t count, const QW& w,
             LeleBuf* out_ids, LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank, const int32_t* cols = nullptr, int64_t ncols = 0,
             LeleBuf* out_at = nullptr) {
    QReq rq;
    rq.head = HeadReq{mode, mode == Head::TopK ? (int)k : 1, out_logprob, cols, ncols, out_at};
    const char* const who = fql_who(rq.head, packed);
    if (rq.head.scored()) LELE_REQUIRE(out_ids && out_logprob && out_ids != out_logprob, "%s: two distinct output buffers required", who);
    if (rq.head.listed())
        LELE_REQUIRE(out_at && out_at != out_ids && out_at != out_logprob, "%s: three distinct output buffers required", who);
    if (rq.head.topk()) LELE_REQUIRE(k >= 1 && k <= 8, "%s: k = %d outside [1, 8]", who, (int)k);
    return packed ? fql_segments_impl(ctx, input, row_offsets, count, w, rq, out_ids, out_shape, out_rank)
                  : fql_impl(ctx, input, w, rq, out_ids, out_shape, out_rank);
}

}  // namespace

extern "C" {

int lele_hip_fused_quantized_linear(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                    const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                    const LeleTensor* bias, int apply_relu, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank) {
    return fql_impl(ctx, input, {weight_int8, weight_scale, weight_zero, bias}, QReq{apply_relu}, out, out_shape, out_rank);
}

int lele_hip_fused_quantized_linear_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                             const LeleTensor* weight_int8, const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                             const LeleTensor* bias, int apply_relu, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    return fql_segments_impl(ctx, input, row_offsets, count, {weight_int8, weight_scale, weight_zero, bias}, QReq{apply_relu}, out, out_shape, out_rank);
}

/* The greedy decode head (tokenizer.rs:50-61 behind quantization.rs:77-169): argmax_last(fused_quantized_linear(.., apply_relu = 0)) bit for
 * bit, with the arg-max inside the GEMM's epilogue (igemm_kernel EM 3) -- the logits are never stored. */
int lele_hip_fused_quantized_linear_argmax(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                           const LeleTensor* weight_zero, const LeleTensor* bias, LeleBuf* out_ids, int64_t* out_shape,
                                           int32_t* out_rank) {
    return fql_head(ctx, Head::Ids, 1, false, input, nullptr, 0, {weight_int8, weight_scale, weight_zero, bias}, out_ids, nullptr, out_shape, out_rank);
}

int lele_hip_fused_quantized_linear_argmax_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                    const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                    const LeleTensor* weight_zero, const LeleTensor* bias, LeleBuf* out_ids,
                                                    int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::Ids, 1, true, input, row_offsets, count, {weight_int8, weight_scale, weight_zero, bias}, out_ids, nullptr, out_shape, out_rank);
}

/* ... with the winner's log-probability (tokenizer.rs:50-71 behind quantization.rs:77-169): -ln sum_j exp(v_j - v_id) from the same epilogue
 * (igemm_kernel EM 4), the ids bit for bit those of the call above. */
int lele_hip_fused_quantized_linear_argmax_logprob(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                                   const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias,
                                                   LeleBuf* out_ids, LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::Scored, 1, false, input, nullptr, 0, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape, out_rank);
}

int lele_hip_fused_quantized_linear_argmax_logprob_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                            const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                            const LeleTensor* weight_zero, const LeleTensor* bias, LeleBuf* out_ids,
                                                            LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::Scored, 1, true, input, row_offsets, count, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape,
                    out_rank);
}

/* ... and the k best tokens a frame (1 <= k <= 8) in argmax_key's order -- greater value first, of equal values the greater column first --
 * with their log-probabilities, from k rounds of the same epilogue (igemm_kernel EM 5).  Slot 0 is the call above bit for bit. */
int lele_hip_fused_quantized_linear_topk(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                         const LeleTensor* weight_zero, const LeleTensor* bias, int32_t k, LeleBuf* out_ids,
                                         LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::TopK, k, false, input, nullptr, 0, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape, out_rank);
}

int lele_hip_fused_quantized_linear_topk_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                  const LeleTensor* weight_int8, const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                                  const LeleTensor* bias, int32_t k, LeleBuf* out_ids, LeleBuf* out_logprob,
                                                  int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::TopK, k, true, input, row_offsets, count, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape,
                    out_rank);
}

/* ... and the log-probabilities of the columns the CALLER lists (forced alignment, rescoring): out_ids / out_logprob are the scored head's
 * bit for bit, out_at[r, u] = (v[r, cols[u]] - v[r, id_r]) + logprob[r], the k-best head's formula, from the same epilogue (igemm_kernel
 * EM 6): a lane whose column is listed stores the values it holds, the finish kernel rewrites them in place. */
int lele_hip_fused_quantized_linear_logprob_at(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                               const LeleTensor* weight_zero, const LeleTensor* bias, const int32_t* cols, int64_t ncols,
                                               LeleBuf* out_ids, LeleBuf* out_logprob, LeleBuf* out_at, int64_t* out_shape, int32_t* out_rank) {
    return fql_head(ctx, Head::At, 1, false, input, nullptr, 0, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape, out_rank,
                    cols, ncols, out_at);
}

int lele_hip_fused_quantized_linear_logprob_at_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                        const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                        const LeleTensor* weight_zero, const LeleTensor* bias, const int32_t* cols, int64_t ncols,
                                                        LeleBuf* out_ids, LeleBuf* out_logprob, LeleBuf* out_at, int64_t* out_shape,
                                                        int32_t* out_rank) {
    return fql_head(ctx, Head::At, 1, true, input, row_offsets, count, {weight_int8, weight_scale, weight_zero, bias}, out_ids, out_logprob, out_shape,
                    out_rank, cols, ncols, out_at);
}

int lele_hip_fused_quantized_linear_residual(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                             const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias,
                                             int apply_relu, const LeleTensor* res1, const LeleTensor* res2, LeleBuf* out,
                                             int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && weight_int8 && res1 && out, "fused_quantized_linear_residual: NULL argument");
    LELE_REQUIRE(res1->dtype == LELE_F32 && (!res2 || res2->dtype == LELE_F32), "fused_quantized_linear_residual: f32 residuals required");
    const int64_t n = weight_int8->shape[weight_int8->rank - 1];
    if (res_same_shape(input, n, res1) && (!res2 || res_same_shape(input, n, res2)))
        return fql_impl(ctx, input, {weight_int8, weight_scale, weight_zero, bias}, QReq{apply_relu, res1, res2}, out, out_shape, out_rank);
    // broadcasting residuals: the node sequence this op stands for -- the plain linear, then one `add` per residual with full
    // numpy broadcasting (a residual may broadcast OUTWARD: intermediates go to library-owned temporaries, the last sum to `out`)
    int64_t sh[LELE_MAX_RANK];
    int32_t r = 0;
    const int nres = res2 ? 2 : 1;
    LeleBuf *t0 = nullptr, *t1 = nullptr;
    LELE_TRY(ctx->tmp_buf(0, &t0));
    LELE_TRY(ctx->tmp_buf(1, &t1));
    LELE_TRY(fql_impl(ctx, input, {weight_int8, weight_scale, weight_zero, bias}, QReq{apply_relu}, t0, sh, &r));
    const char *const op = ctx->route[1], *const core = ctx->route[2];  // the linear's, put back behind the adds
    LeleBuf* cur = t0;
    for (int i = 0; i < nres; ++i) {
        const LeleTensor* res = i == 0 ? res1 : res2;
        LeleBuf* dst = i == nres - 1 ? out : (cur == t0 ? t1 : t0);
        LeleTensor t{cur->data, sh, r, LELE_F32, LELE_MEM_DEVICE};
        int64_t sh2[LELE_MAX_RANK];
        int32_t r2 = 0;
        LELE_TRY(lele_hip_binary(ctx, 0 /* add */, &t, res, dst, sh2, &r2));
        for (int d = 0; d < r2; ++d) sh[d] = sh2[d];
        r = r2;
        cur = dst;
    }
    ctx->set_route(op, core);
    calls_family(ctx);
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(sh, sh + r));
}

/* x1 = fused_quantized_linear[_residual](input, W.., relu, res1, res2);  x1n = layer_norm(x1, ln_scale, ln_bias, axis = -1, epsilon)
 * -- a projection, the Adds behind it and the LayerNorm that reads their sum (norm.rs:226 -> avx/norm.rs:10-133), bit for bit the
 * two calls.  Where a workgroup of the GEMM holds whole rows of the result (K = 512, N = 512 over a batch: igemm_as_kernel) the
 * normalisation runs in its epilogue; everywhere else the two calls are issued here.  res1 may be NULL (then res2 must be). */
int lele_hip_fused_quantized_linear_residual_ln(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                                const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias,
                                                int apply_relu, const LeleTensor* res1, const LeleTensor* res2, const LeleTensor* ln_scale,
                                                const LeleTensor* ln_bias, float epsilon, LeleBuf* out, LeleBuf* ln_out, int64_t* out_shape,
                                                int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && weight_int8 && ln_scale && ln_bias && out && ln_out, "fused_quantized_linear_residual_ln: NULL argument");
    LELE_REQUIRE(out != ln_out, "fused_quantized_linear_residual_ln: the sum and its normalised form need two buffers");
    LELE_REQUIRE(res1 || !res2, "fused_quantized_linear_residual_ln: res2 without res1");
    LELE_REQUIRE(input->rank >= 2 && weight_int8->rank >= 2, "fused_quantized_linear: rank >= 2 required");
    LnReq ln{ln_scale, ln_bias, epsilon, ln_out};
    int64_t sh[LELE_MAX_RANK];
    int32_t r = 0;
    const int64_t n = weight_int8->shape[weight_int8->rank - 1];
    // same-shape residuals: the call that may normalise in its epilogue
    if (!res1 || (res_same_shape(input, n, res1) && (!res2 || res_same_shape(input, n, res2))))
        LELE_TRY(fql_impl(ctx, input, {weight_int8, weight_scale, weight_zero, bias}, QReq{apply_relu, res1, res2, &ln}, out, sh, &r));
    else
        LELE_TRY(lele_hip_fused_quantized_linear_residual(ctx, input, weight_int8, weight_scale, weight_zero, bias, apply_relu, res1, res2, out, sh, &r));
    LELE_TRY(finish_ln(ctx, ln, out, sh, r));
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(sh, sh + r));
}

/* The output half of a SAN-M attention block (SenseVoice's encoder layer) as ONE call:
 *   mem = depthwise_conv1d_tlc(v_src, fsmn_w, fsmn_bias, x_offset, pad_left, pad_right, relu = 0, add_input = 1)     (FSMN memory + v)
 *   out = fused_quantized_linear_residual(input, W.., apply_relu, mem, res2);  ln_out = layer_norm(out, ln_scale, ln_bias, -1, epsilon)
 * bit for bit those three calls.  With K = N = 512 over a batch of utterances the GEMM's workgroup (one 32-row tile, all columns)
 * computes the memory block of its rows from a (32 + k - 1)-row window of v in LDS and normalises its rows in the epilogue:
 * three launches become one; every other shape issues the three calls. */
int lele_hip_sanm_out_block(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                            const LeleTensor* weight_zero, const LeleTensor* bias, int apply_relu, const LeleTensor* v_src,
                            const LeleTensor* fsmn_w, const LeleTensor* fsmn_bias, int64_t x_offset, int64_t pad_left, int64_t pad_right,
                            const LeleTensor* res2, const LeleTensor* ln_scale, const LeleTensor* ln_bias, float epsilon, LeleBuf* out,
                            LeleBuf* ln_out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && weight_int8 && v_src && fsmn_w && ln_scale && ln_bias && out && ln_out, "sanm_out_block: NULL argument");
    LELE_REQUIRE(out != ln_out, "sanm_out_block: the sum and its normalised form need two buffers");
    LELE_REQUIRE(input->rank >= 2 && weight_int8->rank >= 2, "fused_quantized_linear: rank >= 2 required");
    const QCall c = call_dims(input, {weight_int8, weight_scale, weight_zero, bias});
    // the one-launch form: the dense linear, asked for its LayerNorm and for the memory block as a first residual that the kernel computes
    LnReq ln{ln_scale, ln_bias, epsilon, ln_out};
    ln.fs_x = v_src, ln.fs_w = fsmn_w, ln.fs_b = fsmn_bias, ln.fs_pl = pad_left, ln.fs_off = x_offset;
    const QReq rq{apply_relu, nullptr, res2, &ln};
    auto one_launch = [&](const void* dout) { return fql_route(ctx, c, rq, staged_addr(input), dout) == QRoute::AsLnFsmn; };
    bool fused = env_int("LELE_HIP_FSMN_FUSED", 1) != 0 && c.kw == c.k && c.rows > 0 && fsmn_fits(c, v_src, fsmn_w, fsmn_bias, x_offset, pad_left, pad_right) &&
                 (!res2 || res_same_shape(input, c.n, res2)) && one_launch(nullptr);  // `out` is not touched unless all else holds
    if (fused) {
        LELE_TRY(out->reserve((size_t)c.rows * c.n * 4));
        fused = one_launch(out->data);
    }
    if (fused) return fql_impl(ctx, input, {weight_int8, weight_scale, weight_zero, bias}, rq, out, out_shape, out_rank);
    LeleBuf* mem = nullptr;
    LELE_TRY(ctx->tmp_buf(2, &mem));
    int64_t msh[LELE_MAX_RANK];
    int32_t mr = 0;
    LELE_TRY(lele_hip_depthwise_conv1d_tlc(ctx, v_src, x_offset, fsmn_w, fsmn_bias, pad_left, pad_right, 0, 1, mem, msh, &mr));
    LeleTensor mt{mem->data, msh, mr, LELE_F32, LELE_MEM_DEVICE};
    LELE_TRY(lele_hip_fused_quantized_linear_residual_ln(ctx, input, weight_int8, weight_scale, weight_zero, bias, apply_relu, &mt, res2, ln_scale,
                                                         ln_bias, epsilon, out, ln_out, out_shape, out_rank));
    calls_family(ctx);  // in front of the linear's route, which the call above left (or put back)
    return 0;
}

int lele_hip_fused_ffn_quantized(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* w1_int8, const LeleTensor* w1_scale,
                                 const LeleTensor* w1_zero, const LeleTensor* b1, const LeleTensor* w2_int8,
                                 const LeleTensor* w2_scale, const LeleTensor* w2_zero, const LeleTensor* b2, int apply_relu2,
                                 const LeleTensor* res1, const LeleTensor* res2, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    return ffn_impl(ctx, input, {w1_int8, w1_scale, w1_zero, b1}, {w2_int8, w2_scale, w2_zero, b2}, QReq{apply_relu2, res1, res2}, out, out_shape, out_rank);
}

/* out = fused_ffn_quantized(...);  ln_out = layer_norm(out, ln_scale, ln_bias, -1, epsilon) -- a transformer layer's feed-forward block,
 * its residual Add(s) and the LayerNorm of the NEXT half-layer that reads the sum, bit for bit the two calls.  On the register-stationary
 * route with 512 output columns the second product runs one row tile a workgroup (igemm_ask_kernel) and normalises in its epilogue. */
int lele_hip_fused_ffn_quantized_ln(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* w1_int8, const LeleTensor* w1_scale,
                                    const LeleTensor* w1_zero, const LeleTensor* b1, const LeleTensor* w2_int8, const LeleTensor* w2_scale,
                                    const LeleTensor* w2_zero, const LeleTensor* b2, int apply_relu2, const LeleTensor* res1,
                                    const LeleTensor* res2, const LeleTensor* ln_scale, const LeleTensor* ln_bias, float epsilon, LeleBuf* out,
                                    LeleBuf* ln_out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && ln_scale && ln_bias && out && ln_out, "fused_ffn_quantized_ln: NULL argument");
    LELE_REQUIRE(out != ln_out, "fused_ffn_quantized_ln: the sum and its normalised form need two buffers");
    LnReq ln{ln_scale, ln_bias, epsilon, ln_out};
    int64_t sh[LELE_MAX_RANK];
    int32_t r = 0;
    LELE_TRY(ffn_impl(ctx, input, {w1_int8, w1_scale, w1_zero, b1}, {w2_int8, w2_scale, w2_zero, b2}, QReq{apply_relu2, res1, res2, &ln}, out, sh, &r));
    LELE_TRY(finish_ln(ctx, ln, out, sh, r));
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(sh, sh + r));
}

/* ---- per-stage stopwatch of fused_quantized_linear (bench.py's roofline block for the model path) ------------------- */
int lele_hip_quant_set_profiling(LeleCtx* ctx, int on) {
    LELE_REQUIRE(ctx, "quant_set_profiling: ctx is NULL");
    ctx->qprof.on = on != 0;
    ctx->qprof.used = 0;
    return 0;
}
int lele_hip_quant_profile_read(LeleCtx* ctx, float* range_ms, float* quantise_ms, float* gemm_ms, int64_t* calls) {
    LELE_REQUIRE(ctx && range_ms && quantise_ms && gemm_ms && calls, "quant_profile_read: NULL argument");
    LELE_REQUIRE(!ctx->capturing, "quant_profile_read: not allowed while a graph is being captured");
    LELE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    double t[3] = {0, 0, 0};
    auto& p = ctx->qprof;
    const size_t n = p.used / 4;
    for (size_t i = 0; i < n; ++i)
        for (int st = 0; st < 3; ++st) {
            float ms = 0.0f;
            LELE_HIP_CHECK(hipEventElapsedTime(&ms, p.ev[4 * i + st], p.ev[4 * i + st + 1]));
            t[st] += ms;
        }
    *calls = (int64_t)n;
    *range_ms = n ? (float)(t[0] / n) : 0.0f;
    *quantise_ms = n ? (float)(t[1] / n) : 0.0f;
    *gemm_ms = n ? (float)(t[2] / n) : 0.0f;
    p.used = 0;
    return 0;
}

/* ---- prepared weights: prepare_weights (quantization.rs:221), mat_mul_integer_prepared (699), fused_dq_gemm_prepared_x86
 *      (454), mat_mul_integer_u8_weights (173).  The handle owns the device copy of the RAW u8 matrix carried as f32 (the
 *      encoding every other entry point takes) and marks it immutable, so the packed forms are built once and cached. ---- */
struct LelePrepared {
    LeleCtx* ctx;
    std::vector<float> host;  // u8 values as f32 [k, n]: the LELE_MEM_WEIGHT identity of this matrix
    int64_t k, n;
    int64_t shape[2];
};
int lele_hip_prepare_weights(LeleCtx* ctx, const uint8_t* b_u8, int64_t k, int64_t n, LelePrepared** out) {
    LELE_REQUIRE(ctx && b_u8 && out, "prepare_weights: NULL argument");
    LELE_REQUIRE(k > 0 && n > 0, "prepare_weights: empty matrix (k=%lld, n=%lld)", (long long)k, (long long)n);
    LelePrepared* p = new LelePrepared();
    p->ctx = ctx;
    p->k = k;
    p->n = n;
    p->shape[0] = k;
    p->shape[1] = n;
    p->host.resize((size_t)k * n);
    for (int64_t i = 0; i < k * n; ++i) p->host[i] = (float)b_u8[i];
    *out = p;
    return 0;
}
int lele_hip_prepared_destroy(LelePrepared* p) {
    if (!p) return 0;
    // free every cached form of this matrix, so a recycled host address cannot alias
    LeleCtx* c = p->ctx;
    (void)hipStreamSynchronize(c->stream);
    c->drop_weights(p->host.data());
    delete p;
    return 0;
}
static LeleTensor prepared_tensor(const LelePrepared* p) {
    return LeleTensor{p->host.data(), p->shape, 2, LELE_F32, LELE_MEM_WEIGHT};
}
int lele_hip_mat_mul_integer_prepared(LeleCtx* ctx, const LeleTensor* a, const LelePrepared* pw, int has_a_zero_point,
                                      float a_zero_point, int has_b_zero_point, int32_t b_zero_point, const LeleTensor* scale,
                                      const LeleTensor* bias, int apply_relu, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && pw && out, "mat_mul_integer_prepared: NULL argument");
    const LeleTensor b = prepared_tensor(pw);
    const float za = has_a_zero_point ? a_zero_point : 0.0f, zb = has_b_zero_point ? (float)(b_zero_point & 0xff) : 0.0f;
    const int64_t one = 1;
    const LeleTensor tza{&za, &one, 1, LELE_F32, LELE_MEM_HOST}, tzb{&zb, &one, 1, LELE_F32, LELE_MEM_HOST};
    return lele_hip_mat_mul_integer_with_scale_bias(ctx, a, &b, &tza, &tzb, scale, bias, apply_relu, out, out_shape, out_rank);
}
int lele_hip_fused_dq_gemm_prepared(LeleCtx* ctx, const LeleTensor* input, const LelePrepared* pw, int has_b_zero_point,
                                    int32_t b_zero_point, const LeleTensor* weight_scale, const LeleTensor* bias, int apply_relu,
                                    LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && input && pw && weight_scale && out, "fused_dq_gemm_prepared: NULL argument");
    const LeleTensor b = prepared_tensor(pw);
    const float zb = has_b_zero_point ? (float)(b_zero_point & 0xff) : 0.0f;
    const int64_t one = 1;
    const LeleTensor tzb{&zb, &one, 1, LELE_F32, LELE_MEM_HOST};
    return lele_hip_fused_quantized_linear(ctx, input, &b, weight_scale, &tzb, bias, apply_relu, out, out_shape, out_rank);
}

int lele_hip_dynamic_quantize_linear(LeleCtx* ctx, const LeleTensor* x, LeleBuf* out_y, LeleBuf* out_scale,
                                     LeleBuf* out_zp, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && x && out_y && out_scale && out_zp, "dynamic_quantize_linear: NULL argument");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t len = numel(x);
    std::vector<int64_t> shp(x->shape, x->shape + x->rank);
    LELE_TRY(out_y->reserve((size_t)len * 4));
    LELE_TRY(out_scale->reserve(4));
    LELE_TRY(out_zp->reserve(4));
    ctx->set_route(len ? "dql.w1" : nullptr);
    if (len == 0) {  // avx/quantization.rs:845-851: scale 1.0, zero point 0.0
        const float one = 1.0f, zero = 0.0f;
        LELE_HIP_CHECK(hipMemcpyAsync(out_scale->data, &one, 4, hipMemcpyHostToDevice, ctx->stream));
        LELE_HIP_CHECK(hipMemcpyAsync(out_zp->data, &zero, 4, hipMemcpyHostToDevice, ctx->stream));
        LELE_REQUIRE(!ctx->capturing, "graph capture: this op must run once eagerly first (it allocates or synchronises)");
        LELE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return set_shape_v(out_shape, out_rank, shp);
    }
    LELE_TRY(ctx->arena_reset());
    const void* dx = nullptr;
    LELE_TRY(ctx->dev_ptr(x, &dx));
    void* prm = nullptr;
    LELE_TRY(ctx->arena_alloc(sizeof(QParams), &prm));
    LELE_TRY(launch_range(ctx, (const float*)dx, 1, len, (QParams*)prm, (float*)out_scale->data, (float*)out_zp->data));
    const int blocks = (int)std::min<int64_t>((len + 255) / 256, 2048);
    hipLaunchKernelGGL(dq_apply_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const float*)dx, len,
                       (const QParams*)prm, (float*)out_y->data);
    LELE_HIP_CHECK(hipGetLastError());
    return set_shape_v(out_shape, out_rank, shp);
}

int lele_hip_mat_mul_integer_with_scale_bias(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b,
                                             const LeleTensor* a_zero_point, const LeleTensor* b_zero_point,
                                             const LeleTensor* scale, const LeleTensor* bias, int apply_relu,
                                             LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && b && out, "mat_mul_integer: NULL argument");
    LELE_REQUIRE(a->rank >= 2 && b->rank >= 2, "mat_mul_integer: rank >= 2 required");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t m = a->shape[a->rank - 2], k = a->shape[a->rank - 1];
    const int64_t kb = b->shape[b->rank - 2], n = b->shape[b->rank - 1];
    LELE_REQUIRE(k == kb, "mat_mul_integer: K mismatch (%lld vs %lld)", (long long)k, (long long)kb);
    int64_t batch_a = 1, batch_b = 1;
    for (int i = 0; i + 2 < a->rank; ++i) batch_a *= a->shape[i];
    for (int i = 0; i + 2 < b->rank; ++i) batch_b *= b->shape[i];
    LELE_REQUIRE(batch_a == batch_b || batch_a == 1 || batch_b == 1, "mat_mul_integer: batch %lld vs %lld",
                 (long long)batch_a, (long long)batch_b);
    const int64_t fb = std::max(batch_a, batch_b);
    std::vector<int64_t> shp;
    if (batch_a >= batch_b)
        shp.assign(a->shape, a->shape + a->rank - 2);
    else
        shp.assign(b->shape, b->shape + b->rank - 2);
    shp.push_back(m);
    shp.push_back(n);
    LELE_TRY(out->reserve((size_t)fb * m * n * 4));
    ctx->set_route(nullptr);  // lele_hip_last_route: "" for a call that launches nothing
    if (fb * m * n == 0) return set_shape_v(out_shape, out_rank, shp);
    float za = 0.0f, zb = 0.0f;  // `.data.first().map(|&v| v as i32).unwrap_or(0)`
    LELE_TRY(first_scalar_of(ctx, a_zero_point, &za));
    LELE_TRY(first_scalar_of(ctx, b_zero_point, &zb));
    const int zp_a = (int)za, zp_b = (int)zb;
    const int64_t slen = scale ? numel(scale) : 0, blen = bias ? numel(bias) : 0;
    LELE_REQUIRE(!scale || slen == 1 || slen >= n, "mat_mul_integer: scale has %lld entries for N=%lld",
                 (long long)slen, (long long)n);
    LELE_REQUIRE(!bias || blen >= n, "mat_mul_integer: bias has %lld entries for N=%lld", (long long)blen, (long long)n);
    LELE_TRY(ctx->arena_reset());
    const void *da = nullptr, *db = nullptr, *ds = nullptr, *dbi = nullptr;
    LELE_TRY(ctx->dev_ptr(a, &da));
    LELE_TRY(ctx->dev_ptr(b, &db));
    if (scale) LELE_TRY(ctx->dev_ptr(scale, &ds));
    if (bias) LELE_TRY(ctx->dev_ptr(bias, &dbi));
    const int kp = (int)((k + 15) & ~int64_t(15));
    PackedW pw;
    LELE_TRY(packed_weights_of(ctx, b, (const float*)db, batch_b, (int)k, (int)n, kp, &pw));
    const int64_t rows_a = batch_a * m;
    void *aq = nullptr, *rs = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)rows_a * kp, &aq));
    LELE_TRY(ctx->arena_alloc((size_t)rows_a * 4, &rs));
    hipLaunchKernelGGL(qrows_kernel<1>, dim3((unsigned)((rows_a + 3) / 4)), dim3(256), 0, ctx->stream, (const float*)da,
                       rows_a, (int)k, kp, (int)m, (QParams*)nullptr, (int8_t*)aq, (int*)rs, (const float*)nullptr, 0, (unsigned*)nullptr, (int*)nullptr);
    // one launch per batch slice unless everything is un-batched on the B side (then all rows share the weights)
    const int64_t launches = (batch_b == 1 && batch_a >= 1) ? 1 : fb;
    for (int64_t bi = 0; bi < launches; ++bi) {
        const int64_t rows = launches == 1 ? rows_a : m;
        const int8_t* aptr = (const int8_t*)aq + (launches == 1 || batch_a == 1 ? 0 : bi * m * kp);
        const int* rsp = (const int*)rs + (launches == 1 || batch_a == 1 ? 0 : bi * m);
        IgemmEpi epi{(float*)out->data + (launches == 1 ? 0 : bi * m * n), rows, n, (int)m, (int)k, rsp,
                     pw.col_sums + (batch_b == 1 ? 0 : bi * n), nullptr, zp_a, zp_b, (const float*)ds, (int)slen,
                     (const float*)dbi, apply_relu};
        const char* core = nullptr;
        LELE_TRY(launch_igemm(ctx, aptr, pw.wt + (batch_b == 1 ? 0 : bi * n * kp), rows, (int)n, kp, (int)m, epi, &core));
        ctx->set_route("mmi.rows", core);  // a batched B: the last slice's launch
    }
    return set_shape_v(out_shape, out_rank, shp);
}

}  // extern "C"
