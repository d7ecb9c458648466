// rnn.hip -- LSTM / GRU forward (one direction; batch 1, or a packed batch of independent sequences) on gfx950.
//
//   lele_hip_lstm <- /root/reference/src/kernels/rnn.rs:67-231 (gate math 15-65)
//   lele_hip_gru  <- /root/reference/src/kernels/rnn.rs:246-357 (gate fusion 359-432)
//
// The reference runs, per time step, two faer GEMVs (W x_t, R h_{t-1}) and an AVX2 gate pass.  The recurrence is
// inherently serial in t, so the device splits it differently:
//   1. W x_t does not depend on the recurrence -> ONE MFMA GEMM for all T steps ([T, I] x [I, G] -> WX[T, G]).
//   2. R is transposed once ([H, G]) so that lane g of the recurrent GEMV reads R^T[k][g]: coalesced across lanes,
//      and the k loop of one lane is a plain FMA chain with independent loads (no cross-lane reduction per row).
//   3. One persistent 1024-thread workgroup walks t = 0..T-1 with h, c and the per-step gate pre-activations in
//      LDS; R^T (G*H*4 bytes, 256 KB for the VAD-sized LSTM) stays L2-resident across steps.
// Gate math follows the x86 code exactly: the same association of the adds, polynomial sigmoid/tanh for hidden
// indices k < (H & ~7), libm for the tail, fma for c_t / h_t.  The GRU always evaluates the linear_before_reset = 1
// form, as gru_gate_fusion_avx2 does regardless of its flag (rnn.rs:366, 393-407); the flag is accepted and ignored.
//
//   lele_hip_lstm_segments / lele_hip_gru_segments: the same over a packed batch of INDEPENDENT sequences (x [R, I] + row offsets),
//   every segment bit for bit the single call on it alone.  W x of all R rows is one GEMM of one FIXED tile form (a route that moved
//   with R would make a segment's bits depend on its neighbours); one workgroup per group of up to NS segments walks them in
//   lockstep (rnn_seg_kernel below), with the recurrent weights in registers where a thread's slice is 16, 32 or 64 values (LSTM H = 64
//   and 128, GRU H = 96 and 128) and streamed from the transposed copy otherwise.  DESIGN.md 3.5b.
//   Every entry point records its route (lele_hip_last_route): rnn.lstm / rnn.gru + the GEMM kernel of W x; rnns.lstm / rnns.gru + the form.
#include "common.h"
#include "gemm_core.h"
#include "simd_math.h"

#include <math.h>

#include <algorithm>
#include <tuple>

using namespace lele;

namespace {

constexpr int kRnnThreads = 1024;

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int r = r0 + j, c = c0 + threadIdx.x;
        tile[j][threadIdx.x] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0.0f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = c0 + j, r = r0 + threadIdx.x;
        if (r < rows && c < cols) dst[(int64_t)c * rows + r] = tile[threadIdx.x][j];
    }
}

__device__ __forceinline__ float sigmoid_tail(float x) { return 1.0f / (1.0f + expf(-x)); }  // activations.rs sigmoid

// MODE 0 = LSTM (NG = 4 gates: i, o, f, c), MODE 1 = GRU (NG = 3: z, r, h)
template <int MODE>
__global__ __launch_bounds__(kRnnThreads) void rnn_kernel(const float* __restrict__ wx /*[T,G]*/,
                                                          const float* __restrict__ rt /*[H,G]*/,
                                                          const float* __restrict__ bias /*[2G] or null*/,
                                                          const float* __restrict__ h0, const float* __restrict__ c0,
                                                          float* __restrict__ y, float* __restrict__ hout,
                                                          float* __restrict__ cout, int T, int H, int S) {
    constexpr int NG = MODE == 0 ? 4 : 3;
    const int G = NG * H;
    extern __shared__ float lds[];
    float* h = lds;           // [H]
    float* c = lds + H;       // [H] (LSTM only)
    float* part = c + H;      // [S][G] partial recurrent sums
    const int tid = threadIdx.x;
    for (int k = tid; k < H; k += kRnnThreads) {
        h[k] = h0 ? h0[k] : 0.0f;
        c[k] = (MODE == 0 && c0) ? c0[k] : 0.0f;
    }
    __syncthreads();
    const int body = H & ~7;
    for (int t = 0; t < T; ++t) {
        // recurrent GEMV: thread (s, g) sums k in [s*H/S, (s+1)*H/S)
        for (int idx = tid; idx < S * G; idx += kRnnThreads) {
            const int s = idx / G, g = idx - s * G;
            const int k0 = (int)((int64_t)s * H / S), k1 = (int)((int64_t)(s + 1) * H / S);
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            int k = k0;
            for (; k + 4 <= k1; k += 4) {
                a0 = fmaf_(rt[(int64_t)(k + 0) * G + g], h[k + 0], a0);
                a1 = fmaf_(rt[(int64_t)(k + 1) * G + g], h[k + 1], a1);
                a2 = fmaf_(rt[(int64_t)(k + 2) * G + g], h[k + 2], a2);
                a3 = fmaf_(rt[(int64_t)(k + 3) * G + g], h[k + 3], a3);
            }
            for (; k < k1; ++k) a0 = fmaf_(rt[(int64_t)k * G + g], h[k], a0);
            part[idx] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        const float* wxt = wx + (int64_t)t * G;
        for (int k = tid; k < H; k += kRnnThreads) {
            float rc[NG], wc[NG], bw[NG], br[NG];
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                float acc = part[q * H + k];
                for (int s = 1; s < S; ++s) acc += part[s * G + q * H + k];
                rc[q] = acc;
                wc[q] = wxt[q * H + k];
                bw[q] = bias ? bias[q * H + k] : 0.0f;
                br[q] = bias ? bias[G + q * H + k] : 0.0f;
            }
            const bool poly = k < body;
            float ht;
            if (MODE == 0) {
                float gate[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) gate[q] = ((wc[q] + rc[q]) + bw[q]) + br[q];  // rnn.rs:152-154
                float ct;
                if (poly) {  // lstm_gates_avx2, rnn.rs:26-63
                    const float ig = sigmoid_poly(gate[0]), og = sigmoid_poly(gate[1]), fg = sigmoid_poly(gate[2]);
                    const float cg = tanh_poly(gate[3]);
                    ct = fmaf_(fg, c[k], ig * cg);
                    ht = og * tanh_poly(ct);
                } else {  // scalar tail, rnn.rs:52-63
                    const float ig = sigmoid_tail(gate[0]), og = sigmoid_tail(gate[1]), fg = sigmoid_tail(gate[2]);
                    const float cg = tanhf(gate[3]);
                    ct = fg * c[k] + ig * cg;
                    ht = og * tanhf(ct);
                }
                c[k] = ct;
            } else {
                if (poly) {  // gru_gate_fusion_avx2, rnn.rs:373-416
                    const float z = sigmoid_poly((wc[0] + rc[0]) + (bw[0] + br[0]));
                    const float rg = sigmoid_poly((wc[1] + rc[1]) + (bw[1] + br[1]));
                    const float hg = tanh_poly((wc[2] + bw[2]) + rg * (rc[2] + br[2]));
                    ht = fmaf_(1.0f - z, hg, z * h[k]);
                } else {  // rnn.rs:418-431
                    const float z = sigmoid_tail(((wc[0] + rc[0]) + bw[0]) + br[0]);
                    const float rg = sigmoid_tail(((wc[1] + rc[1]) + bw[1]) + br[1]);
                    const float hg = tanhf((wc[2] + bw[2]) + rg * (rc[2] + br[2]));
                    ht = (1.0f - z) * hg + z * h[k];
                }
            }
            h[k] = ht;  // only this thread reads h[k] in the gate phase; the next GEMV starts after the barrier
            y[(int64_t)t * H + k] = ht;
        }
        __syncthreads();
    }
    for (int k = tid; k < H; k += kRnnThreads) {
        hout[k] = h[k];
        if (MODE == 0) cout[k] = c[k];
    }
}

// what lele_hip_lstm / _gru and their *_segments forms check alike: W [1, G, I], R [1, G, H], the bias and the initial state of
// `states` sequences; gives H, G = gates * H, the k-slices S a gate row is summed in and the LDS bytes of one sequence
template <int MODE>
int check_rnn_weights(const char* name, const LeleTensor* w, const LeleTensor* r, const LeleTensor* bias, const LeleTensor* h0,
                      const LeleTensor* c0, int64_t I, int64_t states, int64_t* Hp, int64_t* Gp, int* Sp, size_t* lds_bytes) {
    constexpr int NG = MODE == 0 ? 4 : 3;
    const int64_t H = w->shape[1] / NG, G = NG * H;
    LELE_REQUIRE(w->shape[1] == G && w->shape[2] == I, "%s: W shape mismatch", name);
    LELE_REQUIRE(r->shape[0] == 1 && r->shape[1] == G && r->shape[2] == H, "%s: R shape mismatch", name);
    if (bias) LELE_REQUIRE(numel(bias) == 2 * G, "%s: bias must hold %lld values", name, (long long)(2 * G));
    if (h0) LELE_REQUIRE(numel(h0) == states * H, "%s: initial_h must hold %lld values", name, (long long)(states * H));
    if (c0) LELE_REQUIRE(numel(c0) == states * H, "%s: initial_c must hold %lld values", name, (long long)(states * H));
    LELE_REQUIRE(H >= 1, "%s: hidden_size must be positive", name);
    int S = (int)std::max<int64_t>(1, kRnnThreads / G);
    S = (int)std::min<int64_t>(S, H);
    *lds_bytes = (size_t)(2 * H + (int64_t)S * G) * 4;
    LELE_REQUIRE(*lds_bytes <= 160 * 1024, "%s: hidden_size %lld exceeds the LDS-resident state limit", name, (long long)H);
    *Hp = H;
    *Gp = G;
    *Sp = S;
    return 0;
}

// R transposed: once per weight when the caller declared it immutable (a streaming model calls this for every chunk)
int rnn_rt(LeleCtx* ctx, const LeleTensor* r, const void* dr, int64_t G, int64_t H, void** rt) {
    return ctx->weight_form(r, WeightForm::RnnRT, {}, (size_t)G * H * 4, rt, [&](void* d) {
        hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((H + 31) / 32), (unsigned)((G + 31) / 32)), dim3(32, 8), 0, ctx->stream,
                           (const float*)dr, (float*)d, (int)G, (int)H);
        LELE_HIP_CHECK(hipGetLastError());
        return 0;
    });
}

template <int MODE>
int run_rnn(LeleCtx* ctx, const char* name, const LeleTensor* x, const LeleTensor* w, const LeleTensor* r,
            const LeleTensor* bias, const LeleTensor* h0, const LeleTensor* c0, LeleBuf* y, LeleBuf* hn, LeleBuf* cn,
            int64_t* y_shape, int32_t* y_rank) {
    constexpr int NG = MODE == 0 ? 4 : 3;
    LELE_REQUIRE(ctx && x && w && r && y && hn && (MODE == 1 || cn), "%s: NULL argument", name);
    LELE_REQUIRE(x->rank == 3 && w->rank == 3 && r->rank == 3, "%s: expected X [T,B,I], W [D,%dH,I], R [D,%dH,H]", name,
                 NG, NG);
    LELE_REQUIRE(x->dtype == LELE_F32 && w->dtype == LELE_F32 && r->dtype == LELE_F32, "%s: f32 tensors required", name);
    LELE_REQUIRE(w->shape[0] == 1, "%s: Only num_directions=1 supported", name);  // rnn.rs:86, 266
    LELE_REQUIRE(x->shape[1] == 1, "%s: Only batch_size=1 supported", name);     // rnn.rs:89, 269
    const int64_t T = x->shape[0], I = x->shape[2];
    int64_t H = 0, G = 0;
    int S = 0;
    size_t lds_bytes = 0;
    LELE_TRY(check_rnn_weights<MODE>(name, w, r, bias, h0, c0, I, 1, &H, &G, &S, &lds_bytes));
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dw = nullptr, *dr = nullptr, *db = nullptr, *dh0 = nullptr, *dc0 = nullptr;
    LELE_TRY(ctx->dev_ptr(x, &dx));
    LELE_TRY(ctx->dev_ptr(w, &dw));
    LELE_TRY(ctx->dev_ptr(r, &dr));
    if (bias) LELE_TRY(ctx->dev_ptr(bias, &db));
    if (h0) LELE_TRY(ctx->dev_ptr(h0, &dh0));
    if (c0) LELE_TRY(ctx->dev_ptr(c0, &dc0));
    void *wx = nullptr, *rt = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)std::max<int64_t>(1, T * G) * 4, &wx));
    LELE_TRY(rnn_rt(ctx, r, dr, G, H, &rt));
    LELE_TRY(y->reserve((size_t)T * H * 4));
    LELE_TRY(hn->reserve((size_t)H * 4));
    if (MODE == 0) LELE_TRY(cn->reserve((size_t)H * 4));
    const char* wx_route = nullptr;  // lele_hip_last_route: rnn.lstm / rnn.gru, then the GEMM kernel of W x (none for T == 0)
    if (T > 0) {
        gemm::LoadRowK al{(const float*)dx, 0, I, (int)T, (int)I, (int)((((uintptr_t)dx & 15) == 0) && I % 4 == 0)};
        gemm::LoadRowK bl{(const float*)dw, 0, I, (int)G, (int)I, (int)((((uintptr_t)dw & 15) == 0) && I % 4 == 0)};
        gemm::EpiAffine epi{(float*)wx, 0, (int)T, (int)G, 1.0f, 0.0f, nullptr, gemm::C_NONE, 1};
        wx_route = gemm::launch(ctx->stream, al, bl, epi, (int)T, (int)G, (int)I, 1, ctx->num_cus);
    }
    ctx->set_route(MODE == 0 ? "rnn.lstm" : "rnn.gru", wx_route);
    LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(&rnn_kernel<MODE>), 160 * 1024));
    hipLaunchKernelGGL(rnn_kernel<MODE>, dim3(1), dim3(kRnnThreads), lds_bytes, ctx->stream, (const float*)wx,
                       (const float*)rt, (const float*)db, (const float*)dh0, (const float*)dc0, (float*)y->data,
                       (float*)hn->data, MODE == 0 ? (float*)cn->data : nullptr, (int)T, (int)H, S);
    LELE_HIP_CHECK(hipGetLastError());
    return set_shape(y_shape, y_rank, {T, 1, 1, H});  // rnn.rs:223, 352; h / c are [1, 1, H]
}

// ---------------------------------------------------------------------------------------------------- the packed batch
// rnn_kernel over a GROUP of up to NS independent sequences walked in lockstep: a 1024-thread workgroup per group, `ns` members
// {first row, rows, segment index} from the layout's table (longest first; a member past its end, or a padding slot, is masked: its
// GEMV sums are computed and dropped).  Every statement that produces a value is rnn_kernel's: the k-slices and their bounds, the four
// accumulators of a slice joined (a0 + a1) + (a2 + a3), the slices added in ascending s, the gate association, polynomial body and
// libm tail -- what a member computes does not depend on NS, on the form or on who shares its workgroup.
//   KS > 0 (register-stationary): H = S * KS, S * G <= 1024.  Thread (s, g) keeps r[g][s*KS .. s*KS + KS) in registers over all steps
//           and all members; h is read from LDS as float4 broadcasts, one register operand feeds NS chains of 4 accumulators.
//   KS = 0 (streamed): rnn_kernel's loop over the transposed R^T in L2, one load feeding the NS members' chains.
// LDS: h[ns][H], c[ns][H], part[ns][S * G]; slots j >= ns of the NS-wide register tiles read member 0's h and store nothing.
template <int MODE, int NS, int KS>
__global__ __launch_bounds__(kRnnThreads) void rnn_seg_kernel(const float* __restrict__ wx /*[R,G]*/,
                                                              const float* __restrict__ rw /*KS > 0: r [G,H]; else rt [H,G]*/,
                                                              const float* __restrict__ bias /*[2G] or null*/,
                                                              const float* h0 /*[count,H] or null; may alias hout*/,
                                                              const float* c0, float* __restrict__ y /*[R,H]*/, float* hout,
                                                              float* cout, const int4* __restrict__ groups, int ns, int H, int S) {
    constexpr int NG = MODE == 0 ? 4 : 3;
    const int G = NG * H, SG = S * G;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* h = lds;                // [ns][H]
    float* c = lds + ns * H;       // [ns][H] (LSTM only)
    float* part = c + ns * H;      // [ns][S][G] partial recurrent sums
    const int tid = threadIdx.x;
    groups += (int64_t)blockIdx.x * ns;  // this workgroup's members (read from global memory: all 160 KiB of LDS may be state)
    for (int idx = tid; idx < ns * H; idx += kRnnThreads) {
        const int j = idx / H, k = idx - j * H, seg = groups[j].z;
        h[idx] = (h0 && seg >= 0) ? h0[(int64_t)seg * H + k] : 0.0f;
        c[idx] = (MODE == 0 && c0 && seg >= 0) ? c0[(int64_t)seg * H + k] : 0.0f;
    }
    const int T = groups[0].y;  // the longest member comes first
    const int4 m0 = groups[tid < ns * H ? tid / H : 0];  // the member of this thread's first gate item, the same at every step
    int hoff[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) hoff[j] = (j < ns ? j : 0) * H;
    float rr[KS > 0 ? KS : 1];
    const int ft = tid < SG ? tid : 0;          // form 1: threads past S * G hold thread 0's weights and compute nothing
    const int sl = ft / G, col = ft - sl * G;   // this thread's slice and gate column
    if (KS > 0) {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) rr[kk] = rw[(int64_t)col * H + sl * KS + kk];
    }
    __syncthreads();
    const int body = H & ~7;
    for (int t = 0; t < T; ++t) {
        if (KS > 0) {
            if (tid < SG) {
                // two members at a time (NS = 2 here): 64 weights + 8 accumulators + two float4 of h per member, the next chunk's
                // loaded before the current one's FMAs; the empty asm pins every chunk's FMAs in place, or the compiler hoists every LDS
                // read of the unrolled loop to the top (all NS members at once spills: DESIGN.md 3.5b)
                for (int jb = 0; jb < ns; jb += NS) {
                    const float* hj[NS];
                    float a[NS][4];
                    float4 cur[NS], nxt[NS];
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        hj[j] = h + (jb + j < ns ? jb + j : 0) * H + sl * KS;
                        a[j][0] = a[j][1] = a[j][2] = a[j][3] = 0.0f;
                        cur[j] = *reinterpret_cast<const float4*>(hj[j]);
                    }
#pragma unroll
                    for (int kk = 0; kk < KS; kk += 4) {
#pragma unroll
                        for (int j = 0; j < NS; ++j)
                            if (kk + 4 < KS) nxt[j] = *reinterpret_cast<const float4*>(hj[j] + kk + 4);
#pragma unroll
                        for (int j = 0; j < NS; ++j) {
                            a[j][0] = fmaf_(rr[kk + 0], cur[j].x, a[j][0]);
                            a[j][1] = fmaf_(rr[kk + 1], cur[j].y, a[j][1]);
                            a[j][2] = fmaf_(rr[kk + 2], cur[j].z, a[j][2]);
                            a[j][3] = fmaf_(rr[kk + 3], cur[j].w, a[j][3]);
                            cur[j] = nxt[j];
                            asm volatile("" : "+v"(a[j][0]), "+v"(a[j][1]), "+v"(a[j][2]), "+v"(a[j][3])::"memory");  // see above
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NS; ++j)
                        if (jb + j < ns) part[(jb + j) * SG + tid] = (a[j][0] + a[j][1]) + (a[j][2] + a[j][3]);
                }
            }
        } else {
            for (int idx = tid; idx < SG; idx += kRnnThreads) {
                const int s = idx / G, g = idx - s * G;
                const int k0 = (int)((int64_t)s * H / S), k1 = (int)((int64_t)(s + 1) * H / S);
                float a[NS][4];
#pragma unroll
                for (int j = 0; j < NS; ++j) a[j][0] = a[j][1] = a[j][2] = a[j][3] = 0.0f;
                int k = k0;
                for (; k + 4 <= k1; k += 4) {
                    const float r0 = rw[(int64_t)(k + 0) * G + g], r1 = rw[(int64_t)(k + 1) * G + g];
                    const float r2 = rw[(int64_t)(k + 2) * G + g], r3 = rw[(int64_t)(k + 3) * G + g];
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const float* hj = h + hoff[j] + k;
                        a[j][0] = fmaf_(r0, hj[0], a[j][0]);
                        a[j][1] = fmaf_(r1, hj[1], a[j][1]);
                        a[j][2] = fmaf_(r2, hj[2], a[j][2]);
                        a[j][3] = fmaf_(r3, hj[3], a[j][3]);
                    }
                }
                for (; k < k1; ++k) {
                    const float rv = rw[(int64_t)k * G + g];
#pragma unroll
                    for (int j = 0; j < NS; ++j) a[j][0] = fmaf_(rv, h[hoff[j] + k], a[j][0]);
                }
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j < ns) part[j * SG + idx] = (a[j][0] + a[j][1]) + (a[j][2] + a[j][3]);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < ns * H; idx += kRnnThreads) {
            const int j = idx / H, k = idx - j * H;
            const int4 m = idx == tid ? m0 : groups[j];
            if (t >= m.y) continue;  // this member has ended: its state stays
            const float* pj = part + j * SG;
            const float* wxt = wx + (int64_t)(m.x + t) * G;
            float rc[NG], wc[NG], bw[NG], br[NG];
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                float acc = pj[q * H + k];
                for (int s = 1; s < S; ++s) acc += pj[s * G + q * H + k];
                rc[q] = acc;
                wc[q] = wxt[q * H + k];
                bw[q] = bias ? bias[q * H + k] : 0.0f;
                br[q] = bias ? bias[G + q * H + k] : 0.0f;
            }
            // KS = 64 holds 64 weights per lane over this phase: one activation at a time, or the interleaved polynomials spill them
            auto fence = [] {
                if (KS >= 64) __builtin_amdgcn_sched_barrier(0);
            };
            const bool poly = KS > 0 || k < body;  // KS > 0: H = S * KS is a multiple of 16, there is no tail (and no libm code to hold registers)
            float ht;
            fence();
            if (MODE == 0) {
                float gate[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) gate[q] = ((wc[q] + rc[q]) + bw[q]) + br[q];  // rnn.rs:152-154
                float ct;
                if (poly) {  // lstm_gates_avx2, rnn.rs:26-63
                    fence();
                    const float ig = sigmoid_poly(gate[0]);
                    fence();
                    const float og = sigmoid_poly(gate[1]);
                    fence();
                    const float fg = sigmoid_poly(gate[2]);
                    fence();
                    const float cg = tanh_poly(gate[3]);
                    fence();
                    ct = fmaf_(fg, c[idx], ig * cg);
                    ht = og * tanh_poly(ct);
                } else {  // scalar tail, rnn.rs:52-63
                    const float ig = sigmoid_tail(gate[0]), og = sigmoid_tail(gate[1]), fg = sigmoid_tail(gate[2]);
                    const float cg = tanhf(gate[3]);
                    ct = fg * c[idx] + ig * cg;
                    ht = og * tanhf(ct);
                }
                c[idx] = ct;
            } else {
                if (poly) {  // gru_gate_fusion_avx2, rnn.rs:373-416
                    const float z = sigmoid_poly((wc[0] + rc[0]) + (bw[0] + br[0]));
                    fence();
                    const float rg = sigmoid_poly((wc[1] + rc[1]) + (bw[1] + br[1]));
                    fence();
                    const float hg = tanh_poly((wc[2] + bw[2]) + rg * (rc[2] + br[2]));
                    fence();
                    ht = fmaf_(1.0f - z, hg, z * h[idx]);
                } else {  // rnn.rs:418-431
                    const float z = sigmoid_tail(((wc[0] + rc[0]) + bw[0]) + br[0]);
                    const float rg = sigmoid_tail(((wc[1] + rc[1]) + bw[1]) + br[1]);
                    const float hg = tanhf((wc[2] + bw[2]) + rg * (rc[2] + br[2]));
                    ht = (1.0f - z) * hg + z * h[idx];
                }
            }
            h[idx] = ht;  // only this thread reads h[j][k] in the gate phase; the next GEMV starts after the barrier
            y[(int64_t)(m.x + t) * H + k] = ht;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < ns * H; idx += kRnnThreads) {
        const int j = idx / H, k = idx - j * H, seg = groups[j].z;
        if (seg < 0) continue;
        hout[(int64_t)seg * H + k] = h[idx];
        if (MODE == 0) cout[(int64_t)seg * H + k] = c[idx];
    }
}

// groups of ns members, longest segment first (stable), empty segments included (their state is stored); the last group is padded
struct GroupArg {
    const int64_t* off;
    int64_t count;
    int ns;
};
void build_groups(const void* arg, std::vector<char>& blob) {
    const GroupArg& a = *(const GroupArg*)arg;
    std::vector<int> order((size_t)a.count);
    for (int64_t i = 0; i < a.count; ++i) order[(size_t)i] = (int)i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int p, int q) { return a.off[p + 1] - a.off[p] > a.off[q + 1] - a.off[q]; });
    const int64_t ngroups = (a.count + a.ns - 1) / a.ns;
    std::vector<int> t((size_t)(ngroups * a.ns) * 4);
    for (int64_t i = 0; i < ngroups * a.ns; ++i) {
        int* e = &t[(size_t)i * 4];
        if (i < a.count) {
            const int sg = order[(size_t)i];
            e[0] = (int)a.off[sg], e[1] = (int)(a.off[sg + 1] - a.off[sg]), e[2] = sg, e[3] = 0;
        } else {
            e[0] = 0, e[1] = 0, e[2] = -1, e[3] = 0;
        }
    }
    blob.resize(t.size() * 4);
    if (!t.empty()) memcpy(blob.data(), t.data(), blob.size());
}

template <int MODE, int NS, int KS>
int launch_rnn_seg(LeleCtx* ctx, unsigned ngroups, size_t lds_bytes, const float* wx, const float* rw, const float* bias,
                   const float* h0, const float* c0, float* y, float* hn, float* cn, const int4* groups, int ns, int H, int S) {
    LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(&rnn_seg_kernel<MODE, NS, KS>), 160 * 1024));
    hipLaunchKernelGGL((rnn_seg_kernel<MODE, NS, KS>), dim3(ngroups), dim3(kRnnThreads), lds_bytes, ctx->stream, wx, rw, bias, h0, c0, y,
                       hn, cn, groups, ns, H, S);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int MODE>
int run_rnn_segments(LeleCtx* ctx, const char* name, const LeleTensor* x, const int64_t* off, int64_t count, const LeleTensor* w,
                     const LeleTensor* r, const LeleTensor* bias, const LeleTensor* h0, const LeleTensor* c0, LeleBuf* y, LeleBuf* hn,
                     LeleBuf* cn, int64_t* y_shape, int32_t* y_rank, int32_t* info) {
    constexpr int NG = MODE == 0 ? 4 : 3;
    LELE_REQUIRE(ctx && x && w && r && y && hn && (MODE == 1 || cn), "%s: NULL argument", name);
    int64_t R = 0, I = 0, tmax = 0;
    LELE_TRY(seg_offsets(x, off, count, &R, &I, &tmax, name));
    LELE_REQUIRE(w->rank == 3 && r->rank == 3, "%s: expected W [1,%dH,I], R [1,%dH,H]", name, NG, NG);
    LELE_REQUIRE(w->dtype == LELE_F32 && r->dtype == LELE_F32, "%s: f32 tensors required", name);
    LELE_REQUIRE(w->shape[0] == 1, "%s: Only num_directions=1 supported", name);  // rnn.rs:86, 266
    int64_t H = 0, G = 0;
    int S = 0;
    size_t seg_bytes = 0;
    LELE_TRY(check_rnn_weights<MODE>(name, w, r, bias, h0, c0, I, count, &H, &G, &S, &seg_bytes));
    LELE_REQUIRE(R <= (int64_t)65535 * 64 && count < (int64_t(1) << 31) / 8 && I < (int64_t(1) << 31), "%s: tensor too large", name);
    // the form and the group width follow from the shapes alone (never from the data, the lengths or the position of a segment)
    int ks = (H % S == 0 && (int64_t)S * G <= kRnnThreads) ? (int)(H / S) : 0;
    // S = min(H, max(1, 1024 / G)) leaves four register-stationary shapes: LSTM H = 64 (KS = 16) and 128 (KS = 64), GRU H = 96 (KS = 32)
    // and 128 (KS = 64); no H gives the LSTM slices of 32 or the GRU slices of 16 (tests/test_rnn_routes.py enumerates H)
    if (ks != (MODE == 0 ? 16 : 32) && ks != 64) ks = 0;
    if (const char* f = lab_env("LELE_HIP_RNN_SEG_FORM"))  // A/B timing (tools/rnn_segments_bench.py): 2 = streamed for every shape
        if (atoi(f) == 2) ks = 0;
    int ns = 1;
    if (count > ctx->num_cus) {
        ns = (int)std::min<int64_t>(8, (count + ctx->num_cus - 1) / ctx->num_cus);
        ns = (int)std::min<int64_t>(ns, (int64_t)(160 * 1024 / seg_bytes));
    }
    if (h0 && h0->mem == LELE_MEM_DEVICE && h0->data == hn->data)
        LELE_REQUIRE(hn->cap >= (size_t)(count * H) * 4, "%s: the in-place state buffer is smaller than count * H values", name);
    if (MODE == 0 && c0 && c0->mem == LELE_MEM_DEVICE && c0->data == cn->data)
        LELE_REQUIRE(cn->cap >= (size_t)(count * H) * 4, "%s: the in-place state buffer is smaller than count * H values", name);
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* groups = nullptr;
    if (R > 0) {
        const GroupArg arg{off, count, ns};
        LELE_TRY(layout_table(ctx, "rnns", ns, 0, off, count, build_groups, &arg, &groups));
    }
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dw = nullptr, *dr = nullptr, *db = nullptr, *dh0 = nullptr, *dc0 = nullptr;
    if (R > 0) {
        LELE_TRY(ctx->dev_ptr(x, &dx));
        LELE_TRY(ctx->dev_ptr(w, &dw));
        LELE_TRY(ctx->dev_ptr(r, &dr));
        if (bias) LELE_TRY(ctx->dev_ptr(bias, &db));
    }
    if (h0 && count > 0) LELE_TRY(ctx->dev_ptr(h0, &dh0));
    if (c0 && count > 0) LELE_TRY(ctx->dev_ptr(c0, &dc0));
    void *wx = nullptr, *rt = nullptr;
    if (R > 0) {
        LELE_TRY(ctx->arena_alloc((size_t)(R * G) * 4, &wx));
        if (ks == 0) LELE_TRY(rnn_rt(ctx, r, dr, G, H, &rt));  // the streamed form reads R transposed
    }
    const size_t state_bytes = (size_t)(count * H) * 4;
    LELE_TRY(y->reserve((size_t)(R * H) * 4));
    LELE_TRY(hn->reserve(state_bytes));
    if (MODE == 0) LELE_TRY(cn->reserve(state_bytes));
    if (info) {
        info[0] = R == 0 ? 0 : ks ? 1 : 2;
        info[1] = ns;
    }
    ctx->set_route(nullptr);
    if (R == 0) {  // every segment is empty: the final state is the initial state (no kernel)
        LeleBuf* outs[2] = {hn, MODE == 0 ? cn : nullptr};
        const void* init[2] = {dh0, dc0};
        for (int i = 0; i < 2; ++i) {
            if (!outs[i] || state_bytes == 0) continue;
            if (!init[i]) LELE_HIP_CHECK(hipMemsetAsync(outs[i]->data, 0, state_bytes, ctx->stream));
            else if (init[i] != outs[i]->data)
                LELE_HIP_CHECK(hipMemcpyAsync(outs[i]->data, init[i], state_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        return set_shape(y_shape, y_rank, {R, H});
    }
    // W x of all R rows: ONE tile form whatever R is -- gemm::launch would move between its thin, small and tiled kernels (each with its
    // own summation order) as the batch grows, and a segment's bits would depend on its neighbours
    gemm::LoadRowK al{(const float*)dx, 0, I, (int)R, (int)I, (int)((((uintptr_t)dx & 15) == 0) && I % 4 == 0)};
    gemm::LoadRowK bl{(const float*)dw, 0, I, (int)G, (int)I, (int)((((uintptr_t)dw & 15) == 0) && I % 4 == 0)};
    gemm::EpiAffine epi{(float*)wx, 0, (int)R, (int)G, 1.0f, 0.0f, nullptr, gemm::C_NONE, 1};
    if (I > 0) {
        gemm::launch_tile<64, 64, 2, 2, 16>(ctx->stream, al, bl, epi, (int)R, (int)G, (int)I, 1);
    } else {
        const unsigned blocks = (unsigned)std::min<int64_t>((R * G + 255) / 256, 1024);
        hipLaunchKernelGGL((gemm::gemm_f32_epilogue_kernel<gemm::EpiAffine>), dim3(blocks, 1), dim3(256), 0, ctx->stream, epi, (int)R, (int)G);
    }
    const unsigned ngroups = (unsigned)((count + ns - 1) / ns);
    const size_t lds_bytes = seg_bytes * ns;
    const float* rw = ks ? (const float*)dr : (const float*)rt;
    float* cnd = MODE == 0 ? (float*)cn->data : nullptr;
#define LELE_RNN_SEG(NSV, KSV)                                                                                                     \
    LELE_TRY((launch_rnn_seg<MODE, NSV, KSV>(ctx, ngroups, lds_bytes, (const float*)wx, rw, (const float*)db, (const float*)dh0,  \
                                             (const float*)dc0, (float*)y->data, (float*)hn->data, cnd, (const int4*)groups, ns, (int)H, S)))
    constexpr int KS_SMALL = MODE == 0 ? 16 : 32;
    const char* form = nullptr;  // lele_hip_last_route: rnns.lstm / rnns.gru, then the kernel form
    if (ks == 64) {  // the register-stationary form walks its members two at a time, whatever ns is
        LELE_RNN_SEG(2, 64);
        form = "rnns.reg64";
    } else if (ks == KS_SMALL) {
        LELE_RNN_SEG(2, KS_SMALL);
        form = MODE == 0 ? "rnns.reg16" : "rnns.reg32";
    } else if (ns == 1) {  // the streamed form: the members' chains share every load of R^T
        LELE_RNN_SEG(1, 0);
        form = "rnns.stream1";
    } else if (ns == 2) {
        LELE_RNN_SEG(2, 0);
        form = "rnns.stream2";
    } else if (ns <= 4) {
        LELE_RNN_SEG(4, 0);
        form = "rnns.stream4";
    } else {
        LELE_RNN_SEG(8, 0);
        form = "rnns.stream8";
    }
#undef LELE_RNN_SEG
    ctx->set_route(MODE == 0 ? "rnns.lstm" : "rnns.gru", form);
    return set_shape(y_shape, y_rank, {R, H});
}

}  // namespace

extern "C" {

int lele_hip_lstm_segments(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* w,
                           const LeleTensor* r, const LeleTensor* bias, const LeleTensor* initial_h, const LeleTensor* initial_c,
                           LeleBuf* out_y, LeleBuf* out_h, LeleBuf* out_c, int64_t* y_shape, int32_t* y_rank, int32_t* info) {
    return run_rnn_segments<0>(ctx, "lstm_segments", x, row_offsets, count, w, r, bias, initial_h, initial_c, out_y, out_h, out_c,
                               y_shape, y_rank, info);
}

int lele_hip_gru_segments(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* w,
                          const LeleTensor* r, const LeleTensor* bias, const LeleTensor* initial_h, int linear_before_reset,
                          LeleBuf* out_y, LeleBuf* out_h, int64_t* y_shape, int32_t* y_rank, int32_t* info) {
    (void)linear_before_reset;  // as lele_hip_gru: the =1 form for either value (rnn.rs:366)
    return run_rnn_segments<1>(ctx, "gru_segments", x, row_offsets, count, w, r, bias, initial_h, nullptr, out_y, out_h, nullptr,
                               y_shape, y_rank, info);
}

int lele_hip_lstm(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* r, const LeleTensor* bias,
                  const LeleTensor* sequence_lens, const LeleTensor* initial_h, const LeleTensor* initial_c, LeleBuf* out_y,
                  LeleBuf* out_h, LeleBuf* out_c, int64_t* y_shape, int32_t* y_rank) {
    (void)sequence_lens;  // ignored by the reference as well (rnn.rs:72)
    return run_rnn<0>(ctx, "LSTM", x, w, r, bias, initial_h, initial_c, out_y, out_h, out_c, y_shape, y_rank);
}

int lele_hip_gru(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* r, const LeleTensor* bias,
                 const LeleTensor* initial_h, int linear_before_reset, LeleBuf* out_y, LeleBuf* out_h, int64_t* y_shape,
                 int32_t* y_rank) {
    (void)linear_before_reset;  // the x86 gate fusion evaluates the =1 form for either value (rnn.rs:366)
    return run_rnn<1>(ctx, "GRU", x, w, r, bias, initial_h, nullptr, out_y, out_h, nullptr, y_shape, y_rank);
}

}  // extern "C"
