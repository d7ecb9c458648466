// segments.hip -- operators of the packed batch (x [R, D] + row_offsets [count + 1], the layout lele_hip_frontend_compute_segments and
// lele_hip_cmvn_segments hand on) that are neither a GEMM nor the attention:
//
//   lele_hip_depthwise_conv1d_tlc_segments  <- lele_hip_depthwise_conv1d_tlc (conv.hip; conv1d.rs:837 between two transposes) on every
//                                              segment alone as [1, len, P]: the FSMN memory block of a SAN-M layer
//   lele_hip_segments_prepend               <- manipulation.rs:108-207 (concat along time) per segment: the prompt rows of a
//                                              SenseVoice-shaped encoder in front of every utterance
//
// Every utterance is computed exactly as if it ran alone; the reference is batch 1 throughout (examples/sensevoice/src/main.rs).
#include "common.h"
#include "tlc_core.h"

#include <algorithm>

using namespace lele;

namespace {

// dwconv1d_tlc_kernel's tile routine (tlc_core.h) on the rows of ONE segment: a lane owns a channel and TT consecutive time steps of a
// tile it finds in the layout's tile list {segment's first row, its rows, first time step of the tile}; taps outside the SEGMENT are
// skipped.  Tiles are listed segment by segment in time order, and the dense kernel's XCD relabelling keeps neighbours on one L2.
template <int KW, int TT>
__global__ __launch_bounds__(256) void dwconv1d_tlc_seg_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               const int4* __restrict__ tiles, int c, int pitch, int pl, int relu,
                                                               int add_input, unsigned total) {
    const unsigned i = tlc_xcd_index(total);
    if (i >= total) return;
    const unsigned ch = i % (unsigned)c;
    const int4 tl = tiles[i / (unsigned)c];
    tlc_tile<KW, TT>(x + (size_t)tl.x * pitch + ch, w, bias, out + (size_t)tl.x * c + ch, ch, tl.z, tl.y, tl.y, c, pitch, pl, relu, add_input);
}

constexpr int kSegTT = 8;  // time steps per thread (a batch of utterances: the dense entry point's choice for full grids)

struct OffArg {
    const int64_t* off;
    int64_t count;
};
void build_tiles(const void* arg, std::vector<char>& blob) {
    const OffArg& a = *(const OffArg*)arg;
    std::vector<int> t;
    for (int64_t i = 0; i < a.count; ++i) {
        const int64_t len = a.off[i + 1] - a.off[i];
        for (int64_t t0 = 0; t0 < len; t0 += kSegTT) {
            const int e[4] = {(int)a.off[i], (int)len, (int)t0, (int)i};
            t.insert(t.end(), e, e + 4);
        }
    }
    blob.resize(t.size() * 4);
    if (!t.empty()) memcpy(blob.data(), t.data(), blob.size());
}

// out rows: for every segment `p` prefix rows, then its rows.  grid.y = segment, a pure copy.
__global__ void seg_prepend_kernel(const float* __restrict__ x, const int64_t* __restrict__ off, int64_t p, int64_t d,
                                   const float* __restrict__ prefix, float* __restrict__ out) {
    const int64_t b = blockIdx.y, r0 = off[b], npre = p * d, total = (off[b + 1] - r0 + p) * d;
    x += r0 * d;
    out += (r0 + p * b) * d;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x)
        out[idx] = idx < npre ? prefix[idx] : x[idx - npre];
}

}  // namespace

extern "C" {

int lele_hip_depthwise_conv1d_tlc_segments(LeleCtx* ctx, const LeleTensor* x, int64_t x_offset, const int64_t* row_offsets, int64_t count,
                                           const LeleTensor* w, const LeleTensor* bias, int64_t pad_left, int64_t pad_right, int relu,
                                           int add_input, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && x && w && out, "depthwise_conv1d_tlc_segments: NULL argument");
    int64_t rows = 0, pitch = 0, tmax = 0;
    LELE_TRY(seg_offsets(x, row_offsets, count, &rows, &pitch, &tmax, "depthwise_conv1d_tlc_segments"));
    LELE_REQUIRE(w->rank == 3 && w->dtype == LELE_F32, "depthwise_conv1d_tlc_segments: w [C,1,K] f32 required");
    const int64_t c = w->shape[0], k = w->shape[2];
    LELE_REQUIRE(w->shape[1] == 1, "depthwise_conv1d_tlc: weight must be [C, 1, K] (group = C)");
    LELE_REQUIRE(x_offset >= 0 && x_offset + c <= pitch, "depthwise_conv1d_tlc: channels [%lld, %lld) outside the last dimension (%lld)",
                 (long long)x_offset, (long long)(x_offset + c), (long long)pitch);
    LELE_REQUIRE(k == 3 || k == 5 || k == 7 || k == 11, "depthwise_conv1d_tlc: kernel sizes 3, 5, 7, 11 (use transpose + conv1d otherwise)");
    LELE_REQUIRE(pad_left >= 0 && pad_right >= 0, "depthwise_conv1d_tlc: negative padding");
    LELE_REQUIRE(pad_left + pad_right == k - 1, "depthwise_conv1d_tlc_segments: pad_left + pad_right must be K - 1 = %lld (every segment keeps its rows), got %lld",
                 (long long)(k - 1), (long long)(pad_left + pad_right));
    if (bias) LELE_REQUIRE(numel(bias) >= c, "conv1d: bias shorter than C_out");
    const int64_t ntiles = [&] {
        int64_t n = 0;
        for (int64_t i = 0; i < count; ++i) n += (row_offsets[i + 1] - row_offsets[i] + kSegTT - 1) / kSegTT;
        return n;
    }();
    const int64_t total = ntiles * c;
    LELE_REQUIRE(total < (int64_t(1) << 31) && rows < (int64_t(1) << 31) && pitch < (int64_t(1) << 31), "depthwise_conv1d_tlc_segments: tensor too large");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* tiles = nullptr;
    if (total > 0) {
        const OffArg arg{row_offsets, count};
        LELE_TRY(layout_table(ctx, "tlc8", 0, 0, row_offsets, count, build_tiles, &arg, &tiles));
    }
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dwp = nullptr, *db = nullptr;
    if (total > 0) {
        LELE_TRY(ctx->dev_ptr(x, &dx));
        LELE_TRY(ctx->dev_ptr(w, &dwp));
        if (bias) LELE_TRY(ctx->dev_ptr(bias, &db));
    }
    LELE_TRY(out->reserve((size_t)(rows * c) * 4));
    if (total > 0) {
        const dim3 grid((unsigned)((total + 255) / 256));
#define LELE_TLC_SEG(KW)                                                                                                              \
    hipLaunchKernelGGL((dwconv1d_tlc_seg_kernel<KW, kSegTT>), grid, dim3(256), 0, ctx->stream, (const float*)dx + x_offset, (const float*)dwp, \
                       (const float*)db, (float*)out->data, (const int4*)tiles, (int)c, (int)pitch, (int)pad_left, relu, add_input,     \
                       (unsigned)total)
        if (k == 3) LELE_TLC_SEG(3);
        else if (k == 5) LELE_TLC_SEG(5);
        else if (k == 7) LELE_TLC_SEG(7);
        else LELE_TLC_SEG(11);
#undef LELE_TLC_SEG
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {rows, c});
}

int lele_hip_segments_prepend(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* prefix,
                              LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && x && prefix && out && out_offsets, "segments_prepend: NULL argument");
    int64_t rows = 0, d = 0, tmax = 0;
    LELE_TRY(seg_offsets(x, row_offsets, count, &rows, &d, &tmax, "segments_prepend"));
    LELE_REQUIRE(prefix->dtype == LELE_F32 && prefix->rank >= 1 && prefix->shape[prefix->rank - 1] == d && d > 0,
                 "segments_prepend: prefix must be f32 [p, D] with D = %lld", (long long)d);
    const int64_t p = numel(prefix) / d;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* doff = nullptr;
    if (count > 0) LELE_TRY(offsets_table(ctx, row_offsets, count, &doff));
    LELE_TRY(ctx->arena_reset());
    const void *dx = nullptr, *dp = nullptr;
    if (rows > 0) LELE_TRY(ctx->dev_ptr(x, &dx));
    if (p > 0) LELE_TRY(ctx->dev_ptr(prefix, &dp));
    const int64_t orows = rows + p * count;
    LELE_TRY(out->reserve((size_t)(orows * d) * 4));
    if (orows > 0) {
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((tmax + p) * d + 255) / 256, 1024));
        for (int64_t c0 = 0; c0 < count; c0 += 65535) {  // grid.y limit
            const int64_t nc = std::min<int64_t>(65535, count - c0);
            hipLaunchKernelGGL(seg_prepend_kernel, dim3(blocks, (unsigned)nc), dim3(256), 0, ctx->stream, (const float*)dx,
                               (const int64_t*)doff + c0, p, d, (const float*)dp, (float*)out->data + c0 * p * d);
        }
        LELE_HIP_CHECK(hipGetLastError());
    }
    for (int64_t i = 0; i <= count; ++i) out_offsets[i] = row_offsets[i] + p * i;
    return set_shape(out_shape, out_rank, {orows, d});
}

}  // extern "C"
