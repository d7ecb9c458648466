// gemm.hip -- lele::kernels::{matmul, matmul_fused_add, gemm} on the f32 MFMA core (gemm_core.h).
//
//   lele_hip_matmul            <- /root/reference/src/kernels/gemm.rs:112-222
//   lele_hip_matmul_fused_add  <- /root/reference/src/kernels/gemm.rs:223-432
//   lele_hip_gemm              <- /root/reference/src/kernels/gemm.rs:433-535
// Shapes, batching/broadcast rules, bias and beta*C broadcast cases and the panics (-> error codes) follow the
// reference; the inner product is the exact-f32 MFMA chain (faer's own summation order is not pinned).
#include "common.h"
#include "gemm_core.h"
#include "gemm_small.h"

using namespace lele;

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct MmShape {
    int64_t batch_a, batch_b, fb, m, k, n;
    std::vector<int64_t> out_shape;
};

int mm_shape(const LeleTensor* a, const LeleTensor* b, MmShape* s, const char* who) {
    LELE_REQUIRE(a->rank >= 2 && b->rank >= 2, "%s: operands must have rank >= 2", who);  // gemm.rs:122-123
    LELE_REQUIRE(a->dtype == LELE_F32 && b->dtype == LELE_F32, "%s: operands must be f32", who);
    s->m = a->shape[a->rank - 2];
    s->k = a->shape[a->rank - 1];
    const int64_t kb = b->shape[b->rank - 2];
    s->n = b->shape[b->rank - 1];
    LELE_REQUIRE(s->k == kb, "MatMul K dim mismatch: %lld vs %lld", (long long)s->k, (long long)kb);  // gemm.rs:129
    s->batch_a = 1;
    for (int i = 0; i + 2 < a->rank; ++i) s->batch_a *= a->shape[i];
    s->batch_b = 1;
    for (int i = 0; i + 2 < b->rank; ++i) s->batch_b *= b->shape[i];
    s->fb = std::max(s->batch_a, s->batch_b);
    s->out_shape.clear();
    if (s->batch_a >= s->batch_b)
        s->out_shape.assign(a->shape, a->shape + a->rank - 2);
    else
        s->out_shape.assign(b->shape, b->shape + b->rank - 2);
    s->out_shape.push_back(s->m);
    s->out_shape.push_back(s->n);
    return 0;
}

// the small-problem kernel publishes one {min, max} pair per workgroup next to the result (LeleBuf::rowstat, kind 1)
float* stat_target(LeleCtx* ctx, LeleBuf* out, int64_t m, int64_t n, int64_t k, int64_t batch, int64_t* count) {
    *count = gemm::small_kernel_blocks((int)m, (int)n, (int)k, (int)batch, ctx->num_cus);
    if (*count <= 0 || *count > 4096 || lab_env("LELE_HIP_GEMM_FORCE")) return nullptr;
    if (m <= 4 || n <= 4) return nullptr;  // matrix-vector shapes go to gemm_f32_thin_kernel, which publishes nothing
    if (out->reserve_rowstat(*count) != 0 || (size_t)*count > out->rowstat_cap) return nullptr;
    return out->rowstat;
}
void stat_publish(LeleBuf* out, float* target, int64_t count, int64_t elements) {
    if (!target) return;
    out->rowstat_rows = count;
    out->rowstat_len = elements;
    out->rowstat_kind = 1;
    out->rowstat_valid = true;
}

int run_matmul(LeleCtx* ctx, const float* da, const float* db, const MmShape& s, float* out, float alpha, float beta,
               const float* c, int cmode, int64_t clen) {
    gemm::LoadRowK al{da, s.batch_a == 1 ? 0 : s.m * s.k, s.k, (int)s.m, (int)s.k,
                      (int)(aligned16(da) && s.k % 4 == 0)};
    gemm::LoadKRow bl{db, s.batch_b == 1 ? 0 : s.k * s.n, s.n, (int)s.n, (int)s.k};
    gemm::EpiAffine epi{out, s.m * s.n, (int)s.m, (int)s.n, alpha, beta, c, cmode, clen};
    ctx->set_route(nullptr, gemm::launch(ctx->stream, al, bl, epi, (int)s.m, (int)s.n, (int)s.k, (int)s.fb, ctx->num_cus));
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

// every name lele_hip_last_route can report (one level of a route each; a route joins its levels with '/')
const char* const kRouteNames[] = {
    "gemm.thin_n", "gemm.thin_m", "gemm.small", "gemm.tile256x128", "gemm.tile128x128", "gemm.tile64x256", "gemm.tile64x64",
    "gemm.tile32x128", "gemm.k0",
    "conv.dw_lds_k3", "conv.dw_lds_k5", "conv.dw_lds_k7", "conv.dw_lds_k11",
    "conv.dw_lds_k3_direct", "conv.dw_lds_k5_direct", "conv.dw_lds_k7_direct", "conv.dw_lds_k11_direct",
    "conv.dw_row4_k3", "conv.dw_row4_k5", "conv.dw_row4_k7", "conv.dw_row4_k11", "conv.dw_generic",
    "conv.win3_oct32", "conv.win3_oct64", "conv.win3_oct32_osplit", "conv.win3_oct64_osplit",
    "conv.win1_oct32", "conv.win1_oct64", "conv.win1_oct128", "conv.win1_oct32_osplit", "conv.win1_oct64_osplit", "conv.win1_oct128_osplit",
    "conv.win3s2_oct32", "conv.win3s2_oct64", "conv.win3s2_oct32_osplit", "conv.win3s2_oct64_osplit",
    "conv.direct_ocb8_s1", "conv.direct_ocb16_s1", "conv.direct_ocb8_s2", "conv.direct_ocb16_s2",
    "conv.direct_ocb8_s1_passes", "conv.direct_ocb16_s1_passes", "conv.direct_ocb8_s2_passes", "conv.direct_ocb16_s2_passes",
    "conv.gemm_pw", "conv.gemm_tap", "conv.gemm_generic",
    "convt.ks", "convt.phase", "convt.phase_fill",
    "ci.f32",
    // the i8 matrix-core ConvInteger: how the image was packed (u8 codes as given / the from_f32 forms' dynamic quantisation), then the
    // instantiation of ci8_conv_kernel<NJ, KSPLIT>; fused_scale_bias(_silu) has one kernel
    "ci8.codes", "ci8.quant", "ci8.nj4", "ci8.nj2", "ci8.nj1", "ci8.nj2_ksplit", "ci8.nj1_ksplit", "fsb.w1",
    // lele_hip_attention_view: the kernel, then its key-tile class (softmax registers per lane = tpad / 32); the one-pass kernel has
    // no classes.  lele_hip_attention_segments: one name for the launches of a layout
    "attn.flash", "attn.rows16", "attn.rows32", "attn.rows64", "attn.rows16_exact", "attn.rows32_exact", "attn.rows64_exact",
    "attn.nt2", "attn.nt4", "attn.nt6", "attn.nt8", "attn.nt10", "attn.nt12", "attn.nt14", "attn.nt16",
    "attn.seg", "attn.seg_exact",
    // manip.hip: the strided copy engine (copy.i64: a second level, 64-bit indexing), resize, max-pool (pool.pb1 / pool.pbn: one or
    // several planes per workgroup of the LDS kernels), top-k, the pitched copy; one fixed name for every entry that has no choice
    "copy.w4", "copy.w8", "copy.vec16", "copy.tile_w4", "copy.tile_w8", "copy.i64",
    "resize.up2", "resize.up4", "resize.up8", "resize.generic",
    "pool.lds", "pool.lds_sep", "pool.direct", "pool.direct_i64", "pool.pb1", "pool.pbn",
    "topk.rank", "topk.select_lds", "topk.select_l2",
    "cpitch.w16", "cpitch.w4", "cpitch.w1",
    "pad.index", "gather.rows", "gather.elements", "apool.window", "tcp.tile32", "range.f32", "range.i64", "fill.words", "cast.convert",
    // eltwise.hip: the kernel, and for the register-resident norm kernels a second level for the rows a block holds (rows.rpb2 / 4 / 8)
    "unary.vec4", "unary.w1", "bin.fast", "bin.flat_f32", "bin.index_f32", "bin.flat_i64", "bin.index_i64", "binp.vec4", "binp.w1",
    "where.index", "clip.w1", "reduce.seq", "reduce.rows16", "reduce.parts",
    "ln.reg8", "ln.reg16", "ln.reg32", "ln.stream", "softmax.reg8", "softmax.reg16", "softmax.reg32", "softmax.stream",
    "rows.rpb2", "rows.rpb4", "rows.rpb8",
    "rms.stream", "bn.w1", "add3.vec4", "add3.w1", "hpas.w1",
    // rnn.hip: the single calls name the GEMM kernel of W x as their second level (none for T == 0); the packed calls name the form of
    // rnn_seg_kernel: recurrent weights in registers in slices of 16 / 32 / 64, or streamed with 1 / 2 / 4 / 8 members a register tile
    "rnn.lstm", "rnn.gru", "rnns.lstm", "rnns.gru",
    "rnns.reg16", "rnns.reg32", "rnns.reg64", "rnns.stream1", "rnns.stream2", "rnns.stream4", "rnns.stream8",
    // frontend.hip: the kernel (main / seg: the 400 / 160 / 512 framing, with the unrolled 80-mel bank or the table-driven mel loop;
    // generic: every other framing, one fused kernel or the four-kernel form), then for the fast kernels how the PCM tile was staged
    // (direct-to-LDS, through registers, or -- a segment launch -- both); fe.two_kernel: the lab form with the separate frame-sum kernel
    "fe.main_std", "fe.main_table", "fe.seg_std", "fe.seg_table", "fe.generic_fused", "fe.generic_four",
    "fe.tile_dma", "fe.tile_regs", "fe.tile_mixed", "fe.two_kernel",
    // resample.hip: the kernel of resample / resample_segments / a stream's step
    "resample.copy", "resample.linear", "resample.fir1", "resample.fir",
    // quant.hip.  The dense linear: the member of QRoute (q.tiled / q.tiled_stream: by which row quantiser ran, prefetching or streaming),
    // the packed linear (q.seg*), the feed-forward block (EM 3 in one launch, EM 1 then EM 2, the tiled form), mat_mul_integer and
    // dynamic_quantize_linear; then what launch_igemm / launch_igemm_head / launch_as launched, or the feed-forward block's second product
    // (rs.ask: the lab build only).  The register-stationary single linear has no second level.  "q.calls" stands in front where an entry
    // point issued the calls it stands for instead of a fused form; the rest is then the (last) quantised linear's route
    "q.rs_fq", "q.rs_frag", "q.as", "q.as_ln", "q.as_ln_fsmn", "q.tiled", "q.tiled_stream", "q.head", "q.seg", "q.seg_stream", "q.seg_head",
    "qffn.rs_one", "qffn.rs_two", "qffn.tiled", "qffn.tiled_stream", "mmi.rows", "dql.w1",
    "igemm.big", "igemm.small_k4", "igemm.small_k16", "igemm.t128x128", "igemm.t32x128", "igemm.t128x64",
    "igemm.head_ids", "igemm.head_scored", "igemm.head_topk", "igemm.head_at",
    "as.two", "as.tpw8", "as.tpw4", "rs.ks4", "rs.ask_ln", "rs.ask",
    "q.calls",
};

}  // namespace

extern "C" {

int lele_hip_matmul(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, LeleBuf* out, int64_t* out_shape,
                    int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && b && out, "matmul: NULL argument");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    MmShape s;
    LELE_TRY(mm_shape(a, b, &s, "matmul"));
    LELE_REQUIRE(s.batch_b == 1 || s.batch_b == s.batch_a, "MatMul broadcast not fully supported yet");  // gemm.rs:134
    LELE_TRY(ctx->arena_reset());
    const void *da = nullptr, *db = nullptr;
    LELE_TRY(ctx->dev_ptr(a, &da));
    LELE_TRY(ctx->dev_ptr(b, &db));
    LELE_TRY(out->reserve((size_t)s.fb * s.m * s.n * 4));
    LELE_TRY(run_matmul(ctx, (const float*)da, (const float*)db, s, (float*)out->data, 1.0f, 0.0f, nullptr,
                        gemm::C_NONE, 0));
    return set_shape_v(out_shape, out_rank, s.out_shape);
}

int lele_hip_matmul_fused_add(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, const LeleTensor* bias,
                              LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && b && bias && out, "matmul_fused_add: NULL argument");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    MmShape s;
    LELE_TRY(mm_shape(a, b, &s, "matmul_fused_add"));
    LELE_REQUIRE(s.batch_b == 1 || s.batch_b == s.batch_a || s.batch_a == 1,
                 "matmul_fused_add: batch dims %lld vs %lld cannot be broadcast", (long long)s.batch_a,
                 (long long)s.batch_b);
    const int64_t blen = numel(bias);
    LELE_REQUIRE(blen > 0 && bias->dtype == LELE_F32, "matmul_fused_add: bias must be a non-empty f32 tensor");
    LELE_TRY(ctx->arena_reset());
    const void *da = nullptr, *db = nullptr, *dc = nullptr;
    LELE_TRY(ctx->dev_ptr(a, &da));
    LELE_TRY(ctx->dev_ptr(b, &db));
    LELE_TRY(ctx->dev_ptr(bias, &dc));
    LELE_TRY(out->reserve((size_t)s.fb * s.m * s.n * 4));
    // bias.len() == n: rows prefilled with the bias (gemm.rs:251-316); otherwise out[i] += bias[i % len] over the
    // flattened result (gemm.rs:354-415)
    const int cmode = (blen == s.n) ? gemm::C_ROWVEC : gemm::C_MODULO;
    LELE_TRY(run_matmul(ctx, (const float*)da, (const float*)db, s, (float*)out->data, 1.0f, 1.0f, (const float*)dc,
                        cmode, blen));
    return set_shape_v(out_shape, out_rank, s.out_shape);
}

int lele_hip_gemm(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, const LeleTensor* c, float alpha, float beta,
                  int trans_a, int trans_b, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && b && out, "gemm: NULL argument");
    LELE_REQUIRE(a->rank >= 2 && b->rank >= 2, "gemm: operands must have rank >= 2");
    LELE_REQUIRE(a->dtype == LELE_F32 && b->dtype == LELE_F32, "gemm: operands must be f32");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t m = trans_a ? a->shape[a->rank - 1] : a->shape[a->rank - 2];  // gemm.rs:446-465
    const int64_t k = trans_a ? a->shape[a->rank - 2] : a->shape[a->rank - 1];
    const int64_t n = trans_b ? b->shape[b->rank - 2] : b->shape[b->rank - 1];
    const int64_t k2 = trans_b ? b->shape[b->rank - 1] : b->shape[b->rank - 2];
    LELE_REQUIRE(k == k2, "Gemm K dim mismatch");  // gemm.rs:466
    LELE_TRY(ctx->arena_reset());
    const void *da = nullptr, *db = nullptr, *dc = nullptr;
    LELE_TRY(ctx->dev_ptr(a, &da));
    LELE_TRY(ctx->dev_ptr(b, &db));
    int cmode = gemm::C_NONE;
    int64_t clen = 0;
    if (c && beta != 0.0f) {  // gemm.rs:484-515
        clen = numel(c);
        LELE_REQUIRE(clen > 0, "gemm: empty C");
        LELE_TRY(ctx->dev_ptr(c, &dc));
        if (clen == m * n)
            cmode = gemm::C_FULL;
        else if (clen == n)
            cmode = gemm::C_ROWVEC;
        else if (clen == m)
            cmode = gemm::C_COLVEC;
        else if (clen == 1)
            cmode = gemm::C_SCALAR;
        else
            cmode = gemm::C_MODULO;
    }
    LELE_TRY(out->reserve((size_t)m * n * 4));
    const float* fa = (const float*)da;
    const float* fb = (const float*)db;
    gemm::EpiAffine epi{(float*)out->data, m * n, (int)m, (int)n, alpha, beta, (const float*)dc, cmode, clen};
    // transposes are strides (gemm.rs:517-520): A(m,k) = a[m*rsa + k*csa], B(k,n) = b[k*rsb + n*csb]
    gemm::LoadRowK a_mk{fa, 0, k, (int)m, (int)k, (int)(aligned16(fa) && k % 4 == 0)};
    gemm::LoadKRow a_km{fa, 0, m, (int)m, (int)k};
    gemm::LoadKRow b_kn{fb, 0, n, (int)n, (int)k};
    gemm::LoadRowK b_nk{fb, 0, k, (int)n, (int)k, (int)(aligned16(fb) && k % 4 == 0)};
    const char* r;
    if (!trans_a && !trans_b)
        r = gemm::launch(ctx->stream, a_mk, b_kn, epi, (int)m, (int)n, (int)k, 1, ctx->num_cus);
    else if (!trans_a && trans_b)
        r = gemm::launch(ctx->stream, a_mk, b_nk, epi, (int)m, (int)n, (int)k, 1, ctx->num_cus);
    else if (trans_a && !trans_b)
        r = gemm::launch(ctx->stream, a_km, b_kn, epi, (int)m, (int)n, (int)k, 1, ctx->num_cus);
    else
        r = gemm::launch(ctx->stream, a_km, b_nk, epi, (int)m, (int)n, (int)k, 1, ctx->num_cus);
    ctx->set_route(nullptr, r);
    LELE_HIP_CHECK(hipGetLastError());
    return set_shape(out_shape, out_rank, {m, n});
}

int lele_hip_matmul_view(LeleCtx* ctx, const LeleTensor* a, const LeleMatView* av, const LeleTensor* b, const LeleMatView* bv,
                         int64_t batch_outer, int64_t batch_inner, int64_t m, int64_t k, int64_t n, const LeleMatView* ov,
                         const int64_t* out_dims, int32_t out_dims_rank, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && a && av && b && bv && ov && out && out_dims, "matmul_view: NULL argument");
    LELE_REQUIRE(a->dtype == LELE_F32 && b->dtype == LELE_F32, "matmul_view: operands must be f32");
    LELE_REQUIRE(batch_outer >= 1 && batch_inner >= 1 && m >= 0 && n >= 0 && k >= 0, "matmul_view: bad dimensions");
    LELE_REQUIRE(av->stride_col == 1 || av->stride_row == 1, "matmul_view: A must be contiguous along k or along its rows");
    LELE_REQUIRE(bv->stride_col == 1 || bv->stride_row == 1, "matmul_view: B must be contiguous along n or along k");
    LELE_REQUIRE(ov->stride_col == 1, "matmul_view: the output must be contiguous along n");
    const int64_t fb = batch_outer * batch_inner, na = numel(a), nb = numel(b);
    int64_t total = 1;
    for (int i = 0; i < out_dims_rank; ++i) total *= out_dims[i];
    LELE_REQUIRE(total == fb * m * n, "matmul_view: output shape holds %lld elements, the product has %lld", (long long)total,
                 (long long)(fb * m * n));
    LELE_REQUIRE(fb < (int64_t(1) << 31) && m < (int64_t(1) << 31) && n < (int64_t(1) << 31) && k < (int64_t(1) << 31), "matmul_view: dimension too large");
    // the last element each view can touch must lie inside its tensor
    auto last = [&](const LeleMatView* v, int64_t r, int64_t c) {
        return v->offset + (batch_outer - 1) * v->stride_outer + (batch_inner - 1) * v->stride_inner + (r - 1) * v->stride_row + (c - 1) * v->stride_col;
    };
    if (fb * m * k) LELE_REQUIRE(av->offset >= 0 && last(av, m, k) < na, "matmul_view: the A view leaves its tensor");
    if (fb * k * n) LELE_REQUIRE(bv->offset >= 0 && last(bv, k, n) < nb, "matmul_view: the B view leaves its tensor");
    if (total) LELE_REQUIRE(ov->offset >= 0 && last(ov, m, n) < total, "matmul_view: the output view leaves its buffer");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void *da = nullptr, *db = nullptr;
    LELE_TRY(ctx->dev_ptr(a, &da));
    LELE_TRY(ctx->dev_ptr(b, &db));
    LELE_TRY(out->reserve((size_t)total * 4));
    ctx->set_route(nullptr);
    if (total) {
        const float* pa = (const float*)da + av->offset;
        const float* pb = (const float*)db + bv->offset;
        const int bi = (int)batch_inner;
        gemm::EpiAffine epi{(float*)out->data + ov->offset, ov->stride_outer, (int)m, (int)n, 1.0f, 0.0f, nullptr, gemm::C_NONE, 0,
                            ov->stride_row, bi, ov->stride_inner};
        int64_t nstat = 0;
        epi.blockstat = stat_target(ctx, out, m, n, k, fb, &nstat);
        // A(row, k): k-contiguous -> LoadRowK(ld = row stride); row-contiguous -> LoadKRow(ld = k stride).  B likewise on (n, k).
        gemm::LoadRowK a_rk{pa, av->stride_outer, av->stride_row, (int)m, (int)k,
                            (int)(aligned16(pa) && av->stride_row % 4 == 0 && av->stride_outer % 4 == 0 && av->stride_inner % 4 == 0), bi, av->stride_inner};
        gemm::LoadKRow a_kr{pa, av->stride_outer, av->stride_col, (int)m, (int)k, bi, av->stride_inner};
        gemm::LoadKRow b_kn{pb, bv->stride_outer, bv->stride_row, (int)n, (int)k, bi, bv->stride_inner};
        gemm::LoadRowK b_nk{pb, bv->stride_outer, bv->stride_col, (int)n, (int)k,
                            (int)(aligned16(pb) && bv->stride_col % 4 == 0 && bv->stride_outer % 4 == 0 && bv->stride_inner % 4 == 0), bi, bv->stride_inner};
        const bool a_k = av->stride_col == 1, b_n = bv->stride_col == 1;
        const char* r;
        if (a_k && b_n) r = gemm::launch(ctx->stream, a_rk, b_kn, epi, (int)m, (int)n, (int)k, (int)fb, ctx->num_cus);
        else if (a_k && !b_n) r = gemm::launch(ctx->stream, a_rk, b_nk, epi, (int)m, (int)n, (int)k, (int)fb, ctx->num_cus);
        else if (!a_k && b_n) r = gemm::launch(ctx->stream, a_kr, b_kn, epi, (int)m, (int)n, (int)k, (int)fb, ctx->num_cus);
        else r = gemm::launch(ctx->stream, a_kr, b_nk, epi, (int)m, (int)n, (int)k, (int)fb, ctx->num_cus);
        ctx->set_route(nullptr, r);
        LELE_HIP_CHECK(hipGetLastError());
        stat_publish(out, epi.blockstat, nstat, total);
    }
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(out_dims, out_dims + out_dims_rank));
}

int lele_hip_last_route(LeleCtx* ctx, char* buf, size_t cap) {
    LELE_REQUIRE(ctx && (buf || cap == 0), "last_route: NULL argument");
    std::string r;
    for (const char* level : ctx->route)
        if (level) r += (r.empty() ? "" : "/") + std::string(level);
    LELE_REQUIRE(r.size() < cap, "last_route: %zu bytes do not hold the %zu-character name", cap, r.size());
    memcpy(buf, r.c_str(), r.size() + 1);
    return 0;
}

int lele_hip_route_names(char* buf, size_t cap) {
    LELE_REQUIRE(buf || cap == 0, "route_names: NULL buffer");
    std::string all;
    for (const char* n : kRouteNames) all += (all.empty() ? "" : "\n") + std::string(n);
    LELE_REQUIRE(all.size() < cap, "route_names: %zu bytes do not hold the %zu-character list", cap, all.size());
    memcpy(buf, all.c_str(), all.size() + 1);
    return 0;
}

}  // extern "C"