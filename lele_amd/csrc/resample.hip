// resample.hip -- sample-rate conversion in front of the audio front-end (see lele_hip.h, "audio resampling"): the reference's linear
// `resample` (examples/web-demo/src/audio.rs:114-138) bit for bit, and a Kaiser-windowed polyphase FIR, each as a packed batch of
// segments of one buffer (one launch) and as N live streams pushed a chunk a tick (one launch a push).
//
// One kernel body serves both forms.  A record (RsRec) names, per segment or stream, a REGION of input samples -- `carry` samples kept
// from earlier pushes, then the new ones in pcm -- and where that region sits on the utterance's own time axis (in0).  Every output is
// computed from its ABSOLUTE index i and absolute input positions, so its value depends on the utterance alone and not on where the
// region starts, how the audio was cut or how many streams there are: that is what makes live and batch equal bit for bit.
//
//   linear  src_pos = (double)i * ratio; idx = floor; frac = src_pos - idx; (float)(s[idx]*(1-frac) + s[idx+1]*frac) in f64 with
//           round-to-nearest multiplies and add, never contracted; the last sample as it is where idx + 1 == len (the tail rule).
//           A thread owns four consecutive outputs, aligned to 16 bytes of `out`: one 16-byte store where all four are the segment's.
//   fir     base = (i*M) div L, phase = (i*M) mod L in 64-bit integers; out = sum over t = 0 .. T-1, IN THIS ORDER, of
//           acc = fmaf(h[phase][t], x[base - T/2 + 1 + t], acc) from acc = +0 in f32, x = 0 outside [0, len) (a select, not a product:
//           a NaN next to a segment cannot leak).  The order depends on nothing but T.  A block of 256 threads stages the input span of
//           1024 consecutive outputs in LDS; thread k computes outputs k, k + 256, k + 512, k + 768 of the block (four independent
//           chains; neighbouring lanes read neighbouring LDS words and store neighbouring floats).
//   fir1    L == 1: every output has phase 0, the T coefficients are read at wave-uniform addresses (scalar loads), no table in LDS.
//   fir     L > 1: the whole table, rows pitched T + 1 floats (odd: the lanes' phases differ), is copied to LDS by every block.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <numeric>

using namespace lele;

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsBlockOut = 1024;  // outputs a block: four a thread
constexpr size_t kRsMaxLds = 160 * 1024;

struct RsRec {
    int64_t src;    // pcm index of the first NEW sample (packed form: the segment's start)
    int64_t state;  // stream form: float index of the stream's carried samples in the state array
    int64_t in0;    // absolute input index of the region's first sample
    int64_t total;  // input samples that exist so far: in0 + carry + new
    int64_t i0;     // absolute index of the first output this call writes
    int64_t out0;   // its place in `out`
    int64_t n_out;
    int32_t carry;  // carried samples in front of the new ones
    int32_t block0;  // first block of this record
    int32_t keep_from, keep;  // stream form: region[keep_from, keep_from + keep) is carried into the next push
};

// sample n of the utterance (absolute); 0 outside [0, total).  Inside, 0 <= n - in0 < carry + new: the host keeps every sample an
// output that is still to come reads (rs_next_needed).
__device__ __forceinline__ float rs_fetch(const float* pcm, const float* state, const RsRec& r, int64_t n) {
    if (n < 0 || n >= r.total) return 0.f;
    const int64_t j = n - r.in0;
    if (j < 0) return 0.f;
    return j < r.carry ? state[r.state + j] : pcm[r.src + (j - r.carry)];
}

// stream form, the blocks behind the compute blocks: one a stream, copies what the next push still needs into the OTHER half of the
// state (read side and write side never overlap, so no ordering against the compute blocks is needed)
__device__ __forceinline__ void rs_carry(const float* pcm, const float* state, const RsRec& r, float* next) {
    for (int j = threadIdx.x; j < r.keep; j += kRsThreads) {
        const int q = r.keep_from + j;
        next[j] = q < r.carry ? state[r.state + q] : pcm[r.src + (q - r.carry)];
    }
}

template <bool COPY>
__global__ __launch_bounds__(kRsThreads) void rs_linear_kernel(const float* pcm, const float* state, const RsRec* recs, const int* blk, int nblk,
                                                               double ratio, float* out, float* state_next, int64_t pitch) {
    if ((int)blockIdx.x >= nblk) {
        const int s = (int)blockIdx.x - nblk;
        rs_carry(pcm, state, recs[s], state_next + (int64_t)s * pitch);
        return;
    }
    const RsRec r = recs[blk[blockIdx.x]];
    const int64_t g4 = (r.out0 & ~int64_t(3)) + (int64_t)((int)blockIdx.x - r.block0) * kRsBlockOut + (int64_t)threadIdx.x * 4;
    float v[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t k = g4 + j - r.out0;
        ok[j] = k >= 0 && k < r.n_out;
        v[j] = 0.f;
        if (!ok[j]) continue;
        const int64_t i = r.i0 + k;
        if (COPY) {
            v[j] = rs_fetch(pcm, state, r, i);
        } else {
            const double src_pos = __dmul_rn((double)i, ratio);
            const int64_t idx = (int64_t)src_pos;
            const double frac = __dsub_rn(src_pos, (double)idx);
            const float a = rs_fetch(pcm, state, r, idx);
            if (idx + 1 < r.total) {
                const float b = rs_fetch(pcm, state, r, idx + 1);
                v[j] = (float)__dadd_rn(__dmul_rn((double)a, __dsub_rn(1.0, frac)), __dmul_rn((double)b, frac));
            } else {
                v[j] = a;  // audio.rs:132-133: the last sample, whatever frac is
            }
        }
    }
    if (ok[0] && ok[1] && ok[2] && ok[3]) {
        *reinterpret_cast<float4*>(out + g4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) out[g4 + j] = v[j];
    }
}

template <bool ONE_PHASE>
__global__ __launch_bounds__(kRsThreads) void rs_fir_kernel(const float* pcm, const float* state, const RsRec* recs, const int* blk, int nblk,
                                                            const float* __restrict__ taps, int L, int M, int T, int tile_cap, float* out,
                                                            float* state_next, int64_t pitch) {
    extern __shared__ float rs_lds[];
    if ((int)blockIdx.x >= nblk) {
        const int s = (int)blockIdx.x - nblk;
        rs_carry(pcm, state, recs[s], state_next + (int64_t)s * pitch);
        return;
    }
    const RsRec r = recs[blk[blockIdx.x]];
    const int64_t k0 = (int64_t)((int)blockIdx.x - r.block0) * kRsBlockOut;  // this block's first output within the call
    const int nb = (int)(r.n_out - k0 < kRsBlockOut ? r.n_out - k0 : kRsBlockOut);
    const int64_t ia = r.i0 + k0;
    const int64_t base_a = (ia * M) / L;
    const int64_t base_z = ((ia + nb - 1) * M) / L;
    const int64_t lo = base_a - T / 2 + 1;
    const int ntile = (int)(base_z - base_a) + T;  // <= (1023 * M) / L + 1 + T < tile_cap
    LELE_DEV_ASSERT(ntile <= tile_cap);
    float* xs = rs_lds;
    for (int q = threadIdx.x; q < ntile; q += kRsThreads) xs[q] = rs_fetch(pcm, state, r, lo + q);
    const int tp = ONE_PHASE ? T : T + 1;
    const float* hs = rs_lds + tile_cap;
    if (!ONE_PHASE) {
        float* hw = rs_lds + tile_cap;
        for (int q = threadIdx.x; q < L * tp; q += kRsThreads) hw[q] = taps[q];
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int xo[4], ho[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = (int)threadIdx.x + kRsThreads * j;
        const int64_t im = (ia + (k < nb ? k : 0)) * M;
        const int64_t base = im / L;
        xo[j] = (int)(base - base_a);
        ho[j] = (int)(im - base * L) * tp;
        LELE_DEV_ASSERT(xo[j] >= 0 && xo[j] + T <= ntile);
    }
    if (ONE_PHASE) {
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
            const float h = taps[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(h, xs[xo[j] + t], acc[j]);
        }
    } else {
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(hs[ho[j] + t], xs[xo[j] + t], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = (int)threadIdx.x + kRsThreads * j;
        if (k < nb) out[r.out0 + k0 + k] = acc[j];
    }
}

double bessel_i0(double x) {  // power series: every term positive, converges for any x
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

}  // namespace

struct LeleResampler {
    LeleCtx* ctx = nullptr;  // NULL: host only (lengths and the table; nothing can be launched)
    int64_t from = 0, to = 0;
    int32_t mode = 0;
    double ratio = 1.0;  // linear: from as f64 / to as f64
    int64_t L = 1, M = 1, T = 0;
    int32_t z = 0;
    double beta = 0, rolloff = 0;
    std::vector<float> table;  // sinc: [L][T], every phase normalised in f64 and rounded
    float* dtable = nullptr;   // rows pitched T + 1 where L > 1
    int64_t tile_cap = 0;
    size_t lds = 0;
    DevTables seg_tables;  // the packed layouts' records and block locators

    bool copy() const { return from == to; }
    // linear: number of i >= 0 with fl(i * ratio) < x, in the kernel's own f64 product
    int64_t below(int64_t x) const {
        if (x <= 0) return 0;
        int64_t i = (int64_t)((double)x / ratio);
        while (i > 0 && !((double)(i - 1) * ratio < (double)x)) --i;
        while ((double)i * ratio < (double)x) ++i;
        return i;
    }
    int64_t linear_len(int64_t len) const { return (int64_t)((double)len / ratio); }  // audio.rs:121
    // outputs that are final once r samples have arrived (fin: and nothing more follows)
    int64_t emitted(int64_t r, bool fin) const {
        if (copy()) return r;
        if (mode == LELE_RESAMPLE_LINEAR) return std::min(linear_len(r), fin ? below(r) : below(r - 1));
        if (fin) return (r * L + M - 1) / M;
        const int64_t q = r - T / 2;  // base_i + T/2 <= r - 1  <=>  i*M < q*L
        return q <= 0 ? 0 : (q * L + M - 1) / M;
    }
    // the first input sample output e reads, within [0, r]
    int64_t next_needed(int64_t e, int64_t r) const {
        int64_t n;
        if (copy()) n = e;
        else if (mode == LELE_RESAMPLE_LINEAR) n = (int64_t)((double)e * ratio);
        else n = (e * M) / L - T / 2 + 1;
        return std::min(std::max<int64_t>(n, 0), r);
    }
    int64_t carry_bound() const {  // the most samples a stream carries between pushes
        if (copy()) return 0;
        if (mode == LELE_RESAMPLE_LINEAR) return (int64_t)std::ceil(ratio) + 2;
        return T;
    }
};

struct LeleResamplerStream {
    LeleResampler* rs = nullptr;
    hipStream_t stream = nullptr;
    int64_t streams = 0, max_chunk = 0, pitch = 0;
    float* state = nullptr;  // [2][streams][pitch]: a push reads half `half` and writes the other
    int half = 0;
    std::vector<int64_t> received, outputs, carry;  // per stream; functions of the chunk lengths alone
};

namespace {

struct RsLayout {
    const LeleResampler* rs;
    const int64_t *starts, *lengths, *offsets;
    int64_t count;
};

int64_t rs_blocks(const LeleResampler* rs, int64_t out0, int64_t n_out) {
    if (n_out == 0) return 0;
    if (rs->copy() || rs->mode == LELE_RESAMPLE_LINEAR) return (out0 + n_out - (out0 & ~int64_t(3)) + kRsBlockOut - 1) / kRsBlockOut;
    return (n_out + kRsBlockOut - 1) / kRsBlockOut;
}

void rs_build_table(const void* arg, std::vector<char>& blob) {
    const RsLayout& l = *(const RsLayout*)arg;
    std::vector<RsRec> recs((size_t)l.count);
    std::vector<int> blk;
    for (int64_t i = 0; i < l.count; ++i) {
        RsRec& r = recs[(size_t)i];
        r = RsRec{};
        r.src = l.starts[i];
        r.total = l.lengths[i];
        r.out0 = l.offsets[i];
        r.n_out = l.offsets[i + 1] - l.offsets[i];
        r.block0 = (int32_t)blk.size();
        blk.insert(blk.end(), (size_t)rs_blocks(l.rs, r.out0, r.n_out), (int)i);
    }
    blob.resize(recs.size() * sizeof(RsRec) + blk.size() * sizeof(int));
    if (!recs.empty()) memcpy(blob.data(), recs.data(), recs.size() * sizeof(RsRec));
    if (!blk.empty()) memcpy(blob.data() + recs.size() * sizeof(RsRec), blk.data(), blk.size() * sizeof(int));
}

// one launch: nblk compute blocks, then `tail` carry blocks (stream form)
int rs_launch(LeleResampler* rs, const float* pcm, const float* state, const RsRec* recs, const int* blk, int64_t nblk, int64_t tail, float* out,
              float* state_next, int64_t pitch) {
    LeleCtx* ctx = rs->ctx;
    const dim3 grid((unsigned)(nblk + tail)), block(kRsThreads);
    if (rs->copy()) {
        ctx->set_route("resample.copy");
        hipLaunchKernelGGL(rs_linear_kernel<true>, grid, block, 0, ctx->stream, pcm, state, recs, blk, (int)nblk, 1.0, out, state_next, pitch);
    } else if (rs->mode == LELE_RESAMPLE_LINEAR) {
        ctx->set_route("resample.linear");
        hipLaunchKernelGGL(rs_linear_kernel<false>, grid, block, 0, ctx->stream, pcm, state, recs, blk, (int)nblk, rs->ratio, out, state_next, pitch);
    } else if (rs->L == 1) {
        if (rs->lds > 60 * 1024) LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(rs_fir_kernel<true>), (int)rs->lds));
        ctx->set_route("resample.fir1");
        hipLaunchKernelGGL(rs_fir_kernel<true>, grid, block, rs->lds, ctx->stream, pcm, state, recs, blk, (int)nblk, (const float*)rs->dtable, (int)rs->L,
                           (int)rs->M, (int)rs->T, (int)rs->tile_cap, out, state_next, pitch);
    } else {
        if (rs->lds > 60 * 1024) LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(rs_fir_kernel<false>), (int)rs->lds));
        ctx->set_route("resample.fir");
        hipLaunchKernelGGL(rs_fir_kernel<false>, grid, block, rs->lds, ctx->stream, pcm, state, recs, blk, (int)nblk, (const float*)rs->dtable, (int)rs->L,
                           (int)rs->M, (int)rs->T, (int)rs->tile_cap, out, state_next, pitch);
    }
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int lele_hip_resampler_create(LeleCtx* ctx, int64_t from_rate, int64_t to_rate, int32_t mode, int32_t z, double beta, double rolloff,
                              LeleResampler** out) {
    LELE_REQUIRE(out, "resampler_create: out is NULL");
    LELE_REQUIRE(from_rate > 0 && from_rate < (int64_t(1) << 20), "resampler_create: from_rate %lld is not a sample rate (1 .. 2^20 - 1)",
                 (long long)from_rate);
    LELE_REQUIRE(to_rate > 0 && to_rate < (int64_t(1) << 20), "resampler_create: to_rate %lld is not a sample rate (1 .. 2^20 - 1)",
                 (long long)to_rate);
    LELE_REQUIRE(mode == LELE_RESAMPLE_LINEAR || mode == LELE_RESAMPLE_SINC, "resampler_create: mode %d is neither LELE_RESAMPLE_LINEAR nor _SINC",
                 (int)mode);
    LELE_REQUIRE(!ctx || !ctx->capturing, "graph capture: resampler_create allocates; create the resampler before capturing");
    LeleResampler rs;
    rs.ctx = ctx;
    rs.from = from_rate;
    rs.to = to_rate;
    rs.mode = mode;
    rs.ratio = (double)from_rate / (double)to_rate;  // audio.rs:120
    if (mode == LELE_RESAMPLE_SINC && from_rate != to_rate) {
        LELE_REQUIRE(z >= 1 && z <= 256, "resampler_create: z %d (zero crossings a side) must be 1 .. 256", (int)z);
        LELE_REQUIRE(beta >= 0.0 && beta <= 40.0, "resampler_create: beta %g must be 0 .. 40", beta);
        LELE_REQUIRE(rolloff > 0.0 && rolloff <= 1.0, "resampler_create: rolloff %g must be in (0, 1]", rolloff);
        const int64_t g = std::gcd(from_rate, to_rate);
        rs.L = to_rate / g;
        rs.M = from_rate / g;
        rs.z = z;
        rs.beta = beta;
        rs.rolloff = rolloff;
        const double cut = std::min(1.0, (double)rs.L / (double)rs.M);
        rs.T = 2 * (int64_t)std::ceil((double)z / cut);
        const int64_t tp = rs.L == 1 ? rs.T : rs.T + 1;
        rs.tile_cap = ((kRsBlockOut - 1) * rs.M) / rs.L + rs.T + 2;
        rs.lds = (size_t)(rs.tile_cap + (rs.L == 1 ? 0 : rs.L * tp)) * sizeof(float);
        LELE_REQUIRE(rs.lds <= kRsMaxLds,
                     "resampler_create: %lld -> %lld Hz needs %lld phases of %lld taps and a %lld-sample tile, %zu bytes of LDS (the limit is %zu)",
                     (long long)from_rate, (long long)to_rate, (long long)rs.L, (long long)rs.T, (long long)rs.tile_cap, rs.lds, kRsMaxLds);
        // w(t) = s sinc(s t) kaiser_beta(t / W), s = rolloff * min(1, L/M), W = T/2; tap t of phase p sits at distance
        // (t - (T/2 - 1)) - p/L from the output's instant
        const double s = rolloff * cut, W = (double)rs.T / 2.0, i0b = bessel_i0(beta), pi = 3.14159265358979323846;
        rs.table.assign((size_t)(rs.L * rs.T), 0.f);
        std::vector<double> row((size_t)rs.T);
        for (int64_t p = 0; p < rs.L; ++p) {
            double sum = 0.0;
            for (int64_t t = 0; t < rs.T; ++t) {
                const double d = (double)(t - (rs.T / 2 - 1)) - (double)p / (double)rs.L;
                const double a = pi * s * d, u = d / W;
                const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
                const double win = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
                row[(size_t)t] = s * sinc * win;
                sum += row[(size_t)t];
            }
            for (int64_t t = 0; t < rs.T; ++t) rs.table[(size_t)(p * rs.T + t)] = (float)(row[(size_t)t] / sum);
        }
        if (ctx) {
            LELE_HIP_CHECK(hipSetDevice(ctx->device));
            std::vector<float> padded((size_t)(rs.L * tp), 0.f);
            for (int64_t p = 0; p < rs.L; ++p) memcpy(&padded[(size_t)(p * tp)], &rs.table[(size_t)(p * rs.T)], (size_t)rs.T * sizeof(float));
            LELE_HIP_CHECK(hipMalloc((void**)&rs.dtable, padded.size() * sizeof(float)));
            hipError_t e = hipMemcpy(rs.dtable, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(rs.dtable);
                LELE_HIP_CHECK(e);
            }
        }
    }
    *out = new LeleResampler(std::move(rs));
    return 0;
}

int lele_hip_resampler_destroy(LeleResampler* rs) {
    if (!rs) return 0;
    if (rs->ctx) {
        (void)hipStreamSynchronize(rs->ctx->stream);
        rs->seg_tables.release();
        if (rs->dtable) (void)hipFree(rs->dtable);
    }
    delete rs;
    return 0;
}

int lele_hip_resampler_table(const LeleResampler* rs, float* table, int64_t capacity, int64_t* l, int64_t* m, int64_t* taps) {
    LELE_REQUIRE(rs, "resampler_table: rs is NULL");
    if (l) *l = rs->L;
    if (m) *m = rs->M;
    if (taps) *taps = rs->T;
    if (table) {
        LELE_REQUIRE(capacity >= (int64_t)rs->table.size(), "resampler_table: room for %lld floats, the table has %lld", (long long)capacity,
                     (long long)rs->table.size());
        if (!rs->table.empty()) memcpy(table, rs->table.data(), rs->table.size() * sizeof(float));
    }
    return 0;
}

int lele_hip_resampler_out_len(const LeleResampler* rs, int64_t samples_before, int64_t chunk_len, int32_t final, int64_t* out_len,
                               int64_t* carry) {
    LELE_REQUIRE(rs, "resampler_out_len: rs is NULL");
    LELE_REQUIRE(samples_before >= 0 && chunk_len >= 0 && samples_before <= (int64_t(1) << 40) && chunk_len <= (int64_t(1) << 40),
                 "resampler_out_len: %lld samples before and a chunk of %lld are not sample counts (0 .. 2^40)", (long long)samples_before,
                 (long long)chunk_len);
    const int64_t r = samples_before + chunk_len;
    const int64_t e0 = rs->emitted(samples_before, false), e1 = rs->emitted(r, final != 0);
    if (out_len) *out_len = e1 - e0;
    if (carry) *carry = final ? 0 : r - rs->next_needed(e1, r);
    return 0;
}

int lele_hip_resample_segments(LeleResampler* rs, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths, int64_t count,
                               LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(rs && pcm && out && out_offsets, "resample_segments: NULL argument");
    LELE_REQUIRE(rs->ctx, "resample_segments: the resampler was created without a context (host arithmetic only)");
    LELE_REQUIRE(count >= 0 && (count == 0 || (starts && lengths)), "resample_segments: bad segment arrays (count %lld)", (long long)count);
    LELE_REQUIRE(pcm->dtype == LELE_F32 && pcm->rank == 1, "resample_segments: pcm must be f32 [N]");
    const int64_t n = pcm->shape[0];
    for (int64_t i = 0; i < count; ++i)
        LELE_REQUIRE(starts[i] >= 0 && lengths[i] >= 0 && starts[i] <= n - lengths[i],
                     "resample_segments: segment %lld (start %lld, length %lld) lies outside the %lld samples of pcm", (long long)i,
                     (long long)starts[i], (long long)lengths[i], (long long)n);
    LELE_REQUIRE(n <= (int64_t(1) << 40), "resample_segments: %lld samples are beyond the kernels' index arithmetic", (long long)n);
    std::vector<int64_t> off((size_t)count + 1, 0);
    int64_t blocks = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t len = rs->emitted(lengths[i], true);
        off[(size_t)i + 1] = off[(size_t)i] + len;
        blocks += rs_blocks(rs, off[(size_t)i], len);
    }
    const int64_t total = off[(size_t)count];
    LELE_REQUIRE(blocks < (int64_t(1) << 31), "resample_segments: %lld blocks exceed the grid", (long long)blocks);
    LeleCtx* ctx = rs->ctx;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    if (total == 0) {  // nothing to write: rank 0, as the front-end's packed calls answer
        ctx->set_route(nullptr);
        memcpy(out_offsets, off.data(), off.size() * sizeof(int64_t));
        out->bytes = 0;
        if (out_rank) *out_rank = 0;
        return 0;
    }
    LELE_TRY(ctx->arena_reset());
    const void* dpcm = nullptr;
    LELE_TRY(ctx->dev_ptr(pcm, &dpcm));
    // the layout's records and block locator: shape metadata, uploaded once per distinct layout and never rewritten
    std::string key((size_t)count * 16, '\0');
    memcpy(&key[0], starts, (size_t)count * 8);
    memcpy(&key[(size_t)count * 8], lengths, (size_t)count * 8);
    const RsLayout lay{rs, starts, lengths, off.data(), count};
    const void* table = nullptr;
    LELE_TRY(rs->seg_tables.get(ctx, std::move(key), rs_build_table, &lay, &table));
    LELE_TRY(out->reserve((size_t)total * sizeof(float)));
    const RsRec* drecs = (const RsRec*)table;
    LELE_TRY(rs_launch(rs, (const float*)dpcm, nullptr, drecs, (const int*)(drecs + count), blocks, 0, (float*)out->data, nullptr, 0));
    memcpy(out_offsets, off.data(), off.size() * sizeof(int64_t));
    return set_shape(out_shape, out_rank, {total});
}

int lele_hip_resampler_stream_create(LeleResampler* rs, int64_t streams, int64_t max_chunk, LeleResamplerStream** out) {
    LELE_REQUIRE(rs && out, "resampler_stream_create: NULL argument");
    LELE_REQUIRE(rs->ctx, "resampler_stream_create: the resampler was created without a context (host arithmetic only)");
    LELE_REQUIRE(streams >= 1 && max_chunk >= 1, "resampler_stream_create: streams %lld and max_chunk %lld must be at least 1", (long long)streams,
                 (long long)max_chunk);
    LELE_REQUIRE(streams < (int64_t(1) << 24) && max_chunk < (int64_t(1) << 30),
                 "resampler_stream_create: %lld streams of %lld samples a push are beyond the kernels' 32-bit offsets", (long long)streams,
                 (long long)max_chunk);
    LeleCtx* ctx = rs->ctx;
    LELE_REQUIRE(!ctx->capturing, "graph capture: resampler_stream_create allocates; create the stream before capturing");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LeleResamplerStream* st = new LeleResamplerStream();
    st->rs = rs;
    st->stream = ctx->stream;
    st->streams = streams;
    st->max_chunk = max_chunk;
    st->pitch = (rs->carry_bound() + 4) & ~int64_t(3);
    st->received.assign((size_t)streams, 0);
    st->outputs.assign((size_t)streams, 0);
    st->carry.assign((size_t)streams, 0);
    hipError_t e = hipMalloc((void**)&st->state, (size_t)(2 * streams * st->pitch) * sizeof(float));
    if (e != hipSuccess) {
        delete st;
        LELE_HIP_CHECK(e);
    }
    *out = st;
    return 0;
}

int lele_hip_resampler_stream_destroy(LeleResamplerStream* st) {
    if (!st) return 0;
    (void)hipStreamSynchronize(st->stream);
    (void)hipFree(st->state);
    delete st;
    return 0;
}

int lele_hip_resampler_stream_reset(LeleResamplerStream* st, const int64_t* ids, int64_t count) {
    LELE_REQUIRE(st, "resampler_stream_reset: st is NULL");
    if (!ids) {
        std::fill(st->received.begin(), st->received.end(), 0);
        std::fill(st->outputs.begin(), st->outputs.end(), 0);
        std::fill(st->carry.begin(), st->carry.end(), 0);
        return 0;
    }
    for (int64_t i = 0; i < count; ++i)
        LELE_REQUIRE(ids[i] >= 0 && ids[i] < st->streams, "resampler_stream_reset: id %lld is not one of the %lld streams", (long long)ids[i],
                     (long long)st->streams);
    for (int64_t i = 0; i < count; ++i) st->received[ids[i]] = st->outputs[ids[i]] = st->carry[ids[i]] = 0;
    return 0;
}

int lele_hip_resampler_stream_counters(const LeleResamplerStream* st, int64_t id, int64_t* samples, int64_t* outputs, int64_t* carry) {
    LELE_REQUIRE(st, "resampler_stream_counters: st is NULL");
    LELE_REQUIRE(id >= 0 && id < st->streams, "resampler_stream_counters: id %lld is not one of the %lld streams", (long long)id,
                 (long long)st->streams);
    if (samples) *samples = st->received[id];
    if (outputs) *outputs = st->outputs[id];
    if (carry) *carry = st->carry[id];
    return 0;
}

int lele_hip_resampler_stream_push(LeleResamplerStream* st, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths,
                                   const uint8_t* final_or_null, LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(st && pcm && starts && lengths && out && out_offsets, "resampler_stream_push: NULL argument");
    LeleResampler* rs = st->rs;
    LeleCtx* ctx = rs->ctx;
    LELE_REQUIRE(!ctx->capturing, "resampler_stream_push: a push cannot be recorded into a graph (the stream counters advance on the host at "
                                  "every call); push eagerly and capture what consumes the samples");
    LELE_REQUIRE(pcm->dtype == LELE_F32 && pcm->rank == 1, "resampler_stream_push: pcm must be f32 [N]");
    const int64_t n = pcm->shape[0], count = st->streams;
    for (int64_t i = 0; i < count; ++i) {
        LELE_REQUIRE(starts[i] >= 0 && lengths[i] >= 0 && starts[i] <= n - lengths[i],
                     "resampler_stream_push: the chunk of stream %lld (start %lld, length %lld) lies outside the %lld samples of pcm", (long long)i,
                     (long long)starts[i], (long long)lengths[i], (long long)n);
        LELE_REQUIRE(lengths[i] <= st->max_chunk, "resampler_stream_push: the chunk of stream %lld has %lld samples, the stream was created for %lld",
                     (long long)i, (long long)lengths[i], (long long)st->max_chunk);
        LELE_REQUIRE(st->received[(size_t)i] + lengths[i] <= (int64_t(1) << 40), "resampler_stream_push: stream %lld is beyond 2^40 samples",
                     (long long)i);
    }
    // the plan of this push: one record a stream, one stream index a compute block.  Host arithmetic only; the counters are committed
    // after the launch has been issued.
    std::vector<RsRec> recs((size_t)count);
    std::vector<int> blk;
    std::vector<int64_t> off((size_t)count + 1, 0), nr((size_t)count), ne((size_t)count), nc((size_t)count);
    const int64_t half_floats = count * st->pitch;
    for (int64_t i = 0; i < count; ++i) {
        const bool fin = final_or_null && final_or_null[i];
        const int64_t r0 = st->received[(size_t)i], e0 = st->outputs[(size_t)i], c0 = st->carry[(size_t)i];
        const int64_t r1 = r0 + lengths[i], e1 = rs->emitted(r1, fin);
        RsRec& r = recs[(size_t)i];
        r = RsRec{};
        r.src = starts[i];
        r.state = (int64_t)st->half * half_floats + i * st->pitch;
        r.in0 = r0 - c0;
        r.total = r1;
        r.i0 = e0;
        r.out0 = off[(size_t)i];
        r.n_out = e1 - e0;
        r.carry = (int32_t)c0;
        r.block0 = (int32_t)blk.size();
        int64_t keep = 0;
        if (!fin) {
            const int64_t from = rs->next_needed(e1, r1);
            keep = r1 - from;
            LELE_REQUIRE(from >= r.in0 && keep <= st->pitch, "resampler_stream_push: stream %lld would carry %lld samples from %lld (internal error)",
                         (long long)i, (long long)keep, (long long)from);
            r.keep_from = (int32_t)(from - r.in0);
            r.keep = (int32_t)keep;
        }
        LELE_REQUIRE(r.n_out >= 0, "resampler_stream_push: stream %lld loses outputs (internal error)", (long long)i);
        off[(size_t)i + 1] = off[(size_t)i] + r.n_out;
        blk.insert(blk.end(), (size_t)rs_blocks(rs, r.out0, r.n_out), (int)i);
        nr[(size_t)i] = fin ? 0 : r1;  // a final push leaves the stream reset
        ne[(size_t)i] = fin ? 0 : e1;
        nc[(size_t)i] = keep;
    }
    const int64_t total = off[(size_t)count];
    LELE_REQUIRE(blk.size() + (size_t)count < (size_t(1) << 31), "resampler_stream_push: %lld streams of up to %lld samples exceed the grid",
                 (long long)count, (long long)st->max_chunk);
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void* dpcm = nullptr;
    LELE_TRY(ctx->dev_ptr(pcm, &dpcm));
    // the table changes every push: through the staging arena
    const size_t rec_bytes = recs.size() * sizeof(RsRec), blk_bytes = blk.size() * sizeof(int);
    std::vector<char> blob(rec_bytes + blk_bytes);
    memcpy(blob.data(), recs.data(), rec_bytes);
    if (blk_bytes) memcpy(blob.data() + rec_bytes, blk.data(), blk_bytes);
    void* dtab = nullptr;
    LELE_TRY(ctx->arena_alloc(blob.size(), &dtab));
    if (total) LELE_TRY(out->reserve((size_t)total * sizeof(float)));
    LELE_HIP_CHECK(hipMemcpyAsync(dtab, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));  // (pageable: staged before it returns)
    const RsRec* drecs = (const RsRec*)dtab;
    LELE_TRY(rs_launch(rs, (const float*)dpcm, st->state, drecs, (const int*)((const char*)dtab + rec_bytes), (int64_t)blk.size(), count,
                       (float*)out->data, st->state + (int64_t)(1 - st->half) * half_floats, st->pitch));
    st->half = 1 - st->half;
    st->received.swap(nr);
    st->outputs.swap(ne);
    st->carry.swap(nc);
    memcpy(out_offsets, off.data(), off.size() * sizeof(int64_t));
    if (total == 0) {  // nothing became final this tick
        out->bytes = 0;
        if (out_rank) *out_rank = 0;
        return 0;
    }
    return set_shape(out_shape, out_rank, {total});
}

}  // extern "C"
