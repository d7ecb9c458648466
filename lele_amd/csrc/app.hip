// app.hip -- the application-side pre/post-processing steps that bracket a lele model run,
// moved to the device so that (a) 16-bit PCM crosses PCIe instead of f32 and (b) only token ids leave the GPU.
//
//   lele_hip_wav_to_f32    <- /root/reference/examples/sensevoice/src/audio.rs:52-73   (s16 / u8 -> f32, stereo -> mono)
//   lele_hip_argmax_last   <- /root/reference/examples/sensevoice/src/tokenizer.rs:50-61 (per-frame arg-max of the logits;
//                             Iterator::max_by keeps the LAST of equal maxima)
//   lele_hip_token_filter  <- tokenizer.rs:63-71  (drop blank / special ids, keep frame order; no CTC collapsing upstream)
//   lele_hip_token_filter_segments <- the same per segment of a packed batch of ids -> [count, W] ids + counts
//   lele_hip_token_align_segments  <- ... and with every kept id its frame within the segment and its score
//   lele_hip_ctc_beam_search_segments <- apps.ctc_prefix_beam_search per segment of a packed batch of k-best candidates (no upstream
//                             counterpart: the reference decodes greedily); float64, one wavefront a segment
//   lele_hip_ctc_align_segments <- apps.ctc_forced_align per segment of a packed batch of listed-column log-probabilities (no upstream
//                             counterpart); Viterbi and the CTC likelihood in float64, one wavefront a segment
//   lele_hip_image_preprocess   <-/root/reference/examples/yolo26n-seg/src/image.rs:62-111 (PIL-style nearest resize to
//                             target x target, HWC u8 -> CHW f32 / 255)
//   lele_hip_yolo_seg_postprocess <- image.rs:127-265 (score / box filter in query order, box rescale, per-detection mask =
//                             sigmoid(coeffs . mask_features), nearest upscale, box crop, thresholds)
//   lele_hip_image_preprocess_batch <- image.rs:62-111 per image of a packed byte buffer of images of different sizes, one launch
//   lele_hip_yolo_seg_postprocess_sized <- image.rs:127-265 per image at a size of its own; the mask (image.rs:213-262) from bit tables
//                             of its exact predicates, each evaluated once, instead of pixel by detection
// All exact: one IEEE operation per sample / pure comparisons / the reference's operation order; the only transcendental
// (the mask sigmoid's expf, libm upstream) is evaluated in double and rounded once, i.e. correctly rounded like glibc's.
#include "common.h"

using namespace lele;

namespace {

__global__ void wav_to_f32_kernel(const uint8_t* __restrict__ bytes, int64_t frames, int bits, int channels,
                                  float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < frames; i += (int64_t)gridDim.x * blockDim.x) {
        float s[2] = {0.0f, 0.0f};
        for (int c = 0; c < channels; ++c) {
            const int64_t k = i * channels + c;
            if (bits == 16) {
                const int16_t v = (int16_t)((uint16_t)bytes[2 * k] | ((uint16_t)bytes[2 * k + 1] << 8));  // i16::from_le_bytes
                s[c] = (float)v / 32768.0f;
            } else {
                s[c] = ((float)bytes[k] - 128.0f) / 128.0f;
            }
        }
        out[i] = channels == 2 ? (s[0] + s[1]) / 2.0f : s[0];
    }
}

// one workgroup per row; (value, index) pairs reduced with "greater value wins, equal values: greater index wins".
// A NaN loses to every number (the reference panics on one, tokenizer.rs:56: partial_cmp().unwrap()): a thread never takes a NaN, so
// the pairs that reach the reduction hold numbers only, and a thread that saw nothing but NaN enters it with index -1, which loses to
// every pair.  The result is the LAST maximum among the row's non-NaN entries, V - 1 for a row without any; rows without a NaN are
// decided by exactly the comparisons they always were.
__global__ __launch_bounds__(256) void argmax_last_kernel(const float* __restrict__ x, int64_t rows, int64_t v,
                                                          int32_t* __restrict__ out) {
    const int64_t row = blockIdx.x;
    const float* p = x + row * v;
    float best = -INFINITY;
    int64_t bi = -1;
    for (int64_t j = threadIdx.x; j < v; j += 256) {
        const float val = p[j];
        if (val == val && (bi < 0 || val >= best)) {  // later index replaces an equal value; val != val: NaN, never taken
            best = val;
            bi = j;
        }
    }
    __shared__ float sv[256];
    __shared__ int64_t si[256];
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float ov = sv[threadIdx.x + off];
            const int64_t oi = si[threadIdx.x + off];
            const float mv = sv[threadIdx.x];
            const int64_t mi = si[threadIdx.x];
            if (oi >= 0 && (mi < 0 || ov > mv || (ov == mv && oi > mi))) {  // index -1 (empty or all-NaN slot) loses; no NaN in sv
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    // no number in the row: V - 1 (all NaN), or unwrap_or(0) for an empty row
    if (threadIdx.x == 0) out[row] = (int32_t)(si[0] >= 0 ? si[0] : (v > 0 ? v - 1 : 0));
}

// one workgroup per batch row: ordered compaction of the ids whose skip flag is clear (ballot prefix inside a wave,
// LDS prefix across waves, a running base across 256-frame chunks)
__global__ __launch_bounds__(256) void token_filter_kernel(const int32_t* __restrict__ ids, int64_t t, const uint8_t* __restrict__ skip,
                                                           int64_t vocab, int32_t* __restrict__ out, int32_t* __restrict__ counts) {
    const int64_t row = blockIdx.x;
    const int32_t* p = ids + row * t;
    int32_t* o = out + row * t;
    __shared__ int wave_cnt[4];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = 0; c0 < t; c0 += 256) {
        const int64_t j = c0 + threadIdx.x;
        const int32_t id = j < t ? p[j] : 0;
        // tokenizer.rs:63-69: ids beyond the vocabulary are dropped, id 0 (blank) and <|...|> specials are skipped
        const bool keep = j < t && id >= 0 && id < vocab && skip[id] == 0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_cnt[w];
        const int b0 = base;
        if (keep) o[b0 + woff + before] = id;
        __syncthreads();
        if (threadIdx.x == 0) base = b0 + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const int n = base;
    for (int64_t j = n + threadIdx.x; j < t; j += 256) o[j] = -1;
    if (threadIdx.x == 0) counts[row] = n;
}

// token_filter_kernel's rule on a packed batch: workgroup b compacts ids[off[b], off[b + 1]) into row b of out [count, w] (w >= the
// segment's rows: checked on the host), then -1 up to w
__global__ __launch_bounds__(256) void token_filter_seg_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ skip, int64_t vocab, int64_t w,
                                                               int32_t* __restrict__ out, int32_t* __restrict__ counts) {
    const int64_t row = blockIdx.x;
    const int64_t t = off[row + 1] - off[row];
    const int32_t* p = ids + off[row];
    int32_t* o = out + row * w;
    __shared__ int wave_cnt[4];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = 0; c0 < t; c0 += 256) {
        const int64_t j = c0 + threadIdx.x;
        const int32_t id = j < t ? p[j] : 0;
        const bool keep = j < t && id >= 0 && id < vocab && skip[id] == 0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int wv = 0; wv < wave; ++wv) woff += wave_cnt[wv];
        const int b0 = base;
        if (keep) o[b0 + woff + before] = id;
        __syncthreads();
        if (threadIdx.x == 0) base = b0 + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const int n = base;
    for (int64_t j = n + threadIdx.x; j < w; j += 256) o[j] = -1;
    if (threadIdx.x == 0) counts[row] = n;
}

// token_filter_seg_kernel with the two things a served transcript needs beside the id: per kept token its frame (row index within the
// segment) into frames [count, w], then -1, and, where out_lp != NULL, its score lp[off[b] + frame] into out_lp [count, w], then 0.0.
// The same ballot / LDS prefix compaction; ids and counts are token_filter_seg_kernel's.
__global__ __launch_bounds__(256) void token_align_seg_kernel(const int32_t* __restrict__ ids, const float* __restrict__ lp,
                                                              const int64_t* __restrict__ off, const uint8_t* __restrict__ skip, int64_t vocab,
                                                              int64_t w, int32_t* __restrict__ out, int32_t* __restrict__ frames,
                                                              float* __restrict__ out_lp /* NULL: no scores */, int32_t* __restrict__ counts) {
    const int64_t row = blockIdx.x;
    const int64_t t = off[row + 1] - off[row];
    const int32_t* p = ids + off[row];
    const float* q = lp + off[row];  // read only where out_lp != NULL (and the segment has rows)
    int32_t* o = out + row * w;
    int32_t* f = frames + row * w;
    float* s = out_lp ? out_lp + row * w : nullptr;
    __shared__ int wave_cnt[4];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = 0; c0 < t; c0 += 256) {
        const int64_t j = c0 + threadIdx.x;
        const int32_t id = j < t ? p[j] : 0;
        const bool keep = j < t && id >= 0 && id < vocab && skip[id] == 0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int wv = 0; wv < wave; ++wv) woff += wave_cnt[wv];
        const int b0 = base;
        if (keep) {
            const int at = b0 + woff + before;
            o[at] = id;
            f[at] = (int32_t)j;
            if (s) s[at] = q[j];
        }
        __syncthreads();
        if (threadIdx.x == 0) base = b0 + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const int n = base;
    for (int64_t j = n + threadIdx.x; j < w; j += 256) {
        o[j] = -1;
        f[j] = -1;
        if (s) s[j] = 0.0f;
    }
    if (threadIdx.x == 0) counts[row] = n;
}

// ---- CTC prefix beam search over the k best candidates of every frame (apps.ctc_prefix_beam_search on the device) ----------------
// A prefix is a node of a trie: {parent node, label}, node 0 the empty prefix.  A beam slot keeps its node, the node's parent and
// label, its depth and the two float64 scores.  Wherever two prefixes are compared they are compared BY CONTENT: equal nodes are equal
// prefixes, different nodes are walked upwards, so a prefix that left the beam and came back under a second node (its descendants
// still hanging from the first) is still recognised.

struct BeamSlots {
    double pb[8], pnb[8], tot[8];
    int node[8], parent[8], last[8], depth[8];
};

// the trie lives in LDS while a segment's nodes fit these bytes, else in the context's scratch block
constexpr int64_t kBeamLdsTrieBytes = 56 * 1024;

__device__ inline double logaddexp64(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double mx = a > b ? a : b, mn = a > b ? b : a;
    if (mx == mn) return mx + 0.693147180559945309417;  // numpy's rule for equal arguments; inf - inf is never formed
    return mx + log1p(exp(mn - mx));
}

// v of lane l, l uniform over the wave: two v_readlane_b32, no LDS round trip
__device__ inline double beam_lane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The wave's LDS writes before, its LDS reads behind.  With the trie in LDS nothing of the search passes through global memory between
// the frames, so the wait covers LDS only: a __syncthreads() would also wait for the next frame's candidates (requested early on
// purpose) and for the trie stores.  With the trie in global memory it is the full barrier.
template <bool LDS_TRIE>
__device__ inline void beam_sync() {
    if (LDS_TRIE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    } else {
        __syncthreads();
    }
}

// the prefixes of nodes a and b, both of depth d: equal?  At most d steps.
__device__ inline bool beam_same_prefix(const int2* trie, int a, int b, int d) {
    for (int i = 0; i < d && a != b; ++i) {
        const int2 x = trie[a], y = trie[b];
        if (x.y != y.y) return false;
        a = x.x;
        b = y.x;
    }
    return a == b;
}

// Python's tuple order of two prefixes, each given as (node of all but the last label, last label, length): is A before B?
// The longer is lifted to the other's length, then both climb until their nodes meet; the labels that differed nearest the root decide,
// and of a sequence and its extension the shorter is first.  At most `lim` steps in all (lim >= both lengths).  Entries of a frame
// whose ids are distinct are different prefixes; should two be EQUAL all the same (duplicate ids: the result is unspecified), the
// entry indices ia / ib decide, so that the order stays strict and total and every rank is taken exactly once.
__device__ inline bool beam_prefix_less(const int2* trie, int ra, int la, int na, int rb, int lb, int nb, int lim, int ia, int ib) {
    if (na == 0 || nb == 0) return na != nb ? na < nb : ia < ib;
    const bool a_shorter = na < nb, same_length = na == nb;
    for (int i = 0; i < lim && na > nb; ++i, --na) {
        const int2 x = trie[ra];
        ra = x.x;
        la = x.y;
    }
    for (int i = 0; i < lim && nb > na; ++i, --nb) {
        const int2 y = trie[rb];
        rb = y.x;
        lb = y.y;
    }
    int res = 0;
    for (int i = 0; i < lim; ++i) {
        if (la != lb) res = la < lb ? -1 : 1;
        if (ra == rb) break;
        const int2 x = trie[ra], y = trie[rb];
        ra = x.x;
        la = x.y;
        rb = y.x;
        lb = y.y;
    }
    return res ? res < 0 : same_length ? ia < ib : a_shorter;
}

extern __shared__ int2 beam_trie_lds[];

// One wavefront per segment.  Lane (s, j) = (lane >> 3, lane & 7) takes beam slot s and candidate j of the frame: it extends s by the
// candidate's label (a NEW entry, or a contribution to the slot that already holds that prefix) and feeds s's own repeat; lane q < 8
// then finishes the STAY entry of slot q (the slot's own prefix) in its registers.  Every entry is ranked by counting the entries that
// beat it -- greater total first, equal totals in tuple order -- and rank r < beam becomes slot r of the other slot set, so the beam is
// always sorted.  The totals are compared lane against lane (v_readlane over the ballot of live entries); only an exact tie, which is
// rare, walks the trie.  Per segment node_stride = 1 + beam * (most frames of a segment) nodes; frame t's new prefixes are nodes
// 1 + t * beam + rank.
template <bool LDS_TRIE>
__global__ __launch_bounds__(64) void ctc_beam_seg_kernel(const int32_t* __restrict__ ids, const float* __restrict__ lp,
                                                          const int64_t* __restrict__ off, int k, int64_t skip_rows, int blank, int beam,
                                                          int nbest, int64_t w, int64_t node_stride, int2* trie_all,
                                                          int32_t* __restrict__ out_tok, int32_t* __restrict__ out_len,
                                                          float* __restrict__ out_score, int32_t* __restrict__ out_cnt) {
    const int64_t seg = blockIdx.x;
    const int lane = threadIdx.x, s = lane >> 3, j = lane & 7;
    const int64_t r0 = off[seg] + skip_rows, r1 = off[seg + 1];
    const int frames = r1 > r0 ? (int)(r1 - r0) : 0;
    int2* trie = LDS_TRIE ? beam_trie_lds : trie_all + seg * node_stride;
    __shared__ BeamSlots slots[2];
    __shared__ double ext_v[8], rep_v[8];
    __shared__ int ext_has[8], rep_has[8], cand[8];
    if (lane < 16) {  // every slot of both sets starts as the empty prefix: whatever is read later is a node of this segment
        BeamSlots& b = slots[lane >> 3];
        b.pb[lane & 7] = 0.0;
        b.pnb[lane & 7] = -INFINITY;
        b.tot[lane & 7] = 0.0;
        b.node[lane & 7] = 0;
        b.parent[lane & 7] = 0;
        b.last[lane & 7] = -1;
        b.depth[lane & 7] = 0;
    }
    if (lane == 0) trie[0] = make_int2(0, -1);
    if (lane < 8) {
        ext_has[lane] = 0;
        rep_has[lane] = 0;
    }
    int cur = 0, nb = 1;
    int c_next = -1;
    float lp_next = -INFINITY;
    if (frames > 0 && j < k) {
        c_next = ids[r0 * k + j];
        lp_next = lp[r0 * k + j];
    }
    beam_sync<LDS_TRIE>();
    for (int t = 0; t < frames; ++t) {
        const int c = c_next;
        const double l = (double)lp_next;
        if (t + 1 < frames && j < k) {  // the next frame's candidates, asked for before this frame's arithmetic
            c_next = ids[(r0 + t + 1) * k + j];
            lp_next = lp[(r0 + t + 1) * k + j];
        }
        const BeamSlots& B = slots[cur];
        BeamSlots& N = slots[cur ^ 1];
        const bool cv = j < k && c >= 0;
        const unsigned long long bm = __ballot(cv && c == blank) & 0xffull;
        const bool has_blank = bm != 0;
        const double lp_blank = beam_lane_f64(l, has_blank ? __ffsll((long long)bm) - 1 : 0);
        if (lane < 8) cand[lane] = c;
        const bool live = s < nb;
        const int my_node = B.node[s], my_last = B.last[s], my_depth = B.depth[s];
        const int q_depth = B.depth[j], q_last = B.last[j], q_parent = B.parent[j];  // slot j's, for the others to read lane j
        const bool ext = live && cv && c != blank;
        const bool rep = ext && c == my_last;
        double e = (rep ? B.pb[s] : B.tot[s]) + l;  // a repeat extends only what ended in a blank
        if (e != e) e = -INFINITY;  // a NaN (a NaN or +inf score came in) would compare false with everything: ranks must stay distinct
        bool fresh = ext;
        for (int q = 0; q < nb; ++q) {
            const int qd = __builtin_amdgcn_readlane(q_depth, q), ql = __builtin_amdgcn_readlane(q_last, q),
                      qp = __builtin_amdgcn_readlane(q_parent, q);
            if (ext && qd == my_depth + 1 && ql == c && beam_same_prefix(trie, qp, my_node, my_depth)) {
                ext_v[q] = e;  // the extension IS slot q's prefix
                ext_has[q] = 1;
                fresh = false;
            }
        }
        if (rep) {
            rep_v[s] = B.pnb[s] + l;
            rep_has[s] = 1;
        }
        beam_sync<LDS_TRIE>();
        // lane q < nb: the stay entry of slot q
        bool stay = false;
        double st_pb = -INFINITY, st_pnb = -INFINITY, st_tot = -INFINITY;
        if (lane < 8) {
            const bool hr = rep_has[lane] != 0, he = ext_has[lane] != 0;
            stay = lane < nb && (has_blank || hr || he);
            st_pb = has_blank ? B.tot[lane] + lp_blank : -INFINITY;
            st_pnb = logaddexp64(hr ? rep_v[lane] : -INFINITY, he ? ext_v[lane] : -INFINITY);
            if (st_pb != st_pb) st_pb = -INFINITY;
            if (st_pnb != st_pnb) st_pnb = -INFINITY;
            st_tot = logaddexp64(st_pb, st_pnb);
            if (st_tot != st_tot) st_tot = -INFINITY;
            ext_has[lane] = 0;  // for the next frame, whose writes come behind this frame's last barrier
            rep_has[lane] = 0;
        }
        // Both of this lane's entries, the new one (e) and, in lanes 0..7, the stay one (st_tot), against every live entry
        const unsigned long long fresh_m = __ballot(fresh);
        const unsigned stay_m = (unsigned)__ballot(stay) & 0xffu;
        int rank = 0, srank = 0;
        unsigned long long tie_nn = 0, tie_sn = 0;  // new entries that tie with my new / my stay entry
        unsigned tie_ns = 0, tie_ss = 0;            // stay entries that tie with my new / my stay entry
        for (unsigned long long m = fresh_m; m; m &= m - 1) {
            const int i = __ffsll((long long)m) - 1;
            const double tm = beam_lane_f64(e, i);
            rank += tm > e;
            srank += tm > st_tot;
            if (tm == e) tie_nn |= 1ull << i;
            if (tm == st_tot) tie_sn |= 1ull << i;
        }
        for (unsigned m = stay_m; m; m &= m - 1) {
            const int q = __ffs((int)m) - 1;
            const double tq = beam_lane_f64(st_tot, q);
            rank += tq > e;
            srank += tq > st_tot;
            if (tq == e) tie_ns |= 1u << q;
            if (tq == st_tot) tie_ss |= 1u << q;
        }
        const int lim = t + 2;
        tie_nn &= ~(1ull << lane);
        if (lane < 8) tie_ss &= ~(1u << lane);
        if (fresh && (tie_nn | tie_ns)) {  // exact ties: the tuple order decides
            for (unsigned long long m = tie_nn; m; m &= m - 1) {
                const int i = __ffsll((long long)m) - 1;
                rank += beam_prefix_less(trie, B.node[i >> 3], cand[i & 7], B.depth[i >> 3] + 1, my_node, c, my_depth + 1, lim, i, lane);
            }
            for (unsigned m = tie_ns; m; m &= m - 1) {
                const int q = __ffs((int)m) - 1;
                rank += beam_prefix_less(trie, B.parent[q], B.last[q], B.depth[q], my_node, c, my_depth + 1, lim, 64 + q, lane);
            }
        }
        if (stay && (tie_sn | tie_ss)) {
            for (unsigned long long m = tie_sn; m; m &= m - 1) {
                const int i = __ffsll((long long)m) - 1;
                srank += beam_prefix_less(trie, B.node[i >> 3], cand[i & 7], B.depth[i >> 3] + 1, B.parent[lane], B.last[lane], B.depth[lane], lim, i,
                                          64 + lane);
            }
            for (unsigned m = tie_ss; m; m &= m - 1) {
                const int q = __ffs((int)m) - 1;
                srank += beam_prefix_less(trie, B.parent[q], B.last[q], B.depth[q], B.parent[lane], B.last[lane], B.depth[lane], lim, 64 + q,
                                          64 + lane);
            }
        }
        if (fresh && rank < beam) {
            const int node = 1 + t * beam + rank;
            trie[node] = make_int2(my_node, c);
            N.node[rank] = node;
            N.parent[rank] = my_node;
            N.last[rank] = c;
            N.depth[rank] = my_depth + 1;
            N.pb[rank] = -INFINITY;
            N.pnb[rank] = e;
            N.tot[rank] = e;
        }
        if (stay && srank < beam) {
            N.node[srank] = B.node[lane];
            N.parent[srank] = B.parent[lane];
            N.last[srank] = B.last[lane];
            N.depth[srank] = B.depth[lane];
            N.pb[srank] = st_pb;
            N.pnb[srank] = st_pnb;
            N.tot[srank] = st_tot;
        }
        const int entries = __popcll(fresh_m) + __popc(stay_m);
        nb = entries < beam ? entries : beam;
        cur ^= 1;
        beam_sync<LDS_TRIE>();  // the new slots and the trie nodes written above, before anyone reads them
    }
    const BeamSlots& F = slots[cur];
    const int cnt = nb < nbest ? nb : nbest;
    if (lane < nbest) {
        const int64_t h = seg * nbest + lane;
        int32_t* o = out_tok + h * w;
        if (lane < cnt) {
            const int d = F.depth[lane] < frames ? F.depth[lane] : frames;  // a depth never exceeds the frames; the store range is held to it
            int rest = F.parent[lane], lab = F.last[lane];
            for (int i = d - 1; i >= 0; --i) {  // from the back; d <= frames <= w
                o[i] = lab;
                const int2 x = trie[rest];
                rest = x.x;
                lab = x.y;
            }
            out_len[h] = d;
            out_score[h] = (float)F.tot[lane];
        } else {
            out_len[h] = 0;
            out_score[h] = -INFINITY;
        }
    }
    if (lane == 0) out_cnt[seg] = cnt;
    for (int n = 0; n < nbest; ++n) {
        int32_t* o = out_tok + (seg * nbest + n) * w;
        const int d = n < cnt ? (F.depth[n] < frames ? F.depth[n] : frames) : 0;
        for (int64_t col = (int64_t)d + lane; col < w; col += 64) o[col] = -1;
    }
}

// ---- CTC forced alignment of a known transcript (apps.ctc_forced_align on the device) ---------------------------------------------
// The lattice of a transcript of L labels has states s = 0 .. 2 L, even = blank, odd = label (s - 1) / 2.  One wavefront a segment:
// lane l owns the SPL states [SPL l, SPL l + SPL) in registers, float64.  A frame is, per state from the lane's last down to its first
// (in place: a state's predecessors are the ones below it, not yet overwritten),
//     best = stay;  if (step > best) best = step;  if (skip allowed && skip > best) best = skip;      alpha = best + (double)emission
// a skip being allowed into an odd state whose label differs from the label before it.  SPL is even, so a lane's first state is a blank
// (no skip into it) and its second an odd one: the ONE value that crosses the lane boundary is lane l - 1's last state, which is the
// first state's step and the second state's skip (one 64-bit move up the wave a frame).  The choice made, 0 / 1 / 2 = how far down the
// predecessor is, is the state's back-pointer: 2 bits a state, one word of 2 SPL bits a lane a frame, 64 words a frame whatever the
// transcript's length -- 16 SPL bytes a frame; the words of a segment's frames live in LDS while the longest segment's fit
// kAlignLdsBytes, else in the context's scratch block (16 SPL * most frames of a segment bytes a segment).
// TOTAL: beside alpha the same recurrence with logaddexp64 for the maximum, paired ((stay + step) + skip): the CTC likelihood.
// The next frame's emissions (the blank's and the lane's SPL / 2 labels') are requested before this frame's maxima are taken.
// Lane 0 then walks the back-pointers from the better end state (2 L unless 2 L - 1 is strictly greater) and notes every label's first
// and last frame; the lanes share the labels for the per-token scores: the float64 sum of the label's emissions over its span in frame
// order, as the path score (alpha itself) is the sum of the path's emissions in frame order.
constexpr int64_t kAlignLdsBytes = 56 * 1024;

extern __shared__ unsigned char align_bp_lds[];

template <int SPL, bool TOTAL, bool LDS_BP>
__global__ __launch_bounds__(64) void ctc_align_seg_kernel(const float* __restrict__ at, int64_t u, const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ tok_off, const int32_t* __restrict__ slots, int bslot,
                                                           int64_t skip_rows, int64_t w, int64_t bp_stride, unsigned char* bp_all,
                                                           int32_t* __restrict__ out_spans, float* __restrict__ out_scores,
                                                           float* __restrict__ out_path, float* __restrict__ out_total,
                                                           int32_t* __restrict__ out_ok) {
    static_assert(SPL == 4 || SPL == 16, "a lane's back-pointers of a frame are one byte or one 32-bit word");
    using Word = typename std::conditional<SPL == 16, uint32_t, uint8_t>::type;
    constexpr int HALF = SPL / 2;
    const int64_t seg = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t r0 = off[seg] + skip_rows, r1 = off[seg + 1];
    const int frames = r1 > r0 ? (int)(r1 - r0) : 0;
    const int64_t tk0 = tok_off[seg];
    const int len = (int)(tok_off[seg + 1] - tk0), nstates = 2 * len + 1;
    Word* const bp = reinterpret_cast<Word*>(LDS_BP ? align_bp_lds : bp_all + seg * bp_stride);
    __shared__ double s_end[4];  // alpha(2 L), alpha(2 L - 1), and the totals there
    __shared__ int s_first[512], s_last[512], s_ok;
    for (int64_t j = lane; j < w; j += 64) {
        out_spans[(seg * w + j) * 2] = -1;
        out_spans[(seg * w + j) * 2 + 1] = -1;
        out_scores[seg * w + j] = 0.0f;
    }
    for (int j = lane; j < len; j += 64) s_first[j] = 0, s_last[j] = -1;  // an empty span until the walk finds the label
    // the lane's labels as slots of `at` (a state past the last: the blank's, loaded and never used) and where a skip is allowed
    int slot[HALF];
    unsigned skip_ok = 0;
#pragma unroll
    for (int k = 0; k < HALF; ++k) {
        const int j = HALF * lane + k;
        slot[k] = j < len ? slots[tk0 + j] : bslot;
        if (j >= 1 && j < len && slots[tk0 + j - 1] != slot[k]) skip_ok |= 1u << k;
    }
    double a[SPL], tot[TOTAL ? SPL : 1];
#pragma unroll
    for (int i = 0; i < SPL; ++i) a[i] = -INFINITY;
#pragma unroll
    for (int i = 0; i < (TOTAL ? SPL : 1); ++i) tot[i] = -INFINITY;
    float eb_next = 0.0f, e_next[HALF];
    auto request = [&](int t) {
        const float* row = at + (r0 + t) * u;
        eb_next = row[bslot];
#pragma unroll
        for (int k = 0; k < HALF; ++k) e_next[k] = row[slot[k]];
    };
    if (frames > 0) request(0);
    for (int t = 0; t < frames; ++t) {
        const float eb = eb_next;
        float e[HALF];
#pragma unroll
        for (int k = 0; k < HALF; ++k) e[k] = e_next[k];
        if (t + 1 < frames) request(t + 1);
        unsigned word = 0;
        if (t == 0) {
            if (lane == 0) {
                a[0] = (double)eb;
                if (len >= 1) a[1] = (double)e[0];
                if (TOTAL) {
                    tot[0] = a[0];
                    if (len >= 1) tot[1] = a[1];
                }
            }
        } else {
            const double up_a = __shfl_up(a[SPL - 1], 1);
            const double below = lane == 0 ? -INFINITY : up_a;
            double below_tot = -INFINITY;
            if (TOTAL) {
                const double up_t = __shfl_up(tot[SPL - 1], 1);
                below_tot = lane == 0 ? -INFINITY : up_t;
            }
#pragma unroll
            for (int i = SPL - 1; i >= 0; --i) {
                const bool odd = (i & 1) != 0;
                const bool live = SPL * lane + i < nstates;
                const bool skip = odd && ((skip_ok >> (i >> 1)) & 1u);
                const double em = (double)(odd ? e[i >> 1] : eb);
                const double step = i >= 1 ? a[i - 1] : below;
                const double far = i >= 2 ? a[i - 2] : below;  // (read for odd i only: i >= 1)
                double best = a[i];
                unsigned from = 0;
                if (step > best) best = step, from = 1;
                if (skip && far > best) best = far, from = 2;
                a[i] = live ? best + em : -INFINITY;
                word |= from << (2 * i);
                if (TOTAL) {
                    const double step_t = i >= 1 ? tot[i - 1] : below_tot;
                    const double far_t = i >= 2 ? tot[i - 2] : below_tot;
                    double sum = logaddexp64(tot[i], step_t);
                    if (skip) sum = logaddexp64(sum, far_t);
                    tot[i] = live ? sum + em : -INFINITY;
                }
            }
        }
        bp[(int64_t)t * 64 + lane] = (Word)word;
    }
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = SPL * lane + i;
        if (s == 2 * len) s_end[0] = a[i];
        if (s == 2 * len - 1) s_end[1] = a[i];
        if (TOTAL && s == 2 * len) s_end[2] = tot[i];
        if (TOTAL && s == 2 * len - 1) s_end[3] = tot[i];
    }
    __syncthreads();  // s_end and the back-pointers (LDS or global) of every lane
    if (lane == 0) {
        const double x2 = s_end[0], x1 = len ? s_end[1] : -INFINITY;
        int s = (len == 0 || x2 >= x1) ? 2 * len : 2 * len - 1;
        const double best = frames == 0 ? (len == 0 ? 0.0 : -INFINITY) : s == 2 * len ? x2 : x1;
        const int ok = best != -INFINITY;
        s_ok = ok;
        out_ok[seg] = ok;
        out_path[seg] = (float)best;
        if (TOTAL) {
            double total = frames == 0 ? (len == 0 ? 0.0 : -INFINITY) : len ? logaddexp64(s_end[2], s_end[3]) : s_end[2];
            out_total[seg] = ok ? (float)total : -INFINITY;
        }
        if (ok) {
            int prev = -1;
            for (int t = frames - 1; t >= 0 && s >= 0; --t) {  // (s < 0: emissions that are no log-probabilities, NaN or +inf)
                if (s & 1) {
                    if (s != prev) s_last[s >> 1] = t;
                    s_first[s >> 1] = t;
                }
                prev = s;
                const unsigned wd = bp[(int64_t)t * 64 + s / SPL];
                s -= (int)((wd >> (2 * (s % SPL))) & 3u);
            }
        }
    }
    __syncthreads();
    if (!s_ok) return;
    for (int j = lane; j < len; j += 64) {
        const int first = s_first[j], last = s_last[j];
        const float* col = at + r0 * u + slots[tk0 + j];
        double sum = 0.0;
        for (int t = first; t <= last; ++t) sum += (double)col[(int64_t)t * u];
        out_spans[(seg * w + j) * 2] = (int32_t)(first + skip_rows);
        out_spans[(seg * w + j) * 2 + 1] = (int32_t)(last + skip_rows);
        out_scores[seg * w + j] = (float)sum;
    }
}

// image.rs:84-105 + 69-79: dst(y, x) <-src(min(floor((y + 0.5) * H / T), H - 1), min(floor((x + 0.5) * W / T), W - 1)) / 255
__global__ void image_preprocess_kernel(const uint8_t* __restrict__ rgb, int h, int w, int target, float* __restrict__ out) {
    const int total = target * target;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / target, x = i - y * target;
        int sx = (int)floorf(((float)x + 0.5f) * (float)w / (float)target);
        int sy = (int)floorf(((float)y + 0.5f) * (float)h / (float)target);
        sx = sx < w - 1 ? sx : w - 1;
        sy = sy < h - 1 ? sy : h - 1;
        const uint8_t* px = rgb + ((int64_t)sy * w + sx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(int64_t)c * total + i] = (float)px[c] / 255.0f;
    }
}

constexpr int kQueries = 300, kLogitLen = 38, kMaskDim = 32;  // image.rs:135-136,151

// image.rs:159-203: one workgroup an image (blockIdx.x); kept queries are written in query order, the rows behind them are zeros
__global__ __launch_bounds__(320) void yolo_dets_kernel(const float* __restrict__ logits_all, float img_w, float img_h, float threshold,
                                                        int num_classes, float* __restrict__ dets_all, int32_t* __restrict__ count_all) {
    __shared__ int wave_cnt[5];
    const float* logits = logits_all + (int64_t)blockIdx.x * kQueries * kLogitLen;
    float* dets = dets_all + (int64_t)blockIdx.x * kQueries * kLogitLen;
    int32_t* count = count_all + blockIdx.x;
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const float* q = logits + (int64_t)(i < kQueries ? i : 0) * kLogitLen;
    const float score = q[4];
    const float x1r = q[0], y1r = q[1], x2r = q[2], y2r = q[3];
    const bool keep = i < kQueries && !(score < threshold) && !(x2r <= x1r || y2r <= y1r);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    if (keep) {
        const float sx = img_w / 640.0f, sy = img_h / 640.0f;
        float* d = dets + (int64_t)pos * kLogitLen;
        d[0] = fmaxf(x1r * sx, 0.0f);
        d[1] = fmaxf(y1r * sy, 0.0f);
        d[2] = fminf(x2r * sx, img_w);
        d[3] = fminf(y2r * sy, img_h);
        d[4] = score;
        // `as usize` saturates (negative / NaN -> 0), then .min(num_classes - 1)
        const float cf = q[5];
        int cid = cf > 0.0f ? (cf >= 2147483520.0f ? 2147483647 : (int)cf) : 0;
        cid = cid < num_classes - 1 ? cid : num_classes - 1;
        d[5] = (float)cid;
        for (int j = 0; j < kMaskDim; ++j) d[6 + j] = q[6 + j];
    }
    const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3] + wave_cnt[4];
    if (i == 0) *count = total;
    // rows [total, 300): zeros (upstream returns a Vec of `total` detections; a fixed-width buffer that travels between ranks must not
    // carry whatever the allocation held).  The kept rows lie below `total`, written by other threads: disjoint.
    for (int r = total + i; r < kQueries; r += blockDim.x)
        for (int j = 0; j < kLogitLen; ++j) dets[(int64_t)r * kLogitLen + j] = 0.0f;
}

// image.rs:213-262: one thread per image pixel; a pixel is set when ANY kept detection covers it (order-free)
__global__ void yolo_mask_kernel(const float* __restrict__ dets_all, const int32_t* __restrict__ count_all, const float* __restrict__ feat_all,
                                 int mask_h, int mask_w, int img_w, int img_h, uint8_t* __restrict__ mask_all) {
    const int total = img_w * img_h, n = count_all[blockIdx.y];   // blockIdx.y = the image
    const float* dets = dets_all + (int64_t)blockIdx.y * kQueries * kLogitLen;
    const float* feat = feat_all + (int64_t)blockIdx.y * kMaskDim * mask_h * mask_w;
    uint8_t* mask_img = mask_all + (int64_t)blockIdx.y * total;
    const float scale_x = (float)mask_w / (float)img_w, scale_y = (float)mask_h / (float)img_h;
    const int plane = mask_h * mask_w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int iy = i / img_w, ix = i - iy * img_w;
        int mx = (int)floorf(((float)ix + 0.5f) * scale_x), my = (int)floorf(((float)iy + 0.5f) * scale_y);
        mx = mx < mask_w - 1 ? mx : mask_w - 1;
        my = my < mask_h - 1 ? my : mask_h - 1;
        const float* f = feat + my * mask_w + mx;
        uint8_t v = 0;
        for (int d = 0; d < n; ++d) {
            const float* det = dets + (int64_t)d * kLogitLen;
            const bool in_bbox = (float)ix >= det[0] && (float)ix <= det[2] && (float)iy >= det[1] && (float)iy <= det[3];
            if (!in_bbox) continue;
            float sum = 0.0f;
            for (int c = 0; c < kMaskDim; ++c) sum = sum + det[6 + c] * f[(int64_t)c * plane];  // separate multiply and add
            const float e = (float)exp((double)(-sum));  // libm expf upstream: correctly rounded, as this is
            const float mv = 1.0f / (1.0f + e);
            if (mv > 0.5f && mv * det[4] > 0.5f) v = 255;
        }
        mask_img[i] = v;
    }
}

// ---- a queue of images of different sizes: one launch in, one call out ---------------------------------------------------------------

// image_preprocess_batch's device table: where image blockIdx.y lies in the byte buffer
struct ImgSrc {
    int64_t off;
    int32_t h, w;
};

// image_preprocess_kernel per image of a packed byte buffer, grid (pixel tiles, image): every image's output is target x target
// whatever its source size.  VEC4 (target % 4 == 0: four consecutive x share a row and a plane's offset is a multiple of 16 bytes):
// a thread writes 4 x of each plane as one 16-byte store; the source reads are byte loads at whatever alignment the offsets give.
template <bool VEC4>
__global__ __launch_bounds__(256) void image_preprocess_batch_kernel(const uint8_t* __restrict__ bytes, const ImgSrc* __restrict__ tab,
                                                                     int target, float* __restrict__ out_all) {
    constexpr int PER = VEC4 ? 4 : 1;
    const ImgSrc s = tab[blockIdx.y];
    const int total = target * target;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * PER;
    if (i0 >= total) return;
    const uint8_t* rgb = bytes + s.off;
    float* out = out_all + (int64_t)blockIdx.y * 3 * total;
    const int y = i0 / target, x0 = i0 - y * target;
    int sy = (int)floorf(((float)y + 0.5f) * (float)s.h / (float)target);
    sy = sy < s.h - 1 ? sy : s.h - 1;
    float v[3][PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        int sx = (int)floorf(((float)(x0 + k) + 0.5f) * (float)s.w / (float)target);
        sx = sx < s.w - 1 ? sx : s.w - 1;
        const uint8_t* px = rgb + ((int64_t)sy * s.w + sx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = (float)px[c] / 255.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + (int64_t)c * total + i0;
        if constexpr (VEC4)
            *reinterpret_cast<float4*>(o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        else
            o[0] = v[c][0];
    }
}

// yolo_seg_postprocess_sized's device table: SizedImg[N], then the pixel kernel's work list int2[blocks] = {image, first pixel}
struct SizedImg {
    int64_t mask_off;  // of the image's first pixel in out_mask
    int64_t ws_off;    // of the image's bit tables in the workspace, in 32-bit words
    int32_t w, h;
};

constexpr int kDetWords = (kQueries + 31) / 32;  // a 300-bit set of detections
constexpr int kPixPerBlock = 2048;               // pixels of one image a block of yolo_pixels_kernel takes

// yolo_dets_kernel with the image's own size, read from the table
__global__ __launch_bounds__(320) void yolo_dets_sized_kernel(const float* __restrict__ logits_all, const SizedImg* __restrict__ tab,
                                                              float threshold, int num_classes, float* __restrict__ dets_all,
                                                              int32_t* __restrict__ count_all) {
    __shared__ int wave_cnt[5];
    const float img_w = (float)tab[blockIdx.x].w, img_h = (float)tab[blockIdx.x].h;
    const float* logits = logits_all + (int64_t)blockIdx.x * kQueries * kLogitLen;
    float* dets = dets_all + (int64_t)blockIdx.x * kQueries * kLogitLen;
    int32_t* count = count_all + blockIdx.x;
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const float* q = logits + (int64_t)(i < kQueries ? i : 0) * kLogitLen;
    const float score = q[4];
    const float x1r = q[0], y1r = q[1], x2r = q[2], y2r = q[3];
    const bool keep = i < kQueries && !(score < threshold) && !(x2r <= x1r || y2r <= y1r);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    if (keep) {
        const float sx = img_w / 640.0f, sy = img_h / 640.0f;
        float* d = dets + (int64_t)pos * kLogitLen;
        d[0] = fmaxf(x1r * sx, 0.0f);
        d[1] = fmaxf(y1r * sy, 0.0f);
        d[2] = fminf(x2r * sx, img_w);
        d[3] = fminf(y2r * sy, img_h);
        d[4] = score;
        const float cf = q[5];
        int cid = cf > 0.0f ? (cf >= 2147483520.0f ? 2147483647 : (int)cf) : 0;
        cid = cid < num_classes - 1 ? cid : num_classes - 1;
        d[5] = (float)cid;
        for (int j = 0; j < kMaskDim; ++j) d[6 + j] = q[6 + j];
    }
    const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3] + wave_cnt[4];
    if (i == 0) *count = total;
    for (int r = total + i; r < kQueries; r += blockDim.x)
        for (int j = 0; j < kLogitLen; ++j) dets[(int64_t)r * kLogitLen + j] = 0.0f;
}

// the mask cell that pixel coordinate v (an integer, as a float) reads: yolo_mask_kernel's expression, non-decreasing in v
__device__ inline int yolo_cell_of(float v, float scale, int side) {
    const int m = (int)floorf((v + 0.5f) * scale);
    return m < side - 1 ? m : side - 1;
}

// The three bit tables of an image, word-major so that neighbouring lanes touch neighbouring words:
//     cell bits [kDetWords][S S] | column bits [kDetWords][w] | row bits [kDetWords][h]          (32-bit words; S = the mask's side)
// bit (d & 31) of word d >> 5.  Grid (cell tiles + box tiles, kDetWords, image); a block whose word lies behind the image's kept
// detections leaves at once (those words are never read).  A thread owns ONE table entry and all 32 bits of its word, so the word is
// written once with a plain store: no atomics, no ballots.
//   cell tiles: the thread keeps its cell's 32 feature values in registers and walks the word's detections (uniform over the wave: the
//     coefficients are scalar loads); the sigmoid is evaluated only where the cell lies in the rectangle the box's pixels map to --
//     pixels ceil(x1) .. min(floor(x2), w - 1) are exactly those with (float)ix >= x1 && (float)ix <= x2, and the cell of a pixel is
//     non-decreasing in the pixel, so no pixel inside the box reads a cell outside [cell(first), cell(last)] -- and then exactly as
//     yolo_mask_kernel evaluates it.
//   box tiles: entry p < w is column p, else row p - w; the bit is yolo_mask_kernel's own comparison pair.
__global__ __launch_bounds__(256) void yolo_bits_kernel(const float* __restrict__ dets_all, const int32_t* __restrict__ count_all,
                                                        const float* __restrict__ feat_all, int64_t feat_stride, int side,
                                                        const SizedImg* __restrict__ tab, uint32_t* __restrict__ ws) {
    const int img = blockIdx.z, word = blockIdx.y;
    const int n = count_all[img], d0 = word * 32;
    if (d0 >= n) return;
    const int d1 = n < d0 + 32 ? n : d0 + 32;
    const SizedImg im = tab[img];
    const float* dets = dets_all + (int64_t)img * kQueries * kLogitLen;
    const int cells = side * side, cell_tiles = (cells + 255) / 256;
    uint32_t* tables = ws + im.ws_off;
    uint32_t bits = 0;
    if ((int)blockIdx.x < cell_tiles) {
        const int cell = blockIdx.x * 256 + threadIdx.x;
        if (cell >= cells) return;
        const int cy = cell / side, cx = cell - cy * side;
        const float* feat = feat_all + (int64_t)img * feat_stride + cell;
        float f[kMaskDim];
#pragma unroll
        for (int c = 0; c < kMaskDim; ++c) f[c] = feat[(int64_t)c * cells];
        const float scale_x = (float)side / (float)im.w, scale_y = (float)side / (float)im.h;
        for (int d = d0; d < d1; ++d) {
            const float* det = dets + (int64_t)d * kLogitLen;
            const float xlo = ceilf(det[0]), xhi = fminf(floorf(det[2]), (float)(im.w - 1));
            const float ylo = ceilf(det[1]), yhi = fminf(floorf(det[3]), (float)(im.h - 1));
            if (!(xlo <= xhi && ylo <= yhi)) continue;  // no pixel inside the box (det[0], det[1] >= 0: yolo_dets_sized_kernel's fmaxf)
            if (cx < yolo_cell_of(xlo, scale_x, side) || cx > yolo_cell_of(xhi, scale_x, side) || cy < yolo_cell_of(ylo, scale_y, side) ||
                cy > yolo_cell_of(yhi, scale_y, side))
                continue;
            float sum = 0.0f;
#pragma unroll
            for (int c = 0; c < kMaskDim; ++c) sum = sum + det[6 + c] * f[c];  // separate multiply and add
            const float e = (float)exp((double)(-sum));
            const float mv = 1.0f / (1.0f + e);
            if (mv > 0.5f && mv * det[4] > 0.5f) bits |= 1u << (d - d0);
        }
        tables[(int64_t)word * cells + cell] = bits;
    } else {
        const int64_t p = (int64_t)(blockIdx.x - cell_tiles) * 256 + threadIdx.x;
        if (p >= (int64_t)im.w + im.h) return;
        const bool col = p < im.w;
        const int at = (int)(col ? p : p - im.w);
        const float v = (float)at;
        for (int d = d0; d < d1; ++d) {
            const float* det = dets + (int64_t)d * kLogitLen;
            if (v >= det[col ? 0 : 1] && v <= det[col ? 2 : 3]) bits |= 1u << (d - d0);
        }
        uint32_t* t = tables + (int64_t)kDetWords * cells;
        if (col)
            t[(int64_t)word * im.w + at] = bits;
        else
            t[(int64_t)kDetWords * im.w + (int64_t)word * im.h + at] = bits;
    }
}

// block b takes kPixPerBlock pixels of image work[b].x from pixel work[b].y on: 255 where some detection has its column bit, its row
// bit and the bit of the pixel's cell set -- yolo_mask_kernel's in_bbox && mv > 0.5f && mv * score > 0.5f for that detection; only the
// ceil(count / 32) words that hold kept detections are visited
__global__ __launch_bounds__(256) void yolo_pixels_kernel(const int32_t* __restrict__ count_all, int side, const SizedImg* __restrict__ tab,
                                                          const int2* __restrict__ work, const uint32_t* __restrict__ ws,
                                                          uint8_t* __restrict__ mask_all) {
    const int2 wk = work[blockIdx.x];
    const SizedImg im = tab[wk.x];
    const int words = (count_all[wk.x] + 31) >> 5;
    const unsigned total = (unsigned)im.w * (unsigned)im.h;  // < 2^31 (checked on the host), so first pixel + 2047 fits 32 bits
    const int cells = side * side;
    const uint32_t* cellb = ws + im.ws_off;
    const uint32_t* colb = cellb + (int64_t)kDetWords * cells;
    const uint32_t* rowb = colb + (int64_t)kDetWords * im.w;
    uint8_t* mask = mask_all + im.mask_off;
    const float scale_x = (float)side / (float)im.w, scale_y = (float)side / (float)im.h;
    for (int k = 0; k < kPixPerBlock / 256; ++k) {
        const unsigned i = (unsigned)wk.y + k * 256 + threadIdx.x;
        if (i >= total) break;
        const int iy = (int)(i / (unsigned)im.w), ix = (int)(i - (unsigned)iy * (unsigned)im.w);
        const int cell = yolo_cell_of((float)iy, scale_y, side) * side + yolo_cell_of((float)ix, scale_x, side);
        uint32_t any = 0;
        for (int wd = 0; wd < words; ++wd)
            any |= colb[(int64_t)wd * im.w + ix] & rowb[(int64_t)wd * im.h + iy] & cellb[(int64_t)wd * cells + cell];
        mask[i] = any ? 255 : 0;
    }
}

}  // namespace

extern "C" {

int lele_hip_wav_to_f32(LeleCtx* ctx, const LeleTensor* bytes, int32_t bits_per_sample, int32_t num_channels, LeleBuf* out,
                        int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && bytes && out, "wav_to_f32: NULL argument");
    LELE_REQUIRE(bytes->dtype == LELE_U8 || bytes->dtype == LELE_I8, "wav_to_f32: the PCM payload must be a byte tensor");
    LELE_REQUIRE(bits_per_sample == 16 || bits_per_sample == 8, "Unsupported bits per sample: %d", bits_per_sample);  // audio.rs:64
    LELE_REQUIRE(num_channels == 1 || num_channels == 2, "wav_to_f32: %d channels (the reference handles mono and stereo)",
                 num_channels);
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t nbytes = numel(bytes);
    const int64_t samples = bits_per_sample == 16 ? nbytes / 2 : nbytes;  // chunks_exact(2): a trailing odd byte is dropped
    // stereo: samples.chunks(2) would emit a last 1-element chunk and index ch[1] out of bounds -> require whole frames
    LELE_REQUIRE(samples % num_channels == 0, "wav_to_f32: sample count %lld is not a multiple of %d channels",
                 (long long)samples, num_channels);
    const int64_t frames = samples / num_channels;
    LELE_TRY(ctx->arena_reset());
    const void* db = nullptr;
    LELE_TRY(ctx->dev_ptr(bytes, &db));
    LELE_TRY(out->reserve((size_t)frames * 4));
    if (frames) {
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((frames + 255) / 256, 8192));
        hipLaunchKernelGGL(wav_to_f32_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const uint8_t*)db, frames,
                           bits_per_sample, num_channels, (float*)out->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {frames});
}

int lele_hip_argmax_last(LeleCtx* ctx, const LeleTensor* x, LeleBuf* out, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && x && out, "argmax_last: NULL argument");
    LELE_REQUIRE(x->dtype == LELE_F32 && x->rank >= 1, "argmax_last: f32 tensor of rank >= 1 required");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t v = x->shape[x->rank - 1];
    int64_t rows = 1;
    for (int i = 0; i + 1 < x->rank; ++i) rows *= x->shape[i];
    LELE_TRY(ctx->arena_reset());
    const void* dx = nullptr;
    LELE_TRY(ctx->dev_ptr(x, &dx));
    LELE_TRY(out->reserve((size_t)std::max<int64_t>(rows, 1) * 4));
    if (rows) {
        hipLaunchKernelGGL(argmax_last_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const float*)dx, rows, v,
                           (int32_t*)out->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(x->shape, x->shape + x->rank - 1));
}

int lele_hip_token_filter(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* skip, LeleBuf* out_ids, LeleBuf* out_counts,
                          int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && ids && skip && out_ids && out_counts, "token_filter: NULL argument");
    LELE_REQUIRE(ids->dtype == LELE_I32 && ids->rank >= 1, "token_filter: i32 ids of rank >= 1 required");
    LELE_REQUIRE((skip->dtype == LELE_U8 || skip->dtype == LELE_I8) && skip->rank == 1, "token_filter: skip must be a byte vector [V]");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t t = ids->shape[ids->rank - 1];
    int64_t rows = 1;
    for (int i = 0; i + 1 < ids->rank; ++i) rows *= ids->shape[i];
    LELE_TRY(ctx->arena_reset());
    const void *di = nullptr, *ds = nullptr;
    LELE_TRY(ctx->dev_ptr(ids, &di));
    LELE_TRY(ctx->dev_ptr(skip, &ds));
    LELE_TRY(out_ids->reserve((size_t)std::max<int64_t>(rows * t, 1) * 4));
    LELE_TRY(out_counts->reserve((size_t)std::max<int64_t>(rows, 1) * 4));
    if (rows) {
        hipLaunchKernelGGL(token_filter_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const int32_t*)di, t,
                           (const uint8_t*)ds, skip->shape[0], (int32_t*)out_ids->data, (int32_t*)out_counts->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape_v(out_shape, out_rank, std::vector<int64_t>(ids->shape, ids->shape + ids->rank));
}

int lele_hip_token_filter_segments(LeleCtx* ctx, const LeleTensor* ids, const int64_t* row_offsets, int64_t count, const LeleTensor* skip,
                                   int64_t width, LeleBuf* out_ids, LeleBuf* out_counts, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && ids && skip && out_ids && out_counts, "token_filter_segments: NULL argument");
    LELE_REQUIRE(ids->dtype == LELE_I32 && ids->rank == 1, "token_filter_segments: ids must be i32 [R]");
    LELE_REQUIRE((skip->dtype == LELE_U8 || skip->dtype == LELE_I8) && skip->rank == 1, "token_filter_segments: skip must be a byte vector [V]");
    LELE_REQUIRE(count >= 0 && row_offsets, "token_filter_segments: bad row_offsets (count %lld)", (long long)count);
    const int64_t rows = ids->shape[0];
    LELE_REQUIRE(row_offsets[0] == 0 && row_offsets[count] == rows, "token_filter_segments: row_offsets must run from 0 to R = %lld (got %lld .. %lld)",
                 (long long)rows, (long long)row_offsets[0], (long long)row_offsets[count]);
    LELE_REQUIRE(width >= 0, "token_filter_segments: negative width");
    int64_t tmax = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t len = row_offsets[i + 1] - row_offsets[i];
        LELE_REQUIRE(len >= 0, "token_filter_segments: row_offsets decrease at segment %lld", (long long)i);
        LELE_REQUIRE(width == 0 || len <= width, "token_filter_segments: segment %lld has %lld rows, more than width = %lld", (long long)i,
                     (long long)len, (long long)width);
        tmax = std::max(tmax, len);
    }
    const int64_t w = width ? width : std::max<int64_t>(tmax, 1);
    LELE_REQUIRE(count < (int64_t(1) << 31) && w < (int64_t(1) << 31), "token_filter_segments: more than 2^31 segments or columns");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* doff = nullptr;
    if (count > 0) LELE_TRY(offsets_table(ctx, row_offsets, count, &doff));
    LELE_TRY(ctx->arena_reset());
    const void *di = nullptr, *ds = nullptr;
    if (rows > 0) LELE_TRY(ctx->dev_ptr(ids, &di));
    if (count > 0) LELE_TRY(ctx->dev_ptr(skip, &ds));
    LELE_TRY(out_ids->reserve((size_t)std::max<int64_t>(count * w, 1) * 4));
    LELE_TRY(out_counts->reserve((size_t)std::max<int64_t>(count, 1) * 4));
    if (count > 0) {
        hipLaunchKernelGGL(token_filter_seg_kernel, dim3((unsigned)count), dim3(256), 0, ctx->stream, (const int32_t*)di, (const int64_t*)doff,
                           (const uint8_t*)ds, skip->shape[0], w, (int32_t*)out_ids->data, (int32_t*)out_counts->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {count, w});
}

int lele_hip_token_align_segments(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* logprob, const int64_t* row_offsets, int64_t count,
                                  const LeleTensor* skip, int64_t width, LeleBuf* out_ids, LeleBuf* out_frames, LeleBuf* out_logprob,
                                  LeleBuf* out_counts, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && ids && skip && out_ids && out_frames && out_counts, "token_align_segments: NULL argument");
    LELE_REQUIRE(!logprob || out_logprob, "token_align_segments: scores given but no out_logprob");
    const bool lp_apart = !logprob || (out_logprob != out_ids && out_logprob != out_frames && out_logprob != out_counts);
    LELE_REQUIRE(out_ids != out_frames && out_ids != out_counts && out_frames != out_counts && lp_apart,
                 "token_align_segments: the output buffers must be distinct");
    LELE_REQUIRE(ids->dtype == LELE_I32 && ids->rank == 1, "token_align_segments: ids must be i32 [R]");
    LELE_REQUIRE(!logprob || (logprob->dtype == LELE_F32 && logprob->rank == 1 && logprob->shape[0] == ids->shape[0]),
                 "token_align_segments: logprob must be f32 [R], one score per id");
    LELE_REQUIRE((skip->dtype == LELE_U8 || skip->dtype == LELE_I8) && skip->rank == 1, "token_align_segments: skip must be a byte vector [V]");
    LELE_REQUIRE(count >= 0 && row_offsets, "token_align_segments: bad row_offsets (count %lld)", (long long)count);
    const int64_t rows = ids->shape[0];
    LELE_REQUIRE(row_offsets[0] == 0 && row_offsets[count] == rows, "token_align_segments: row_offsets must run from 0 to R = %lld (got %lld .. %lld)",
                 (long long)rows, (long long)row_offsets[0], (long long)row_offsets[count]);
    LELE_REQUIRE(width >= 0, "token_align_segments: negative width");
    int64_t tmax = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t len = row_offsets[i + 1] - row_offsets[i];
        LELE_REQUIRE(len >= 0, "token_align_segments: row_offsets decrease at segment %lld", (long long)i);
        LELE_REQUIRE(width == 0 || len <= width, "token_align_segments: segment %lld has %lld rows, more than width = %lld", (long long)i,
                     (long long)len, (long long)width);
        tmax = std::max(tmax, len);
    }
    const int64_t w = width ? width : std::max<int64_t>(tmax, 1);
    LELE_REQUIRE(count < (int64_t(1) << 31) && w < (int64_t(1) << 31), "token_align_segments: more than 2^31 segments or columns");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* doff = nullptr;
    if (count > 0) LELE_TRY(offsets_table(ctx, row_offsets, count, &doff));
    LELE_TRY(ctx->arena_reset());
    const void *di = nullptr, *dl = nullptr, *ds = nullptr;
    if (rows > 0) LELE_TRY(ctx->dev_ptr(ids, &di));
    if (rows > 0 && logprob) LELE_TRY(ctx->dev_ptr(logprob, &dl));
    if (count > 0) LELE_TRY(ctx->dev_ptr(skip, &ds));
    const size_t cells = (size_t)std::max<int64_t>(count * w, 1) * 4;
    LELE_TRY(out_ids->reserve(cells));
    LELE_TRY(out_frames->reserve(cells));
    if (logprob) LELE_TRY(out_logprob->reserve(cells));
    LELE_TRY(out_counts->reserve((size_t)std::max<int64_t>(count, 1) * 4));
    if (count > 0) {
        hipLaunchKernelGGL(token_align_seg_kernel, dim3((unsigned)count), dim3(256), 0, ctx->stream, (const int32_t*)di, (const float*)dl,
                           (const int64_t*)doff, (const uint8_t*)ds, skip->shape[0], w, (int32_t*)out_ids->data, (int32_t*)out_frames->data,
                           logprob ? (float*)out_logprob->data : (float*)nullptr, (int32_t*)out_counts->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {count, w});
}

int lele_hip_ctc_beam_search_segments(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* logprob, const int64_t* row_offsets, int64_t count,
                                      int64_t skip_rows, int32_t blank, int32_t beam, int32_t nbest, int64_t width, LeleBuf* out_tokens,
                                      LeleBuf* out_lengths, LeleBuf* out_scores, LeleBuf* out_counts, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(ctx && ids && logprob && out_tokens && out_lengths && out_scores && out_counts, "ctc_beam_search_segments: NULL argument");
    LELE_REQUIRE(out_tokens != out_lengths && out_tokens != out_scores && out_tokens != out_counts && out_lengths != out_scores &&
                     out_lengths != out_counts && out_scores != out_counts,
                 "ctc_beam_search_segments: the output buffers must be distinct");
    LELE_REQUIRE(ids->dtype == LELE_I32 && ids->rank == 2, "ctc_beam_search_segments: ids must be i32 [R, k]");
    LELE_REQUIRE(logprob->dtype == LELE_F32 && logprob->rank == 2 && logprob->shape[0] == ids->shape[0] && logprob->shape[1] == ids->shape[1],
                 "ctc_beam_search_segments: logprob must be f32 [R, k], one score per id");
    const int64_t rows = ids->shape[0], k = ids->shape[1];
    LELE_REQUIRE(k >= 1 && k <= 8, "ctc_beam_search_segments: k = %lld outside [1, 8]", (long long)k);
    LELE_REQUIRE(beam >= 1 && beam <= 8, "ctc_beam_search_segments: beam = %d outside [1, 8]", (int)beam);
    LELE_REQUIRE(nbest >= 1 && nbest <= beam, "ctc_beam_search_segments: nbest = %d outside [1, beam = %d]", (int)nbest, (int)beam);
    LELE_REQUIRE(skip_rows >= 0 && blank >= 0, "ctc_beam_search_segments: negative skip_rows or blank");
    LELE_REQUIRE(count >= 0 && row_offsets, "ctc_beam_search_segments: bad row_offsets (count %lld)", (long long)count);
    LELE_REQUIRE(row_offsets[0] == 0 && row_offsets[count] == rows, "ctc_beam_search_segments: row_offsets must run from 0 to R = %lld (got %lld .. %lld)",
                 (long long)rows, (long long)row_offsets[0], (long long)row_offsets[count]);
    LELE_REQUIRE(width >= 0, "ctc_beam_search_segments: negative width");
    int64_t tmax = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t len = row_offsets[i + 1] - row_offsets[i];
        LELE_REQUIRE(len >= 0, "ctc_beam_search_segments: row_offsets decrease at segment %lld", (long long)i);
        const int64_t frames = std::max<int64_t>(len - skip_rows, 0);
        LELE_REQUIRE(width == 0 || frames <= width, "ctc_beam_search_segments: segment %lld has %lld frames, more than width = %lld", (long long)i,
                     (long long)frames, (long long)width);
        tmax = std::max(tmax, frames);
    }
    const int64_t w = width ? width : std::max<int64_t>(tmax, 1);
    LELE_REQUIRE(count < (int64_t(1) << 31) && w < (int64_t(1) << 31) && tmax < (int64_t(1) << 27),
                 "ctc_beam_search_segments: more than 2^31 segments or columns, or a segment of 2^27 frames");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* doff = nullptr;
    if (count > 0) LELE_TRY(offsets_table(ctx, row_offsets, count, &doff));
    LELE_TRY(ctx->arena_reset());
    const void *di = nullptr, *dl = nullptr;
    if (rows > 0) LELE_TRY(ctx->dev_ptr(ids, &di));
    if (rows > 0) LELE_TRY(ctx->dev_ptr(logprob, &dl));
    // the prefix trie: per segment the root and at most `beam` new prefixes a frame, 8 bytes a node; in LDS while it fits, else in the
    // context's scratch block
    const int64_t node_stride = 1 + tmax * beam;
    const bool lds_trie = node_stride * (int64_t)sizeof(int2) <= kBeamLdsTrieBytes;
    void* trie = nullptr;
    if (count > 0 && !lds_trie) LELE_TRY(ctx->get_scratch((size_t)(count * node_stride) * sizeof(int2), &trie));
    const size_t hyps = (size_t)std::max<int64_t>(count * nbest, 1) * 4;
    LELE_TRY(out_tokens->reserve((size_t)std::max<int64_t>(count * nbest * w, 1) * 4));
    LELE_TRY(out_lengths->reserve(hyps));
    LELE_TRY(out_scores->reserve(hyps));
    LELE_TRY(out_counts->reserve((size_t)std::max<int64_t>(count, 1) * 4));
    if (count > 0) {
        auto kernel = lds_trie ? ctc_beam_seg_kernel<true> : ctc_beam_seg_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(64), lds_trie ? (size_t)node_stride * sizeof(int2) : 0, ctx->stream,
                           (const int32_t*)di, (const float*)dl, (const int64_t*)doff, (int)k, skip_rows, (int)blank, (int)beam, (int)nbest, w,
                           node_stride, (int2*)trie, (int32_t*)out_tokens->data, (int32_t*)out_lengths->data, (float*)out_scores->data,
                           (int32_t*)out_counts->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {count, (int64_t)nbest, w});
}

namespace {
// the aligner's one table: [int64 off[count + 1]][int64 tok_off[count + 1]][int slot[labels]], a label's slot its place in `cols`
struct AlignTableArg {
    const int64_t *off, *tok_off;
    int64_t count;
    const std::vector<int32_t>* slots;
};
void build_align_table(const void* arg, std::vector<char>& blob) {
    const AlignTableArg& a = *(const AlignTableArg*)arg;
    const size_t ob = (size_t)(a.count + 1) * 8;
    blob.resize(2 * ob + a.slots->size() * 4);
    memcpy(blob.data(), a.off, ob);
    memcpy(blob.data() + ob, a.tok_off, ob);
    if (!a.slots->empty()) memcpy(blob.data() + 2 * ob, a.slots->data(), a.slots->size() * 4);
}
// a column's slot in the strictly ascending cols[ncols], or -1
int64_t align_slot(const int32_t* cols, int64_t ncols, int32_t col) {
    const int32_t* p = std::lower_bound(cols, cols + ncols, col);
    return p != cols + ncols && *p == col ? p - cols : -1;
}
}  // namespace

int lele_hip_ctc_align_segments(LeleCtx* ctx, const LeleTensor* at, const int32_t* cols, int64_t ncols, const int64_t* row_offsets, int64_t count,
                                int64_t skip_rows, int32_t blank, const int32_t* tokens, const int64_t* token_offsets, int64_t width,
                                LeleBuf* out_spans, LeleBuf* out_scores, LeleBuf* out_path, LeleBuf* out_total, LeleBuf* out_ok, int64_t* out_shape,
                                int32_t* out_rank) {
    LELE_REQUIRE(ctx && at && cols && out_spans && out_scores && out_path && out_ok, "ctc_align_segments: NULL argument");
    LeleBuf* const outs[5] = {out_spans, out_scores, out_path, out_ok, out_total};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) LELE_REQUIRE(!outs[j] || outs[i] != outs[j], "ctc_align_segments: the output buffers must be distinct");
    LELE_REQUIRE(at->dtype == LELE_F32 && at->rank == 2 && ncols >= 1 && at->shape[1] == ncols,
                 "ctc_align_segments: at must be f32 [R, U] with U = ncols = %lld columns", (long long)ncols);
    const int64_t rows = at->shape[0];
    for (int64_t c = 0; c < ncols; ++c)
        LELE_REQUIRE(cols[c] >= 0 && (c == 0 || cols[c] > cols[c - 1]), "ctc_align_segments: cols[%lld] = %d (strictly ascending, >= 0 required)",
                     (long long)c, (int)cols[c]);
    LELE_REQUIRE(skip_rows >= 0 && width >= 0, "ctc_align_segments: negative skip_rows or width");
    LELE_REQUIRE(count >= 0 && row_offsets && token_offsets, "ctc_align_segments: bad row_offsets or token_offsets (count %lld)", (long long)count);
    LELE_REQUIRE(row_offsets[0] == 0 && row_offsets[count] == rows, "ctc_align_segments: row_offsets must run from 0 to R = %lld (got %lld .. %lld)",
                 (long long)rows, (long long)row_offsets[0], (long long)row_offsets[count]);
    LELE_REQUIRE(token_offsets[0] == 0, "ctc_align_segments: token_offsets must start at 0 (got %lld)", (long long)token_offsets[0]);
    const int64_t bslot = align_slot(cols, ncols, blank);
    LELE_REQUIRE(bslot >= 0, "ctc_align_segments: blank = %d is not among the %lld listed columns", (int)blank, (long long)ncols);
    int64_t tmax = 0, lmax = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t len = row_offsets[i + 1] - row_offsets[i], labels = token_offsets[i + 1] - token_offsets[i];
        LELE_REQUIRE(len >= 0, "ctc_align_segments: row_offsets decrease at segment %lld", (long long)i);
        LELE_REQUIRE(labels >= 0, "ctc_align_segments: token_offsets decrease at segment %lld", (long long)i);
        LELE_REQUIRE(labels <= 511, "ctc_align_segments: segment %lld has a transcript of %lld labels, more than 511", (long long)i, (long long)labels);
        LELE_REQUIRE(width == 0 || labels <= width, "ctc_align_segments: segment %lld has a transcript of %lld labels, more than width = %lld",
                     (long long)i, (long long)labels, (long long)width);
        tmax = std::max(tmax, std::max<int64_t>(len - skip_rows, 0));
        lmax = std::max(lmax, labels);
    }
    const int64_t total_labels = token_offsets[count];
    LELE_REQUIRE(total_labels == 0 || tokens, "ctc_align_segments: NULL tokens");
    std::vector<int32_t> slots((size_t)total_labels);
    for (int64_t i = 0; i < count; ++i)
        for (int64_t j = token_offsets[i]; j < token_offsets[i + 1]; ++j) {
            LELE_REQUIRE(tokens[j] != blank, "ctc_align_segments: segment %lld, position %lld: the label is the blank (%d)", (long long)i,
                         (long long)(j - token_offsets[i]), (int)blank);
            const int64_t s = align_slot(cols, ncols, tokens[j]);
            LELE_REQUIRE(s >= 0, "ctc_align_segments: segment %lld, position %lld: label %d is not among the listed columns", (long long)i,
                         (long long)(j - token_offsets[i]), (int)tokens[j]);
            slots[(size_t)j] = (int32_t)s;
        }
    const int64_t w = width ? width : std::max<int64_t>(lmax, 1);
    LELE_REQUIRE(count < (int64_t(1) << 31) && tmax < (int64_t(1) << 27), "ctc_align_segments: more than 2^31 segments, or a segment of 2^27 frames");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* tab = nullptr;
    if (count > 0) {
        // keyed by the layout, the transcripts' lengths and their slots
        std::vector<int64_t> key(row_offsets, row_offsets + count + 1);
        key.insert(key.end(), token_offsets, token_offsets + count + 1);
        key.insert(key.end(), slots.begin(), slots.end());
        const AlignTableArg arg{row_offsets, token_offsets, count, &slots};
        LELE_TRY(layout_table(ctx, "calg", count, 0, key.data(), (int64_t)key.size() - 1, build_align_table, &arg, &tab));
    }
    LELE_TRY(ctx->arena_reset());
    const void* da = nullptr;
    if (rows > 0) LELE_TRY(ctx->dev_ptr(at, &da));
    // back-pointers: 2 bits a state, a lane's SPL states of a frame one word, 64 words a frame: 16 SPL bytes a frame.  4 states a lane
    // while every transcript fits them (L <= 127), else 16.
    const int spl = lmax <= 127 ? 4 : 16;
    const int64_t bp_stride = std::max<int64_t>(tmax, 1) * 16 * spl;
    const bool lds_bp = bp_stride <= kAlignLdsBytes;
    void* bp = nullptr;
    if (count > 0 && !lds_bp) LELE_TRY(ctx->get_scratch((size_t)(count * bp_stride), &bp));
    const size_t cells = (size_t)std::max<int64_t>(count * w, 1) * 4, segs = (size_t)std::max<int64_t>(count, 1) * 4;
    LELE_TRY(out_spans->reserve(2 * cells));
    LELE_TRY(out_scores->reserve(cells));
    LELE_TRY(out_path->reserve(segs));
    if (out_total) LELE_TRY(out_total->reserve(segs));
    LELE_TRY(out_ok->reserve(segs));
    if (count > 0) {
        const int which = (spl == 16 ? 4 : 0) + (out_total ? 2 : 0) + (lds_bp ? 1 : 0);
        using Kernel = decltype(&ctc_align_seg_kernel<4, false, false>);
        static const Kernel kernels[8] = {ctc_align_seg_kernel<4, false, false>,  ctc_align_seg_kernel<4, false, true>,  ctc_align_seg_kernel<4, true, false>,
                                     ctc_align_seg_kernel<4, true, true>,    ctc_align_seg_kernel<16, false, false>, ctc_align_seg_kernel<16, false, true>,
                                     ctc_align_seg_kernel<16, true, false>,  ctc_align_seg_kernel<16, true, true>};
        const size_t ob = (size_t)(count + 1) * 8;
        hipLaunchKernelGGL(kernels[which], dim3((unsigned)count), dim3(64), lds_bp ? (size_t)bp_stride : 0, ctx->stream, (const float*)da, ncols,
                           (const int64_t*)tab, (const int64_t*)((const char*)tab + ob), (const int32_t*)((const char*)tab + 2 * ob), (int)bslot,
                           skip_rows, w, bp_stride, (unsigned char*)bp, (int32_t*)out_spans->data, (float*)out_scores->data, (float*)out_path->data,
                           out_total ? (float*)out_total->data : (float*)nullptr, (int32_t*)out_ok->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {count, w});
}

int lele_hip_image_preprocess(LeleCtx* ctx, const LeleTensor* rgb, int32_t target, LeleBuf* out, int64_t* out_shape,
                              int32_t* out_rank) {
    LELE_REQUIRE(ctx && rgb && out, "image_preprocess: NULL argument");
    LELE_REQUIRE(rgb->dtype == LELE_U8 && rgb->rank == 3 && rgb->shape[2] == 3, "image_preprocess: u8 [H, W, 3] image required");
    LELE_REQUIRE(rgb->shape[0] > 0 && rgb->shape[1] > 0 && target > 0 && target <= 16384, "image_preprocess: empty image or bad target");
    LELE_REQUIRE(rgb->shape[0] < (1 << 24) && rgb->shape[1] < (1 << 24), "image_preprocess: image side exceeds 2^24");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void* dr = nullptr;
    LELE_TRY(ctx->dev_ptr(rgb, &dr));
    LELE_TRY(out->reserve((size_t)3 * target * target * 4));
    const int total = target * target;
    hipLaunchKernelGGL(image_preprocess_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, (const uint8_t*)dr,
                       (int)rgb->shape[0], (int)rgb->shape[1], target, (float*)out->data);
    LELE_HIP_CHECK(hipGetLastError());
    return set_shape(out_shape, out_rank, {1, 3, target, target});
}

int lele_hip_yolo_seg_postprocess(LeleCtx* ctx, const LeleTensor* logits, const LeleTensor* mask_features, int32_t img_width,
                                  int32_t img_height, float threshold, int32_t num_classes, LeleBuf* out_dets,
                                  LeleBuf* out_count, LeleBuf* out_mask) {
    LELE_REQUIRE(ctx && logits && mask_features && out_dets && out_count && out_mask, "yolo_seg_postprocess: NULL argument");
    const int64_t per = (int64_t)kQueries * kLogitLen;
    LELE_REQUIRE(logits->dtype == LELE_F32 && numel(logits) > 0 && numel(logits) % per == 0,
                 "yolo_seg_postprocess: logits must hold N x 300 x 38 f32 values");
    const int64_t images = numel(logits) / per;   // upstream: one image a call (image.rs:127); a batch is the same routine per image
    LELE_REQUIRE(mask_features->dtype == LELE_F32, "yolo_seg_postprocess: f32 mask features required");
    LELE_REQUIRE(img_width > 0 && img_height > 0 && (int64_t)img_width * img_height < (int64_t(1) << 31) && num_classes > 0,
                 "yolo_seg_postprocess: bad image size or class count");
    LELE_REQUIRE(numel(mask_features) % (images * kMaskDim) == 0 && images < 65536, "yolo_seg_postprocess: mask features do not match %lld images",
                 (long long)images);
    const int64_t mask_hw = numel(mask_features) / (images * kMaskDim);      // image.rs:142-145
    const int mask_h = (int)sqrtf((float)mask_hw), mask_w = mask_h;
    LELE_REQUIRE(mask_h > 0, "yolo_seg_postprocess: empty mask features");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void *dl = nullptr, *df = nullptr;
    LELE_TRY(ctx->dev_ptr(logits, &dl));
    LELE_TRY(ctx->dev_ptr(mask_features, &df));
    LELE_TRY(out_dets->reserve((size_t)(images * per) * 4));
    LELE_TRY(out_count->reserve((size_t)images * 4));
    LELE_TRY(out_mask->reserve((size_t)images * img_width * img_height));
    hipLaunchKernelGGL(yolo_dets_kernel, dim3((unsigned)images), dim3(320), 0, ctx->stream, (const float*)dl, (float)img_width, (float)img_height,
                       threshold, num_classes, (float*)out_dets->data, (int32_t*)out_count->data);
    const int total = img_width * img_height;
    hipLaunchKernelGGL(yolo_mask_kernel, dim3(std::min((total + 255) / 256, 16384), (unsigned)images), dim3(256), 0, ctx->stream,
                       (const float*)out_dets->data, (const int32_t*)out_count->data, (const float*)df, mask_h, mask_w, img_width,
                       img_height, (uint8_t*)out_mask->data);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"

namespace {
struct ImgTableArg {
    const int64_t* offsets;
    const int32_t *heights, *widths;
    int64_t count;
};
void build_img_table(const void* arg, std::vector<char>& blob) {
    const ImgTableArg& a = *(const ImgTableArg*)arg;
    blob.resize((size_t)a.count * sizeof(ImgSrc));
    ImgSrc* t = (ImgSrc*)blob.data();
    for (int64_t i = 0; i < a.count; ++i) t[i] = ImgSrc{a.offsets[i], a.heights[i], a.widths[i]};
}

// the sized post-processing's table: SizedImg[count], then yolo_pixels_kernel's work list, kPixPerBlock pixels of one image a block
struct SizedTableArg {
    const int32_t *widths, *heights;
    int64_t count, cells;
};
int64_t sized_blocks(int32_t w, int32_t h) { return ((int64_t)w * h + kPixPerBlock - 1) / kPixPerBlock; }
int64_t sized_ws_words(int64_t cells, int32_t w, int32_t h) { return (int64_t)kDetWords * (cells + w + h); }
void build_sized_table(const void* arg, std::vector<char>& blob) {
    const SizedTableArg& a = *(const SizedTableArg*)arg;
    int64_t blocks = 0;
    for (int64_t n = 0; n < a.count; ++n) blocks += sized_blocks(a.widths[n], a.heights[n]);
    blob.resize((size_t)a.count * sizeof(SizedImg) + (size_t)blocks * sizeof(int2));
    SizedImg* t = (SizedImg*)blob.data();
    int2* work = (int2*)(blob.data() + (size_t)a.count * sizeof(SizedImg));
    int64_t mask_off = 0, ws_off = 0;
    for (int64_t n = 0; n < a.count; ++n) {
        const int32_t w = a.widths[n], h = a.heights[n];
        t[n] = SizedImg{mask_off, ws_off, w, h};
        for (int64_t b = 0; b < sized_blocks(w, h); ++b) *work++ = make_int2((int)n, (int)(b * kPixPerBlock));
        mask_off += (int64_t)w * h;
        ws_off += sized_ws_words(a.cells, w, h);
    }
}
}  // namespace

extern "C" {

int lele_hip_image_preprocess_batch(LeleCtx* ctx, const LeleTensor* bytes, const int64_t* offsets, const int32_t* heights,
                                    const int32_t* widths, int64_t count, int32_t target, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank) {
    LELE_REQUIRE(ctx && bytes && out, "image_preprocess_batch: NULL argument");
    LELE_REQUIRE(bytes->dtype == LELE_U8 && bytes->rank == 1, "image_preprocess_batch: bytes must be u8 [total]");
    LELE_REQUIRE(count >= 0 && count < 65536, "image_preprocess_batch: count = %lld outside [0, 65536)", (long long)count);
    LELE_REQUIRE(count == 0 || (offsets && heights && widths), "image_preprocess_batch: NULL argument");  // (an empty std::vector's data())
    LELE_REQUIRE(target >= 1 && target <= 16384, "image_preprocess_batch: target = %d outside [1, 16384]", (int)target);
    const int64_t total = bytes->shape[0];
    for (int64_t i = 0; i < count; ++i) {
        LELE_REQUIRE(heights[i] >= 1 && widths[i] >= 1 && heights[i] < (1 << 24) && widths[i] < (1 << 24),
                     "image_preprocess_batch: image %lld is %d x %d (sides in [1, 2^24) required)", (long long)i, (int)heights[i], (int)widths[i]);
        const int64_t len = (int64_t)3 * heights[i] * widths[i];
        LELE_REQUIRE(offsets[i] >= 0 && len <= total && offsets[i] <= total - len,
                     "image_preprocess_batch: image %lld (%d x %d at offset %lld) does not lie inside the %lld bytes", (long long)i,
                     (int)heights[i], (int)widths[i], (long long)offsets[i], (long long)total);
    }
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    const void* tab = nullptr;
    if (count > 0) {
        std::vector<int64_t> key;  // the table's contents are its key
        for (int64_t i = 0; i < count; ++i) key.insert(key.end(), {offsets[i], (int64_t)heights[i], (int64_t)widths[i]});
        const ImgTableArg arg{offsets, heights, widths, count};
        LELE_TRY(layout_table(ctx, "imgb", count, 0, key.data(), (int64_t)key.size() - 1, build_img_table, &arg, &tab));
    }
    LELE_TRY(ctx->arena_reset());
    const void* db = nullptr;
    if (count > 0) LELE_TRY(ctx->dev_ptr(bytes, &db));
    const int64_t pixels = (int64_t)target * target;
    LELE_TRY(out->reserve((size_t)(count * 3 * pixels) * 4));
    if (count > 0) {
        const bool vec4 = target % 4 == 0;
        const unsigned tiles = (unsigned)((pixels / (vec4 ? 4 : 1) + 255) / 256);
        hipLaunchKernelGGL(vec4 ? image_preprocess_batch_kernel<true> : image_preprocess_batch_kernel<false>, dim3(tiles, (unsigned)count), dim3(256),
                           0, ctx->stream, (const uint8_t*)db, (const ImgSrc*)tab, (int)target, (float*)out->data);
        LELE_HIP_CHECK(hipGetLastError());
    }
    return set_shape(out_shape, out_rank, {count, 3, (int64_t)target, (int64_t)target});
}

int lele_hip_yolo_seg_postprocess_sized(LeleCtx* ctx, const LeleTensor* logits, const LeleTensor* mask_features,
                                        const int32_t* img_widths, const int32_t* img_heights, int64_t count, float threshold,
                                        int32_t num_classes, LeleBuf* out_dets, LeleBuf* out_count, LeleBuf* out_mask,
                                        int64_t* mask_offsets) {
    LELE_REQUIRE(ctx && logits && mask_features && img_widths && img_heights && out_dets && out_count, "yolo_seg_postprocess_sized: NULL argument");
    LELE_REQUIRE(out_dets != out_count && out_dets != out_mask && out_count != out_mask, "yolo_seg_postprocess_sized: the output buffers must be distinct");
    const int64_t per = (int64_t)kQueries * kLogitLen;
    LELE_REQUIRE(logits->dtype == LELE_F32 && numel(logits) > 0 && numel(logits) % per == 0,
                 "yolo_seg_postprocess_sized: logits must hold N x 300 x 38 f32 values");
    const int64_t images = numel(logits) / per;
    LELE_REQUIRE(count == images, "yolo_seg_postprocess_sized: %lld sizes for N = %lld images", (long long)count, (long long)images);
    LELE_REQUIRE(mask_features->dtype == LELE_F32 && num_classes > 0, "yolo_seg_postprocess_sized: f32 mask features and a positive class count required");
    LELE_REQUIRE(numel(mask_features) % (images * kMaskDim) == 0 && images < 65536,
                 "yolo_seg_postprocess_sized: mask features do not match %lld images", (long long)images);
    const int64_t mask_hw = numel(mask_features) / (images * kMaskDim);  // image.rs:142-145, as lele_hip_yolo_seg_postprocess reads it
    const int side = (int)sqrtf((float)mask_hw);
    LELE_REQUIRE(side > 0 && side < 32768, "yolo_seg_postprocess_sized: empty mask features, or a mask side of 2^15 or more");
    const int64_t cells = (int64_t)side * side;
    int64_t pixels = 0, ws_words = 0, blocks = 0, longest = 0;
    for (int64_t n = 0; n < images; ++n) {
        const int32_t w = img_widths[n], h = img_heights[n];
        LELE_REQUIRE(w >= 1 && h >= 1 && w < (1 << 24) && h < (1 << 24), "yolo_seg_postprocess_sized: image %lld is %d x %d (sides in [1, 2^24) required)",
                     (long long)n, (int)w, (int)h);
        pixels += (int64_t)w * h;
        LELE_REQUIRE(pixels < (int64_t(1) << 31), "yolo_seg_postprocess_sized: the masks up to image %lld hold 2^31 pixels or more", (long long)n);
        ws_words += sized_ws_words(cells, w, h);
        blocks += sized_blocks(w, h);
        longest = std::max<int64_t>(longest, (int64_t)w + h);
    }
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<int64_t> key;
    for (int64_t n = 0; n < images; ++n) key.insert(key.end(), {(int64_t)img_widths[n], (int64_t)img_heights[n]});
    const SizedTableArg arg{img_widths, img_heights, images, cells};
    const void* tab = nullptr;
    LELE_TRY(layout_table(ctx, "ysiz", cells, 0, key.data(), (int64_t)key.size() - 1, build_sized_table, &arg, &tab));
    LELE_TRY(ctx->arena_reset());
    const void *dl = nullptr, *df = nullptr;
    LELE_TRY(ctx->dev_ptr(logits, &dl));
    if (out_mask) LELE_TRY(ctx->dev_ptr(mask_features, &df));
    void* ws = nullptr;
    if (out_mask) {  // 40 * sum (S S + w + h) bytes: the arena while it holds them, else the scratch block (grown once, then kept)
        const size_t ws_bytes = (size_t)ws_words * 4;
        if (ctx->arena_used + ws_bytes + 256 <= ctx->arena_cap) LELE_TRY(ctx->arena_alloc(ws_bytes, &ws));
        else LELE_TRY(ctx->get_scratch(ws_bytes, &ws));
    }
    LELE_TRY(out_dets->reserve((size_t)(images * per) * 4));
    LELE_TRY(out_count->reserve((size_t)images * 4));
    if (out_mask) LELE_TRY(out_mask->reserve((size_t)pixels));
    const SizedImg* imgs = (const SizedImg*)tab;
    hipLaunchKernelGGL(yolo_dets_sized_kernel, dim3((unsigned)images), dim3(320), 0, ctx->stream, (const float*)dl, imgs, threshold, num_classes,
                       (float*)out_dets->data, (int32_t*)out_count->data);
    if (out_mask) {
        const unsigned tiles = (unsigned)((cells + 255) / 256 + (longest + 255) / 256);
        hipLaunchKernelGGL(yolo_bits_kernel, dim3(tiles, kDetWords, (unsigned)images), dim3(256), 0, ctx->stream, (const float*)out_dets->data,
                           (const int32_t*)out_count->data, (const float*)df, (int64_t)kMaskDim * mask_hw, side, imgs, (uint32_t*)ws);
        hipLaunchKernelGGL(yolo_pixels_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const int32_t*)out_count->data, side, imgs,
                           (const int2*)(imgs + images), (const uint32_t*)ws, (uint8_t*)out_mask->data);
    }
    LELE_HIP_CHECK(hipGetLastError());
    if (mask_offsets) {
        mask_offsets[0] = 0;
        for (int64_t n = 0; n < images; ++n) mask_offsets[n + 1] = mask_offsets[n] + (int64_t)img_widths[n] * img_heights[n];
    }
    return 0;
}

}  // extern "C"
