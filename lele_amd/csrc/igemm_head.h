// igemm_head.h -- the decode heads of the tiled i8 GEMM (included by quant.hip behind IgemmEpi and QParams, in front of igemm_kernel).
//
// A head leaves none of the product in HBM: igemm_kernel's epilogue (head_epilogue below, EM >= 3) reduces a tile of logits to one or
// a few keys per (row, column tile), head_finish_kernel reduces the column tiles of a row, launch_igemm_head runs the two.
//   EM 3 (Head::Ids)    lele_hip_fused_quantized_linear_argmax: of the result only each row's arg-max leaves the chip, as one argmax_key
//                       per (row, column tile) in epi.arg_keys.  Row context as EM 0 (any number of slices a tile).
//   EM 4 (Head::Scored) lele_hip_fused_quantized_linear_argmax_logprob: besides the key, per (row, column tile) the sum over the tile's
//                       valid columns of exp(value - the tile's maximum) in epi.arg_sums; the finish kernel rescales and adds the tiles.
//                       The maximum is the one the key fold found, so the sums are taken after it, by the same fold with plain f32 adds
//                       (commutative bit for bit, the pairing lane ^ 16, 8, 4, 2, 1 the same for every row) and joined over the waves in
//                       wave order: a row's sum depends on (n, column) only, not on where the row sits in its tile.
//   EM 5 (Head::TopK)   lele_hip_fused_quantized_linear_topk: the tile's epi.topk best keys per row instead of one -- epi.topk rounds of
//                       EM 3's fold and join over the lane's 32 kept logits.  Round j stores the tile's j-th key per row in
//                       epi.arg_keys[tile][j][row]; a column that has won a row takes no part in that row from then on (masked by COLUMN
//                       -- the lane clears its own key word of that row: equal values in other columns stay candidates), and a round that
//                       finds nothing left stores key 0.  Round 0 is EM 3's key, the sums are EM 4's, taken behind round 0.
//   EM 6 (Head::At)     lele_hip_fused_quantized_linear_logprob_at: EM 4, and a lane whose column the caller listed (epi.at_slot()[column] >= 0)
//                       stores the logits it holds of the tile's rows, raw, to epi.at_out()[row][slot]; the finish kernel, which knows the
//                       row's maximum and its log-probability, rewrites them in place as (x - maximum) + logprob -- MODE 5's slot j.
// The contracts between the heads -- scored ids are the ids-only head's, slot 0 of the k best is the scored head bit for bit -- hold
// because every step below exists once: the three modes are three instantiations of the same fold, join, sums and finish.
#pragma once

namespace {

// (value, column) as one unsigned key whose order is "greater value wins, equal values: greater column wins" (tokenizer.rs:50-61,
// Iterator::max_by keeps the last of equal maxima).  The value's bits are made order-preserving (negative: all bits flipped, else the
// sign bit set) after -0.0 is folded onto +0.0, which partial_cmp holds equal.  Every key of a real value is > 0, what a masked column carries.
__device__ __forceinline__ unsigned long long argmax_key(float v, int col) {
    unsigned b = __float_as_uint(v);
    b = b == 0x80000000u ? 0u : b;
    b ^= (unsigned)((int)b >> 31) | 0x80000000u;
    return ((unsigned long long)b << 32) | (unsigned)col;
}
// the value a key's high word was made of (-0.0 comes back as +0.0)
__device__ __forceinline__ float argmax_key_value(unsigned long long key) {
    const unsigned b = (unsigned)(key >> 32);
    return __uint_as_float((b & 0x80000000u) ? b ^ 0x80000000u : ~b);
}
// x into a list sorted greatest first; the least of the nine falls out.  Keys of real candidates are distinct (they carry their column),
// so the list a set of keys leaves does not depend on the order they came in.
__device__ __forceinline__ void topk_insert(unsigned long long (&list)[8], unsigned long long x) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned long long hi = max(list[i], x);
        x = min(list[i], x);
        list[i] = hi;
    }
}

// the tile row behind register r of accumulator tile i (v_mfma_i32_32x32x32_i8's result layout: half-wave hv holds rows 4 hv + [0, 4)
// of every group of eight), for the wave in row wm of the workgroup's WM x WN waves
template <int TMT>
__device__ __forceinline__ int acc_row(int wm, int hv, int i, int r) {
    return wm * TMT * 32 + i * 32 + 4 * hv + (r & 3) + 8 * (r >> 2);
}
// the tile row whose result half_wave_fold leaves in lane l31 of half-wave hv: the lane's value l31 of 32
template <int TMT>
__device__ __forceinline__ int owner_row(int wm, int hv, int l31) {
    return acc_row<TMT>(wm, hv, l31 >> 4, l31 & 15);
}

// the two operations the heads fold and join with: op(what the lane kept, what came in)
struct HeadMax {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long keep, unsigned long long got) const { return max(keep, got); }
};
struct HeadAdd {
    __device__ __forceinline__ float operator()(float keep, float got) const { return keep + got; }
};
// Across the 32 lanes of a half-wave (the columns), a lane holding 32 values (the rows), value(t) for t < 32: each step a lane hands
// half of its values to its partner and folds the partner's other half into its own, so 16 + 8 + 4 + 2 + 1 exchanges leave lane l31
// with value l31 of all 32 lanes, which is returned.  The values are asked for inside the first step, so that a caller whose values are
// cheap to make holds 16 of them and not 32.  (Plain `inline`, on purpose: forced into igemm_kernel before the compiler's first passes,
// the selects below were rewritten there into selects of the array INDEX, and v[] went to scratch memory.)
template <class T, class Op, class Value>
__device__ inline T half_wave_fold(int lane, Op op, Value value) {
    T v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const bool up = (lane & 16) != 0;
        const T lo = value(t), hi = value(t + 16);
        v[t] = op(up ? hi : lo, (T)__shfl_xor(up ? lo : hi, 16));
    }
#pragma unroll
    for (int s = 1; s < 5; ++s) {
        const int half = 16 >> s;
        const bool up = (lane & half) != 0;
#pragma unroll
        for (int t = 0; t < half; ++t) {
            const T send = up ? v[t] : v[t + half];
            const T keep = up ? v[t + half] : v[t];
            v[t] = op(keep, (T)__shfl_xor(send, half));
        }
    }
    return v[0];
}
// a row's results of the WN waves, s[WN][BM] in LDS, in wave order
template <int BM, int WN, class T, class Op>
__device__ __forceinline__ T wave_join(const T* s, int row, Op op) {
    T x = s[row];
#pragma unroll
    for (int w = 1; w < WN; ++w) x = op(x, s[w * BM + row]);
    return x;
}

// where a thread stands in igemm_kernel's tile
struct HeadPos {
    int tid, lane, wm, wn;
    unsigned tx;  // column tile
    int64_t m0, rows;
    int rows_here;
    __device__ __forceinline__ int hv() const { return lane >> 5; }
    __device__ __forceinline__ int l31() const { return lane & 31; }
};
// EM 4 / 5: per row the sum over the tile's valid columns of exp(value - s_max[row]), value(t) the lane's 32 logits, into epi.arg_sums.
// Nothing for a padded column (its value is the clamped column's).  Ends behind a barrier's reads of s_sum.
template <int BM, int WN, int TMT, class Value>
__device__ __forceinline__ void tile_sums(const IgemmEpi& epi, const HeadPos& p, bool valid, const float* s_max, float* s_sum, Value value) {
    float val[TMT * 16];
#pragma unroll
    for (int i = 0; i < TMT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __expf(value(i * 16 + r) - s_max[acc_row<TMT>(p.wm, p.hv(), i, r)]);
            val[i * 16 + r] = valid ? e : 0.0f;
        }
    s_sum[p.wn * BM + owner_row<TMT>(p.wm, p.hv(), p.l31())] = half_wave_fold<float>(p.lane, HeadAdd(), [&](int t) { return val[t]; });
    __syncthreads();
    if (p.tid < p.rows_here) epi.arg_sums[(int64_t)p.tx * p.rows + p.m0 + p.tid] = wave_join<BM, WN>(s_sum, p.tid, HeadAdd());
}

// igemm_kernel's epilogue for EM >= 3, behind the K loop's last barrier: `lds` is the K loop's LDS, s_ca / s_rterm / s_ds the tile's row terms
template <int EM, int BM, int WM, int WN, int TMT, int TNT>
__device__ __forceinline__ void head_epilogue(const IgemmEpi& epi, const v16i (&acc)[TMT][TNT], const IgemmEpi::ColCtx (&cc)[TNT],
                                              const int (&cols)[TNT], const int* s_ca, const int* s_rterm, const float* s_ds, char* lds,
                                              int tid, int wm, int wn, unsigned tx, int64_t m0, int64_t rows, int n) {
    constexpr int NT = WM * WN * 64;
    static_assert(TMT == 2, "half_wave_fold folds 32 rows a lane onto the 32 lanes of a half-wave");
    static_assert(EM == 3 || (TNT == 1 && NT >= BM), "EM 4 / 5 / 6: one column a lane, one thread a row in the joins");
    constexpr bool SUMS = EM == 4 || EM == 6;  // EM 6 is EM 4 with the listed columns' values stored behind it
    const HeadPos p{tid, tid & 63, wm, wn, tx, m0, rows, (int)(rows - m0 < BM ? rows - m0 : BM)};
    const int hv = p.hv(), rows_here = p.rows_here;
    auto value = [&](int i, int j, int r) {
        const int lr = acc_row<TMT>(wm, hv, i, r);
        const IgemmEpi::RowCtx rc{s_ca[lr], s_rterm[lr], s_ds[lr], nullptr};
        return epi.value24(rc, cc[j], acc[i][j][r]);
    };
    const int mine = owner_row<TMT>(wm, hv, p.l31());
    unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(lds);  // [WN][BM]
    float* const s_max = reinterpret_cast<float*>(lds + WN * BM * 8);              // EM 4 / 5: [BM], the tile's maximum per row
    float* const s_sum = s_max + BM;                                               // EM 4 / 5: [WN][BM]
    if constexpr (EM == 5) {
        const int kk = epi.topk;
        // the lane's 32 logits as the high words of their keys: a key is the register pair {column, word}, made by no instruction.  (The
        // sums take the values back out, -0.0 as +0.0, which no difference to a maximum and no exponential tells apart; kept as values the
        // rounds' loop would hold both forms, 32 registers more than two workgroups a CU leave.)  Word 0 is "no candidate": a padded
        // column from the start, a column that has won the row from then on -- masked by COLUMN, equal values elsewhere stay.  Every
        // real value's word is > 0.
        const bool valid = cols[0] < n;
        unsigned kb[TMT * 16];
#pragma unroll
        for (int i = 0; i < TMT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) kb[i * 16 + r] = valid ? (unsigned)(argmax_key(value(i, 0, r), 0) >> 32) : 0u;
        unsigned* const s_win = reinterpret_cast<unsigned*>(s_sum + WN * BM);  // [BM], the round's winning column per row
        for (int j = 0; j < kk; ++j) {
            // the keys are made inside the fold's first step, so that 16 of them are live and not 32 (registers: two workgroups a CU need <= 128)
            s_key[wn * BM + mine] =
                half_wave_fold<unsigned long long>(p.lane, HeadMax(), [&](int t) { return ((unsigned long long)kb[t] << 32) | (unsigned)cols[0]; });
            __syncthreads();
            if (tid < BM) {  // rows past the last are the last row again (clamped context): computed, never stored
                const unsigned long long best = wave_join<BM, WN>(s_key, tid, HeadMax());
                const bool any = (best >> 32) != 0ull;  // nothing left in this tile: key 0, and no column matches
                if (tid < rows_here) epi.arg_keys[((int64_t)tx * kk + j) * rows + m0 + tid] = any ? best : 0ull;
                if (j == 0) s_max[tid] = argmax_key_value(best);
                s_win[tid] = any ? (unsigned)best : ~0u;
            }
            __syncthreads();  // (the next round's s_key stores come after every read of this round's; its s_win stores after its first barrier)
            if (j == 0) tile_sums<BM, WN, TMT>(epi, p, valid, s_max, s_sum, [&](int t) { return argmax_key_value((unsigned long long)kb[t] << 32); });
            if (j + 1 == kk) break;  // nothing follows the last round's winners
#pragma unroll
            for (int i = 0; i < TMT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    kb[i * 16 + r] = s_win[acc_row<TMT>(wm, hv, i, r)] == (unsigned)cols[0] ? 0u : kb[i * 16 + r];
        }
    } else {
        float val[SUMS ? TMT * 16 : 1];  // EM 4 / 6: the lane's 32 logits, kept for the sums
        // a lane holds 32 rows x TNT columns: its best key per row over its own valid columns (a padded column's context is the clamped
        // column's, so it is masked to 0, below every real key)
        unsigned long long key[TMT * 16];
#pragma unroll
        for (int i = 0; i < TMT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                unsigned long long best = 0ull;
#pragma unroll
                for (int j = 0; j < TNT; ++j) {
                    const float v = value(i, j, r);
                    if constexpr (SUMS) val[i * 16 + r] = v;
                    const unsigned long long kj = argmax_key(v, cols[j]);
                    best = max(best, cols[j] < n ? kj : 0ull);
                }
                key[i * 16 + r] = best;
            }
        // across the WN waves in the K loop's LDS, then one store per row of the tile
        s_key[wn * BM + mine] = half_wave_fold<unsigned long long>(p.lane, HeadMax(), [&](int t) { return key[t]; });
        __syncthreads();
        if constexpr (SUMS) {
            if (tid < BM) {  // rows past the last are the last row again (clamped context): computed, never stored
                const unsigned long long best = wave_join<BM, WN>(s_key, tid, HeadMax());
                if (tid < rows_here) epi.arg_keys[(int64_t)tx * rows + m0 + tid] = best;
                s_max[tid] = argmax_key_value(best);
            }
            __syncthreads();
            tile_sums<BM, WN, TMT>(epi, p, cols[0] < n, s_max, s_sum, [&](int t) { return val[t]; });
            if constexpr (EM == 6) {  // a listed column: the lane's values of the tile's real rows, each to its row's slot
                const int slot = cols[0] < n ? epi.at_slot()[cols[0]] : -1;
                if (slot >= 0) {
#pragma unroll
                    for (int i = 0; i < TMT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = acc_row<TMT>(wm, hv, i, r);
                            LELE_DEV_ASSERT(slot < epi.at_ncols());
                            if (lr < rows_here) epi.at_out()[(m0 + lr) * epi.at_ncols() + slot] = val[i * 16 + r];
                        }
                }
            }
        } else {
            for (int t = tid; t < rows_here; t += NT) epi.arg_keys[(int64_t)tx * rows + m0 + t] = wave_join<BM, WN>(s_key, t, HeadMax());
        }
    }
}

// The column tiles' keys and sums -> a row's ids (and log-probabilities).  Nothing depends on the order the tiles ran in.  A workgroup
// takes 16 rows; 16 threads a row share its tiles (a row's whole list behind ONE thread is a chain of ~200 loads: 45 us at any size):
// thread g takes tiles g, g + 16, .. in that order, thread 0 joins the 16 threads' results from LDS in thread order.
//   MODE 3: keys [tiles][rows] -> ids [rows], the greatest key's column.
//   MODE 4: ... with the winner's log-probability: with M the greatest key and m_t the maximum of tile t (its key's high word),
//           S = sum_t sums[t] * exp(m_t - M) and logprob = -ln S, never value - (max + ln S).  The order of the additions is a function
//           of the tile count alone, at most 15 + ceil(tiles / 16) deep.
//   MODE 5: keys [tiles][k][rows] -> a row's k greatest keys as ids [rows][k] and log-probabilities: thread g keeps the 8 greatest keys
//           of its tiles, thread 0 merges the 16 lists.  Slot 0's log-probability is MODE 4's, from the tiles' round-0 keys and sums;
//           slot j's is (v_j - v_0) + logprob_0 with the values the keys carry.  Key 0 is "no candidate" (fewer than k columns): id -1, -inf.
//   MODE 6: MODE 4, then the workgroup's 16 rows x ncols raw values in `at` (one contiguous stretch) in place as (x - v_0) + logprob_0,
//           MODE 5's formula, by all 256 threads.
template <int MODE>
__global__ __launch_bounds__(256) void head_finish_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ sums, int64_t rows,
                                                          int tiles, int k, int32_t* __restrict__ ids, float* __restrict__ logprob,
                                                          float* __restrict__ at, int ncols) {
    constexpr bool SCORED = MODE >= 4, LIST = MODE == 5, AT = MODE == 6;
    constexpr int L = LIST ? 8 : 1;
    __shared__ unsigned long long s_list[16][L][17];
    __shared__ float s_part[SCORED ? 16 : 1][17];
    __shared__ float s_row[AT ? 2 : 1][16];  // MODE 6: a row's maximum and log-probability
    const int rr = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int64_t r = (int64_t)blockIdx.x * 16 + rr;
    unsigned long long list[L] = {};
    if (r < rows) {
#pragma unroll(LIST ? 2 : 8)
        for (int t = g; t < tiles; t += 16) {
            if constexpr (LIST) {  // a tile's keys are requested together (a load behind every insertion is a chain of ~50 round trips)
                unsigned long long x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = j < k ? keys[((int64_t)t * k + j) * rows + r] : 0ull;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x[j] > list[7]) topk_insert(list, x[j]);
            } else {
                list[0] = max(list[0], keys[(int64_t)t * rows + r]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < L; ++i) s_list[g][i][rr] = list[i];
    __syncthreads();
    unsigned long long best = list[0];
    auto join_best = [&](int from) {
#pragma unroll
        for (int o = from; o < 16; ++o) best = max(best, s_list[o][0][rr]);
    };
    float part = 0.0f, mx = 0.0f;
    if constexpr (SCORED) {
        join_best(0);  // every thread: the row's maximum
        mx = argmax_key_value(best);
        if (r < rows) {
#pragma unroll 8
            for (int t = g; t < tiles; t += 16) {
                const int64_t at = (int64_t)t * rows + r;
                part += sums[at] * __expf(argmax_key_value(keys[LIST ? (int64_t)t * k * rows + r : at]) - mx);
            }
        }
        s_part[g][rr] = part;
        __syncthreads();
    }
    if (g == 0 && r < rows) {
        if constexpr (!SCORED) join_best(1);
        if constexpr (SCORED) {
#pragma unroll
            for (int o = 1; o < 16; ++o) part += s_part[o][rr];
        }
        if constexpr (LIST) {
            for (int o = 1; o < 16; ++o)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned long long x = s_list[o][i][rr];
                    if (x > list[7]) topk_insert(list, x);
                }
        }
        if constexpr (!LIST) ids[r] = (int32_t)(unsigned)best;
        const float lp0 = SCORED ? 0.0f - logf(part) : 0.0f;  // S == 1 gives +0.0
        if constexpr (LIST) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < k) {
                    const bool none = list[j] == 0ull;
                    ids[r * k + j] = none ? -1 : (int32_t)(unsigned)list[j];
                    logprob[r * k + j] = j == 0 ? lp0 : none ? -INFINITY : (argmax_key_value(list[j]) - mx) + lp0;
                }
        } else if constexpr (SCORED) {
            logprob[r] = lp0;
        }
        if constexpr (AT) s_row[0][rr] = mx, s_row[1][rr] = lp0;
    }
    if constexpr (AT) {
        __syncthreads();
        const int64_t r0 = (int64_t)blockIdx.x * 16;
        const int here = (int)(rows - r0 < 16 ? rows - r0 : 16);
        float* const a = at + r0 * ncols;
        for (int e = threadIdx.x; e < here * ncols; e += 256) {
            const int row = e / ncols;
            a[e] = (a[e] - s_row[0][row]) + s_row[1][row];
        }
    }
}

// ------------------------------------------------------------------------------------------ host side
enum class Head { None, Ids, Scored, TopK, At };  // igemm_kernel EM 0 / 3 / 4 / 5 / 6
// what a caller wants in place of the product
struct HeadReq {
    Head mode = Head::None;  // Ids: `out` receives argmax_last of the result as i32 [rows], the result itself is never stored
    int k = 1;               // TopK: the k best a row, 1 .. 8 -- `out` i32 [rows][k], logprob f32 [rows][k]
    LeleBuf* logprob = nullptr;  // Scored / TopK / At: the log-probabilities of the ids, f32
    // At: the caller's columns (host, strictly ascending, validated), `at` f32 [rows][ncols] their log-probabilities; at_slot is the
    // column -> slot map [n] on the device (-1: not listed), part of the call's one table
    const int32_t* cols = nullptr;
    int64_t ncols = 0;
    LeleBuf* at = nullptr;
    const int* at_slot = nullptr;
    explicit operator bool() const { return mode != Head::None; }
    bool scored() const { return mode == Head::Scored || mode == Head::TopK || mode == Head::At; }
    bool listed() const { return mode == Head::At; }
    bool topk() const { return mode == Head::TopK; }
};
// the tables between the two kernels and the results: keys [column tiles][k][rows], sums [column tiles][rows], ids / logprob [rows][k]
struct HeadOut {
    unsigned long long* keys = nullptr;
    float* sums = nullptr;  // scored heads only, logprob with it
    int32_t* ids = nullptr;
    float* logprob = nullptr;
    float* at = nullptr;
    void results(const LeleBuf* out, const HeadReq& head) {  // all reserved
        ids = (int32_t*)out->data, logprob = head.scored() ? (float*)head.logprob->data : nullptr;
        at = head.listed() ? (float*)head.at->data : nullptr;
    }
};
size_t head_key_bytes(int64_t rows, int64_t n) { return (size_t)rows * (size_t)((n + 127) / 128) * 8; }
size_t head_sum_bytes(int64_t rows, int64_t n) { return (size_t)rows * (size_t)((n + 127) / 128) * 4; }
// The tables' place.  The k-best head's two, rows * ceil(n / 128) * (8 k + 4) bytes together, live in the context's scratch block, not
// in the staging arena: at 64 x 171 rows and k = 4 they are 77 MB, more than the arena holds, and an arena that overflows cannot be
// captured; the scratch block grows in the eager run that a capture needs anyway.  The single tables go to the arena.
int head_workspace(LeleCtx* ctx, const HeadReq& head, int64_t rows, int64_t n, HeadOut* o) {
    void *keys = nullptr, *sums = nullptr;
    if (head.topk()) {
        const size_t key_bytes = (size_t)head.k * head_key_bytes(rows, n);
        LELE_TRY(ctx->get_scratch(key_bytes + head_sum_bytes(rows, n), &keys));
        sums = (char*)keys + key_bytes;
    } else {
        LELE_TRY(ctx->arena_alloc(head_key_bytes(rows, n), &keys));
        if (head.scored()) LELE_TRY(ctx->arena_alloc(head_sum_bytes(rows, n), &sums));
    }
    o->keys = (unsigned long long*)keys, o->sums = (float*)sums;
    return 0;
}

template <int BM, int BN, int WM, int WN, int BKB /* bytes of K per LDS tile: 64 or 128 */, int OCC = 1, int EM = 0>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(OCC))) void igemm_kernel(const int8_t* __restrict__ a, const int8_t* __restrict__ b,
                                                            int64_t rows, int n, int kp, int64_t b_batch_stride,
                                                            int m_per_batch, IgemmEpi epi);  // (quant.hip)
// a head: the tiled kernel in its big-shape configuration with the head's epilogue, then the finish kernel over its column tiles
// *name: what was launched, as lele_hip_last_route reports it
int launch_igemm_head(LeleCtx* ctx, const int8_t* aq, const int8_t* wt, int64_t rows, int n, int kp, int m, const IgemmEpi& epi_in,
                      const HeadReq& head, const HeadOut& o, const char** name) {
    *name = head.topk() ? "igemm.head_topk" : head.listed() ? "igemm.head_at" : head.scored() ? "igemm.head_scored" : "igemm.head_ids";
    LELE_REQUIRE(rows < (int64_t(128) * 65535), "quantized GEMM: more than 128 x 65535 rows");
    constexpr size_t lds = (size_t)2 * (128 + 128) * (128 + 16);
    IgemmEpi epi = epi_in;
    epi.arg_keys = o.keys, epi.arg_sums = o.sums, epi.topk = head.topk() ? head.k : 0;
    if (head.listed()) epi.out = o.at, epi.q_rowsum = const_cast<int*>(head.at_slot), epi.topk = (int)head.ncols;  // (IgemmEpi: EM 6)
    const dim3 grid((n + 127) / 128, (unsigned)((rows + 127) / 128));
    // EM 5, <= 128 registers: two workgroups a CU, as EM 3 / EM 4 get by themselves
    auto kern = head.topk()     ? igemm_kernel<128, 128, 2, 4, 128, 4, 5>
                : head.listed() ? igemm_kernel<128, 128, 2, 4, 128, 1, 6>
                : head.scored() ? igemm_kernel<128, 128, 2, 4, 128, 1, 4>
                                : igemm_kernel<128, 128, 2, 4, 128, 1, 3>;
    auto finish = head.topk() ? head_finish_kernel<5> : head.listed() ? head_finish_kernel<6> : head.scored() ? head_finish_kernel<4> : head_finish_kernel<3>;
    LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(kern), (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, ctx->stream, aq, wt, rows, n, kp, (int64_t)0, m, epi);
    hipLaunchKernelGGL(finish, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, ctx->stream, (const unsigned long long*)o.keys, (const float*)o.sums, rows,
                       (int)grid.x, head.k, o.ids, o.logprob, o.at, (int)head.ncols);
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace
