// frontend.hip -- SenseVoiceFrontend on gfx950: PCM -> (x32768, mean, pre-emphasis, Hann) -> 512-pt FFT ->
// power -> sparse mel -> ln -> LFR, one launch pair per batch of utterances.
//
// Replaces /root/reference/src/features/pipeline.rs:38-193 (+ window.rs, fft.rs, mel.rs, lfr.rs) and
// /root/reference/src/kernels/fft.rs:51-266.
//
// Numerics contract: the power spectrum is BIT-EXACT with the reference's x86 path (see fe_core.h for why a
// merely "accurate" FFT is not enough); the mel sum uses the reference's order and roundings; only logf may
// differ in the last ulp.  Two kernels:
//   fe_frame_sum_kernel : the per-frame mean is a sequential f32 sum of 400 samples (pipeline.rs:115-116);
//                         reproduced exactly by giving each LANE one frame (64 independent chains per wave)
//                         and transposing the PCM tile through LDS so every step is a conflict-free row read.
//   fe_main_kernel      : 16 lanes per frame, 4 frames per wave pass; stages 1-5 in registers, one LDS
//                         exchange (two 2 KB rounds), stages 6-9 in registers, power -> LDS (aliasing the
//                         exchange buffer) -> lane-per-filter sparse mel -> ln -> LFR scatter store.
// HBM traffic per utterance: PCM read once by each kernel (the second read is an L2/MALL hit for batches
// below the 256 MiB Infinity Cache) + the LFR output; algorithmic bytes = 4*S + 4*T*560.
#include <type_traits>
#include "common.h"
#include "fe_core.h"

#include <math.h>

#include <algorithm>

using namespace lele;

namespace {

constexpr int kMaxMelRounds = 8;  // n_mels <= 128 on the fast path

struct FeDev {                 // device tables (all owned by LeleFrontend)
    const float* tw_re;        // 511 (+1 pad) reference twiddle table
    const float* tw_im;
    const float2* tw;          // same, interleaved, for LDS staging
    const float* window;       // [frame_len]
    const float* melw;         // [total_steps][16]: weight of step t for lane pm
    const float* melw_lds;     // default bank only: the same 640 weights as the kernel's LDS image ([chunk][lane][4], kMelLdsFloats)
    const int* mel_start;      // [rounds*16] first bin of filter m (0 for padding filters)
    const int* mel_step_off;   // [rounds+1] first step of each round in melw
    int mel_rounds;            // ceil(n_mels/16)
    int mel_steps;             // total steps (rows of melw)
    int n_mels;
    int lfr_m, lfr_n;
    int tile_dma;              // aligned runs of the fused kernels are staged by direct-to-LDS loads (LELE_HIP_FE_TILE_DMA, default 1)
    const float2* tw_conj;     // tw with the entries of primed lanes conjugated (fe::tw_conj_image): what phase B reads behind phase_a_conj
};

// Which 64-frame block of which utterance a workgroup takes.  compute / compute_batch: block x of utterance y of the grid (equal-length
// utterances utt_stride samples apart).  compute_segments: the kernel has located the block's segment in its table and offset every
// pointer to it; the body then sees ONE utterance (y = 0) and the block's index inside the segment.
struct GridBlock {
    __device__ __forceinline__ unsigned x() const { return blockIdx.x; }
    __device__ __forceinline__ unsigned y() const { return blockIdx.y; }
};
struct SegBlock {
    unsigned bx;
    __device__ __forceinline__ unsigned x() const { return bx; }
    __device__ __forceinline__ unsigned y() const { return 0u; }
};

// One segment of compute_segments (a (start, length) range of the PCM buffer with at least one frame), built on the host.
struct FeSeg {
    int64_t start, len;         // samples
    int64_t num_frames, t_lfr;  // as compute() gives them for pcm[start, start + len)
    int64_t row0;               // first output row of the packed result
    int64_t block0;             // first 64-frame block of the 1-D grid
};

// ------------------------------------------------------------------------------------------------------
// Kernel 1: exact sequential frame sums.  grid (ceil(F/64), batch), block 64.
// ------------------------------------------------------------------------------------------------------
constexpr int kSumRows = 66;     // hop-sized rows covered by 64 consecutive frames (64 + 2 of overlap, 400 = 2.5 hops)
constexpr int kSumPitch = 164;   // floats per row (656 B, 16-B aligned): lane l reads row l(+1,+2) with ds_read_b128
                                 // at word 164*l = 36*l (mod 64) -> a 16-lane group covers all 64 banks exactly once

__global__ __launch_bounds__(64) void fe_frame_sum_kernel(const float* __restrict__ pcm, int64_t utt_stride,
                                                          int64_t pcm_len, int64_t num_frames,
                                                          float* __restrict__ mean_out, int aligned16) {
    // The 64 frames of this block span one contiguous run of samples; it is read from HBM exactly once
    // (linear, coalesced float4) and laid out as [hop row][offset in hop]: frame i = rows i, i+1 and half of i+2.
    __shared__ __attribute__((aligned(16))) float tile[kSumRows * kSumPitch];
    const int lane = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * 64;
    const float* base = pcm + (int64_t)blockIdx.y * utt_stride;
    const int64_t s0 = f0 * fe::kHop;  // first sample of the run
    constexpr int kVecPerRow = fe::kHop / 4;
    constexpr int kVecs = kSumRows * kVecPerRow;
    constexpr int kIters = (kVecs + 63) / 64;  // 42 float4 per lane
    constexpr int kBatch = 14;                  // loads kept in flight together (56 VGPRs)
    static_assert(kIters % kBatch == 0, "batching");
    for (int b0 = 0; b0 < kIters; b0 += kBatch) {
        float4 st[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int idx = (b0 + u) * 64 + lane;
            int64_t s = s0 + 4 * (int64_t)idx;
            // clamp instead of branching so that every load of the batch is issued before the first wait; lanes
            // that would read past the utterance only ever feed frames >= num_frames, whose sums are discarded
            if (s + 3 >= pcm_len) s = aligned16 ? ((pcm_len - 4) & ~int64_t(3)) : (pcm_len - 4);
            if (s < 0) s = 0;
            const float* src = base + s;
            if (aligned16) {
                st[u] = *reinterpret_cast<const float4*>(src);
            } else {
                st[u] = make_float4(src[0], src[1], src[2], src[3]);
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int idx = (b0 + u) * 64 + lane;
            if (idx < kVecs) {
                float4 xv = st[u];
                // 1. Scale (pipeline.rs:90-112): exact multiplication by 2^15
                xv.x *= 32768.0f;
                xv.y *= 32768.0f;
                xv.z *= 32768.0f;
                xv.w *= 32768.0f;
                const int row = idx / kVecPerRow, c = idx - row * kVecPerRow;
                *reinterpret_cast<float4*>(&tile[row * kSumPitch + 4 * c]) = xv;
            }
        }
    }
    __syncthreads();
    // 2. raw_frame.iter().sum() (pipeline.rs:115): one lane per frame, 400 adds in index order
    float sum = 0.0f;
#pragma unroll
    for (int seg = 0; seg < 3; ++seg) {
        const float* rowp = &tile[(lane + seg) * kSumPitch];
        const int nvec = seg < 2 ? kVecPerRow : (fe::kFrame - 2 * fe::kHop) / 4;
#pragma unroll 10
        for (int k = 0; k < nvec; ++k) {
            const float4 r = *reinterpret_cast<const float4*>(rowp + 4 * k);
            sum = sum + r.x;
            sum = sum + r.y;
            sum = sum + r.z;
            sum = sum + r.w;
        }
    }
    const int64_t f = f0 + lane;
    if (f < num_frames) mean_out[(int64_t)blockIdx.y * num_frames + f] = sum / (float)fe::kFrame;  // pipeline.rs:116
}

// ------------------------------------------------------------------------------------------------------
// Kernel 2: FFT + mel + log + LFR.  grid (ceil(F/64), batch), block 256 = 4 independent waves of 16 frames.
// ------------------------------------------------------------------------------------------------------
constexpr int kFrameXchgFloats = 2 * 16 * fe::kXchgPitch;  // 544 floats = 2176 B: odd frames start 32 banks later
constexpr int kWaveLdsFloats = 4 * kFrameXchgFloats;  // 8704 B per wave
constexpr int kPStride = 272;          // power row stride (words); 4*272 <= kWaveLdsFloats.  = 16 mod 32: the two frames of a half-wave write disjoint banks
                                       // and the lane-per-filter reads collide least (model of the 80-filter bank over all pitches: 186 cycles a pass, 258: 236)

struct TwLds {  // twiddle accessor over the LDS copy (phase B: per-lane indices)
    const float2* t;
    __device__ __forceinline__ float2 at(int i) const { return t[i]; }
};

// One direct-to-LDS load of 16 bytes per lane (global_load_lds_dwordx4): LDS address = lds_dst (wave-uniform) + 16 * lane.  The
// compiler's builtin, not inline assembly: a volatile asm statement counts as a write to all memory, after which the pass loop's
// scalar table loads become vector loads (190 registers, two waves a SIMD); the builtin's own cost of that kind is what
// fe_const_table below takes back.  The compiler also counts it: the block's __syncthreads() waits for it by itself.
__device__ __forceinline__ void fe_dma16(const void* gsrc, __attribute__((address_space(3))) char* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, lds_dst, 16, 0, 0);
}

// A table that no kernel writes, seen through the constant address space.  The pass loop reads its wave-uniform twiddles with scalar
// loads; the compiler grants those to a plain global pointer only while nothing before the load may have written memory, and it
// counts a direct-to-LDS load as such a write.  A constant-space pointer needs no such proof.
__device__ __forceinline__ const float* fe_const_table(const float* t, int pass) {
    auto c = (const __attribute__((address_space(4))) float*)t;
    asm("" : "+s"(c) : "s"(pass));  // opaque, or the two casts fold away; tied to the pass, or the loads leave the loop and their 58 SGPRs spill
    return (const float*)c;
}

template <int MODE>
__device__ __forceinline__ float lane_rot_prev(float v, int p) {
    // value of lane (p-1) mod 16 inside this 16-lane row
    if (MODE == 1) {
        // DPP row_ror:1 -- data moves to the next higher lane, lane 0 receives lane 15
        return __builtin_bit_cast(float,
                                  __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, true));
    } else {
        return __shfl(v, (p + 15) & 15, 16);
    }
}

// STDMEL: the mel bank has the round structure of the default config (80 mels @16 kHz/512: 5 rounds of
// 3,4,6,10,17 steps, no filter reaching past bin 256) -- verified on the host -- so the lane-per-filter dot
// products are fully unrolled with immediate LDS offsets; otherwise the table-driven loop is used.
constexpr int kStdMelLen[5] = {3, 4, 6, 10, 17};
constexpr int kStdMelOff[6] = {0, 3, 7, 13, 23, 40};

// FUSED: the block first stages its run of PCM (64 frames = 10 480 samples, read from HBM once) into an LDS tile that
// aliases the exchange region, wave 0 computes the 64 exact sequential frame sums from it (as fe_frame_sum_kernel
// does), and the per-pass sample loads below then hit L2 -- no separate sum kernel, no second HBM read of the PCM.
// One form: four passes a workgroup (64 frames, a wave takes 4 frames a pass) at three waves per SIMD; four waves with three passes were
// measured twice and lost (docs/experiments.md).
// OPT (the default bank's fused kernels only; 0 elsewhere): bit 0 (kFeConstTw) -- phase A's 27 wave-uniform twiddles are literals
// (fe::TwConst) instead of scalar loads from the table; bit 1 (kFeLdsMel) -- the 640 mel weights are read from an LDS copy, ten
// ds_read_b128 a pass, instead of 40 global loads a pass.  OPT = 0 is the table-reading form; the host selects (frontend_create).
// bit 2 (kFeLeanLds, with the other two only) -- the 64 eight-byte accesses of a pass's exchange are single ds_write_b64 /
// ds_read_b64 instead of pairs (ds_read2_b64 moves two slots at half the LDS rate: 64 LDS-array cycles a pass and wave less, measured;
// ds_write2_b64's five-dword transfer costs the store path more than two ds_write_b64 do: the LDS waits fell by a sixth), and the next
// pass's sample pointer is carried instead of rebuilt from the frame index.  The
// phase-B twiddle reads stay paired: read singly, their (-wi, wi) operand is no longer an operand modifier of the packed multiply
// but two more instructions a twiddle, which costs more than the LDS cycles give (docs/experiments.md).
// bit 3 (kFeConjA, with the other three only) -- phase A keeps structurally real values as scalars and half of the complex ones as
// conjugates (fe::phase_a_conj: no sign flips, real butterflies where both inputs are real), and s_tw is filled from the table image
// whose entries are conjugated for the lanes that then hold conjugates (tb.tw_conj); phase B's code and the power are unchanged.
using fe::FeForm;
using fe::kFeConstTw, fe::kFeLdsMel, fe::kFeLeanLds, fe::kFeConjA;
// One eight-byte LDS access that stays one ds_read_b64 / ds_write_b64: a volatile access is not merged with its neighbour.  The
// compiler still counts it (lgkmcnt) and still folds the constant part of the address into the instruction's offset.
typedef float fe_f2 __attribute__((ext_vector_type(2)));
typedef volatile __attribute__((address_space(3))) fe_f2* fe_lds_f2v;
__device__ __forceinline__ fe::cf fe_lds_read8(const float* p) {
    const fe_f2 t = *(fe_lds_f2v)p;
    return fe::cmk(t.x, t.y);
}
__device__ __forceinline__ void fe_lds_write8(float* p, fe::cf v) { *(fe_lds_f2v)p = (fe_f2){v.x, v.y}; }
constexpr int kMelLdsFloats = 768;  // 640 weights at fe::mel_lds_index (fe_core.h), padded to three 1 KiB loads
static_assert(fe::mel_lds_index(fe::kMelLdsWeights - 1, 15) < kMelLdsFloats && kStdMelOff[5] == fe::kMelLdsWeights, "the image holds the default bank");

template <int MODE, bool STDMEL, bool FUSED, int OPT, class Blk>
__device__ __forceinline__ void fe_main_body(const float* __restrict__ pcm, int64_t utt_stride,
                                             int64_t num_frames, int64_t t_lfr,
                                             const float* __restrict__ means, const FeDev& tb,
                                             float* __restrict__ out, float* __restrict__ logmel_out,
                                             int aligned16, float* s_melw, Blk bl) {
    constexpr int PASSES = 4;
    constexpr int FR = 16 * PASSES;           // frames per workgroup
    constexpr int kRows = FR + 2;             // hop rows of the run (400 = 2.5 hops)
    constexpr int kXFloats = FUSED ? (kRows * kSumPitch > 4 * kWaveLdsFloats ? kRows * kSumPitch : 4 * kWaveLdsFloats)
                                   : 4 * kWaveLdsFloats;
    __shared__ float2 s_tw[512];
    __shared__ __attribute__((aligned(16))) float s_x[kXFloats];
    __shared__ float s_mean[64];
    __shared__ int s_mstart[16 * (STDMEL ? 5 : kMaxMelRounds)];
    __shared__ int s_moff[kMaxMelRounds + 1];
    constexpr bool kConstTw = (OPT & kFeConstTw) != 0;
    constexpr bool kLdsMel = (OPT & kFeLdsMel) != 0;
    constexpr bool kLean = (OPT & kFeLeanLds) != 0;
    constexpr bool kConj = (OPT & kFeConjA) != 0;
    static_assert(!kLean || (kConstTw && kLdsMel), "the lean pass is a form of the constant-table kernel");
    static_assert(!kConj || kLean, "the conjugate phase A is a form of the lean pass");
    static_assert(OPT == 0 || (MODE == 1 && STDMEL && FUSED), "the constant / LDS table forms belong to the default bank's fused kernel");
    __shared__ __attribute__((aligned(16))) float s_melt[kLdsMel ? kMelLdsFloats : 4];
    // three workgroups a CU: 160 KiB / 3 = 54 613 bytes each (the table-driven mel loop's dynamic s_melw comes on top where OPT == 0)
    static_assert(sizeof(s_tw) + sizeof(s_x) + sizeof(s_mean) + sizeof(s_mstart) + sizeof(s_moff) + sizeof(s_melt) <= 54613, "LDS of three workgroups fits a CU");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, p = lane & 15;
    constexpr int kVecPerRow = fe::kHop / 4;
    constexpr int kVecs = kRows * kVecPerRow;
    constexpr int kIters = (kVecs + 255) / 256;
    constexpr bool kTwDma = FUSED;  // the whole 4 KiB twiddle table by four direct-to-LDS loads
    // FUSED: the block's run [64*blockIdx.x*hop, +66 hops) goes into the LDS tile as [hop row][offset] -- the layout and bank argument of
    // fe_frame_sum_kernel -- as RAW samples (the x32768 is in the sum chain below).  The tile is a copy, so where the run is 16-byte
    // aligned it is made by direct-to-LDS loads: no staging registers, no ds_write, half a dozen address instructions a KiB.  A wave
    // instruction fills 64 consecutive 16-byte slots of the tile; a row is 41 slots (40 of data + the pad slot), and lane l of
    // instruction u of wave w owns slot i = (4u + w)*64 + l = 256u + threadIdx.x.  Slot i sits in row i / 41, so its data are the 16
    // bytes at 16 * (i - i / 41) of the run (a pad slot fetches the first vector of the next row; nothing reads it).  42 instructions
    // cover slots 0 .. 2687; the last slot the sums read is 65*41 + 19 = 2684 (frame 63 ends half-way through row 65), so nothing
    // is written past the tile.  They are the first thing the kernel issues: no table load and no window coefficient stands between
    // the workgroup's start and its first HBM request.
    // Bounds: the source offset is clamped in 32-bit arithmetic RELATIVE TO THE RUN's first sample: `rem` = samples of the utterance from
    // there on (wave-uniform, at least one frame; capped far above the run's 10 560 so that it fits an int), and a slot that would end
    // past it fetches the utterance's last four samples instead.  No lane reads outside its utterance; slots that are clamped only
    // ever feed frames >= num_frames, whose sums are discarded.
    const bool tile_dma = FUSED && aligned16 && tb.tile_dma;  // wave-uniform (LELE_HIP_FE_TILE_DMA=0: register staging everywhere)
    float4 st[FUSED ? kIters : 1];
    if constexpr (FUSED) {
        const float* run = pcm + (int64_t)bl.y() * utt_stride + (int64_t)bl.x() * FR * fe::kHop;
        const int64_t rem64 = utt_stride - (int64_t)bl.x() * FR * fe::kHop;
        const int rem = (int)(rem64 < (1 << 20) ? rem64 : (1 << 20));
        if (tile_dma) {
            constexpr int kSlotsPerRow = kSumPitch / 4;
            constexpr int kDma = (FR - 1 + 2) * kSlotsPerRow + (fe::kFrame - 2 * fe::kHop) / 4;  // slots the sums read: 2685
            constexpr int kDmaInstr = (kDma + 63) / 64;
            static_assert(kDmaInstr * 64 * 4 <= kXFloats, "the tile DMA stays inside s_x");
            auto* tile_lds = (__attribute__((address_space(3))) char*)s_x;
            static_assert(kSlotsPerRow == 41 && kDmaInstr * 64 * 1599 < (1 << 24), "i / 41 == (i * 1599) >> 16 for every slot");
            const unsigned last = 4u * (unsigned)rem - 16u;  // rem is a multiple of 4 here (aligned16) and >= kFrame
            const int wave_s = __builtin_amdgcn_readfirstlane(wave);  // the LDS destination is a scalar operand
#pragma unroll
            for (int u = 0; 4 * u < kDmaInstr; ++u) {
                const unsigned i = 256u * u + threadIdx.x;
                const unsigned ob = 16u * (i - ((i * 1599u) >> 16));
                if (4 * u + 3 < kDmaInstr || 4 * u + wave_s < kDmaInstr)
                    fe_dma16(reinterpret_cast<const char*>(run) + (ob < last ? ob : last), tile_lds + (4 * u + wave_s) * 1024);
            }
        }
        if (kTwDma && wave == 3) {  // s_tw: 511 entries + the pad = 4 KiB (the device table is padded to 512 too)
            auto* tw_lds = (__attribute__((address_space(3))) char*)s_tw;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                fe_dma16(reinterpret_cast<const char*>(kConj ? tb.tw_conj : tb.tw) + 1024 * k + 16 * lane, tw_lds + 1024 * k);
        }
        if (kLdsMel && wave == 2) {  // s_melt: three 1 KiB loads of the host-built image, beside the twiddle table's
            auto* mel_lds = (__attribute__((address_space(3))) char*)s_melt;
#pragma unroll
            for (int k = 0; k < kMelLdsFloats / 256; ++k)
                fe_dma16(reinterpret_cast<const char*>(tb.melw_lds) + 1024 * k + 16 * lane, mel_lds + 1024 * k);
        }
        if (!tile_dma) {
            // register staging (unaligned runs -- most compute_segments blocks): 256 threads, all loads of a thread issued before the
            // first use
#pragma unroll
            for (int u = 0; u < kIters; ++u) {
                const int idx = u * 256 + (int)threadIdx.x;
                int o = 4 * idx;
                if (o + 3 >= rem) o = aligned16 ? ((rem - 4) & ~3) : (rem - 4);
                const float* src = run + o;
                if (aligned16)
                    st[u] = *reinterpret_cast<const float4*>(src);
                else
                    st[u] = make_float4(src[0], src[1], src[2], src[3]);
            }
        }
    }
    if (!kTwDma)
        for (int i = threadIdx.x; i < 511; i += 256) s_tw[i] = tb.tw[i];
    if (!STDMEL)
        for (int i = threadIdx.x; i < tb.mel_steps * 16; i += 256) s_melw[i] = tb.melw[i];
    if (threadIdx.x < tb.mel_rounds * 16) s_mstart[threadIdx.x] = tb.mel_start[threadIdx.x];
    if (threadIdx.x <= tb.mel_rounds) s_moff[threadIdx.x] = tb.mel_step_off[threadIdx.x];
    if (FUSED) {
        if (!tile_dma) {
#pragma unroll
            for (int u = 0; u < kIters; ++u) {
                const int idx = u * 256 + (int)threadIdx.x;
                if (idx < kVecs) {
                    const int row = idx / kVecPerRow, c = idx - row * kVecPerRow;
                    *reinterpret_cast<float4*>(&s_x[row * kSumPitch + 4 * c]) = st[u];
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's direct-to-LDS loads have landed; the barrier covers the others'
        __syncthreads();
    }
    // window coefficients and the first pass's samples are requested before the sums / barrier below, so that their
    // latency overlaps the 400-step add chain of wave 0
    const int h = fe::rev4(p);
    float* xw = s_x + wave * kWaveLdsFloats;           // this wave's exchange / power region
    float* xf = xw + g * kFrameXchgFloats;             // this frame's 2 KB round buffer
    const float* base = pcm + (int64_t)bl.y() * utt_stride;
    const float* mean_u = means + (int64_t)bl.y() * num_frames;
    const int d_out = tb.n_mels * tb.lfr_m;
    float* out_u = out ? out + (int64_t)bl.y() * t_lfr * d_out : nullptr;
    float* lm_u = logmel_out ? logmel_out + (int64_t)bl.y() * num_frames * tb.n_mels : nullptr;

    // Hann window coefficients of this lane's samples n = p + 16 q (features/window.rs), kept in registers
    float win[fe::kQ];
#pragma unroll
    for (int q = 0; q < fe::kQ; ++q) win[q] = tb.window[p + 16 * q];

    // raw PCM of the next pass is fetched while the current pass computes (software prefetch): the loads are
    // unconditional (clamped to frame 0 for the tail) so that all 25 are in flight together.
    float xr[fe::kQ];
    float mean_next = 0.0f;
    // kLean: the lane's frame advances by four a pass, so its first sample's address is carried (one 64-bit add) and the tail clamp is a
    // select between it and frame 0's; the frame index is compared in 32 bits, as everywhere below
    const float* src_carry = base + ((int64_t)bl.x() * FR + wave * (4 * PASSES) + g) * fe::kHop + p;
    auto issue_loads = [&](int pass) {
        const int64_t f = (int64_t)bl.x() * FR + wave * (4 * PASSES) + pass * 4 + g;
        const int64_t fc = f < num_frames ? f : 0;
        const float* src = base + fc * fe::kHop + p;
        if constexpr (kLean) {
            src = (int)(bl.x() * FR) + wave * (4 * PASSES) + g + pass * 4 < (int)num_frames ? src_carry : base + p;
            src_carry += 4 * fe::kHop;
        }
        if (!FUSED) mean_next = mean_u[fc];
#pragma unroll
        for (int q = 0; q < fe::kQ; ++q) xr[q] = src[16 * q];
    };
    issue_loads(0);
    if (FUSED) {
        // raw_frame.iter().sum() (pipeline.rs:115) over the scaled samples (pipeline.rs:90-112): one lane per frame, 400 steps in index
        // order.  The tile holds RAW samples: x * 32768 is exact (a power of two), so `sum + x * 32768` rounds once -- which is what one
        // fused multiply-add does: the same bits, and the scaling costs no instruction (the argument of the pass body's x * 32768 - mean;
        // like it, it breaks only where x * 2^15 overflows)
        // (wave 0 always: rotating the summing wave with the block index measured the same, docs/experiments.md)
        if (wave == 0 && lane < FR) {
            float sum = 0.0f;
#pragma unroll
            for (int seg = 0; seg < 3; ++seg) {
                const float* rowp = &s_x[(lane + seg) * kSumPitch];
                const int nvec = seg < 2 ? kVecPerRow : (fe::kFrame - 2 * fe::kHop) / 4;
#pragma unroll 10
                for (int k = 0; k < nvec; ++k) {
                    const float4 r = *reinterpret_cast<const float4*>(rowp + 4 * k);
                    sum = __builtin_fmaf(r.x, 32768.0f, sum);
                    sum = __builtin_fmaf(r.y, 32768.0f, sum);
                    sum = __builtin_fmaf(r.z, 32768.0f, sum);
                    sum = __builtin_fmaf(r.w, 32768.0f, sum);
                }
            }
            s_mean[lane] = sum / (float)fe::kFrame;  // pipeline.rs:116
        }
    }
    __syncthreads();  // tables (and, when FUSED, the means) are in LDS; the PCM tile may now be overwritten

    // STDMEL: the first bins of this lane's five filters are the same in every pass: read here, once
    int mstart[5] = {0, 0, 0, 0, 0};
    if (STDMEL) {
#pragma unroll
        for (int rd = 0; rd < 5; ++rd) mstart[rd] = s_mstart[rd * 16 + p];
    }

    // LFR targets of a frame f (lfr.rs:36-52): rows i, blocks b with n*i + b - pad == f; the first is b = (f + pad) % n in row
    // i = (f + pad) / n, the others follow at b + n in row i - 1, ...  A lane's frame advances by 4 a pass, so the division is done
    // here, once, and (b, i) are carried: b += 4, then the carry into i (next_targets below).  lfr_o is the first target's BYTE
    // offset inside the utterance's output, carried the same way, so that a store is the utterance's (wave-uniform) base plus a
    // 32-bit lane offset; the host refuses an utterance whose output does not fit 4 GiB.  Offsets are formed modulo 2^32 and used
    // only where (i, b) is a real target, where the true value fits.
    const int f_first = (int)(bl.x() * FR) + wave * (4 * PASSES) + g;
    const int nfr = (int)num_frames, tl = (int)t_lfr;
    const int pad = (tb.lfr_m - 1) / 2;
    const unsigned blk_bytes = 4u * (unsigned)tb.n_mels, row_bytes = 4u * (unsigned)d_out;
    auto target_off = [&](int i, int b) { return (unsigned)i * row_bytes + (unsigned)b * blk_bytes + 4u * (unsigned)p; };
    int lfr_b = (f_first + pad) % tb.lfr_n, lfr_i = (f_first + pad) / tb.lfr_n;
    unsigned lfr_o = target_off(lfr_i, lfr_b);
    auto next_targets = [&]() {
        lfr_b += 4;
        if (tb.lfr_n >= 4) {  // (wave-uniform) at most one row further: a compare and three selects
            const bool carry = lfr_b >= tb.lfr_n;
            lfr_b -= carry ? tb.lfr_n : 0;
            lfr_i += carry ? 1 : 0;
            lfr_o += carry ? 4u * blk_bytes + row_bytes - (unsigned)tb.lfr_n * blk_bytes : 4u * blk_bytes;
        } else {  // up to four rows further
            lfr_i += lfr_b / tb.lfr_n;
            lfr_b = lfr_b % tb.lfr_n;
            lfr_o = target_off(lfr_i, lfr_b);
        }
    };

    // One pass = 4 frames per wave.  The last pass is a second copy of the body WITHOUT the request for the next pass's samples: with
    // that request behind a branch the compiler sank half of the pre-emphasis below it -- the lane rotation and its multiply ended up
    // in different blocks (no DPP operand: 25 v_mov_dpp + 25 v_mov a pass) and the 25 samples were copied twice per pass.
    auto run_pass = [&](int pass, auto load_next_c) {
        constexpr bool load_next = decltype(load_next_c)::value;
        const int fi = f_first + pass * 4;
        const bool valid = fi < nfr;
        const float mean = FUSED ? s_mean[wave * (4 * PASSES) + pass * 4 + g] : mean_next;

        // 1./2. scale and mean subtraction (pipeline.rs:90-137): x * 32768 is exact (a power of two), so the product followed by the
        // subtraction rounds once -- which is what ONE fused multiply-add does: the same bits in half the instructions
        float v[fe::kQ];
        const float neg_mean = -mean;
#pragma unroll
        for (int q = 0; q < fe::kQ; ++q) v[q] = __builtin_fmaf(xr[q], 32768.0f, neg_mean);
        // next pass's samples: requested as early as the registers are free -- the workgroup's tile is still in its XCD's L2 then (requested
        // half a pass later, after phase A: the same time, 9 % more fabric traffic)
        if (load_next) issue_loads(pass + 1);
        // 3. pre-emphasis (pipeline.rs:140-142): y[n] = v[n] - 0.97*v[n-1] for n >= 1; v[n-1] lives in lane p-1
        //    (same q) or, for p == 0, in lane 15 at q-1.  4. window (pipeline.rs:145-166).
        float xin[fe::kRegs];
#pragma unroll
        for (int r = 0; r < fe::kRegs; ++r) xin[r] = 0.0f;
        //    The select happens BEFORE the rotation, on lane 15 (it sends v[q - 1], every other lane v[q]): the rotation then has one
        //    consumer and becomes that multiply's DPP operand (v_mul_f32_dpp; 0.97 in a register, a DPP instruction takes no literal)
        float k97;
        asm("v_mov_b32 %0, 0x3f7851ec" : "=v"(k97));  // 0.97f
#pragma unroll
        for (int q = 0; q < fe::kQ; ++q) {
            const float send = (p == 15 && q > 0) ? v[q > 0 ? q - 1 : 0] : v[q];
            const float prev = lane_rot_prev<MODE>(send, p);
            float y = fe::fsub(v[q], fe::fmul(k97, prev));
            if (q == 0) y = (p == 0) ? v[0] : y;  // sample 0 is not pre-emphasised
            xin[fe::rev5(q)] = fe::fmul(y, win[q]);
        }

        // 5. FFT stages 1..5 (wave-uniform twiddles straight from the table)
        fe::cf a[fe::kRegs];
        if constexpr (kConj)
            fe::phase_a_conj(xin, a, fe::TwConst{false}, fe::TwConst{true});
        else if constexpr (kConstTw)
            fe::phase_a_fast(xin, a, fe::TwConst{false}, fe::TwConst{true});
        else
            fe::phase_a_fast(xin, a, fe_const_table(tb.tw_re, pass), fe_const_table(tb.tw_im, pass));

        float pw[2][8];
        float p256 = 0.0f;
#pragma unroll
        for (int rho = 0; rho < 2; ++rho) {
            // exchange: register r = rho*16 + cc of lane h  ->  lane cc, register v = h
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) {
                const int slot = fe::xchg_slot(h, cc);
                if constexpr (kLean)
                    fe_lds_write8(xf + 2 * slot, a[rho * 16 + cc]);
                else
                    *reinterpret_cast<float2*>(xf + 2 * slot) = make_float2(a[rho * 16 + cc].x, a[rho * 16 + cc].y);
            }
            __builtin_amdgcn_wave_barrier();
            fe::cf bq[16];
#pragma unroll
            for (int vv = 0; vv < 16; ++vv) {
                if constexpr (kLean) {
                    bq[vv] = fe_lds_read8(xf + 2 * fe::xchg_slot(vv, p));
                } else {
                    const float2 t = *reinterpret_cast<const float2*>(xf + 2 * fe::xchg_slot(vv, p));
                    bq[vv] = fe::cmk(t.x, t.y);
                }
            }
            __builtin_amdgcn_wave_barrier();
            // stages 6..9 with per-lane twiddles from LDS
            float re256 = 0.0f;
            fe::phase_b(bq, p, rho, [&](int i) { const float2 w = s_tw[i]; return fe::cmk(w.x, w.y); }, &re256);
            if (rho == 0) p256 = re256;  // position 256 (used by lane p == 0)
            // 6. power spectrum (pipeline.rs:165-169); bins 0 and 256 have im forced to 0 (kernels/fft.rs:256-261)
#pragma unroll
            for (int vv = 0; vv < 8; ++vv) {
                fe::cf z = bq[vv];
                if (vv == 0 && rho == 0) z = fe::cmk(z.x, (p == 0) ? 0.0f : z.y);
                pw[rho][vv] = fe::power(z);
            }
        }
        // power -> LDS, row layout [frame g][bin]; aliases the exchange region (all exchange reads are done)
        float* prow = xw + g * kPStride;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rho = 0; rho < 2; ++rho)
#pragma unroll
            for (int vv = 0; vv < 8; ++vv) prow[(2 * vv + rho) * 16 + p] = pw[rho][vv];
        if (p == 0) prow[256] = fe::power(p256, 0.0f);
        __builtin_amdgcn_wave_barrier();

        // 7. sparse mel: lane pm = p owns filters m = 16*rd + p; sequential sum += w*P (mel.rs:92-104)
        // 8. ln(max(x, 1e-5)) (mel.rs:124-128) and LFR scatter (lfr.rs:18-54)
        float vals[STDMEL ? 5 : kMaxMelRounds];
        // kLdsMel: the lane's 40 weights come from the LDS image, ten 16-byte reads (fe::mel_lds_index: the 16 lanes of a frame read 16
        // consecutive slots, every bank once; the four frames of the wave read the same addresses), each the lane's base plus an immediate
        float wl[kLdsMel ? fe::kMelLdsWeights : 1];
        if constexpr (kLdsMel) {
#pragma unroll
            for (int j = 0; j < fe::kMelLdsChunks; ++j) {
                const float4 c = *reinterpret_cast<const float4*>(s_melt + fe::mel_lds_index(4 * j, p));
                wl[4 * j] = c.x, wl[4 * j + 1] = c.y, wl[4 * j + 2] = c.z, wl[4 * j + 3] = c.w;
            }
        }
#pragma unroll
        for (int rd = 0; rd < (STDMEL ? 5 : kMaxMelRounds); ++rd) {
            vals[rd] = 0.0f;
            if (!STDMEL && rd >= tb.mel_rounds) continue;
            const int m = rd * 16 + p;
            const int start = STDMEL ? mstart[rd < 5 ? rd : 0] : s_mstart[m];
            const float* pp = prow + start;
            float acc = 0.0f;
            if (STDMEL) {
                const float* wp = tb.melw + kStdMelOff[rd < 5 ? rd : 0] * 16 + p;  // L1-resident table, coalesced
                // every weight and every power of the round is requested before the (sequential) sum starts
                float w[17], pv[17];
#pragma unroll
                for (int t = 0; t < 17; ++t)
                    if (t < kStdMelLen[rd < 5 ? rd : 0]) w[t] = kLdsMel ? wl[kLdsMel ? kStdMelOff[rd < 5 ? rd : 0] + t : 0] : wp[t * 16];
#pragma unroll
                for (int t = 0; t < 17; ++t)
                    if (t < kStdMelLen[rd < 5 ? rd : 0]) pv[t] = pp[t];
#pragma unroll
                for (int t = 0; t < 17; ++t)
                    if (t < kStdMelLen[rd < 5 ? rd : 0]) {
                        // step 0: 0 + w*P is w*P itself -- a weight is +0 or positive and a power is a sum of squares, so the
                        // product is never the -0 that the addition would turn into +0
                        const float wp0 = fe::fmul(w[t], pv[t]);
                        acc = t == 0 ? wp0 : fe::fadd(acc, wp0);
                    }
            } else {
                const int t0 = s_moff[rd], t1 = s_moff[rd + 1];
                const float* wp = s_melw + t0 * 16 + p;
                const int lim = 256 - start;
#pragma unroll 4
                for (int t = 0; t < t1 - t0; ++t) {
                    const float pv = pp[t < lim ? t : lim];
                    acc = fe::fadd(acc, fe::fmul(wp[t * 16], pv));
                }
            }
            // ln(x) = log2(x) * ln2 with ln2 as hi + lo (what __logf expands to: v_log_f32, then the product in extended precision), without
            // __logf's rescaling of denormal inputs and its infinity test (compare, two selects, ldexp, a subtraction of 0, compare,
            // select): the input is in [1e-5, f32 max) here, so the bits are the same in 5 instructions instead of 12 (a mel sum that
            // overflowed to +inf -- samples beyond 1e9 -- gives NaN here and +inf there)
            {
                const float l2 = __builtin_amdgcn_logf(fmaxf(acc, 1e-5f));
                const float hi = __builtin_bit_cast(float, 0x3f317217u), lo = __builtin_bit_cast(float, 0x3377d1cfu);
                const float r = fe::fmul(l2, hi);
                vals[rd] = fe::fadd(r, fe::ffma(l2, lo, fe::ffma(l2, hi, -r)));
            }
        }
        // store: log-mel row (test hook) and/or the LFR scatter; lane p writes mels p, p+16, ... of each target (the targets of this
        // pass's frame: lfr_b, lfr_i, lfr_o above); the clamped first/last frames are handled in the rare branches below
        if (valid) {
            constexpr int kR = STDMEL ? 5 : kMaxMelRounds;
            auto put = [&](float* dst_u, unsigned off) {  // dst_u: wave-uniform; off: bytes, this lane's mel 0 .. 15 of the target
                float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(dst_u) + off);
#pragma unroll
                for (int rd = 0; rd < kR; ++rd)
                    if (STDMEL || rd * 16 + p < tb.n_mels)  // (STDMEL: 80 mels = five full rounds, no lane to mask)
                        __builtin_nontemporal_store(vals[rd], &dst[rd * 16]);  // streamed: keep L2 for the PCM
            };
            if (lm_u) put(lm_u, (unsigned)fi * blk_bytes + 4u * (unsigned)p);
            if (out_u) {
                int i = lfr_i;
                unsigned o = lfr_o;
                for (int b = lfr_b; b < tb.lfr_m && i >= 0; b += tb.lfr_n, --i, o += (unsigned)tb.lfr_n * blk_bytes - row_bytes)
                    if (i < tl) put(out_u, o);
                if (fi == 0) {  // left clamp: raw index < 0 reads frame 0
                    for (int i2 = 0; i2 * tb.lfr_n - pad < 0 && i2 < tl; ++i2)
                        for (int b = 0; b < tb.lfr_m && i2 * tb.lfr_n + b - pad < 0; ++b) put(out_u, target_off(i2, b));
                }
                if (fi == nfr - 1) {  // right clamp: raw index > T-1 reads the last frame
                    for (int i2 = tl - 1; i2 >= 0 && i2 * tb.lfr_n + (tb.lfr_m - 1) - pad > fi; --i2)
                        for (int b = tb.lfr_m - 1; b >= 0 && i2 * tb.lfr_n + b - pad > fi; --b) put(out_u, target_off(i2, b));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
#pragma unroll 1
    for (int pass = 0; pass + 1 < PASSES; ++pass) {
        run_pass(pass, std::true_type{});
        next_targets();
    }
    run_pass(PASSES - 1, std::false_type{});
}

template <int MODE, bool STDMEL, bool FUSED, int OPT = 0>
__global__ __launch_bounds__(256) void fe_main_kernel(const float* __restrict__ pcm, int64_t utt_stride, int64_t num_frames, int64_t t_lfr,
                                                      const float* __restrict__ means, FeDev tb, float* __restrict__ out,
                                                      float* __restrict__ logmel_out, int aligned16) {
    extern __shared__ float s_melw[];  // [mel_steps][16] (the table-driven mel loop only)
    fe_main_body<MODE, STDMEL, FUSED, OPT>(pcm, utt_stride, num_frames, t_lfr, means, tb, out, logmel_out, aligned16, s_melw, GridBlock{});
}

// ------------------------------------------------------------------------------------------------------
// compute_segments: fe_main_body over a 1-D grid of every segment's 64-frame blocks (a segment's last block is partial, so no block
// spans two segments).  Always the fused form (the frame sums inside the block): the two-kernel form is a lab switch of compute().  A block finds its segment through a per-block index (blk_seg[block] = segment) rather than a binary
// search over the segments' first blocks: the search would be log2(count) DEPENDENT loads at the head of every block (11 for 2048
// segments, each an L2 round trip before the first PCM request can go out), the index is one, plus the segment's record, for 4 bytes a
// block of table.  Everything after the lookup is fe_main_body on that segment alone, with the segment's own length
// for the float4 / scalar clamp and its own alignment, so each segment's rows are those compute() gives for it, bit for bit.
// ------------------------------------------------------------------------------------------------------
template <int MODE, bool STDMEL, int OPT = 0>
__global__ __launch_bounds__(256) void fe_seg_main_kernel(const float* __restrict__ pcm, const FeSeg* __restrict__ segs,
                                                          const int* __restrict__ blk_seg, FeDev tb, float* __restrict__ out) {
    extern __shared__ float s_melw[];
    const FeSeg s = segs[blk_seg[blockIdx.x]];
    const float* base = pcm + s.start;
    const int aligned16 = (((uintptr_t)base & 15) == 0) && (s.len % 4 == 0);  // per block: the segment's own alignment and length
    fe_main_body<MODE, STDMEL, true, OPT>(base, s.len, s.num_frames, s.t_lfr, nullptr, tb, out + s.row0 * (tb.n_mels * tb.lfr_m), nullptr,
                                          aligned16, s_melw, SegBlock{(unsigned)(blockIdx.x - s.block0)});
}
// ------------------------------------------------------------------------------------------------------
// Generic path: any FeatureConfig the reference accepts (other sample rates / frame lengths / n_fft = 1024).
// The same operations in the same order as pipeline.rs:84-187, spread over four simple kernels + the generic
// radix-2 FFT of features_ops.hip; nothing is fused, it only has to be bit-exact.
// ------------------------------------------------------------------------------------------------------
// (rows = utterances x frames: row r is frame r % num_frames of utterance r / num_frames, utterances pcm_len samples apart)
__global__ void fe_generic_mean_kernel(const float* __restrict__ pcm, int64_t rows, int64_t num_frames, int64_t pcm_len, int frame_len, int hop,
                                       float* __restrict__ mean) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= rows) return;
    const float* src = pcm + (f / num_frames) * pcm_len + (f % num_frames) * hop;
    float sum = 0.0f;
    int j = 0;
    if ((((uintptr_t)src) & 15) == 0) {   // sixteen samples requested (as four 16-byte loads) before their additions, which stay sequential
        for (; j + 16 <= frame_len; j += 16) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(src + j + 4 * u);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sum = sum + v[u].x * 32768.0f;
                sum = sum + v[u].y * 32768.0f;
                sum = sum + v[u].z * 32768.0f;
                sum = sum + v[u].w * 32768.0f;
            }
        }
    }
    for (; j < frame_len; ++j) sum = sum + src[j] * 32768.0f;  // raw_frame.iter().sum(), pipeline.rs:115
    mean[f] = sum / (float)frame_len;
}
__global__ void fe_generic_frame_kernel(const float* __restrict__ pcm, const float* __restrict__ mean,
                                        const float* __restrict__ window, int64_t rows, int64_t num_frames, int64_t pcm_len, int frame_len, int hop,
                                        int n_fft, float* __restrict__ frames) {
    const int64_t total = rows * n_fft;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / n_fft;
        const int j = (int)(i - f * n_fft);
        float v = 0.0f;
        if (j < frame_len) {
            const float* src = pcm + (f / num_frames) * pcm_len + (f % num_frames) * hop;
            const float m = mean[f];
            const float cur = fe::fsub(fe::fmul(src[j], 32768.0f), m);
            float y = cur;
            if (j >= 1) y = fe::fsub(cur, fe::fmul(0.97f, fe::fsub(fe::fmul(src[j - 1], 32768.0f), m)));  // pipeline.rs:140-142
            v = fe::fmul(y, window[j]);
        }
        frames[i] = v;
    }
}
__global__ void fe_generic_mel_kernel(const float* __restrict__ power, int64_t num_frames, int n_bins, int n_mels,
                                      const int* __restrict__ mstart, const int* __restrict__ moff,
                                      const float* __restrict__ mw, float* __restrict__ logmel) {
    const int64_t total = num_frames * n_mels;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / n_mels;
        const int m = (int)(i - f * n_mels);
        const float* p = power + f * n_bins + mstart[m];
        float acc = 0.0f;
        for (int t = moff[m]; t < moff[m + 1]; ++t) acc = fe::fadd(acc, fe::fmul(mw[t], p[t - moff[m]]));  // mel.rs:92-104
        logmel[i] = __logf(fmaxf(acc, 1e-5f));                                                            // mel.rs:124-128
    }
}
// The composed path's first four kernels as ONE (every FeatureConfig other than 400 / 160 / 512 ran frame means |
// pre-emphasis + window | radix-2 FFT | sparse mel + log as four launches over [rows, n_fft] and [rows, bins] scratch tensors --
// 10-20 x the fused default).  A workgroup takes FPB consecutive frames of one utterance: their PCM span goes to LDS once, one lane a
// frame forms the frame sum in the reference's order (pipeline.rs:115: a sequential f32 sum), all threads write the windowed frames
// bit-reversed into LDS, run the butterfly network of fft.rs:172-266 stage by stage there (twiddles in LDS), form the power spectrum
// and the sparse mel sums (mel.rs:92-104) out of LDS and store ln(max(x, 1e-5)).  The SAME operations in the SAME order as the four
// kernels (the fe:: helpers of fe_core.h): bit-identical log-mel rows; nothing but the log-mel leaves the workgroup.
#define FE_PAD(i) ((i) + ((i) >> 5))
__global__ __launch_bounds__(256) void fe_generic_fused_kernel(const float* __restrict__ pcm, int64_t pcm_len, int64_t num_frames, int frame_len,
                                                               int hop, int n, int log2n, int fpb, const float* __restrict__ window,
                                                               const float* __restrict__ tw_re_g, const float* __restrict__ tw_im_g, int n_mels,
                                                               const int* __restrict__ mstart, const int* __restrict__ moff,
                                                               const float* __restrict__ mw, const float* __restrict__ means,
                                                               float* __restrict__ logmel) {
    extern __shared__ float gfl[];
    const int nb = n / 2 + 1, span = (fpb - 1) * hop + frame_len;
    // re / im [fpb][n], one pad word per 32 (FE_PAD): the register passes read 2^R points a thread at strides of 1, 8, 64, ...
    float* re = gfl;
    float* im = re + FE_PAD(fpb * n) + 1;
    float* pw = im + FE_PAD(fpb * n) + 1;  // [fpb][nb]
    float* sp = pw + fpb * nb;             // [span] samples, then [fpb] means
    float* smean = sp + span;
    const int tid = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * fpb;
    const int nfr = (int)(num_frames - f0 < fpb ? num_frames - f0 : fpb);
    const float* src = pcm + (int64_t)blockIdx.y * pcm_len + f0 * hop;
    const int have = (nfr - 1) * hop + frame_len;   // samples of the frames that exist (every frame lies inside the utterance)
    for (int i = tid; i < span; i += 256) sp[i] = i < have ? src[i] : 0.0f;
    __syncthreads();
    if (means) {   // the frame sums come from fe_generic_mean_kernel (one LANE a frame there: a sequential sum of frame_len samples by one
        // lane holds a whole workgroup here for 8 k cycles -- measured 1 ms of 6 at 32 kHz)
        if (tid < nfr) smean[tid] = means[(int64_t)blockIdx.y * num_frames + f0 + tid];
    } else if (tid < nfr) {   // pipeline.rs:115-116: raw_frame.iter().sum() / frame_len, samples scaled by 32768 first
        const float* fr = sp + tid * hop;
        float sum = 0.0f;
        int j = 0;
        for (; j + 16 <= frame_len; j += 16) {   // sixteen samples requested before the (dependent) additions: an LDS round trip per
            float v[16];                         // sample made this loop 38 us of a workgroup's 40
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = fr[j + u];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum = sum + v[u] * 32768.0f;
        }
        for (; j < frame_len; ++j) sum = sum + fr[j] * 32768.0f;
        smean[tid] = sum / (float)frame_len;
    }
    __syncthreads();
    for (int i = tid; i < fpb * n; i += 256) {   // fe_generic_frame_kernel's value, at its bit-reversed slot
        const int f = i >> log2n, j = i & (n - 1);
        float v = 0.0f;
        if (j < frame_len && f < nfr) {
            const float* fr = sp + f * hop;
            const float m = smean[f];
            const float cur = fe::fsub(fe::fmul(fr[j], 32768.0f), m);
            float y = cur;
            if (j >= 1) y = fe::fsub(cur, fe::fmul(0.97f, fe::fsub(fe::fmul(fr[j - 1], 32768.0f), m)));  // pipeline.rs:140-142
            v = fe::fmul(y, window[j]);
        }
        const int r = (int)(__brev((unsigned)j) >> (32 - log2n));
        re[FE_PAD(f * n + r)] = v;
        im[FE_PAD(f * n + r)] = 0.0f;
    }
    __syncthreads();
    // The butterfly network, up to THREE stages per trip through LDS: a thread takes the 2^R points that stages s0 .. s0 + R - 1 combine
    // among themselves (indices base + j h, h = 2^s0), runs those stages on them in registers -- every butterfly with the twiddle and
    // the form (scalar below half = 4, fma from there: fft.rs:172-266) it has in the stage-by-stage network, so the same bits -- and
    // writes them back: 4 barriers for 1024 points instead of 10, 0.4 x the LDS traffic.
    for (int s0 = 0; s0 < log2n;) {
        const int R = log2n - s0 >= 3 ? 3 : log2n - s0, h = 1 << s0, gsz = 1 << R, groups = n >> R;
        for (int idx = tid; idx < fpb * groups; idx += 256) {
            const int f = idx / groups, g = idx - f * groups;
            const int lo = g & (h - 1), base = f * n + ((g >> s0) << (s0 + R)) + lo;
            float xr[8], xi[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < gsz) xr[j] = re[FE_PAD(base + j * h)], xi[j] = im[FE_PAD(base + j * h)];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if (r >= R) break;
                const int half = h << r, off = half - 1;   // the stage's twiddles start at 1 + 2 + ... + half / 2
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j >= gsz || (j >> r) & 1) continue;
                    const int k = lo + (j & ((1 << r) - 1)) * h;
                    const float wr = tw_re_g[off + k], wi = tw_im_g[off + k];   // (L1-resident: a copy in LDS costs occupancy)
                    if (half >= 4)
                        fe::bfly_fma(wr, wi, xr[j], xi[j], xr[j + (1 << r)], xi[j + (1 << r)]);
                    else
                        fe::bfly_scalar(wr, wi, xr[j], xi[j], xr[j + (1 << r)], xi[j + (1 << r)]);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < gsz) re[FE_PAD(base + j * h)] = xr[j], im[FE_PAD(base + j * h)] = xi[j];
        }
        s0 += R;
        __syncthreads();
    }
    for (int i = tid; i < fpb * nb; i += 256) {   // fft_frames_kernel mode 1: bins 0 and n / 2 have im forced to 0 (fft.rs:256-261)
        const int f = i / nb, k = i - f * nb;
        const float r = re[FE_PAD(f * n + k)];
        const float q = (k == 0 || k == nb - 1) ? 0.0f : im[FE_PAD(f * n + k)];
        pw[i] = fe::power(r, q);
    }
    __syncthreads();
    for (int i = tid; i < nfr * n_mels; i += 256) {   // fe_generic_mel_kernel
        const int f = i / n_mels, m = i - f * n_mels;
        const float* pp = pw + f * nb + mstart[m];
        const float* wp = mw + moff[m];
        const int cnt = moff[m + 1] - moff[m];
        float acc = 0.0f;
        int t = 0;
        for (; t + 8 <= cnt; t += 8) {   // eight weights and eight powers requested before the (sequential) sum: a filter has up to ~60 taps,
            float w8[8], p8[8];          // and one memory round trip a tap was most of a workgroup's life (62 % of the wave cycles waiting)
#pragma unroll
            for (int u = 0; u < 8; ++u) w8[u] = wp[t + u], p8[u] = pp[t + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fe::fadd(acc, fe::fmul(w8[u], p8[u]));  // mel.rs:92-104
        }
        for (; t < cnt; ++t) acc = fe::fadd(acc, fe::fmul(wp[t], pp[t]));
        logmel[((int64_t)blockIdx.y * num_frames + f0 + f) * n_mels + m] = __logf(fmaxf(acc, 1e-5f));      // mel.rs:124-128
    }
}
__global__ void fe_generic_lfr_kernel(const float* __restrict__ x, int64_t t, int64_t d, int64_t m, int64_t n,
                                      int64_t t_lfr, float* __restrict__ out) {  // lfr.rs:18-54; grid.y = utterance
    const int64_t d_out = d * m, total = t_lfr * d_out, pad = (m - 1) / 2;
    x += (int64_t)blockIdx.y * t * d;
    out += (int64_t)blockIdx.y * total;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx / d_out, rem = idx - i * d_out, block = rem / d, k = rem - block * d;
        int64_t raw = i * n + block - pad;
        raw = raw < 0 ? 0 : (raw > t - 1 ? t - 1 : raw);
        out[idx] = x[raw * d + k];
    }
}

// ------------------------------------------------------------------------------------------------------
// stream_push: N live streams fed chunk by chunk (lele_hip.h).  Each stream owns a PCM region (its carried samples, then this tick's
// chunk) and a log-mel region (its carried rows, then this tick's new frames); the counters live on the host and one record per
// stream, rebuilt every push, tells the four kernels below what to do.  A push is append -> log-mel -> emit -> compact in stream
// order, each one launch over ALL streams; no kernel reads a state range that another workgroup of the SAME launch writes.
// ------------------------------------------------------------------------------------------------------
struct FeStreamRec {
    int64_t src;           // first sample of this tick's chunk in the pcm buffer
    int64_t mel_base;      // global index of the frame in row 0 of the log-mel region
    int64_t row_lo;        // index (inside the utterance) of the first LFR row this push emits
    int64_t last_frame;    // T - 1 after this push (the right clamp of a final push)
    int64_t out_row0;      // first row of the packed result
    int32_t chunk, carry;  // samples of the chunk / carried in front of it
    int32_t nf;            // frames this push completes: frame j of them starts at sample j * hop of the region
    int32_t block0;        // first 64-frame block of the log-mel grid
    int32_t mel_carry;     // rows carried in the log-mel region (the new frames go behind them)
    int32_t rows;          // LFR rows this push emits
    int32_t emit_block0;   // first block of the emit grid
    int32_t final;         // the right clamp applies
    int32_t pcm_keep, pcm_from;  // compact: samples [pcm_from, pcm_from + pcm_keep) of the region move to its front
    int32_t mel_keep, mel_from;  // compact: rows [mel_from, mel_from + mel_keep) of the log-mel region move to its front
};

typedef float fe_f4 __attribute__((ext_vector_type(4)));
constexpr int kAppendPiece = 256;  // floats a workgroup of 64 copies: 1 KB
constexpr int kEmitRows = 4;       // LFR rows a workgroup of 256 gathers: one wave a row
constexpr int kCompactRegs = 8;    // floats a thread of the compact kernel holds across its barrier

// 1. append: the chunk goes behind the carried samples.  grid = streams x pieces of the longest chunk; an exact copy.
__global__ __launch_bounds__(64) void fe_stream_append_kernel(const float* __restrict__ pcm, const FeStreamRec* __restrict__ recs, int pieces,
                                                              float* __restrict__ pcm_state, int64_t pcm_pitch) {
    const int s = blockIdx.x / pieces, piece = blockIdx.x - s * pieces;
    const FeStreamRec r = recs[s];
    const int o = piece * kAppendPiece;
    if (o >= r.chunk) return;
    const float* src = pcm + r.src + o;
    float* dst = pcm_state + (int64_t)s * pcm_pitch + r.carry + o;
    const int n = min(kAppendPiece, r.chunk - o);
    LELE_DEV_ASSERT(r.carry + o + n <= pcm_pitch);
    const int t = threadIdx.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && 4 * t + 4 <= n) {
        *reinterpret_cast<float4*>(dst + 4 * t) = *reinterpret_cast<const float4*>(src + 4 * t);
    } else if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        for (int j = 4 * t; j < n; ++j) dst[j] = src[j];  // the piece's last, partial vector
    } else {
#pragma unroll
        for (int u = 0; u < kAppendPiece / 64; ++u)
            if (t + 64 * u < n) dst[t + 64 * u] = src[t + 64 * u];
    }
}

// 2. log-mel: fe_main_body over every stream's new frames, as fe_seg_main_kernel runs it over segments -- the "utterance" is the
// stream's PCM region (carry + chunk samples, frame j at j * hop), the LFR output is off and the log-mel rows go behind the carried ones.
// (SegBlock's twin rather than SegBlock itself: the body's LDS arrays are statics of the fe_main_body instantiation, and sharing one
// instantiation with fe_seg_main_kernel reordered operands in THAT kernel's code; a block type of its own leaves it as it was.)
struct StreamBlock {
    unsigned bx;
    __device__ __forceinline__ unsigned x() const { return bx; }
    __device__ __forceinline__ unsigned y() const { return 0u; }
};
template <int MODE, bool STDMEL, int OPT = 0>
__global__ __launch_bounds__(256) void fe_stream_main_kernel(const float* __restrict__ pcm_state, int64_t pcm_pitch,
                                                             const FeStreamRec* __restrict__ recs, const int* __restrict__ blk_stream, FeDev tb,
                                                             float* __restrict__ mel_state, int64_t mel_pitch) {
    extern __shared__ float s_melw[];
    const int s = blk_stream[blockIdx.x];
    const FeStreamRec r = recs[s];
    const float* base = pcm_state + (int64_t)s * pcm_pitch;  // 16-byte aligned: the region's base is, and the pitch is a multiple of 4
    const int64_t len = (int64_t)r.carry + r.chunk;
    const int aligned16 = len % 4 == 0;
    fe_main_body<MODE, STDMEL, true, OPT>(base, len, r.nf, 0, nullptr, tb, nullptr,
                                          mel_state + (int64_t)s * mel_pitch + (int64_t)r.mel_carry * tb.n_mels, aligned16, s_melw,
                                          StreamBlock{(unsigned)(blockIdx.x - r.block0)});
}

// 3. emit: LFR row i of a stream is blocks b = 0 .. m-1 = frames i*n + b - pad; frame g sits in row g - mel_base of the stream's
// log-mel region.  The left clamp goes to the utterance's frame 0 (still carried while any row needs it), the right clamp to frame T-1
// exists only on a final push: every other row's right-most frame is in the region by the closed form that selected it.
template <bool VEC>
__global__ __launch_bounds__(256) void fe_stream_emit_kernel(const float* __restrict__ mel_state, int64_t mel_pitch,
                                                             const FeStreamRec* __restrict__ recs, const int* __restrict__ blk_stream, int n_mels,
                                                             int lfr_m, int lfr_n, float* __restrict__ out) {
    const int s = blk_stream[blockIdx.x];
    const FeStreamRec r = recs[s];
    const int lane = threadIdx.x & 63;
    const int k = (int)(blockIdx.x - r.emit_block0) * kEmitRows + (int)(threadIdx.x >> 6);  // row of this push, one wave each
    if (k >= r.rows) return;
    const int64_t i = r.row_lo + k;
    const int pad = (lfr_m - 1) / 2;
    const float* mel = mel_state + (int64_t)s * mel_pitch;
    const int d_out = n_mels * lfr_m;
    float* dst = out + (r.out_row0 + k) * d_out;
    constexpr int W = VEC ? 4 : 1;
    const int per = n_mels / W;  // VEC: n_mels % 4 == 0, so every block of every row starts 16-byte aligned on both sides
    for (int v = lane; v < per * lfr_m; v += 64) {
        const int b = v / per, c = v - b * per;
        int64_t g = i * lfr_n + b - pad;
        g = g < 0 ? 0 : g;
        if (r.final) g = g > r.last_frame ? r.last_frame : g;
        LELE_DEV_ASSERT(g >= r.mel_base && g - r.mel_base < r.mel_carry + r.nf);
        const float* src = mel + (g - r.mel_base) * n_mels + W * c;
        float* d = dst + b * n_mels + W * c;
        if (VEC)
            __builtin_nontemporal_store(*reinterpret_cast<const fe_f4*>(src), reinterpret_cast<fe_f4*>(d));
        else
            __builtin_nontemporal_store(*src, d);
    }
}

// 4. compact: what the next push needs moves to the front of both regions.  Source and destination overlap when little was added, so
// ONE workgroup a stream takes the whole move through registers: everything is read, one barrier, everything is written (a move past
// 256 * kCompactRegs floats -- an LFR window far beyond the default's 399 + 6 * 80 -- goes in rounds of that size: a round's
// destination ends below every later round's source, since the move is towards the front).
__device__ __forceinline__ void fe_stream_move(float* region, int from, int count) {
    if (from == 0) return;
    for (int r0 = 0; r0 < count; r0 += 256 * kCompactRegs) {
        float v[kCompactRegs];
#pragma unroll
        for (int u = 0; u < kCompactRegs; ++u) {
            const int j = r0 + u * 256 + (int)threadIdx.x;
            v[u] = j < count ? region[from + j] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kCompactRegs; ++u) {
            const int j = r0 + u * 256 + (int)threadIdx.x;
            if (j < count) region[j] = v[u];
        }
    }
}
__global__ __launch_bounds__(256) void fe_stream_compact_kernel(const FeStreamRec* __restrict__ recs, float* pcm_state, int64_t pcm_pitch,
                                                                float* mel_state, int64_t mel_pitch, int n_mels) {
    const FeStreamRec r = recs[blockIdx.x];  // (block-uniform: every thread takes the same barriers)
    LELE_DEV_ASSERT(r.pcm_from + r.pcm_keep <= pcm_pitch && (int64_t)(r.mel_from + r.mel_keep) * n_mels <= mel_pitch);
    fe_stream_move(pcm_state + (int64_t)blockIdx.x * pcm_pitch, r.pcm_from, r.pcm_keep);
    fe_stream_move(mel_state + (int64_t)blockIdx.x * mel_pitch, r.mel_from * n_mels, r.mel_keep * n_mels);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// Host side: mirrors SenseVoiceFrontend::new (pipeline.rs:38-65)
// ------------------------------------------------------------------------------------------------------
struct LeleFrontend {
    LeleCtx* ctx = nullptr;
    LeleFeatureConfig cfg{};
    int64_t frame_len = 0, hop_len = 0, n_fft = 0;
    bool fast = false;
    // the fused kernel this front-end runs (fe::select_form, once, in frontend_create).  mode: the DPP row_ror unless the lab's
    // LELE_HIP_FE_DPP says __shfl; fused: the lab's LELE_HIP_FE_FUSED=0 selects the two-kernel form of compute()
    FeForm form{1, false, true, 0};
    int last_launch = -1;  // the tuple fe_dispatch launched last (test hook lele_hip_frontend_last_launch)
    // generic path tables (configs other than 400/160/512)
    const float* g_window = nullptr;
    const int* g_mstart = nullptr;
    const int* g_moff = nullptr;
    const float* g_mw = nullptr;
    FeDev dev{};
    std::vector<void*> allocs;
    DevTables seg_tables;  // compute_segments: [FeSeg x segments][int blk_seg x blocks] per distinct layout
    // optional per-kernel stopwatch (bench.py roofline block): 3 events per run, read back lazily
    bool profiling = false;
    std::vector<hipEvent_t> events;  // triples (before sum, between, after main)
    size_t events_used = 0;
};

namespace {

static const float PI_F = 3.14159265358979323846264338327950288f;

void host_hann(int64_t size, std::vector<float>& w) {  // window.rs:2-13
    w.resize(size);
    if (size == 1) w[0] = 1.0f;
    for (int64_t n = 0; size > 1 && n < size; ++n) w[n] = 0.5f * (1.0f - cosf(2.0f * PI_F * (float)n / (float)(size - 1)));
}

void host_twiddles(int64_t n, std::vector<float>& re, std::vector<float>& im) {  // kernels/fft.rs:136-157
    re.clear();
    im.clear();
    for (int64_t size = 2; size <= n; size *= 2) {
        int64_t half = size / 2, step = n / size;
        for (int64_t k = 0; k < half; ++k) {
            float angle = -2.0f * PI_F * (float)(k * step) / (float)n;
            re.push_back(cosf(angle));
            im.push_back(sinf(angle));
        }
    }
}

float hz_to_mel(float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); }       // mel.rs:1-3
float mel_to_hz(float mel) { return 700.0f * (powf(10.0f, mel / 2595.0f) - 1.0f); }  // mel.rs:4-6

// mel_filterbank (mel.rs:7-56): the dense [n_mels][n_fft / 2 + 1] triangles, HTK mel scale
void host_dense_mel(float sr, int64_t n_fft, int64_t n_mels, float f_min, float f_max, float* bank) {
    const int64_t n_freqs = n_fft / 2 + 1;
    const float mel_min = hz_to_mel(f_min), mel_max = hz_to_mel(f_max);
    const float mel_step = (mel_max - mel_min) / (float)(n_mels + 1);
    std::vector<float> hz(n_mels + 2), ff(n_freqs);
    for (int64_t i = 0; i < n_mels + 2; ++i) hz[i] = mel_to_hz(mel_min + (float)i * mel_step);
    for (int64_t i = 0; i < n_freqs; ++i) ff[i] = (float)i * sr / (float)n_fft;
    for (int64_t i = 0; i < n_mels; ++i) {
        const float fl = hz[i], fc = hz[i + 1], fr = hz[i + 2];
        for (int64_t j = 0; j < n_freqs; ++j) {
            const float f = ff[j];
            float val = 0.0f;
            if (f > fl && f < fc)
                val = (f - fl) / (fc - fl);
            else if (f >= fc && f < fr)
                val = (fr - f) / (fr - fc);
            bank[i * n_freqs + j] = val;
        }
    }
}

// SparseMelBank::new (mel.rs:58-90) over it: per filter (start_bin, weights[])
void host_sparse_mel(float sr, int64_t n_fft, int64_t n_mels, float f_min, std::vector<int>& start,
                     std::vector<std::vector<float>>& w) {
    const int64_t n_freqs = n_fft / 2 + 1;
    std::vector<float> bank((size_t)n_mels * n_freqs);
    host_dense_mel(sr, n_fft, n_mels, f_min, sr / 2.0f, bank.data());
    start.assign(n_mels, 0);
    w.assign(n_mels, {});
    for (int64_t i = 0; i < n_mels; ++i) {
        const float* row = bank.data() + i * n_freqs;
        int64_t s = 0;
        while (s < n_freqs && row[s] == 0.0f) ++s;
        int64_t e = n_freqs;
        while (e > s && row[e - 1] == 0.0f) --e;
        if (s < e) {
            start[i] = (int)s;
            w[i].assign(row + s, row + e);
        }
    }
}

template <typename T>
int upload(LeleFrontend* fe, const std::vector<T>& v, const T** out) {
    void* d = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    LELE_HIP_CHECK(hipMalloc(&d, bytes));
    fe->allocs.push_back(d);
    if (!v.empty()) LELE_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)d;
    return 0;
}

// a product switch ("Run-time switches"): on unless set to something whose atoi is 0
bool fe_switch(const char* name) {
    const char* e = getenv(name);
    return !(e && *e && atoi(e) == 0);
}

// The tag fe_dispatch hands to its callable: the template arguments <MODE, STDMEL, FUSED, OPT> of fe_main_kernel, fe_seg_main_kernel and
// fe_stream_main_kernel as constants.
template <int MODE, bool STDMEL, bool FUSED, int OPT>
struct FeTag {
    static constexpr int mode = MODE, opt = OPT;
    static constexpr bool std_mel = STDMEL, fused = FUSED;
    static constexpr int id = MODE | STDMEL << 1 | FUSED << 2 | OPT << 3;  // what lele_hip_frontend_last_launch reports
};
// Calls launch(tag) with the tag of form f and records the tuple it launches from the tag's own constants.  The fused kernels that exist
// are listed here and nowhere else; mode == 0 and fused == false are lab values (lab_env), so their tuples are compiled into the lab
// library alone.  A form outside the list is an error (select_form yields none with the lab values at their defaults).
template <class F>
int fe_dispatch(LeleFrontend* fe, FeForm f, F&& launch) {
    const int id = f.mode | f.std_mel << 1 | f.fused << 2 | f.opt << 3;
    auto is = [&](auto t) {
        if (id != t.id) return false;
        fe->last_launch = t.id;
        launch(t);
        return true;
    };
    const bool found = is(FeTag<1, false, true, 0>{}) || is(FeTag<1, true, true, 0>{}) || is(FeTag<1, true, true, kFeConstTw>{}) ||
                       is(FeTag<1, true, true, kFeConstTw | kFeLdsMel>{}) || is(FeTag<1, true, true, kFeConstTw | kFeLdsMel | kFeLeanLds>{}) ||
                       is(FeTag<1, true, true, kFeConstTw | kFeLdsMel | kFeLeanLds | kFeConjA>{})
#ifdef LELE_HIP_LAB
                       || is(FeTag<0, false, true, 0>{}) || is(FeTag<0, true, true, 0>{}) || is(FeTag<1, false, false, 0>{}) ||
                       is(FeTag<1, true, false, 0>{}) || is(FeTag<0, false, false, 0>{}) || is(FeTag<0, true, false, 0>{})
#endif
        ;
    LELE_REQUIRE(found, "frontend: no kernel for the form mode %d std_mel %d fused %d opt %d", f.mode, (int)f.std_mel, (int)f.fused, f.opt);
    return 0;
}
// dynamic LDS of a fused kernel: the table-driven mel loop's weights (opt != 0: the kernel's own static tables instead)
size_t fe_mel_lds(const LeleFrontend* fe) { return fe->form.opt ? 0 : (size_t)fe->dev.mel_steps * 16 * sizeof(float); }
// lele_hip_last_route: how the fused kernel's blocks stage their PCM tile -- n_dma of the launch's n utterances / segments / streams meet
// fe_main_body's own condition (`tile_dma` there: a 16-byte aligned run and LELE_HIP_FE_TILE_DMA on)
const char* fe_tile_route(int64_t n_dma, int64_t n) { return n_dma == n ? "fe.tile_dma" : n_dma == 0 ? "fe.tile_regs" : "fe.tile_mixed"; }

}  // namespace

extern "C" {

/* The table builders of lele::features as the library computes them itself (window.rs:2-13, mel.rs:7-56): host arithmetic, host
 * pointers, no ctx.  A binding exposes `hann_window` / `mel_filterbank` through these instead of restating the formulas. */
int lele_hip_hann_window(int64_t size, float* out) {
    LELE_REQUIRE(size >= 0 && (out || size == 0), "hann_window: bad argument");
    std::vector<float> w;
    host_hann(size, w);
    if (size) memcpy(out, w.data(), (size_t)size * 4);
    return 0;
}
float lele_hip_hz_to_mel_htk(float hz) { return hz_to_mel(hz); }      /* mel.rs:1-3 */
float lele_hip_mel_to_hz_htk(float mel) { return mel_to_hz(mel); }    /* mel.rs:4-6 */
int lele_hip_mel_filterbank(float sample_rate, int64_t n_fft, int64_t n_mels, float f_min, int32_t has_f_max, float f_max, float* out) {
    LELE_REQUIRE(n_fft >= 0 && n_mels >= 0 && (out || n_mels == 0), "mel_filterbank: bad argument");
    if (n_mels) host_dense_mel(sample_rate, n_fft, n_mels, f_min, has_f_max ? f_max : sample_rate / 2.0f, out);
    return 0;
}


int lele_hip_frontend_create(LeleCtx* ctx, const LeleFeatureConfig* cfg, LeleFrontend** out) {
    LELE_REQUIRE(ctx && cfg && out, "frontend_create: NULL argument");
    LELE_REQUIRE(cfg->sample_rate > 0 && cfg->n_mels > 0 && cfg->lfr_m > 0 && cfg->lfr_n > 0,
                 "frontend_create: invalid FeatureConfig");
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LeleFrontend* fe = new LeleFrontend();
    fe->ctx = ctx;
    fe->cfg = *cfg;
    fe->frame_len = (int64_t)((float)cfg->sample_rate * cfg->frame_length_ms / 1000.0f);  // pipeline.rs:39
    fe->n_fft = fe->frame_len > 400 ? 1024 : 512;                                        // pipeline.rs:40
    fe->hop_len = (int64_t)((float)cfg->sample_rate * cfg->frame_shift_ms / 1000.0f);     // pipeline.rs:42
    fe->fast = (fe->frame_len == fe::kFrame && fe->hop_len == fe::kHop && fe->n_fft == fe::kNfft &&
                cfg->n_mels <= 16 * kMaxMelRounds);
    if (!fe->fast) {
        // generic path: window + flat sparse mel bank; the FFT tables live in the ctx (features_ops.hip)
        if (fe->frame_len < 1 || fe->hop_len < 1 || fe->frame_len > fe->n_fft) {
            const long long fl = (long long)fe->frame_len, hl = (long long)fe->hop_len, nf = (long long)fe->n_fft;
            delete fe;
            // upstream indexes frame_buf[..fft_len] with frame_len (pipeline.rs:145-166) and divides by hop_len (:73)
            set_error("frontend_create: frame_len=%lld hop_len=%lld do not fit fft_len=%lld (the reference panics here)", fl, hl, nf);
            return 3;
        }
        std::vector<float> gwin;
        host_hann(fe->frame_len, gwin);
        std::vector<int> gstart;
        std::vector<std::vector<float>> gw;
        host_sparse_mel((float)cfg->sample_rate, fe->n_fft, cfg->n_mels, 20.0f, gstart, gw);  // pipeline.rs:45-51
        std::vector<int> goff(cfg->n_mels + 1, 0);
        std::vector<float> gflat;
        for (int64_t m = 0; m < cfg->n_mels; ++m) {
            goff[m] = (int)gflat.size();
            gflat.insert(gflat.end(), gw[m].begin(), gw[m].end());
        }
        goff[cfg->n_mels] = (int)gflat.size();
        int rc = 0;
        rc |= upload(fe, gwin, &fe->g_window);
        rc |= upload(fe, gstart, &fe->g_mstart);
        rc |= upload(fe, goff, &fe->g_moff);
        rc |= upload(fe, gflat, &fe->g_mw);
        if (rc) {
            lele_hip_frontend_destroy(fe);
            return rc;
        }
        *out = fe;
        return 0;
    }
    std::vector<float> win, twr, twi;
    host_hann(fe->frame_len, win);
    host_twiddles(fe->n_fft, twr, twi);
    // phase_a_fast folds the k = 0 entries of stages 1, 2, 4 and 5 == (1, -0) away: make sure this libm agrees (it must: cos(-0)=1)
    for (int i : {0, 1, fe::tw_off(4), fe::tw_off(5)})
        LELE_REQUIRE(twr[i] == 1.0f && twi[i] == 0.0f, "frontend_create: unexpected twiddle table entry %d", i);
    std::vector<float2> tw(512, make_float2(0.f, 0.f));
    for (size_t i = 0; i < twr.size(); ++i) tw[i] = make_float2(twr[i], twi[i]);
    twr.resize(512, 0.0f);
    twi.resize(512, 0.0f);
    std::vector<int> mstart;
    std::vector<std::vector<float>> mw;
    host_sparse_mel((float)cfg->sample_rate, fe->n_fft, cfg->n_mels, 20.0f, mstart, mw);  // pipeline.rs:45-51
    FeDev& d = fe->dev;
    d.n_mels = (int)cfg->n_mels;
    d.lfr_m = (int)cfg->lfr_m;
    d.lfr_n = (int)cfg->lfr_n;
    d.mel_rounds = (int)((cfg->n_mels + 15) / 16);
    std::vector<int> start_pad(d.mel_rounds * 16, 0);
    std::vector<float> melw;
    std::vector<int> step_off(d.mel_rounds + 1, 0);
    int off = 0;
    for (int rd = 0; rd < d.mel_rounds; ++rd) {
        size_t maxlen = 0;
        for (int pm = 0; pm < 16; ++pm) {
            int m = rd * 16 + pm;
            if (m < cfg->n_mels) {
                start_pad[m] = mstart[m];
                maxlen = std::max(maxlen, mw[m].size());
            }
        }
        step_off[rd] = off;
        for (size_t t = 0; t < maxlen; ++t)
            for (int pm = 0; pm < 16; ++pm) {
                int m = rd * 16 + pm;
                melw.push_back((m < cfg->n_mels && t < mw[m].size()) ? mw[m][t] : 0.0f);
            }
        off += (int)maxlen;
    }
    step_off[d.mel_rounds] = off;
    d.mel_steps = off;
    bool std_mel = (d.mel_rounds == 5 && cfg->n_mels == 80);  // the bank has the default round structure (fully unrolled kernel variant)
    for (int rd = 0; std_mel && rd < 5; ++rd) {
        if (step_off[rd] != kStdMelOff[rd] || step_off[rd + 1] != kStdMelOff[rd + 1]) std_mel = false;
        for (int pm = 0; pm < 16; ++pm)
            if (start_pad[rd * 16 + pm] + kStdMelLen[rd] - 1 > 256) std_mel = false;
    }
    if (lab_env("LELE_HIP_FE_GENERIC_MEL")) std_mel = false;
    int rc = 0;
    rc |= upload(fe, twr, &d.tw_re);
    rc |= upload(fe, twi, &d.tw_im);
    rc |= upload(fe, tw, &d.tw);
    {   // the same table with the entries of primed lanes conjugated (fe_core.h), padded to 512 like tw
        std::vector<float2> twc(512, make_float2(0.f, 0.f));
        fe::tw_conj_image(twr.data(), twi.data(), 511, reinterpret_cast<float*>(twc.data()));
        rc |= upload(fe, twc, &d.tw_conj);
    }
    rc |= upload(fe, win, &d.window);
    rc |= upload(fe, melw, &d.melw);
    {   // the default bank's weights as the kernel's LDS image: weight s = step_off[rd] + t of lane pm at [s / 4][pm][s % 4]
        std::vector<float> img(kMelLdsFloats, 0.0f);
        for (int sidx = 0; std_mel && sidx < fe::kMelLdsWeights; ++sidx)
            for (int pm = 0; pm < 16; ++pm) img[fe::mel_lds_index(sidx, pm)] = melw[sidx * 16 + pm];
        rc |= upload(fe, img, &d.melw_lds);
    }
    rc |= upload(fe, start_pad, &d.mel_start);
    rc |= upload(fe, step_off, &d.mel_step_off);
    if (rc) {
        lele_hip_frontend_destroy(fe);
        return rc;
    }
    // product switch: 0 = aligned runs take the register staging of unaligned ones -- same bits, the A/B handle and
    // the on-device cross-check of the direct-to-LDS tile
    d.tile_dma = fe_switch("LELE_HIP_FE_TILE_DMA");
    // a table that differs from the compiled-in constants in any bit (another libm) keeps the kernels that read every twiddle from
    // it.  LELE_HIP_FE_CONST_TW=mismatch is the tests' way to get there: the switch counts as on, and the check alone -- on a table
    // with one entry moved by an ulp -- decides
    const char* envc = getenv("LELE_HIP_FE_CONST_TW");
    const bool mismatch = envc && !strcmp(envc, "mismatch");
    bool const_match = fe::tw_const_matches(twr.data(), twi.data());
    if (mismatch) {
        std::vector<float> other = twr;
        other[fe::tw_off(5) + 3] = nextafterf(other[fe::tw_off(5) + 3], 2.0f);
        const_match = fe::tw_const_matches(other.data(), twi.data());
    }
    // The four product switches give the same bits either way.  LELE_HIP_FE_CONST_TW=0: every twiddle is read from the table;
    // _LDS_TABLES=0: the mel weights stay in global memory; _LEAN_LDS=0: the pass loop keeps the exchange's paired LDS accesses and
    // rebuilds the sample address every pass; _CONJ_A=0: phase A keeps its sign flips and packed butterflies on real values
    // (fe::phase_a_fast).  The two lab values: 1 = DPP row_ror, 0 = __shfl (ds_bpermute); fused = 0: the two-kernel form.
    const char* envp = lab_env("LELE_HIP_FE_DPP");
    const char* envf = lab_env("LELE_HIP_FE_FUSED");
    fe->form = fe::select_form(std_mel, const_match, mismatch || fe_switch("LELE_HIP_FE_CONST_TW"), fe_switch("LELE_HIP_FE_LDS_TABLES"),
                               fe_switch("LELE_HIP_FE_LEAN_LDS"), fe_switch("LELE_HIP_FE_CONJ_A"), envp ? atoi(envp) : 1, envf ? atoi(envf) != 0 : true);
    *out = fe;
    return 0;
}

/* test hooks (not part of include/lele_hip.h), views of the form frontend_create selected.  kernel_form -- bit 0: phase A's twiddles are
 * compiled-in constants, bit 1: the mel weights are read from LDS; 0: the table-reading kernels.  lean_lds / conj_a -- 1 where the
 * default bank's fused kernels run the lean pass (kFeLeanLds) / phase A on real and conjugate values (kFeConjA). */
int lele_hip_frontend_kernel_form(const LeleFrontend* fe) { return fe ? fe->form.opt & (kFeConstTw | kFeLdsMel) : -1; }
int lele_hip_frontend_lean_lds(const LeleFrontend* fe) { return fe ? (fe->form.opt & kFeLeanLds) != 0 : -1; }
int lele_hip_frontend_conj_a(const LeleFrontend* fe) { return fe ? (fe->form.opt & kFeConjA) != 0 : -1; }
/* test hook: the tuple the last fused launch of this front-end ran, mode | std_mel << 1 | fused << 2 | opt << 3 as fe_dispatch
 * recorded it; -1 before any */
int lele_hip_frontend_last_launch(const LeleFrontend* fe) { return fe ? fe->last_launch : -1; }

int lele_hip_frontend_destroy(LeleFrontend* fe) {
    if (!fe) return 0;
    (void)hipStreamSynchronize(fe->ctx->stream);
    for (void* p : fe->allocs) (void)hipFree(p);
    fe->seg_tables.release();
    for (hipEvent_t e : fe->events) (void)hipEventDestroy(e);
    delete fe;
    return 0;
}

int lele_hip_frontend_out_rows(const LeleFrontend* fe, int64_t pcm_len, int64_t* rows, int64_t* cols,
                               int64_t* num_frames) {
    LELE_REQUIRE(fe, "frontend_out_rows: fe is NULL");
    int64_t nf = 0, t = 0;
    if (pcm_len >= fe->frame_len) {  // pipeline.rs:70-73
        nf = (pcm_len - fe->frame_len) / fe->hop_len + 1;
        t = (nf + fe->cfg.lfr_n - 1) / fe->cfg.lfr_n;  // lfr.rs:33
    }
    if (rows) *rows = t;
    if (cols) *cols = fe->cfg.n_mels * fe->cfg.lfr_m;
    if (num_frames) *num_frames = nf;
    return 0;
}

static int ilog2_i(int n) {
    int l = 0;
    while ((1 << (l + 1)) <= n) ++l;
    return l;
}
// generic path (FeatureConfigs other than 400 / 160 / 512): `batch` utterances pcm_len samples apart at dpcm -> outp ([batch, t_lfr,
// cols] or, want_logmel, [batch, nf, n_mels]); dmean: batch * nf floats of scratch
static int fe_generic(LeleFrontend* fe, const float* dpcm, int64_t batch, int64_t pcm_len, int64_t nf, int64_t t_lfr, int64_t cols,
                      float* outp, bool want_logmel, void* dmean) {
    LeleCtx* ctx = fe->ctx;
    // generic path: as many utterances per pass as fit 256 MiB of scratch (means, frames [rows, n_fft], power [rows, bins], logmel
    // [rows, mels]; rows = utterances x frames) -- five launches a pass (looping over utterances on the host made the launches
    // the cost: 256 x 30 s at 16 kHz / 20 ms frames 16.1 ms)
    const int64_t bins = fe->n_fft / 2 + 1, nm = fe->cfg.n_mels;
    // the fused form (fe_generic_fused_kernel): frames per workgroup so that their LDS image stays under 64 KB; anything larger
    // (n_fft > 4096) keeps the four kernels
    if (fe->form.fused && fe->n_fft <= 4096 && fe->frame_len <= fe->n_fft && batch <= 65535) {   // (lab: LELE_HIP_FE_FUSED=0 keeps the four kernels)
        const int n = (int)fe->n_fft;
        // (the kernel is bound by latency under its barriers, so by occupancy against work per workgroup: 4 frames of 1024 points with
        // the twiddles in LDS = 55 KB = two workgroups a CU ran 15 ms where the four kernels took 12)
        int fpb = n <= 512 ? 4 : n <= 1024 ? 2 : 1;   // measured (tools/fe_fpb.sh): n = 512: 3.9 / 2.6 / 2.4 / 3.1 ms for 1 / 2 / 4 / 8; n = 1024: 6.1 / 5.2 / 7.1 / 17.2
        if (const char* e = lab_env("LELE_HIP_FE_FPB")) fpb = std::max(1, atoi(e));   // (lab) frames per workgroup
        const size_t padded = (size_t)fpb * n + (((size_t)fpb * n) >> 5) + 1;
        const size_t lds = (2 * padded + (size_t)fpb * bins + (size_t)(fpb - 1) * fe->hop_len + fe->frame_len + fpb) * 4;
        if (lds <= 96 * 1024) {
            ctx->set_route("fe.generic_fused");
            const float *twr = nullptr, *twi = nullptr;
            LELE_TRY(fft_twiddles(ctx, n, &twr, &twi));
            LELE_HIP_CHECK(ensure_dyn_lds(reinterpret_cast<const void*>(fe_generic_fused_kernel), (int)lds));
            const int64_t per_utt_lm = nf * nm * 4;
            const int64_t ubf = want_logmel ? batch : std::max<int64_t>(1, std::min<int64_t>(batch, (int64_t(1) << 28) / std::max<int64_t>(per_utt_lm, 1)));
            void* glm = nullptr;
            if (!want_logmel) LELE_TRY(ctx->arena_alloc((size_t)ubf * nf * nm * 4, &glm));
            for (int64_t u = 0; u < batch; u += ubf) {
                const int64_t nu = std::min<int64_t>(ubf, batch - u);
                const float* up = (const float*)dpcm + u * pcm_len;
                float* lm = want_logmel ? outp + u * nf * nm : (float*)glm;
                hipLaunchKernelGGL(fe_generic_mean_kernel, dim3((unsigned)((nu * nf + 63) / 64)), dim3(64), 0, ctx->stream, up, nu * nf, nf, pcm_len,
                                   (int)fe->frame_len, (int)fe->hop_len, (float*)dmean);
                hipLaunchKernelGGL(fe_generic_fused_kernel, dim3((unsigned)((nf + fpb - 1) / fpb), (unsigned)nu), dim3(256), lds, ctx->stream, up,
                                   pcm_len, nf, (int)fe->frame_len, (int)fe->hop_len, n, ilog2_i(n), fpb, fe->g_window, twr, twi, (int)nm,
                                   fe->g_mstart, fe->g_moff, fe->g_mw, (const float*)dmean, lm);
                if (!want_logmel) {
                    dim3 lg((unsigned)std::max<int64_t>(1, std::min<int64_t>((t_lfr * cols + 255) / 256, 8192)), (unsigned)nu);
                    hipLaunchKernelGGL(fe_generic_lfr_kernel, lg, dim3(256), 0, ctx->stream, (const float*)lm, nf, nm, fe->cfg.lfr_m,
                                       fe->cfg.lfr_n, t_lfr, outp + u * t_lfr * cols);
                }
            }
            LELE_HIP_CHECK(hipGetLastError());
            return 0;
        }
    }
    ctx->set_route("fe.generic_four");
    const int64_t per_utt = nf * (4 + fe->n_fft * 4 + bins * 4 + nm * 4);
    const int64_t ub = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(batch, 65535), (int64_t(1) << 28) / std::max<int64_t>(per_utt, 1)));
    void *gm = nullptr, *gf = nullptr, *gp = nullptr, *gl = nullptr;
    LELE_TRY(ctx->arena_alloc((size_t)ub * nf * 4, &gm));
    LELE_TRY(ctx->arena_alloc((size_t)ub * nf * fe->n_fft * 4, &gf));
    LELE_TRY(ctx->arena_alloc((size_t)ub * nf * bins * 4, &gp));
    if (!want_logmel) LELE_TRY(ctx->arena_alloc((size_t)ub * nf * nm * 4, &gl));
    auto blocks = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192))); };
    for (int64_t u = 0; u < batch; u += ub) {
        const int64_t nu = std::min<int64_t>(ub, batch - u), rows = nu * nf;
        const float* up = (const float*)dpcm + u * pcm_len;
        float* lm = want_logmel ? outp + u * nf * nm : (float*)gl;
        hipLaunchKernelGGL(fe_generic_mean_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, ctx->stream, up, rows, nf, pcm_len,
                           (int)fe->frame_len, (int)fe->hop_len, (float*)gm);
        hipLaunchKernelGGL(fe_generic_frame_kernel, blocks(rows * fe->n_fft), dim3(256), 0, ctx->stream, up, (const float*)gm,
                           fe->g_window, rows, nf, pcm_len, (int)fe->frame_len, (int)fe->hop_len, (int)fe->n_fft, (float*)gf);
        LELE_TRY(fft_rows_power(ctx, (const float*)gf, rows, fe->n_fft, (float*)gp));
        hipLaunchKernelGGL(fe_generic_mel_kernel, blocks(rows * nm), dim3(256), 0, ctx->stream, (const float*)gp, rows, (int)bins,
                           (int)nm, fe->g_mstart, fe->g_moff, fe->g_mw, lm);
        if (!want_logmel) {
            dim3 lg = blocks(t_lfr * cols);
            lg.y = (unsigned)nu;
            hipLaunchKernelGGL(fe_generic_lfr_kernel, lg, dim3(256), 0, ctx->stream, (const float*)lm, nf, nm,
                               fe->cfg.lfr_m, fe->cfg.lfr_n, t_lfr, outp + u * t_lfr * cols);
        }
    }
    LELE_HIP_CHECK(hipGetLastError());
    return 0;
}

static int fe_run(LeleFrontend* fe, const LeleTensor* pcm, int64_t batch, int64_t pcm_len, LeleBuf* out,
                  bool want_logmel, int64_t* out_shape, int32_t* out_rank) {
    LeleCtx* ctx = fe->ctx;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_REQUIRE(pcm->dtype == LELE_F32, "frontend: pcm must be f32");
    int64_t t_lfr = 0, cols = 0, nf = 0;
    lele_hip_frontend_out_rows(fe, pcm_len, &t_lfr, &cols, &nf);
    ctx->set_route(nullptr);  // lele_hip_last_route: "" for a call that launches nothing
    if (nf == 0 || batch == 0) {  // TensorView::empty()
        out->bytes = 0;
        if (out_rank) *out_rank = 0;
        return 0;
    }
    LELE_TRY(ctx->arena_reset());
    const void* dpcm = nullptr;
    LELE_TRY(ctx->dev_ptr(pcm, &dpcm));
    void* dmean = nullptr;
    LELE_TRY(ctx->get_scratch((size_t)batch * nf * sizeof(float), &dmean));
    const size_t out_elems = want_logmel ? (size_t)batch * nf * fe->cfg.n_mels : (size_t)batch * t_lfr * cols;
    LELE_TRY(out->reserve(out_elems * sizeof(float)));
    if (!fe->fast) {
        LELE_TRY(fe_generic(fe, (const float*)dpcm, batch, pcm_len, nf, t_lfr, cols, (float*)out->data, want_logmel, dmean));
        if (want_logmel) {
            if (batch == 1) return set_shape(out_shape, out_rank, {nf, fe->cfg.n_mels});
            return set_shape(out_shape, out_rank, {batch, nf, fe->cfg.n_mels});
        }
        return 0;
    }
    // the kernel addresses an utterance's output by 32-bit byte offsets from the utterance's base
    LELE_REQUIRE((want_logmel ? nf * fe->cfg.n_mels : t_lfr * cols) < (int64_t(1) << 30),
                 "frontend: the features of one utterance (%lld frames) exceed 4 GiB", (long long)nf);
    const int aligned16 = ((uintptr_t)dpcm % 16 == 0) && (pcm_len % 4 == 0);
    // lele_hip_last_route: the kernel, then how it stages its PCM tile -- the condition fe_main_body evaluates (`tile_dma` there) on the
    // same two values; the two-kernel lab form has no tile
    const FeForm form = fe->form;
    ctx->set_route(form.std_mel ? "fe.main_std" : "fe.main_table",
                   !form.fused ? "fe.two_kernel" : fe_tile_route(aligned16 && fe->dev.tile_dma, 1));
    constexpr int64_t kMaxGridY = 65535;  // utterances a launch: a longer batch runs in chunks (pcm_len % 4 == 0 where aligned16, so it holds for every chunk)
    hipEvent_t* ev = nullptr;
    if (fe->profiling) {
        if (fe->events_used + 3 > fe->events.size()) {
            for (int i = 0; i < 3; ++i) {
                hipEvent_t e;
                LELE_HIP_CHECK(hipEventCreate(&e));
                fe->events.push_back(e);
            }
        }
        ev = &fe->events[fe->events_used];
        fe->events_used += 3;
        LELE_HIP_CHECK(hipEventRecord(ev[0], ctx->stream));
    }
    for (int64_t c0 = 0; !form.fused && c0 < batch; c0 += kMaxGridY) {
        const dim3 grid((unsigned)((nf + 63) / 64), (unsigned)std::min<int64_t>(kMaxGridY, batch - c0));
        hipLaunchKernelGGL(fe_frame_sum_kernel, grid, dim3(64), 0, ctx->stream, (const float*)dpcm + c0 * pcm_len, pcm_len, pcm_len, nf,
                           (float*)dmean + c0 * nf, aligned16);
    }
    if (ev) LELE_HIP_CHECK(hipEventRecord(ev[1], ctx->stream));
    LELE_TRY(fe_dispatch(fe, form, [&](auto t) {
        using T = decltype(t);
        for (int64_t c0 = 0; c0 < batch; c0 += kMaxGridY) {  // every chunk's utterances land where the one launch would put them
            const dim3 grid((unsigned)((nf + 63) / 64), (unsigned)std::min<int64_t>(kMaxGridY, batch - c0));
            float* o = want_logmel ? nullptr : (float*)out->data + c0 * t_lfr * cols;
            float* lm = want_logmel ? (float*)out->data + c0 * nf * fe->cfg.n_mels : nullptr;
            hipLaunchKernelGGL((fe_main_kernel<T::mode, T::std_mel, T::fused, T::opt>), grid, dim3(256), fe_mel_lds(fe), ctx->stream,
                               (const float*)dpcm + c0 * pcm_len, pcm_len, nf, t_lfr, (const float*)dmean + c0 * nf, fe->dev, o, lm, aligned16);
        }
    }));
    LELE_HIP_CHECK(hipGetLastError());
    if (ev) LELE_HIP_CHECK(hipEventRecord(ev[2], ctx->stream));
    if (want_logmel) {
        if (batch == 1) return set_shape(out_shape, out_rank, {nf, fe->cfg.n_mels});
        return set_shape(out_shape, out_rank, {batch, nf, fe->cfg.n_mels});
    }
    return 0;
}

int lele_hip_frontend_compute(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                              int32_t* out_rank) {
    LELE_REQUIRE(fe && pcm && out, "frontend_compute: NULL argument");
    const int64_t n = numel(pcm);
    LELE_TRY(fe_run(fe, pcm, 1, n, out, false, out_shape, out_rank));
    if (out->bytes == 0) return 0;
    int64_t t = 0, cols = 0;
    lele_hip_frontend_out_rows(fe, n, &t, &cols, nullptr);
    return set_shape(out_shape, out_rank, {t, cols});
}

int lele_hip_frontend_compute_batch(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank) {
    LELE_REQUIRE(fe && pcm && out, "frontend_compute_batch: NULL argument");
    LELE_REQUIRE(pcm->rank == 2, "frontend_compute_batch: pcm must be [batch, pcm_len]");
    const int64_t batch = pcm->shape[0], n = pcm->shape[1];
    LELE_TRY(fe_run(fe, pcm, batch, n, out, false, out_shape, out_rank));
    if (out->bytes == 0) return 0;
    int64_t t = 0, cols = 0;
    lele_hip_frontend_out_rows(fe, n, &t, &cols, nullptr);
    return set_shape(out_shape, out_rank, {batch, t, cols});
}

int lele_hip_frontend_logmel(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                             int32_t* out_rank) {
    LELE_REQUIRE(fe && pcm && out, "frontend_logmel: NULL argument");
    if (pcm->rank == 2) return fe_run(fe, pcm, pcm->shape[0], pcm->shape[1], out, true, out_shape, out_rank);
    return fe_run(fe, pcm, 1, numel(pcm), out, true, out_shape, out_rank);
}

/* Segments of one PCM buffer in one launch pair (see lele_hip.h).  Validation first (nothing is launched and `out` is untouched on
 * failure), then the packed row offsets, then either the segment-aware kernels (default config) or, on the generic path, the
 * generic kernels once per segment. */
struct SegLayout {  // host inputs of the table builder below
    const LeleFrontend* fe;
    const int64_t* starts;
    const int64_t* lengths;
    int64_t count;
    const int64_t* rows;  // row_offsets
};
static void build_seg_table(const void* arg, std::vector<char>& blob) {
    const SegLayout& L = *(const SegLayout*)arg;
    std::vector<FeSeg> segs;
    std::vector<int> blk;
    for (int64_t i = 0; i < L.count; ++i) {
        int64_t t = 0, nf = 0;
        lele_hip_frontend_out_rows(L.fe, L.lengths[i], &t, nullptr, &nf);
        if (nf == 0) continue;
        const int64_t nb = (nf + 63) / 64;
        segs.push_back(FeSeg{L.starts[i], L.lengths[i], nf, t, L.rows[i], (int64_t)blk.size()});
        blk.insert(blk.end(), (size_t)nb, (int)segs.size() - 1);
    }
    blob.resize(segs.size() * sizeof(FeSeg) + blk.size() * sizeof(int));
    memcpy(blob.data(), segs.data(), segs.size() * sizeof(FeSeg));
    memcpy(blob.data() + segs.size() * sizeof(FeSeg), blk.data(), blk.size() * sizeof(int));
}

int lele_hip_frontend_compute_segments(LeleFrontend* fe, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths, int64_t count,
                                       LeleBuf* out, int64_t* row_offsets, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(fe && pcm && out && row_offsets, "frontend_compute_segments: NULL argument");
    LELE_REQUIRE(count >= 0 && (count == 0 || (starts && lengths)), "frontend_compute_segments: bad segment arrays (count %lld)",
                 (long long)count);
    LELE_REQUIRE(pcm->dtype == LELE_F32 && pcm->rank == 1, "frontend_compute_segments: pcm must be f32 [N]");
    const int64_t n = pcm->shape[0];
    for (int64_t i = 0; i < count; ++i)
        LELE_REQUIRE(starts[i] >= 0 && lengths[i] >= 0 && starts[i] <= n - lengths[i],
                     "frontend_compute_segments: segment %lld (start %lld, length %lld) lies outside the %lld samples of pcm", (long long)i,
                     (long long)starts[i], (long long)lengths[i], (long long)n);
    int64_t cols = fe->cfg.n_mels * fe->cfg.lfr_m, blocks = 0, max_nf = 0;
    row_offsets[0] = 0;
    for (int64_t i = 0; i < count; ++i) {
        int64_t t = 0, nf = 0;
        lele_hip_frontend_out_rows(fe, lengths[i], &t, nullptr, &nf);
        row_offsets[i + 1] = row_offsets[i] + t;
        blocks += (nf + 63) / 64;
        max_nf = std::max(max_nf, nf);
    }
    const int64_t rows = row_offsets[count];
    fe->ctx->set_route(nullptr);  // lele_hip_last_route: "" for a call that launches nothing
    if (rows == 0) {  // no segment holds a frame: TensorView::empty()
        out->bytes = 0;
        if (out_rank) *out_rank = 0;
        return 0;
    }
    LELE_REQUIRE(blocks < (int64_t(1) << 31), "frontend_compute_segments: %lld blocks exceed the grid", (long long)blocks);
    // (fe_run's bound, per segment: 32-bit byte offsets inside a segment's rows)
    LELE_REQUIRE(!fe->fast || (max_nf + fe->cfg.lfr_n - 1) / fe->cfg.lfr_n * cols < (int64_t(1) << 30),
                 "frontend_compute_segments: the features of one segment (%lld frames) exceed 4 GiB", (long long)max_nf);
    LeleCtx* ctx = fe->ctx;
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LELE_TRY(ctx->arena_reset());
    const void* dpcm = nullptr;
    LELE_TRY(ctx->dev_ptr(pcm, &dpcm));
    LELE_TRY(out->reserve((size_t)rows * cols * sizeof(float)));
    float* o = (float*)out->data;
    if (!fe->fast) {
        // generic path: correct, not fast -- the generic kernels once per segment (they take equal-length batches only); the arena
        // scratch of one segment is reused by the next, which the stream orders after it
        void* dmean = nullptr;
        LELE_TRY(ctx->get_scratch((size_t)max_nf * sizeof(float), &dmean));
        const size_t mark = ctx->arena_used;
        for (int64_t i = 0; i < count; ++i) {
            int64_t t = 0, nf = 0;
            lele_hip_frontend_out_rows(fe, lengths[i], &t, nullptr, &nf);
            if (nf == 0) continue;
            LELE_TRY(fe_generic(fe, (const float*)dpcm + starts[i], 1, lengths[i], nf, t, cols, o + row_offsets[i] * cols, false, dmean));
            ctx->arena_used = mark;
        }
        return set_shape(out_shape, out_rank, {rows, cols});
    }
    // the layout's device table (shape metadata: uploaded once per distinct layout, never rewritten -- safe under graph capture)
    std::string key((size_t)count * 16, '\0');
    memcpy(&key[0], starts, (size_t)count * 8);
    memcpy(&key[(size_t)count * 8], lengths, (size_t)count * 8);
    const SegLayout lay{fe, starts, lengths, count, row_offsets};
    const void* table = nullptr;
    LELE_TRY(fe->seg_tables.get(ctx, std::move(key), build_seg_table, &lay, &table));
    int64_t nseg = 0;
    for (int64_t i = 0; i < count; ++i) nseg += lengths[i] >= fe->frame_len;
    const FeSeg* dsegs = (const FeSeg*)table;
    const int* dblk = (const int*)(dsegs + nseg);
    // lele_hip_last_route: the kernel, then the tile staging of its blocks -- fe_seg_main_kernel's own per-segment condition, evaluated
    // here on the same values; one name for a launch that holds both kinds
    int64_t n_dma = 0;
    for (int64_t i = 0; i < count; ++i)
        if (lengths[i] >= fe->frame_len)
            n_dma += (((uintptr_t)((const float*)dpcm + starts[i]) & 15) == 0) && (lengths[i] % 4 == 0) && fe->dev.tile_dma;
    FeForm form = fe->form;
    form.fused = true;  // (the two-kernel form is a lab switch of compute() alone)
    ctx->set_route(form.std_mel ? "fe.seg_std" : "fe.seg_table", fe_tile_route(n_dma, nseg));
    LELE_TRY(fe_dispatch(fe, form, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((fe_seg_main_kernel<T::mode, T::std_mel, T::opt>), dim3((unsigned)blocks), dim3(256), fe_mel_lds(fe), ctx->stream,
                           (const float*)dpcm, dsegs, dblk, fe->dev, o);
    }));
    LELE_HIP_CHECK(hipGetLastError());
    return set_shape(out_shape, out_rank, {rows, cols});
}

/* ---- chunked streaming (see lele_hip.h): the closed forms, the per-stream state and one push ---- */
}  // extern "C"

namespace {
struct FeStreamDims {
    int64_t frame_len, hop, m, n, pad;
    int64_t frames(int64_t len) const { return len < frame_len ? 0 : (len - frame_len) / hop + 1; }  // pipeline.rs:70-73
    // rows whose right-most frame i*n + m-1-pad exists among t frames
    int64_t rows(int64_t t) const { return t - 1 >= m - 1 - pad ? (t - 1 - (m - 1 - pad)) / n + 1 : 0; }
    int64_t rows_final(int64_t t) const { return (t + n - 1) / n; }  // lfr.rs:33
    // samples that a later frame still needs: from the first sample of frame t on (everything while there is no frame)
    int64_t pcm_carry(int64_t len, int64_t t) const { return t == 0 ? len : std::max<int64_t>(0, len - t * hop); }
    // frames that a later row still needs: from the left-most frame of row e on
    int64_t mel_carry(int64_t t, int64_t e) const { return std::max<int64_t>(0, t - std::max<int64_t>(0, e * n - pad)); }
};
int fe_stream_dims(const LeleFeatureConfig* cfg, FeStreamDims* d) {
    LELE_REQUIRE(cfg->sample_rate > 0 && cfg->n_mels > 0 && cfg->lfr_m > 0 && cfg->lfr_n > 0, "frontend_stream: invalid FeatureConfig");
    d->frame_len = (int64_t)((float)cfg->sample_rate * cfg->frame_length_ms / 1000.0f);  // pipeline.rs:39
    d->hop = (int64_t)((float)cfg->sample_rate * cfg->frame_shift_ms / 1000.0f);         // pipeline.rs:42
    d->m = cfg->lfr_m;
    d->n = cfg->lfr_n;
    d->pad = (cfg->lfr_m - 1) / 2;
    LELE_REQUIRE(d->frame_len >= 1 && d->hop >= 1, "frontend_stream: frame_len=%lld hop_len=%lld", (long long)d->frame_len, (long long)d->hop);
    return 0;
}
}  // namespace

struct LeleFrontendStream {
    LeleFrontend* fe = nullptr;
    hipStream_t stream = nullptr;  // the ctx stream the pushes are issued on (drained before the state is freed)
    FeStreamDims dims{};
    int64_t streams = 0, max_chunk = 0;
    int64_t max_new_frames = 0;  // the most frames one push can complete
    float* pcm_state = nullptr;  // [streams][pcm_pitch]: carried samples, then the chunk
    float* mel_state = nullptr;  // [streams][mel_pitch]: carried log-mel rows, then the new frames'
    int64_t pcm_pitch = 0, mel_pitch = 0;  // floats
    std::vector<int64_t> samples, frames, rows;  // L, T, E of every stream: functions of the chunk lengths alone
};

extern "C" {

int lele_hip_frontend_stream_rows(const LeleFeatureConfig* cfg, int64_t samples_before, int64_t chunk_len, int32_t final, int64_t* rows,
                                  int64_t* new_frames, int64_t* pcm_carry, int64_t* mel_carry) {
    LELE_REQUIRE(cfg, "frontend_stream_rows: cfg is NULL");
    LELE_REQUIRE(samples_before >= 0 && chunk_len >= 0, "frontend_stream_rows: negative sample count");
    FeStreamDims d;
    LELE_TRY(fe_stream_dims(cfg, &d));
    const int64_t t0 = d.frames(samples_before), len = samples_before + chunk_len, t1 = d.frames(len);
    const int64_t e0 = d.rows(t0), e1 = final ? d.rows_final(t1) : d.rows(t1);
    if (rows) *rows = e1 - e0;
    if (new_frames) *new_frames = t1 - t0;
    if (pcm_carry) *pcm_carry = final ? 0 : d.pcm_carry(len, t1);  // (a final push resets the stream)
    if (mel_carry) *mel_carry = final ? 0 : d.mel_carry(t1, e1);
    return 0;
}

int lele_hip_frontend_stream_create(LeleFrontend* fe, int64_t streams, int64_t max_chunk, LeleFrontendStream** out) {
    LELE_REQUIRE(fe && out, "frontend_stream_create: NULL argument");
    LELE_REQUIRE(streams >= 1 && max_chunk >= 1, "frontend_stream_create: streams %lld and max_chunk %lld must be at least 1", (long long)streams,
                 (long long)max_chunk);
    FeStreamDims d;
    LELE_TRY(fe_stream_dims(&fe->cfg, &d));
    // (a shift longer than the frame would have to DROP samples between two frames; no model this library serves is framed that way)
    LELE_REQUIRE(d.hop <= d.frame_len, "frontend_stream_create: the frame shift (%lld samples) is longer than the frame (%lld)", (long long)d.hop,
                 (long long)d.frame_len);
    LeleCtx* ctx = fe->ctx;
    LELE_REQUIRE(!ctx->capturing, "graph capture: frontend_stream_create allocates; create the stream before capturing");
    const int64_t max_new = (max_chunk - 1) / d.hop + 1;
    const int64_t pcm_pitch = (d.frame_len - 1 + max_chunk + 3) & ~int64_t(3);
    const int64_t mel_pitch = ((d.m - 1 + max_new) * fe->cfg.n_mels + 3) & ~int64_t(3);
    // the kernels index a region with 32-bit offsets, the grids count blocks in 32 bits
    LELE_REQUIRE(pcm_pitch < (int64_t(1) << 30) && mel_pitch < (int64_t(1) << 30) && streams < (int64_t(1) << 24),
                 "frontend_stream_create: %lld streams of %lld samples a push are beyond the kernels' 32-bit offsets", (long long)streams,
                 (long long)max_chunk);
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    LeleFrontendStream* st = new LeleFrontendStream();
    st->fe = fe;
    st->stream = ctx->stream;
    st->dims = d;
    st->streams = streams;
    st->max_chunk = max_chunk;
    st->max_new_frames = max_new;
    st->pcm_pitch = pcm_pitch;
    st->mel_pitch = mel_pitch;
    st->samples.assign((size_t)streams, 0);
    st->frames.assign((size_t)streams, 0);
    st->rows.assign((size_t)streams, 0);
    hipError_t e = hipMalloc((void**)&st->pcm_state, (size_t)streams * pcm_pitch * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&st->mel_state, (size_t)streams * mel_pitch * sizeof(float));
    if (e != hipSuccess) {
        if (st->pcm_state) (void)hipFree(st->pcm_state);
        delete st;
        LELE_HIP_CHECK(e);
    }
    *out = st;
    return 0;
}

int lele_hip_frontend_stream_destroy(LeleFrontendStream* st) {
    if (!st) return 0;
    (void)hipStreamSynchronize(st->stream);
    (void)hipFree(st->pcm_state);
    (void)hipFree(st->mel_state);
    delete st;
    return 0;
}

int lele_hip_frontend_stream_reset(LeleFrontendStream* st, const int64_t* ids, int64_t count) {
    LELE_REQUIRE(st, "frontend_stream_reset: st is NULL");
    if (!ids) {
        std::fill(st->samples.begin(), st->samples.end(), 0);
        std::fill(st->frames.begin(), st->frames.end(), 0);
        std::fill(st->rows.begin(), st->rows.end(), 0);
        return 0;
    }
    for (int64_t i = 0; i < count; ++i)
        LELE_REQUIRE(ids[i] >= 0 && ids[i] < st->streams, "frontend_stream_reset: id %lld is not one of the %lld streams", (long long)ids[i],
                     (long long)st->streams);
    for (int64_t i = 0; i < count; ++i) st->samples[ids[i]] = st->frames[ids[i]] = st->rows[ids[i]] = 0;
    return 0;
}

int lele_hip_frontend_stream_counters(const LeleFrontendStream* st, int64_t id, int64_t* samples, int64_t* frames, int64_t* rows) {
    LELE_REQUIRE(st, "frontend_stream_counters: st is NULL");
    LELE_REQUIRE(id >= 0 && id < st->streams, "frontend_stream_counters: id %lld is not one of the %lld streams", (long long)id, (long long)st->streams);
    if (samples) *samples = st->samples[id];
    if (frames) *frames = st->frames[id];
    if (rows) *rows = st->rows[id];
    return 0;
}

int lele_hip_frontend_stream_push(LeleFrontendStream* st, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths,
                                  const uint8_t* final_or_null, LeleBuf* out, int64_t* row_offsets, int64_t* out_shape, int32_t* out_rank) {
    LELE_REQUIRE(st && pcm && starts && lengths && out && row_offsets, "frontend_stream_push: NULL argument");
    LeleFrontend* fe = st->fe;
    LeleCtx* ctx = fe->ctx;
    LELE_REQUIRE(!ctx->capturing, "frontend_stream_push: a push cannot be recorded into a graph (the stream counters advance on the host at "
                                  "every call); push eagerly and capture what consumes the rows");
    LELE_REQUIRE(pcm->dtype == LELE_F32 && pcm->rank == 1, "frontend_stream_push: pcm must be f32 [N]");
    const int64_t n = pcm->shape[0], count = st->streams;
    for (int64_t i = 0; i < count; ++i) {
        LELE_REQUIRE(starts[i] >= 0 && lengths[i] >= 0 && starts[i] <= n - lengths[i],
                     "frontend_stream_push: the chunk of stream %lld (start %lld, length %lld) lies outside the %lld samples of pcm", (long long)i,
                     (long long)starts[i], (long long)lengths[i], (long long)n);
        LELE_REQUIRE(lengths[i] <= st->max_chunk, "frontend_stream_push: the chunk of stream %lld has %lld samples, the stream was created for %lld",
                     (long long)i, (long long)lengths[i], (long long)st->max_chunk);
    }
    // the plan of this push: one record a stream, one stream index a block of the log-mel and the emit grids.  Host arithmetic only;
    // the counters are committed after the last launch has been issued.
    const FeStreamDims& d = st->dims;
    const int64_t nm = fe->cfg.n_mels, cols = nm * d.m;
    std::vector<FeStreamRec> recs((size_t)count);
    std::vector<int> blk, eblk;
    std::vector<int64_t> nl((size_t)count), nt((size_t)count), ne((size_t)count);
    int64_t max_chunk = 0, max_nf = 0, n_live = 0, n_dma = 0;
    bool moves = false;
    row_offsets[0] = 0;
    for (int64_t i = 0; i < count; ++i) {
        const bool fin = final_or_null && final_or_null[i];
        const int64_t L = st->samples[i], T = st->frames[i], E = st->rows[i];
        const int64_t c = d.pcm_carry(L, T), mc = d.mel_carry(T, E), len = c + lengths[i];
        const int64_t L2 = L + lengths[i], T2 = d.frames(L2), E2 = fin ? d.rows_final(T2) : d.rows(T2);
        FeStreamRec& r = recs[(size_t)i];
        r = FeStreamRec{};
        r.src = starts[i];
        r.chunk = (int32_t)lengths[i];
        r.carry = (int32_t)c;
        r.nf = (int32_t)(T2 - T);
        r.block0 = (int32_t)blk.size();
        r.mel_carry = (int32_t)mc;
        r.mel_base = T - mc;
        r.row_lo = E;
        r.rows = (int32_t)(E2 - E);
        r.emit_block0 = (int32_t)eblk.size();
        r.final = fin;
        r.last_frame = T2 - 1;
        r.out_row0 = row_offsets[i];
        if (!fin) {
            r.pcm_keep = (int32_t)d.pcm_carry(L2, T2);
            r.pcm_from = (int32_t)(len - r.pcm_keep);
            r.mel_keep = (int32_t)d.mel_carry(T2, E2);
            r.mel_from = (int32_t)(mc + r.nf - r.mel_keep);
            moves = moves || (r.pcm_keep && r.pcm_from) || (r.mel_keep && r.mel_from);
        }
        blk.insert(blk.end(), (size_t)((r.nf + 63) / 64), (int)i);
        eblk.insert(eblk.end(), (size_t)((r.rows + kEmitRows - 1) / kEmitRows), (int)i);
        row_offsets[i + 1] = row_offsets[i] + r.rows;
        max_chunk = std::max<int64_t>(max_chunk, lengths[i]);
        max_nf = std::max<int64_t>(max_nf, r.nf);
        n_live += r.nf > 0;
        n_dma += r.nf > 0 && len % 4 == 0 && fe->dev.tile_dma;  // fe_stream_main_kernel's own condition: the regions start 16-byte aligned
        nl[(size_t)i] = fin ? 0 : L2;   // a final push leaves the stream reset
        nt[(size_t)i] = fin ? 0 : T2;
        ne[(size_t)i] = fin ? 0 : E2;
    }
    const int64_t total_rows = row_offsets[count];
    const int64_t pieces = (max_chunk + kAppendPiece - 1) / kAppendPiece;
    LELE_REQUIRE(count * pieces < (int64_t(1) << 31) && blk.size() < (size_t(1) << 31) && eblk.size() < (size_t(1) << 31),
                 "frontend_stream_push: %lld streams of up to %lld samples exceed the grid", (long long)count, (long long)max_chunk);
    LELE_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->set_route(nullptr);  // lele_hip_last_route: "" when no stream gained a frame
    LELE_TRY(ctx->arena_reset());
    const void* dpcm = nullptr;
    LELE_TRY(ctx->dev_ptr(pcm, &dpcm));
    // the table changes every push: through the staging arena, not through the exact-keyed seg_tables
    const size_t rec_bytes = recs.size() * sizeof(FeStreamRec), blk_bytes = blk.size() * sizeof(int), eblk_bytes = eblk.size() * sizeof(int);
    std::vector<char> blob(rec_bytes + blk_bytes + eblk_bytes);
    memcpy(blob.data(), recs.data(), rec_bytes);
    if (blk_bytes) memcpy(blob.data() + rec_bytes, blk.data(), blk_bytes);
    if (eblk_bytes) memcpy(blob.data() + rec_bytes + blk_bytes, eblk.data(), eblk_bytes);
    void* dtab = nullptr;
    LELE_TRY(ctx->arena_alloc(blob.size(), &dtab));
    void* dmean = nullptr;
    if (!fe->fast && max_nf) LELE_TRY(ctx->get_scratch((size_t)max_nf * sizeof(float), &dmean));
    if (total_rows) LELE_TRY(out->reserve((size_t)total_rows * cols * sizeof(float)));
    LELE_HIP_CHECK(hipMemcpyAsync(dtab, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));  // (pageable: staged before it returns)
    const FeStreamRec* drecs = (const FeStreamRec*)dtab;
    const int* dblk = (const int*)((const char*)dtab + rec_bytes);
    const int* deblk = (const int*)((const char*)dtab + rec_bytes + blk_bytes);
    if (pieces)
        hipLaunchKernelGGL(fe_stream_append_kernel, dim3((unsigned)(count * pieces)), dim3(64), 0, ctx->stream, (const float*)dpcm, drecs, (int)pieces,
                           st->pcm_state, st->pcm_pitch);
    if (n_live && !fe->fast) {
        // generic path: correct, not fast -- the generic kernels once per stream on the same regions (compute_segments does the same)
        const size_t mark = ctx->arena_used;
        for (int64_t i = 0; i < count; ++i) {
            const FeStreamRec& r = recs[(size_t)i];
            if (r.nf == 0) continue;
            LELE_TRY(fe_generic(fe, st->pcm_state + i * st->pcm_pitch, 1, (int64_t)r.carry + r.chunk, r.nf, 0, cols,
                                st->mel_state + i * st->mel_pitch + (int64_t)r.mel_carry * nm, true, dmean));
            ctx->arena_used = mark;
        }
    } else if (n_live) {
        // lele_hip_last_route: this is the segment kernel's body over the streams' regions, so it reports the segment names
        FeForm form = fe->form;
        form.fused = true;
        ctx->set_route(form.std_mel ? "fe.seg_std" : "fe.seg_table", fe_tile_route(n_dma, n_live));
        LELE_TRY(fe_dispatch(fe, form, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((fe_stream_main_kernel<T::mode, T::std_mel, T::opt>), dim3((unsigned)blk.size()), dim3(256), fe_mel_lds(fe),
                               ctx->stream, (const float*)st->pcm_state, st->pcm_pitch, drecs, dblk, fe->dev, st->mel_state, st->mel_pitch);
        }));
    }
    if (total_rows) {
        if (nm % 4 == 0)
            hipLaunchKernelGGL(fe_stream_emit_kernel<true>, dim3((unsigned)eblk.size()), dim3(256), 0, ctx->stream, (const float*)st->mel_state,
                               st->mel_pitch, drecs, deblk, (int)nm, (int)d.m, (int)d.n, (float*)out->data);
        else
            hipLaunchKernelGGL(fe_stream_emit_kernel<false>, dim3((unsigned)eblk.size()), dim3(256), 0, ctx->stream, (const float*)st->mel_state,
                               st->mel_pitch, drecs, deblk, (int)nm, (int)d.m, (int)d.n, (float*)out->data);
    }
    if (moves)
        hipLaunchKernelGGL(fe_stream_compact_kernel, dim3((unsigned)count), dim3(256), 0, ctx->stream, drecs, st->pcm_state, st->pcm_pitch,
                           st->mel_state, st->mel_pitch, (int)nm);
    LELE_HIP_CHECK(hipGetLastError());
    st->samples.swap(nl);
    st->frames.swap(nt);
    st->rows.swap(ne);
    if (total_rows == 0) {  // nothing became final this tick: TensorView::empty()
        out->bytes = 0;
        if (out_rank) *out_rank = 0;
        return 0;
    }
    return set_shape(out_shape, out_rank, {total_rows, cols});
}

int lele_hip_frontend_set_profiling(LeleFrontend* fe, int on) {
    LELE_REQUIRE(fe, "frontend_set_profiling: fe is NULL");
    fe->profiling = on != 0;
    fe->events_used = 0;
    return 0;
}

int lele_hip_frontend_profile_read(LeleFrontend* fe, float* sum_kernel_ms, float* main_kernel_ms, int64_t* runs) {
    LELE_REQUIRE(fe, "frontend_profile_read: fe is NULL");
    LELE_HIP_CHECK(hipStreamSynchronize(fe->ctx->stream));
    double a = 0, b = 0;
    const size_t n = fe->events_used / 3;
    for (size_t i = 0; i < n; ++i) {
        float m0 = 0, m1 = 0;
        LELE_HIP_CHECK(hipEventElapsedTime(&m0, fe->events[3 * i], fe->events[3 * i + 1]));
        LELE_HIP_CHECK(hipEventElapsedTime(&m1, fe->events[3 * i + 1], fe->events[3 * i + 2]));
        a += m0;
        b += m1;
    }
    if (sum_kernel_ms) *sum_kernel_ms = n ? (float)(a / n) : 0.f;
    if (main_kernel_ms) *main_kernel_ms = n ? (float)(b / n) : 0.f;
    if (runs) *runs = (int64_t)n;
    fe->events_used = 0;
    return 0;
}

}  // extern "C"
