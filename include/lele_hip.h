/*
 * lele_hip.h -- C ABI of liblele_hip.so: an MI355X (gfx950) implementation of lele's hot path.
 *
 * Every entry point is what lele's FFI for the path would bind.  lele (Rust) has no GPU back end; the
 * precedent for a C-ABI kernel boundary in the reference is its macOS cblas_sgemm binding
 * (/root/reference/src/kernels/gemm.rs:30-47).  Each function below names the reference function it
 * replaces (file:line under /root/reference).  INTEGRATION.md shows the Rust `extern "C"` stub for each.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns 0 on success, non-zero on error; lele_hip_last_error() then describes it.
 *     lele's kernels panic! on shape/attr violations (e.g. rnn.rs:85-90, norm.rs:218); the Rust shim turns
 *     a non-zero code into the same panic, nothing unwinds across the FFI.
 *   - tensors are row-major, described by LeleTensor {data, shape, rank, dtype, mem}: the C image of
 *     lele::tensor::TensorView (src/tensor.rs:5-12).  mem says where `data` lives:
 *       LELE_MEM_HOST   : host memory, staged to the device for the call (drop-in semantics);
 *       LELE_MEM_DEVICE : device memory (e.g. lele_hip_buf_data() of a previous op's output);
 *       LELE_MEM_WEIGHT : host memory that is immutable for the life of the ctx (weights.bin slices):
 *                         uploaded (and pre-packed where an op needs it) once, cached by (ptr, bytes) --
 *                         the analogue of lele's thread-local B_WEIGHT_CACHE (avx/quantization.rs:12-95).
 *   - outputs go to a LeleBuf: a growable device allocation that mirrors the `out: &mut Vec<f32>` workspace
 *     buffers of generated code (src/compiler/mod.rs:148-290).  The op resizes it, writes the result and
 *     reports the result shape through out_shape[0..*out_rank) (capacity LELE_MAX_RANK).
 *   - a LeleCtx owns one HIP stream; all work of a ctx is stream-ordered; lele_hip_sync() drains it.
 *     One ctx per host thread (lele itself is single-threaded with thread-local scratch, conv2d.rs:601-603).
 */
#ifndef LELE_HIP_H
#define LELE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LELE_MAX_RANK 8

typedef enum { LELE_F32 = 0, LELE_I64 = 1, LELE_I32 = 2, LELE_U8 = 3, LELE_I8 = 4 } LeleDType;
typedef enum { LELE_MEM_HOST = 0, LELE_MEM_DEVICE = 1, LELE_MEM_WEIGHT = 2 } LeleMem;
typedef enum { LELE_ACT_NONE = 0, LELE_ACT_RELU = 1, LELE_ACT_SILU = 2 } LeleAct;

typedef struct LeleTensor {
    const void* data;
    const int64_t* shape;
    int32_t rank;
    int32_t dtype; /* LeleDType */
    int32_t mem;   /* LeleMem   */
} LeleTensor;

/* Channel views.  A Concat along C of NCHW tensors and a Split along C move no value: an operand of the Concat is the window
 * [c0, c1) of the result, a result of the Split the window [c0, c1) of its operand -- image n of such a window starts
 * n * pitch elements after image 0 (pitch = C_total * H * W of the enclosing tensor) and is dense inside.  The *_pitched entry
 * points take operands and / or write results of that form, so that the convolution / addition / pooling / resize that produces a
 * Concat operand writes it in place and the one that consumes a Split result reads it in place (lele copies: manipulation.rs:108-207,
 * 1091-1151; the values are the same).  All fields in ELEMENTS; 0 = dense.
 *   x_pitch, y_pitch : first / second tensor operand (its `data` already points at the window's first element)
 *   out_offset, out_pitch : the result goes to out's data + out_offset, images out_pitch apart; `out` must ALREADY hold the
 *                       enclosing tensor (lele_hip_buf_reserve) -- it is not resized, its other contents are untouched.  With
 *                       out_pitch == 0 the op resizes `out` and writes a dense result, as its plain form does. */
typedef struct LelePitch {
    int64_t x_pitch;
    int64_t y_pitch;
    int64_t out_offset;
    int64_t out_pitch;
} LelePitch;

typedef struct LeleCtx LeleCtx;
typedef struct LeleBuf LeleBuf;
typedef struct LeleFrontend LeleFrontend;
typedef struct LeleGraph LeleGraph;

/* ---- context / memory ------------------------------------------------------------------------------ */
const char* lele_hip_last_error(void);
int lele_hip_device_count(int* count);
int lele_hip_ctx_create(int device, LeleCtx** out);
int lele_hip_ctx_destroy(LeleCtx* ctx);
int lele_hip_sync(LeleCtx* ctx);
void* lele_hip_ctx_stream(LeleCtx* ctx); /* hipStream_t */
int lele_hip_ctx_num_cus(LeleCtx* ctx);  /* compute units of the ctx's device, as the dispatch thresholds read them; 0 for NULL */
/* hipGraph capture of an op sequence.  lele's generated forward() is a fixed sequence of kernel calls per input shape
 * (src/compiler/mod.rs:1291-1303); at SenseVoice's token counts every call is launch-latency bound, so the sequence is
 * recorded once and replayed as ONE graph launch.  Between begin and end every lele_hip_* op on this ctx is recorded
 * instead of executed; ops must not allocate, grow a LeleBuf, synchronise, or take LELE_MEM_HOST inputs while
 * capturing (they return an error) -- run the sequence once eagerly first, with the same buffers and shapes.  Replays
 * read and write the same device buffers as the recorded calls. */
int lele_hip_graph_begin(LeleCtx* ctx);
int lele_hip_graph_end(LeleCtx* ctx, LeleGraph** out);
int lele_hip_graph_abort(LeleCtx* ctx);
int lele_hip_graph_launch(LeleGraph* graph);
int lele_hip_graph_destroy(LeleGraph* graph);
/* Lanes: a ctx owns up to 4 HIP streams.  lele's generated forward() is a SEQUENCE, but the graph behind it is not: the FSMN memory
 * block of a SenseVoice layer does not depend on the attention beside it, the three detection heads of Yolo26n-seg not on each other
 * (examples/yolo26n-seg/src/yolo26seg.rs:509-627).  A plan runner that knows the dependencies issues independent branches on
 * different lanes; recorded between graph_begin and graph_end they become parallel branches of ONE hipGraph (while capturing, a lane
 * is a chain of graph nodes and an event the set of nodes it stands for: node-to-node edges on the one capturing stream).
 *   lane_set    : ops issued from now on go to `lane` (0 = the ctx stream of lele_hip_ctx_stream).  A lane has its own stream,
 *                 staging arena, scratch block and temporary buffers; it is created on first use (not while capturing: run the
 *                 sequence once eagerly with its lanes, as for every other allocation).  Results are ordered between lanes ONLY by
 *                 record / wait: the caller orders every cross-lane read-after-write, write-after-read and write-after-write.
 *   lane_record : event := everything issued on the current lane so far.
 *   lane_wait   : the current lane continues only after that point.
 * lele_hip_sync drains every lane; buf_to_host / graph_launch / the communicator use the CURRENT lane (call them on lane 0). */
int lele_hip_lane_set(LeleCtx* ctx, int lane);
int lele_hip_lane_record(LeleCtx* ctx, int event);
int lele_hip_lane_wait(LeleCtx* ctx, int event);
/* stream-ordered stopwatch (HIP events on the ctx stream) used by bench.py */
int lele_hip_timer_start(LeleCtx* ctx);
int lele_hip_timer_stop(LeleCtx* ctx, float* elapsed_ms);

int lele_hip_buf_create(LeleCtx* ctx, LeleBuf** out);
int lele_hip_buf_destroy(LeleBuf* buf);
int lele_hip_buf_reserve(LeleBuf* buf, size_t bytes);
void* lele_hip_buf_data(LeleBuf* buf);
/* Tell the library that the buffer's contents were written behind its back (through lele_hip_buf_data() + the ctx stream: a
 * hipMemcpy, an RCCL receive, the integrator's own kernel).  Producer-side statistics kept next to the buffer (the {min, max}
 * row pairs a LayerNorm / linear leaves for the dynamic quantisation that reads the tensor next) are dropped.  Every op of this
 * library does the equivalent on its own outputs. */
int lele_hip_buf_mark_dirty(LeleBuf* buf);
size_t lele_hip_buf_bytes(LeleBuf* buf); /* size of the last result in bytes */
int lele_hip_buf_from_host(LeleBuf* buf, const void* src, size_t bytes);
int lele_hip_buf_to_host(LeleBuf* buf, void* dst, size_t bytes); /* synchronises the ctx stream */

/* ---- src/features ---------------------------------------------------------------------------------- */
/* FeatureConfig, src/features/pipeline.rs:8-27 */
typedef struct LeleFeatureConfig {
    int64_t sample_rate;
    int64_t n_mels;
    float frame_length_ms;
    float frame_shift_ms;
    int64_t lfr_m;
    int64_t lfr_n;
} LeleFeatureConfig;

/* SenseVoiceFrontend::new, pipeline.rs:38-65 (window, twiddle/bit-reverse tables, sparse mel bank, LFR) */
/* hann_window (window.rs:2-13) and mel_filterbank (mel.rs:7-56; f_max = sample_rate / 2 unless has_f_max) as the library builds
 * them for its own front-end: host arithmetic into host memory (`size` floats / n_mels * (n_fft / 2 + 1) floats), no ctx. */
int lele_hip_hann_window(int64_t size, float* out);
float lele_hip_hz_to_mel_htk(float hz);   /* mel.rs:1-3 */
float lele_hip_mel_to_hz_htk(float mel);  /* mel.rs:4-6 */
int lele_hip_mel_filterbank(float sample_rate, int64_t n_fft, int64_t n_mels, float f_min, int32_t has_f_max, float f_max, float* out);
int lele_hip_frontend_create(LeleCtx* ctx, const LeleFeatureConfig* cfg, LeleFrontend** out);
int lele_hip_frontend_destroy(LeleFrontend* fe);
/* rows of the [T, n_mels*lfr_m] result for a pcm of `pcm_len` samples; 0 <=> TensorView::empty() (pipeline.rs:70-73) */
int lele_hip_frontend_out_rows(const LeleFrontend* fe, int64_t pcm_len, int64_t* rows, int64_t* cols,
                               int64_t* num_frames);
/* SenseVoiceFrontend::compute, pipeline.rs:67-193.  pcm: f32 [pcm_len] -> out [T, n_mels*lfr_m] */
int lele_hip_frontend_compute(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                              int32_t* out_rank);
/* The same for `batch` equal-length utterances stored back to back: pcm [batch, pcm_len] ->
 * out [batch, T, n_mels*lfr_m].  (lele loops over utterances on the host; examples/sensevoice/src/main.rs:58-86) */
int lele_hip_frontend_compute_batch(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank);
/* Segments of ONE pcm buffer (f32 [N]) in one launch: segment i = pcm[starts[i], starts[i] + lengths[i]) (host arrays of `count`;
 * any order, overlaps and repeats allowed, any start).  out [R, n_mels*lfr_m] holds the segments' rows one after another (the packed
 * layout): rows row_offsets[i] .. row_offsets[i+1] (host array of count + 1, written) are what lele_hip_frontend_compute gives for
 * that segment alone, bit for bit.  A segment shorter than one frame has 0 rows (its offsets repeat); count == 0 or R == 0 gives rank
 * 0.  Segments are checked before anything is launched (start < 0, length < 0 or start + length > N fail and leave `out` as it
 * was).  The default FeatureConfig takes one launch over every segment's 64-frame blocks; the segment layout is shape metadata,
 * uploaded once per distinct layout into a table the frontend owns until it is destroyed, so a graph may record the call (run the
 * layout once before capturing it).  Other FeatureConfigs (the generic path) run the generic kernels once per segment: correct,
 * not fast. */
int lele_hip_frontend_compute_segments(LeleFrontend* fe, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths,
                                       int64_t count, LeleBuf* out, int64_t* row_offsets, int64_t* out_shape, int32_t* out_rank);
/* log-mel before LFR ([num_frames, n_mels]) of the last compute call's shape, for tests */
int lele_hip_frontend_logmel(LeleFrontend* fe, const LeleTensor* pcm, LeleBuf* out, int64_t* out_shape,
                             int32_t* out_rank);
/* per-kernel stopwatch for bench.py's roofline block: while on, every compute call records HIP events around
 * its two kernels on the ctx stream (no synchronisation); profile_read() drains the stream and returns the
 * average duration of fe_frame_sum_kernel and fe_main_kernel over the `runs` calls since the last read. */
int lele_hip_frontend_set_profiling(LeleFrontend* fe, int on);
int lele_hip_frontend_profile_read(LeleFrontend* fe, float* sum_kernel_ms, float* main_kernel_ms, int64_t* runs);

/* ---- chunked streaming: N live streams (open microphones) fed a chunk a tick.  One push takes this tick's chunk of EVERY stream and
 * returns every feature row that has become final; concatenated per stream, the rows are bit for bit what lele_hip_frontend_compute
 * gives on the whole utterance, for any cut of the audio into chunks.  Per stream, after L samples in total (frame_len, hop, m, n of
 * the FeatureConfig, pad = (m - 1) / 2):
 *   frames        T(L) = L < frame_len ? 0 : (L - frame_len) / hop + 1
 *   rows emitted  E(L) = number of i >= 0 with i*n + (m-1-pad) <= T-1   (row i is final once its right-most frame exists; it is written
 *                 in the push that delivers that frame's last sample, no earlier and no later)
 * A push flagged final also emits rows E .. ceil(T/n)-1 with the right clamp to frame T-1 (lfr.rs:43-44), drops the samples that
 * complete no frame (as compute does) and resets the stream; a stream that never reaches one frame yields 0 rows.  The left clamp (raw
 * index < 0 reads frame 0) applies at the start of a stream only.  Between pushes the device keeps, per stream, fewer than frame_len
 * samples (the last L - T*hop, or all L while L < frame_len) and at most m-1 log-mel rows (frames max(0, E*n - pad) .. T-1); the
 * counters L, T, E live on the host and are functions of the chunk lengths alone. */
typedef struct LeleFrontendStream LeleFrontendStream;
/* The closed forms above for one push of chunk_len samples onto a stream that has seen samples_before: rows the push emits, frames it
 * completes, and the samples / log-mel rows carried AFTER it (0 and 0 after a final push).  Host arithmetic, no ctx, no GPU. */
int lele_hip_frontend_stream_rows(const LeleFeatureConfig* cfg, int64_t samples_before, int64_t chunk_len, int32_t final, int64_t* rows,
                                  int64_t* new_frames, int64_t* pcm_carry, int64_t* mel_carry);
/* State of `streams` streams that take at most max_chunk samples a push, all of it allocated here: per stream a PCM region of
 * frame_len - 1 + max_chunk samples (16-byte aligned base, pitch a multiple of 4 floats) and a log-mel region of m - 1 + (the most frames
 * one push completes) rows.  Destroy it before its LeleFrontend.  Refused: a frame shift longer than the frame. */
int lele_hip_frontend_stream_create(LeleFrontend* fe, int64_t streams, int64_t max_chunk, LeleFrontendStream** out);
int lele_hip_frontend_stream_destroy(LeleFrontendStream* st);
/* A new utterance in streams ids[0 .. count) (ids == NULL: in every stream).  Host counters only, nothing is launched. */
int lele_hip_frontend_stream_reset(LeleFrontendStream* st, const int64_t* ids, int64_t count);
/* samples seen (L), frames completed (T) and rows emitted (E) by stream `id` since its last reset or final push */
int lele_hip_frontend_stream_counters(const LeleFrontendStream* st, int64_t id, int64_t* samples, int64_t* frames, int64_t* rows);
/* One tick.  pcm: f32 [N], host or device; stream i's chunk is pcm[starts[i], starts[i] + lengths[i]) -- exactly one entry per stream,
 * length 0 = no audio this tick (legal together with final).  final_or_null: one flag a stream, NULL = none.  out [R, n_mels*lfr_m]
 * packed, row_offsets (streams + 1, written): the layout of lele_hip_frontend_compute_segments, so cmvn_apply_with_stats, the encoder's
 * forward_segments and the decode heads take it as it is.  R == 0 gives rank 0.  Everything is checked before anything is launched: a
 * range outside pcm, a length above max_chunk, a NULL argument or a call while the ctx records a graph (the counters advance on the
 * host, so a push cannot be replayed) fail and leave `out` AND the streams as they were.  Three or four launches a push over all
 * streams on the default framing (append, log-mel, emit, compact); other framings run the generic kernels once per stream. */
int lele_hip_frontend_stream_push(LeleFrontendStream* st, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths,
                                  const uint8_t* final_or_null, LeleBuf* out, int64_t* row_offsets, int64_t* out_shape, int32_t* out_rank);

/* ---- audio resampling: other sample rates in front of the front-end.  A LeleResampler converts from_rate -> to_rate in one of two
 * modes; its packed call and its live-stream form return f32 [N'] packed + out_offsets, which together with the offsets' differences
 * are the (pcm, starts, lengths) that lele_hip_frontend_compute_segments and lele_hip_frontend_stream_push take.
 *   LELE_RESAMPLE_LINEAR  the reference's `resample` (examples/web-demo/src/audio.rs:114-138) bit for bit: ratio = from as f64 / to as
 *     f64, output_len = (len as f64 / ratio) as usize, output i at src_pos = i as f64 * ratio between samples idx = floor(src_pos) and
 *     idx + 1 in f64 (two multiplies and an add, not contracted), the last sample as it is where idx + 1 == len, nothing where
 *     idx >= len (the result is then shorter than output_len; lele_hip_resampler_out_len gives the true length).  from == to copies.
 *   LELE_RESAMPLE_SINC    a Kaiser-windowed polyphase FIR: g = gcd(from, to), L = to / g, M = from / g; output i sits at input time
 *     i*M / L: base = (i*M) div L, phase = (i*M) mod L (64-bit integers); T = 2 * ceil(z / min(1, L/M)) taps a phase; tap t weighs input
 *     sample base - T/2 + 1 + t by w(d) = s sinc(s d) kaiser_beta(d / (T/2)) at d = (t - T/2 + 1) - phase/L, s = rolloff * min(1, L/M),
 *     each phase normalised to sum 1 in f64 and rounded to f32 (built on the host, uploaded at create).  The input is zero outside
 *     [0, len); output_len = ceil(len * L / M).  Accumulation: acc = fmaf(h[t], x[t], acc) in f32 for t = 0 .. T-1 in this order from
 *     +0 -- the order depends on T alone, never on the position in the buffer, the cut into chunks or the number of streams.
 * Routes (lele_hip_last_route): resample.copy, resample.linear, resample.fir1 (L == 1: coefficients by scalar loads), resample.fir.
 * A rate pair whose L * (T + 1) table and input tile exceed 160 KiB of LDS is refused at create. */
typedef enum { LELE_RESAMPLE_LINEAR = 0, LELE_RESAMPLE_SINC = 1 } LeleResampleMode;
typedef struct LeleResampler LeleResampler;
typedef struct LeleResamplerStream LeleResamplerStream;
/* z zero crossings a side (16), beta (8.6) and rolloff (0.9) shape the SINC table and are ignored by LINEAR.  ctx == NULL creates a
 * host-only object: lengths and the table, no GPU; it cannot resample.  Destroy it after its streams and before its ctx. */
int lele_hip_resampler_create(LeleCtx* ctx, int64_t from_rate, int64_t to_rate, int32_t mode, int32_t z, double beta, double rolloff,
                              LeleResampler** out);
int lele_hip_resampler_destroy(LeleResampler* rs);
/* The f32 table as uploaded, [L][T] (LINEAR and from == to: L = M = 1 ... and T = 0, no table); table may be NULL to ask for the sizes */
int lele_hip_resampler_table(const LeleResampler* rs, float* table, int64_t capacity, int64_t* l, int64_t* m, int64_t* taps);
/* Host arithmetic, nothing is launched: the outputs that become final when chunk_len samples follow samples_before, and the input
 * samples carried after that (0 after a final chunk).  samples_before = 0 with final = 1: the length of a whole utterance's result.
 * An output is final, LINEAR: once sample idx + 1 has arrived and i < output_len of what has arrived; the rest (the tail rule) with
 * `final`.  SINC: once its last tap's sample base + T/2 has arrived; with `final` the input is zero-extended. */
int lele_hip_resampler_out_len(const LeleResampler* rs, int64_t samples_before, int64_t chunk_len, int32_t final, int64_t* out_len,
                               int64_t* carry);
/* Segments of ONE pcm buffer (f32 [N], host or device), taken exactly as lele_hip_frontend_compute_segments takes them (any order,
 * overlaps, repeats, any 4-byte-aligned start), each resampled on its own in ONE launch.  out f32 [N'] packed, out_offsets
 * (count + 1, written on the host).  N' == 0 gives rank 0.  Everything is checked before anything is launched; a failing call leaves
 * out and out_offsets as they were.  The layout is shape metadata uploaded once per distinct layout, so a graph may record the call
 * (run the layout once before capturing it). */
int lele_hip_resample_segments(LeleResampler* rs, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths, int64_t count,
                               LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank);
/* `streams` live streams of at most max_chunk samples a push.  Per stream the device keeps the input samples the next output still
 * needs (LINEAR: at most ceil(ratio) + 2, SINC: fewer than T), in two halves that a push reads and writes in turn; the host keeps the
 * samples received and the absolute output index.  Concatenated per stream, the pushes are bit for bit lele_hip_resample_segments on
 * the whole utterance for any cut into chunks, zero-length chunks and a final push without audio included.  A final push resets the
 * stream.  reset / counters (samples received, outputs emitted, samples carried) / push mirror lele_hip_frontend_stream_*: one entry a
 * stream, everything checked before the one launch, a failing push leaves out and the streams as they were. */
int lele_hip_resampler_stream_create(LeleResampler* rs, int64_t streams, int64_t max_chunk, LeleResamplerStream** out);
int lele_hip_resampler_stream_destroy(LeleResamplerStream* st);
int lele_hip_resampler_stream_reset(LeleResamplerStream* st, const int64_t* ids, int64_t count);
int lele_hip_resampler_stream_counters(const LeleResamplerStream* st, int64_t id, int64_t* samples, int64_t* outputs, int64_t* carry);
int lele_hip_resampler_stream_push(LeleResamplerStream* st, const LeleTensor* pcm, const int64_t* starts, const int64_t* lengths,
                                   const uint8_t* final_or_null, LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank);

/* Lfr::compute, src/features/lfr.rs:18-54: [T, D] (or [1,T,D]) -> [ceil(T/n), D*m] */
int lele_hip_lfr(LeleCtx* ctx, const LeleTensor* x, int64_t m, int64_t n, LeleBuf* out, int64_t* out_shape,
                 int32_t* out_rank);
/* Cmvn::compute, src/features/cmvn.rs:14-66: per-utterance mean/var over time.  [T,D] or [1,T,D] as upstream; extension:
 * [B,T,D] with B > 1 normalises each of the B utterances with its own statistics in one launch pair */
int lele_hip_cmvn(LeleCtx* ctx, const LeleTensor* x, float eps, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* Cmvn::compute of every segment of a packed x [R, D] (row_offsets: host, count + 1, from 0 to R, non-decreasing): each segment
 * normalised with its own statistics, bit for bit what lele_hip_cmvn gives on that segment's rows alone; 0-row segments are
 * skipped.  out [R, D]. */
int lele_hip_cmvn_segments(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, float eps, LeleBuf* out,
                           int64_t* out_shape, int32_t* out_rank);
/* Packed x [R, D] -> out [count, t_max, D]: segment b's rows, then `pad` up to t_max (0 = the longest segment's rows; a smaller
 * non-zero t_max is an error).  An exact copy: the [B, T, D] + lengths form a padded encoder input takes. */
int lele_hip_segments_to_padded(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, int64_t t_max,
                                float pad, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* Cmvn::apply_with_stats, cmvn.rs:67-92 */
int lele_hip_cmvn_apply_with_stats(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* mean, const LeleTensor* std_,
                                   float eps, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* RealFft::process (features/fft.rs:18-43) / rfft_forward_f32_precomputed (kernels/fft.rs:51-77):
 * x [rows, n] real, n power of two -> re, im [rows, n/2+1] */
int lele_hip_rfft(LeleCtx* ctx, const LeleTensor* x, LeleBuf* out_re, LeleBuf* out_im, int64_t* out_shape,
                  int32_t* out_rank);
/* kernels::stft / stft_power_spectrum, src/kernels/math.rs:2304-2439; window may be NULL (periodic Hann).  signal: ONE signal, [L]
 * -> [frames, n_fft/2+1(, 2)] or [1, L] -> [1, frames, n_fft/2+1(, 2)].  Leading dimensions whose product exceeds 1 are an error
 * ("Data length mismatch"): upstream transforms the flattened data once, shapes the result [batch, ..] and panics there (tensor.rs:66). */
int lele_hip_stft(LeleCtx* ctx, const LeleTensor* signal, int64_t n_fft, int64_t hop_length, int64_t win_length,
                  const LeleTensor* window, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
int lele_hip_stft_power_spectrum(LeleCtx* ctx, const LeleTensor* signal, int64_t n_fft, int64_t hop_length,
                                 int64_t win_length, const LeleTensor* window, LeleBuf* out, int64_t* out_shape,
                                 int32_t* out_rank);

/* ---- src/kernels/gemm.rs ---------------------------------------------------------------------------- */
/* matmul, gemm.rs:112-222: [..,M,K] x [..,K,N]; B may be un-batched (batch_b == 1) else batches must match */
int lele_hip_matmul(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, LeleBuf* out, int64_t* out_shape,
                    int32_t* out_rank);
/* matmul_fused_add, gemm.rs:223-432: bias.len()==N -> per-column bias, else out[i] += bias[i % len] */
int lele_hip_matmul_fused_add(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, const LeleTensor* bias,
                              LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* gemm, gemm.rs:433-535: 2-D, out[M,N] = alpha*op(A)*op(B) + beta*C (C broadcast: full / [N] / [M] / scalar / modulo) */
int lele_hip_gemm(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, const LeleTensor* c_or_null, float alpha,
                  float beta, int trans_a, int trans_b, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* ---- src/kernels/quantization.rs --------------------------------------------------------------------- */
/* fused_quantized_linear, quantization.rs:77-169: DynamicQuantizeLinear (one range PER BATCH SLICE) + MatMulInteger
 * + scale + bias [+ ReLU].  weight_int8: u8 values carried as f32 [K,N]; weight_scale [1] or [N]; weight_zero [1];
 * bias [N] or empty/NULL.  Bit-exact with the reference's x86 path. */
int lele_hip_fused_quantized_linear(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                    const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                    const LeleTensor* bias_or_null, int apply_relu, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank);
/* dynamic_quantize_linear, quantization.rs:1628-1657: y (u8 values as f32, shape of x), scale [1], zero_point [1] */
int lele_hip_dynamic_quantize_linear(LeleCtx* ctx, const LeleTensor* x, LeleBuf* out_y, LeleBuf* out_scale,
                                     LeleBuf* out_zp, int64_t* out_shape, int32_t* out_rank);
/* mat_mul_integer / _with_bias / _with_scale_bias / _with_scale_bias_relu, quantization.rs:8-72, 927-992:
 * a, b hold u8 values as f32; zero points [1], scale [1] or [N], bias [N] -- each may be NULL */
int lele_hip_mat_mul_integer_with_scale_bias(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b,
                                             const LeleTensor* a_zero_point, const LeleTensor* b_zero_point,
                                             const LeleTensor* scale, const LeleTensor* bias, int apply_relu,
                                             LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* prepare_weights (quantization.rs:221) / PreparedWeights: a weight matrix given as RAW u8 bytes [K, N] (row-major), packed for
 * the i8 matrix cores once.  mat_mul_integer_prepared (quantization.rs:699): `a` holds u8 values as f32; zero points are host
 * scalars (has_* == 0 <=> None).  fused_dq_gemm_prepared (fused_dq_gemm_prepared_x86, quantization.rs:454): dynamic
 * quantisation per batch slice + prepared GEMM + scale + bias [+ ReLU] -- fused_quantized_linear on a prepared matrix.
 * mat_mul_integer_u8_weights (quantization.rs:173) is prepare_weights + mat_mul_integer_prepared; the shim keeps the handle. */
typedef struct LelePrepared LelePrepared;
int lele_hip_prepare_weights(LeleCtx* ctx, const uint8_t* b_u8, int64_t k, int64_t n, LelePrepared** out);
int lele_hip_prepared_destroy(LelePrepared* pw);
int lele_hip_mat_mul_integer_prepared(LeleCtx* ctx, const LeleTensor* a, const LelePrepared* pw, int has_a_zero_point,
                                      float a_zero_point, int has_b_zero_point, int32_t b_zero_point, const LeleTensor* scale,
                                      const LeleTensor* bias, int apply_relu, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
int lele_hip_fused_dq_gemm_prepared(LeleCtx* ctx, const LeleTensor* input, const LelePrepared* pw, int has_b_zero_point,
                                    int32_t b_zero_point, const LeleTensor* weight_scale, const LeleTensor* bias, int apply_relu,
                                    LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* per-stage stopwatch of fused_quantized_linear for bench.py's roofline block: while on, every EAGER call records HIP events on
 * the ctx stream between its stages (range pass | row quantisation | i8 GEMM; a stage a call skips reads 0); profile_read()
 * drains the stream and returns the average duration of each stage over the calls since the last read. */
int lele_hip_quant_set_profiling(LeleCtx* ctx, int on);
int lele_hip_quant_profile_read(LeleCtx* ctx, float* range_ms, float* quantise_ms, float* gemm_ms, int64_t* calls);

/* ---- src/kernels/math.rs: activations and element-wise ops ---------------------------------------------- */
/* Unary f32 ops.  LeleUnaryOp names the lele kernel it replaces (math.rs file:line in eltwise.hip). */
typedef enum {
    LELE_U_EXP = 0, LELE_U_SIGMOID = 1, LELE_U_TANH = 2, LELE_U_SILU = 3, LELE_U_ERF = 4, LELE_U_GELU = 5,
    LELE_U_FAST_GELU = 6, LELE_U_RELU = 7, LELE_U_SQRT = 8, LELE_U_LOG = 9, LELE_U_SIN = 10, LELE_U_COS = 11,
    LELE_U_NEG = 12, LELE_U_RECIPROCAL = 13, LELE_U_SOFTPLUS = 14, LELE_U_NOT = 15, LELE_U_ABS = 16,
    LELE_U_FLOOR = 17, LELE_U_CEIL = 18
} LeleUnaryOp;
int lele_hip_unary(LeleCtx* ctx, int op, const LeleTensor* x, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* Binary ops with numpy-style broadcasting (math.rs:69-264): add, sub, mul, div work on f32 and i64 */
typedef enum {
    LELE_B_ADD = 0, LELE_B_SUB = 1, LELE_B_MUL = 2, LELE_B_DIV = 3, LELE_B_POW = 4, LELE_B_MAX = 5, LELE_B_MIN = 6,
    LELE_B_EQUAL = 7, LELE_B_LESS = 8, LELE_B_GREATER = 9, LELE_B_PRELU = 10, LELE_B_MOD = 11, LELE_B_AND = 12,
    LELE_B_OR = 13
} LeleBinaryOp;
int lele_hip_binary(LeleCtx* ctx, int op, const LeleTensor* a, const LeleTensor* b, LeleBuf* out, int64_t* out_shape,
                    int32_t* out_rank);
/* the same op on SAME-SHAPE f32 operands that are channel views and / or with a channel-view result (LelePitch above: a residual
 * add whose operand is a Split result and whose result is a Concat operand; math.rs:414 on copies) */
int lele_hip_binary_pitched(LeleCtx* ctx, int op, const LeleTensor* a, const LeleTensor* b, const LelePitch* pitch, LeleBuf* out,
                            int64_t* out_shape, int32_t* out_rank);
/* where_op, manipulation.rs:1215: out = cond != 0 ? x : y */
int lele_hip_where(LeleCtx* ctx, const LeleTensor* cond, const LeleTensor* x, const LeleTensor* y, LeleBuf* out,
                   int64_t* out_shape, int32_t* out_rank);
/* clip, math.rs:1984-2010 */
int lele_hip_clip(LeleCtx* ctx, const LeleTensor* x, int has_min, float min_v, int has_max, float max_v, LeleBuf* out,
                  int64_t* out_shape, int32_t* out_rank);
/* reduce_sum / reduce_mean / reduce_max / reduce_l2 (/ min), math.rs:1527-1920 */
typedef enum { LELE_R_SUM = 0, LELE_R_MEAN = 1, LELE_R_MAX = 2, LELE_R_L2 = 3, LELE_R_MIN = 4 } LeleReduceOp;
int lele_hip_reduce(LeleCtx* ctx, int op, const LeleTensor* x, const int64_t* axes, size_t naxes, int keepdims,
                    LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* ---- src/kernels/norm.rs --------------------------------------------------------------------------------- */
int lele_hip_layer_norm(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* scale, const LeleTensor* bias,
                        int32_t axis, float epsilon, LeleBuf* out, int64_t* out_shape, int32_t* out_rank); /* norm.rs:226 */
int lele_hip_rms_norm(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* weight, int32_t axis, float epsilon,
                      LeleBuf* out, int64_t* out_shape, int32_t* out_rank);                                /* norm.rs:420 */
int lele_hip_softmax(LeleCtx* ctx, const LeleTensor* x, int32_t axis, LeleBuf* out, int64_t* out_shape,
                     int32_t* out_rank);                                                                    /* norm.rs:8 */
int lele_hip_batch_norm(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* scale, const LeleTensor* bias,
                        const LeleTensor* mean, const LeleTensor* var, float epsilon, LeleBuf* out, int64_t* out_shape,
                        int32_t* out_rank);                                                                  /* norm.rs:313 */

/* ---- src/kernels/manipulation.rs, shape.rs, conv2d.rs:1051-1502: data movement (bit-exact) ---------------- */
/* out[c] = x[offset + sum_k c_k*strides[k]] (c_k taken modulo mods[k] when mods && mods[k] > 0): the engine behind
 * slice (manipulation.rs:209), transpose (644), expand (math.rs:2168), tile (math.rs:2249), split (1091) */
int lele_hip_strided_copy(LeleCtx* ctx, const LeleTensor* x, const int64_t* out_dims, const int64_t* strides,
                          const int64_t* mods_or_null, int32_t rank, int64_t offset, LeleBuf* out, int64_t* out_shape,
                          int32_t* out_rank);
int lele_hip_concat(LeleCtx* ctx, const LeleTensor* const* inputs, size_t ninputs, int64_t axis, LeleBuf* out,
                    int64_t* out_shape, int32_t* out_rank);                                   /* manipulation.rs:108 */
/* pads = [begin_0..begin_{r-1}, end_0..end_{r-1}]; mode 0 constant, 1 edge, 2 reflect; fill_bits = raw element */
int lele_hip_pad(LeleCtx* ctx, const LeleTensor* x, const int64_t* pads, int32_t mode, uint64_t fill_bits,
                 LeleBuf* out, int64_t* out_shape, int32_t* out_rank);                        /* manipulation.rs:382 */
int lele_hip_gather(LeleCtx* ctx, const LeleTensor* data, const LeleTensor* indices, int64_t axis, LeleBuf* out,
                    int64_t* out_shape, int32_t* out_rank);                                   /* manipulation.rs:589 */
int lele_hip_gather_elements(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* indices, int64_t axis, LeleBuf* out,
                             int64_t* out_shape, int32_t* out_rank);                          /* conv2d.rs:1438 */
int lele_hip_resize_nearest(LeleCtx* ctx, const LeleTensor* x, int64_t out_h, int64_t out_w, int asymmetric,
                            LeleBuf* out, int64_t* out_shape, int32_t* out_rank);             /* conv2d.rs:1261 */
int lele_hip_max_pool2d(LeleCtx* ctx, const LeleTensor* x, const int64_t* kernel_shape, size_t nk,
                        const int64_t* strides, size_t ns, const int64_t* pads, size_t np, const int64_t* dilations,
                        size_t nd, int ceil_mode, LeleBuf* out, int64_t* out_shape, int32_t* out_rank); /* conv2d.rs:1051 */
/* resize_nearest / max_pool2d reading and / or writing channel views, and the plain copy between views (LelePitch above):
 * what concat (manipulation.rs:108) and split (manipulation.rs:1091) along C are when an operand cannot be produced in place */
int lele_hip_resize_nearest_pitched(LeleCtx* ctx, const LeleTensor* x, int64_t out_h, int64_t out_w, int asymmetric,
                                    const LelePitch* pitch, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
int lele_hip_max_pool2d_pitched(LeleCtx* ctx, const LeleTensor* x, const int64_t* kernel_shape, size_t nk, const int64_t* strides,
                                size_t ns, const int64_t* pads, size_t np, const int64_t* dilations, size_t nd, int ceil_mode,
                                const LelePitch* pitch, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
int lele_hip_copy_pitched(LeleCtx* ctx, const LeleTensor* x, const LelePitch* pitch, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* The transposing copy of a channel view: x [N, C, ...] (image pitch x_pitch) -> [N, P, C] (P = the product of the trailing
 * dimensions), dense or into the window (out_offset, out_pitch) of an already reserved buffer -- rows [p0, p0 + P) of a wider
 * [N, P_total, C] tensor are the window p0 * C, P_total * C.  lele's detection tails are Concat(levels, axis = 2) -> Transpose(0, 2, 1)
 * -> Split(heads, axis = 2) (examples/yolo26n-seg/src/yolo26seg.rs): three passes over the predictions, each a copy; the same
 * values arrive with one of these calls per (level, head) (lele_amd/plan.py, fold_transposed_splits). */
int lele_hip_transpose_cp_pitched(LeleCtx* ctx, const LeleTensor* x, const LelePitch* pitch, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* adaptive_avg_pool1d, pooling.rs:1-30: x [.., L] -> [.., output_len]; window i = [floor(i*L/O), ceil((i+1)*L/O)) */
int lele_hip_adaptive_avg_pool1d(LeleCtx* ctx, const LeleTensor* x, int64_t output_len, LeleBuf* out, int64_t* out_shape,
                                 int32_t* out_rank);
int lele_hip_topk(LeleCtx* ctx, const LeleTensor* x, int64_t k, int largest, LeleBuf* out_values, LeleBuf* out_indices,
                  int64_t* out_shape, int32_t* out_rank);                                     /* conv2d.rs:1385 */
int lele_hip_range_f32(LeleCtx* ctx, float start, float delta, int64_t n, LeleBuf* out, int64_t* out_shape,
                       int32_t* out_rank);                                                    /* math.rs:2033 */
int lele_hip_range_i64(LeleCtx* ctx, int64_t start, int64_t delta, int64_t n, LeleBuf* out, int64_t* out_shape,
                       int32_t* out_rank);                                                    /* math.rs:2057 */
int lele_hip_fill(LeleCtx* ctx, const int64_t* shape, int32_t rank, int32_t dtype, uint64_t bits, LeleBuf* out,
                  int64_t* out_shape, int32_t* out_rank);                                     /* shape.rs:122 */
int lele_hip_cast(LeleCtx* ctx, const LeleTensor* x, int32_t to_dtype, LeleBuf* out, int64_t* out_shape,
                  int32_t* out_rank);                                                         /* utils.rs:66-101 */

/* ---- src/kernels/conv2d.rs, conv1d.rs: convolutions (implicit GEMM on the f32 MFMA core) ------------------- */
/* conv2d (conv2d.rs:107), conv2d_fused (conv2d.rs:420: act = LELE_ACT_RELU), conv2d_silu (conv2d.rs:437:
 * act = LELE_ACT_SILU).  x [N,C,H,W], w [C_out,C_in/g,kH,kW], bias [C_out] or NULL.  dilations / strides hold 0, 1 or 2
 * values (one value is used for both axes), pads holds 0, 2 ([ph, pw]) or 4 ([top, left, bottom, right]) values.
 * The SiLU of the epilogue is x * rcp(1 + exp2(-x log2 e)) on the transcendental unit: within 1e-5 relative + 1e-7 of the reference's
 * (avx/math.rs polynomial body, libm tail) -- the sum under it is pinned to 1e-4 only.  LELE_HIP_CONV_SILU_EXACT=1 (read per call)
 * selects the replica of the reference's form instead. */
int lele_hip_conv2d(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* bias,
                    const int64_t* dilations, size_t ndil, int64_t group, const int64_t* pads, size_t npads,
                    const int64_t* strides, size_t nstr, int act, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* conv2d on channel views (LelePitch above; group == 1): x may be a Split result read in place, the result a Concat operand
 * written in place.  Same kernels, same arithmetic order as lele_hip_conv2d on dense copies: identical bits. */
int lele_hip_conv2d_pitched(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* bias,
                            const int64_t* dilations, size_t ndil, int64_t group, const int64_t* pads, size_t npads,
                            const int64_t* strides, size_t nstr, int act, const LelePitch* pitch, LeleBuf* out, int64_t* out_shape,
                            int32_t* out_rank);
/* conv2d followed by the Add of a residual block, in one call: out = act(conv(x) + bias) + res, res [N,C_out,H_out,W_out] f32.
 * lele's generated code issues conv2d_silu and then `add` (examples/yolo26n-seg/src/yolo26seg.rs: every bottleneck's
 * `x + cv2(cv1(x))`); the sum is formed from the same two f32 values, so the bits are those of the two calls.  `pitch` may be NULL;
 * with it, x / the result may be channel views as for lele_hip_conv2d_pitched and y_pitch is the residual's image pitch (0 = dense). */
int lele_hip_conv2d_res(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* bias, const LeleTensor* res,
                        const int64_t* dilations, size_t ndil, int64_t group, const int64_t* pads, size_t npads,
                        const int64_t* strides, size_t nstr, int act, const LelePitch* pitch, LeleBuf* out, int64_t* out_shape,
                        int32_t* out_rank);
/* reset_conv_stats / print_conv_stats (conv2d.rs:75, 101 -- no-ops upstream; examples/yolo26n-seg/src/main.rs:64,74 calls them):
 * 2-D convolutions issued on ctx since the last reset, as call count and multiply-accumulate count */
int lele_hip_conv_stats_reset(LeleCtx* ctx);
int lele_hip_conv_stats(LeleCtx* ctx, int64_t* calls, int64_t* macs);
/* The kernel route the most recent f32 GEMM, convolution or attention call on ctx dispatched (matmul, matmul_fused_add, gemm,
 * matmul_view, conv2d*, conv1d, conv_transpose, the f32 form of conv_integer, attention_view, attention_segments): its levels joined
 * by '/', e.g. "gemm.tile64x64", "conv.win3_oct32_osplit", "conv.gemm_tap/gemm.small" or "attn.rows16/attn.nt6" (the kernel, then its
 * key-tile class; "attn.flash" and the packed form's "attn.seg" have one level); "" when the result was empty.
 * The data-movement calls report theirs as well: the strided copy engine behind strided_copy and concat ("copy.w4", "copy.w8",
 * "copy.vec16", "copy.tile_w4", "copy.tile_w8", then "copy.i64" under 64-bit indexing; concat: its last launch), resize_nearest
 * ("resize.up2" / "up4" / "up8" / "resize.generic"), max_pool2d ("pool.lds" or "pool.lds_sep", then "pool.pb1" / "pool.pbn" for one or
 * several planes per workgroup; "pool.direct", "pool.direct_i64"), topk ("topk.rank", "topk.select_lds", "topk.select_l2"),
 * copy_pitched ("cpitch.w16" / "w4" / "w1"), and one fixed name each for pad, gather, gather_elements, adaptive_avg_pool1d,
 * transpose_cp_pitched, range_f32, range_i64, fill and cast ("pad.index", "gather.rows", "gather.elements", "apool.window",
 * "tcp.tile32", "range.f32", "range.i64", "fill.words", "cast.convert").
 * So do the element-wise, reduce and norm calls: unary ("unary.vec4", or "unary.w1" when a pointer is not 16-byte aligned), binary
 * ("bin.fast" for the float4 patterns, else "bin.flat_f32" / "bin.index_f32" / "bin.flat_i64" / "bin.index_i64": equal shapes or the index
 * walk; add3 with broadcasting operands: its second add), binary_pitched ("binp.vec4" / "binp.w1"), where ("where.index"), clip
 * ("clip.w1"), reduce ("reduce.seq", min / max over a contiguous last axis "reduce.rows16", few long rows "reduce.parts"), layer_norm and
 * softmax / softmax_scaled ("ln.reg8" / "reg16" / "reg32" and "softmax.reg8" / "reg16" / "reg32" by row length, then "rows.rpb2" / "rpb4" /
 * "rpb8" for the rows a block holds; "ln.stream", "softmax.stream" past 1024 elements), rms_norm ("rms.stream"), batch_norm ("bn.w1"),
 * add3 ("add3.vec4" / "add3.w1"), halves_pow_add_sqrt ("hpas.w1").  And the recurrent calls: lstm / gru ("rnn.lstm" / "rnn.gru", then
 * the GEMM kernel of W x: "gemm.thin_m", "gemm.small", a tile, "gemm.k0" for I = 0; nothing more for T = 0), lstm_segments / gru_segments
 * ("rnns.lstm" / "rnns.gru", then "rnns.reg16" / "reg32" / "reg64" for recurrent weights in registers or "rnns.stream1" / "stream2" /
 * "stream4" / "stream8" for the streamed form by the width of its members' register tile).  And the ConvInteger family on the i8 matrix
 * cores: conv_integer ("ci8.codes") and conv_integer_from_f32 / _multi ("ci8.quant": the image is quantised as it is packed), then the
 * kernel: "ci8.nj4" / "ci8.nj2" / "ci8.nj1" (a wave owns 4 / 2 / 1 strips of 32 positions) or "ci8.nj2_ksplit" / "ci8.nj1_ksplit" (the four
 * waves of a workgroup share the strips and split K); the f32 form reports "ci.f32", then the convolution's own route.
 * fused_scale_bias(_silu) reports "fsb.w1".  And the audio front-end (frontend_compute / _compute_batch / _logmel / _compute_segments): the
 * kernel -- "fe.main_std" / "fe.main_table" (400 / 160 / 512 framing: the unrolled 80-mel bank, or the table-driven mel loop of every other
 * n_mels), "fe.seg_std" / "fe.seg_table" (the same two for compute_segments), "fe.generic_fused" (every other framing, one kernel) or
 * "fe.generic_four" (its four-kernel form: batches beyond 65535 utterances) -- then for the main / seg kernels how the PCM tile was staged:
 * "fe.tile_dma" (direct-to-LDS: 16-byte aligned runs), "fe.tile_regs" (through registers), "fe.tile_mixed" (a segment launch that holds
 * both); "fe.two_kernel" instead for the lab form with the separate frame-sum kernel.  compute_segments on another framing reports its
 * last segment's route.  frontend_stream_push adds no name: its log-mel launch is the segment kernel's body over the streams' regions and
 * reports "fe.seg_std" / "fe.seg_table", then "fe.tile_dma" / "fe.tile_regs" / "fe.tile_mixed" by the same per-record condition (a region's carry +
 * chunk is a multiple of 4 samples); the generic names on another framing (the last stream's); "" when no stream gained a frame.
 * And the quantised linears: fused_quantized_linear[_residual[_ln]], sanm_out_block and fused_dq_gemm_prepared report "q.rs_fq" / "q.rs_frag"
 * (register-stationary, one level), "q.as" / "q.as_ln" / "q.as_ln_fsmn" then "as.two" / "as.tpw8" / "as.tpw4" (activation-stationary: all, 8 or 4
 * column tiles a workgroup), or "q.tiled" / "q.tiled_stream" (rows to i8 in memory by the prefetching / streaming row quantiser) then the tiled
 * GEMM: "igemm.big", "igemm.small_k4", "igemm.small_k16", "igemm.t128x128", "igemm.t32x128", "igemm.t128x64"; the decode heads "q.head" then
 * "igemm.head_ids" / "head_scored" / "head_topk" / "head_at"; the packed calls "q.seg" / "q.seg_stream" / "q.seg_head" then the same cores;
 * fused_ffn_quantized[_ln] "qffn.rs_one" / "qffn.rs_two" (the first product's two passes in one launch or two) then "rs.ks4" / "rs.ask_ln"
 * ("rs.ask": lab build), or "qffn.tiled" / "qffn.tiled_stream" then the tiled GEMM; mat_mul_integer* "mmi.rows" then the tiled GEMM (a batched
 * B: its last launch); dynamic_quantize_linear "dql.w1".  Where one of these issued the calls it stands for instead of a fused form (the two
 * linears of the feed-forward block, a residual that broadcasts, a LayerNorm or the three calls of sanm_out_block behind the linear), "q.calls"
 * stands in front of the (last) quantised linear's route: "q.calls/q.as/as.tpw8".
 * After a call that succeeded the route never names an earlier call; after one that returned an error it is undefined (an argument
 * check may fail before the route is cleared).  Recorded on the
 * host when the call is issued (a call recorded into a graph reports the route it recorded).  NUL-terminated into buf; an error when cap is too small.
 * lele_hip_route_names: every level name a route can hold, one per line; host only, no GPU needed. */
int lele_hip_last_route(LeleCtx* ctx, char* buf, size_t cap);
int lele_hip_route_names(char* buf, size_t cap);
/* conv1d (conv1d.rs:837) / conv1d_fused (conv1d.rs:1464: relu != 0).  x [N,C,L], w [C_out,C_in/g,K], pads [left,right] */
int lele_hip_conv1d(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* bias,
                    const int64_t* dilations, size_t ndil, int64_t group, const int64_t* pads, size_t npads,
                    const int64_t* strides, size_t nstr, int relu, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* conv_transpose (conv2d.rs:2952): x [N,C,H,W], w [C_in,C_out,kH,kW], group must be 1 (error otherwise, as upstream) */
int lele_hip_conv_transpose(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* bias,
                            const int64_t* dilations, size_t ndil, int64_t group, const int64_t* pads, size_t npads,
                            const int64_t* strides, size_t nstr, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* ---- src/kernels/rnn.rs: LSTM / GRU (batch 1, one direction; anything else is an error, as upstream panics) ---- */
/* lstm (rnn.rs:67): x [T,1,I], w [1,4H,I], r [1,4H,H], bias [1,8H] or NULL; gate order i,o,f,c.
 * out_y [T,1,1,H] (shape written to y_shape), out_h / out_c hold [1,1,H]. sequence_lens is ignored (as upstream). */
int lele_hip_lstm(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* r, const LeleTensor* bias,
                  const LeleTensor* sequence_lens, const LeleTensor* initial_h, const LeleTensor* initial_c,
                  LeleBuf* out_y, LeleBuf* out_h, LeleBuf* out_c, int64_t* y_shape, int32_t* y_rank);
/* gru (rnn.rs:246): w [1,3H,I], r [1,3H,H], bias [1,6H] or NULL; gate order z,r,h */
int lele_hip_gru(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* r, const LeleTensor* bias,
                 const LeleTensor* initial_h, int linear_before_reset, LeleBuf* out_y, LeleBuf* out_h, int64_t* y_shape,
                 int32_t* y_rank);

/* ---- ConvInteger family, src/kernels/conv2d.rs:1507-2761 ------------------------------------- */
/* conv_integer (conv2d.rs:2216): x, w hold u8 values as f32; zero points are host scalars ([1] or NULL = 0);
 * out = f32 conv2d(x - x_zp, w - w_zp) with zero padding, as the x86 path computes it */
int lele_hip_conv_integer(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* w, const LeleTensor* x_zero_point,
                          const LeleTensor* w_zero_point, const int64_t* dilations, size_t ndil, int64_t group,
                          const int64_t* pads, size_t npads, const int64_t* strides, size_t nstr, LeleBuf* out,
                          int64_t* out_shape, int32_t* out_rank);
/* conv_integer_from_f32 (conv2d.rs:2246; nsrc == 1) and conv_integer_from_f32_multi (conv2d.rs:2420; nsrc > 1, sources
 * concatenated along C, upstream always 1x1/s1/p0): DynamicQuantizeLinear over ALL sources, then conv_integer.
 * out_scale receives the quantisation scale ([1] f32, on the device -- upstream returns it as a host float) */
int lele_hip_conv_integer_from_f32(LeleCtx* ctx, const LeleTensor* const* sources, size_t nsrc, const LeleTensor* w,
                                   const LeleTensor* w_zero_point, const int64_t* dilations, size_t ndil, int64_t group,
                                   const int64_t* pads, size_t npads, const int64_t* strides, size_t nstr, LeleBuf* out,
                                   LeleBuf* out_scale, int64_t* out_shape, int32_t* out_rank);
/* fused_scale_bias / fused_scale_bias_silu (conv2d.rs:2636-2761): out = data * scale + bias[c] (then x / (1 + exp(-x)));
 * scale = scale_dev[0] * scale_mul (scale_dev may be NULL: scale = scale_mul) so that the scale produced by
 * conv_integer_from_f32 never has to visit the host.  Passing the buffer of `data` as `out` is the in-place form. */
int lele_hip_fused_scale_bias(LeleCtx* ctx, const LeleTensor* data, const LeleTensor* scale_dev_or_null, float scale_mul,
                              const LeleTensor* bias, int silu, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* ---- application-side pre/post-processing ----------------------------------------------------- */
/* examples/sensevoice/src/audio.rs:52-73: WAV payload bytes -> f32 mono.  16-bit: i16::from_le_bytes / 32768.0;
 * 8-bit: (b - 128) / 128; stereo: (l + r) / 2.  bytes: U8 [n].  out: f32 [frames] */
int lele_hip_wav_to_f32(LeleCtx* ctx, const LeleTensor* bytes, int32_t bits_per_sample, int32_t num_channels, LeleBuf* out,
                        int64_t* out_shape, int32_t* out_rank);
/* examples/sensevoice/src/tokenizer.rs:50-61: arg-max over the last axis; the LAST of equal maxima wins (Iterator::max_by;
 * +0.0 == -0.0).  A NaN loses to every number (upstream panics on one): the id is the last maximum among the row's non-NaN entries,
 * V - 1 for a row of nothing but NaN; rows without a NaN are unaffected.
 * x: f32 [.., V] -> i32 ids [..]; only the ids need to leave the device */
int lele_hip_argmax_last(LeleCtx* ctx, const LeleTensor* x, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* tokenizer.rs:63-71: the ids the greedy decoder keeps, in frame order -- an id is dropped when it is outside the vocabulary
 * or its skip flag is set (the host sets skip[0] and skip[id] for every "<|...|>" token once per vocabulary).  No CTC
 * collapsing (upstream does none).  ids: i32 [.., T]; skip: U8 [V]; out_ids: i32 [.., T] (kept ids first, then -1);
 * out_counts: i32 [..] */
int lele_hip_token_filter(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* skip, LeleBuf* out_ids, LeleBuf* out_counts,
                          int64_t* out_shape, int32_t* out_rank);
/* examples/yolo26n-seg/src/image.rs:62-111 (Image::preprocess): PIL-style nearest resize to target x target
 * (src = min(floor((dst + 0.5) * src_size / target), src_size - 1), f32 arithmetic), HWC u8 -> NCHW f32 / 255.
 * rgb: U8 [H, W, 3] -> out f32 [1, 3, target, target] */
int lele_hip_image_preprocess(LeleCtx* ctx, const LeleTensor* rgb, int32_t target, LeleBuf* out, int64_t* out_shape,
                              int32_t* out_rank);
/* image.rs:127-265 (postprocess_segmentation), per image of a batch.  logits: f32 [N, 300, 38] = box(4, 640-space) + score + class id
 * + 32 mask coefficients; mask_features: f32 [N, 32, Hm, Wm].  out_dets: f32 [N, 300, 38], the first out_count[n] rows of image n are
 * its kept detections in query order (box rescaled and clamped to the image, class id clamped to num_classes - 1), the rows behind
 * them zeros (fixed width: what the ranks of a sharded batch exchange, SURVEY.md 8e "C5");
 * out_count: i32 [N]; out_mask: U8 [N, img_height, img_width] (255 where a detection's mask covers the pixel).
 * The counts stay on the device: the call is graph-capturable. */
int lele_hip_yolo_seg_postprocess(LeleCtx* ctx, const LeleTensor* logits, const LeleTensor* mask_features, int32_t img_width,
                                  int32_t img_height, float threshold, int32_t num_classes, LeleBuf* out_dets,
                                  LeleBuf* out_count, LeleBuf* out_mask);
/* A queue of camera frames of different sizes, one call each way (image.rs:62-111 in, image.rs:127-265 out).
 *
 * lele_hip_image_preprocess_batch: image i is HWC RGB at bytes[offsets[i] .. offsets[i] + 3 heights[i] widths[i]) of ONE byte buffer
 * (bytes: U8 [total]); the offsets may come in any order, be unaligned, leave gaps and repeat.  offsets / heights / widths are HOST
 * arrays of `count` entries: shape metadata, held on the device as one table per distinct layout (like the row offsets of the
 * *_segments calls), so the call is graph-capturable once the layout has run eagerly once -- a replay reads whatever bytes the same
 * device buffer then holds.  out: f32 [count, 3, target, target]; image i of it is bit for bit lele_hip_image_preprocess of that image
 * alone (image.rs:84-105 + 69-79: src = min(floor((dst + 0.5f) * src_size / target), src_size - 1) in f32, then / 255).  One launch,
 * grid (pixel tiles, image).  Refused before anything is launched, `out` left as it was: a NULL argument, count < 0 or >= 65536,
 * target < 1 or > 16384, a side < 1 or >= 2^24, an image that does not lie inside the buffer (the message names the image).
 * count == 0: shape [0, 3, target, target], no launch. */
int lele_hip_image_preprocess_batch(LeleCtx* ctx, const LeleTensor* bytes, const int64_t* offsets, const int32_t* heights,
                                    const int32_t* widths, int64_t count, int32_t target, LeleBuf* out, int64_t* out_shape,
                                    int32_t* out_rank);
/* lele_hip_yolo_seg_postprocess_sized: lele_hip_yolo_seg_postprocess (image.rs:127-265) with a size of its own for every image of
 * the batch.  img_widths / img_heights: HOST arrays of count == N entries (shape metadata, one device table per distinct list of
 * sizes).  out_dets f32 [N, 300, 38] and out_count i32 [N] as above; out_mask: U8 [sum h_n w_n], image n's [h_n, w_n] mask at
 * mask_offsets[n] .. mask_offsets[n + 1] (mask_offsets: HOST out [N + 1], may be NULL).  out_mask may be NULL: detections only, no mask
 * work.  All three outputs of image n are EQUAL to what lele_hip_yolo_seg_postprocess leaves for that image alone at (w_n, h_n) --
 * whatever its neighbours and its place in the batch; like that call the mask grid is the reference's square one of side
 * S = floor(sqrt(Hm Wm)) over the first S S values of each of an image's 32 planes (image.rs:142-145).  Inputs are finite (a NaN in
 * logits: unspecified, as there).  The counts stay on the device: graph-capturable once the layout has run eagerly once.
 * The mask is not computed pixel by detection (image.rs:213-262) but from three bit tables of 10 words (300 detections) per entry,
 * each predicate of the reference evaluated once: per mask cell the detections whose sigmoid passes both thresholds there (evaluated
 * only inside the cells the box's pixels map to), per image column and per image row the detections whose box covers it; a pixel is set
 * iff the AND of its column's, its row's and its cell's words is non-zero.  Workspace, from the context's arena (its scratch block
 * where the arena is too small; no allocation after the first call of a size): exactly 40 * sum_n (S S + w_n + h_n) bytes.
 * Refused before launch: a NULL argument other than out_mask / mask_offsets, count != N, N >= 65536, a size < 1 or >= 2^24,
 * sum h_n w_n >= 2^31. */
int lele_hip_yolo_seg_postprocess_sized(LeleCtx* ctx, const LeleTensor* logits, const LeleTensor* mask_features,
                                        const int32_t* img_widths, const int32_t* img_heights, int64_t count, float threshold,
                                        int32_t num_classes, LeleBuf* out_dets, LeleBuf* out_count, LeleBuf* out_mask,
                                        int64_t* mask_offsets);

/* ---- multi-GPU: the one exchange step of the utterance-sharded recogniser ------------------------------ */
/* lele is single-process; its route to several devices is one instance per shard of the utterances (one process per GPU here).
 * Nothing is exchanged while computing; at the end ONE all-gather of the decoded token ids (i32) over RCCL / xGMI gives every
 * rank the transcripts of the whole batch.  RCCL is loaded on first use (dlopen): no link-time dependency.
 * The 128-byte unique id is made by rank 0 (comm_unique_id) and handed to the other ranks by the launcher; comm_init_file does
 * that through a file (rank 0 removes what is there and writes [32-byte job token][id] atomically, the others poll for up to
 * timeout_ms for a file carrying THEIR token).  The token is a digest of the environment variable LELE_JOB_ID (else
 * TORCHELASTIC_RUN_ID), which the launcher sets to a value unique to the launch: a file of an earlier job is never accepted.
 * Without a token the file carries an 8-byte beat that rank 0 keeps incrementing while it waits for the others (and removes the
 * file once all have joined): a reader accepts an id only after it has seen two different beats -- proof that the writer is alive,
 * whatever the ages and clocks involved.  comm_read_id_file is the reader's half on its own (no device, no RCCL). */
typedef struct LeleComm LeleComm;
int lele_hip_comm_unique_id(uint8_t* id128);
int lele_hip_comm_init(LeleCtx* ctx, const uint8_t* id128, int rank, int world, LeleComm** out);
int lele_hip_comm_init_file(LeleCtx* ctx, const char* path, int rank, int world, int timeout_ms, LeleComm** out);
int lele_hip_comm_read_id_file(const char* path, int timeout_ms, uint8_t* id128);
int lele_hip_comm_rank(const LeleComm* comm, int* rank, int* world);
/* send: DEVICE i32 tensor of the same element count on every rank -> out [world, count] in rank order, on the ctx stream
 * (graph-capturable; the result is ordered after everything queued before it, e.g. lele_hip_token_filter) */
int lele_hip_comm_allgather_i32(LeleComm* comm, const LeleTensor* send, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* the same for a DEVICE tensor of any element type (configs[4]: every rank's fixed-width detection rows, f32 [images, 300, 38], and their
 * i32 counts -- the (logits, mask_features) pair of examples/yolo26n-seg/src/yolo26seg.rs:706-716 after lele_hip_yolo_seg_postprocess):
 * out [world, ...send's shape] in rank order, moved as bytes */
int lele_hip_comm_allgather(LeleComm* comm, const LeleTensor* send, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* MAX over ranks of a host scalar, in place (row width of ragged shards, a wall time in ns); synchronises the ctx stream */
int lele_hip_comm_allreduce_max_i64(LeleComm* comm, int64_t* value);
int lele_hip_comm_barrier(LeleComm* comm); /* every rank's ctx stream has drained when any rank returns */
int lele_hip_comm_destroy(LeleComm* comm);

/* ---- fused forms beyond the reference's own patterns (emitted by lele_amd.compiler, each bit-identical to the sequence it
 *      replaces; never required by lele-generated code) ---------------------------------------------------------------- */
/* fused_quantized_linear followed by one or two Adds of same-shape tensors, folded into the GEMM's store:
 * ((linear(x) + res1) + res2), each sum rounded as the separate `add`s would (res2 may be NULL) */
int lele_hip_fused_quantized_linear_residual(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                             const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias,
                                             int apply_relu, const LeleTensor* res1, const LeleTensor* res2, LeleBuf* out,
                                             int64_t* out_shape, int32_t* out_rank);
/* the same followed by the LayerNorm over the last axis that reads the sum (src/kernels/norm.rs:226 -> avx/norm.rs:10-133):
 *   out = fused_quantized_linear[_residual](input, W.., apply_relu, res1, res2);  ln_out = layer_norm(out, ln_scale, ln_bias, -1, epsilon)
 * bit for bit the two calls (res1 / res2 may be NULL).  With K = 512 and N = 512 over a batch a workgroup of the GEMM holds whole
 * rows of the result and normalises them in its epilogue: one launch and one read of the sum less per transformer half-layer. */
int lele_hip_fused_quantized_linear_residual_ln(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                                const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias,
                                                int apply_relu, const LeleTensor* res1, const LeleTensor* res2, const LeleTensor* ln_scale,
                                                const LeleTensor* ln_bias, float epsilon, LeleBuf* out, LeleBuf* ln_out, int64_t* out_shape,
                                                int32_t* out_rank);
/* the output half of a SAN-M attention block (SenseVoice's encoder layer; an FSMN memory block beside the attention) as one call:
 *   mem = depthwise_conv1d_tlc(v_src, x_offset, fsmn_w, fsmn_bias, pad_left, pad_right, relu = 0, add_input = 1)
 *   out = fused_quantized_linear_residual(input, W.., apply_relu, mem, res2);  ln_out = layer_norm(out, ln_scale, ln_bias, -1, epsilon)
 * (conv1d.rs:837 between two transposes + an Add, quantization.rs:77, two Adds, norm.rs:226) bit for bit those three calls; res2 and
 * fsmn_bias may be NULL.  With K = N = 512 over a batch the GEMM's workgroup computes the memory block of its 32 rows from a window of
 * v staged in LDS and normalises the rows in its epilogue -- three launches become one; other shapes issue the three calls. */
int lele_hip_sanm_out_block(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                            const LeleTensor* weight_zero, const LeleTensor* bias, int apply_relu, const LeleTensor* v_src,
                            const LeleTensor* fsmn_w, const LeleTensor* fsmn_bias, int64_t x_offset, int64_t pad_left, int64_t pad_right,
                            const LeleTensor* res2, const LeleTensor* ln_scale, const LeleTensor* ln_bias, float epsilon, LeleBuf* out,
                            LeleBuf* ln_out, int64_t* out_shape, int32_t* out_rank);
/* two quantised linears with a ReLU between them (a transformer layer's feed-forward block):
 *   fused_quantized_linear[_residual](fused_quantized_linear(input, w1.., apply_relu = 1), w2.., apply_relu2, res1, res2)
 * (quantization.rs:77-169 twice; res1 / res2 may be NULL).  When the hidden layer is large its f32 tensor is never stored: the first
 * product runs twice on the matrix cores (once for the range, once quantising straight to the i8 rows the second product reads) */
int lele_hip_fused_ffn_quantized(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* w1_int8, const LeleTensor* w1_scale,
                                 const LeleTensor* w1_zero, const LeleTensor* b1, const LeleTensor* w2_int8,
                                 const LeleTensor* w2_scale, const LeleTensor* w2_zero, const LeleTensor* b2, int apply_relu2,
                                 const LeleTensor* res1, const LeleTensor* res2, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* the same followed by the LayerNorm over the last axis that reads the result (the NEXT half-layer's LayerNorm in a transformer stack):
 *   out = fused_ffn_quantized(...);  ln_out = layer_norm(out, ln_scale, ln_bias, -1, epsilon)
 * bit for bit the two calls.  With 2048 hidden and 512 output columns over a batch the second product runs one 32-row tile a workgroup
 * with all columns (weights streamed from L2) and normalises its rows in the epilogue: the LayerNorm launch and one round trip of the sum go. */
int lele_hip_fused_ffn_quantized_ln(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* w1_int8, const LeleTensor* w1_scale,
                                    const LeleTensor* w1_zero, const LeleTensor* b1, const LeleTensor* w2_int8, const LeleTensor* w2_scale,
                                    const LeleTensor* w2_zero, const LeleTensor* b2, int apply_relu2, const LeleTensor* res1,
                                    const LeleTensor* res2, const LeleTensor* ln_scale, const LeleTensor* ln_bias, float epsilon, LeleBuf* out,
                                    LeleBuf* ln_out, int64_t* out_shape, int32_t* out_rank);
/* softmax(x * scale[0]) over the last axis: `mul` by a one-element tensor followed by `softmax` (norm.rs:8) */
int lele_hip_softmax_scaled(LeleCtx* ctx, const LeleTensor* x, const LeleTensor* scale, int32_t axis, LeleBuf* out,
                            int64_t* out_shape, int32_t* out_rank);
/* sqrt(pow(x[.., lo_start:lo_end, ..], exp_lo) + pow(x[.., hi_start:hi_end, ..], exp_hi)) along `axis` (bounds as Slice's: negative
 * from the end, clamped; the two ranges must be equally long): `slice`, `pow`, `slice`, `pow`, `add`, `sqrt` (manipulation.rs:209,
 * math.rs:1481, 414, 1460) in one pass -- the magnitude of a spectrum stored as [re | im] channel halves (Silero's
 * STFT-as-convolution).  exp_lo / exp_hi are one-element host constants. */
int lele_hip_halves_pow_add_sqrt(LeleCtx* ctx, const LeleTensor* x, int32_t axis, int64_t lo_start, int64_t lo_end, int64_t hi_start,
                                 int64_t hi_end, const LeleTensor* exp_lo, const LeleTensor* exp_hi, LeleBuf* out, int64_t* out_shape,
                                 int32_t* out_rank);
/* (a + b) + c on equal shapes: two consecutive `add`s (math.rs:414) */
int lele_hip_add3(LeleCtx* ctx, const LeleTensor* a, const LeleTensor* b, const LeleTensor* c, LeleBuf* out, int64_t* out_shape,
                  int32_t* out_rank);
/* Transpose(0,2,1) -> depthwise conv1d (group = C, stride 1, dilation 1, conv1d.rs:837) -> Transpose(0,2,1), without the
 * transposes.  x f32 [B, T, P]: the C = w.shape[0] channels [x_offset, x_offset + C) of the last dimension are convolved
 * along T (x_offset = 0 and P = C for a plain [B, T, C] tensor; a non-zero offset reads one part of a packed projection in
 * place); w [C, 1, K] (K in 3, 5, 7, 11), bias [C] or NULL -> out [B, T + pad_left + pad_right - K + 1, C].
 * add_input: out += the convolved input itself (the FSMN "memory + input" Add that follows; needs equal lengths). */
int lele_hip_depthwise_conv1d_tlc(LeleCtx* ctx, const LeleTensor* x, int64_t x_offset, const LeleTensor* w, const LeleTensor* bias,
                                  int64_t pad_left, int64_t pad_right, int relu, int add_input, LeleBuf* out, int64_t* out_shape,
                                  int32_t* out_rank);
/* Batched matmul whose operands and result are STRIDED VIEWS (heads inside a packed [B, T, 3*D] projection; the result
 * stored straight into the [B, T, H, Dh] layout): the same MFMA kernels and tile choice as lele_hip_matmul, so the values
 * are bit-identical to copying the views out (slice / reshape / transpose) and calling matmul.  Element (bo, bi, r, c) of a
 * view lives at data[offset + bo*stride_outer + bi*stride_inner + r*stride_row + c*stride_col] (in elements); A is [m, k],
 * B is [k, n], the result [m, n]; A and B need unit stride along one of their two dimensions, the result along n.
 * out_dims is the shape reported for `out` (batch_outer*batch_inner*m*n elements). */
typedef struct LeleMatView {
    int64_t offset, stride_outer, stride_inner, stride_row, stride_col;
} LeleMatView;
int lele_hip_matmul_view(LeleCtx* ctx, const LeleTensor* a, const LeleMatView* a_view, const LeleTensor* b, const LeleMatView* b_view,
                         int64_t batch_outer, int64_t batch_inner, int64_t m, int64_t k, int64_t n, const LeleMatView* out_view,
                         const int64_t* out_dims, int32_t out_dims_rank, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* softmax(Q K^T * scale) V in one launch: lele_hip_matmul_view(Q view, K^T view) -> lele_hip_softmax_scaled ->
 * lele_hip_matmul_view(P, V view, out view), with the [.., T, T] score and probability tensors kept on chip.  Views as in
 * lele_hip_matmul_view: q is [t_q, dh], k is the B operand of the first product, i.e. K TRANSPOSED [dh, t_k], v is [t_k, dh],
 * the result [t_q, dh].  scale: one f32 value or NULL.  Same arithmetic as the sequence (f32 MFMA with the tiled GEMM's k order,
 * the row softmax of norm.rs:8), so batched results carry the sequence's bits.  Supported: dh == 128, t_k <= 512, unit stride
 * along dh for q / k / v / out, 16-byte aligned q / k rows -- anything else returns an error and the caller issues the sequence. */
int lele_hip_attention_view(LeleCtx* ctx, const LeleTensor* q, const LeleMatView* q_view, const LeleTensor* k, const LeleMatView* k_view,
                            const LeleTensor* v, const LeleMatView* v_view, int64_t batch_outer, int64_t batch_inner, int64_t t_q,
                            int64_t t_k, int64_t dh, const LeleTensor* scale_or_null, const LeleMatView* out_view,
                            const int64_t* out_dims, int32_t out_dims_rank, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);

/* ---- The packed batch behind the front-end: x [R, D] + row_offsets (host, count + 1 values from 0 to R, non-decreasing, checked
 * before anything is launched: a failing call leaves `out` as it was), the layout lele_hip_frontend_compute_segments and
 * lele_hip_cmvn_segments produce.  Every segment is computed exactly as if it ran alone -- the reference is batch 1 throughout
 * (examples/sensevoice/src/main.rs) -- and 0-row segments are skipped.  A layout's device tables are uploaded once and never rewritten,
 * so a graph may record these calls after the layout has run once.  Row-wise operators (layer_norm, add, add3) take [R, D] as it is. */

/* fused_quantized_linear (quantization.rs:77-169) with every segment as a batch slice of its own (quantization.rs:104-128: one dynamic
 * range per slice): rows of segment i are, bit for bit, lele_hip_fused_quantized_linear of input[off[i]:off[i+1]] alone as a rank-2
 * tensor.  input f32 [R, K] -> out [R, N].  Producer-side row statistics of `input` are not read. */
int lele_hip_fused_quantized_linear_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                             const LeleTensor* weight_int8, const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                             const LeleTensor* bias_or_null, int apply_relu, LeleBuf* out, int64_t* out_shape,
                                             int32_t* out_rank);
/* The greedy decode head (examples/sensevoice/src/tokenizer.rs:50-71 behind quantization.rs:77-169): out_ids = i32, the input's shape
 * without its last axis, bit for bit lele_hip_argmax_last(lele_hip_fused_quantized_linear(input, .., apply_relu = 0)) -- one dynamic
 * range per batch slice, the same result elements, of equal maxima the LAST index wins, +0.0 and -0.0 compare equal (partial_cmp).  The
 * arg-max is taken inside the GEMM's epilogue: the logits [rows, N] are never stored and no buffer of rows x N elements is reserved.
 * A row whose logits hold a NaN has an unspecified id (the reference panics there: tokenizer.rs:56, partial_cmp(..).unwrap()).
 * rows == 0 gives an empty result of the right shape; K == 0 or N == 0 is an error.  Everything is checked before anything is launched
 * or resized; graph-capturable after one eager run of the same shape. */
int lele_hip_fused_quantized_linear_argmax(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                           const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias_or_null,
                                           LeleBuf* out_ids, int64_t* out_shape, int32_t* out_rank);
/* ... of a packed batch (tokenizer.rs:50-71, quantization.rs:77-169): input f32 [R, K] -> out_ids i32 [R]; every segment is a slice of
 * its own exactly as in lele_hip_fused_quantized_linear_segments (the same offset checks, layout table and per-segment range pass), so
 * segment i's ids are bit for bit lele_hip_fused_quantized_linear_argmax of input[off[i]:off[i+1]] alone.  0-row segments are skipped.
 * NaN rows as above.  Graph-capturable after one eager run of the same layout. */
int lele_hip_fused_quantized_linear_argmax_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                    const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                    const LeleTensor* weight_zero, const LeleTensor* bias_or_null, LeleBuf* out_ids,
                                                    int64_t* out_shape, int32_t* out_rank);
/* lele_hip_token_filter per segment of packed ids (tokenizer.rs:50-71 after quantization.rs:77-169 produced them): ids i32 [R],
 * row_offsets host [count + 1] from 0 to R, skip U8 [V] -> out_ids i32 [count, W], out_counts i32 [count].  Row i holds the kept ids of
 * segment i in frame order, then -1: lele_hip_token_filter on that segment's ids alone, padded with -1 to W (ids outside [0, V) are
 * dropped).  W = width; width == 0 means the longest segment's row count, at least 1.  A non-zero width smaller than a segment is an
 * error that names the segment.  Everything is checked before anything is launched or resized; the [count, W] ids + counts are the
 * form the ranks of a sharded batch exchange.  Graph-capturable after one eager run of the same layout. */
int lele_hip_token_filter_segments(LeleCtx* ctx, const LeleTensor* ids, const int64_t* row_offsets, int64_t count, const LeleTensor* skip,
                                   int64_t width, LeleBuf* out_ids, LeleBuf* out_counts, int64_t* out_shape, int32_t* out_rank);
/* The greedy decode head with the winner's confidence (examples/sensevoice/src/tokenizer.rs:50-71 behind quantization.rs:77-169):
 * out_ids as lele_hip_fused_quantized_linear_argmax, bit for bit; out_logprob = f32 of the same shape, the log of the winner's soft-max
 * posterior, logprob = -ln sum_j exp(v_j - v_id) over the row's N logits v (the result elements of lele_hip_fused_quantized_linear,
 * apply_relu = 0), in [-ln N, 0]; N == 1 gives exactly 0.0.  It is formed from differences to the maximum inside the GEMM's epilogue,
 * never as v_id - (max + ln sum): within 1e-5 of the float64 value of that formula for any offset of the logits.  The logits are never
 * stored.  A row holding a NaN or +-inf logit has an unspecified score, as its id.  The two buffers must be distinct.  rows == 0 gives
 * empty results of the right shape; K == 0 or N == 0 is an error.  Everything is checked before anything is launched or resized;
 * graph-capturable after one eager run of the same shape. */
int lele_hip_fused_quantized_linear_argmax_logprob(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                                   const LeleTensor* weight_scale, const LeleTensor* weight_zero,
                                                   const LeleTensor* bias_or_null, LeleBuf* out_ids, LeleBuf* out_logprob, int64_t* out_shape,
                                                   int32_t* out_rank);
/* ... of a packed batch (tokenizer.rs:50-71, quantization.rs:77-169): input f32 [R, K] -> out_ids i32 [R], out_logprob f32 [R]; the
 * checks, layout table and per-segment range pass of lele_hip_fused_quantized_linear_argmax_segments, so segment i's ids and scores are
 * bit for bit lele_hip_fused_quantized_linear_argmax_logprob of input[off[i]:off[i+1]] alone.  0-row segments are skipped.  Graph-capturable
 * after one eager run of the same layout. */
int lele_hip_fused_quantized_linear_argmax_logprob_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                            const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                            const LeleTensor* weight_zero, const LeleTensor* bias_or_null, LeleBuf* out_ids,
                                                            LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank);
/* The decode head with the k best tokens a frame (tokenizer.rs:50-61 continued past the winner, behind quantization.rs:77-169), for CTC
 * prefix beam search, n-best lists and rescoring: 1 <= k <= 8, out_ids i32 of the input's shape without its last axis plus a trailing
 * axis of k, out_logprob f32 of the same shape.  Slot j of a row holds the column of its (j + 1)-th greatest logit v (the result elements
 * of lele_hip_fused_quantized_linear, apply_relu = 0): the greater value first, of equal values the GREATER COLUMN FIRST, +0.0 and -0.0
 * equal -- the order the arg-max head breaks ties in, NOT the stable lowest-index-first order of lele_hip_topk (conv2d.rs:1385-1435).
 * Slot 0 is lele_hip_fused_quantized_linear_argmax_logprob bit for bit, id and score; out_logprob[.., j] = (v_j - v_0) + logprob_0 in
 * f32; slots j >= N hold id -1 and -inf.  The logits are never stored and no buffer of rows x N elements is reserved: the workspace is
 * rows * ceil(N / 128) * (8 k + 4) bytes, k keys and one sum per (row, 128-column tile).  No atomics, nothing depends on workgroup
 * order.  A row holding a NaN or +-inf logit is unspecified.  The two buffers must be distinct.  rows == 0 gives empty results of the
 * right shape; K == 0, N == 0 or k outside [1, 8] is an error.  Everything is checked before anything is launched or resized;
 * graph-capturable after one eager run of the same shape. */
int lele_hip_fused_quantized_linear_topk(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                         const LeleTensor* weight_zero, const LeleTensor* bias_or_null, int32_t k, LeleBuf* out_ids,
                                         LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank);
/* ... of a packed batch: input f32 [R, K] -> out_ids i32 [R, k], out_logprob f32 [R, k]; the checks, layout table and per-segment range
 * pass of lele_hip_fused_quantized_linear_argmax_segments, so segment i's rows are bit for bit lele_hip_fused_quantized_linear_topk of
 * input[off[i]:off[i+1]] alone.  0-row segments are skipped.  Graph-capturable after one eager run of the same layout. */
int lele_hip_fused_quantized_linear_topk_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                  const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                  const LeleTensor* weight_zero, const LeleTensor* bias_or_null, int32_t k, LeleBuf* out_ids,
                                                  LeleBuf* out_logprob, int64_t* out_shape, int32_t* out_rank);
/* lele_hip_token_filter_segments with each kept token's frame and score (tokenizer.rs:50-71 after quantization.rs:77-169 produced the
 * ids): ids i32 [R], logprob_or_null f32 [R], row_offsets host [count + 1] from 0 to R, skip U8 [V] -> out_ids i32 [count, W] and
 * out_counts i32 [count], identical to lele_hip_token_filter_segments for the same arguments; out_frames i32 [count, W]: for each kept
 * id its row index within its segment (row - off[i]), then -1; out_logprob f32 [count, W]: the input score at that frame, copied bit for
 * bit, then 0.0 -- left untouched, and may be NULL, when logprob_or_null is NULL.  The width rule and its error (which names the
 * segment) are lele_hip_token_filter_segments'.  A dense [B, T] batch is the packed layout with off[i] = i * T (ids flattened to
 * [B * T]): there is no dense twin.  Everything is checked before anything is launched or resized; count == 0 and R == 0 give empty
 * results of the right shape.  Graph-capturable after one eager run of the same layout. */
int lele_hip_token_align_segments(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* logprob_or_null, const int64_t* row_offsets,
                                  int64_t count, const LeleTensor* skip, int64_t width, LeleBuf* out_ids, LeleBuf* out_frames,
                                  LeleBuf* out_logprob, LeleBuf* out_counts, int64_t* out_shape, int32_t* out_rank);
/* CTC prefix beam search over the k best candidates of every frame, per segment of a packed batch (the consumer of
 * lele_hip_fused_quantized_linear_topk_segments): ids i32 [R, k], logprob f32 [R, k], 1 <= k <= 8, row_offsets host [count + 1] from 0 to
 * R.  Segment i's frames are rows off[i] + skip_rows .. off[i + 1] (none when it has at most skip_rows rows; SenseVoice: 4 prompt rows).
 * 1 <= beam <= 8 prefixes survive a frame, 1 <= nbest <= beam are reported, best first: out_tokens i32 [count, nbest, W] (the reported
 * shape): the label sequence, then -1; out_lengths i32 [count, nbest]; out_scores f32 [count, nbest]: the log of the summed probability
 * of the alignments that collapse to the sequence, accumulated and ordered in float64 and rounded once; out_counts i32 [count]: the
 * hypotheses the segment has (<= nbest; a segment without frames has one, empty, score +0.0; slots past it hold -1 / 0 / -inf).  A
 * candidate with id < 0 is skipped; equal totals are ordered as tuples of labels compare (element by element, of a sequence and its
 * extension the shorter first); ids are labels only, nothing is indexed by one.  The ids of a frame must be distinct; with duplicates, or with
 * NaN / +inf scores, the result is unspecified but the call terminates and stays inside its buffers (entries are ordered strictly,
 * by total, tuple and entry index; a NaN total ranks as -inf).  W = width, or with width == 0 the most frames of any segment (at least 1); a segment
 * with more frames than a given width is an error that names it.  The four buffers must be distinct.  Workspace: the prefix trie, 8 * (1 +
 * beam * most frames) bytes a segment -- in LDS while that is at most 56 KiB (895 frames at beam 8), beyond it count times as much of the
 * context's scratch block.  A dense [B, T, k] batch is the packed layout with off[i] = i * T: there is
 * no dense twin.  Everything is checked before anything is launched or resized; count == 0 and R == 0 give empty results of the right
 * shape.  Graph-capturable after one eager run of the same layout. */
int lele_hip_ctc_beam_search_segments(LeleCtx* ctx, const LeleTensor* ids, const LeleTensor* logprob, const int64_t* row_offsets,
                                      int64_t count, int64_t skip_rows, int32_t blank, int32_t beam, int32_t nbest, int64_t width,
                                      LeleBuf* out_tokens, LeleBuf* out_lengths, LeleBuf* out_scores, LeleBuf* out_counts,
                                      int64_t* out_shape, int32_t* out_rank);
/* The decode head with the log-probabilities of the columns the CALLER names (tokenizer.rs:50-71 behind quantization.rs:77-169), for
 * forced alignment of a known transcript and for rescoring under the full-vocabulary posterior.  cols is a HOST array of ncols columns,
 * strictly ascending, every one in [0, N), 1 <= ncols <= N; an error names the offending index.  out_ids and out_logprob are
 * lele_hip_fused_quantized_linear_argmax_logprob bit for bit (the reported shape is theirs): one call serves greedy decoding and
 * alignment.  out_at is f32 of that shape plus a trailing axis of ncols: out_at[r, u] = (v[r, cols[u]] - v[r, id_r]) + logprob[r] in
 * f32, v the result elements of lele_hip_fused_quantized_linear (apply_relu = 0).  That is the formula of slot j of
 * lele_hip_fused_quantized_linear_topk, so a listed column that is among a row's k best holds the k-best head's log-probability bit for
 * bit, and the arg-max column holds logprob[r] itself; against the float64 log-soft-max it is within 1.1e-5 + 2^-23 |value| (the scored
 * head's 1e-5, then two f32 roundings).  The logits are never stored and no buffer of rows x N elements is reserved: the workspace is
 * the scored head's, rows * ceil(N / 128) * 12 bytes, plus the column -> slot map, 4 N bytes, in the call's layout table.  No atomics,
 * nothing depends on workgroup order.  A row holding a NaN or +-inf logit is unspecified.  The three buffers must be distinct.  rows ==
 * 0 gives empty results of the right shape; K == 0 or N == 0 is an error.  Everything, the columns included, is checked before anything
 * is launched or resized; graph-capturable after one eager run of the same shape AND the same columns (the table is keyed by them). */
int lele_hip_fused_quantized_linear_logprob_at(LeleCtx* ctx, const LeleTensor* input, const LeleTensor* weight_int8,
                                               const LeleTensor* weight_scale, const LeleTensor* weight_zero, const LeleTensor* bias_or_null,
                                               const int32_t* cols, int64_t ncols, LeleBuf* out_ids, LeleBuf* out_logprob, LeleBuf* out_at,
                                               int64_t* out_shape, int32_t* out_rank);
/* ... of a packed batch: input f32 [R, K] -> out_ids i32 [R], out_logprob f32 [R], out_at f32 [R, ncols]; the checks and per-segment
 * range pass of lele_hip_fused_quantized_linear_argmax_segments, so segment i's rows are bit for bit
 * lele_hip_fused_quantized_linear_logprob_at of input[off[i]:off[i+1]] alone.  The call's ONE layout table holds the offsets, the row ->
 * segment map and the column -> slot map (8 (count + 1) + 4 R + 4 N bytes), keyed by the layout and the columns.  0-row segments are
 * skipped.  Graph-capturable after one eager run of the same layout and the same columns. */
int lele_hip_fused_quantized_linear_logprob_at_segments(LeleCtx* ctx, const LeleTensor* input, const int64_t* row_offsets, int64_t count,
                                                        const LeleTensor* weight_int8, const LeleTensor* weight_scale,
                                                        const LeleTensor* weight_zero, const LeleTensor* bias_or_null, const int32_t* cols,
                                                        int64_t ncols, LeleBuf* out_ids, LeleBuf* out_logprob, LeleBuf* out_at,
                                                        int64_t* out_shape, int32_t* out_rank);
/* CTC forced alignment of a known transcript per segment of a packed batch (the consumer of
 * lele_hip_fused_quantized_linear_logprob_at_segments; lele_amd.apps.ctc_forced_align is the host reference): at f32 [R, U] holds the
 * log-probabilities of the U = ncols columns cols (host, strictly ascending), row_offsets host [count + 1] from 0 to R.  Segment i's
 * frames are rows off[i] + skip_rows .. off[i + 1] (none when it has at most skip_rows rows), its transcript the L_i labels
 * tokens[token_offsets[i] : token_offsets[i + 1]] (host; token_offsets [count + 1] from 0).  Every label and `blank` must be listed in
 * cols, no label may be the blank, L_i <= 511 (1023 lattice states, 16 a lane of the wavefront): an error names the segment and the
 * position.  W = width, or with width == 0 the longest transcript, at least 1; a transcript longer than a given width is an error that
 * names the segment.
 * The lattice has states s = 0 .. 2 L, even = blank, odd = label (s - 1) / 2.  Viterbi, exactly: alpha_0(0) = e_0(blank), alpha_0(1) =
 * e_0(label 0), the rest -inf; alpha_t(s) = best + (double)e_t(s), best over alpha_{t-1}(s), alpha_{t-1}(s - 1) and -- for an odd s whose
 * label differs from the one before it -- alpha_{t-1}(s - 2), a later candidate replacing an earlier one only if strictly greater (stay
 * wins over step, step over skip); the end is state 2 L unless alpha(2 L - 1) is strictly greater.  All in float64, one addition a
 * frame: the path score is the float64 sum in frame order of the path's f32 emissions, and the results EQUAL the host function's.
 * -> out_spans i32 [count, W, 2]: first and last row of label j within its segment (prompt rows counted, as the frames of
 * lele_hip_token_align_segments), unused slots -1; out_scores f32 [count, W] (the reported shape): the float64 sum in frame order of
 * label j's emissions over its span, rounded once, unused slots 0.0; out_path f32 [count]: the path score rounded once; out_ok i32
 * [count]: 1, or 0 when no alignment exists (fewer frames than L + the number of adjacent equal labels, or a best end of -inf): then
 * spans -1, scores 0.0, path and total -inf.  A segment without frames and with an empty transcript is ok, its scores +0.0.
 * out_total_or_null f32 [count]: the log of the summed probability of ALL alignments of the transcript (the CTC likelihood), the same
 * recurrence with a float64 logaddexp paired ((stay + step) + skip) in the same pass; without it the kernel does not compute it.  It
 * passes through exp / log1p: within 2^-24 |total| + 40 T 2^-53 max(1, largest |alpha|) of the host function's float64.
 * Workspace: the back-pointers, 2 bits a state a frame, 64 words of 2 SPL bits a frame with SPL = 4 states a lane while every transcript
 * has at most 127 labels, else 16: 16 SPL * (most frames of a segment) bytes a segment -- in LDS while that is at most 56 KiB (896 frames
 * at SPL 4, 224 at SPL 16), beyond it count times as much of the context's scratch block.  The call's one layout table holds the
 * offsets, the token offsets and the labels' slots, keyed by all three.  The output buffers must be distinct.  NaN or +inf emissions:
 * unspecified, but the call terminates and stays inside its buffers.  A dense [B, T, U] batch is the packed layout with off[i] = i * T:
 * there is no dense twin.  Everything is checked before anything is launched or resized; count == 0 and R == 0 give empty results of
 * the right shape.  Graph-capturable after one eager run of the same layout and transcripts. */
int lele_hip_ctc_align_segments(LeleCtx* ctx, const LeleTensor* at, const int32_t* cols, int64_t ncols, const int64_t* row_offsets,
                                int64_t count, int64_t skip_rows, int32_t blank, const int32_t* tokens, const int64_t* token_offsets,
                                int64_t width, LeleBuf* out_spans, LeleBuf* out_scores, LeleBuf* out_path, LeleBuf* out_total_or_null,
                                LeleBuf* out_ok, int64_t* out_shape, int32_t* out_rank);
/* lele_hip_attention_view per segment: qkv f32 [R, P] holds Q, K, V of `heads` heads of width dh at columns q_offset, k_offset,
 * v_offset (head h at + h * dh); for every segment and head softmax(Q K^T * scale) V over THAT SEGMENT's rows only, queries and keys
 * alike (gemm.rs:112-222, norm.rs:8) -> out [R, heads * dh], heads merged.  Supported: dh == 128, every segment <= 512 rows, q_offset,
 * k_offset and P multiples of 4; anything else is an error that names the offending segment.  A segment runs the kernel
 * lele_hip_attention_view picks for it ALONE among its 16-row and 32-row forms (16 rows per workgroup while heads * ceil(len / 32) is
 * below half the CUs: then the segment's result is that call's bit for bit), so it does not depend on the rest of the batch.  At most
 * 9 launches a call, whatever the number of segments: one per key-tile class present (8), one more for the class that rule splits.
 * LELE_HIP_ATTENTION_EXACT=1 selects the f32-MFMA arithmetic as it does there. */
int lele_hip_attention_segments(LeleCtx* ctx, const LeleTensor* qkv, int64_t q_offset, int64_t k_offset, int64_t v_offset, int64_t heads,
                                int64_t dh, const int64_t* row_offsets, int64_t count, const LeleTensor* scale_or_null, LeleBuf* out,
                                int64_t* out_shape, int32_t* out_rank);
/* lele_hip_attention_segments with no limit on a segment's rows (utterances over 30 s in a packed batch): same arguments, same checks,
 * same result shape.  A segment of at most 512 rows runs through that call's own work lists, kernels and launches and gets its result
 * bit for bit, whatever else is in the layout.  Longer segments take ONE more launch a call, of the one-pass kernel behind
 * attention_view's large grids (online softmax over 32-key tiles, split-bf16 products) in a single fixed form behind a block locator:
 * 128 query rows of one (segment, head) a workgroup, the longest segments' workgroups first; a long segment's result depends on its own
 * rows only -- not on the batch, the order or the position -- and is the node sequence's values to ~1e-6 relative, not its bits.  So
 * under LELE_HIP_ATTENTION_EXACT=1, which promises those bits, a segment of more than 512 rows is an error that names it and the
 * switch; shorter ones behave as in lele_hip_attention_segments.  No key split: one long utterance alone is heads * ceil(len / 128)
 * workgroups.  Everything is checked before anything is launched or resized: a failing call leaves `out` as it was.
 * Graph-capturable after one eager run of the same layout. */
int lele_hip_attention_segments_long(LeleCtx* ctx, const LeleTensor* qkv, int64_t q_offset, int64_t k_offset, int64_t v_offset,
                                     int64_t heads, int64_t dh, const int64_t* row_offsets, int64_t count, const LeleTensor* scale_or_null,
                                     LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* lele_hip_depthwise_conv1d_tlc (conv1d.rs:837 between two transposes) per segment: x f32 [R, P], channels [x_offset, x_offset + C),
 * w [C, 1, K], pad_left + pad_right == K - 1 (rows are kept) -> out [R, C].  A segment ends where its rows end: taps outside it are
 * skipped, so segment i is bit for bit the dense entry point on it alone as [1, len, P], segments shorter than the stencil included. */
int lele_hip_depthwise_conv1d_tlc_segments(LeleCtx* ctx, const LeleTensor* x, int64_t x_offset, const int64_t* row_offsets, int64_t count,
                                           const LeleTensor* w, const LeleTensor* bias_or_null, int64_t pad_left, int64_t pad_right,
                                           int relu, int add_input, LeleBuf* out, int64_t* out_shape, int32_t* out_rank);
/* concat along time (manipulation.rs:108-207) per segment: `prefix` [p, D] rows, then the segment's rows, for every segment, empty ones
 * included -> out [R + p * count, D]; out_offsets (host, count + 1, written) = row_offsets[i] + p * i.  An exact copy: the prompt
 * embeddings a SenseVoice-shaped encoder puts in front of every utterance. */
int lele_hip_segments_prepend(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* prefix,
                              LeleBuf* out, int64_t* out_offsets, int64_t* out_shape, int32_t* out_rank);
/* lele_hip_lstm / lele_hip_gru (rnn.rs:67, 246) over `count` INDEPENDENT sequences: segment i is the rows [off[i], off[i+1]) of
 * x f32 [R, I] and runs exactly as if it went through the single call alone as [len, 1, I] with its own initial state -- y, h and c
 * are that call's bit for bit, whatever the neighbours, the position or `count` (W x of all R rows is one MFMA GEMM of ONE fixed tile
 * form, the recurrence keeps the single call's summation order).  w [1, 4H, I] / [1, 3H, I], r [1, 4H, H] / [1, 3H, H], bias 8H / 6H
 * values or NULL; initial_h / initial_c hold count * H values (segment i at i * H) or are NULL (zeros).  out_y [R, H] (y_shape),
 * out_h / out_c [1, count, H].  A 0-row segment writes no y row and its final state is its initial state.  out_h / out_c may be the
 * buffers initial_h / initial_c live in: N streams fed chunk by chunk (row_offsets = 0, 1, .., N) keep their state on the device.
 * One 1024-thread workgroup walks a group of up to NS segments in lockstep; info_or_null receives {kernel form: 0 = nothing launched
 * (R == 0), 1 = recurrent weights held in registers (H / S in {16, 32, 64}), 2 = streamed from the transposed copy in L2; NS}.
 * Everything is checked before anything is launched or resized: a failing call leaves every out buffer as it was. */
int lele_hip_lstm_segments(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* w,
                           const LeleTensor* r, const LeleTensor* bias_or_null, const LeleTensor* initial_h_or_null,
                           const LeleTensor* initial_c_or_null, LeleBuf* out_y, LeleBuf* out_h, LeleBuf* out_c, int64_t* y_shape,
                           int32_t* y_rank, int32_t* info_or_null);
int lele_hip_gru_segments(LeleCtx* ctx, const LeleTensor* x, const int64_t* row_offsets, int64_t count, const LeleTensor* w,
                          const LeleTensor* r, const LeleTensor* bias_or_null, const LeleTensor* initial_h_or_null,
                          int linear_before_reset, LeleBuf* out_y, LeleBuf* out_h, int64_t* y_shape, int32_t* y_rank,
                          int32_t* info_or_null);

#ifdef __cplusplus
}
#endif
#endif /* LELE_HIP_H */
