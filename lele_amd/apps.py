"""Host-side halves of the application steps around a lele model run.

The device halves are in csrc/app.hip (`kernels.wav_to_f32`, `argmax_last`, `token_filter`, `image_preprocess`,
`yolo_seg_postprocess`); what remains on the host is string handling and a tiny sequential state machine:

  * `special_token_mask`  -- the per-vocabulary skip flags of examples/sensevoice/src/tokenizer.rs:63-69
  * `detokenize`          -- tokenizer.rs:74-81 (join, sentencepiece underscore -> space, trim)
  * `vad_segments`        -- examples/silero/src/main.rs:151-228 (speech segments from per-chunk probabilities)
  * `token_times`         -- encoder frames of kept tokens (kernels.token_align_segments) -> start times in seconds
  * `ctc_prefix_beam_search` -- the reference of kernels.ctc_beam_search_segments, one utterance on the host
  * `beam_results`        -- that kernel's four arrays -> the reference's list format
  * `ctc_forced_align`    -- the reference of kernels.ctc_align_segments: a known transcript's Viterbi alignment and CTC likelihood
  * `align_results`       -- that kernel's five arrays -> the reference's format
  * `pack_images`, `unpack_masks` -- a queue of images of different sizes into kernels.image_preprocess_batch's one byte buffer, and
    kernels.yolo_seg_postprocess_sized's packed masks back into one array per image
  * `resample_linear`, `resample_fir_table`, `resample_fir` -- the references of features.Resampler: the reference's linear
    `resample` and the Kaiser-windowed polyphase FIR in float64 (never used by the device path)
"""
import numpy as np


def special_token_mask(id_to_token):
    """skip[id] = 1 for the blank (id 0) and every "<|...|>" token (tokenizer.rs:66)"""
    skip = np.zeros(len(id_to_token), np.uint8)
    for i, tok in enumerate(id_to_token):
        if i == 0 or (tok.startswith("<|") and tok.endswith("|>")):
            skip[i] = 1
    return skip


def detokenize(ids, id_to_token):
    """tokenizer.rs:74-81: kept ids (as produced by kernels.token_filter, -1 padding ignored) -> text"""
    text = "".join(id_to_token[int(i)] for i in ids if int(i) >= 0)
    return text.replace("▁", " ").strip()


def token_times(frames, prompt_rows=4, lfr_n=6, frame_shift_ms=10.0):
    """frames as kernels.token_align_segments gives them (row index within the utterance, -1 = padding) -> start times in seconds,
    float64 of the same shape: an encoder row behind the `prompt_rows` prompt rows covers `lfr_n` feature frames of `frame_shift_ms`,
    so row f starts at (f - prompt_rows) * lfr_n * frame_shift_ms / 1000.  A frame inside the prompt rows is reported as 0.0, padding
    is passed through as -1."""
    f = np.asarray(frames, np.int64)
    t = np.maximum(f - int(prompt_rows), 0).astype(np.float64) * (int(lfr_n) * float(frame_shift_ms)) / 1000.0
    return np.where(f < 0, -1.0, t)


def ctc_prefix_beam_search(ids, logprob, blank=0, beam=4, nbest=1):
    """CTC prefix beam search over the k best candidates of every frame, as kernels.fused_quantized_linear_topk gives them for ONE
    utterance (the caller slices the prompt rows off, as with token_times): ids int [T, k], logprob [T, k] -> the `nbest` best label
    sequences as [(tuple of ids, log score)], best first, equal scores in the order of the tuples.  The score of a sequence is the log
    of the sum, over the alignments that collapse to it (repeats merged, then blanks removed) and use only the given candidates, of the
    product of their frame probabilities.  float64 log space, one blank-ended and one label-ended score per prefix; at most `beam`
    prefixes survive a frame; a candidate with id -1 (fewer than k columns) is skipped.  Pure host code."""
    ids, logprob = np.asarray(ids, np.int64), np.asarray(logprob, np.float64)
    if ids.ndim != 2 or ids.shape != logprob.shape:
        raise ValueError("ctc_prefix_beam_search: ids and logprob must both be [T, k]")
    if beam < 1 or nbest < 1:
        raise ValueError("ctc_prefix_beam_search: beam and nbest must be at least 1")
    ninf = -np.inf
    beams = {(): (0.0, ninf)}                   # prefix -> (log p ending in blank, log p ending in its last label)
    total = lambda s: np.logaddexp(s[0], s[1])  # noqa: E731
    for t in range(ids.shape[0]):
        nxt = {}

        def add(prefix, which, lp):
            s = nxt.setdefault(prefix, [ninf, ninf])
            s[which] = np.logaddexp(s[which], lp)

        for prefix, (pb, pnb) in beams.items():
            for c, lp in zip(ids[t].tolist(), logprob[t].tolist()):
                if c < 0:
                    continue
                if c == blank:
                    add(prefix, 0, np.logaddexp(pb, pnb) + lp)
                elif prefix and prefix[-1] == c:
                    add(prefix, 1, pnb + lp)             # the repeat merges
                    add(prefix + (c,), 1, pb + lp)       # ... unless a blank separates the two
                else:
                    add(prefix + (c,), 1, np.logaddexp(pb, pnb) + lp)
        ranked = sorted(nxt.items(), key=lambda kv: (-total(kv[1]), kv[0]))
        beams = {p: (s[0], s[1]) for p, s in ranked[:beam]}
    ranked = sorted(beams.items(), key=lambda kv: (-total(kv[1]), kv[0]))
    return [(p, float(total(s))) for p, s in ranked[:nbest]]


def beam_results(tokens, lengths, scores, counts):
    """the four host arrays of kernels.ctc_beam_search_segments (tokens [count, nbest, W], lengths and scores [count, nbest], counts
    [count]) -> per utterance the list ctc_prefix_beam_search returns: [(tuple of ids, score)], best first"""
    tokens, lengths = np.asarray(tokens), np.asarray(lengths)
    scores, counts = np.asarray(scores), np.asarray(counts)
    if tokens.ndim != 3 or lengths.shape != tokens.shape[:2] or scores.shape != tokens.shape[:2] or counts.shape != tokens.shape[:1]:
        raise ValueError("beam_results: tokens [count, nbest, W], lengths / scores [count, nbest] and counts [count] required")
    return [[(tuple(int(v) for v in tokens[i, n, :int(lengths[i, n])]), float(scores[i, n])) for n in range(int(counts[i]))]
            for i in range(tokens.shape[0])]


def ctc_forced_align(logprob_at, cols, tokens, blank=0, skip_rows=0, return_bound=False):
    """CTC forced alignment of a known transcript for ONE utterance: logprob_at float32 [rows, U], the log-probabilities of the U
    strictly ascending columns `cols` as kernels.fused_quantized_linear_logprob_at gives them; the frames are the rows behind the first
    `skip_rows`; `tokens` the transcript's L labels (every one and `blank` listed in cols, none the blank, L <= 511)
    -> (ok, spans, token_scores, path_score, total): spans [(first, last)] the rows (within logprob_at, prompt rows counted) of every
    label on the best path, token_scores the float64 sum in frame order of the label's emissions over its span, path_score the best
    path's, total the log of the summed probability of ALL alignments (the CTC likelihood).  Without an alignment -- fewer frames than L
    + the number of adjacent equal labels, or a best end of -inf -- (False, [], [], -inf, -inf); no frames and no labels is (True, [],
    [], 0.0, 0.0).
    The lattice has states s = 0 .. 2 L, even = blank, odd = label (s - 1) / 2; alpha_0(0) = e_0(blank), alpha_0(1) = e_0(label 0);
    alpha_t(s) = best + e_t(s) with best over alpha_{t-1}(s) (stay), (s - 1) (step) and, for an odd s whose label differs from the one
    before it, (s - 2) (skip), a later candidate replacing an earlier one only if strictly greater; the end is state 2 L unless 2 L - 1 is
    strictly greater.  float64 with one addition a frame, so the path score is the sum in frame order of the path's float32 emissions:
    the device kernel performs the same IEEE additions, its spans and scores are EQUAL to these.  The total is the same recurrence with
    logaddexp paired ((stay, step), skip).  return_bound appends the largest finite |alpha| either recurrence met (what a tolerance on
    the total is stated in).  Pure host code."""
    e32 = np.asarray(logprob_at, np.float32)
    cols = np.asarray(cols, np.int64).reshape(-1)
    if e32.ndim != 2 or e32.shape[1] != len(cols) or len(cols) < 1:
        raise ValueError("ctc_forced_align: logprob_at must be [rows, U] with one column per entry of cols")
    if np.any(cols[1:] <= cols[:-1]):
        raise ValueError("ctc_forced_align: cols must be strictly ascending")
    tokens = [int(t) for t in tokens]
    n = len(tokens)
    if n > 511:
        raise ValueError("ctc_forced_align: a transcript of %d labels, more than 511" % n)

    def slot(c, what):
        i = int(np.searchsorted(cols, c))
        if i >= len(cols) or int(cols[i]) != c:
            raise ValueError("ctc_forced_align: %s %d is not among the listed columns" % (what, c))
        return i

    bslot = slot(int(blank), "blank")
    for j, t in enumerate(tokens):
        if t == int(blank):
            raise ValueError("ctc_forced_align: position %d: the label is the blank (%d)" % (j, t))
    slots = [slot(t, "position %d: label" % j) for j, t in enumerate(tokens)]
    ninf = -np.inf
    fail = (False, [], [], ninf, ninf)
    bound = 0.0

    def done(res):
        return res + (bound,) if return_bound else res

    frames = e32[int(skip_rows):]
    nt, ns = frames.shape[0], 2 * n + 1
    if nt == 0:
        return done((True, [], [], 0.0, 0.0) if n == 0 else fail)
    state_slot = np.full(ns, bslot, np.int64)
    state_slot[1::2] = slots
    allowed = np.zeros(ns, bool)
    for j in range(1, n):
        allowed[2 * j + 1] = tokens[j] != tokens[j - 1]
    em = frames[:, state_slot].astype(np.float64)
    a = np.full(ns, ninf)
    a[0] = em[0, 0]
    if n:
        a[1] = em[0, 1]
    tot = a.copy()
    back = np.zeros((nt, ns), np.uint8)

    def finite_max(x):
        f = np.abs(x[np.isfinite(x)])
        return float(f.max()) if f.size else 0.0

    bound = max(finite_max(a), 0.0)
    for t in range(1, nt):
        p = np.concatenate(([ninf, ninf], a))
        step, skip = p[1:-1], np.where(allowed, p[:-2], ninf)
        best, frm = a.copy(), np.zeros(ns, np.uint8)
        m = step > best
        best[m], frm[m] = step[m], 1
        m = skip > best
        best[m], frm[m] = skip[m], 2
        a = best + em[t]
        back[t] = frm
        p = np.concatenate(([ninf, ninf], tot))
        tot = np.logaddexp(np.logaddexp(tot, p[1:-1]), np.where(allowed, p[:-2], ninf)) + em[t]
        bound = max(bound, finite_max(a), finite_max(tot))
    repeats = sum(1 for j in range(1, n) if tokens[j] == tokens[j - 1])
    s = 2 * n if n == 0 or a[2 * n] >= a[2 * n - 1] else 2 * n - 1
    if nt < n + repeats or a[s] == ninf:
        return done(fail)
    path_score = float(a[s])
    total = float(np.logaddexp(tot[2 * n], tot[2 * n - 1])) if n else float(tot[0])
    first, last = [0] * n, [-1] * n
    prev = -1
    for t in range(nt - 1, -1, -1):
        if s & 1:
            if s != prev:
                last[s >> 1] = t
            first[s >> 1] = t
        prev = s
        s -= int(back[t, s])
    scores = []
    for j in range(n):
        acc = 0.0
        for t in range(first[j], last[j] + 1):
            acc += float(em[t, 2 * j + 1])
        scores.append(acc)
    k = int(skip_rows)
    return done((True, [(first[j] + k, last[j] + k) for j in range(n)], scores, path_score, total))


def align_results(spans, scores, path, total, ok, lengths):
    """the five host arrays of kernels.ctc_align_segments (spans [count, W, 2], scores [count, W], path / total / ok [count]; total may
    be None) and the transcripts' lengths -> per utterance what ctc_forced_align returns, the scores as the float32 values the kernel
    rounded them to: (ok, [(first, last)], [score], path score, total or None)"""
    spans, scores, path, ok = np.asarray(spans), np.asarray(scores), np.asarray(path), np.asarray(ok)
    total = None if total is None else np.asarray(total)
    if spans.ndim != 3 or spans.shape[2] != 2 or scores.shape != spans.shape[:2] or path.shape != spans.shape[:1] or \
            ok.shape != spans.shape[:1] or (total is not None and total.shape != spans.shape[:1]) or len(lengths) != spans.shape[0]:
        raise ValueError("align_results: spans [count, W, 2], scores [count, W], path / total / ok [count] and count lengths required")
    out = []
    for i, n in enumerate(lengths):
        n = int(n) if ok[i] else 0
        out.append((bool(ok[i]), [(int(spans[i, j, 0]), int(spans[i, j, 1])) for j in range(n)], [float(scores[i, j]) for j in range(n)],
                    float(path[i]), None if total is None else float(total[i])))
    return out


def _ms_to_samples(ms, sample_rate):
    # ((sr as f32) * (ms / 1000.0)).round() as usize -- f32 arithmetic, round half away from zero
    v = np.float32(sample_rate) * (np.float32(ms) / np.float32(1000.0))
    return int(np.floor(np.abs(v) + np.float32(0.5)) * np.sign(v))


def vad_segments(probs, chunk_size, padded_len, audio_len, sample_rate=16000, threshold=0.3, min_silence_ms=200.0,
                 min_speech_ms=400.0, speech_pad_ms=120.0, merge_gap_ms=200.0):
    """examples/silero/src/main.rs:151-228 with VadConfig::default (main.rs:18-28) -> [(start, end)] in samples"""
    min_silence = max(_ms_to_samples(min_silence_ms, sample_rate), 1)
    min_speech = max(_ms_to_samples(min_speech_ms, sample_rate), 1)
    speech_pad = _ms_to_samples(speech_pad_ms, sample_rate)
    merge_gap = _ms_to_samples(merge_gap_ms, sample_rate)
    thr = np.float32(threshold)
    segments, triggered, start, silence = [], False, 0, 0
    for i, prob in enumerate(np.asarray(probs, np.float32).reshape(-1)):
        offset = i * chunk_size
        frame_end = min(offset + chunk_size, padded_len)
        if prob >= thr:
            if not triggered:
                triggered, start = True, max(offset - speech_pad, 0)
            silence = 0
        elif triggered:
            silence += frame_end - offset
            if silence >= min_silence:
                end = min(frame_end + speech_pad, audio_len)
                if end > start and end - start >= min_speech:
                    segments.append([start, end])
                triggered, silence = False, 0
    if triggered and audio_len > start and audio_len - start >= min_speech:
        segments.append([start, audio_len])
    merged = []
    for seg in sorted(segments, key=lambda s: s[0]):  # stable, as sort_by_key
        if merged:
            last = merged[-1]
            if seg[0] <= last[1] or max(seg[0] - last[1], 0) <= merge_gap:
                last[1] = max(last[1], seg[1])
                continue
        merged.append(list(seg))
    return [(a, b) for a, b in merged]


def pack_images(images):
    """a queue of [H, W, 3] u8 images of different sizes -> (bytes u8 [total], offsets int64 [n], heights int32 [n], widths int32 [n]),
    the arguments of kernels.image_preprocess_batch.  An array listed more than once (the same object) is stored once: its entries
    share an offset."""
    offsets, heights, widths, parts, seen, total = [], [], [], [], {}, 0
    for img in images:
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("pack_images: u8 [H, W, 3] images required, got %s %s" % (a.dtype, a.shape))
        if id(img) not in seen:
            seen[id(img)] = total
            parts.append(np.ascontiguousarray(a).reshape(-1))
            total += a.size
        offsets.append(seen[id(img)])
        heights.append(a.shape[0])
        widths.append(a.shape[1])
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return data, np.array(offsets, np.int64), np.array(heights, np.int32), np.array(widths, np.int32)


def unpack_masks(mask, mask_offsets, sizes):
    """kernels.yolo_seg_postprocess_sized's packed mask u8 [sum h * w] -> one [h, w] array per image; sizes = [(width, height)]"""
    flat = np.asarray(mask.numpy() if hasattr(mask, "numpy") else mask).reshape(-1)
    sz = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if len(mask_offsets) != len(sz) + 1:
        raise ValueError("unpack_masks: %d offsets for %d sizes" % (len(mask_offsets), len(sz)))
    out = []
    for n, (w, h) in enumerate(sz):
        a, b = int(mask_offsets[n]), int(mask_offsets[n + 1])
        if b - a != w * h or b > flat.size:
            raise ValueError("unpack_masks: image %d is %d x %d but its mask holds %d bytes" % (n, w, h, b - a))
        out.append(flat[a:b].reshape(int(h), int(w)))
    return out


def resample_linear(samples, from_rate, to_rate):
    """examples/web-demo/src/audio.rs:114-138 (the reference of features.Resampler(mode="linear")): f32 in, f32 out, every output by
    the reference's own float64 operations in its own order -- written over arrays; resample_linear_loop is the same line by line"""
    s = np.asarray(samples, np.float32).reshape(-1)
    if from_rate == to_rate:                                        # :116-118
        return s.copy()
    ratio = float(from_rate) / float(to_rate)                       # :120
    output_len = int(float(len(s)) / ratio)                         # :121
    i = np.arange(output_len, dtype=np.int64)
    src_pos = i.astype(np.float64) * ratio                          # :125
    idx = src_pos.astype(np.int64)                                  # :126 (src_pos >= 0: `as usize` truncates)
    frac = src_pos - idx.astype(np.float64)                         # :127
    keep = idx < len(s)                                             # :132: past the end nothing is pushed
    idx, frac = idx[keep], frac[keep]
    if len(idx) == 0:
        return np.zeros(0, np.float32)
    s64 = s.astype(np.float64)
    nxt = np.minimum(idx + 1, len(s) - 1)
    val = (s64[idx] * (1.0 - frac) + s64[nxt] * frac).astype(np.float32)   # :130-131: two products, one sum, then `as f32`
    return np.where(idx + 1 < len(s), val, s[idx])                  # :129 / :132-133: the last sample as it is


def resample_linear_loop(samples, from_rate, to_rate):
    """audio.rs:114-138 line by line, one output at a time (slow; tests pin resample_linear to it)"""
    s = np.asarray(samples, np.float32).reshape(-1)
    if from_rate == to_rate:
        return s.copy()
    ratio = float(from_rate) / float(to_rate)
    output_len = int(float(len(s)) / ratio)
    out = []
    for i in range(output_len):
        src_pos = float(i) * ratio
        idx = int(src_pos)
        frac = src_pos - float(idx)
        if idx + 1 < len(s):
            val = float(s[idx]) * (1.0 - frac) + float(s[idx + 1]) * frac
            out.append(np.float32(val))
        elif idx < len(s):
            out.append(s[idx])
    return np.asarray(out, np.float32)


def _bessel_i0(x):
    """modified Bessel function of the first kind, order 0: its power series (every term positive)"""
    x = np.asarray(x, np.float64)
    q = x * x / 4.0
    total = np.ones_like(x)
    term = np.ones_like(x)
    for k in range(1, 500):
        term = term * q / (float(k) * float(k))
        total = total + term
        if np.all(term < total * 1e-18):
            break
    return total


def resample_fir_shape(from_rate, to_rate, z=16):
    """(L, M, T) of the polyphase FIR: L = to / gcd, M = from / gcd, T = 2 * ceil(z / min(1, L/M)) taps a phase"""
    import math
    g = math.gcd(int(from_rate), int(to_rate))
    L, M = int(to_rate) // g, int(from_rate) // g
    return L, M, 2 * int(math.ceil(float(z) / min(1.0, float(L) / float(M))))


def resample_fir_table(from_rate, to_rate, z=16, beta=8.6, rolloff=0.9):
    """The Kaiser-windowed sinc table of features.Resampler(mode="sinc") in float64, [L, T]: tap t of phase p weighs input sample
    base - T/2 + 1 + t, at distance d = (t - T/2 + 1) - p/L from the output's instant, by s sinc(s d) kaiser_beta(d / (T/2)),
    s = rolloff * min(1, L/M); every phase normalised to sum 1.  The library uploads this table rounded to float32."""
    L, M, T = resample_fir_shape(from_rate, to_rate, z)
    s = float(rolloff) * min(1.0, float(L) / float(M))
    W = float(T) / 2.0
    d = (np.arange(T, dtype=np.float64)[None, :] - float(T // 2 - 1)) - np.arange(L, dtype=np.float64)[:, None] / float(L)
    a = np.pi * s * d
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    u = d / W
    win = _bessel_i0(float(beta) * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / _bessel_i0(float(beta))
    w = s * sinc * win
    return w / w.sum(axis=1, keepdims=True)


def resample_fir(samples, table, L, M):
    """The polyphase FIR on the host: float64 accumulation of `table` [L, T] as given (pass the float32-rounded table to get the
    reference of the device kernel).  The input is zero outside [0, len); ceil(len * L / M) outputs, float64."""
    s = np.asarray(samples, np.float64).reshape(-1)
    tab = np.asarray(table, np.float64)
    T = tab.shape[1]
    n = len(s)
    n_out = (n * L + M - 1) // M
    i = np.arange(n_out, dtype=np.int64)
    base, phase = (i * M) // L, (i * M) % L
    pad = np.concatenate([np.zeros(T, np.float64), s, np.zeros(T, np.float64)])
    out = np.zeros(n_out, np.float64)
    for t in range(T):
        out += tab[phase, t] * pad[base - T // 2 + 1 + t + T]
    return out
