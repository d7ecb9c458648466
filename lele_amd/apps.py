"""Host-side halves of the application steps around a lele model run.

The device halves are in csrc/app.hip (`kernels.wav_to_f32`, `argmax_last`, `token_filter`, `image_preprocess`,
`yolo_seg_postprocess`); what remains on the host is string handling and a tiny sequential state machine:

  * `special_token_mask`  -- the per-vocabulary skip flags of examples/sensevoice/src/tokenizer.rs:63-69
  * `detokenize`          -- tokenizer.rs:74-81 (join, sentencepiece underscore -> space, trim)
  * `vad_segments`        -- examples/silero/src/main.rs:151-228 (speech segments from per-chunk probabilities)
  * `token_times`         -- encoder frames of kept tokens (kernels.token_align_segments) -> start times in seconds
  * `ctc_prefix_beam_search` -- the reference of kernels.ctc_beam_search_segments, one utterance on the host
  * `beam_results`        -- that kernel's four arrays -> the reference's list format
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
