#!/usr/bin/env python3
"""Forced alignment on the CTC projection's shape ([rows, 512] x [512, 25055]): what the listed-columns head and the lattice kernel cost.

    scored     fused_quantized_linear_argmax_logprob_segments             -> ids + logprob (the head `at` extends)
    atU        fused_quantized_linear_logprob_at_segments, U columns      -> ... + f32 [rows, U], U ~ 50 / 500 / 2000
    align      ctc_align_segments on a stored [rows, U] table, Viterbi + total, and `align_viterbi` without the total
    chain      at (the transcripts' own columns) -> align
    today      fused_quantized_linear_segments -> logits to the host -> float64 log-soft-max, gather -> apps.ctc_forced_align per utterance
               (timed with the wall clock, once: it is seconds, not microseconds)

Layouts 32 x 171 and 1 x 504 rows, four prompt rows a segment, transcripts of ~40 and ~150 labels (fewer where the frames do not hold
them).  Device legs are recorded hipGraphs; one timing is hipEvents around `steps` warmed replays; the legs of a layout alternate
`reps` (>= 20) times in one process and the medians are reported.  The chain's spans are compared with the host's before anything is
timed.  One JSON record goes to --out (profiles/ctc_align.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, VOCAB = 512, 25055
LAYOUTS = [(32, 171), (1, 504)]
WIDTHS = (50, 500, 2000)
LABELS = (40, 150)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--seed", type=int, default=2025)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repeats a leg"

    import lele_amd
    from lele_amd import kernels as K
    from lele_amd.apps import align_results, ctc_forced_align
    from sensevoice_graph import QLinear

    ctx = lele_amd.default_ctx(0)
    rng = np.random.default_rng(args.seed)
    p = QLinear(rng, D, VOCAB, K.Weight)
    w = (p.w, p.scale, p.zero, p.bias)
    res = {"device": "MI355X (gfx950)", "k": D, "n": VOCAB, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "seed": args.seed,
           "timing": "hipEvents around `steps` warmed hipGraph replays; the legs of a layout alternate, `reps` times; medians; `today` wall clock, once",
           "layouts": {}}
    bufs = [ctx.buf() for _ in range(12)]
    for batch, m in LAYOUTS:
        rows = batch * m
        off = np.arange(batch + 1, dtype=np.int64) * m
        x = ctx.buf().upload(rng.standard_normal((rows, D)).astype(np.float32))
        ids, _ = K.fused_quantized_linear_argmax_logprob_segments(x, off, *w, out_ids=bufs[0], out_logprob=bufs[1], ctx=ctx)
        ids = ids.numpy().reshape(batch, m)
        rec = {"rows": rows, "batch": batch, "m": m}
        legs = {"scored": lambda: K.fused_quantized_linear_argmax_logprob_segments(x, off, *w, out_ids=bufs[0], out_logprob=bufs[1], ctx=ctx)}
        for u in WIDTHS:
            cols = sorted({0} | {int(c) for c in rng.choice(VOCAB, u - 1, replace=False)})
            legs["at%d" % u] = lambda cols=cols: K.fused_quantized_linear_logprob_at_segments(x, off, *w, cols, out_ids=bufs[0], out_logprob=bufs[1],
                                                                                             out_at=bufs[2], ctx=ctx)
        for labels in LABELS:
            # a transcript the frames can hold: the utterance's own greedy labels first (so the path is a likely one), then seeded ones
            trs = []
            for b in range(batch):
                own = [int(v) for v in ids[b, 4:] if v != 0]
                tr = (own + [int(v) for v in rng.integers(1, VOCAB, labels)])[:min(labels, (m - 4) // 2)]
                trs.append(tuple(tr))
            cols = sorted({0} | {t for tr in trs for t in tr})
            tag = "L%d" % labels
            rec[tag + "_labels"], rec[tag + "_columns"] = [len(t) for t in trs][:4], len(cols)
            at_buf = ctx.buf()
            _, _, at = K.fused_quantized_linear_logprob_at_segments(x, off, *w, cols, out_ids=bufs[0], out_logprob=bufs[1], out_at=at_buf, ctx=ctx)
            legs["align_" + tag] = lambda at=at, cols=cols, trs=trs: K.ctc_align_segments(
                at, cols, off, trs, 0, 4, 0, out_spans=bufs[3], out_scores=bufs[4], out_path=bufs[5], out_total=bufs[6], out_ok=bufs[7], ctx=ctx)
            legs["align_viterbi_" + tag] = lambda at=at, cols=cols, trs=trs: K.ctc_align_segments(
                at, cols, off, trs, 0, 4, 0, total=False, out_spans=bufs[3], out_scores=bufs[4], out_path=bufs[5], out_ok=bufs[7], ctx=ctx)

            def chain(cols=cols, trs=trs):
                _, _, a = K.fused_quantized_linear_logprob_at_segments(x, off, *w, cols, out_ids=bufs[0], out_logprob=bufs[1], out_at=bufs[2], ctx=ctx)
                return K.ctc_align_segments(a, cols, off, trs, 0, 4, 0, out_spans=bufs[3], out_scores=bufs[4], out_path=bufs[5], out_total=bufs[6],
                                            out_ok=bufs[7], ctx=ctx)
            legs["chain_" + tag] = chain
            got = align_results(*(o.numpy().copy() for o in chain()), [len(t) for t in trs])
            # today's route, and the comparison of the two
            t0 = time.perf_counter()
            logits = K.fused_quantized_linear_segments(x, off, *w, False, out=bufs[8], ctx=ctx).numpy().astype(np.float64)
            mx = logits.max(axis=1, keepdims=True)
            lsm = ((logits - mx) - np.log(np.exp(logits - mx).sum(axis=1, keepdims=True)))[:, cols].astype(np.float32)
            want = [ctc_forced_align(lsm[off[b]:off[b + 1]], cols, trs[b], 0, 4) for b in range(batch)]
            rec["today_" + tag + "_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            rec["today_logits_bytes"] = rows * VOCAB * 4
            rec[tag + "_spans_equal_to_host_route"] = bool(all(g[:2] == h[:2] for g, h in zip(got, want)))
            rec[tag + "_aligned"] = int(sum(g[0] for g in got))
        for leg in legs.values():      # eagerly first: buffers at their final size, every table on the device
            leg()
            leg()
        ctx.sync()
        graphs = {}
        for name, leg in legs.items():
            ctx.graph_begin()
            leg()
            graphs[name] = ctx.graph_end()

        def timed(name):
            for _ in range(args.warmup):
                graphs[name].launch()
            ctx.sync()
            ctx.timer_start()
            for _ in range(args.steps):
                graphs[name].launch()
            return ctx.timer_stop() / args.steps

        ms = {name: [] for name in graphs}
        for _ in range(args.reps):
            for name in graphs:
                ms[name].append(timed(name))
        for name, v in ms.items():
            rec[name + "_us_median"] = round(1e3 * float(np.median(v)), 2)
            rec[name + "_us_q1"], rec[name + "_us_q3"] = (round(1e3 * float(q), 2) for q in np.percentile(v, [25, 75]))
        for u in WIDTHS:
            rec["at%d_minus_scored_us_median" % u] = round(rec["at%d_us_median" % u] - rec["scored_us_median"], 2)
        for labels in LABELS:
            rec["align_L%d_us_per_frame" % labels] = round(rec["align_L%d_us_median" % labels] / (m - 4), 3)
            rec["align_viterbi_L%d_us_per_frame" % labels] = round(rec["align_viterbi_L%d_us_median" % labels] / (m - 4), 3)
        res["layouts"]["%dx%d" % (batch, m)] = rec
        print("%dx%d" % (batch, m), json.dumps(rec), flush=True)
        for g in graphs.values():
            g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
