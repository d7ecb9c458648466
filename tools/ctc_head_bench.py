#!/usr/bin/env python3
"""The greedy decode head against the pair of calls it stands for, on the CTC projection's shape ([rows, 512] x [512, 25055]):

    fused   fused_quantized_linear_argmax[_segments]                    -> int32 ids, the logits never stored
    pair    fused_quantized_linear[_segments] -> argmax_last            -> f32 logits [rows, 25055] written, read back, dropped

With --scored a third leg runs in the same alternation:

    scored  fused_quantized_linear_argmax_logprob[_segments]            -> int32 ids + f32 log-probability of each winner

and the record (profiles/ctc_head_scored.json) says what the scores cost over `fused` and whether `scored` stays under the pair (going
back to stored logits must not be the cheaper way to a score).  --compare sets the `fused` medians of another build's run (a saved copy
of the library under LELE_HIP_LIBRARY, run turn about with this one) beside this run's, against `fused`'s own spread (the interquartile
range of its timings).

Dense shapes 32 x 171, 64 x 171, 1 x 504 and one packed layout of mixed lengths.  Every leg is a recorded hipGraph; one timing is
hipEvents around `steps` warmed replays; the legs of a shape alternate `reps` (>= 20) times in one process and the medians are
reported, with the two halves of the pair timed on their own as well.  The ids of both forms are compared before anything is timed.
One JSON record goes to --out (profiles/ctc_head.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, VOCAB = 512, 25055
DENSE = [(32, 171), (64, 171), (1, 504)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/ctc_head.json, with --scored profiles/ctc_head_scored.json")
    ap.add_argument("--scored", action="store_true", help="add the scored head's leg")
    ap.add_argument("--compare", default=None, help="the record of another build's run of this tool (taken turn about with this one): "
                    "its `fused` medians are set beside this run's, with whether they lie within three of this run's same-leg spreads")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--packed-count", type=int, default=32)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repeats a leg"
    args.out = args.out or os.path.join(ROOT, "profiles", "ctc_head_scored.json" if args.scored else "ctc_head.json")

    import lele_amd
    from lele_amd import kernels as K
    from sensevoice_graph import QLinear

    ctx = lele_amd.default_ctx(0)
    rng = np.random.default_rng(args.seed)
    p = QLinear(rng, D, VOCAB, K.Weight)
    w = (p.w, p.scale, p.zero, p.bias)
    lengths = [int(v) for v in rng.integers(20, 505, size=args.packed_count)]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    shapes = [("dense_%dx%d" % s, s, None) for s in DENSE] + [("packed_%d_mixed" % args.packed_count, (1, int(off[-1])), off)]
    logits_buf, ids_pair, ids_fused, ids_scored, lp_scored = (ctx.buf() for _ in range(5))

    res = {"library": os.environ.get("LELE_HIP_LIBRARY") or "liblele_hip.so", "device": "MI355X (gfx950)", "k": D, "n": VOCAB, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "seed": args.seed,
           "timing": "hipEvents around `steps` warmed hipGraph replays; the legs of a shape alternate, `reps` times; medians",
           "packed_lengths": lengths, "shapes": {}}
    for name, (batch, m), offsets in shapes:
        rows = batch * m
        x = ctx.buf().upload(rng.standard_normal((rows, D) if offsets is not None else (batch, m, D)).astype(np.float32))
        if offsets is None:
            legs = {"fused": lambda: K.fused_quantized_linear_argmax(x, *w, out=ids_fused, ctx=ctx),
                    "linear": lambda: K.fused_quantized_linear(x, *w, out=logits_buf, ctx=ctx)}
        else:
            legs = {"fused": lambda: K.fused_quantized_linear_argmax_segments(x, offsets, *w, out=ids_fused, ctx=ctx),
                    "linear": lambda: K.fused_quantized_linear_segments(x, offsets, *w, out=logits_buf, ctx=ctx)}
        if args.scored and offsets is None:
            legs["scored"] = lambda: K.fused_quantized_linear_argmax_logprob(x, *w, out_ids=ids_scored, out_logprob=lp_scored, ctx=ctx)
        elif args.scored:
            legs["scored"] = lambda: K.fused_quantized_linear_argmax_logprob_segments(x, offsets, *w, out_ids=ids_scored, out_logprob=lp_scored,
                                                                                      ctx=ctx)
        lg = legs["linear"]()
        legs["argmax"] = lambda: K.argmax_last(lg, out=ids_pair, ctx=ctx)
        legs["pair"] = lambda: (legs["linear"](), legs["argmax"]())
        for _ in range(2):   # eagerly first: weights packed, buffers at their final size, the layout's table on the device
            a = legs["fused"]().numpy()
            legs["pair"]()
            b = K.argmax_last(lg, out=ids_pair, ctx=ctx).numpy()
        assert np.array_equal(a.reshape(-1), b.reshape(-1)), "%s: the fused ids are not the pair's" % name
        if args.scored:
            for _ in range(2):
                si, sl = legs["scored"]()
                si, sl = si.numpy(), sl.numpy()
            assert np.array_equal(si.reshape(-1), a.reshape(-1)), "%s: the scored ids are not the fused ids" % name
            # against the stored logits of the pair: float64 -log sum exp(v - max) of a sample of rows
            v = lg.numpy().reshape(rows, VOCAB)[::max(1, rows // 64)].astype(np.float64)
            ref = -np.log(np.exp(v - v.max(axis=1, keepdims=True)).sum(axis=1))
            lp_err = float(np.max(np.abs(sl.reshape(-1)[::max(1, rows // 64)].astype(np.float64) - ref)))
            assert lp_err <= 1e-5, "%s: log-probabilities off by %g" % (name, lp_err)
        ctx.sync()
        graphs = {}
        # `scored` right behind `fused`: the leg that runs in front of `fused` is `argmax` with and without it
        for leg in ("fused",) + (("scored",) if args.scored else ()) + ("pair", "linear", "argmax"):
            ctx.graph_begin()
            legs[leg]()
            graphs[leg] = ctx.graph_end()

        def timed(leg):
            for _ in range(args.warmup):
                graphs[leg].launch()
            ctx.sync()
            ctx.timer_start()
            for _ in range(args.steps):
                graphs[leg].launch()
            return ctx.timer_stop() / args.steps

        ms = {leg: [] for leg in graphs}
        for _ in range(args.reps):
            for leg in graphs:
                ms[leg].append(timed(leg))
        tiles = (VOCAB + 127) // 128
        rec = {"rows": rows, "batch": batch, "m": m}
        for leg, v in ms.items():
            rec[leg + "_us_median"] = round(1e3 * float(np.median(v)), 2)
            rec[leg + "_us_min"] = round(1e3 * min(v), 2)
            rec[leg + "_us_max"] = round(1e3 * max(v), 2)
        rec["fused_over_pair_median"] = round(rec["fused_us_median"] / rec["pair_us_median"], 4)
        rec["fused_median_not_above_pair_median"] = bool(rec["fused_us_median"] <= rec["pair_us_median"])
        rec["pair_logits_bytes"] = rows * VOCAB * 4          # allocated, written and read back by the pair only
        rec["fused_key_table_bytes"] = rows * tiles * 8      # workspace of the fused call only: one key per (row, column tile)
        rec["ids_equal"] = True
        q1, q3 = np.percentile(ms["fused"], [25, 75])
        rec["fused_us_iqr"] = round(1e3 * float(q3 - q1), 2)
        if args.scored:
            rec["scored_over_pair_median"] = round(rec["scored_us_median"] / rec["pair_us_median"], 4)
            rec["scored_median_below_pair_median"] = bool(rec["scored_us_median"] < rec["pair_us_median"])
            rec["scored_minus_fused_us_median"] = round(rec["scored_us_median"] - rec["fused_us_median"], 2)
            rec["scored_sum_table_bytes"] = rows * tiles * 4     # the second workspace table: one tile sum per (row, column tile)
            rec["scored_logprob_max_abs_err_sampled"] = lp_err
        res["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        for g in graphs.values():
            g.close()
    if args.compare:
        other = json.load(open(args.compare))
        res["compared_with"] = {"library": other.get("library"), "spread": "interquartile range of this run's `fused` timings of the shape"}
        for name, rec in res["shapes"].items():
            theirs = other["shapes"][name]["fused_us_median"]
            spread = rec["fused_us_iqr"]
            rec["fused_us_median_other_build"] = theirs
            rec["fused_within_3_spreads_of_other_build"] = bool(rec["fused_us_median"] <= theirs + 3 * spread)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
