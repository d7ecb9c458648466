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

With --topk K[,K..] (which implies --scored) every k adds two legs to the same alternation:

    topkK       fused_quantized_linear_topk[_segments](.., K)           -> int32 ids + f32 log-probabilities [rows, K]
    pair_topkK  fused_quantized_linear[_segments] -> topk(.., K)        -> the stored logits read back for their K greatest

and the record (profiles/ctc_head_topk.json) says whether `topkK` stays under its pair, what the extra candidates cost over `scored`, and
what the epilogue's rounds cost a (128-row, 128-column) tile, by subtraction from `fused`.

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
    ap.add_argument("--topk", default=None, help="comma-separated k (1 .. 8): add the k-best head's legs and their pairs; implies --scored")
    ap.add_argument("--compare", default=None, help="the record of another build's run of this tool (taken turn about with this one): "
                    "its `fused` medians are set beside this run's, with whether they lie within three of this run's same-leg spreads")
    ap.add_argument("--merge", default=None, help="no run: take this record of a --topk run and write it to --out with --parents and --resources")
    ap.add_argument("--parents", nargs=3, default=None, metavar=("BEFORE", "BETWEEN", "AFTER"), help="with --merge: the records of three "
                    "--scored runs in turn, the parent build (LELE_HIP_LIBRARY), this build, the parent build -- the same legs in the same "
                    "order, which a --topk run's longer alternation is not: per shape, `fused` and `scored` of this build are set against "
                    "the spread of the two parent runs (their interquartile ranges taken together); three --topk runs of the same K "
                    "add their `topkK` legs")
    ap.add_argument("--resources", default=None, help="with --merge: a JSON file of the compiler's resource-usage remarks, embedded as build_resources")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--packed-count", type=int, default=32)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repeats a leg"
    ks = [int(v) for v in args.topk.split(",")] if args.topk else []
    assert all(1 <= k <= 8 for k in ks), "--topk: k in 1 .. 8"
    args.scored = args.scored or bool(ks)
    args.out = args.out or os.path.join(ROOT, "profiles", "ctc_head_topk.json" if ks or args.merge else
                                        "ctc_head_scored.json" if args.scored else "ctc_head.json")
    if args.merge:
        res = json.load(open(args.merge))
        if args.parents:
            runs = [json.load(open(p)) for p in (args.parents[0], args.parents[2])]
            mine = json.load(open(args.parents[1]))
            res["parent_build"] = {"library": runs[0].get("library"), "this_build": mine.get("library"),
                                   "order": "parent, this build, parent: three processes of one session with the same legs",
                                   "spread": "from the least first quartile to the greatest third quartile of the two parent runs' timings"}
            for name, rec in res["shapes"].items():
                # ... and the `topkK` legs, where all three runs were --topk runs of the same K (the same alternation again)
                ks = [k for k in range(1, 9) if all("topk%d_us_q1" % k in r["shapes"][name] for r in runs + [mine])]
                for leg in ["fused", "scored"] + ["topk%d" % k for k in ks]:
                    a, b = (r["shapes"][name] for r in runs)
                    lo, hi = min(a[leg + "_us_q1"], b[leg + "_us_q1"]), max(a[leg + "_us_q3"], b[leg + "_us_q3"])
                    med = mine["shapes"][name][leg + "_us_median"]
                    rec[leg + "_us_median_parent_runs"] = [a[leg + "_us_median"], b[leg + "_us_median"]]
                    rec[leg + "_us_parent_spread"] = [lo, hi]
                    rec[leg + "_us_median_same_legs"] = med
                    rec[leg + "_median_inside_parent_spread"] = bool(lo <= med <= hi)
                    rec[leg + "_median_not_above_parent_spread"] = bool(med <= hi)
        if args.resources:
            res["build_resources"] = json.load(open(args.resources))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return

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
    ids_topk, lp_topk, val_pair, idx_pair = ({k: ctx.buf() for k in ks} for _ in range(4))

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
        for k in ks:
            if offsets is None:
                legs["topk%d" % k] = lambda k=k: K.fused_quantized_linear_topk(x, *w, k, out_ids=ids_topk[k], out_logprob=lp_topk[k], ctx=ctx)
            else:
                legs["topk%d" % k] = lambda k=k: K.fused_quantized_linear_topk_segments(x, offsets, *w, k, out_ids=ids_topk[k],
                                                                                        out_logprob=lp_topk[k], ctx=ctx)
        lg = legs["linear"]()
        for k in ks:
            legs["pair_topk%d" % k] = lambda k=k: (legs["linear"](), K.topk(lg, k, out_values=val_pair[k], out_indices=idx_pair[k], ctx=ctx))
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
        topk_err = {}
        for k in ks:   # against the stored logits of the pair: slot 0 is the scored head bit for bit, a sample of rows in float64
            for _ in range(2):
                ti, tl = legs["topk%d" % k]()
                legs["pair_topk%d" % k]()
                ti, tl = ti.numpy().reshape(rows, k), tl.numpy().reshape(rows, k)
            assert np.array_equal(ti[:, 0], si.reshape(-1)), "%s: slot 0 of topk%d is not the scored id" % (name, k)
            assert np.array_equal(tl[:, 0].view(np.uint32), sl.reshape(-1).view(np.uint32)), "%s: slot 0 of topk%d is not the scored log-probability" % (name, k)
            step = max(1, rows // 64)
            v32 = lg.numpy().reshape(rows, VOCAB)[::step]
            want = (VOCAB - 1 - np.argsort(-v32[:, ::-1], axis=-1, kind="stable")[:, :k]).astype(np.int32)
            assert np.array_equal(ti[::step], want), "%s: topk%d ids are not the stored logits' k greatest" % (name, k)
            v = v32.astype(np.float64)
            mx = v.max(axis=1, keepdims=True)
            ref = np.take_along_axis(v, want.astype(np.int64), axis=1) - (mx + np.log(np.exp(v - mx).sum(axis=1, keepdims=True)))
            topk_err[k] = float(np.max(np.abs(tl[::step].astype(np.float64) - ref) - 2.0 ** -22 * np.abs(ref)))
            assert topk_err[k] <= 1e-5, "%s: topk%d log-probabilities off by %g" % (name, k, topk_err[k])
        ctx.sync()
        graphs = {}
        # `scored` right behind `fused`: the leg that runs in front of `fused` is `argmax` with and without it
        for leg in ("fused",) + (("scored",) if args.scored else ()) + tuple("topk%d" % k for k in ks) + ("pair", "linear", "argmax") + tuple(
                "pair_topk%d" % k for k in ks):
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
            rec[leg + "_us_q1"], rec[leg + "_us_q3"] = (round(1e3 * float(q), 2) for q in np.percentile(v, [25, 75]))
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
        for k in ks:
            t, pr = rec["topk%d_us_median" % k], rec["pair_topk%d_us_median" % k]
            rec["topk%d_over_pair_median" % k] = round(t / pr, 4)
            rec["topk%d_median_below_pair_median" % k] = bool(t < pr)
            rec["topk%d_minus_scored_us_median" % k] = round(t - rec["scored_us_median"], 2)
            rec["topk%d_minus_fused_us_median" % k] = round(t - rec["fused_us_median"], 2)
            # the k rounds and the wider finish against the one round of `fused`, spread over the launch's (row tile, column tile) pairs
            rec["topk%d_minus_fused_ns_per_tile" % k] = round(1e3 * (t - rec["fused_us_median"]) / (((rows + 127) // 128) * tiles), 3)
            rec["topk%d_workspace_bytes" % k] = rows * tiles * (8 * k + 4)
            rec["topk%d_logprob_max_excess_over_2p-22_rel_sampled" % k] = topk_err[k]
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
