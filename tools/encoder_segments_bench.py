#!/usr/bin/env python3
"""The 70-layer SenseVoice-shaped encoder over a packed batch of variable-length utterances (Encoder.forward_segments) against what a
caller had before it.  Every leg is recorded into hipGraphs once and timed with events around STEPS warmed replays; the legs of a
case alternate inside one process, REPS times; minimum and median per leg are kept.  Writes one JSON:

  mixed:  COUNT utterances of 1 - 30 s (seeded lengths)
            packed  forward_segments once                          (one graph)
            loop    Encoder.forward([1, T, 560]) per utterance     (one graph per utterance, launched back to back)
          requirement: median(packed) < min(loop)
  equal:  COUNT x 171 rows (10 s)
            packed  forward_segments                               (one graph)
            dense   Encoder.forward([COUNT, 171, 560])             (one graph)   -- reported, not required
  long:   COUNT utterances of 1 - 120 s (seeded lengths; --long-max-seconds): most of them past the 512 rows the packed attention
          stopped at before lele_hip_attention_segments_long
            packed  forward_segments once                          (one graph)
            loop    Encoder.forward([1, T, 560]) per utterance     (past 512 rows its attention is the three-call sequence)
          requirement: median(packed) < min(loop)

    python tools/encoder_segments_bench.py --out profiles/encoder_segments_mi355x.json [--layers 70] [--count 32] [--steps 20] [--reps 5]
    python tools/encoder_segments_bench.py --eager equal_packed --runs 4     # no graphs, no timing: a leg to put under rocprofv3
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SR = 16000


def lfr_rows(samples):
    frames = (samples - 400) // 160 + 1
    return -(-frames // 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=70)
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--long-max-seconds", type=int, default=120)
    ap.add_argument("--cases", default="mixed,equal,long")
    ap.add_argument("--eager", default=None, choices=["mixed_packed", "mixed_loop", "equal_packed", "equal_dense", "long_packed", "long_loop"])
    ap.add_argument("--runs", type=int, default=4)
    args = ap.parse_args()

    import lele_amd
    from sensevoice_graph import Encoder

    ctx = lele_amd.default_ctx(0)
    enc = Encoder(ctx, args.layers, damped=True)
    rng = np.random.default_rng(args.seed)
    seconds = rng.integers(1, 31, size=args.count)
    rows = [int(lfr_rows(int(s) * SR)) for s in seconds]
    off_mixed = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    off_equal = (np.arange(args.count + 1) * 171).astype(np.int64)
    f_mixed = rng.standard_normal((int(off_mixed[-1]), 560)).astype(np.float32)
    f_equal = rng.standard_normal((args.count * 171, 560)).astype(np.float32)
    d_mixed, d_equal = ctx.buf().upload(f_mixed), ctx.buf().upload(f_equal)
    d_dense = ctx.buf().upload(f_equal.reshape(args.count, 171, 560))
    d_each = [ctx.buf().upload(f_mixed[off_mixed[i]:off_mixed[i + 1]][None]) for i in range(args.count)]
    long_seconds = rng.integers(1, args.long_max_seconds + 1, size=args.count)
    long_rows = [int(lfr_rows(int(s) * SR)) for s in long_seconds]
    off_long = np.concatenate([[0], np.cumsum(long_rows)]).astype(np.int64)
    f_long = rng.standard_normal((int(off_long[-1]), 560)).astype(np.float32)
    d_long = ctx.buf().upload(f_long)
    d_long_each = [ctx.buf().upload(f_long[off_long[i]:off_long[i + 1]][None]) for i in range(args.count)]

    legs = {
        "mixed_packed": [lambda: enc.forward_segments(d_mixed, off_mixed)],
        "mixed_loop": [(lambda t=t: enc.forward(t)) for t in d_each],
        "equal_packed": [lambda: enc.forward_segments(d_equal, off_equal)],
        "equal_dense": [lambda: enc.forward(d_dense)],
        "long_packed": [lambda: enc.forward_segments(d_long, off_long)],
        "long_loop": [(lambda t=t: enc.forward(t)) for t in d_long_each],
    }
    cases = [c for c in args.cases.split(",") if c]
    legs = {n: f for n, f in legs.items() if n.split("_")[0] in cases or n == args.eager}
    if args.eager:
        for _ in range(args.runs):
            for fn in legs[args.eager]:
                fn()
        ctx.sync()
        print(json.dumps({"eager": args.eager, "runs": args.runs, "layers": args.layers}))
        return

    # every sequence eagerly first (twice): weights packed, the workspace at its final size, the layouts' tables on the device --
    # nothing a recorded graph has baked in is re-allocated afterwards
    for _ in range(2):
        for fns in legs.values():
            for fn in fns:
                fn()
    ctx.sync()
    graphs = {}
    for name, fns in legs.items():
        graphs[name] = []
        for fn in fns:
            ctx.graph_begin()
            fn()
            graphs[name].append(ctx.graph_end())

    def run(name):
        for g in graphs[name]:
            g.launch()

    def timed(name):
        for _ in range(args.warmup):
            run(name)
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            run(name)
        return ctx.timer_stop() / args.steps

    res = {"device": "MI355X (gfx950)", "layers": args.layers, "count": args.count, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "seed": args.seed, "timing": "hipEvents around `steps` warmed hipGraph replays; legs of a case alternate, `reps` times",
           "mixed_seconds": [int(s) for s in seconds], "mixed_rows": rows, "mixed_rows_total": int(off_mixed[-1]),
           "equal_rows_total": int(off_equal[-1]), "long_seconds": [int(s) for s in long_seconds], "long_rows": long_rows,
           "long_rows_total": int(off_long[-1]), "cases": {}}
    for case, pair in (("mixed", ("mixed_packed", "mixed_loop")), ("equal", ("equal_packed", "equal_dense")), ("long", ("long_packed", "long_loop"))):
        if case not in cases:
            continue
        ms = {n: [] for n in pair}
        for _ in range(args.reps):
            for n in pair:
                ms[n].append(timed(n))
        c = {n: {"ms_min": round(min(v), 4), "ms_median": round(float(np.median(v)), 4), "ms_all": [round(x, 4) for x in v],
                 "graphs_per_pass": len(graphs[n])} for n, v in ms.items()}
        a, b = pair
        c["ratio_%s_min_over_%s_median" % (b.split("_")[1], a.split("_")[1])] = round(c[b]["ms_min"] / c[a]["ms_median"], 3)
        if case in ("mixed", "long"):
            c["packed_median_below_loop_min"] = bool(c[a]["ms_median"] < c[b]["ms_min"])
        res["cases"][case] = c
        print(case, json.dumps(c), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for gs in graphs.values():
        for g in gs:
            g.close()


if __name__ == "__main__":
    main()
