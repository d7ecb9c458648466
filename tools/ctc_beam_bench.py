#!/usr/bin/env python3
"""CTC prefix beam search on the device against the way the parent commit had to do it, on the candidates of the k-best head of the CTC
projection ([rows, 512] x [512, 25055]); every utterance behind 4 prompt rows (skip_rows = 4), nbest = beam:

    search       ctc_beam_search_segments on candidates that already lie on the device                       (recorded hipGraph)
    head_search  fused_quantized_linear_topk_segments -> ctc_beam_search_segments, one graph                  (recorded hipGraph)
    topk         the k-best head alone                                                                        (recorded hipGraph)
    scored       the scored greedy head, for scale                                                            (recorded hipGraph)
    host         the parent commit's way: the candidates copied to the host, apps.ctc_prefix_beam_search looped over the
                 utterances                                                                                   (wall clock)

Shapes 32 x 171, 64 x 171, 1 x 504 and one packed layout of 32 utterances of 20 .. 504 rows; (k, beam) = (4, 4) and (4, 8) everywhere
and (8, 8) once, at 32 x 171.  The method of tools/ctc_head_bench.py: one timing of a graph leg is hipEvents around `steps` warmed
replays, the graph legs of a shape alternate `reps` (>= 20) times in one process, medians are reported.  The host leg runs `host_reps`
times in the same process (one run takes 0.1 .. 3 s, a thousand times the others, so its spread does not matter to the ratio).  Before
anything is timed the device's sequences are compared with the host's.  The per-frame cost is search / frames of the longest utterance:
that dependent chain is the kernel's bound.  One JSON record goes to --out (profiles/ctc_beam.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, VOCAB, SKIP = 512, 25055, 4
DENSE = [(32, 171), (64, 171), (1, 504)]
CONFIGS = [(4, 4), (4, 8)]
ONCE = ("dense_32x171", (8, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--packed-count", type=int, default=32)
    ap.add_argument("--resources", default=None, help="a JSON file of the compiler's resource-usage remarks, embedded as build_resources")
    ap.add_argument("--heads", nargs=3, default=None, metavar=("BEFORE", "THIS", "AFTER"), help="no run: add `heads_vs_parent` to the record at "
                    "--out from three records of tools/ctc_head_bench.py --scored taken in turn -- the parent build (LELE_HIP_LIBRARY), this "
                    "build, the parent build: the ids-only and scored heads of this build against the two parent runs' interquartile ranges")
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repeats a leg"
    if args.heads:
        before, mine, after = (json.load(open(f))["shapes"] for f in args.heads)
        res = json.load(open(args.out))
        res["heads_vs_parent"] = {"order": "parent build, this build, parent build: three processes of tools/ctc_head_bench.py --scored in one session",
                                  "shapes": {}}
        for name in mine:
            rec = {}
            for leg in ("fused", "scored"):
                a, b = before[name], after[name]
                lo, hi = min(a[leg + "_us_q1"], b[leg + "_us_q1"]), max(a[leg + "_us_q3"], b[leg + "_us_q3"])
                med = mine[name][leg + "_us_median"]
                rec[leg] = {"parent_runs_us_median": [a[leg + "_us_median"], b[leg + "_us_median"]], "this_build_us_median": med,
                            "parent_spread_q1_q3": [lo, hi], "inside_parent_spread": bool(lo <= med <= hi)}
            res["heads_vs_parent"]["shapes"][name] = rec
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return

    import lele_amd
    from lele_amd import kernels as K
    from lele_amd.apps import beam_results, ctc_prefix_beam_search
    from sensevoice_graph import QLinear

    ctx = lele_amd.default_ctx(0)
    rng = np.random.default_rng(args.seed)
    p = QLinear(rng, D, VOCAB, K.Weight)
    w = (p.w, p.scale, p.zero, p.bias)
    lengths = [int(v) for v in rng.integers(20, 505, size=args.packed_count)]
    shapes = [("dense_%dx%d" % s, np.arange(s[0] + 1, dtype=np.int64) * s[1]) for s in DENSE]
    shapes.append(("packed_%d_mixed" % args.packed_count, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)))
    ids_buf, lp_buf, ids_sc, lp_sc = (ctx.buf() for _ in range(4))
    hyp = [ctx.buf() for _ in range(4)]

    res = {"device": "MI355X (gfx950)", "k_dim": D, "n": VOCAB, "skip_rows": SKIP, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "host_reps": args.host_reps, "seed": args.seed, "packed_lengths": lengths,
           "timing": "graph legs: hipEvents around `steps` warmed hipGraph replays, alternating, `reps` times, medians; host leg: wall clock of "
                     "the device-to-host copy of the candidates plus the loop over utterances, `host_reps` times, median", "shapes": {}}
    if args.resources:
        res["build_resources"] = json.load(open(args.resources))
    for name, off in shapes:
        rows, count = int(off[-1]), len(off) - 1
        frames = [max(int(off[i + 1] - off[i]) - SKIP, 0) for i in range(count)]
        x = ctx.buf().upload(rng.standard_normal((rows, D)).astype(np.float32))
        for k, beam in CONFIGS + ([ONCE[1]] if name == ONCE[0] else []):
            head = lambda: K.fused_quantized_linear_topk_segments(x, off, *w, k, out_ids=ids_buf, out_logprob=lp_buf, ctx=ctx)  # noqa: E731
            cand = head()
            search = lambda: K.ctc_beam_search_segments(cand[0], cand[1], off, 0, beam, beam, SKIP, 0, out_tokens=hyp[0], out_lengths=hyp[1],  # noqa: E731
                                                        out_scores=hyp[2], out_counts=hyp[3], ctx=ctx)
            legs = {"search": search, "head_search": lambda: (head(), search()), "topk": head,
                    "scored": lambda: K.fused_quantized_linear_argmax_logprob_segments(x, off, *w, out_ids=ids_sc, out_logprob=lp_sc, ctx=ctx)}

            def host():
                ci, cl = cand[0].numpy(), cand[1].numpy()
                return [ctc_prefix_beam_search(ci[off[i] + SKIP:off[i + 1]], cl[off[i] + SKIP:off[i + 1]], 0, beam, beam) for i in range(count)]

            for _ in range(2):   # eagerly first: weights packed, buffers and the scratch block at their final size, the layout's table staged
                for leg in legs.values():
                    leg()
            got = beam_results(*(o.numpy() for o in search()))
            host_ms = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                want = host()
                host_ms.append(1e3 * (time.perf_counter() - t0))
            same = [[s for s, _ in g] == [s for s, _ in h] for g, h in zip(got, want)]
            err = max((abs(a[1] - b[1]) for g, h in zip(got, want) for a, b in zip(g, h) if np.isfinite(b[1])), default=0.0)
            ctx.sync()
            graphs = {}
            for leg in legs:
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
            rec = {"rows": rows, "segments": count, "k": k, "beam": beam, "nbest": beam, "longest_frames": max(frames), "frames_total": sum(frames)}
            for leg, v in ms.items():
                rec[leg + "_us_median"] = round(1e3 * float(np.median(v)), 2)
                rec[leg + "_us_min"], rec[leg + "_us_max"] = round(1e3 * min(v), 2), round(1e3 * max(v), 2)
                rec[leg + "_us_q1"], rec[leg + "_us_q3"] = (round(1e3 * float(q), 2) for q in np.percentile(v, [25, 75]))
            rec["host_us_median"] = round(1e3 * float(np.median(host_ms)), 1)
            rec["host_us_min"], rec["host_us_max"] = round(1e3 * min(host_ms), 1), round(1e3 * max(host_ms), 1)
            rec["host_over_search_median"] = round(rec["host_us_median"] / rec["search_us_median"], 1)
            rec["search_below_host"] = bool(rec["search_us_median"] < rec["host_us_median"])
            rec["search_us_per_frame_of_longest"] = round(rec["search_us_median"] / max(max(frames), 1), 3)
            rec["search_over_topk_median"] = round(rec["search_us_median"] / rec["topk_us_median"], 3)
            rec["search_costs_more_than_the_head"] = bool(rec["search_us_median"] > rec["topk_us_median"])
            rec["head_search_minus_topk_us_median"] = round(rec["head_search_us_median"] - rec["topk_us_median"], 2)
            rec["segments_with_the_hosts_sequences"] = int(sum(same))
            rec["score_max_abs_diff_from_host"] = float(err)
            rec["trie_workspace_bytes"] = count * (1 + beam * max(frames)) * 8
            res["shapes"]["%s_k%d_beam%d" % (name, k, beam)] = rec
            print(name, json.dumps(rec), flush=True)
            for g in graphs.values():
                g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
