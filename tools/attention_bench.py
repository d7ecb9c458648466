#!/usr/bin/env python3
"""Time lele_hip_attention_view at the SenseVoice-shaped sizes (BASELINE configs[2]: 1 x 504 rows, configs[3]: 32 x 171 rows;
4 heads of 128) as the library dispatches it, as the f32 replica, and as the three-call sequence it replaces (with the lab
library also the row-block forms selected by hand).
--long: lele_hip_attention_segments_long on layouts with utterances over 30 s (1 x 1004, 1 x 2004, 8 x 1004 rows, 32 utterances of
1 - 120 s) against the only way there was before it, attention_view per utterance (the three-call sequence past 512 keys), with the
time per (128-row block x 32-key tile) beside the dense one-pass kernel's at 16 x 512; --passes repeats every measurement (spread).
Twenty calls are captured into a hipGraph and its replays timed with HIP events.  Output: one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, DH = 4, 128
QC = [["slice", 2, 0, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
KC = [["slice", 2, 512, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 3, 1]]]
VC = [["slice", 2, 1024, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]


def timed(ctx, call, reps, per_graph=20):
    """ms per call: `per_graph` calls recorded into one graph after an eager run, reps / per_graph warmed replays between two events"""
    call()
    ctx.sync()
    ctx.graph_begin()
    for _ in range(per_graph):
        call()
    gr = ctx.graph_end()
    gr.launch()
    ctx.sync()
    n = max(1, reps // per_graph)
    ctx.timer_start()
    for _ in range(n):
        gr.launch()
    ms = ctx.timer_stop() / (n * per_graph)
    gr.close()
    return ms


def tile_units(lengths):
    """(128-row block x 32-key tile) pairs of one head of every utterance: what the one-pass kernels' time is proportional to"""
    return sum(-(-t // 128) * -(-t // 32) for t in lengths)


def long_rows(args, ctx, K, scale):
    rng = np.random.default_rng(1)
    sec_rows = lambda s: -(-((s * 16000 - 400) // 160 + 1) // 6) + 4   # LFR rows of s seconds + the four prompt rows
    mixed = [int(sec_rows(int(s))) for s in rng.integers(1, 121, size=32)]
    out = {}
    stats = lambda v: {"us_min": round(min(v) * 1e3, 2), "us_median": round(float(np.median(v)) * 1e3, 2), "us_all": [round(x * 1e3, 2) for x in v]}
    for name, lengths in (("1x1004", [1004]), ("1x2004", [2004]), ("8x1004", [1004] * 8), ("32 of 1-120 s", mixed), ("16x512 (short lists)", [512] * 16)):
        if args.only and args.only not in name:
            continue
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        qkv = (rng.standard_normal((int(off[-1]), 1536)) * 1.5).astype(np.float32)
        qd, dst = ctx.buf().upload(qkv), ctx.buf()
        each = [ctx.buf().upload(qkv[off[i]:off[i + 1]][None]) for i in range(len(lengths))]
        outs = [ctx.buf() for _ in lengths]

        def packed():
            K.attention_segments_long(qd, off, H, DH, scale, out=dst, ctx=ctx)

        def loop():   # what a caller had: every utterance alone through the dense call (past 512 keys its three-call sequence)
            for x, o in zip(each, outs):
                K.attention_view(x, QC, x, KC, x, VC, scale, [0, 2, 1, 3], [0, 0, H * DH], out=o, ctx=ctx)

        per = 20 if len(lengths) <= 8 else 4
        ms = {"packed": [], "loop": []}
        for _ in range(args.passes):
            ms["packed"].append(timed(ctx, packed, args.reps, per))
            ms["loop"].append(timed(ctx, loop, max(per, args.reps // 4), per))
        units = H * tile_units(lengths)
        row = {"rows": [int(t) for t in lengths] if len(lengths) > 8 and len(set(lengths)) > 1 else "%d x %d" % (len(lengths), lengths[0]),
               "attention_segments_long": stats(ms["packed"]), "attention_view per utterance": stats(ms["loop"]),
               "loop_min_over_packed_median": round(min(ms["loop"]) / float(np.median(ms["packed"])), 2)}
        if min(lengths) > 512:
            row["block_tiles"] = units
            row["ns_per_block_tile"] = round(float(np.median(ms["packed"])) * 1e6 / units, 2)
        out[name] = row
    # the dense one-pass kernel at 16 x 512: the per-tile cost to hold the long form against
    if not args.only:
        xd, dst = ctx.buf().upload((rng.standard_normal((16, 512, 1536)) * 1.5).astype(np.float32)), ctx.buf()
        v = [timed(ctx, lambda: K.attention_view(xd, QC, xd, KC, xd, VC, scale, [0, 2, 1, 3], [0, 0, H * DH], out=dst, ctx=ctx), args.reps)
             for _ in range(args.passes)]
        assert K.last_route(ctx) == "attn.flash"
        units = 16 * H * tile_units([512])
        out["attn.flash 16x512"] = dict(stats(v), block_tiles=units, ns_per_block_tile=round(float(np.median(v)) * 1e6 / units, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--long", action="store_true", help="the packed call on utterances over 30 s against attention_view per utterance")
    ap.add_argument("--passes", type=int, default=1, help="repeat every measurement this often and report all (run-to-run spread)")
    args = ap.parse_args()
    from lele_amd import kernels as K
    from lele_amd._lib import Ctx, Weight
    ctx = Ctx()
    rng = np.random.default_rng(0)
    scale = Weight(np.array([DH ** -0.5], np.float32))
    if args.long:
        print(json.dumps(long_rows(args, ctx, K, scale), indent=1))
        return
    out = {}
    for name, (b, t) in (("c4 32x171", (32, 171)), ("c3 1x504", (1, 504)), ("8x171", (8, 171)), ("64x171", (64, 171)), ("16x512", (16, 512))):
        qd = ctx.buf().upload((rng.standard_normal((b, t, 1536)) * 1.5).astype(np.float32))
        dst = ctx.buf()
        flops = 2 * 2 * b * H * t * t * DH
        row = {}
        variants = [("default (one pass over the keys for a batch)", {"LELE_HIP_ATTENTION_MIN_BLOCKS": "1"}),
                    ("replica (LELE_HIP_ATTENTION_EXACT=1)", {"LELE_HIP_ATTENTION_MIN_BLOCKS": "1", "LELE_HIP_ATTENTION_EXACT": "1"}),
                    ("sequence", {"LELE_HIP_ATTENTION_FUSED": "0"})]
        if os.environ.get("LELE_HIP_LAB") == "1":  # the row-block forms by hand: lab-only switches
            variants += [("fused rt=1", {"LELE_HIP_ATTENTION_RT": "1", "LELE_HIP_ATTENTION_MIN_BLOCKS": "1", "LELE_HIP_ATTENTION_ROWS": "32"}),
                         ("fused rt=2", {"LELE_HIP_ATTENTION_RT": "2", "LELE_HIP_ATTENTION_MIN_BLOCKS": "1", "LELE_HIP_ATTENTION_ROWS": "32"}),
                         ("fused 16 rows", {"LELE_HIP_ATTENTION_RT": "1", "LELE_HIP_ATTENTION_MIN_BLOCKS": "1", "LELE_HIP_ATTENTION_ROWS": "16"})]
        for label, env in variants:
            if args.only and args.only not in label:
                continue
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                call = lambda: K.attention_view(qd, QC, qd, KC, qd, VC, scale, [0, 2, 1, 3], [0, 0, H * DH], out=dst, ctx=ctx)
                all_ms = [timed(ctx, call, args.reps) for _ in range(args.passes)]
                ms = float(np.median(all_ms))
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            row[label] = {"us": round(ms * 1e3, 2), "tflops_f32": round(flops / ms / 1e9, 2)}
            if args.passes > 1:
                row[label]["us_all"] = [round(x * 1e3, 2) for x in all_ms]
        out[name] = row
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
