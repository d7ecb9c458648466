#!/usr/bin/env python3
"""lstm_segments (one launch chain for N independent sequences) against the loop of single lstm calls a caller had before it.
LSTM, I = H = 128 (the Silero class).  Every leg is recorded into ONE hipGraph and timed with events around STEPS warmed replays; the
legs of a case alternate inside one process, REPS times; minimum and median per leg are kept.  Writes one JSON:

  streams:    N in {1, 64, 256, 1024, 4096} streams x T = 1, state in place (row_offsets = 0, 1, .., N)
                packed  lstm_segments once
                loop    min(N, LOOP_CAP) lstm calls back to back, each with its own state buffers; us_per_stream is what is compared
                        (the loop is serial on one stream: its cost per stream does not depend on N)
  sequences:  1 and 32 sequences x T = 175 (the zh.wav chain length)
                packed            lstm_segments, the form the library picks (register-stationary at H = 128)
                packed_streamed   the same call with the streamed form forced -- LAB BUILD ONLY (LELE_HIP_LAB=1 python -m lele_amd.build,
                                  then LELE_HIP_LAB=1 for this tool); absent from the JSON otherwise
                loop              one lstm call per sequence

    python tools/rnn_segments_bench.py --out profiles/rnn_segments.json [--steps 20] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I = H = 128
LOOP_CAP = 256
FORM_SWITCH = "LELE_HIP_RNN_SEG_FORM"   # read by the lab build only (lele_amd/csrc/rnn.hip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 256, 1024, 4096])
    ap.add_argument("--sequences", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--t", type=int, default=175)
    args = ap.parse_args()

    import lele_amd
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView

    lab = os.environ.get("LELE_HIP_LAB", "0") not in ("", "0")
    ctx = lele_amd.default_ctx(0)
    rng = np.random.default_rng(2024)
    sc = np.float32(1.0 / np.sqrt(H))
    dev = lambda a: TensorView(ctx.buf().upload(np.ascontiguousarray(a, np.float32)))   # noqa: E731
    w, r = dev(rng.standard_normal((1, 4 * H, I)) * sc), dev(rng.standard_normal((1, 4 * H, H)) * sc)
    b = dev(rng.standard_normal((1, 8 * H)) * 0.2)

    def packed_leg(n, t, form=None):
        """n sequences of t rows, state in place; -> (callable, info)"""
        x = dev(rng.standard_normal((n * t, I)))
        off = (np.arange(n + 1) * t).astype(np.int64)
        hb, cb, yb = ctx.buf(), ctx.buf(), ctx.buf()
        hv, cv = TensorView(hb.upload(np.zeros((1, n, H), np.float32))), TensorView(cb.upload(np.zeros((1, n, H), np.float32)))
        info = {}

        def fn():
            if form is not None:
                os.environ[FORM_SWITCH] = str(form)
            try:
                K.lstm_segments(x, off, w, r, b, hv, cv, outs=[yb, hb, cb], info=info, ctx=ctx)
            finally:
                os.environ.pop(FORM_SWITCH, None)
        return fn, info

    def loop_leg(n, t):
        xs = [dev(rng.standard_normal((t, 1, I))) for _ in range(n)]
        st = []
        for _ in range(n):
            hb, cb, yb = ctx.buf(), ctx.buf(), ctx.buf()
            st.append((TensorView(hb.upload(np.zeros((1, 1, H), np.float32))), TensorView(cb.upload(np.zeros((1, 1, H), np.float32))), [yb, hb, cb]))

        def fn():
            for x, (hv, cv, outs) in zip(xs, st):
                K.lstm(x, w, r, b, None, hv, cv, outs=outs, ctx=ctx)
        return fn

    def record(fn):
        fn()
        fn()   # twice eagerly: buffers at their final size, the layout's table on the device
        ctx.sync()
        ctx.graph_begin()
        fn()
        return ctx.graph_end()

    def timed(g):
        for _ in range(args.warmup):
            g.launch()
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            g.launch()
        return ctx.timer_stop() / args.steps * 1e3   # us per replay

    def measure(legs):
        """legs: name -> (graph, divisor); alternate, reps times -> name -> {us_min, us_median, ...}"""
        us = {n: [] for n in legs}
        for _ in range(args.reps):
            for n, (g, _) in legs.items():
                us[n].append(timed(g))
        out = {}
        for n, v in us.items():
            d = legs[n][1]
            out[n] = {"us_min": round(min(v), 2), "us_median": round(float(np.median(v)), 2), "us_all": [round(x, 2) for x in v],
                      "units": d, "us_per_unit_min": round(min(v) / d, 3), "us_per_unit_median": round(float(np.median(v)) / d, 3)}
        for g, _ in legs.values():
            g.close()
        return out

    res = {"device": "MI355X (gfx950)", "library": "lab" if lab else "product", "num_cus": K.num_cus(ctx), "I": I, "H": H, "steps": args.steps,
           "warmup": args.warmup, "reps": args.reps, "loop_cap": LOOP_CAP,
           "timing": "hipEvents around `steps` warmed replays of one hipGraph per leg; legs of a case alternate, `reps` times; microseconds",
           "streams": {}, "sequences": {}}
    for n in args.streams:   # (a) a unit is one stream's 1-row chunk
        fn, info = packed_leg(n, 1)
        nl = min(n, LOOP_CAP)
        c = measure({"packed": (record(fn), n), "loop": (record(loop_leg(nl, 1)), nl)})
        c["packed"].update(info)
        c["loop_us_per_stream_min_over_packed_us_per_stream_median"] = round(c["loop"]["us_per_unit_min"] / c["packed"]["us_per_unit_median"], 2)
        res["streams"][str(n)] = c
        print("streams", n, json.dumps(c), flush=True)
    for n in args.sequences:   # (b) a unit is one time step of the chain (all sequences advance together in the packed legs)
        fn, info = packed_leg(n, args.t)
        legs = {"packed": (record(fn), args.t), "loop": (record(loop_leg(n, args.t)), args.t)}
        info2 = None
        if lab:
            fn2, info2 = packed_leg(n, args.t, form=2)
            legs["packed_streamed"] = (record(fn2), args.t)
        c = measure(legs)
        c["packed"].update(info)
        if info2 is not None:
            c["packed_streamed"].update(info2)
            c["register_stationary_faster_than_streamed"] = bool(c["packed"]["us_median"] < c["packed_streamed"]["us_median"])
        c["t"] = args.t
        res["sequences"][str(n)] = c
        print("sequences", n, json.dumps(c), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
