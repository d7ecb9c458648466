#!/usr/bin/env python3
"""One steady-state push of the chunked front-end (lele_amd.features.FrontendStream) for N live streams, against what a host can run
without it: compute_segments on N segments of the same `carry + chunk` samples -- the same frames of log-mel work, with the LFR rows
at every chunk boundary wrong.  (compute_segments' kernels are instruction for instruction the parent commit's, so the baseline is
timed in this process, alternating with the push.)  Writes one JSON:

  cases["N<streams>_<ms>ms"] = push_ms, segments_ms (medians of --samples windows of --pushes calls each, every window ending in a
  synchronise), their ratio, and idle_push_ms: a push of empty chunks, which builds and uploads the per-push table and launches
  nothing -- the host side of every push.  What a push adds to the baseline is that, plus the append, emit and compact launches.

PCM is device-resident; chunks are multiples of the hop, so every push completes the same number of frames and carries 320 samples
(a total that is a multiple of 160 ends 320 samples past the start of the first incomplete frame).

    python tools/frontend_stream_bench.py --out profiles/frontend_stream.json [--samples 21] [--pushes 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 16000


def windows(fn, ctx, samples, pushes):
    """ms per call: `samples` windows of `pushes` calls, each window closed by a synchronise"""
    out = []
    for _ in range(samples):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(pushes):
            fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3 / pushes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--chunk-ms", type=int, nargs="*", default=[100, 600])
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    import lele_amd
    from lele_amd import kernels as K
    from lele_amd.features import FrontendStream, SenseVoiceFrontend

    ctx = lele_amd.default_ctx(0)
    fe = SenseVoiceFrontend(ctx=ctx)
    rng = np.random.default_rng(0)
    res = {"samples": args.samples, "pushes_per_sample": args.pushes, "warmup": args.warmup, "cases": {}}
    for n in args.streams:
        for ms in args.chunk_ms:
            chunk = SR * ms // 1000
            carry = 320   # what a stream carries once it has a frame and is fed multiples of the hop
            seg = carry + chunk
            # one buffer that holds every stream's `carry + chunk` samples: the push reads the last `chunk` of each, the baseline all
            pcm = ctx.buf().upload((0.3 * rng.uniform(-1, 1, n * seg)).astype(np.float32))
            starts = np.arange(n, dtype=np.int64) * seg
            lengths = np.full(n, chunk, np.int64)
            segs = [(int(s), int(s + seg)) for s in starts]
            st = FrontendStream(fe, n, chunk)
            o_seg = ctx.buf()
            idle = (pcm, np.zeros(n, np.int64), np.zeros(n, np.int64))

            def push():
                st.push((pcm, starts + carry, lengths))

            def segments():
                fe.compute_segments(pcm, segs, o_seg)

            for _ in range(args.warmup):
                push()
                segments()
            push()
            route_push = K.last_route(ctx)
            a, b = [], []
            for _ in range(args.samples):   # alternating: both see the same neighbours on the machine
                a += windows(push, ctx, 1, args.pushes)
                b += windows(segments, ctx, 1, args.pushes)
            c = windows(lambda: st.push(idle), ctx, args.samples, args.pushes)
            frames = int(n * (chunk // 160))
            case = dict(streams=n, chunk_samples=chunk, frames_per_push=frames, route=route_push,
                        push_ms=round(statistics.median(a), 4), push_ms_min=round(min(a), 4), push_ms_max=round(max(a), 4),
                        segments_ms=round(statistics.median(b), 4), segments_ms_min=round(min(b), 4), segments_ms_max=round(max(b), 4),
                        idle_push_ms=round(statistics.median(c), 4))
            case["push_over_segments"] = round(case["push_ms"] / case["segments_ms"], 3)
            res["cases"]["N%d_%dms" % (n, ms)] = case
            print("N%d_%dms" % (n, ms), json.dumps(case), flush=True)
            st.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
