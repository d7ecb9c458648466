#!/usr/bin/env python3
"""features.Resampler / ResamplerStream at 8 -> 16, 44.1 -> 16 and 48 -> 16 kHz, both modes, two rows each:

  batch   32 utterances of 10 s in one compute_segments call
  live    256 streams, one 100 ms tick: ResamplerStream.push followed by FrontendStream.push on what it returns

and, taken in the same run with the same windows, what each row is measured against:

  copy_ms       a device-to-device hipMemcpyAsync of the row's OUTPUT bytes on the context's stream (the yardstick of "linear")
  host_ms       the numpy form of the same work (apps.resample_linear / apps.resample_fir per utterance or chunk), one timing
  frontend_ms   the front-end call that follows (compute_segments on the batch's result; in the live row FrontendStream.push alone,
                timed as pair - resampler push)

PCM is device-resident.  Medians of --samples windows of --calls calls, every window ending in a synchronise.  Writes one JSON.

    python tools/resample_bench.py --out profiles/resample.json [--samples 15] [--calls 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TO = 16000
RATES = [8000, 44100, 48000]


def windows(fn, ctx, samples, calls):
    out = []
    for _ in range(samples):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tick-ms", type=int, default=100)
    args = ap.parse_args()

    import lele_amd
    from lele_amd import _lib, apps, kernels as K
    from lele_amd.features import FrontendStream, Resampler, ResamplerStream, SenseVoiceFrontend

    ctx = lele_amd.default_ctx(0)
    fe = SenseVoiceFrontend(ctx=ctx)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = _lib.lib().lele_hip_ctx_stream(ctx._h)
    rng = np.random.default_rng(0)
    res = {"samples": args.samples, "calls_per_sample": args.calls, "warmup": args.warmup, "cases": {}}
    for mode in ("linear", "sinc"):
        for fr in RATES:
            rs = Resampler(fr, TO, mode, ctx=ctx)
            tab, L, M = rs.table()

            def host(x, rs=rs, tab=tab, L=L, M=M, fr=fr, mode=mode):
                return apps.resample_linear(x, fr, TO) if mode == "linear" else apps.resample_fir(x, tab, L, M)

            # ---- batch: 32 x 10 s
            n = fr * args.seconds
            x = (0.3 * rng.uniform(-1, 1, args.batch * n)).astype(np.float32)
            b_pcm, o_rs, o_fe, o_cp = ctx.buf(), ctx.buf(), ctx.buf(), ctx.buf()
            pcm = b_pcm.upload(x)
            segs = [(i * n, (i + 1) * n) for i in range(args.batch)]
            y, ysegs = rs.compute_segments(pcm, segs, out=o_rs)
            route = K.last_route(ctx)
            out_bytes = int(ysegs[-1][1]) * 4
            o_cp.reserve(out_bytes)

            def run_rs():
                rs.compute_segments(pcm, segs, out=o_rs)

            def run_fe():
                fe.compute_segments(y, ysegs, out=o_fe)

            def run_copy():
                hip.hipMemcpyAsync(C.c_void_p(o_cp.ptr), C.c_void_p(o_rs.ptr), C.c_size_t(out_bytes), C.c_int(3), C.c_void_p(stream))

            for _ in range(args.warmup):
                run_rs(), run_fe(), run_copy()
            a, b, c = [], [], []
            for _ in range(args.samples):     # alternating: all three see the same neighbours on the machine
                a += windows(run_rs, ctx, 1, args.calls)
                c += windows(run_copy, ctx, 1, args.calls)
                b += windows(run_fe, ctx, 1, args.calls)
            t0 = time.perf_counter()
            for s, e in segs:
                host(x[s:e])
            host_ms = (time.perf_counter() - t0) * 1e3
            case = dict(mode=mode, from_rate=fr, to_rate=TO, route=route, utterances=args.batch, seconds=args.seconds, out_bytes=out_bytes,
                        resample_ms=med(a), resample_ms_min=round(min(a), 4), resample_ms_max=round(max(a), 4), copy_ms=med(c),
                        copy_ms_min=round(min(c), 4), frontend_ms=med(b), host_ms=round(host_ms, 2))
            case["resample_over_copy"] = round(case["resample_ms"] / case["copy_ms"], 3)
            res["cases"]["%s_%d_batch" % (mode, fr)] = case
            print("%s_%d_batch" % (mode, fr), json.dumps(case), flush=True)
            for bf in (b_pcm, o_rs, o_fe, o_cp):
                bf.close()

            # ---- live: 256 streams, one 100 ms tick, then FrontendStream.push
            chunk = fr * args.tick_ms // 1000
            ns = args.streams
            xl = (0.3 * rng.uniform(-1, 1, ns * chunk)).astype(np.float32)
            b_pcm = ctx.buf()
            pcm = b_pcm.upload(xl)
            starts = np.arange(ns, dtype=np.int64) * chunk
            lengths = np.full(ns, chunk, np.int64)
            st = ResamplerStream(rs, ns, chunk)
            fs = FrontendStream(fe, ns, rs.out_len(chunk) + 64)
            o_cp = ctx.buf()

            def push_rs():
                return st.push((pcm, starts, lengths))

            def push_pair():
                fs.push(push_rs())

            for _ in range(args.warmup):
                push_pair()
            tv, _, ol = push_rs()
            route = K.last_route(ctx)
            out_bytes = int(ol.sum()) * 4
            o_cp.reserve(out_bytes)

            def run_copy_live():
                hip.hipMemcpyAsync(C.c_void_p(o_cp.ptr), C.c_void_p(st._out.ptr), C.c_size_t(out_bytes), C.c_int(3), C.c_void_p(stream))

            a, b, c = [], [], []
            for _ in range(args.samples):
                a += windows(push_rs, ctx, 1, args.calls)
                c += windows(run_copy_live, ctx, 1, args.calls)
                b += windows(push_pair, ctx, 1, args.calls)
            t0 = time.perf_counter()
            for i in range(ns):
                host(xl[i * chunk:(i + 1) * chunk])
            host_ms = (time.perf_counter() - t0) * 1e3
            case = dict(mode=mode, from_rate=fr, to_rate=TO, route=route, streams=ns, tick_ms=args.tick_ms, out_bytes=out_bytes,
                        resample_ms=med(a), resample_ms_min=round(min(a), 4), resample_ms_max=round(max(a), 4), copy_ms=med(c),
                        copy_ms_min=round(min(c), 4), pair_ms=med(b), frontend_ms=round(med(b) - med(a), 4), host_ms=round(host_ms, 2))
            case["resample_over_copy"] = round(case["resample_ms"] / case["copy_ms"], 3)
            res["cases"]["%s_%d_live" % (mode, fr)] = case
            print("%s_%d_live" % (mode, fr), json.dumps(case), flush=True)
            fs.close()
            st.close()
            b_pcm.close()
            o_cp.close()
            rs.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
