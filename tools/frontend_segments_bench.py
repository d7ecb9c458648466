#!/usr/bin/env python3
"""Front-end over variable-length segments (SenseVoiceFrontend.compute_segments) against the equal-length batch and the per-utterance
loop, on device-resident PCM.  Writes one JSON:

  (a) equal:  COUNT x 30 s as contiguous segments   vs  compute_batch on the same buffer ([COUNT, 30 s])
  (b) mixed:  COUNT segments of 1-30 s (seeded lengths, arbitrary starts)  vs  compute() once per segment (asynchronous loop), and the
              sum of per-segment times (each call synchronised)

Algorithmic bytes of a run = 4 * sum(lengths) + 4 * R * 560 (PCM read once, features written once).

    python tools/frontend_segments_bench.py --out profiles/frontend_segments.json [--count 2048] [--steps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 16000


def timed(fn, ctx, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--count", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=3)
    args = ap.parse_args()

    import lele_amd
    from lele_amd import _lib
    from lele_amd import kernels as K
    from lele_amd.features import SenseVoiceFrontend
    from lele_amd.tensor import TensorView

    ctx = lele_amd.default_ctx(0)
    fe = SenseVoiceFrontend(ctx=ctx)
    n30 = 30 * SR
    count = args.count
    # COUNT x 30 s resident in HBM: 64 distinct synthetic utterances tiled on the device (the work does not depend on the samples)
    rng = np.random.default_rng(0)
    distinct = min(64, count)
    t = np.arange(n30) / SR
    base_h = np.stack([(0.3 * np.sin(2 * np.pi * (200 + 10 * i) * t) + 0.05 * rng.uniform(-1, 1, n30)).astype(np.float32)
                       for i in range(distinct)])
    base = ctx.buf().upload(base_h)
    reps = -(-count // distinct)
    pbuf = ctx.buf()
    pcm2 = K.tile(base, [reps, 1], out=pbuf, ctx=ctx)
    ctx.sync()
    pcm2 = TensorView(_lib.DevTensor(pbuf, (count, n30), np.float32))  # the first COUNT rows
    flat = TensorView(_lib.DevTensor(pbuf, (count * n30,), np.float32))
    total = count * n30
    cols = fe.out_rows(n30)[1]
    res = {"count": count, "steps": args.steps, "warmup": args.warmup, "cases": {}}

    def rec(name, ms, samples, rows, **kw):
        b = 4 * samples + 4 * rows * cols
        res["cases"][name] = dict(ms=round(ms, 4), bytes=int(b), gbps=round(b / ms / 1e6, 1), **kw)
        print(name, res["cases"][name], flush=True)

    # (a) equal lengths
    o_b, o_s = ctx.buf(), ctx.buf()
    segs_eq = [(i * n30, (i + 1) * n30) for i in range(count)]
    rows_eq = count * fe.out_rows(n30)[0]
    rec("a_compute_batch", timed(lambda: fe.compute_batch(pcm2, o_b), ctx, args.steps, args.warmup), count * n30, rows_eq)
    rec("a_segments", timed(lambda: fe.compute_segments(flat, segs_eq, o_s), ctx, args.steps, args.warmup), count * n30, rows_eq)

    # (b) mixed lengths, 1-30 s, seeded, arbitrary (unaligned) starts inside the buffer
    r2 = np.random.default_rng(1)
    lens = r2.integers(1 * SR, 30 * SR + 1, size=count)
    starts = r2.integers(0, total - lens + 1)
    segs = [(int(s), int(s + ln)) for s, ln in zip(starts, lens)]
    rows_mx = int(sum(fe.out_rows(int(ln))[0] for ln in lens))
    samples_mx = int(lens.sum())
    rec("b_segments", timed(lambda: fe.compute_segments(flat, segs, o_s), ctx, args.steps, args.warmup), samples_mx, rows_mx)

    lib = _lib.lib()
    sh = _lib.OutShape()
    o_l = ctx.buf()
    keep = []
    tensors = []
    for s, e in segs:  # device views of each segment: LeleTensor straight at the segment's first sample
        shp = (C.c_int64 * 1)(e - s)
        tt = _lib.LeleTensor(C.c_void_p(pbuf.ptr + 4 * s), shp, 1, _lib.F32, _lib.MEM_DEVICE)
        keep.append(shp)
        tensors.append(tt)

    def loop():
        for tt in tensors:
            _lib.check(lib.lele_hip_frontend_compute(fe._h, C.byref(tt), o_l._h, sh.shape, C.byref(sh.rank)))

    rec("b_compute_loop", timed(loop, ctx, args.loop_steps, 1), samples_mx, rows_mx)
    per = 0.0
    for tt in tensors:  # sum of per-segment times: each call on its own, synchronised
        ctx.sync()
        t0 = time.perf_counter()
        _lib.check(lib.lele_hip_frontend_compute(fe._h, C.byref(tt), o_l._h, sh.shape, C.byref(sh.rank)))
        ctx.sync()
        per += time.perf_counter() - t0
    rec("b_sum_of_segments", per * 1e3, samples_mx, rows_mx)

    c = res["cases"]
    res["ratios"] = {
        "a_segments_over_batch_gbps": round(c["a_segments"]["gbps"] / c["a_compute_batch"]["gbps"], 4),
        "b_over_a_gbps": round(c["b_segments"]["gbps"] / c["a_segments"]["gbps"], 4),
        "b_loop_over_segments_time": round(c["b_compute_loop"]["ms"] / c["b_segments"]["ms"], 2),
        "b_sum_over_segments_time": round(c["b_sum_of_segments"]["ms"] / c["b_segments"]["ms"], 2),
    }
    print(json.dumps(res["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
