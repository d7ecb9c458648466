#!/usr/bin/env python3
"""kernels.image_preprocess_batch and kernels.yolo_seg_postprocess_sized against what they replace, old and new alternating in one
process on the same seeded, device-resident inputs:

  equal_300 / equal_20   64 images of 640 x 640 over a 160 x 160 mask, all 300 queries kept (bench.py's case) / about 20 an image:
                         the sized call against ONE yolo_seg_postprocess call on the same batch
  mixed                  64 images of sizes drawn from 640 x 480 .. 1920 x 1080, about 20 kept an image: the sized call (and its
                         masks=False form) against the loop of 64 yolo_seg_postprocess calls
  preprocess             image_preprocess_batch on those 64 images against the loop of 64 image_preprocess calls

Every row: the median of --samples windows, each window about --window-ms of calls between two device synchronisations, with min
and max (the spread); the results of old and new are compared (`equal`) at the timed sizes; the work each form does is counted from the shapes and
the boxes (pixel x detection pairs against cells inside the boxes' cell rectangles).  Writes one JSON.

    python tools/yolo_batch_bench.py --out profiles/yolo_batch_bench.json [--samples 11] [--window-ms 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F = np.float32


def window(fn, ctx, calls):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def alternate(fns, ctx, samples, window_ms, warmup):
    """fns: {name: callable}; one window of each in turn, `samples` times over: every form sees the same neighbours on the machine.
    A form's window holds as many calls as fill about window_ms (sized from a trial window after the warm-up)."""
    calls = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        calls[k] = max(3, int(window_ms / max(window(fn, ctx, 3), 1e-3)))
    out = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            out[k].append(window(fn, ctx, calls[k]))
    return {k: dict(stats(v), calls_per_window=calls[k]) for k, v in out.items()}


def make_logits(rng, images, kept):
    """[images, 300, 38]: `kept` queries an image pass threshold 0.25 with random boxes (640-space, 40 .. 240 wide), the rest do not"""
    lg = np.zeros((images, 300, 38), F)
    lg[:, :, 4] = rng.random((images, 300)) * 0.2
    for n in range(images):
        rows = rng.choice(300, kept, replace=False)
        xy = rng.random((kept, 2)) * 400
        lg[n, rows, 0:2] = xy
        lg[n, rows, 2:4] = xy + 40 + rng.random((kept, 2)) * 200
        lg[n, rows, 4] = 0.55 + rng.random(kept) * 0.45
        lg[n, rows, 5] = rng.integers(0, 80, kept)
        lg[n, rows, 6:] = rng.standard_normal((kept, 32))
    return lg


def count_work(dets, counts, sizes, side):
    """(pixel x detection pairs the per-pixel loop evaluates, cells inside the boxes' cell rectangles), summed over the batch"""
    pairs = cells = 0
    for d, c, (w, h) in zip(dets, counts, sizes):
        b = d[:int(c), :4].astype(np.float64)
        lo = np.ceil(b[:, :2])
        hi = np.minimum(np.floor(b[:, 2:]), [w - 1, h - 1])
        ok = (lo <= hi).all(axis=1)
        lo, hi = lo[ok], hi[ok]
        pairs += int(((hi - lo + 1).prod(axis=1)).sum())
        sc = np.array([F(side) / F(w), F(side) / F(h)], F)
        clo = np.minimum(np.floor((lo.astype(F) + F(0.5)) * sc), side - 1)
        chi = np.minimum(np.floor((hi.astype(F) + F(0.5)) * sc), side - 1)
        cells += int(((chi - clo + 1).prod(axis=1)).sum())
    return pairs, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--mask", type=int, default=160)
    args = ap.parse_args()

    import lele_amd
    from lele_amd import apps, kernels as K

    ctx = lele_amd.default_ctx(0)
    rng = np.random.default_rng(0)
    n, side = args.images, args.mask
    res = {"images": n, "mask": [side, side], "samples": args.samples, "warmup": args.warmup, "window_ms": args.window_ms, "threshold": 0.25, "cases": {}}
    feat_host = (rng.standard_normal((n, 32, side, side)) * 0.5).astype(F)
    feat = ctx.buf().upload(feat_host)
    bufs = [ctx.buf() for _ in range(8)]

    # ---- (i) equal sizes: one parent call against one sized call
    sizes = [(640, 640)] * n
    for name, kept in (("equal_300", 300), ("equal_20", 20)):
        logits = ctx.buf().upload(make_logits(rng, n, kept))
        old = lambda: K.yolo_seg_postprocess(logits, feat, 640, 640, 0.25, 80, out_dets=bufs[0], out_count=bufs[1], out_mask=bufs[2], ctx=ctx)  # noqa: E731
        new = lambda: K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.25, 80, out_dets=bufs[3], out_count=bufs[4], out_mask=bufs[5], ctx=ctx)  # noqa: E731
        od, oc, om = old()
        nd, nc, nm, _ = new()
        equal = bool(np.array_equal(od.numpy(), nd.numpy()) and np.array_equal(oc.numpy(), nc.numpy()) and
                     np.array_equal(om.numpy().reshape(-1), nm.numpy()))
        pairs, cells = count_work(nd.numpy(), nc.numpy(), sizes, side)
        case = alternate({"parent_one_call": old, "sized": new}, ctx, args.samples, args.window_ms, args.warmup)
        case.update(kept_per_image=kept, equal=equal, pixel_detection_pairs=pairs, cells_in_rectangles=cells,
                    mask_bytes=n * 640 * 640, table_bytes=40 * n * (side * side + 1280),
                    sized_over_parent=round(case["sized"]["median_ms"] / case["parent_one_call"]["median_ms"], 3))
        res["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        logits.buf.close()

    # ---- (ii) mixed sizes: the loop of per-image parent calls against one sized call
    sizes = [(int(rng.integers(640, 1921)), int(rng.integers(480, 1081))) for _ in range(n)]
    lg_host = make_logits(rng, n, 20)
    logits = ctx.buf().upload(lg_host)
    lg_each = [ctx.buf().upload(lg_host[i:i + 1]) for i in range(n)]
    ft_each = [ctx.buf().upload(feat_host[i:i + 1]) for i in range(n)]

    def old_loop():
        for i, (w, h) in enumerate(sizes):
            K.yolo_seg_postprocess(lg_each[i], ft_each[i], w, h, 0.25, 80, out_dets=bufs[0], out_count=bufs[1], out_mask=bufs[2], ctx=ctx)

    new = lambda: K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.25, 80, out_dets=bufs[3], out_count=bufs[4], out_mask=bufs[5], ctx=ctx)  # noqa: E731
    nomask = lambda: K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.25, 80, out_dets=bufs[3], out_count=bufs[4], masks=False, ctx=ctx)  # noqa: E731
    nd, nc, nm, moff = new()
    masks = apps.unpack_masks(nm, moff, sizes)
    equal = True
    for i, (w, h) in enumerate(sizes):
        od, oc, om = K.yolo_seg_postprocess(lg_each[i], ft_each[i], w, h, 0.25, 80, out_dets=bufs[0], out_count=bufs[1], out_mask=bufs[2], ctx=ctx)
        equal = equal and bool(np.array_equal(od.numpy(), nd.numpy()[i]) and oc.numpy()[0] == nc.numpy()[i] and np.array_equal(om.numpy(), masks[i]))
    pairs, cells = count_work(nd.numpy(), nc.numpy(), sizes, side)
    case = alternate({"parent_loop": old_loop, "sized": new, "sized_no_masks": nomask}, ctx, args.samples, args.window_ms, args.warmup)
    case.update(kept_per_image=20, equal=equal, pixel_detection_pairs=pairs, cells_in_rectangles=cells,
                mask_bytes=int(moff[-1]), table_bytes=40 * sum(side * side + w + h for w, h in sizes),
                sized_over_parent=round(case["sized"]["median_ms"] / case["parent_loop"]["median_ms"], 3))
    res["cases"]["mixed"] = case
    print("mixed", json.dumps(case), flush=True)

    # ---- (iii) preprocess: the loop of per-image calls against one batch call
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    data_host, off, hs, ws = apps.pack_images(imgs)
    data = ctx.buf().upload(data_host)
    each = [ctx.buf().upload(im) for im in imgs]

    def pre_loop():
        for t in each:
            K.image_preprocess(t, 640, out=bufs[6], ctx=ctx)

    pre_new = lambda: K.image_preprocess_batch(data, off, hs, ws, 640, out=bufs[7], ctx=ctx)  # noqa: E731
    got = pre_new().numpy()
    equal = all(np.array_equal(got[i], K.image_preprocess(each[i], 640, out=bufs[6], ctx=ctx).numpy()[0]) for i in range(n))
    case = alternate({"parent_loop": pre_loop, "batch": pre_new}, ctx, args.samples, args.window_ms, args.warmup)
    case.update(equal=bool(equal), source_bytes=int(data_host.size), out_bytes=n * 3 * 640 * 640 * 4,
                batch_over_parent=round(case["batch"]["median_ms"] / case["parent_loop"]["median_ms"], 3))
    res["cases"]["preprocess"] = case
    print("preprocess", json.dumps(case), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
