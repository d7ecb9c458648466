#!/usr/bin/env python3
"""Same kernels, same geometry, same bytes: the convolution dispatch of two builds of the library, call by call (the pattern of
tools/quant_dispatch_ab.py, whose trace reader and comparison this tool uses).

  run      (on the GPU, once per library, under `rocprofv3 --kernel-trace` as tools/ktrace.sh runs it, nothing else collected;
           LELE_HIP_LIBRARY picks the build) issues ONE call per row and prints one JSON line per row with the route the library
           reported and the SHA-256 of the result's bytes.  Rows: every conv / conv_transpose / conv_integer case of
           tests/test_f32_routes.py, the route table of tests/test_conv_integer_routes.py, conv1d, depthwise_conv1d_tlc on both sides
           of its time-steps line, and both sides of each threshold of conv.hip's conv_route() at the smallest shapes that reach
           it on 256 CUs (THRESHOLDS below).  A one-element constant_of_shape in front of every row leaves fill_kernel -- which no
           convolution path launches: `compare` counts the separators against the rows -- in the trace as the row separator.
  compare  (anywhere) reads the two kernel-trace CSVs and the two outputs of `run` and writes the comparison as JSON: per row the
           sequence of (kernel, grid, workgroup, LDS bytes), the route and the hash of both builds; exit status 1 unless they agree
           everywhere.  Optional further arguments are JSON files of timings that are copied into the document under "speed".

  tools/conv_dispatch_ab.py run > out.jsonl
  tools/conv_dispatch_ab.py compare a_trace.csv a_out.jsonl b_trace.csv b_out.jsonl profiles/conv_dispatch_ab.json [speed.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quant_dispatch_ab as Q  # noqa: E402

MARK = "fill_kernel<"
P1 = (1, 1, 1, 1)
# (what, n, c, h, w, oc, k, group, pads, stride): both sides of each line conv_route() draws, on 256 CUs
THRESHOLDS = [
    ("w1_max_oc: 256 output channels", 16, 32, 20, 20, 256, 1, 1, (0, 0, 0, 0), 1),
    ("w1_max_oc: 257 -> the GEMM", 16, 32, 20, 20, 257, 1, 1, (0, 0, 0, 0), 1),
    ("w1_min_plane: 400 positions", 64, 32, 20, 20, 64, 1, 1, (0, 0, 0, 0), 1),
    ("w1_min_plane: 399 -> the GEMM", 64, 32, 19, 21, 64, 1, 1, (0, 0, 0, 0), 1),
    ("w1_min_c: 32 channels", 64, 32, 20, 20, 64, 1, 1, (0, 0, 0, 0), 1),
    ("w1_min_c: 16 -> the GEMM", 64, 16, 20, 20, 64, 1, 1, (0, 0, 0, 0), 1),
    ("win_min_oc_narrow: 5 output channels", 16, 16, 48, 48, 5, 3, 1, P1, 1),
    ("win_min_oc_narrow: 4 -> not the window kernel", 16, 16, 48, 48, 4, 3, 1, P1, 1),
    ("window, half the CUs: 133 units", 19, 16, 40, 44, 32, 3, 1, P1, 1),
    ("window, half the CUs: 126 -> the GEMM", 18, 16, 40, 44, 32, 3, 1, P1, 1),
    ("oct 64 -> 32: too few 64-channel workgroups", 32, 16, 40, 44, 64, 3, 1, P1, 1),
    ("oct 64 kept", 128, 16, 24, 40, 64, 3, 1, P1, 1),
    ("oct 128: 103 channels, a quarter padding", 40, 32, 40, 40, 103, 1, 1, (0, 0, 0, 0), 1),
    ("oct 128: 102 channels -> 64 / 32", 40, 32, 40, 40, 102, 1, 1, (0, 0, 0, 0), 1),
    ("oct 128: 520 units", 40, 32, 40, 40, 128, 1, 1, (0, 0, 0, 0), 1),
    ("oct 128: 507 units -> 64", 39, 32, 40, 40, 128, 1, 1, (0, 0, 0, 0), 1),
    ("osplit: 512 tiles (eight of 44 x 5 an image), whole items", 64, 16, 40, 44, 128, 3, 1, P1, 1),
    ("osplit: 504 tiles, blocks split", 63, 16, 40, 44, 128, 3, 1, P1, 1),
    ("stride-2 window: 520 units", 40, 16, 80, 80, 64, 3, 1, P1, 2),
    ("stride-2 window: 507 -> the GEMM", 39, 16, 80, 80, 64, 3, 1, P1, 2),
    ("direct: 516 tiles", 43, 8, 48, 48, 8, 3, 1, P1, 1),
    ("direct: 504 -> the GEMM", 42, 8, 48, 48, 8, 3, 1, P1, 1),
    ("direct: 26 channels, one LDS pass", 128, 26, 32, 32, 6, 3, 1, P1, 1),
    ("direct: 27 channels, two passes", 128, 27, 32, 32, 6, 3, 1, P1, 1),
    ("depthwise: 10240 planes, pb as the LDS allows", 64, 160, 20, 20, 160, 3, 160, P1, 1),
    ("depthwise: 4096 planes, pb halved twice", 64, 64, 20, 20, 64, 3, 64, P1, 1),
    ("depthwise: 64 planes, one a workgroup", 2, 32, 20, 20, 32, 3, 32, P1, 1),
]


def run():
    import lele_amd
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    from tests import test_conv_integer_routes as CI
    from tests import test_f32_routes as F

    ctx = lele_amd.default_ctx(0)
    cus = int(K.num_cus(ctx))
    print(json.dumps({"cus": cus, "library": os.environ.get("LELE_HIP_LIBRARY") or "liblele_hip.so"}), flush=True)
    rng = np.random.default_rng(2027)

    def f32(*shape):
        return rng.standard_normal(shape).astype(np.float32)

    def row(name, call):
        K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)  # the separator
        got = call()
        route = K.last_route(ctx)
        got = got if isinstance(got, (tuple, list)) else (got,)
        h = hashlib.sha256()
        for g in got:
            h.update(np.ascontiguousarray(g.numpy() if hasattr(g, "numpy") else g).tobytes())
        print(json.dumps({"row": name, "route": route, "sha256": h.hexdigest()}), flush=True)

    for i, case in enumerate(F.CASES):
        if case["kind"] != "gemm":
            inp = F.make_inputs(i, case)
            row("f32_routes %s" % F.case_id(i, case), lambda: F.run(ctx, case, inp))
    for r in CI.ALL_ROWS:
        n = CI.batch_of(r, cus)
        if r["form"] == "codes":
            _, x, w, zx, zw = CI.cases(r, "random", cus)[0]
            row("conv_integer_routes %s" % r["id"], lambda: K.conv_integer(x, Weight(w), CI.zp(zx), CI.zp(zw), list(r["dil"]), 1, list(r["pads"]),
                                                                          list(r["strides"]), ctx=ctx))
        else:
            w = CI.codes(rng, (r["OC"], r["C"]) + r["k"])
            srcs = [CI.f32_source(rng, (n, c, r["H"], r["W"]), "random") for c in CI.MULTI_SOURCES.get(r["id"], (r["C"],))]
            if r["id"] in CI.MULTI_SOURCES:
                row("conv_integer_routes %s" % r["id"], lambda: K.conv_integer_from_f32_multi(srcs, Weight(w), CI.zp(113.0), ctx=ctx))
            else:
                row("conv_integer_routes %s" % r["id"], lambda: K.conv_integer_from_f32(srcs[0], Weight(w), CI.zp(113.0), list(r["dil"]), 1,
                                                                                       list(r["pads"]), list(r["strides"]), ctx=ctx))
    for what, n, c, h, w_, oc, k, group, pads, s in THRESHOLDS:
        x, w, b = f32(n, c, h, w_), f32(oc, c // group, k, k) * np.float32(0.3), f32(oc)
        row("threshold %s" % what, lambda: K.conv2d_silu(x, w, b, [1, 1], group, list(pads), [s, s], ctx=ctx))
    # conv1d: the STFT-as-convolution of the VAD model, a grouped one with unequal pads and a dilation, [N, L] as one channel
    for xs, ws, group, dil, strides, pads in (((1, 1, 4000), (258, 1, 256), 1, [], [128], []), ((2, 8, 50), (12, 4, 3), 2, [2], [1], [2, 0]),
                                              ((3, 40), (5, 1, 4), 1, [], [2], [1, 1])):
        x, w, b = f32(*xs), f32(*ws), f32(ws[0])
        row("conv1d %s %s" % (xs, ws), lambda: K.conv1d_fused(x, w, b, dil, group, pads, strides, True, ctx=ctx))
    # depthwise_conv1d_tlc: 4 time steps a thread below 256 workgroup-loads of 8 per CU, 8 from there on (1016 | 1024 steps at 256 CUs)
    for t in (1016, 1024):
        for k in (3, 5, 7, 11):
            x, w, b = f32(1, t, 512), f32(512, 1, k), f32(512)
            row("depthwise_conv1d_tlc T = %d, K = %d" % (t, k), lambda: K.depthwise_conv1d_tlc(x, w, b, k // 2, k - 1 - k // 2, True, ctx=ctx))
    x, w = f32(1, 504, 1536), f32(512, 1, 11)
    row("depthwise_conv1d_tlc channels [1024, 1536), the input added", lambda: K.depthwise_conv1d_tlc(x, w, None, 5, 5, False, 1024, True, ctx=ctx))
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)


def compare(a_trace, a_out, b_trace, b_out, dest, *speed):
    Q.MARK = MARK
    (ha, ra), (hb, rb) = Q.read_out(a_out), Q.read_out(b_out)
    ta, tb = Q.read_trace(a_trace), Q.read_trace(b_trace)
    # the separator is one launch that no convolution launches: as many row sequences as rows, none of them empty but an empty result's
    ok = len(ra) == len(rb) == len(ta) == len(tb) and ha["cus"] == hb["cus"]
    rows = []
    for i in range(min(len(ra), len(rb), len(ta), len(tb))):
        same = all(ra[i][f] == rb[i][f] for f in ("row", "route", "sha256")) and ta[i] == tb[i] and bool(ta[i]) == bool(ra[i]["route"])
        ok = ok and same
        e = {"row": ra[i]["row"], "agree": same, "route": ra[i]["route"], "sha256": ra[i]["sha256"], "dispatches": ta[i]}
        if not same:
            e["b_route"], e["b_sha256"], e["b_dispatches"] = rb[i]["route"], rb[i]["sha256"], tb[i]
        rows.append(e)
    doc = {"what": "tools/conv_dispatch_ab.py: one call per row under rocprofv3 --kernel-trace, once per library; dispatches are "
                   "[kernel, grid (threads), workgroup, LDS bytes]; where the two libraries agree the row is written once",
           "cus": ha["cus"], "a": ha["library"], "b": hb["library"], "rows_a": len(ra), "rows_b": len(rb), "separators_a": len(ta),
           "separators_b": len(tb), "agree": bool(ok)}
    for f in speed:
        with open(f) as fh:
            doc.setdefault("speed", {}).update(json.load(fh))
    doc["rows"] = rows
    with open(dest, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d rows, %d CUs: %s" % (len(rows), ha["cus"], "the two libraries agree" if ok else "MISMATCH"))
    for e in rows:
        if not e["agree"]:
            print("  differs:", e["row"])
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 7 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
