#!/usr/bin/env python3
"""Same kernels, same geometry, same bytes: the quantised-linear dispatch of two builds of the library, call by call.

  run      (on the GPU, once per library, under `rocprofv3 --kernel-trace` as tools/ktrace.sh runs it; LELE_HIP_LIBRARY picks the build)
           issues ONE call per row of the shape matrix below -- a row per branch and threshold side of quant.hip's route decisions, at
           the smallest shapes that reach it on 256 CUs -- and prints one JSON line per row with the SHA-256 of the result's bytes.
           A one-element dynamic_quantize_linear in front of every row leaves dq_apply_kernel in the trace as the row separator.
  compare  (anywhere) reads the two kernel-trace CSVs and the two outputs of `run` and writes the comparison as JSON: per row the
           sequence of (kernel, grid, workgroup, LDS bytes) and the hash of both builds; exit status 1 unless they agree everywhere.

  tools/quant_dispatch_ab.py run > out.jsonl
  tools/quant_dispatch_ab.py compare a_trace.csv a_out.jsonl b_trace.csv b_out.jsonl profiles/quant_dispatch_ab.json
"""
import csv
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MARK = "dq_apply_kernel"


class env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run():
    import lele_amd
    from lele_amd import kernels as K
    from lele_amd._lib import Weight

    ctx = lele_amd.default_ctx(0)
    print(json.dumps({"cus": int(K.num_cus(ctx)), "library": os.environ.get("LELE_HIP_LIBRARY") or "liblele_hip.so"}), flush=True)
    rng = np.random.default_rng(2026)
    one = np.zeros(1, np.float32)

    def qw(k, n, lead=()):
        return (Weight(np.clip(np.round(128 + 32 * rng.standard_normal(lead + (k, n))), 0, 255).astype(np.float32)),
                Weight((np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32)), Weight(np.array([121.0], np.float32)),
                Weight((rng.standard_normal(n) * 0.02).astype(np.float32)))

    def f32(*shape):
        return rng.standard_normal(shape).astype(np.float32)

    def dev(a):
        return ctx.buf().upload(a)

    def ln(n=512):
        return Weight((1 + 0.1 * rng.standard_normal(n)).astype(np.float32)), Weight((0.1 * rng.standard_normal(n)).astype(np.float32))

    def row(name, call):
        K.dynamic_quantize_linear(one, ctx=ctx)  # the separator
        got = call()
        got = got if isinstance(got, (tuple, list)) else (got,)
        h = hashlib.sha256()
        for g in got:
            h.update(np.ascontiguousarray(g.numpy()).tobytes())
        print(json.dumps({"row": name, "sha256": h.hexdigest()}), flush=True)

    # ---- dense
    dense = [(1, 512, 512, 1024), (1, 480, 512, 1024),  # register-stationary | small-problem tiled across the 2-tiles-per-CU line
             (1, 512, 500, 1024),                       # qrows_frag in front
             (4, 128, 512, 1024),                       # several slices a workgroup
             (1, 256, 512, 128), (1, 256, 512, 512), (1, 1376, 512, 512), (1, 2752, 512, 512),  # activation-stationary: whole rows / 4 / 8 / all
             (1, 255, 512, 512),                        # just under as_fits
             (1, 504, 2048, 512),                       # igemm_small<16>
             (1, 2048, 1024, 4096), (1, 2048, 1024, 3840),  # igemm_big | the 128 x 64 tile just under it
             (1, 4096, 576, 2048),                      # the 128 x 128 tile
             (1, 32, 64, 32768),                        # the 32 x 128 tile
             (1, 2304, 2064, 512)]                      # rows and kp both past 2048: the streaming row quantiser
    for b, m, k, n in dense:
        x, w = dev(f32(b, m, k)), qw(k, n)
        row("dense %s" % ((b, m, k, n),), lambda: K.fused_quantized_linear(x, *w, False, ctx=ctx))
    for b, m, k, n in [(1, 512, 512, 1024), (1, 256, 512, 512), (1, 504, 2048, 512)]:  # the three GEMM families with a residual and ReLU
        x, w, r1, r2 = dev(f32(b, m, k)), qw(k, n), dev(f32(b, m, n)), dev(f32(b, m, n))
        row("residual relu %s" % ((b, m, k, n),), lambda: K.fused_quantized_linear_residual(x, *w, True, r1, r2, ctx=ctx))
        row("residual one %s" % ((b, m, k, n),), lambda: K.fused_quantized_linear_residual(x, *w, False, r1, None, ctx=ctx))

    # ---- _residual_ln and sanm_out_block
    for b, m in [(32, 171), (1, 504), (40, 100)]:
        x, w, r1, r2, (g, be) = dev(f32(b, m, 512)), qw(512, 512), dev(f32(b, m, 512)), dev(f32(b, m, 512)), ln()
        row("residual_ln %s" % ((b, m),), lambda: K.fused_quantized_linear_residual_ln(x, *w, False, r1, r2, g, be, 1e-5, ctx=ctx))
        row("residual_ln no residual %s" % ((b, m),), lambda: K.fused_quantized_linear_residual_ln(x, *w, False, None, None, g, be, 1e-5, ctx=ctx))
        qkv, fw, fb = dev(f32(b, m, 1536)), Weight((f32(512, 1, 11) / np.sqrt(11)).astype(np.float32)), Weight(f32(512))
        row("sanm_out_block %s" % ((b, m),), lambda: K.sanm_out_block(x, *w, False, qkv, fw, None, 1024, 5, 5, r2, g, be, 1e-5, ctx=ctx))
        row("sanm_out_block bias, no res2 %s" % ((b, m),), lambda: K.sanm_out_block(x, *w, False, qkv, fw, fb, 1024, 5, 5, None, g, be, 1e-5, ctx=ctx))
    x, w, rb, (g, be) = dev(f32(32, 171, 512)), qw(512, 512), dev(f32(512)), ln()
    row("residual_ln broadcasting (32, 171)", lambda: K.fused_quantized_linear_residual_ln(x, *w, False, rb, None, g, be, 1e-5, ctx=ctx))
    qkv, fw, r2 = dev(f32(32, 171, 1536)), Weight((f32(512, 1, 11) / np.sqrt(11)).astype(np.float32)), dev(f32(171, 512))
    row("sanm_out_block broadcasting res2 (32, 171)", lambda: K.sanm_out_block(x, *w, False, qkv, fw, None, 1024, 5, 5, r2, g, be, 1e-5, ctx=ctx))

    # ---- feed-forward 512 -> 2048 -> 512
    w1, w2, (g, be) = qw(512, 2048), qw(2048, 512), ln()
    for b, m in [(1, 504), (1, 480)]:
        x, r1 = dev(f32(b, m, 512)), dev(f32(b, m, 512))
        row("ffn %s" % ((b, m),), lambda: K.fused_ffn_quantized(x, *w1, *w2, False, ctx=ctx))
        row("ffn residual %s" % ((b, m),), lambda: K.fused_ffn_quantized(x, *w1, *w2, False, r1, ctx=ctx))
    x, r1 = dev(f32(1, 504, 512)), dev(f32(1, 504, 512))
    with env(LELE_HIP_FFN_ONE_LAUNCH=0):
        row("ffn (1, 504) LELE_HIP_FFN_ONE_LAUNCH=0", lambda: K.fused_ffn_quantized(x, *w1, *w2, False, ctx=ctx))
    row("ffn_ln (1, 504)", lambda: K.fused_ffn_quantized_ln(x, *w1, *w2, False, r1, None, g, be, 1e-5, ctx=ctx))
    x5, w5 = dev(f32(1, 504, 500)), qw(500, 2048)
    row("ffn k1 = 500 (1, 504)", lambda: K.fused_ffn_quantized(x5, *w5, *w2, False, ctx=ctx))
    x, r1, r2 = dev(f32(16, 171, 512)), dev(f32(16, 171, 512)), dev(f32(16, 171, 512))
    row("ffn_ln (16, 171)", lambda: K.fused_ffn_quantized_ln(x, *w1, *w2, False, r1, r2, g, be, 1e-5, ctx=ctx))
    row("ffn (16, 171)", lambda: K.fused_ffn_quantized(x, *w1, *w2, True, r1, ctx=ctx))
    x, w1t, w2t = dev(f32(1, 8192, 512)), qw(512, 1024), qw(1024, 512)
    row("ffn tiled fused n1 = 1024 (1, 8192)", lambda: K.fused_ffn_quantized(x, *w1t, *w2t, False, ctx=ctx))

    # ---- other entries
    x, w = dev(f32(513, 512)), qw(512, 512)
    row("segments ragged [0, 37, 37, 200, 513]", lambda: K.fused_quantized_linear_segments(x, [0, 37, 37, 200, 513], *w, True, ctx=ctx))
    a = dev(rng.integers(0, 256, (3, 70, 100)).astype(np.float32))
    wu = Weight(rng.integers(0, 256, (100, 130)).astype(np.float32))
    wb = Weight(rng.integers(0, 256, (3, 100, 130)).astype(np.float32))
    row("mat_mul_integer B un-batched", lambda: K.mat_mul_integer(a, wu, [3.0], [131.0], ctx=ctx))
    row("mat_mul_integer B batched", lambda: K.mat_mul_integer(a, wb, [3.0], [131.0], ctx=ctx))
    K.dynamic_quantize_linear(one, ctx=ctx)


def read_trace(path):
    """-> the dispatches in order as [kernel, grid, workgroup, lds], split at the separator into rows"""
    with open(path, newline="") as f:
        recs = list(csv.DictReader(f))
    cols = {c.lower(): c for c in recs[0]}

    def col(*names):
        for n in names:
            if n in cols:
                return cols[n]
        raise KeyError("%s: none of %s among %s" % (path, names, sorted(cols)))

    name, lds = col("kernel_name"), col("lds_block_size", "lds_block_size_v", "lds_memory_size")
    wg = [col("workgroup_size_%s" % a, "workgroup_size_%s" % a.upper()) for a in "xyz"]
    grid = [col("grid_size_%s" % a, "grid_size_%s" % a.upper()) for a in "xyz"]
    order = col("dispatch_id") if "dispatch_id" in cols else col("start_timestamp")
    recs.sort(key=lambda r: int(r[order]))
    rows, cur = [], None
    for r in recs:
        if MARK in r[name]:
            if cur is not None:
                rows.append(cur)
            cur = []
        elif cur is not None:
            cur.append([r[name].replace("(anonymous namespace)::", ""), [int(r[c]) for c in grid], [int(r[c]) for c in wg], int(r[lds])])
    return rows  # what follows the last separator is dropped: `run` ends with one


def read_out(path):
    head, rows = None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line.startswith("{"):
                continue
            d = json.loads(line)
            if "cus" in d:
                head = d
            elif "row" in d:
                rows.append(d)
    return head, rows


def strip_sep(seq):
    """the separator's own range pass (qminmax_kernel + qparams_kernel over one element) precedes dq_apply_kernel: it closes the row before"""
    if len(seq) >= 2 and "qminmax_kernel" in seq[-2][0] and "qparams_kernel" in seq[-1][0]:
        return seq[:-2]
    return seq


def compare(a_trace, a_out, b_trace, b_out, dest):
    (ha, ra), (hb, rb) = read_out(a_out), read_out(b_out)
    ta, tb = [strip_sep(s) for s in read_trace(a_trace)], [strip_sep(s) for s in read_trace(b_trace)]
    ok = len(ra) == len(rb) == len(ta) == len(tb) and ha["cus"] == hb["cus"]
    rows = []
    for i in range(min(len(ra), len(rb), len(ta), len(tb))):
        same = ra[i]["row"] == rb[i]["row"] and ra[i]["sha256"] == rb[i]["sha256"] and ta[i] == tb[i]
        ok = ok and same
        e = {"row": ra[i]["row"], "agree": same, "sha256": ra[i]["sha256"], "dispatches": ta[i]}
        if not same:
            e["b_sha256"], e["b_dispatches"] = rb[i]["sha256"], tb[i]
        rows.append(e)
    doc = {"what": "tools/quant_dispatch_ab.py: one call per row under rocprofv3 --kernel-trace, once per library; dispatches are "
                   "[kernel, grid (threads), workgroup, LDS bytes]; where the two libraries agree the row is written once",
           "cus": ha["cus"], "a": ha["library"], "b": hb["library"], "rows_a": len(ra), "rows_b": len(rb), "agree": bool(ok), "rows": rows}
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
    elif len(sys.argv) == 7 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
