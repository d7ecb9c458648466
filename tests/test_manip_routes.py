"""Every data-movement route (lele_amd/csrc/manip.hip, the bit-exact class) against a numpy restatement, bit for bit: one table row
per dispatch branch, threshold and refusal.

Behind each entry point of manip.hip a dispatcher picks a kernel by alignment, divisibility, tile fit, row length and the CU count.
Every row names the route the library must report (kernels.last_route()) and the condition that selects it, so a re-tune that moves a
shape to another kernel fails here instead of leaving that kernel untested.

Pure copies (COPY_ROWS, pad, gather, resize, transpose_cp, the pitched copy): word i of an input is (i * 2654435761 + 12345) mod 2^32
(8-byte types: the odd multiplier 0x9E3779B97F4A7C15 mod 2^64) -- a bijection, so all words differ and equal output bits mean the right
index map; NaN payloads, denormals and -0 occur among them.  Compared as .view(uint32 / uint64) with numpy index arithmetic.  An operand
that is a slice or a channel view sits in a parent that carries the same tagging, so a read outside it cannot match; a result written
into an out_window sits in a buffer prefilled with a sentinel that must survive outside the window.

Max-pool: oracle/npref.py::max_pool2d restates the reference's `if val > max_val` over the taps in (kh, kw) order (a NaN never wins,
the first of equal values stays); pinned here on a literal triple loop of conv2d.rs:1222-1251.  Every row runs on POOL_FAMILIES.
Top-k: npref.topk (stable, a NaN last, the lower index first) on TOPK_FAMILIES, both directions, values and indices by bits.
Casts: Rust's `as` restated in integer arithmetic.

CPU part: name coverage, every row against the dispatch restated in Python for 256 CUs, pairwise distinct words, npref.max_pool2d
against the literal scan, and the special-value families telling the oracle from emulated wrong kernels (VARIANTS_*).
GPU part: every row asserts last_route() and then the bits."""
import functools
import re

import numpy as np
import pytest

from oracle import npref

CUS = 256
F32, I64, I32, U8 = np.dtype(np.float32), np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.uint8)

# the 64-bit index routes need more than 2^31 elements (8 GiB and more in one tensor): named, not covered
NOT_COVERED = {"copy.i64": "64-bit indexing in strided_copy_kernel needs a tensor of 2^31 elements or offsets that far apart",
               "pool.direct_i64": "max_pool2d_kernel<int64_t> needs 2^31 input or output elements"}
PREFIXES = ("copy.", "resize.", "pool.", "topk.", "cpitch.", "pad.", "gather.", "apool.", "tcp.", "range.", "fill.", "cast.")


# ------------------------------------------------------------------------------------------------------------- tagged inputs
def words(n, es):
    i = np.arange(n, dtype=np.uint64)
    if es == 4:
        return ((i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if es == 8:
        with np.errstate(over="ignore"):
            return i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)
    return ((i * np.uint64(167) + np.uint64(45)) & np.uint64(0xFF)).astype(np.uint8)   # bytes: distinct up to 256 of them


def tagged(shape, dt):
    dt = np.dtype(dt)
    return words(int(np.prod(shape, dtype=np.int64)), dt.itemsize).view(dt).reshape(shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------- the strided copy engine
def copy_route(launches, es):
    """launch_copy restated: the route of the last non-empty launch; a launch = (oshape, istride, imod, ostride, ioff, ooff) in
    elements, base pointers 16-byte aligned"""
    route = ""
    for oshape, istr, imod, ostr, ioff, ooff in launches:
        numel = int(np.prod(oshape, dtype=np.int64))
        if numel == 0:
            continue
        d = [[o, i, m, s] for o, i, m, s in zip(oshape, istr, imod, ostr) if o != 1]   # unit dims dropped
        k = len(d) - 2
        while k >= 0:   # dims contiguous on both sides merged
            if d[k][2] == 0 and d[k + 1][2] == 0 and d[k][1] == d[k + 1][1] * d[k + 1][0] and d[k][3] == d[k + 1][3] * d[k + 1][0]:
                d[k] = [d[k][0] * d[k + 1][0], d[k + 1][1], 0, d[k + 1][3]]
                del d[k + 1]
            k -= 1
        r, v = len(d), 16 // es
        vec = (r >= 1 and d[-1][1] == 1 and d[-1][3] == 1 and d[-1][2] == 0 and d[-1][0] % v == 0 and ioff % v == 0 and ooff % v == 0
               and all(x[1] % v == 0 and x[3] % v == 0 for x in d[:-1]))
        if vec:
            numel //= v
            ioff, ooff = ioff // v, ooff // v
            d = [[x[0], x[1] // v, x[2], x[3] // v] for x in d[:-1]] + [[d[-1][0] // v, 1, 0, 1]]
        imax = abs(ioff) + sum((x[0] - 1) * abs(x[1]) for x in d)
        omax = abs(ooff) + sum((x[0] - 1) * abs(x[3]) for x in d)
        i32 = numel < 2 ** 31 and imax < 2 ** 31 and omax < 2 ** 31
        tiled = False
        if not vec and r >= 2 and d[-1][3] == 1 and d[-1][1] != 1 and d[-1][0] >= 8 and all(x[2] == 0 for x in d):
            tj = -1
            for k in range(r - 1):
                if d[k][1] == 1 and d[k][0] >= 8:
                    tj = k
            others = int(np.prod([d[k][0] for k in range(r - 1) if k != tj], dtype=np.int64))
            tiled = tj >= 0 and others <= 65535 and (d[tj][0] + 63) // 64 <= 65535
        if tiled:
            route = "copy.tile_w%d" % es
        else:
            route = ("copy.vec16" if vec else "copy.w%d" % es) + ("" if i32 else "/copy.i64")
    return route


def _strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return st[::-1]


def _view_launch(shape, fn):
    """the launch a numpy view of a [shape] tensor stands for: numpy's own strides and offset, dense output"""
    idx = np.arange(int(np.prod(shape, dtype=np.int64)), dtype=np.int64).reshape(shape)
    v = fn(idx)
    off = (v.__array_interface__["data"][0] - idx.__array_interface__["data"][0]) // 8 if v.size else 0
    return (list(v.shape), [s // 8 for s in v.strides], [0] * v.ndim, _strides(v.shape), off, 0)


def _slices(sl):
    return tuple(slice(*s) for s in sl)


def C(route, kind, dt, shape, arg, why):
    return dict(route=route, kind=kind, dt=np.dtype(dt), shape=shape, arg=arg, why=why)


COPY_ROWS = [
    # the plain strided kernel: nothing contiguous on both sides, no dim of 8 contiguous in the input
    C("copy.w4", "transpose", F32, (5, 6, 7), [2, 0, 1], "inner dim strided in the input, the input-contiguous dim has 7 < 8 elements"),
    C("copy.w8", "transpose", I64, (5, 6, 7), [2, 0, 1], "the same, 8-byte words"),
    # 16-byte words: inner dim contiguous on both sides, length / offsets / outer strides multiples of 16 bytes
    C("copy.vec16", "slice", F32, (40, 64), [(0, 40, 2), (0, 64, 1)], "rows at step 2: inner 64 % 4 == 0, outer stride 128 % 4 == 0"),
    C("copy.vec16", "slice", I64, (40, 64), [(0, 40, 2), (0, 64, 1)], "rows at step 2, 8-byte: inner 64 % 2 == 0"),
    C("copy.w4", "slice", F32, (40, 64), [(0, 40, 2), (1, 61, 1)], "refusal: inner start 1 (ioff % 4 != 0), inner length 60"),
    C("copy.w8", "slice", I64, (40, 64), [(0, 40, 2), (1, 61, 1)], "refusal: inner start 1 (ioff % 2 != 0), 8-byte"),
    C("copy.w4", "slice", F32, (40, 72), [(0, 40, 2), (0, 66, 1)], "refusal: inner length 66 % 4 != 0"),
    C("copy.w4", "slice", F32, (40, 66), [(0, 40, 1), (0, 64, 1)], "refusal: outer stride 66 % 4 != 0"),
    C("copy.w8", "slice", I64, (40, 65), [(0, 40, 1), (0, 64, 1)], "refusal: outer stride 65 % 2 != 0, 8-byte"),
    C("copy.vec16", "slice", F32, (6, 10, 8), [(1, 5, 1), (2, 10, 2), (0, 8, 1)], "three dims, offset 96: every stride and offset % 4 == 0"),
    C("copy.w4", "tile", F32, (3, 8), [2, 1], "tile carries a modulus on every dim, the inner one too: never 16-byte words, never tiles"),
    C("copy.w8", "tile", I64, (2, 3, 4), [2, 3, 2], "tile, 8-byte, repeats on every dim"),
    # the 64 x 64 LDS tiles: inner dim strided in the input and >= 8, another dim of >= 8 contiguous there, <= 65535 remaining
    C("copy.tile_w4", "transpose", F32, (3, 130, 65), [0, 2, 1], "inner 130 = 2 tiles + 2, contiguous dim 65 = 1 tile + 1, 3 in grid.z"),
    C("copy.tile_w4", "transpose", F32, (64, 64), [1, 0], "exactly one whole tile"),
    C("copy.tile_w4", "transpose", F32, (8, 8), [1, 0], "both thresholds at their least: inner 8, contiguous 8"),
    C("copy.tile_w4", "transpose", F32, (2, 3, 9, 70), [1, 0, 3, 2], "two outer dims swapped too: grid.z = 6 decoded into two coordinates"),
    C("copy.tile_w4", "transpose", F32, (65, 130), [1, 0], "rank 2: inner 65, contiguous 130"),
    C("copy.tile_w4", "strided", F32, (4, 21, 13), ([4, 12, 20], [-273, 1, 13], 833), "offset 833, outer stride -273: a window of a mirrored parent"),
    C("copy.tile_w4", "expand", F32, (9, 1), [9, 16], "a broadcast inner dim (stride 0) beside a contiguous dim of 9"),
    C("copy.tile_w8", "transpose", I64, (2, 70, 65), [0, 2, 1], "8-byte tiles, ragged on both sides"),
    C("copy.tile_w8", "transpose", I64, (8, 8), [1, 0], "8-byte, both thresholds at their least"),
    C("copy.tile_w4", "transpose", F32, (65535, 8, 8), [0, 2, 1], "65535 remaining: the largest grid.z"),
    C("copy.w4", "transpose", F32, (65536, 8, 8), [0, 2, 1], "refusal: 65536 remaining would overflow grid.z"),
    C("copy.w4", "transpose", F32, (7, 9), [1, 0], "refusal: inner dim 7 < 8"),
    C("copy.w4", "transpose", F32, (9, 7), [1, 0], "refusal: contiguous dim 7 < 8"),
    C("copy.w8", "transpose", I64, (7, 9), [1, 0], "refusal: inner dim 7 < 8, 8-byte"),
    # concat reports its last launch
    C("copy.vec16", "concat", F32, [(6, 4), (6, 8)], 1, "inner axis, widths 4 and 8: output offset 4, row stride 12"),
    C("copy.w4", "concat", F32, [(6, 3), (6, 5)], 1, "inner axis, widths 3 and 5: nothing divides by 4"),
    C("copy.vec16", "concat", I64, [(6, 4), (6, 8)], 1, "8-byte, widths 4 and 8"),
    C("copy.w4", "concat", F32, [(2, 3, 5), (4, 3, 5), (0, 3, 5)], 0, "outer axis, the last input empty: the route of the one before it"),
    C("copy.w4", "split", F32, (4, 10, 6), (1, [3, 7]), "parts of 18 and 42 contiguous elements a row"),
    C("copy.vec16", "split", F32, (4, 10, 6), (1, [4, 6]), "parts of 24 and 36 contiguous elements a row, offset 24"),
    C("copy.w4", "expand", F32, (3, 1), [3, 4], "broadcast inner dim of 4 < 8"),
    C("copy.vec16", "expand", F32, (1, 8), [5, 8], "broadcast outer dim (stride 0 % 4 == 0)"),
    C("", "slice", F32, (4, 5), [(2, 2, 1), (0, 5, 1)], "an empty result launches nothing"),
]
COPY_IDS = ["%d-%s-%s-%s" % (i, r["route"] or "none", r["kind"], r["dt"].name) for i, r in enumerate(COPY_ROWS)]


def copy_inputs(row):
    if row["kind"] == "concat":   # the parts continue one tagging, so they share no word
        n, parts = 0, []
        for s in row["shape"]:
            m = int(np.prod(s))
            parts.append(words(n + m, row["dt"].itemsize)[n:].view(row["dt"]).reshape(s))
            n += m
        return parts
    return [tagged(row["shape"], row["dt"])]


def copy_launches(row):
    kind, shape, arg = row["kind"], row["shape"], row["arg"]
    if kind == "transpose":
        return [_view_launch(shape, lambda a: a.transpose(arg))]
    if kind == "slice":
        return [_view_launch(shape, lambda a: a[_slices(arg)])]
    if kind == "expand":
        return [_view_launch(shape, lambda a: np.broadcast_to(a, arg))]
    if kind == "strided":
        return [(arg[0], arg[1], [0] * len(arg[0]), _strides(arg[0]), arg[2], 0)]
    if kind == "tile":
        osh = [d * r for d, r in zip(shape, arg)]
        return [(osh, _strides(shape), list(shape), _strides(osh), 0, 0)]
    if kind == "split":
        ax, sizes = arg
        res, pos = [], 0
        for sz in sizes:
            res.append(_view_launch(shape, lambda a: a[(slice(None),) * ax + (slice(pos, pos + sz),)]))
            pos += sz
        return res[-1:]   # every part is a call of its own: the route is the last one's
    if kind == "concat":
        osh = list(shape[0])
        osh[arg] = sum(s[arg] for s in shape)
        ostr, res, pos = _strides(osh), [], 0
        for s in shape:
            res.append((list(s), _strides(s), [0] * len(s), ostr, 0, pos * ostr[arg]))
            pos += s[arg]
        return res
    raise KeyError(kind)


def copy_reference(row, xs):
    kind, arg = row["kind"], row["arg"]
    x = xs[0]
    if kind == "transpose":
        return [np.ascontiguousarray(x.transpose(arg))]
    if kind == "slice":
        return [np.ascontiguousarray(x[_slices(arg)])]
    if kind == "expand":
        return [np.ascontiguousarray(np.broadcast_to(x, arg))]
    if kind == "strided":
        idx = arg[2] + sum(np.arange(n, dtype=np.int64).reshape([-1 if j == k else 1 for j in range(len(arg[0]))]) * arg[1][k]
                           for k, n in enumerate(arg[0]))
        return [x.reshape(-1)[idx]]
    if kind == "tile":
        return [np.tile(x, arg)]
    if kind == "split":
        return [np.ascontiguousarray(p) for p in np.split(x, np.cumsum(arg[1])[:-1], axis=arg[0])]
    if kind == "concat":
        return [np.concatenate(xs, arg)]
    raise KeyError(kind)


def copy_run(K, ctx, row, xs):
    kind, arg = row["kind"], row["arg"]
    dev = [ctx.buf().upload(x) if x.size else x for x in xs]   # (a buffer cannot hold an empty tensor: that one stays on the host)
    if kind == "transpose":
        return [K.transpose(dev[0], arg, ctx=ctx)]
    if kind == "slice":
        return [K.slice(dev[0], [s[0] for s in arg], [s[1] for s in arg], list(range(len(arg))), [s[2] for s in arg], ctx=ctx)]
    if kind == "expand":
        return [K.expand(dev[0], arg, ctx=ctx)]
    if kind == "strided":
        return [K._strided(dev[0], arg[0], arg[1], arg[2], ctx=ctx)]
    if kind == "tile":
        return [K.tile(dev[0], arg, ctx=ctx)]
    if kind == "split":
        return K.split(dev[0], arg[0], arg[1], ctx=ctx)
    if kind == "concat":
        return [K.concat(dev, arg, ctx=ctx)]
    raise KeyError(kind)


def tile_emulation(launch, x, predicate=True):
    """transpose_tile_kernel in numpy, block by block: loads from clamped coordinates, stores under `j < nj && i < ni`.  predicate =
    False is the wrong kernel that clamps but stores from every lane: the stray stores (applied after the proper ones, where they
    fall inside the result) put an edge value over a neighbour"""
    oshape, istr, _, ostr, ioff, _ = launch
    d = [(o, i, s) for o, i, s in zip(oshape, istr, ostr) if o != 1]
    ni, is_, _ = d[-1]
    tj = max(k for k in range(len(d) - 1) if d[k][1] == 1 and d[k][0] >= 8)
    nj, js, jos = d[tj]
    rest = [d[k] for k in range(len(d) - 1) if k != tj]
    n = int(np.prod(oshape))
    out = np.zeros(n, x.dtype)
    stray = []
    flat = x.reshape(-1)
    for z in np.ndindex(*[o for o, _, _ in rest]):
        si = ioff + sum(c * i for c, (_, i, _) in zip(z, rest))
        di = sum(c * s for c, (_, _, s) in zip(z, rest))
        for j0 in range(0, nj, 64):
            for i0 in range(0, ni, 64):
                jj, ii = np.meshgrid(np.arange(j0, j0 + 64), np.arange(i0, i0 + 64), indexing="ij")
                val = flat[si + np.minimum(jj, nj - 1) * js + np.minimum(ii, ni - 1) * is_]
                dst = di + jj * jos + ii
                ok = (jj < nj) & (ii < ni)
                out[dst[ok]] = val[ok]
                if not predicate:
                    inside = ~ok & (dst < n)
                    stray.append((dst[inside], val[inside]))
    for dst, val in stray:
        out[dst] = val
    return out.reshape(oshape)


# ------------------------------------------------------------------------------------------------------- pad, gather, resize
PAD_ROWS = [   # (dtype, shape, pads, mode, constant)
    (F32, (7,), [2, 3], "constant", -0.0), (F32, (7,), [2, 3], "edge", None), (F32, (7,), [6, 7], "reflect", None),
    (I64, (7,), [2, 3], "constant", 0x0123456789ABCDEF), (I64, (7,), [2, 3], "edge", None), (I64, (7,), [6, 7], "reflect", None),
    (F32, (2, 3, 4, 5), [1, 0, 2, 3, 0, 2, 1, 4], "constant", -0.0), (F32, (2, 3, 4, 5), [1, 0, 2, 3, 0, 2, 1, 4], "edge", None),
    (F32, (2, 3, 4, 5), [1, 2, 3, 4, 2, 3, 4, 5], "reflect", None),   # begin = dim - 1, end = dim on every axis
    (I64, (2, 3, 4, 5), [1, 0, 2, 3, 0, 2, 1, 4], "constant", -2), (I64, (2, 3, 4, 5), [1, 2, 3, 4, 2, 3, 4, 5], "reflect", None),
    (I64, (2, 3, 4, 5), [0, 1, 1, 0, 1, 0, 0, 2], "edge", None), (F32, (2, 3, 4, 5), [2, 1, 1, 2], "reflect", None),   # trailing dims only
    (F32, (300,), [299, 300], "reflect", None),   # more than one workgroup
]


def rust_f32_as_i64(v):
    """Rust's `f32 as i64` (utils.rs, AsI64 for f32; conv2d.rs:1484): toward zero, saturating, NaN -> 0"""
    out = np.empty(np.shape(v), np.int64)
    flat = out.reshape(-1)
    for i, f in enumerate(np.asarray(v, np.float32).reshape(-1)):
        f = float(f)
        flat[i] = 0 if f != f else 2 ** 63 - 1 if f >= 2.0 ** 63 else -2 ** 63 if f <= -2.0 ** 63 else int(f)
    return out


def index_of(idx, dim):
    """manipulation.rs:626-633 / conv2d.rs:1484-1490: `as i64`, then a negative index counts from the end"""
    i = rust_f32_as_i64(idx) if np.asarray(idx).dtype == np.float32 else np.asarray(idx).astype(np.int64)
    return np.where(i < 0, i + dim, i)


GATHER_IDX = {   # axis dim 5: the f32 values are truncated toward zero first, so -0.5 is index 0 and -1.5 is -1 = 4
    "f32": np.array([[0.9, -0.5, -1.5], [4.99, 2.0, -5.0]], np.float32),
    "i64": np.array([[0, -1, 3], [4, 2, -5]], np.int64),
    "i32": np.array([[1, -2, 3], [4, 0, -5]], np.int32),
}
GATHER_ROWS = [(dt, name, shape, axis) for dt in (F32, I64) for name in GATHER_IDX
               for shape, axis in (((3, 5, 4), 1), ((5, 6), 0), ((4, 5), -1))]   # a middle axis with inner 4; the first; the last
GE_ROWS = [((4, 5, 6), (3, 4, 5), 0), ((4, 5, 6), (3, 4, 5), 1), ((4, 5, 6), (4, 5, 2), 2), ((4, 5, 6), (4, 5, 6), -2), ((300,), (257,), 0)]


def gather_elements_reference(x, idx, axis):
    """conv2d.rs:1474-1499: the coordinates of the index tensor, the one along `axis` replaced"""
    axis = axis + x.ndim if axis < 0 else axis
    co = list(np.indices(idx.shape))
    co[axis] = index_of(idx, x.shape[axis])
    return x[tuple(co)]


def resize_route(shape, oh, ow, asymmetric, x_pitch=0, out_pitch=0, x_off=0, out_off=0):
    n, c, h, w = shape
    up = oh // h if oh % h == 0 else 0
    xbs, obs = x_pitch or c * h * w, out_pitch or c * oh * ow
    fast = (asymmetric and up in (2, 4, 8) and ow == up * w and w % 4 == 0 and n <= 65535 and x_off % 4 == 0 and out_off % 4 == 0
            and xbs % 4 == 0 and obs % 4 == 0)
    return "resize.up%d" % up if fast else "resize.generic"


def Rz(route, shape, scales, mode="asymmetric", view=None, window=None, why=""):
    return dict(route=route, shape=shape, scales=scales, mode=mode, view=view, window=window, why=why)


RESIZE_ROWS = [
    Rz("resize.up2", (2, 3, 5, 8), (2, 2), why="x2 of both, W % 4 == 0"), Rz("resize.up4", (2, 3, 5, 8), (4, 4), why="x4"),
    Rz("resize.up8", (2, 3, 5, 8), (8, 8), why="x8"),
    Rz("resize.up2", (1, 5, 9, 24), (2, 2), why="270 quads an image: a second workgroup with 14 live lanes"),
    Rz("resize.up4", (2, 3, 5, 8), (4, 4), view=(7, 2), why="channels 2 .. 4 of 7: image pitch 280, offset 80, both % 4 == 0"),
    Rz("resize.up2", (2, 3, 5, 8), (2, 2), view=(7, 2), window=(6, 1), why="a channel view into channels 1 .. 3 of a 6-channel result"),
    Rz("resize.generic", (2, 3, 5, 8), (2, 2), view=(7, 2), window=(6, 1), mode="half_pixel", why="refusal through views: half_pixel"),
    Rz("resize.generic", (2, 3, 5, 6), (2, 2), why="refusal: W = 6 is no multiple of 4"),
    Rz("resize.generic", (2, 3, 5, 8), (2, 4), why="refusal: scales (2, 4) differ"),
    Rz("resize.generic", (2, 3, 5, 8), (2, 2), mode="half_pixel", why="refusal: half_pixel"),
    Rz("resize.generic", (2, 3, 5, 8), (3, 3), why="refusal: x3"), Rz("resize.generic", (2, 3, 6, 8), (0.5, 1.5), why="refusal: down-sampling"),
]

TCP_SIZES = (1, 31, 32, 33, 63)

CPITCH_ROWS = [   # (route, dtype, parent shape, c0, c1, condition)
    ("cpitch.w16", F32, (3, 10, 8), 2, 6, "row 128 B, offset 64 B, pitch 320 B: all multiples of 16"),
    ("cpitch.w16", I64, (2, 6, 4), 1, 3, "8-byte elements: row 64 B, offset 32 B, pitch 192 B"),
    ("cpitch.w4", F32, (3, 10, 3), 1, 4, "row 36 B: a multiple of 4 only"),
    ("cpitch.w4", F32, (3, 10, 6), 1, 3, "row 48 B, pitch 240 B, but offset 24 B: a multiple of 4 only"),
    ("cpitch.w1", U8, (3, 10, 3), 1, 4, "a u8 tensor, row 9 B"),
]


# ------------------------------------------------------------------------------------------------------------------ max-pool
def pool_dims(shape, k, s, p, d, ceil):
    kh, kw = k[0], k[1] if len(k) > 1 else k[0]
    sh = s[0] if len(s) else 1
    sw = s[1] if len(s) > 1 else sh
    pt = p[0] if len(p) else 0
    pl = p[1] if len(p) > 1 else pt
    pb = p[2] if len(p) > 2 else pt
    pr = p[3] if len(p) > 3 else pl
    dh = d[0] if len(d) else 1
    dw = d[1] if len(d) > 1 else dh
    nh, nw = shape[2] + pt + pb - (dh * (kh - 1) + 1), shape[3] + pl + pr - (dw * (kw - 1) + 1)
    oh = (nh + sh - 1) // sh + 1 if ceil else nh // sh + 1
    ow = (nw + sw - 1) // sw + 1 if ceil else nw // sw + 1
    return kh, kw, sh, sw, pt, pl, dh, dw, oh, ow


def pool_route(shape, k, s=(), p=(), d=(), ceil=False, cus=CUS):
    """max_pool2d_entry restated: (route, planes per workgroup)"""
    n, c, ih, iw = shape
    kh, kw, sh, sw, pt, pl, dh, dw, oh, ow = pool_dims(shape, k, s, p, d, ceil)
    pin, pout = ih * iw, oh * ow
    sep = kh * kw > kh + kw + 2
    per_plane = ((pin + 3) & ~3) + ((pout + 3) & ~3) + (ih * ow if sep else 0)
    ppb = min(12 * 1024 // max(per_plane, 1), c)
    while ppb > 1 and n * ((c + ppb - 1) // ppb) < 4 * cus:
        ppb = (ppb + 1) // 2
    if ppb >= 1 and n <= 65535 and c * pin < 2 ** 31 and c * pout < 2 ** 31 and pin % 4 == 0 and pout % 4 == 0:
        return ("pool.lds_sep" if sep else "pool.lds") + ("/pool.pbn" if ppb > 1 else "/pool.pb1"), ppb
    return ("pool.direct" if n * c * pout < 2 ** 31 and n * c * pin < 2 ** 31 else "pool.direct_i64"), 0


def P(route, shape, k, s=(), p=(), d=(), ceil=False, view=None, window=None, ppb=None, why=""):
    return dict(route=route, shape=shape, args=(list(k), list(s), list(p), list(d), ceil), view=view, window=window, ppb=ppb, why=why)


POOL_ROWS = [
    P("pool.lds/pool.pb1", (1, 3, 8, 8), [2, 2], [2, 2], ppb=1, why="4 cells <= kh + kw + 2: the (kh, kw) scan in LDS; 3 planes: one a workgroup"),
    P("pool.lds_sep/pool.pb1", (1, 3, 8, 8), [5, 5], [1, 1], [2, 2, 2, 2], ppb=1, why="25 cells > 12: rows, then columns"),
    P("pool.lds_sep/pool.pb1", (1, 3, 8, 8), [3, 3], [2, 2], [1, 1, 1, 1], ppb=1, why="9 cells > 8, stride 2"),
    P("pool.lds_sep/pool.pbn", (1, 2049, 4, 4), [3, 3], [1, 1], [1, 1, 1, 1], ppb=2, why="1025 groups of 2 >= 1024: the last group holds one plane"),
    P("pool.lds_sep/pool.pbn", (2, 2049, 4, 4), [3, 3], [1, 1], [1, 1, 1, 1], ppb=4, why="two images: 2 x 513 groups of 4, the last of each one plane"),
    P("pool.lds/pool.pbn", (1, 2049, 4, 4), [2, 2], [2, 2], ppb=2, why="the scan kernel, 2 planes a group, ragged"),
    P("pool.lds_sep/pool.pbn", (1, 2048, 4, 4), [3, 3], [1, 1], [1, 1, 1, 1], ppb=2, why="C % pb == 0: 1024 full groups"),
    P("pool.lds/pool.pbn", (3, 1368, 2, 4), [1, 2], [1, 2], ppb=4, why="3 x 342 groups of 4, C % pb == 0, a 1 x 2 window"),
    P("pool.direct", (1, 3, 6, 6), [2, 2], [1, 1], why="25 outputs a plane: no multiple of 4"),
    P("pool.direct", (2, 3, 7, 9), [3, 3], [2, 2], [1, 1, 1, 1], why="a 7 x 9 plane: 63 inputs"),
    P("pool.direct", (1, 1, 112, 112), [2, 2], [2, 2], why="12544 + 3136 floats a plane exceed the 12288 of LDS"),
    P("pool.lds_sep/pool.pb1", (1, 3, 8, 8), [3, 3], [1, 1], [2, 2, 2, 2], [2, 2], ppb=1, why="dilation 2"),
    P("pool.direct", (1, 2, 7, 9), [3, 3], [1, 1], [], [2, 2], why="dilation 2, no padding: 3 x 5 outputs"),
    P("pool.lds_sep/pool.pb1", (1, 3, 8, 8), [3], [2], [1], ppb=1, why="a [3] kernel, a one-entry pad list: both stand for both axes and ends"),
    P("pool.lds_sep/pool.pb1", (1, 3, 8, 8), [3, 3], [2, 2], [], [], True, ppb=1, why="ceil_mode: the last window holds one row / column of input"),
    P("pool.direct", (1, 2, 7, 7), [3, 3], [2, 2], [], [], True, why="ceil_mode on an odd plane: the floor result, 3 x 3"),
    P("pool.lds/pool.pb1", (1, 2, 4, 8), [1, 1], [2, 2], [0, 0, 2, 0], ppb=1, why="k = 1, s = 2, bottom pad 2: the third output row lies wholly outside"),
    P("pool.direct", (1, 2, 4, 4), [1, 1], [2, 2], [0, 0, 2, 0], why="the same window on 3 x 2 outputs"),
    P("pool.lds_sep/pool.pbn", (2, 2049, 4, 4), [3, 3], [1, 1], [1, 1, 1, 1], view=(2053, 3), window=(2051, 1), ppb=4,
      why="channels 3 .. 2051 of 2053 into channels 1 .. 2049 of 2051"),
    P("pool.lds_sep/pool.pb1", (2, 3, 8, 8), [5, 5], [1, 1], [2, 2, 2, 2], view=(6, 2), window=(5, 1), ppb=1, why="a channel view into a window"),
    P("pool.direct", (2, 3, 6, 6), [2, 2], [1, 1], view=(6, 2), window=(5, 1), why="the one-output-per-thread kernel through both pitches"),
]
POOL_IDS = ["%d-%s-%s" % (i, r["route"].replace("/", "+"), "x".join(map(str, r["shape"]))) for i, r in enumerate(POOL_ROWS)]

NAN2 = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)   # quiet, negative, signalling, all ones


def _nans(rng, n):
    return NAN2[rng.integers(0, 4, n)]


def pf_random(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def pf_zeros(rng, shape):
    """+0, -0 and -1 at random: windows hold the two zeros in both orders, within a row and across rows"""
    return np.array([0.0, -0.0, -1.0], np.float32)[rng.integers(0, 3, shape)]


def pf_nan_cells(rng, shape):
    """a NaN (four payloads) at a quarter of the cells: first, middle and last cells of windows"""
    x = rng.standard_normal(shape).astype(np.float32)
    m = rng.random(shape) < 0.25
    x[m] = _nans(rng, int(m.sum()))
    return x


def pf_nan_window(rng, shape):
    """the upper left 7 x 7 corner of every plane and all of every third plane is NaN: all-NaN windows, which give -inf"""
    x = rng.standard_normal(shape).astype(np.float32)
    x[:, :, :7, :7] = _nans(rng, x[:, :, :7, :7].size).reshape(x[:, :, :7, :7].shape)
    x[:, ::3] = np.float32(np.nan)
    return x


def pf_neginf_window(rng, shape):
    """the same regions -inf"""
    x = rng.standard_normal(shape).astype(np.float32)
    x[:, :, :7, :7] = -np.inf
    x[:, ::3] = -np.inf
    return x


def pf_inf_mix(rng, shape):
    """+inf and -inf at a fifth of the cells each, a NaN at a tenth"""
    x = rng.standard_normal(shape).astype(np.float32)
    u = rng.random(shape)
    x[u < 0.2] = np.inf
    x[(u >= 0.2) & (u < 0.4)] = -np.inf
    x[u > 0.9] = np.nan
    return x


POOL_FAMILIES = [("random", pf_random), ("zeros", pf_zeros), ("nan_cells", pf_nan_cells), ("nan_window", pf_nan_window),
                 ("neginf_window", pf_neginf_window), ("inf_mix", pf_inf_mix)]


def _padded(x, args):
    k, s, p, d, ceil = args
    kh, kw, sh, sw, pt, pl, dh, dw, oh, ow = pool_dims(x.shape, k, s, p, d, ceil)
    n, c, ih, iw = x.shape
    xp = np.full((n, c, pt + max(ih, oh * sh + dh * kh), pl + max(iw, ow * sw + dw * kw)), -np.inf, np.float32)
    xp[:, :, pt:pt + ih, pl:pl + iw] = x
    return xp, (kh, kw, sh, sw, dh, dw, oh, ow)


def _keep(out, tap, mode):
    with np.errstate(invalid="ignore"):
        if mode == "first":
            return np.where(tap > out, tap, out)
        if mode == "last":
            return np.where(tap >= out, tap, out)
        return np.maximum(out, tap)   # "nan": propagates


def pool_scan(x, args, mode):
    """the (kh, kw) scan with a pluggable comparison; mode "first" is the operation"""
    xp, (kh, kw, sh, sw, dh, dw, oh, ow) = _padded(x, args)
    out = np.full(x.shape[:2] + (oh, ow), -np.inf, np.float32)
    for a in range(kh):
        for b in range(kw):
            out = _keep(out, xp[:, :, a * dh:a * dh + oh * sh:sh, b * dw:b * dw + ow * sw:sw], mode)
    return out


def pool_separable(x, args, row_mode, col_mode):
    """max_pool2d_lds_kernel's separable form: the maximum of every row's window, then over the window's rows"""
    xp, (kh, kw, sh, sw, dh, dw, oh, ow) = _padded(x, args)
    rows = np.full(xp.shape[:3] + (ow,), -np.inf, np.float32)
    for b in range(kw):
        rows = _keep(rows, xp[:, :, :, b * dw:b * dw + ow * sw:sw], row_mode)
    out = np.full(x.shape[:2] + (oh, ow), -np.inf, np.float32)
    for a in range(kh):
        out = _keep(out, rows[:, :, a * dh:a * dh + oh * sh:sh], col_mode)
    return out


def pool_literal(x, args):
    """conv2d.rs:1222-1251, loop for loop"""
    k, s, p, d, ceil = args
    kh, kw, sh, sw, pt, pl, dh, dw, oh, ow = pool_dims(x.shape, k, s, p, d, ceil)
    n, c, ih, iw = x.shape
    out = np.empty((n, c, oh, ow), np.float32)
    for b in range(n):
        for ch in range(c):
            for y in range(oh):
                for xx in range(ow):
                    max_val = np.float32(-np.inf)
                    for ki in range(kh):
                        r = y * sh + ki * dh - pt
                        if r < 0 or r >= ih:
                            continue
                        for kj in range(kw):
                            q = xx * sw + kj * dw - pl
                            if q < 0 or q >= iw:
                                continue
                            val = x[b, ch, r, q]
                            if val > max_val:
                                max_val = val
                    out[b, ch, y, xx] = max_val
    return out


VARIANTS_POOL = [   # (name, emulation, applies(row), the families that must each tell it from the operation)
    ("a NaN propagates", lambda x, a: pool_scan(x, a, "nan"), lambda r: True, ("nan_cells", "nan_window", "inf_mix")),
    (">=: the last of equal values wins", lambda x, a: pool_scan(x, a, "last"), lambda r: r["args"][0][0] * r["args"][0][-1] > 1, ("zeros",)),
    ("separable, the row pass keeps the last", lambda x, a: pool_separable(x, a, "last", "first"), lambda r: "lds_sep" in r["route"], ("zeros",)),
    ("separable, the column pass keeps the last", lambda x, a: pool_separable(x, a, "first", "last"), lambda r: "lds_sep" in r["route"], ("zeros",)),
]


@functools.lru_cache(maxsize=None)
def pool_case(i, fam):
    row = POOL_ROWS[i]
    f = [name for name, _ in POOL_FAMILIES].index(fam)
    x = POOL_FAMILIES[f][1](np.random.default_rng([7, i, f]), row["shape"])
    want = npref.max_pool2d(x, *row["args"])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


# --------------------------------------------------------------------------------------------------------------------- top-k
def topk_route(n, k):
    k = min(k, n)
    if n > 1024 and k <= 1024:
        return "topk.select_lds" if n <= 28672 else "topk.select_l2"
    return "topk.rank"


TOPK_ROWS = [   # (route, n, k, condition)
    ("topk.rank", 1, 1, "n <= 1024"), ("topk.rank", 3, 2, "n <= 1024"), ("topk.rank", 3, 3, "k == n"), ("topk.rank", 255, 17, "one partial workgroup"),
    ("topk.rank", 256, 256, "one whole workgroup, k == n"), ("topk.rank", 257, 100, "a second workgroup with one element"),
    ("topk.rank", 1024, 300, "the longest row ranked"), ("topk.rank", 1024, 1024, "k == n"),
    ("topk.rank", 2049, 1025, "k > 1024: more candidates than the select kernels hold; a second 2048-element chunk of one element"),
    ("topk.rank", 2049, 2049, "k == n over two chunks"), ("topk.rank", 5000, 1025, "three chunks: whole chunks before and after an element's own"),
    ("topk.select_lds", 1025, 300, "n > 1024, k <= 1024, the keys staged in LDS"), ("topk.select_lds", 1025, 1024, "k at its most"),
    ("topk.select_lds", 28672, 300, "the longest staged row"), ("topk.select_l2", 28673, 301, "one more: swept from L2"),
]
TOPK_IDS = ["%d-%s-n%d-k%d" % (i, r[0], r[1], r[2]) for i, r in enumerate(TOPK_ROWS)]


def _nan_tagged(idx):
    """a NaN whose payload names its index, the sign alternating"""
    return ((np.uint32(0x7FC00000) | (np.asarray(idx, np.uint32) & np.uint32(0x3FFFFF))) | (np.asarray(idx, np.uint32) & np.uint32(1)) << np.uint32(31)).view(np.float32)


def tf_ties(rng, n, k):
    return np.round(rng.standard_normal(n) * 3).astype(np.float32)


def tf_equal(rng, n, k):
    return np.full(n, 2.5, np.float32)


def tf_zeros(rng, n, k):
    return np.array([0.0, -0.0, 1.0, -1.0], np.float32)[rng.integers(0, 4, n)]


def tf_inf(rng, n, k):
    x = tf_ties(rng, n, k)
    u = rng.random(n)
    x[u < 0.2] = np.inf
    x[u > 0.8] = -np.inf
    return x


def tf_nan_some(rng, n, k):
    x = tf_ties(rng, n, k)
    at = np.unique(np.concatenate([[0, n // 2, n - 1], rng.integers(0, n, max(1, n // 16))]))
    x[at] = _nan_tagged(at)
    return x


def tf_nan_most(rng, n, k):
    """fewer non-NaN elements than k (k // 2 of them): the result ends in NaNs, lower index first"""
    x = _nan_tagged(np.arange(n))
    keep = rng.permutation(n)[:k // 2]
    x[keep] = np.round(rng.standard_normal(len(keep)) * 3).astype(np.float32)
    return x


def tf_nan_all(rng, n, k):
    return _nan_tagged(np.arange(n))


TOPK_FAMILIES = [("ties", tf_ties), ("equal", tf_equal), ("zeros", tf_zeros), ("inf", tf_inf), ("nan_some", tf_nan_some), ("nan_most", tf_nan_most),
                 ("nan_all", tf_nan_all)]


@functools.lru_cache(maxsize=None)
def topk_case(i):
    """x [families, n]; per direction the oracle's (values, indices)"""
    _, n, k, _ = TOPK_ROWS[i]
    x = np.stack([f(np.random.default_rng([11, i, j]), n, k) for j, (_, f) in enumerate(TOPK_FAMILIES)])
    x.setflags(write=False)
    return x, {largest: npref.topk(x, k, largest) for largest in (True, False)}


def topk_order(x, k, largest, nan_first=False, high_index_first=False):
    """a sort-based top-k with the two wrong orders switchable; with neither it restates npref.topk"""
    n = x.shape[-1]
    res = []
    for row in x:
        key = np.where(np.isnan(row), -np.inf if nan_first else np.inf, -row if largest else row).astype(np.float64)
        idx = np.arange(n)
        order = np.lexsort((-idx if high_index_first else idx, key))[:k]
        res.append(order)
    order = np.array(res)
    return np.take_along_axis(x, order, -1), order.astype(np.float32)


VARIANTS_TOPK = [
    ("a NaN ranks first", dict(nan_first=True), ("nan_some", "nan_most")),
    ("equal values: the higher index first", dict(high_index_first=True), ("ties", "equal", "zeros", "inf", "nan_all")),
]


# ---------------------------------------------------------------------------------------------------------------------- cast
def rust_i64_as_f32(v):
    """Rust's `i64 as f32`: round to nearest, ties to even -- in integer arithmetic"""
    out = []
    for i in np.asarray(v).reshape(-1).tolist():
        a = abs(i)
        if a.bit_length() > 24:
            sh = a.bit_length() - 24
            q, r = divmod(a, 1 << sh)
            q += 1 if (r > (1 << (sh - 1)) or (r == (1 << (sh - 1)) and q & 1)) else 0
            a = q << sh
        out.append(float(-a if i < 0 else a))   # exact in f64, and in f32
    return np.array(out, np.float32).reshape(np.shape(v))


def _nextafter32(v, to):
    return np.nextafter(np.float32(v), np.float32(to))


CAST_F32 = np.array([np.nan, -np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 63, -2.0 ** 63, _nextafter32(2.0 ** 63, 0), _nextafter32(2.0 ** 63, np.inf),
                     _nextafter32(-2.0 ** 63, 0), _nextafter32(-2.0 ** 63, -np.inf), 2.0 ** 62, -2.0 ** 62, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32 + 512, -0.0, 0.0, 0.99,
                     -0.99, 1.7, -2.2, 3.0, 1e-40, -1e-40, 1.4e-45, 16777217.0, -8388607.5, 3.4e38, -3.4e38], np.float32)
CAST_I64 = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), -(2 ** 24 + 3), 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 63 - 1, -(2 ** 63 - 1), -2 ** 63, 0, 1, -1,
                     2 ** 24, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 40 + 2 ** 16, 2 ** 40 + 2 ** 16 + 1, 2 ** 62 + 2 ** 38, 2 ** 62 + 3 * 2 ** 38, 123456789012345678], np.int64)
CAST_I32 = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 31 - 1, -2 ** 31, -1, 0, 5, 2 ** 30 + 2 ** 6], np.int32)


def cast_x86(v):
    """a non-saturating f32 -> i64: cvttss2si's "integer indefinite" -2^63 for a NaN and everything out of range"""
    want = rust_f32_as_i64(v)
    f = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(f) | (f >= np.float32(2.0 ** 63)) | (f < np.float32(-2.0 ** 63)), np.int64(-2 ** 63), want)


# =============================================================================================================== CPU tests
def all_routes():
    used = {r["route"] for r in COPY_ROWS} | {r["route"] for r in RESIZE_ROWS} | {r["route"] for r in POOL_ROWS} | {r[0] for r in TOPK_ROWS}
    used |= {r[0] for r in CPITCH_ROWS} | {"pad.index", "gather.rows", "gather.elements", "apool.window", "tcp.tile32", "range.f32", "range.i64",
                                          "fill.words", "cast.convert"}
    return {lvl for r in used for lvl in r.split("/") if lvl}


def test_rows_cover_every_data_movement_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}   # every other name: tests/test_f32_routes.py, tests/test_attention_routes.py
    used = all_routes()
    assert not (used | set(NOT_COVERED)) - mine, "routes the library cannot report: %s" % sorted((used | set(NOT_COVERED)) - mine)
    assert not used & set(NOT_COVERED)
    assert mine - used == set(NOT_COVERED), "routes no row reaches: %s" % sorted(mine - used - set(NOT_COVERED))
    # both LDS pool kernels with one and with several planes a workgroup
    assert {"%s/%s" % (a, b) for a in ("pool.lds", "pool.lds_sep") for b in ("pool.pb1", "pool.pbn")} <= {r["route"] for r in POOL_ROWS}


def test_rows_satisfy_the_dispatch_conditions_they_state():
    for row in COPY_ROWS:
        assert copy_route(copy_launches(row), row["dt"].itemsize) == row["route"], row
    for row in RESIZE_ROWS:
        n, c, h, w = row["shape"]
        oh, ow = int(h * row["scales"][0]), int(w * row["scales"][1])
        xp, xo = (row["view"][0] * h * w, row["view"][1] * h * w) if row["view"] else (0, 0)
        op, oo = (row["window"][0] * oh * ow, row["window"][1] * oh * ow) if row["window"] else (0, 0)
        assert resize_route(row["shape"], oh, ow, row["mode"] == "asymmetric", xp, op, xo, oo) == row["route"], row
    for row in POOL_ROWS:
        route, ppb = pool_route(row["shape"], *row["args"])
        assert route == row["route"] and (ppb == 0 or ppb == row["ppb"]), (row, route, ppb)
        if route.endswith("pool.pbn"):   # the ragged rows really end in a partial group, the others do not
            assert (row["shape"][1] % ppb != 0) == ("C % pb == 0" not in row["why"]), row
    for route, n, k, _ in TOPK_ROWS:
        assert topk_route(n, k) == route, (route, n, k)
    for route, dt, shape, c0, c1, _ in CPITCH_ROWS:
        per = int(np.prod(shape[2:])) * dt.itemsize
        row, off, pitch = (c1 - c0) * per, c0 * per, shape[1] * per
        dp = (c1 - c0 + 3) * per   # the windowed call's destination pitch (test_cpitch_rows)
        for dst in ((row,), (per, dp)):   # dense result; window at channel 1 of c + 3
            w = 16 if all(v % 16 == 0 for v in (row, off, pitch) + dst) else 4 if all(v % 4 == 0 for v in (row, off, pitch) + dst) else 1
            assert "cpitch.w%d" % w == route, (route, shape, dst)
    # the 64-bit routes: 2^31 elements select them in the restated dispatch
    assert copy_route([([2 ** 31 + 8, 3], [1, 2 ** 31 + 8], [0, 0], [3, 1], 0, 0)], 4) == "copy.w4/copy.i64"
    assert pool_route((1, 2 ** 19 + 1, 64, 66), [2, 2], [1, 1])[0] == "pool.direct_i64"


def test_pure_copy_inputs_have_pairwise_distinct_words():
    for row in COPY_ROWS:
        w = np.concatenate([bits(x).reshape(-1) for x in copy_inputs(row)])
        assert len(np.unique(w)) == len(w), row
    for dt in (F32, I64):
        for n in (1 << 16, 65536 * 64):
            w = words(n, dt.itemsize)
            assert len(np.unique(w)) == n
    f = words(1 << 16, 4).view(np.float32)
    assert np.isnan(f).any() and (np.abs(f[~np.isnan(f)]) < np.float32(1.2e-38)).any()   # NaN payloads and denormals are among them
    assert len(np.unique(words(256, 1))) == 256


def test_copy_references_are_the_index_maps_of_their_launches():
    """the numpy reference of every row == the row's launch descriptors applied by index arithmetic (what the dispatch test reads)"""
    for row in COPY_ROWS:
        if int(np.prod(row["shape"][0] if row["kind"] == "concat" else row["shape"], dtype=np.int64)) > 1 << 16 or row["kind"] in ("split", "concat"):
            continue
        x = copy_inputs(row)[0]
        oshape, istr, imod, _, ioff, _ = copy_launches(row)[-1]
        co = np.indices(oshape).reshape(len(oshape), -1)
        src = ioff + sum((co[k] % imod[k] if imod[k] else co[k]) * istr[k] for k in range(len(oshape)))
        assert same_bits(x.reshape(-1)[src].reshape(oshape), copy_reference(row, [x])[0]), row


def test_tile_rows_tell_a_missing_store_predicate():
    """the off-by-one at a tile edge: a kernel that clamps its loads but stores from every lane.  On every ragged tile row the stray
    stores that fall inside the result change it; the emulation with the predicate is the reference"""
    seen = 0
    for row in COPY_ROWS:
        if not row["route"].startswith("copy.tile") or row["kind"] in ("expand",) or row["shape"][0] > 64:
            continue
        x = copy_inputs(row)[0]
        launch, want = copy_launches(row)[0], copy_reference(row, [x])[0]
        assert same_bits(tile_emulation(launch, x), want), row
        ragged = launch[0][-1] % 64 != 0 or any(o % 64 for o, i in zip(launch[0][:-1], launch[1][:-1]) if i == 1)
        if ragged:
            assert not same_bits(tile_emulation(launch, x, predicate=False), want), row
            seen += 1
    assert seen >= 6


def test_npref_max_pool2d_is_the_literal_scan():
    for i, row in enumerate(POOL_ROWS):
        if int(np.prod(row["shape"])) > 2000:
            continue
        for fam, _ in POOL_FAMILIES:
            x, want = pool_case(i, fam)
            assert same_bits(want, pool_literal(x, row["args"])), (row, fam)
    x = pool_case(0, "nan_cells")[0]   # the clean-data behaviour of the former np.maximum oracle is unchanged
    clean = np.nan_to_num(x, nan=1.0) + 0.0
    assert same_bits(npref.max_pool2d(clean, [2, 2], [2, 2]), pool_scan(clean, ([2, 2], [2, 2], [], [], False), "nan"))


def test_pool_families_tell_wrong_comparisons():
    """on every row and family the restated scan is the oracle and the separable form with first-wins passes keeps its bits (the
    claim in max_pool2d_lds_kernel); every wrong variant is told apart by each of its families on at least one row"""
    seen = {(name, fam): False for name, _, _, fams in VARIANTS_POOL for fam in fams}
    for i, row in enumerate(POOL_ROWS):
        if row["view"] or row["shape"][1] > 2048:   # the same cases through pitches; one 2049-plane row is enough
            continue
        for fam, _ in POOL_FAMILIES:
            x, want = pool_case(i, fam)
            assert same_bits(pool_scan(x, row["args"], "first"), want)
            assert same_bits(pool_separable(x, row["args"], "first", "first"), want), (row, fam)
            for name, emul, applies, fams in VARIANTS_POOL:
                if fam in fams and applies(row) and not same_bits(emul(x, row["args"]), want):
                    seen[(name, fam)] = True
    assert all(seen.values()), "no row tells: %s" % [k for k, v in seen.items() if not v]
    # all-NaN and all -inf windows give -inf
    for fam in ("nan_window", "neginf_window"):
        assert np.all(pool_case(1, fam)[1][:, 0] == -np.inf) and np.all(pool_case(1, fam)[1][:, 1, 0, 0] == -np.inf)
    assert np.all(pool_case(16, "random")[1][:, :, 2] == -np.inf)   # the wholly outside row


def test_topk_families_tell_wrong_orders():
    seen = {(name, fam): False for name, _, fams in VARIANTS_TOPK for fam in fams}
    fams = [name for name, _ in TOPK_FAMILIES]
    for i, (_, n, k, _) in enumerate(TOPK_ROWS):
        if n > 5000:
            continue
        x, want = topk_case(i)
        for largest in (True, False):
            v, ix = topk_order(x, k, largest)
            assert same_bits(v, want[largest][0]) and np.array_equal(ix, want[largest][1]), (n, k, largest)
            for name, kw, vf in VARIANTS_TOPK:
                wv, wi = topk_order(x, k, largest, **kw)
                for fam in vf:
                    j = fams.index(fam)
                    if not (same_bits(wv[j], want[largest][0][j]) and np.array_equal(wi[j], want[largest][1][j])):
                        seen[(name, fam)] = True
    assert all(seen.values()), "no row tells: %s" % [k for k, v in seen.items() if not v]


def test_cast_restatements():
    want = rust_f32_as_i64(CAST_F32)
    assert want[:8].tolist() == [0, 0, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, -2 ** 63]
    assert want[8] == 2 ** 63 - 2 ** 39 and want[10] == -(2 ** 63 - 2 ** 39) and want[17:23].tolist() == [0, 0, 0, 0, 1, -2]
    inside = np.abs(CAST_F32.astype(np.float64)) < 2.0 ** 63
    assert np.array_equal(want[inside], CAST_F32[inside].astype(np.int64))   # numpy agrees wherever C defines the conversion
    assert not np.array_equal(cast_x86(CAST_F32), want)                      # the special values tell a non-saturating cast
    assert np.array_equal(cast_x86(CAST_F32[inside]), want[inside])
    f = rust_i64_as_f32(CAST_I64)
    assert f[:4].tolist() == [2.0 ** 24, 2.0 ** 24 + 4, -2.0 ** 24, -2.0 ** 24 - 4] and f[4] == 2.0 ** 53 and f[6] == 2.0 ** 63 and f[8] == -2.0 ** 63
    assert same_bits(f, CAST_I64.astype(np.float32))
    assert index_of(GATHER_IDX["f32"], 5).tolist() == [[0, 0, 4], [4, 2, 0]]


# =============================================================================================================== GPU tests
def expect_route(K, ctx, want):
    got = K.last_route(ctx)
    assert got == want, "route moved: the library ran %r, the row covers %r" % (got, want)
    assert set(filter(None, got.split("/"))) <= set(K.route_names())


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(COPY_ROWS)), ids=COPY_IDS)
def test_copy_rows(ctx, i):
    from lele_amd import kernels as K
    row = COPY_ROWS[i]
    xs = copy_inputs(row)
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)   # another route first: a stale name would show
    got = copy_run(K, ctx, row, xs)
    expect_route(K, ctx, row["route"])
    want = copy_reference(row, xs)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = g.numpy()
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = bits(g) != bits(w)
        assert not bad.any(), "%s: %d of %d words differ, the first at %s" % (row["why"], int(bad.sum()), bad.size, np.argwhere(bad)[0])


@pytest.mark.gpu
def test_view_copy_chain(ctx):
    """view_copy materialises a slice / reshape / transpose chain through the same engine"""
    from lele_amd import kernels as K
    x = tagged((2, 70, 3, 24), F32)
    got = K.view_copy(ctx.buf().upload(x), [["slice", 1, 3, 65], ["transpose", [0, 2, 3, 1]]], ctx=ctx)
    expect_route(K, ctx, "copy.tile_w4")
    assert same_bits(got.numpy(), np.ascontiguousarray(x[:, 3:68].transpose(0, 2, 3, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(PAD_ROWS)))
def test_pad_rows(ctx, i):
    from lele_amd import kernels as K
    dt, shape, pads, mode, cv = PAD_ROWS[i]
    x = tagged(shape, dt)
    got = K.pad(ctx.buf().upload(x), pads, None if cv is None else np.array([cv], dt), mode, ctx=ctx)
    expect_route(K, ctx, "pad.index")
    want = npref.pad(x, pads, 0 if cv is None else np.array(cv, dt), mode)
    assert same_bits(got.numpy(), want), (shape, pads, mode)
    if mode == "constant":
        assert (bits(got.numpy()) == bits(np.array([cv], dt))[0]).sum() == got.numpy().size - x.size   # the fill's own bits, sign and high half


@pytest.mark.gpu
def test_gather_rows(ctx):
    from lele_amd import kernels as K
    for dt, name, shape, axis in GATHER_ROWS:
        x, idx = tagged(shape, dt), GATHER_IDX[name]
        for dev in (False, True):   # host-visible indices are checked on the host first, device-resident ones in the kernel
            got = K.gather(ctx.buf().upload(x), ctx.buf().upload(idx) if dev else idx, axis, ctx=ctx)
            expect_route(K, ctx, "gather.rows")
            assert same_bits(got.numpy(), np.take(x, index_of(idx, shape[axis]), axis=axis)), (dt, name, shape, axis)
    rng = np.random.default_rng(3)
    for xs, ishape, axis in GE_ROWS:
        x = tagged(xs, F32)
        dim = xs[axis]
        idx = (rng.integers(-dim, dim, ishape) + rng.choice([0.0, 0.25, 0.9], ishape) * (rng.integers(-dim, dim, ishape) >= 0)).astype(np.float32)
        idx = np.where((idx >= dim) | (index_of(idx, dim) >= dim), np.float32(0), idx).astype(np.float32)
        got = K.gather_elements(ctx.buf().upload(x), idx, axis, ctx=ctx)
        expect_route(K, ctx, "gather.elements")
        assert same_bits(got.numpy(), gather_elements_reference(x, idx, axis)), (xs, ishape, axis)
    ctx.sync()   # no index was out of range


def _parent(n, c_total, c0, x, outside):
    """x [n, c, ..] as channels c0 .. c0 + c of a parent whose other channels hold `outside` (an array [n, c_total, ..] or a value)"""
    par = np.array(np.broadcast_to(outside, (n, c_total) + x.shape[2:]), dtype=x.dtype)
    par[:, c0:c0 + x.shape[1]] = x
    return par


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(RESIZE_ROWS)), ids=["%d-%s" % (i, r["route"]) for i, r in enumerate(RESIZE_ROWS)])
def test_resize_rows(ctx, i):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    row = RESIZE_ROWS[i]
    n, c, h, w = row["shape"]
    oh, ow = int(h * row["scales"][0]), int(w * row["scales"][1])
    if row["view"]:   # the parent carries the tagging: x is its channel window
        ct, c0 = row["view"]
        par = tagged((n, ct, h, w), F32)
        x, src = np.ascontiguousarray(par[:, c0:c0 + c]), TensorView(ctx.buf().upload(par)).channels(c0, c0 + c)
    else:
        x = tagged(row["shape"], F32)
        src = ctx.buf().upload(x)
    want = npref.resize_nearest(x, oh, ow, row["mode"] == "asymmetric")
    kw = dict(scales=[1, 1, row["scales"][0], row["scales"][1]], coordinate_transform_mode=row["mode"], ctx=ctx)
    if row["window"]:
        ot, o0 = row["window"]
        sent = np.full((n, ot, oh, ow), -7.25, np.float32)
        ob = ctx.buf()
        ob.upload(sent)
        got = K.resize_nearest(src, out=ob, out_window=(o0 * oh * ow, ot * oh * ow), **kw)
        expect_route(K, ctx, row["route"])
        sent[:, o0:o0 + c] = want
        assert same_bits(ob.to_numpy(sent.shape), sent), "the window or its surroundings differ"
    else:
        got = K.resize_nearest(src, **kw)
        expect_route(K, ctx, row["route"])
    assert same_bits(got.numpy(), want), row["why"]


@pytest.mark.gpu
def test_transpose_cp_rows(ctx):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    for c in TCP_SIZES:
        for pos in TCP_SIZES:
            par = tagged((2, c + 3, pos), F32)
            src = TensorView(ctx.buf().upload(par)).channels(2, 2 + c)
            want = np.ascontiguousarray(par[:, 2:2 + c].transpose(0, 2, 1))
            got = K.transpose_cp(src, ctx=ctx)
            expect_route(K, ctx, "tcp.tile32")
            assert same_bits(got.numpy(), want), (c, pos, "dense")
            sent = np.full((2, pos + 5, c), -7.25, np.float32)
            ob = ctx.buf()
            ob.upload(sent)
            got = K.transpose_cp(src, out=ob, out_window=(3 * c, (pos + 5) * c), ctx=ctx)
            expect_route(K, ctx, "tcp.tile32")
            sent[:, 3:3 + pos] = want
            assert same_bits(ob.to_numpy(sent.shape), sent) and same_bits(got.numpy(), want), (c, pos, "window")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CPITCH_ROWS)), ids=["%d-%s" % (i, r[0]) for i, r in enumerate(CPITCH_ROWS)])
def test_cpitch_rows(ctx, i):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    route, dt, shape, c0, c1, why = CPITCH_ROWS[i]
    par = tagged(shape, dt)
    src = TensorView(ctx.buf().upload(par)).channels(c0, c1)
    want = np.ascontiguousarray(par[:, c0:c1])
    got = K.copy_view(src, ctx=ctx)
    expect_route(K, ctx, route)
    assert same_bits(got.numpy(), want), why
    per = int(np.prod(shape[2:]))
    sent = np.full((shape[0], c1 - c0 + 3) + shape[2:] + (dt.itemsize,), 0x5A, np.uint8).view(dt)[..., 0]   # the sentinel: every byte 0x5A
    ob = ctx.buf()
    ob.upload(sent)
    got = K.copy_view(src, out=ob, out_window=(per, (c1 - c0 + 3) * per), ctx=ctx)
    expect_route(K, ctx, route)
    sent[:, 1:1 + c1 - c0] = want
    assert same_bits(ob.to_numpy(sent.shape, dt), sent) and same_bits(got.numpy(), want), why


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(POOL_ROWS)), ids=POOL_IDS)
def test_pool_rows(ctx, i):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    row = POOL_ROWS[i]
    n, c = row["shape"][:2]
    failures = []
    for fam, _ in POOL_FAMILIES:
        x, want = pool_case(i, fam)
        if row["view"]:   # the other channels of the parent are +inf: a read outside the view wins every window
            ct, c0 = row["view"]
            src = TensorView(ctx.buf().upload(_parent(n, ct, c0, x, np.float32(np.inf)))).channels(c0, c0 + c)
        else:
            src = ctx.buf().upload(x)
        if row["window"]:
            ot, o0 = row["window"]
            plane = want.shape[2] * want.shape[3]
            sent = np.full((n, ot) + want.shape[2:], -7.25, np.float32)
            ob = ctx.buf()
            ob.upload(sent)
            got = K.max_pool2d(src, *row["args"], out=ob, out_window=(o0 * plane, ot * plane), ctx=ctx)
            expect_route(K, ctx, row["route"])
            sent[:, o0:o0 + c] = want
            if not same_bits(ob.to_numpy(sent.shape), sent):
                failures.append("%s: the window or its surroundings differ" % fam)
        else:
            got = K.max_pool2d(src, *row["args"], ctx=ctx)
            expect_route(K, ctx, row["route"])
        g = got.numpy()
        assert g.shape == want.shape
        bad = bits(g) != bits(want)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            failures.append("%s: %d of %d outputs differ, the first at %s: got %r want %r" % (fam, int(bad.sum()), bad.size, at, g[at], want[at]))
    assert not failures, row["why"] + "\n" + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TOPK_ROWS)), ids=TOPK_IDS)
def test_topk_rows(ctx, i):
    from lele_amd import kernels as K
    route, n, k, why = TOPK_ROWS[i]
    x, want = topk_case(i)
    dev = ctx.buf().upload(x)
    failures = []
    for largest in (True, False):
        # the result buffers are prefilled: a slot the kernel leaves unwritten shows
        ov, oi = ctx.buf(), ctx.buf()
        ov.upload(np.full((x.shape[0], k), -7.25, np.float32))
        oi.upload(np.full((x.shape[0], k), -7.25, np.float32))
        v, ix = K.topk(dev, k, -1, largest, True, out_values=ov, out_indices=oi, ctx=ctx)
        expect_route(K, ctx, route)
        v, ix = v.numpy(), ix.numpy()
        for j, (fam, _) in enumerate(TOPK_FAMILIES):
            bad = (bits(v[j]) != bits(want[largest][0][j])) | (ix[j] != want[largest][1][j])
            if bad.any():
                at = int(np.argwhere(bad)[0][0])
                failures.append("%s, largest=%s: %d of %d slots differ, the first at %d: got (%r, %r) want (%r, %r)" % (
                    fam, largest, int(bad.sum()), k, at, v[j, at], ix[j, at], want[largest][0][j, at], want[largest][1][j, at]))
    assert not failures, why + "\n" + "\n".join(failures)


@pytest.mark.gpu
def test_cast_rows(ctx):
    from lele_amd import kernels as K
    got = K.cast_to_i64(CAST_F32, ctx=ctx)
    expect_route(K, ctx, "cast.convert")
    got, want = got.numpy(), rust_f32_as_i64(CAST_F32)
    print("f32 -> i64 on the device: " + "  ".join("%r -> %d" % (float(f), int(g)) for f, g in zip(CAST_F32, got)))
    bad = got != want
    assert not bad.any(), "f32 -> i64: %s" % ["%r: got %d want %d" % (float(f), int(g), int(w)) for f, g, w in zip(CAST_F32[bad], got[bad], want[bad])]
    assert same_bits(K.cast_to_f32(CAST_I64, ctx=ctx).numpy(), rust_i64_as_f32(CAST_I64))
    assert same_bits(K.cast_to_f32(CAST_I32, ctx=ctx).numpy(), rust_i64_as_f32(CAST_I32))
    neg = np.array([-1, -2 ** 31, 2 ** 31 - 1, -123456789, 0], np.int32)
    assert np.array_equal(K.cast_to_i64(neg, ctx=ctx).numpy(), neg.astype(np.int64))
    u = np.arange(256, dtype=np.uint8)
    for src in (u, u.view(np.int8)):
        assert same_bits(K.cast_to_f32(src, ctx=ctx).numpy(), np.array([float(v) for v in src.tolist()], np.float32))
        assert np.array_equal(K.cast_to_i64(src, ctx=ctx).numpy(), np.array(src.tolist(), np.int64))
    expect_route(K, ctx, "cast.convert")
    assert K.cast_to_i64(np.zeros((0,), np.float32), ctx=ctx).shape == (0,)
    expect_route(K, ctx, "")


@pytest.mark.gpu
def test_range_fill_rows(ctx):
    from lele_amd import kernels as K
    start, delta, n = np.float32(0.1), np.float32(0.3), 70000
    limit = np.float32(start + np.float32(n - 0.5) * delta)
    assert int(np.ceil(np.float32(np.float32(limit - start) / delta))) == n
    got = K.range([start], [limit], [delta], ctx=ctx)
    expect_route(K, ctx, "range.f32")
    i = np.arange(n, dtype=np.float32)   # exact up to 2^24
    want = (start + (i * delta).astype(np.float32)).astype(np.float32)   # both roundings: the product, then the sum (math.rs:2049-2053)
    assert same_bits(got.numpy(), want)
    fused = (np.float64(start) + i.astype(np.float64) * np.float64(delta)).astype(np.float32)
    assert not same_bits(fused, want)   # 70000 elements tell a fused multiply-add from the two roundings
    assert K.range([3.0], [1.0], [1.0], ctx=ctx).shape == (0,)
    expect_route(K, ctx, "")
    from lele_amd import _lib
    import ctypes as Ct
    for s, d, m in ((5, -3, 300), (-2 ** 62, 2 ** 40 + 1, 257)):
        out, sh = ctx.buf(), _lib.OutShape()
        _lib.check(_lib.lib().lele_hip_range_i64(ctx._h, Ct.c_int64(s), Ct.c_int64(d), Ct.c_int64(m), out._h, sh.shape, Ct.byref(sh.rank)))
        expect_route(K, ctx, "range.i64")
        assert sh.get() == (m,) and np.array_equal(out.to_numpy((m,), np.int64), s + d * np.arange(m, dtype=np.int64))
    for dt, value in ((F32, -0.0), (F32, NAN2[1]), (I64, -0x0123456789ABCDEF), (I32, -5)):
        for m in (1, 255, 257):
            got = K.constant_of_shape(np.array([m], np.int64), value, dt, ctx=ctx)
            expect_route(K, ctx, "fill.words")
            assert same_bits(got.numpy(), np.full((m,), value, dt)), (dt, m)
    assert K.constant_of_shape(np.array([3, 0], np.int64), 1.0, ctx=ctx).shape == (3, 0)
    expect_route(K, ctx, "")
    got = K.adaptive_avg_pool1d(np.arange(12, dtype=np.float32).reshape(2, 6), 3, ctx=ctx)
    expect_route(K, ctx, "apool.window")
    assert np.array_equal(got.numpy(), npref.adaptive_avg_pool1d(np.arange(12, dtype=np.float32).reshape(2, 6), 3))
