"""Every element-wise, reduce and norm route (lele_amd/csrc/eltwise.hip) against a plain reference: one table row per dispatch branch,
threshold side and refusal.

Behind each entry point of eltwise.hip the host picks a kernel by alignment, broadcast pattern, element type, row length, row count and
the CU count.  Every row names the route the library must report (kernels.last_route()) and the condition that selects it, so a re-tune
that moves a shape to another kernel fails here instead of leaving that kernel untested.

References.  Polynomial bodies and the norms: oracle/pyoracle (the reference's own AVX2 sequence), bit for bit; the oracle itself is
pinned to float64 on finite families, and on constant / outlier / overflowing rows -- where float64 cannot agree with f32 statistics --
to a line-by-line numpy restatement of the 4x8 accumulation (layer_norm_np, rms_norm_np, softmax_np).  libm tails: the same formula with
each libm call taken in float64 and every step rounded to f32 (unary_ref); judged with 1e-4 |ref| + 1e-7 on bounded inputs, by class
(NaN / +-inf / +-0 / finite) outside.  One-rounding ops, broadcast ops, where, clip, reductions: oracle/npref, bit for bit; i64 ops in
integer arithmetic.  A comparison "by bits" accepts any NaN where the reference yields a NaN and asserts the NaN masks equal
(accept_bits); no row drops elements.

CPU part: name coverage, every row against the dispatch restated in Python for 256 CUs, the references against each other, and emulated
wrong kernels (MUTATIONS) failing the acceptance functions the GPU part uses.
GPU part: every row asserts last_route() and then the values."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from oracle import npref

CUS = 256
F32, I64 = np.dtype(np.float32), np.dtype(np.int64)
FLT_MAX, FLT_MIN = np.float32(3.40282347e+38), np.float32(1.17549435e-38)
PREFIXES = ("unary.", "bin.", "binp.", "where.", "clip.", "reduce.", "ln.", "softmax.", "rows.", "rms.", "bn.", "add3.", "hpas.")

# what no row asserts, and why (a key that is a route name takes that name out of the coverage requirement; there is none)
NOT_COVERED = {
    "softmax: a NaN in a row": "the reference's _mm256_max_ps(acc, load) keeps or drops a NaN depending on the accumulator slot and the "
                               "position it sits in, the device takes the row maximum with fmaxf (a NaN never wins): neither is asserted",
    "binary: n >= 2^32 refusal of bin.fast": "the 32-bit index guard of binary_fast_kernel needs a 16 GiB result",
    "reduce: on >= 2^34 / on > 65535 guards": "the row-count guards of the min / max kernels need 2^34 output rows, or 65536 rows of 65536",
    "binary_pitched: image >= 2^32 elements": "an error, not a route; needs a 16 GiB image",
}


def prod(v):
    return int(np.prod(list(v), dtype=np.int64))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ============================================================================================================ acceptance
def accept_bits(got, want):
    """"" when got == want bit for bit -- any NaN where the reference yields a NaN, the NaN masks equal -- else what differs"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, want %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~wn & (bits(got) != bits(want)))
    else:
        bad = got != want
    if not bad.any():
        return ""
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d of %d differ, the first at %s: got %r want %r" % (int(bad.sum()), bad.size, at, got[at], want[at])


def accept_value(got, want):
    """equal as numbers (-0 == +0), the NaN masks equal"""
    got, want = np.asarray(got), np.asarray(want)
    ok = got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    return "" if ok else "values differ: got %r want %r" % (got, want)


def klass(v):
    """NaN 0, +inf 1, -inf 2, +0 3, -0 4, finite 5"""
    v = np.asarray(v, np.float32)
    return np.where(np.isnan(v), 0, np.where(np.isinf(v), np.where(v > 0, 1, 2), np.where(v == 0, np.where(np.signbit(v), 4, 3), 5)))


def accept_close(got, ref, inb, rel=1e-4, floor=1e-7):
    """libm results: |got - ref| <= rel |ref| + floor where `inb` (the input is inside the op's bounds), the same class elsewhere"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    with np.errstate(all="ignore"):
        close = np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= rel * np.abs(ref.astype(np.float64)) + floor
    close |= (klass(got) == klass(ref)) & ~np.isfinite(ref)   # a NaN or an infinity inside the bounds: the same one
    bad = np.where(inb, ~close, klass(got) != klass(ref))
    if not bad.any():
        return ""
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d of %d outside the tolerance / class, the first at %s: got %r want %r" % (int(bad.sum()), bad.size, at, got[at], ref[at])


# ================================================================================================================= unary
POLY = ("exp", "sigmoid", "tanh", "silu", "erf", "gelu", "fast_gelu")            # polynomial 8-wide body, libm tail
ONE = ("relu", "sqrt", "neg", "abs", "floor", "ceil", "reciprocal", "not_")      # one rounding: the same bits in body and tail
LIBM = ("log", "sin", "cos", "softplus")                                         # libm for every element
KNAME = {"tanh": "tanh_kernel"}
BOUND = {"log": None, "sin": 1e5, "cos": 1e5}                                    # every other libm op: |x| <= 80 (the exp family)
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _lm(fn, x):
    """one libm call: float64, rounded to f32"""
    with np.errstate(all="ignore"):
        return fn(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def unary_ref(name, x):
    """the reference's scalar formula (avx/math.rs tails, math.rs:893-1104), every step in f32, each libm call through float64"""
    x = np.asarray(x, np.float32)
    one, half = np.float32(1), np.float32(0.5)
    with np.errstate(all="ignore"):
        if name == "exp":
            return _lm(np.exp, x)
        if name == "sigmoid":
            return one / (one + _lm(np.exp, -x))
        if name == "tanh":
            return _lm(np.tanh, x)
        if name == "silu":
            return x / (one + _lm(np.exp, -x))
        if name == "erf":
            return _lm(_erf, x)
        if name == "gelu":
            return x * half * (one + _lm(_erf, x * np.float32(0.7071067811865475)))
        if name == "fast_gelu":
            inner = np.float32(0.7978845608028654) * (x + np.float32(0.044715) * x * x * x)
            return half * x * (one + _lm(np.tanh, inner))
        if name == "softplus":   # log(f32(1 + f32(exp x))), not log1p: math.rs:1046-1056
            return np.where(x > np.float32(20), x, _lm(np.log, one + _lm(np.exp, x))).astype(np.float32)
        if name in ("log", "sin", "cos"):
            return _lm(getattr(np, name), x)
    raise KeyError(name)


def bounded(name, x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        if name == "log":
            return (x >= FLT_MIN) & (x <= FLT_MAX)
        return np.abs(x) <= np.float32(BOUND.get(name, 80.0))


def unary_want(name, x, orc):
    """the reference of a whole buffer: oracle bits (body and, for the one-rounding ops, tail), unary_ref where libm decides"""
    x = np.asarray(x, np.float32)
    if name in LIBM:
        return unary_ref(name, x)
    if name in ("relu", "sqrt") or name in POLY:
        return orc.unary(name, x)
    return npref.unary_exact(name, x)


def check_unary(name, x, got, orc):
    """the acceptance of one unary result: "" or what is wrong"""
    x, got = np.asarray(x, np.float32).reshape(-1), np.asarray(got).reshape(-1)
    body = x.size & ~7
    want = unary_want(name, x, orc)
    if name in LIBM:
        return accept_close(got, want, bounded(name, x))
    if name in ONE:
        if name == "relu":   # a tail -0: `x.max(0.0)` keeps it or not depending on the build -- by value there
            return accept_bits(got[:body], want[:body]) or accept_value(got[body:], want[body:])
        return accept_bits(got, want)
    return accept_bits(got[:body], want[:body]) or accept_close(got[body:], unary_ref(name, x[body:]), bounded(name, x[body:]))


def _next(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


SPECIALS = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1.1754942e-38, -1.1754942e-38, FLT_MIN, -FLT_MIN, 1.0, -1.0,
                     -87.33654, _next(-87.33654, False), _next(-87.33654, True), 88.72284, _next(88.72284, False), _next(88.72284, True),
                     44.0, -44.0, 44.5, -44.5, 1e30, -1e30, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], np.float32)


def specials_in_every_lane():
    """SPECIALS eight times, shifted by one lane each time (every special meets every lane position of an 8-chunk), padded with 0.5"""
    parts = []
    for p in range(8):
        seg = np.concatenate([np.full(p, 0.5, np.float32), SPECIALS])
        parts.append(np.concatenate([seg, np.full(-seg.size % 8, 0.5, np.float32)]))
    x = np.concatenate(parts)
    assert x.size % 8 == 0
    return x


def specials_tails():
    """the table again behind a whole-chunk body, seven specials at a time in the tail"""
    body = specials_in_every_lane()[:64]
    return [np.concatenate([body, SPECIALS[k:k + 7]]) for k in range(0, SPECIALS.size, 7)]


def binade_sweep(per=8, seed=11):
    """log-uniform over every binade of both signs, subnormal ones included: `per` values a binade, a whole number of 8-chunks"""
    rng = np.random.default_rng(seed)
    e = np.repeat(np.arange(-149, 128), per).astype(np.float64)
    mag = np.ldexp(1.0 + rng.uniform(0, 1, e.size), e.astype(np.int64)).astype(np.float32)
    x = np.concatenate([mag, -mag])
    rng.shuffle(x)
    return x[:x.size & ~7]


BIG_UNARY = 4 * 4096 * 256 + 11
UNARY_ROWS = [   # route, length, byte offset of the input pointer, why
    ("unary.vec4", 8, 0, "one whole 8-chunk: two float4, no tail"),
    ("unary.vec4", 13, 0, "a float4 of the tail (elements 8..11) and one remainder element"),
    ("unary.vec4", 1003, 0, "several blocks' worth of float4, 3 tail elements in the remainder loop"),
    ("unary.vec4", BIG_UNARY, 0, "nvec > 4096 * 256: a second grid-stride trip, the float4 remainder and the libm tail (len % 8 == 3)"),
    ("unary.w1", 1003, 4, "refusal: the input pointer is 4 bytes past a 16-byte boundary"),
]


def unary_route(length, off):
    return "" if length == 0 else "unary.vec4" if off % 16 == 0 else "unary.w1"


def grid_for(n):
    return max(1, min((n + 255) // 256, 4096))


# ================================================================================================================ binary
def bcast(shapes):
    """make_bcast: the broadcast shape and each operand's strides (0 on broadcast dims)"""
    rank = max(len(s) for s in shapes)
    osh = [1] * rank
    for d in range(rank):
        for s in shapes:
            od = d - (rank - len(s))
            dim = 1 if od < 0 else s[od]
            if dim != 1:
                assert osh[d] in (1, dim)
                osh[d] = dim
    strides = []
    for s in shapes:
        st, acc = [0] * rank, 1
        for d in range(rank - 1, -1, -1):
            od = d - (rank - len(s))
            dim = 1 if od < 0 else s[od]
            st[d] = 0 if dim == 1 else acc
            acc *= dim
        strides.append(st)
    return osh, strides


def fast_map(osh, stride, addr, n, count):
    """binary_fast_map: (inner, len, full) or None"""
    if addr % 16:
        return None
    if count == n:
        return (1, 1, 1)
    run = [d for d in range(len(osh)) if stride[d] != 0 and osh[d] != 1]
    if not run:
        return (1, 1, 0)
    if any(stride[d] == 0 and osh[d] != 1 for d in range(run[0], run[-1] + 1)):
        return None
    inner, ln = prod(osh[run[-1] + 1:]), prod(osh[run[0]:run[-1] + 1])
    if not (inner % 4 == 0 or (inner == 1 and ln % 4 == 0)):
        return None
    return (inner, ln, 0)


def binary_route(sa, sb, dt=F32, offs=(0, 0)):
    osh, (sta, stb) = bcast([sa, sb])
    n = prod(osh)
    if n == 0:
        return ""
    same = prod(sa) == n and prod(sb) == n
    if dt == F32 and n < 2 ** 32 and fast_map(osh, sta, offs[0], n, prod(sa)) and fast_map(osh, stb, offs[1], n, prod(sb)):
        return "bin.fast"
    return ("bin.flat_" if same else "bin.index_") + ("f32" if dt == F32 else "i64")


def fast_geometry(n):
    """binary_fast_kernel's launch: does the two-chunk loop run, do some threads (not all) take the single-chunk epilogue behind it, is
    the grid capped, how many trips does the loop make at most"""
    blocks = grid_for((n + 7) // 8)
    gs, nvec = blocks * 256, n // 4
    g = np.arange(gs, dtype=np.int64)
    trips = np.maximum(0, -(-(nvec - gs - g) // (2 * gs)))
    last = g + 2 * gs * trips < nvec   # the threads that take the single-chunk epilogue
    return dict(two_chunk=nvec > gs, epilogue=bool(last.any() and not last.all()), capped=((n + 7) // 8 + 255) // 256 > 4096,
                trips=int(trips.max()), scalar_tail=n % 4)


BIN_OPS = ("add", "sub", "mul", "div", "max", "min", "equal", "less", "greater", "prelu", "mod_f32", "and_", "or_")
BIG_FAST = 3 * 2 ** 22 + 1003
BINARY_ROWS = [   # route, shape a, shape b, dtype, byte offsets of the operand pointers, why
    ("bin.fast", (2, 3, 4), (2, 3, 4), F32, (0, 0), "both operands full"),
    ("bin.fast", (5, 7), (1,), F32, (0, 0), "a scalar operand: n % 4 == 3, the scalar remainder loop"),
    ("bin.fast", (1,), (5, 8), F32, (0, 0), "the scalar on the left"),
    ("bin.fast", (3, 5, 8), (8,), F32, (0, 0), "a trailing bias: inner == 1, len % 4 == 0"),
    ("bin.fast", (2, 6, 2, 4), (6, 1, 1), F32, (0, 0), "per-channel over NCHW on the right: inner = 8"),
    ("bin.fast", (1, 5, 1, 1), (2, 5, 3, 4), F32, (0, 0), "per-channel on the left: inner = 12"),
    ("bin.fast", (3000,), (3000,), F32, (0, 0), "nvec 750 > gstride 512, 750 % 512 != 0: the two-chunk loop and the epilogue behind it"),
    ("bin.fast", (BIG_FAST,), (1,), F32, (0, 0), "n > 8 * 256 * 4096: the capped grid, the two-chunk loop makes a second trip"),
    ("bin.index_f32", (2, 6, 3, 2), (6, 1, 1), F32, (0, 0), "refusal: inner = 6, inner % 4 != 0"),
    ("bin.index_f32", (3, 5, 6), (6,), F32, (0, 0), "refusal: inner == 1 with len 6 % 4 != 0"),
    ("bin.index_f32", (3, 1, 8), (1, 4, 8), F32, (0, 0), "refusal: a broadcast dimension inside the run of both operands"),
    ("bin.flat_f32", (6, 8), (6, 8), F32, (4, 0), "refusal: operand a 4 bytes past a 16-byte boundary, equal shapes"),
    ("bin.index_f32", (6, 8), (8,), F32, (0, 4), "refusal: operand b 4 bytes past a 16-byte boundary, broadcast"),
    ("bin.flat_i64", (5, 7), (5, 7), I64, (0, 0), "i64, equal shapes"),
    ("bin.index_i64", (5, 7), (7,), I64, (0, 0), "i64, the index walk"),
    ("bin.index_f32", (2 ** 20 + 5, 3), (1, 3), F32, (0, 0), "over 2^20 elements through the index walk: a second grid-stride trip (inner 3 % 4 != 0)"),
]

# special values for the broadcast ops: the cross product of these on both sides
BIN_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, FLT_MAX, -FLT_MAX, 1.4e-45, -1.1754942e-38, 2.5, -0.75], np.float32)
I64_SPECIALS = np.array([0, 1, -1, 2, -2, 3, -3, 7, -7, 10 ** 9 + 7, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3, 2 ** 62 + 12345, -(2 ** 62 + 12345),
                         2 ** 63 - 1, -(2 ** 63 - 1), 123456789012345678, -987654321098765432], np.int64)


def cross(v):
    a, b = np.meshgrid(v, v, indexing="ij")
    return np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b.reshape(-1))


def i64_literal(op, a, b):
    """i64 div / mod one pair at a time in Python integers: truncation toward zero, the remainder has the dividend's sign, x / 0 -> 0"""
    out = []
    for x, y in zip(a.tolist(), b.tolist()):
        if y == 0:
            out.append(0)
            continue
        q = abs(x) // abs(y) * (1 if (x < 0) == (y < 0) else -1)
        out.append(q if op == "div" else x - q * y)
    return np.array(out, np.int64)


BINP_ROWS = [   # route, parent shape, channel window of a, of b, result window (c0 of a parent with C + 3 channels), why
    ("binp.vec4", (2, 6, 2, 4), (2, 5), (0, 3), 2, "offsets 16 and 0, pitch 48, result offset 16 / pitch 48: all multiples of 4"),
    ("binp.w1", (2, 5, 3, 3), (1, 4), (0, 3), 1, "refusal: the image pitch 45 is not a multiple of 4"),
    ("binp.w1", (2, 4, 2, 3), (1, 3), (2, 4), 2, "refusal: the window of operand a starts at the odd channel 1 = element 6 (pitch 24 % 4 == 0)"),
]


def binp_route(parent, wa, wb, oc0):
    n, ct = parent[:2]
    plane = prod(parent[2:])
    c = wa[1] - wa[0]
    offs = (wa[0] * plane, wb[0] * plane, oc0 * plane)
    pitches = (ct * plane, ct * plane, (c + 3) * plane)
    return "binp.vec4" if all(o % 4 == 0 for o in offs) and all(p % 4 == 0 for p in pitches) else "binp.w1"


# ================================================================================================================ reduce
def reduce_route(op, shape, axes, cus=CUS):
    dims = len(shape)
    mask = [False] * dims
    for a in axes:
        mask[a + dims if a < 0 else a] = True
    if not axes:
        mask = [True] * dims
    istr = [prod(shape[d + 1:]) for d in range(dims)]
    red = [(shape[d], istr[d]) for d in range(dims) if mask[d]]
    keep = [(shape[d], istr[d]) for d in range(dims) if not mask[d]]
    rc, on = prod(s for s, _ in red), prod(s for s, _ in keep)
    if on == 0:
        return ""
    rows_first = op in ("max", "min") and len(red) == 1 and red[0][1] == 1 and rc >= 16 and on < 2 ** 34
    expect = rc
    for ks, kst in reversed(keep):   # the kept dims row after row
        if not rows_first:
            break
        rows_first = kst == expect
        expect *= ks
    if rows_first and on <= 2 * cus and rc >= 65536 and on <= 65535:
        return "reduce.parts"
    return "reduce.rows16" if rows_first else "reduce.seq"


def R(route, op, shape, axes, why):
    """shape: a tuple, or a function of the CU count"""
    return dict(route=route, op=op, shape=shape, axes=axes, why=why)


REDUCE_ROWS = [R("reduce.seq", op, (3, 50, 7), [1], "%s over a middle axis" % op) for op in ("sum", "mean", "l2", "max", "min")]
REDUCE_ROWS += [R("reduce.seq", op, (3, 50, 7), ax, "%s, several axes / kept dims not row after row: axes %s" % (op, ax))
                for op in ("sum", "max", "min") for ax in ([0, 2], [1, 2], [0, 1, 2], [])]
REDUCE_ROWS += [R("reduce.seq", op, (37, 15), [-1], "%s over a last axis of 15 < 16" % op) for op in ("max", "min", "sum")]
REDUCE_ROWS += [R("reduce.seq", op, (4, 32, 1), [1], "%s: the reduced axis is contiguous but a kept dim of 1 follows it: the layout check refuses" % op)
                for op in ("max", "min")]
for _op in ("max", "min"):
    REDUCE_ROWS += [
        R("reduce.rows16", _op, (37, 16), [-1], "%s over a last axis of exactly 16; 37 rows, no multiple of 16" % _op),
        R("reduce.rows16", _op, (2, 19, 17), [2], "%s over 17: the second trip of a lane holds one element; 38 rows" % _op),
        R("reduce.rows16", _op, (5, 1, 80), [-1], "%s with a kept dim of 1 before the axis" % _op),
        R("reduce.rows16", _op, (1, 65535), [1], "%s: red_count 65535 < 65536 stays on 16 lanes a row" % _op),
        R("reduce.parts", _op, (1, 65536), [1], "%s: red_count 65536, one row: 8 pieces of 8192" % _op),
        R("reduce.parts", _op, (3, 300001), [-1], "%s: pieces of 8192, the last one 5089 long" % _op),
        R("reduce.parts", _op, (9000001,), [0], "%s: a global reduction, per = 8790 > 8192, the last piece shorter" % _op),
        R("reduce.parts", _op, lambda cus: (2 * cus, 65536), [1], "%s: on == 2 * CUs" % _op),
        R("reduce.rows16", _op, lambda cus: (2 * cus + 1, 65536), [1], "%s: on == 2 * CUs + 1 leaves the two-stage form" % _op),
    ]
REDUCE_ROWS.append(R("reduce.seq", "sum", (40, 200), [0], "200 outputs: four blocks of 64 threads, the last one 8 live"))


def row_shape(row, cus=CUS):
    return row["shape"](cus) if callable(row["shape"]) else row["shape"]


def minmax_rows(x, op):
    """max / min of every row of x [rows, n] as the sequential scan gives it (NaN never wins, the first of equal values stays, +-inf
    for a row of NaN), without a Python loop over n: npref.reduce restated for the long rows (pinned against it on the CPU)"""
    x = np.asarray(x, np.float32)
    seed = np.float32(-np.inf if op == "max" else np.inf)
    xx = np.where(np.isnan(x), seed, x)
    m = xx.max(axis=1) if op == "max" else xx.min(axis=1)
    hit = (xx == m[:, None]) & ~np.isnan(x)
    first = hit.argmax(axis=1)
    out = x[np.arange(x.shape[0]), first]
    return np.where(hit.any(axis=1), out, seed).astype(np.float32)


def reduce_input(shape, seed, specials=True):
    """random values; on the first rows of the last axis: +-0 ties both ways round, a NaN inside a row, a row of NaN"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape, dtype=np.float32) * np.float32(3)
    if specials and len(shape) >= 1:
        v = x.reshape(-1, shape[-1])
        n = shape[-1]
        if v.shape[0] >= 1 and n >= 3:   # every value <= 0 (max) is told by row 0, >= 0 (min) by row 1: the first zero decides the sign
            v[0] = -np.abs(v[0])
            v[0, n // 3], v[0, 2 * n // 3] = -0.0, 0.0
        if v.shape[0] >= 2 and n >= 3:
            v[1] = np.abs(v[1])
            v[1, n // 3], v[1, 2 * n // 3] = 0.0, -0.0
        if v.shape[0] >= 3:
            v[2, n // 2] = np.nan
        if v.shape[0] >= 4:
            v[3] = np.nan
    return x


def reduce_want(op, x, axes):
    if op in ("max", "min") and x.ndim >= 1 and len(axes) == 1 and axes[0] in (-1, x.ndim - 1) and x.shape[-1] > 4096:
        return minmax_rows(x.reshape(-1, x.shape[-1]), op).reshape(x.shape[:-1])
    return npref.reduce(op, x, axes, False)


# ================================================================================================================= norms
LENGTHS = (1, 7, 8, 9, 31, 32, 33, 40, 55, 255, 256, 257, 511, 512, 513, 563, 1023, 1024, 1025, 1031)   # 55, 563: two remainder chunks
OUTERS = (1, 2, 3, 1023, 1024, 1027, 4095, 4096, 4099)
OUTER_LENGTHS = (9, 40)   # many rows only at short lengths: one tail element; one whole and one remainder register row
VALUE_LENGTHS = (8, 64, 520)


def norm_route(kind, length, outer):
    if length * outer == 0:
        return ""
    if kind == "rms":
        return "rms.stream"
    if length > 1024:
        return kind + ".stream"
    return "%s.reg%d/rows.rpb%d" % (kind, 8 if length <= 256 else 16 if length <= 512 else 32, 8 if outer >= 4096 else 4 if outer >= 1024 else 2)


def fma32(a, b, c):
    """_mm256_fmadd_ps on f32 arrays: the product is exact in float64, one rounding of the sum (to 53 bits, then to 24)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def row_sums_np(v, square, order="4x8", pad=False):
    """avx/norm.rs: four 8-wide accumulators over whole 32-chunks, (s0 + s1) + (s2 + s3), the 8-wide remainder chunks into the merged
    vector, the horizontal sum (i) + (i + 4), (i) + (i + 2), [0] + [1], then the scalar tail.  Emulated wrong kernels: order="seq" adds
    left to right; pad=True counts the clamped copies of the last element that fill the last register row"""
    v = np.asarray(v, np.float32)
    rows, n = v.shape
    with np.errstate(all="ignore"):
        if pad and n % 32:
            v = np.concatenate([v, np.repeat(v[:, -1:], 32 - n % 32, axis=1)], axis=1)
            n = v.shape[1]
        if order == "seq":
            s = np.zeros(rows, np.float32)
            for k in range(n):
                s = fma32(v[:, k], v[:, k], s) if square else s + v[:, k]
            return s
        acc = np.zeros((rows, 32), np.float32)
        j = 0
        while j + 32 <= n:
            c = v[:, j:j + 32]
            acc = fma32(c, c, acc) if square else acc + c
            j += 32
        sv = (acc[:, 0:8] + acc[:, 8:16]) + (acc[:, 16:24] + acc[:, 24:32])
        while j + 8 <= n:
            c = v[:, j:j + 8]
            sv = fma32(c, c, sv) if square else sv + c
            j += 8
        s = sv[:, 0:4] + sv[:, 4:8]
        s = s[:, 0:2] + s[:, 2:4]
        s = s[:, 0] + s[:, 1]
        for k in range(j, n):
            s = s + v[:, k] * v[:, k] if square else s + v[:, k]
        return s.astype(np.float32)


def layer_norm_np(x, g, b, eps, order="4x8", pad=False):
    x = np.asarray(x, np.float32)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        inv_n = np.float32(1) / np.float32(n)
        mean = row_sums_np(x, False, order, pad) * inv_n
        var = row_sums_np(x, True, order, pad) * inv_n - mean * mean
        inv_std = np.float32(1) / np.sqrt(var + np.float32(eps))
        t = (x - mean[:, None]) * inv_std[:, None]
        body = n & ~7
        return np.concatenate([fma32(t[:, :body], g[None, :body], b[None, :body]), t[:, body:] * g[None, body:] + b[None, body:]], axis=1).astype(np.float32)


def rms_norm_np(x, w, eps, order="4x8"):
    x = np.asarray(x, np.float32)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        rms_inv = np.float32(1) / np.sqrt(row_sums_np(x, True, order) * (np.float32(1) / np.float32(n)) + np.float32(eps))
        body = n & ~7
        return np.concatenate([x[:, :body] * (w[None, :body] * rms_inv[:, None]), x[:, body:] * rms_inv[:, None] * w[None, body:]], axis=1).astype(np.float32)


def softmax_np(x, orc, order="4x8", miss_last=False):
    """rows without a NaN, a whole number of 8-chunks (no libm tail); the polynomial exp is the oracle's"""
    x = np.asarray(x, np.float32)
    assert x.shape[1] % 8 == 0
    with np.errstate(all="ignore"):
        m = np.maximum(np.float32(-FLT_MAX), (x[:, :-1] if miss_last else x).max(axis=1))
        e = orc.unary("exp", (x - m[:, None]).reshape(-1)).reshape(x.shape)
        return (e * (np.float32(1) / row_sums_np(e, False, order))[:, None]).astype(np.float32)


NORM_FAMILIES = ("random", "constant", "constant_large", "squares_overflow", "subnormals", "outlier", "plus_inf", "minus_inf", "nan", "sum_overflow")
SOFTMAX_FAMILIES = ("random", "masked", "all_masked", "plus_inf", "equal", "spread", "subnormals", "huge_negative")


def norm_family_rows(n, seed=5):
    """[len(NORM_FAMILIES), n]"""
    rng = np.random.default_rng(seed + n)
    x = (rng.standard_normal((len(NORM_FAMILIES), n)) * 2 + 0.3).astype(np.float32)
    x[1] = np.float32(3.7)
    x[2] = np.float32(1000.0)
    x[3] = x[3] * np.float32(3e19)
    x[4] = x[4] * np.float32(1e-40)
    x[5] = x[5] * np.float32(1e-3)
    x[5, n // 2] = np.float32(1e6)
    x[6, n // 3] = np.inf
    x[7, n // 3] = -np.inf
    x[8, n - 1] = np.nan
    x[9] = np.float32(3e38)
    return x


def softmax_family_rows(n, seed=6):
    rng = np.random.default_rng(seed + n)
    x = (rng.standard_normal((len(SOFTMAX_FAMILIES), n)) * 3).astype(np.float32)
    x[1, ::3] = -np.inf
    x[2] = -np.inf
    x[3, n // 2] = np.inf
    x[4] = np.float32(2.5)
    x[5] = np.linspace(-200, 50, n).astype(np.float32)
    x[6] = x[6] * np.float32(1e-40)
    x[7] = np.float32(-1e30)
    x[7, n - 3] = np.float32(0)
    return x


def norm_params(n, seed=9):
    rng = np.random.default_rng(seed + n)
    return (1 + 0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)


def accept_softmax(got, want, n):
    """bits when the row is whole 8-chunks; with a libm tail every output carries the tail's exponentials through the sum"""
    if n % 8 == 0:
        return accept_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    ok = got.shape == want.shape and bool(np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-9))
    return "" if ok else "softmax with a libm tail: max |diff| %r" % float(np.abs(got - want).max())


# ============================================================================================== add3, halves_pow_add_sqrt, batch_norm
ADD3_ROWS = [   # route, shapes of a, b, c, byte offset of a, why
    ("add3.vec4", [(8,)] * 3, 0, "n % 4 == 0"),
    ("add3.vec4", [(3, 7)] * 3, 0, "n % 4 == 1"),
    ("add3.vec4", [(1002,)] * 3, 0, "n % 4 == 2"),
    ("add3.vec4", [(5, 203)] * 3, 0, "n % 4 == 3, several blocks"),
    ("add3.vec4", [(2 ** 22 + 4 * 2 ** 10 + 3,)] * 3, 0, "nvec > 4096 * 256: a second grid-stride trip"),
    ("add3.w1", [(1003,)] * 3, 4, "refusal: operand a 4 bytes past a 16-byte boundary: the scalar branch"),
    ("bin.fast", [(4, 6, 8), (8,), (4, 6, 8)], 0, "broadcasting operands: two adds, the route of the second (both operands full)"),
    ("bin.index_f32", [(6, 1), (1, 7), (5, 1, 1)], 0, "the third operand broadcasts outward: the second add walks indices"),
]


def add3_route(shapes, off):
    if len(set(shapes)) > 1:
        osh, _ = bcast(shapes[:2])
        return binary_route(tuple(osh), shapes[2])
    return "" if prod(shapes[0]) == 0 else "add3.vec4" if off % 16 == 0 else "add3.w1"


HPAS_ROWS = [   # shape, axis, lo, hi, why
    ((3, 10), 1, (0, 5), (5, 10), "inner 1: the last axis in halves"),
    ((2, 8, 5), 1, (0, 4), (4, 8), "inner 5"),
    ((2, 8, 5), 1, (0, 4), (4, 2 ** 62), "an open upper bound clamps to the axis"),
    ((2, 8, 5), -2, (-8, -4), (-4, 2 ** 62), "negative bounds count from the end, a negative axis"),
    ((4, 9, 3), 1, (1, 4), (6, 9), "two windows that are not the halves"),
]
BN_SHAPES = [(6,), (6, 3), (2, 3, 7), (2, 3, 8), (2, 3, 13), (2, 5, 3, 11), (2, 3, 2 ** 18 + 5)]   # rank 1 and 2: all tail; inner 7 / 8 / 13 / 33; > 2^20


# ================================================================================================================ CPU tests
def all_routes():
    used = {r[0] for r in UNARY_ROWS} | {r[0] for r in BINARY_ROWS} | {r[0] for r in BINP_ROWS} | {r["route"] for r in REDUCE_ROWS} | {r[0] for r in ADD3_ROWS}
    used |= {norm_route(k, n, 3) for k in ("ln", "softmax", "rms") for n in LENGTHS}
    used |= {norm_route(k, n, o) for k in ("ln", "softmax") for n in OUTER_LENGTHS for o in OUTERS}
    used |= {"where.index", "clip.w1", "bn.w1", "hpas.w1"}
    return {lvl for r in used for lvl in r.split("/") if lvl}


def test_rows_cover_every_eltwise_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}   # every other name: the three other route tables
    assert len(mine) == 30
    used = all_routes()
    named = set(NOT_COVERED) & set(names)
    assert not (used | named) - mine, "routes the library cannot report: %s" % sorted((used | named) - mine)
    assert not used & named
    assert mine - used == named, "routes no row reaches: %s" % sorted(mine - used - named)
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_COVERED.values())
    # every register class with every rows-per-block class, for both kernels that have them
    for kind in ("ln", "softmax"):
        got = {norm_route(kind, n, o) for n in LENGTHS for o in (3,)} | {norm_route(kind, n, o) for n in OUTER_LENGTHS for o in OUTERS}
        assert {"%s.reg%d/rows.rpb2" % (kind, c) for c in (8, 16, 32)} | {"%s.reg8/rows.rpb%d" % (kind, r) for r in (2, 4, 8)} | {kind + ".stream"} <= got


def test_rows_satisfy_the_dispatch_conditions_they_state():
    for route, n, off, why in UNARY_ROWS:
        assert unary_route(n, off) == route, why
    n = BIG_UNARY
    assert n % 8 == 3 and (n >> 2) > 4096 * 256 and grid_for((n + 3) // 4) == 4096 and n - 4 * (n >> 2) == 3
    for route, sa, sb, dt, offs, why in BINARY_ROWS:
        assert binary_route(sa, sb, dt, offs) == route, why
    # the refusals are refused for the reason they state: the same shapes at aligned pointers / friendlier sizes take the fast path
    assert binary_route((6, 8), (6, 8)) == "bin.fast" and binary_route((6, 8), (8,)) == "bin.fast"
    assert binary_route((2, 6, 3, 4), (6, 1, 1)) == "bin.fast" and binary_route((3, 5, 8), (8,)) == "bin.fast"
    assert binary_route((3, 4, 8), (1, 4, 8)) == "bin.fast" and binary_route((3, 1, 8), (1, 4, 8)) == "bin.index_f32"
    assert binary_route((2 ** 16, 2 ** 16), (1,)) == "bin.index_f32"   # the 2^32 guard (NOT_COVERED)
    g = fast_geometry(3000)
    assert g["two_chunk"] and g["epilogue"] and not g["capped"] and (3000 // 4) % (grid_for(375) * 256) != 0
    assert not fast_geometry(1024)["two_chunk"]   # the largest fast-path case there was
    g = fast_geometry(BIG_FAST)
    assert g["capped"] and g["trips"] == 2 and g["epilogue"] and g["scalar_tail"] == 3
    assert prod((2 ** 20 + 5, 3)) > 4096 * 256
    for route, parent, wa, wb, oc0, why in BINP_ROWS:
        assert binp_route(parent, wa, wb, oc0) == route, why
        assert wa[1] - wa[0] == wb[1] - wb[0] and max(wa[1], wb[1]) <= parent[1] and oc0 <= 3   # the windows lie inside their parents
    assert (BINP_ROWS[1][1][1] * prod(BINP_ROWS[1][1][2:])) % 4 != 0                      # the pitch refuses
    assert (BINP_ROWS[2][1][1] * prod(BINP_ROWS[2][1][2:])) % 4 == 0 and (BINP_ROWS[2][2][0] * prod(BINP_ROWS[2][1][2:])) % 4 != 0   # the start does
    for row in REDUCE_ROWS:
        assert reduce_route(row["op"], row_shape(row), row["axes"]) == row["route"], row["why"]
    for op in ("max", "min"):   # each condition of the two-stage form on both sides, and min / max on every min / max route
        assert {(r["route"], row_shape(r)) for r in REDUCE_ROWS if r["op"] == op} >= {
            ("reduce.rows16", (1, 65535)), ("reduce.parts", (1, 65536)), ("reduce.parts", (2 * CUS, 65536)), ("reduce.rows16", (2 * CUS + 1, 65536)),
            ("reduce.seq", (37, 15)), ("reduce.rows16", (37, 16)), ("reduce.seq", (4, 32, 1))}
        assert {r["route"] for r in REDUCE_ROWS if r["op"] == op} == {"reduce.seq", "reduce.rows16", "reduce.parts"}
    assert reduce_route("sum", (37, 16), [-1]) == "reduce.seq" and 300001 % 8192 != 0 and -(-9000001 // 1024) > 8192
    for kind in ("ln", "softmax"):
        for a, b, cls in ((256, 257, (8, 16)), (512, 513, (16, 32))):
            assert norm_route(kind, a, 3) == "%s.reg%d/rows.rpb2" % (kind, cls[0]) and norm_route(kind, b, 3) == "%s.reg%d/rows.rpb2" % (kind, cls[1])
        assert norm_route(kind, 1024, 3) == kind + ".reg32/rows.rpb2" and norm_route(kind, 1025, 3) == kind + ".stream"
        for o, rpb in ((1023, 2), (1024, 4), (4095, 4), (4096, 8)):
            assert norm_route(kind, 40, o).endswith("rows.rpb%d" % rpb)
    # every remainder-chunk count and tail length, a last block with 1, 3 and 7 live rows
    assert {(n % 32) // 8 for n in LENGTHS} == {0, 1, 2, 3} and {n % 8 for n in LENGTHS} >= {0, 1, 3, 7}
    assert {(1027 % 4), (4099 % 8), (3 % 2), (4095 % 4)} == {3, 1} and 4095 % 8 == 7 and 1 % 2 == 1
    assert all(n % 32 != 0 for n in OUTER_LENGTHS)   # a partly filled last register row under every rows-per-block class
    for route, shapes, off, why in ADD3_ROWS:
        assert add3_route(shapes, off) == route, why
    assert {prod(s[0]) % 4 for r, s, o, w in ADD3_ROWS if r == "add3.vec4"} == {0, 1, 2, 3} and max(prod(s[0]) for r, s, o, w in ADD3_ROWS) // 4 > 4096 * 256
    assert max(prod(s) for s in BN_SHAPES) > 4096 * 256 and {prod(s[2:]) for s in BN_SHAPES if len(s) > 2} >= {7, 8, 13}


def test_reference_restatements(orc):
    # npref: max / min keep the first operand of equal values, the other one of a NaN; clamp leaves a NaN and a -0 at the bound
    a, b = cross(BIN_SPECIALS)
    for op, fn in (("max", max), ("min", min)):
        r = npref.binary(op, a, b)
        for x, y, z in zip(a, b, r):
            want = y if np.isnan(x) else x if np.isnan(y) else (x if x == y else np.float32(fn(x, y)))
            assert accept_bits(np.float32(z), np.float32(want)) == "", (op, x, y, z)
    z = npref.binary("max", np.float32([0.0, -0.0]), np.float32([-0.0, 0.0]))
    assert np.signbit(z).tolist() == [False, True]
    c = npref.clip(np.float32([np.nan, -0.0, 0.0, 5, -5, np.inf]), 0.0, 1.0)
    assert np.isnan(c[0]) and np.signbit(c[1]) and c[2:].tolist() == [0, 1, 0, 1]
    # i64 div / mod: integer arithmetic, pinned on Python integers; the float64 detour is wrong beyond 2^53
    ai, bi = cross(I64_SPECIALS)
    for op in ("div", "mod"):
        assert np.array_equal(npref.binary(op, ai, bi), i64_literal(op, ai, bi)), op
    with np.errstate(all="ignore"):
        old = np.where(bi == 0, 0, np.trunc(ai / np.where(bi == 0, 1, bi))).astype(np.int64)
    assert not np.array_equal(old, npref.binary("div", ai, bi))
    # the fast row min / max == the sequential scan, on the special rows
    x = reduce_input((6, 50), 3)
    for op in ("max", "min"):
        assert accept_bits(minmax_rows(x, op), npref.reduce(op, x, [-1], False)) == "", op
    assert np.signbit(minmax_rows(x, "max")[0]) and not np.signbit(minmax_rows(x, "min")[1]) and np.isinf(minmax_rows(x, "max")[3])


def test_oracle_against_float64_and_the_numpy_restatement(orc):
    # polynomial bodies: within the existing tolerances of float64 on finite, bounded inputs (the sweep cut to each op's range)
    sweep = binade_sweep()
    for name, bound, tol in (("exp", 80.0, 1e-4), ("sigmoid", 80.0, 1e-5), ("tanh", 44.0, 1e-5), ("silu", 80.0, 1e-5), ("erf", 80.0, 1e-5),
                             ("gelu", 80.0, 1e-5), ("fast_gelu", 9.0, 1e-5)):
        x = sweep[np.abs(sweep) <= bound]
        x = x[:x.size & ~7]
        got, ref = orc.unary(name, x), unary_ref(name, x).astype(np.float64)
        assert np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))), name
    # libm tails: an independent f32 libm passes the acceptance against the float64 reference -- the oracle's scalar mode (glibc) for
    # the ops that have a polynomial body, numpy's own f32 routines for log / sin / cos / softplus
    tails = np.concatenate([sweep, SPECIALS])
    for name in POLY + LIBM:
        ref = unary_ref(name, tails)
        if name in POLY:
            with orc.scalar():
                got = orc.unary(name, tails)
        else:
            with np.errstate(all="ignore"):
                got = (np.where(tails > np.float32(20), tails, np.log(np.float32(1) + np.exp(tails))) if name == "softplus" else getattr(np, name)(tails)).astype(np.float32)
            assert got.dtype == np.float32
        assert accept_close(got, ref, bounded(name, tails)) == "", name
    # the norms on finite random rows: float64, with the tolerances of test_oracle_norms_against_float64
    for n in VALUE_LENGTHS + (33, 1031):
        rng = np.random.default_rng(n)
        x = (rng.standard_normal((5, n)) * 2 + 0.5).astype(np.float32)
        g, b = norm_params(n)
        x64 = x.astype(np.float64)
        ref = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-5) * g + b
        assert np.allclose(orc.layer_norm(x, g, b), ref, rtol=1e-4, atol=1e-5)
        e = np.exp(x64 - x64.max(1, keepdims=True))
        assert np.allclose(orc.softmax(x), e / e.sum(1, keepdims=True), rtol=1e-5, atol=1e-8)
        assert np.allclose(orc.rms_norm(x, g), x64 / np.sqrt((x64 ** 2).mean(1, keepdims=True) + 1e-5) * g, rtol=1e-5, atol=1e-6)
    # the constant / outlier / overflowing families: the line-by-line restatement of the 4x8 accumulation, bit for bit
    for n in VALUE_LENGTHS + (7, 33, 255, 1031):
        x = norm_family_rows(n)
        g, b = norm_params(n)
        assert accept_bits(orc.layer_norm(x, g, b, -1, 1e-5), layer_norm_np(x, g, b, 1e-5)) == "", n
        assert accept_bits(orc.rms_norm(x, g, -1, 1e-6), rms_norm_np(x, g, 1e-6)) == "", n
    for n in VALUE_LENGTHS:
        x = softmax_family_rows(n)
        assert accept_bits(orc.softmax(x), softmax_np(x, orc)) == "", n
        assert not np.isnan(orc.softmax(x)).any()
    xb = np.random.default_rng(2).standard_normal((2, 3, 13)).astype(np.float32)
    s, bb, m, v = bn_params(3)
    sv = (s / np.sqrt(v + np.float32(1e-5))).astype(np.float32)
    bv = (bb - m * sv).astype(np.float32)
    want = np.concatenate([fma32(xb[..., :8], sv[None, :, None], bv[None, :, None]), xb[..., 8:] * sv[None, :, None] + bv[None, :, None]], axis=-1)
    assert accept_bits(orc.batch_norm(xb, s, bb, m, v), want.astype(np.float32)) == ""


def bn_params(c, seed=8):
    rng = np.random.default_rng(seed)
    s, bb, m = (rng.standard_normal(c).astype(np.float32) for _ in range(3))
    return s, bb, m, rng.uniform(0.5, 2, c).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- emulated wrong kernels
def unary_emulation(name, x, orc, shift=0):
    """the device kernel with its body / tail boundary moved by `shift` elements: the polynomial up to it, libm behind it"""
    x = np.asarray(x, np.float32)
    edge = min(x.size, max(0, (x.size & ~7) + shift))
    pad = np.concatenate([x[:edge], np.zeros(-edge % 8, np.float32)])
    return np.concatenate([orc.unary(name, pad)[:edge], unary_ref(name, x[edge:])])


def reduce_emulation(op, x, axes, variant):
    x = np.asarray(x, np.float32)
    ax = sorted({a + x.ndim if a < 0 else a for a in axes}) or list(range(x.ndim))
    keep = [d for d in range(x.ndim) if d not in ax]
    order = ax[::-1] if variant == "column_major" else ax
    xt = np.transpose(x, keep + order).reshape(prod(x.shape[d] for d in keep), -1)
    with np.errstate(all="ignore"):
        if op in ("max", "min"):
            out = np.full(xt.shape[0], -np.inf if op == "max" else np.inf, np.float32)
            for j in range(xt.shape[1]):
                col = xt[:, j]
                win = col > out if op == "max" else col < out
                if variant == "last_wins":
                    win |= col == out
                if variant == "nan_wins":
                    win |= np.isnan(col)
                out = np.where(win, col, out)
            return out.reshape([x.shape[d] for d in keep])
        acc = np.zeros(xt.shape[0], np.float32)
        for j in range(xt.shape[1]):
            acc = acc + xt[:, j]
        return acc.reshape([x.shape[d] for d in keep])


def fast_emulation(op, a, b, inner_scale=1):
    """binary_fast_kernel's operand fetch, p[(i / inner) % len]; inner_scale != 1: `inner` off by that factor"""
    osh, (sta, stb) = bcast([a.shape, b.shape])
    n = prod(osh)
    i = np.arange(n)
    ops = []
    for t, st in ((a, sta), (b, stb)):
        inner, ln, full = fast_map(osh, st, 0, n, t.size)
        ops.append(t.reshape(-1)[i if full else (i // max(1, inner // inner_scale)) % ln])
    return npref.binary(op, ops[0], ops[1]).reshape(osh)


LAST_CHUNK = np.float32([-39.863247, -39.84371, -8.996337, -2.998779, -4.5421247, -39.64835, -3.956044, -2.862027])   # where the polynomials and libm part in the last bits


def test_acceptance_rejects_emulated_wrong_kernels(orc):
    """every variant differs from the reference in at least one output bit on the inputs the GPU part uses, and the acceptance function
    the GPU part applies rejects it; the emulation without the fault is accepted"""
    seen = {}

    def told(name, reference, wrong, verdict):
        assert accept_bits(wrong, reference) != "", "%s: the variant gives the reference's bits on this input" % name
        assert verdict != "", "%s: the acceptance lets the variant pass" % name
        seen[name] = True

    # the body / tail boundary one 8-chunk early (libm inside the body) and late (the polynomial in the tail)
    rng = np.random.default_rng(3)
    for name in POLY:
        x = np.concatenate([(rng.standard_normal(56) * 4).astype(np.float32), LAST_CHUNK, np.float32([-44.5, -200.0, 3.0, -1e-3, 0.5])])
        assert check_unary(name, x, unary_emulation(name, x, orc), orc) == "", name
        early = unary_emulation(name, x, orc, -8)
        told("boundary_early." + name, unary_emulation(name, x, orc), early, check_unary(name, x, early, orc))
    for name, why in (("tanh", "the polynomial's NaN at -44.5"), ("exp", "the polynomial's clamp at -200"), ("fast_gelu", "NaN"), ("erf", "1e-3")):
        x = np.concatenate([(rng.standard_normal(56) * 4).astype(np.float32), LAST_CHUNK, np.float32([-44.5, -200.0, 3.0, -1e-3, 0.5])])
        late = unary_emulation(name, x, orc, 8)
        if name == "erf" and check_unary(name, x, late, orc) == "":
            continue   # Abramowitz-Stegun is inside the tail's tolerance at these points: not claimed
        told("boundary_late." + name, unary_emulation(name, x, orc), late, check_unary(name, x, late, orc))
    assert seen.get("boundary_late.tanh") and seen.get("boundary_late.exp")
    # row sums left to right; the clamped padding of the last register row counted; the last row of the last block not written
    for n in (40, 520):
        x = np.concatenate([norm_family_rows(n), (np.random.default_rng(n).standard_normal((3, n)) * 2 + 0.3).astype(np.float32)])
        g, b = norm_params(n)
        want = orc.layer_norm(x, g, b, -1, 1e-5)
        for name, wrong in (("ln_sequential_sums", layer_norm_np(x, g, b, 1e-5, order="seq")), ("ln_padding_counted", layer_norm_np(x, g, b, 1e-5, pad=True))):
            told("%s.%d" % (name, n), want, wrong, accept_bits(wrong, want))
        wrong = want.copy()
        wrong[-1] = 0
        told("ln_last_row_unwritten.%d" % n, want, wrong, accept_bits(wrong, want))
        wrong = rms_norm_np(x, g, 1e-6, order="seq")
        told("rms_sequential_sums.%d" % n, orc.rms_norm(x, g, -1, 1e-6), wrong, accept_bits(wrong, orc.rms_norm(x, g, -1, 1e-6)))
    for n in (64, 520):
        x = softmax_family_rows(n)
        x[0, -1] = np.float32(9.0)   # the row maximum in the last position
        want = orc.softmax(x)
        told("softmax_sequential_sums.%d" % n, want, softmax_np(x, orc, order="seq"), accept_softmax(softmax_np(x, orc, order="seq"), want, n))
        told("softmax_max_misses_last.%d" % n, want, softmax_np(x, orc, miss_last=True), accept_softmax(softmax_np(x, orc, miss_last=True), want, n))
    # min / max: the last of equal values, a NaN winning; the reduced dims walked column-major
    for shape, axes in (((37, 16), [-1]), ((3, 50, 7), [1])):
        x = reduce_input(shape, 4)
        if axes == [1]:
            x[0, 10, 0], x[0, 30, 0], x[0, :, 0] = 0.0, -0.0, -np.abs(x[0, :, 0])
            x[0, 10, 0], x[0, 30, 0] = 0.0, -0.0
            x[1, 5, 2] = np.nan
        for op in ("max", "min"):
            want = npref.reduce(op, x, axes, False)
            assert accept_bits(reduce_emulation(op, x, axes, None), want) == ""
            for variant in ("last_wins", "nan_wins"):
                wrong = reduce_emulation(op, x, axes, variant)
                if variant == "last_wins" and accept_bits(wrong, want) == "":
                    continue   # this op's tie sits in the other op's row
                told("reduce_%s.%s" % (variant, op), want, wrong, accept_bits(wrong, want))
    assert all(seen.get("reduce_%s.%s" % (v, op)) for v in ("last_wins", "nan_wins") for op in ("max", "min"))
    x = reduce_input((3, 50, 7), 5, specials=False)
    want = npref.reduce("sum", x, [0, 2], False)
    told("reduce_column_major", want, reduce_emulation("sum", x, [0, 2], "column_major"), accept_bits(reduce_emulation("sum", x, [0, 2], "column_major"), want))
    # a broadcast operand indexed with `inner` off by a factor of 4
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((2, 6, 2, 4)).astype(np.float32), rng.standard_normal((6, 1, 1)).astype(np.float32)
    assert accept_bits(fast_emulation("add", a, b), npref.binary("add", a, b)) == ""
    told("broadcast_inner_off_by_4", npref.binary("add", a, b), fast_emulation("add", a, b, 4), accept_bits(fast_emulation("add", a, b, 4), npref.binary("add", a, b)))
    for family in ("boundary_early.", "boundary_late.", "ln_sequential_sums.", "rms_sequential_sums.", "softmax_sequential_sums.", "ln_padding_counted.",
                   "softmax_max_misses_last.", "reduce_last_wins.", "reduce_nan_wins.", "reduce_column_major", "broadcast_inner_off_by_4",
                   "ln_last_row_unwritten."):
        assert any(k.startswith(family) for k in seen), family


# ================================================================================================================ GPU tests
def expect_route(K, ctx, want):
    got = K.last_route(ctx)
    assert got == want, "route moved: the library ran %r, the row covers %r" % (got, want)
    assert set(filter(None, got.split("/"))) <= set(K.route_names())


def stale(K, ctx):
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)   # another route first: a stale name would show


def at_offset(ctx, arr, off_bytes):
    """arr on the device, its first element `off_bytes` past the (256-byte aligned) start of a buffer -> (LeleTensor, keep-alive)"""
    from lele_amd import _lib
    arr = np.ascontiguousarray(arr)
    assert off_bytes % arr.dtype.itemsize == 0
    lead = np.full(off_bytes // arr.dtype.itemsize, -7.25 if arr.dtype.kind == "f" else -7, arr.dtype)
    buf = ctx.buf()
    buf.upload(np.concatenate([lead, arr.reshape(-1)]))
    assert buf.ptr % 256 == 0
    shape = (C.c_int64 * max(1, arr.ndim))(*arr.shape)
    return _lib.LeleTensor(C.c_void_p(buf.ptr + off_bytes), shape, arr.ndim, _lib._NP2DT[arr.dtype], _lib.MEM_DEVICE), (buf, shape)


def abi_call(ctx, fn, prefix, arrays, offs, dtype=np.float32):
    """fn(ctx, *prefix, *tensors, out, out_shape, out_rank) on device tensors at the given byte offsets: as_tensor refuses views, so
    the structs are built here"""
    from lele_amd import _lib
    keep, args = [], [ctx._h] + list(prefix)
    for a, off in zip(arrays, offs):
        t, k = at_offset(ctx, a, off)
        keep.append((t, k))
        args.append(C.byref(t))
    out, sh = ctx.buf(), _lib.OutShape()
    _lib.check(fn(*args, out._h, sh.shape, C.byref(sh.rank)))
    return out.to_numpy(sh.get(), dtype)


def run_unary(K, ctx, name, x, off=0):
    from lele_amd import _lib
    if off:
        return abi_call(ctx, _lib.lib().lele_hip_unary, [C.c_int(K._UNARY[KNAME.get(name, name)])], [x], [off])
    return getattr(K, KNAME.get(name, name))(x, ctx=ctx).numpy()


def unary_input(name, n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 4).astype(np.float32)
    return np.abs(x) + np.float32(0.1) if name == "log" else x


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(UNARY_ROWS)), ids=["%d-%s-%d" % (i, r[0], r[1]) for i, r in enumerate(UNARY_ROWS)])
def test_unary_rows(ctx, orc, i):
    from lele_amd import kernels as K
    route, n, off, why = UNARY_ROWS[i]
    failures = []
    for name in (POLY + ONE + LIBM) if n < 10 ** 6 else ("exp", "gelu", "sqrt", "log"):
        x = unary_input(name, n, 3 + n)
        stale(K, ctx)
        got = run_unary(K, ctx, name, x, off)
        expect_route(K, ctx, route)
        bad = check_unary(name, x, got, orc)
        if bad:
            failures.append("%s: %s" % (name, bad))
    assert not failures, why + "\n" + "\n".join(failures)
    if i == 0:
        assert K.exp(np.zeros((0, 3), np.float32), ctx=ctx).shape == (0, 3)
        expect_route(K, ctx, "")


@pytest.mark.gpu
@pytest.mark.parametrize("name", POLY + ONE + LIBM)
def test_unary_values(ctx, orc, name):
    """the special values in every lane position of an 8-chunk and in the tail, and every binade of both signs"""
    from lele_amd import kernels as K
    failures = []
    for label, x in [("specials in every lane", specials_in_every_lane()), ("binade sweep", binade_sweep())] + [("specials in the tail %d" % k, t) for k, t in enumerate(specials_tails())]:
        got = run_unary(K, ctx, name, x)
        expect_route(K, ctx, "unary.vec4")
        bad = check_unary(name, x, got, orc)
        if bad:
            failures.append("%s: %s" % (label, bad))
    assert not failures, "\n".join(failures)


def run_binary(K, ctx, name, a, b, offs=(0, 0)):
    from lele_amd import _lib
    if any(offs):
        return abi_call(ctx, _lib.lib().lele_hip_binary, [C.c_int(K._BINARY[name])], [a, b], offs, a.dtype)
    return getattr(K, name)(a, b, ctx=ctx).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(BINARY_ROWS)), ids=["%d-%s" % (i, r[0]) for i, r in enumerate(BINARY_ROWS)])
def test_binary_rows(ctx, i):
    from lele_amd import kernels as K
    route, sa, sb, dt, offs, why = BINARY_ROWS[i]
    rng = np.random.default_rng(20 + i)
    if dt == F32:
        a, b = (rng.standard_normal(s, dtype=np.float32) * np.float32(3) for s in (sa, sb))
        b = np.where(np.abs(b) < 0.3, np.float32(0), b).astype(np.float32)   # zeros for equal / mod / and / or
        ops = BIN_OPS if prod(bcast([sa, sb])[0]) < 10 ** 6 else ("add", "max")   # by the size of the result
    else:
        a, b = (rng.integers(-50, 50, s).astype(np.int64) for s in (sa, sb))
        ops = ("add", "sub", "mul", "div", "max", "min", "equal", "less", "greater", "mod_f32")
    failures = []
    for name in ops:
        stale(K, ctx)
        got = run_binary(K, ctx, name, a, b, offs)
        expect_route(K, ctx, route)
        bad = accept_bits(got, npref.binary("mod" if (name == "mod_f32" and dt == I64) else name, a, b))
        if bad:
            failures.append("%s: %s" % (name, bad))
    assert not failures, why + "\n" + "\n".join(failures)
    if i == 0:
        assert K.add(np.zeros((0, 3), np.float32), np.zeros((3,), np.float32), ctx=ctx).shape == (0, 3)
        expect_route(K, ctx, "")


def pow_class_and_tolerance(got, a, b):
    want = npref.binary("pow", a, b)
    fin = np.isfinite(want) & (want != 0)
    if not np.array_equal(klass(got), klass(want)):
        at = int(np.argwhere(klass(got) != klass(want))[0][0])
        return "pow class: %r ** %r: got %r want %r" % (a[at], b[at], got[at], want[at])
    ok = np.abs(got[fin].astype(np.float64) - want[fin]) <= 1e-4 * np.abs(want[fin].astype(np.float64))
    return "" if ok.all() else "pow tolerance: %d of %d" % (int((~ok).sum()), ok.size)


@pytest.mark.gpu
def test_binary_values(ctx):
    """the cross product of the special values through the fast path (equal shapes) and the index walk (a column against a row)"""
    from lele_amd import kernels as K
    a, b = cross(BIN_SPECIALS)
    failures = []
    for name in BIN_OPS:
        got = getattr(K, name)(a, b, ctx=ctx).numpy()
        expect_route(K, ctx, "bin.fast")
        bad = accept_bits(got, npref.binary(name, a, b))
        if bad:
            failures.append("%s, fast: %s" % (name, bad))
        got = getattr(K, name)(BIN_SPECIALS[:, None].copy(), BIN_SPECIALS[None, :].copy(), ctx=ctx).numpy()
        expect_route(K, ctx, "bin.index_f32")   # inner = 1, len 13 % 4 != 0
        bad = accept_bits(got.reshape(-1), npref.binary(name, a, b))
        if bad:
            failures.append("%s, index walk: %s" % (name, bad))
    bad = pow_class_and_tolerance(K.pow(a, b, ctx=ctx).numpy(), a, b)
    if bad:
        failures.append(bad)
    ai, bi = cross(I64_SPECIALS)
    for name in ("div", "mod_f32", "max", "min", "equal", "less", "greater"):
        got = getattr(K, name)(ai, bi, ctx=ctx).numpy()
        expect_route(K, ctx, "bin.flat_i64")
        assert got.dtype == np.int64
        bad = accept_bits(got, npref.binary("mod" if name == "mod_f32" else name, ai, bi))
        if bad:
            failures.append("i64 %s: %s" % (name, bad))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_binary_pitched_rows(ctx):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    for route, parent, wa, wb, oc0, why in BINP_ROWS:
        rng = np.random.default_rng(sum(parent))
        pa, pb = (rng.standard_normal(parent).astype(np.float32) for _ in range(2))
        c, plane = wa[1] - wa[0], prod(parent[2:])
        va, vb = TensorView(ctx.buf().upload(pa)).channels(*wa), TensorView(ctx.buf().upload(pb)).channels(*wb)
        for name in ("add", "mul", "max"):
            want = npref.binary(name, pa[:, wa[0]:wa[1]], pb[:, wb[0]:wb[1]])
            sent = np.full((parent[0], c + 3) + parent[2:], -7.25, np.float32)
            ob = ctx.buf()
            ob.upload(sent)
            stale(K, ctx)
            got = getattr(K, name)(va, vb, out=ob, out_window=(oc0 * plane, (c + 3) * plane), ctx=ctx)
            expect_route(K, ctx, route)
            sent[:, oc0:oc0 + c] = want
            assert accept_bits(ob.to_numpy(sent.shape), sent) == "" and accept_bits(got.numpy(), want) == "", (why, name)


@pytest.mark.gpu
def test_where_clip_batch_norm_rows(ctx, orc):
    from lele_amd import kernels as K
    rng = np.random.default_rng(12)
    for sc, sx, sy in (((2, 1, 4), (2, 3, 4), (4,)), ((2 ** 20 + 7, 1), (1, 3), (2 ** 20 + 7, 3))):
        cond = (rng.uniform(size=sc) > 0.5).astype(np.float32)
        x, y = rng.standard_normal(sx, dtype=np.float32), rng.standard_normal(sy, dtype=np.float32)
        stale(K, ctx)
        got = K.where_op(cond, x, y, ctx=ctx).numpy()
        expect_route(K, ctx, "where.index")
        assert accept_bits(got, npref.where_op(cond, x, y)) == "", sc
    cond = np.float32([0.0, -0.0, np.nan, 1.4e-45, -1.1754942e-38, 1.0, np.inf, -np.inf])   # -0 is false; a NaN and a subnormal are true
    x, y = np.arange(8, dtype=np.float32) + 1, -np.arange(8, dtype=np.float32) - 1
    assert accept_bits(K.where_op(cond, x, y, ctx=ctx).numpy(), np.where([False, False] + [True] * 6, x, y).astype(np.float32)) == ""
    for n in (37, 2 ** 20 + 9):
        x = rng.standard_normal(n, dtype=np.float32) * np.float32(2)
        x[:8] = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, -0.5, 7])
        for lo, hi in ((-0.5, 0.5), (None, 0.25), (0.0, None), (None, None)):
            stale(K, ctx)
            got = K.clip(x, None if lo is None else [lo], None if hi is None else [hi], ctx=ctx).numpy()
            expect_route(K, ctx, "clip.w1")
            assert accept_bits(got, npref.clip(x, lo, hi)) == "", (n, lo, hi)
    for shape in BN_SHAPES:
        x = rng.standard_normal(shape, dtype=np.float32)
        s, bb, m, v = bn_params(shape[1] if len(shape) > 1 else shape[0])
        stale(K, ctx)
        got = K.batch_norm(x, s, bb, m, v, 1e-5, ctx=ctx).numpy()
        expect_route(K, ctx, "bn.w1")
        assert accept_bits(got, orc.batch_norm(x, s, bb, m, v)) == "", shape


REDUCE_FN = {"sum": "reduce_sum", "mean": "reduce_mean", "max": "reduce_max", "l2": "reduce_l2"}


def run_reduce(K, ctx, op, x, axes, keepdims=False):
    if op == "min":
        return K._reduce(4, x, axes, keepdims, None, ctx).numpy()
    return getattr(K, REDUCE_FN[op])(x, axes, keepdims, ctx=ctx).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(REDUCE_ROWS)), ids=["%d-%s-%s" % (i, r["route"], r["op"]) for i, r in enumerate(REDUCE_ROWS)])
def test_reduce_rows(ctx, i):
    from lele_amd import kernels as K
    row = REDUCE_ROWS[i]
    cus = K.num_cus(ctx)
    assert cus > 0
    shape = row_shape(row, cus)
    assert reduce_route(row["op"], shape, row["axes"], cus) == row["route"]   # the table at this device's CU count
    x = reduce_input(shape, 40 + i)
    stale(K, ctx)
    got = run_reduce(K, ctx, row["op"], x, row["axes"])
    expect_route(K, ctx, row["route"])
    assert accept_bits(got, reduce_want(row["op"], x, row["axes"])) == "", row["why"]
    if prod(shape) < 10 ** 5:
        got = run_reduce(K, ctx, row["op"], x, row["axes"], True)
        expect_route(K, ctx, row["route"])
        assert accept_bits(got, npref.reduce(row["op"], x, row["axes"], True)) == "", row["why"]


@pytest.mark.gpu
def test_min_max_is_the_min_and_max_routes(ctx):
    from lele_amd import kernels as K
    x = reduce_input((2, 70001), 77, specials=False)
    assert K.min_max(x, ctx=ctx) == (float(x.min()), float(x.max()))
    expect_route(K, ctx, "reduce.seq")   # several axes reduced: the sequential kernel
    assert K.min_max(x.reshape(-1), ctx=ctx) == (float(x.min()), float(x.max()))
    expect_route(K, ctx, "reduce.parts")
    assert K.reduce_max(np.zeros((0, 4), np.float32), [1], False, ctx=ctx).shape == (0,)
    expect_route(K, ctx, "")


def norm_case(kind, n, outer, orc):
    rng = np.random.default_rng(n * 7 + outer)
    x = (rng.standard_normal((outer, n)) * 2 + 0.3).astype(np.float32)
    g, b = norm_params(n)
    if kind == "ln":
        return x, (g, b), orc.layer_norm(x, g, b, -1, 1e-5)
    if kind == "rms":
        return x, (g,), orc.rms_norm(x, g, -1, 1e-6)
    return x, (), orc.softmax(x)


def run_norm(K, ctx, kind, x, params):
    if kind == "ln":
        return K.layer_norm(x, params[0], params[1], -1, 1e-5, ctx=ctx)
    if kind == "rms":
        return K.rms_norm(x, params[0], -1, 1e-6, ctx=ctx)
    return K.softmax(x, -1, ctx=ctx)


def check_norm_shape(K, ctx, orc, n, outer):
    failures = []
    for kind in ("ln", "rms", "softmax"):
        x, params, want = norm_case(kind, n, outer, orc)
        stale(K, ctx)
        got = run_norm(K, ctx, kind, x, params).numpy()
        expect_route(K, ctx, norm_route(kind, n, outer))
        bad = accept_softmax(got, want, n) if kind == "softmax" else accept_bits(got, want)
        if bad:
            failures.append("%s [%d, %d]: %s" % (kind, outer, n, bad))
    return failures


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_norm_lengths(ctx, orc, n):
    """three rows (a last block of one live row) at every length: each register class on both sides, 0..3 remainder chunks, 0..7 tail
    elements, the streaming kernels past 1024"""
    from lele_amd import kernels as K
    failures = check_norm_shape(K, ctx, orc, n, 3)
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("outer", OUTERS)
def test_norm_outers(ctx, orc, outer):
    """every rows-per-block class on both sides of its threshold, a last block with 1, 3 or 7 live rows, on partly filled register rows"""
    from lele_amd import kernels as K
    failures = [f for n in OUTER_LENGTHS for f in check_norm_shape(K, ctx, orc, n, outer)]
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_norm_variants(ctx, orc):
    from lele_amd import kernels as K
    rng = np.random.default_rng(14)
    for n in (40, 300, 520, 1031):   # one row length of each class: softmax_scaled == mul then softmax, bit for bit
        x = (rng.standard_normal((3, n)) * 3).astype(np.float32)
        sc = np.float32([0.17677669])
        stale(K, ctx)
        got = K.softmax_scaled(x, sc, -1, ctx=ctx).numpy()
        expect_route(K, ctx, norm_route("softmax", n, 3))
        assert accept_bits(got, K.softmax(K.mul(x, sc, ctx=ctx), -1, ctx=ctx).numpy()) == "", n
        assert accept_softmax(got, orc.softmax(npref.binary("mul", x, sc)), n) == "", n
    x = rng.standard_normal((2, 3, 4, 5)).astype(np.float32)   # a multi-dim normalised shape: the trailing [4, 5]
    g, b = rng.standard_normal((4, 5)).astype(np.float32), rng.standard_normal((4, 5)).astype(np.float32)
    assert accept_bits(K.layer_norm(x, g, b, 2, 1e-5, ctx=ctx).numpy(), orc.layer_norm(x, g, b, 2, 1e-5)) == ""
    expect_route(K, ctx, "ln.reg8/rows.rpb2")
    g1, b1 = np.float32([1.5]), np.float32([-0.25])   # axis == rank: every element is a row of one
    assert accept_bits(K.layer_norm(x, g1, b1, 4, 1e-5, ctx=ctx).numpy(), orc.layer_norm(x, g1, b1, 4, 1e-5)) == ""
    expect_route(K, ctx, "ln.reg8/rows.rpb2")
    assert K.layer_norm(np.zeros((0, 8), np.float32), np.ones(8, np.float32), np.zeros(8, np.float32), -1, 1e-5, ctx=ctx).shape == (0, 8)
    expect_route(K, ctx, "")


@pytest.mark.gpu
@pytest.mark.parametrize("n", VALUE_LENGTHS)
def test_norm_values(ctx, orc, n):
    """constant, overflowing, subnormal, outlier, +-inf and NaN rows through layer_norm and rms_norm; masked, all-masked, +inf, equal,
    spread and subnormal rows through softmax: the oracle's bits (any NaN where it yields one)"""
    from lele_amd import kernels as K
    x = norm_family_rows(n)
    g, b = norm_params(n)
    failures = []
    y = K.layer_norm(x, g, b, -1, 1e-5, ctx=ctx)
    expect_route(K, ctx, norm_route("ln", n, x.shape[0]))
    # the {min, max} pair per row the kernel leaves next to its result: fused_quantized_linear reads them instead of running its own
    # range pass (find_partials, quant.hip), so on the rows that come out as NaN (the +-inf, NaN and overflowing families) it must give
    # the bits of the same call on a copy, which carries no statistics.  A pair that let a NaN in, or was left unwritten, moves the range
    from lele_amd._lib import Weight
    wr = np.random.default_rng(70 + n)
    w = Weight(np.clip(np.round(128 + 32 * wr.standard_normal((n, 24))), 0, 255).astype(np.float32))
    ws, wz, wb = Weight((wr.random(24) * 0.01 + 0.002).astype(np.float32)), Weight(np.array([128.0], np.float32)), Weight(wr.standard_normal(24).astype(np.float32))
    assert np.isnan(y.numpy()).all(axis=1).sum() >= 3 and np.isfinite(y.numpy()).all(axis=1).sum() >= 4
    fused = K.fused_quantized_linear(y, w, ws, wz, wb, False, ctx=ctx).numpy()
    bad = accept_bits(fused, K.fused_quantized_linear(ctx.buf().upload(y.numpy()), w, ws, wz, wb, False, ctx=ctx).numpy())
    if bad:
        failures.append("fused_quantized_linear(layer_norm) against the same call on a copy without row statistics: %s" % bad)
    # dynamic_quantize_linear runs its own range pass whatever the buffer carries: the same bits on the result and on a copy of it
    q = [t.numpy() for t in K.dynamic_quantize_linear(y, ctx=ctx)]
    plain = [t.numpy() for t in K.dynamic_quantize_linear(ctx.buf().upload(y.numpy()), ctx=ctx)]
    for name, a, c in zip(("y", "scale", "zero point"), q, plain):
        bad = accept_bits(a, c)
        if bad:
            failures.append("dynamic_quantize_linear(layer_norm) against the same call on a copy, %s: %s" % (name, bad))
    for fam, got, want in zip(NORM_FAMILIES, y.numpy(), orc.layer_norm(x, g, b, -1, 1e-5)):
        bad = accept_bits(got, want)
        if bad:
            failures.append("layer_norm, %s: %s" % (fam, bad))
    got_all = K.rms_norm(x, g, -1, 1e-6, ctx=ctx).numpy()
    expect_route(K, ctx, "rms.stream")
    for fam, got, want in zip(NORM_FAMILIES, got_all, orc.rms_norm(x, g, -1, 1e-6)):
        bad = accept_bits(got, want)
        if bad:
            failures.append("rms_norm, %s: %s" % (fam, bad))
    xs = softmax_family_rows(n)
    got_all = K.softmax(xs, -1, ctx=ctx).numpy()
    expect_route(K, ctx, norm_route("softmax", n, xs.shape[0]))
    for fam, got, want in zip(SOFTMAX_FAMILIES, got_all, orc.softmax(xs)):
        bad = accept_bits(got, want)
        if bad:
            failures.append("softmax, %s: %s" % (fam, bad))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_add3_rows(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    for i, (route, shapes, off, why) in enumerate(ADD3_ROWS):
        rng = np.random.default_rng(60 + i)
        a, b, c = (rng.standard_normal(s, dtype=np.float32) * np.float32(3) for s in shapes)
        stale(K, ctx)
        if off:
            got = abi_call(ctx, _lib.lib().lele_hip_add3, [], [a, b, c], [off, 0, 0])
        else:
            got = K.add3(a, b, c, ctx=ctx).numpy()
        expect_route(K, ctx, route)
        assert accept_bits(got, npref.binary("add", npref.binary("add", a, b), c)) == "", why


@pytest.mark.gpu
def test_halves_pow_add_sqrt_rows(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(15)
    for shape, axis, lo, hi, why in HPAS_ROWS:
        x = rng.standard_normal(shape, dtype=np.float32) * np.float32(2)
        two = np.float32([2.0])
        stale(K, ctx)
        got = K.halves_pow_add_sqrt(x, axis, lo, hi, two, two, ctx=ctx)
        expect_route(K, ctx, "hpas.w1")
        parts = [K.pow(K.slice(x, [w[0]], [w[1]], [axis], ctx=ctx), two, ctx=ctx) for w in (lo, hi)]   # the six-node chain it stands for
        want = K.sqrt(K.add(parts[0], parts[1], ctx=ctx), ctx=ctx).numpy()
        assert accept_bits(got.numpy(), want) == "", why
        ax = axis % len(shape)
        sl = [npref.slice_(x, [w[0]], [w[1]], [ax]) for w in (lo, hi)]
        ref = np.sqrt(sl[0].astype(np.float64) ** 2 + sl[1].astype(np.float64) ** 2)
        assert got.shape == ref.shape and np.all(np.abs(got.numpy() - ref) <= 1e-4 * np.abs(ref) + 1e-7), why
