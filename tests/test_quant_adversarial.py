"""Every i8 quantisation route against the oracle on values built to separate a right rounding from a wrong one.

The random activations of tests/test_quant.py almost never put x * inv_scale + zp on a half-integer, a zero point on a tie, or a
slice's only extreme at a tile boundary.  The constructors here do, on purpose:

  * a range of [-8, 7.9375] gives scale = 2^-4 and zp = 128 exactly, so (j + 0.5 - 128) / 16 are exact ties: round-half-even
    (SIMD body) and round-half-away (scalar tail) give different codes for every even j;
  * a range of [-6.28125, 9.65625] gives -min / scale = 100.5: a tie in the zero point itself (f32::round -> 101, rint -> 100);
  * for an arbitrary range, values within an ulp of a tie where fma(x, inv, zp) and x * inv + zp round to different integers;
  * degenerate slices: constant, all zero, all positive (zp = 0), all negative (zp = 255), a range below 1e-5, -0.0 mixed in, one
    spike 1000x the rest as the only extreme.

The CPU test checks that each case bites: the oracle's result must differ from at least one named wrong implementation emulated
here in numpy (half-away in the body, half-even in the tail, mul + add instead of fma, rint for the zero point, inv_scale one ulp
off, the range of the slice without one element, ...).  The GPU tests run the cases through every route the dispatch code selects
and demand the oracle's bits."""
import ctypes as C
import os

import numpy as np
import pytest

F = np.float32

# ------------------------------------------------------------------------------------------------ f32 arithmetic in numpy


def fma32(x, a, b):
    """fmaf(x, a, b) element-wise: the exact x * a + b rounded ONCE to f32.  x * a is exact in f64; the sum is made exact by
    TwoSum and rounded to odd in f64 (53 >= 24 + 2 bits), after which the f64 -> f32 conversion rounds as a single rounding would"""
    p = np.asarray(x, np.float64) * np.float64(a)
    b = np.float64(b)
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)
    bits = s.view(np.int64) if isinstance(s, np.ndarray) else np.array(s).view(np.int64)
    odd = (bits & 1) == 1
    s = np.where((e != 0) & ~odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return np.asarray(s).astype(np.float32)


def round_away(v):
    v = np.asarray(v, np.float64)  # f32 values + 0.5 are exact in f64
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.float32)


def round_even(v):
    return np.rint(np.asarray(v, np.float32))


# ------------------------------------------------------------------------------------------------ the quantiser and its wrong variants

VARIANTS = ("body_half_away", "tail_half_even", "body_mul_add", "zp_rint", "inv_scale_ulp", "range_minus_min_element",
            "range_minus_max_element", "range_without_zero", "no_range_floor")


def qparams(x, variant=None):
    """make_qparams (quant.hip) / dyn_params (oracle/quant.cpp) over the whole slice x, in f32; `variant` names a wrong one"""
    x = np.asarray(x, np.float32).ravel()
    if variant in ("range_minus_min_element", "range_minus_max_element") and x.size > 1:
        x = np.delete(x, int(np.argmin(x) if variant == "range_minus_min_element" else np.argmax(x)))
    mn, mx = F(x.min()), F(x.max())
    if variant == "range_without_zero":
        amax, amin = mx, mn
    else:
        amax, amin = (mx if mx > 0 else F(0)), (mn if mn < 0 else F(0))
    rng = F(amax - amin)
    if variant != "no_range_floor" and not rng > F(1e-5):
        rng = F(1e-5)
    scale = F(rng / F(255))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = F(-amin) / scale
        z = round_even(z) if variant == "zp_rint" else round_away(z)
        zp = F(np.clip(z, 0, 255)) if np.isfinite(z) else F(0)
        inv = F(F(1) / scale)
    if variant == "inv_scale_ulp":
        inv = np.nextafter(inv, F(np.inf))
    return scale, zp, inv


def quantize(x, scale_zp_inv, body, variant=None):
    """codes of x: `body` marks the SIMD body (rint(fma)), the rest is the scalar tail (roundf(x * inv + zp))"""
    _, zp, inv = scale_zp_inv
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = fma32(x, inv, zp)
        ma = (x * inv).astype(np.float32) + zp
        qb = round_even(ma) if variant == "body_mul_add" else (round_away(f) if variant == "body_half_away" else round_even(f))
        qt = round_even(ma) if variant == "tail_half_even" else round_away(ma)
        q = np.where(body, qb, qt)
        return np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.float32)


def model_dql(x, variant=None):
    """dynamic_quantize_linear: one range over the tensor, SIMD body = the first len & ~7 elements"""
    flat = np.asarray(x, np.float32).ravel()
    q = qparams(flat, variant)
    body = np.arange(flat.size) < (flat.size // 8) * 8
    return quantize(flat, q, body, variant).reshape(np.shape(x)), q[0], q[1]


def model_fql_identity(x, variant=None):
    """fused_quantized_linear(x, W = 128 + I, weight_scale 1, weight_zero 128, no bias) of one slice [m, k]: row i, column j is
    float(code(x[i, j]) - zp) * scale -- the codes, the scale and the zero point all show in the result.  SIMD body = the first
    k & ~7 elements of each row"""
    m, k = x.shape
    q = qparams(x, variant)
    body = np.broadcast_to(np.arange(k) < (k // 8) * 8, (m, k))
    codes = quantize(x, q, body, variant)
    return ((codes.astype(np.int32) - int(q[1])).astype(np.float32) * q[0]).astype(np.float32)   # (float)i32 total * scale


def oracle_fql_identity(orc, x):
    k = x.shape[-1]
    w = (np.eye(k, dtype=np.float32) + F(128))
    return orc.fused_quantized_linear(x[None], w, np.array([1.0], np.float32), [128.0], None, False)[0]


# ------------------------------------------------------------------------------------------------ case constructors

GRID = (F(-8.0), F(7.9375))           # scale 2^-4, zp 128: (j + 0.5 - 128) / 16 are exact ties
ZP_TIE = (F(-6.28125), F(9.65625))    # scale 2^-4, -min / scale = 100.5: the zero point is a tie (101 half away, 100 half even)
KINDS = ("grid", "zp_tie", "near", "pos", "neg", "negzero", "spike", "const_pos", "const_neg", "zero", "tiny")
# an all-zero slice gives (0 - zp) * scale = 0 through a linear whatever the scale: it bites dynamic_quantize_linear (whose scale is an
# output) but no variant of the fused linear, so the fused routes run it only as a check that nothing turns it into NaN
FUSED_KINDS = tuple(k for k in KINDS if k != "zero")


def near_ties(lo, hi, n, rng):
    """n values in (lo, hi) within an ulp or two of a tie of the slice [lo, hi]'s quantiser, preferring those where
    rint(fma(x, inv, zp)) != rint(x * inv + zp)"""
    _, zp, inv = qparams(np.array([lo, hi], np.float32))
    t = rng.integers(1, 254, 4 * n).astype(np.float64) + 0.5
    x0 = ((t - np.float64(zp)) / np.float64(inv)).astype(np.float32)
    cands = [x0]
    up, dn = x0, x0
    for _ in range(3):
        up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))
        cands += [up, dn]
    c = np.stack(cands, 1)                                             # [4n, 7]
    split = round_even(fma32(c, inv, zp)) != round_even((c * inv).astype(np.float32) + zp)
    pick = np.where(split.any(1), split.argmax(1), 0)
    v = c[np.arange(c.shape[0]), pick]
    good = split.any(1) & (v > lo) & (v < hi)
    v = np.concatenate([v[good], v[~good & (v > lo) & (v < hi)]])
    return v[:n] if v.size >= n else np.resize(v, n)


def make_slice(kind, shape, rng, at_min=None, at_max=None):
    """an f32 slice of `shape` of the given kind; its minimum and maximum (each one element where the kind has a single extreme)
    sit at the flat positions at_min / at_max"""
    size = int(np.prod(shape))
    at_min = 0 if at_min is None else at_min
    at_max = size - 1 if at_max is None else at_max
    lo = hi = None
    if kind == "grid" or kind == "negzero":
        lo, hi = GRID
        x = ((rng.integers(0, 255, size) + 0.5 - 128) / 16).astype(np.float32)
        if kind == "negzero":
            x[rng.random(size) < 0.25] = F(-0.0)
            x[rng.random(size) < 0.05] = F(0.0)
    elif kind == "zp_tie":
        lo, hi = ZP_TIE
        x = ((rng.integers(1, 255, size) + 0.5 - 101) / 16).astype(np.float32)
    elif kind == "near":
        lo, hi = F(-rng.uniform(0.3, 3.0)), F(rng.uniform(0.3, 3.0))
        x = near_ties(lo, hi, size, rng)
        rng.shuffle(x)
    elif kind == "pos":       # zp = 0; [0.25, 15.9375] -> scale 2^-4; ties (j + 0.5) / 16
        lo, hi = F(0.25), F(15.9375)
        x = ((rng.integers(4, 255, size) + 0.5) / 16).astype(np.float32)
    elif kind == "neg":       # zp = 255; [-15.9375, -0.25] -> scale 2^-4; ties (j + 0.5 - 255) / 16
        lo, hi = F(-15.9375), F(-0.25)
        x = ((rng.integers(0, 251, size) + 0.5 - 255) / 16).astype(np.float32)
    elif kind == "spike":     # the only extreme is one element 1000x the rest
        x = rng.standard_normal(size).astype(np.float32)
        hi = F(1000 * np.abs(x).max())
        lo = None
    elif kind == "const_pos":
        x = np.full(size, 0.7, np.float32)
    elif kind == "const_neg":
        x = np.full(size, -0.3, np.float32)
    elif kind == "zero":
        x = np.zeros(size, np.float32)
    elif kind == "tiny":      # range below the 1e-5 floor
        x = rng.uniform(-3e-6, 4e-6, size).astype(np.float32)
        lo, hi = F(-3.5e-6), F(4.5e-6)
    else:
        raise ValueError(kind)
    if lo is not None:
        x[at_min] = lo
    if hi is not None:
        x[at_max] = hi
    return x.reshape(shape)


def boundary_rows(b, m, tile=32):
    """global rows where routes change hands: first / last row of every slice, both sides of every `tile`-row boundary that falls
    inside the tensor, the last row (the ragged last tile)"""
    rows = b * m
    r = {0, rows - 1}
    for s in range(b):
        r |= {s * m, s * m + m - 1}
    for t in range(tile, rows, tile):
        r |= {t - 1, t}
    return sorted(x for x in r if 0 <= x < rows)


def adversarial_batch(b, m, k, seed, kinds=KINDS, tile=32):
    """[b, m, k]: slice s is of kind kinds[s % len(kinds)]; its single minimum and maximum sit in boundary rows of that slice
    (cycling through them), in column 0, the last column (the scalar tail when k % 8 != 0) or a middle one"""
    rng = np.random.default_rng(seed)
    rows = boundary_rows(b, m, tile)
    cols = [0, k - 1, k // 2, (k // 8) * 8 - 1 if k >= 8 else 0]
    x = np.empty((b, m, k), np.float32)
    for s in range(b):
        mine = [r - s * m for r in rows if s * m <= r < (s + 1) * m] or [0]
        rmin, rmax = mine[(2 * s) % len(mine)], mine[(2 * s + 1) % len(mine)]
        cmin, cmax = cols[s % len(cols)], cols[(s + 1) % len(cols)]
        pmin, pmax = rmin * k + cmin, rmax * k + cmax
        if pmin == pmax:
            pmax = (pmax + 1) % (m * k)
        x[s] = make_slice(kinds[s % len(kinds)], (m, k), rng, pmin, pmax)
    return x


# ------------------------------------------------------------------------------------------------ 1. the cases bite (CPU)


def _same(a, b):
    """equal shapes and values (NaN equals nothing: a NaN anywhere fails)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, b)


def _bites(ref, variants):
    """names of the wrong variants whose (codes, scale, zp) differ from `ref` (NaN differs from everything)"""
    return [name for name, v in variants if not all(np.array_equal(np.float32(a), np.float32(b)) for a, b in zip(v, ref))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", [64, 65, 71, 1000, 1007])  # = 0, 1 and 7 (mod 8): the scalar tail of dynamic_quantize_linear
def test_dynamic_quantize_cases_bite(orc, kind, length):
    """every constructed slice: the numpy model equals the oracle bit for bit, and at least one wrong variant does not"""
    rng = np.random.default_rng(length * 31 + KINDS.index(kind))
    for at_min, at_max in ((0, length - 1), (length - 1, 0), (length // 2, (length // 8) * 8 % length)):
        x = make_slice(kind, (length,), rng, at_min, at_max)
        if kind == "negzero":
            assert (np.signbit(x) & (x == 0)).any()
        y, s, z = orc.dynamic_quantize_linear(x)
        ref = (y, s[0], z[0])
        got = model_dql(x)
        assert not _bites(ref, [("model", got)]), (kind, length)
        bit = _bites(ref, [(v, model_dql(x, v)) for v in VARIANTS])
        assert bit, "case %s / %d separates the oracle from no wrong variant" % (kind, length)
        if kind in ("grid", "zp_tie", "pos", "neg", "negzero") and length % 8:
            # ties in the scalar tail are caught by the tail variant on their own
            _, zp, inv = qparams(x)
            ma = (x[(length // 8) * 8:] * inv).astype(np.float32) + zp
            if (round_away(ma) != round_even(ma)).any():
                assert "tail_half_even" in bit, (kind, length)


@pytest.mark.parametrize("kind", FUSED_KINDS)
@pytest.mark.parametrize("m,k", [(5, 37), (3, 64), (4, 100)])
def test_fused_linear_cases_bite(orc, kind, m, k):
    """the same for the fused linear's per-row SIMD body / scalar tail (weights 128 + I expose every code, the scale and the zero
    point in the result); each named variant is exercised by at least one kind (checked in the test below)"""
    rng = np.random.default_rng(m * k + KINDS.index(kind))
    x = make_slice(kind, (m, k), rng, k - 1, (m - 1) * k)
    ref = oracle_fql_identity(orc, x)
    assert _same(model_fql_identity(x), ref), (kind, m, k)
    bit = [v for v in VARIANTS if not _same(model_fql_identity(x, v), ref)]
    assert bit, "case %s (%d, %d) separates the oracle from no wrong variant" % (kind, m, k)


def test_every_wrong_variant_is_caught_by_some_case(orc):
    caught = set()
    for kind in FUSED_KINDS:
        for m, k in ((5, 37), (4, 100)):
            rng = np.random.default_rng(m * k + KINDS.index(kind))
            x = make_slice(kind, (m, k), rng, k - 1, (m - 1) * k)
            ref = oracle_fql_identity(orc, x)
            caught |= {v for v in VARIANTS if not _same(model_fql_identity(x, v), ref)}
    assert caught == set(VARIANTS), set(VARIANTS) - caught


def test_adversarial_batches_put_the_extremes_where_asked():
    b, m, k = 5, 70, 37
    x = adversarial_batch(b, m, k, 0, kinds=("grid", "zp_tie", "pos", "neg", "near"))
    rows = boundary_rows(b, m)
    for s in range(b):
        xs = x[s]
        assert (xs == xs.min()).sum() == 1 and (xs == xs.max()).sum() == 1, s
        rmin, rmax = int(np.argmin(xs)) // k, int(np.argmax(xs)) // k
        assert s * m + rmin in rows and s * m + rmax in rows, s
    assert qparams(make_slice("grid", (64,), np.random.default_rng(0)))[1:] == (F(128), F(16))
    assert qparams(make_slice("zp_tie", (64,), np.random.default_rng(0)))[1] == F(101)
    assert qparams(make_slice("zp_tie", (64,), np.random.default_rng(0)), "zp_rint")[1] == F(100)
    nt = near_ties(F(-1.3), F(2.7), 200, np.random.default_rng(1))
    _, zp, inv = qparams(np.array([-1.3, 2.7], np.float32))
    assert (round_even(fma32(nt, inv, zp)) != round_even((nt * inv).astype(np.float32) + zp)).sum() >= 20


def test_fma_emulation_rounds_once():
    """fma32 against exact rational arithmetic on values built to sit next to f32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    x = rng.standard_normal(3000).astype(np.float32)
    a = F(16.000002)
    b = F(128.0)
    got = fma32(x, a, b)
    for xi, gi in zip(x[:300], got[:300]):
        exact = Fraction(float(xi)) * Fraction(float(a)) + Fraction(float(b))
        lo = np.float32(float(exact))
        cands = [lo, np.nextafter(lo, F(np.inf)), np.nextafter(lo, F(-np.inf))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(np.array(c).view(np.uint32)) & 1))
        assert gi == best, (xi, gi, best)


# ------------------------------------------------------------------------------------------------ 2. the route matrix (GPU)


def _qw(rng, k, n, wz=128.0):
    from lele_amd._lib import Weight
    return (Weight(np.clip(np.round(128 + 32 * rng.standard_normal((k, n))), 0, 255).astype(np.float32)),
            Weight((np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32)), Weight(np.array([wz], np.float32)),
            Weight((rng.standard_normal(n) * 0.02).astype(np.float32)))


class _env:
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


def _diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = ~(a == b)
    return "%d of %d differ, first at %s" % (int(bad.sum()), bad.size, np.argwhere(bad)[:1].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("length", [8 * 125, 8 * 125 + 1, 8 * 125 + 7, 93 * 560, 93 * 560 + 7])
def test_dynamic_quantize_linear_on_adversarial_slices(ctx, orc, length):
    """lele_hip_dynamic_quantize_linear: one range over the tensor, SIMD body + scalar tail of length % 8 -- codes, scale and zero
    point equal the oracle's on every kind of slice, its extremes at the first / last element and at the body / tail seam"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(length)
    for kind in KINDS:
        for at_min, at_max in ((0, length - 1), ((length // 8) * 8 % length, (length // 8) * 8 - 1), (length - 1, length // 2)):
            x = make_slice(kind, (length,), rng, at_min, at_max)
            y, s, z = K.dynamic_quantize_linear(ctx.buf().upload(x), ctx=ctx)
            ry, rs, rz = orc.dynamic_quantize_linear(x)
            assert _same(s.numpy(), rs) and _same(z.numpy(), rz), (kind, length, at_min, float(s.numpy()[0]), float(rs[0]))
            assert _same(y.numpy(), ry), (kind, length, at_min, _diff(y.numpy(), ry))


# (b, m, k, n) -> the route fql_route (quant.hip) selects for it, in words, then as lele_hip_last_route reports it on 256 CUs and, with
# LELE_HIP_IGEMM_RS=0, for the tiled chain alone.  On any CU count the test asserts what tests/test_quant_routes.py::dispatch derives.
ROUTES = [
    ((1, 93, 560, 1536), "tiled: K = 560 pads to 576 (rs_fits needs kp == 512) -> qrows_kernel + igemm_kernel",
     ("q.tiled/igemm.small_k16", "q.tiled/igemm.small_k16")),
    ((2, 5, 37, 19), "tiled chain on a tiny product (launch_igemm's small-problem kernel); K = 37: a scalar tail of 5 per row",
     ("q.tiled/igemm.small_k4", "q.tiled/igemm.small_k4")),
    ((32, 171, 512, 512), "activation-stationary igemm_as_kernel (as_fits: K = 512, N <= 512, >= 256 rows): rows quantised in the GEMM",
     ("q.as/as.two", "q.tiled/igemm.t128x64")),
    ((32, 171, 512, 1024), "register-stationary igemm_rs_kernel (rs_fits: kp 512, N >= 1024, >= 2 tiles per CU) with rs_fq: the loader "
                           "waves quantise the rows", ("q.rs_fq", "q.tiled/igemm.t128x64")),
    ((9, 1000, 500, 1536), "register-stationary with K = 500 padded to 512: launch_qrows_frag quantises first (scalar tail of 4)",
     ("q.rs_frag", "q.tiled/igemm.t128x128")),
    ((1, 504, 2048, 512), "K = 2048 stand-alone: tiled (rs_fits needs kp == 512; igemm_rs_ks4 runs only inside fused_ffn_quantized)",
     ("q.tiled/igemm.small_k16", "q.tiled/igemm.small_k16")),
    ((1, 2125, 1024, 3844), "compute-bound igemm_big_kernel (K a multiple of 128 >= 1024, half a chip of 256 x 256 results)",
     ("q.tiled/igemm.big", "q.tiled/igemm.big")),
    # (14 x 8 results of 256 x 256 are 112, short of half of 256 CUs: not the compute-bound kernel, as this line once said.  Its slices
    # straddling the 256-row results: tests/test_quant_routes.py, the row "tiled-big-slices-straddle")
    ((5, 700, 1152, 2048), "K a multiple of 128 >= 1024 on too few 256 x 256 results for igemm_big_kernel: 128 x 64 tiles, 128-byte K steps",
     ("q.tiled/igemm.t128x64", "q.tiled/igemm.t128x64")),
    ((1, 33, 100, 130), "tiled, generic K with a scalar tail of 4 per row", ("q.tiled/igemm.small_k4", "q.tiled/igemm.small_k4")),
]


def _route_is(ctx, b, m, k, n, named=None):
    """last_route() is what the restated dispatch derives for this device and environment -- and, on 256 CUs, the string written down"""
    from lele_amd import kernels as K
    # (imported here, not at the top: tests/test_quant_routes.py imports this module's constructors when it is loaded)
    from tests.test_quant_routes import ENV, dispatch
    env = {name: int(os.environ.get(name, dflt)) for name, dflt in ENV.items()}
    cus = K.num_cus(ctx)
    want = dispatch("fql", b, m, k, n, cus, env)[0]
    assert K.last_route(ctx) == want, (K.last_route(ctx), want, (b, m, k, n), cus)
    if named is not None and cus == 256:
        assert want == named, (want, named)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,route,named", ROUTES, ids=[str(r[0]) for r in ROUTES])
def test_fused_quantized_linear_routes_on_adversarial_slices(ctx, orc, shape, route, named):
    """fused_quantized_linear on each route: every slice kind, the single extremes in rows at slice, 32-row tile and ragged-last-tile
    boundaries, equal to the oracle bit for bit -- and the tiled chain alone (LELE_HIP_IGEMM_RS=0) as well"""
    from lele_amd import kernels as K
    b, m, k, n = shape
    rng = np.random.default_rng(b * m + k + n)
    w = _qw(rng, k, n, 121.0)
    big = b * m * k * n > 1e9
    kinds_sets = [KINDS] if b >= len(KINDS) else [KINDS[i:i + b] for i in range(0, len(KINDS), b)]
    if big:
        kinds_sets = kinds_sets[:2]
    for i, kinds in enumerate(kinds_sets):
        x = adversarial_batch(b, m, k, 100 * i + b, kinds=kinds)
        ref = orc.fused_quantized_linear(x, w[0].arr, w[1].arr, w[2].arr, w[3].arr, False)
        xd = ctx.buf().upload(x)
        got = K.fused_quantized_linear(xd, *w, False, ctx=ctx).numpy()
        _route_is(ctx, b, m, k, n, named[0])
        assert _same(got, ref), (route, kinds, _diff(got, ref))
        if not big:
            with _env(LELE_HIP_IGEMM_RS=0):
                got = K.fused_quantized_linear(xd, *w, False, ctx=ctx).numpy()
                _route_is(ctx, b, m, k, n, named[1])
                assert _same(got, ref), ("tiled", route, kinds, _diff(got, ref))


def _ln(rng, n=512):
    from lele_amd._lib import Weight
    return Weight((1 + 0.1 * rng.standard_normal(n)).astype(np.float32)), Weight((0.1 * rng.standard_normal(n)).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("b,m", [(32, 171), (3, 1000), (1, 504)])
def test_residual_ln_on_adversarial_slices(ctx, orc, b, m):
    """fused_quantized_linear_residual_ln: (32, 171) normalises in igemm_as_kernel's epilogue, (3, 1000) straddles row tiles with a
    ragged last one, (1, 504) issues the two calls -- the projection against the oracle bit for bit, the LayerNorm against the
    oracle's on the same sum"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(b + m)
    x = adversarial_batch(b, m, 512, b * m)
    w = _qw(rng, 512, 512)
    r1, r2 = rng.standard_normal((b, m, 512)).astype(np.float32), rng.standard_normal((b, m, 512)).astype(np.float32)
    g, be = _ln(rng)
    got = K.fused_quantized_linear_residual_ln(ctx.buf().upload(x), *w, False, r1, r2, g, be, 1e-5, ctx=ctx)
    o = (orc.fused_quantized_linear(x, w[0].arr, w[1].arr, w[2].arr, w[3].arr) + r1) + r2
    assert _same(got[0].numpy(), o), _diff(got[0].numpy(), o)
    assert _same(got[1].numpy(), orc.layer_norm(o, g.arr, be.arr, -1, 1e-5))


def _ffn_tie_weights(k1, n1, n2, rng):
    """first-layer weights that put every hidden value on a tie of the hidden slice's quantiser.  With x on the GRID (scale 2^-4, zp
    128) and weight scale 1, column j of W1 is 128 except one 129 at row 2 + j % (k1 - 2), so acc = code(x[., 2 + j % ..]) - 128 and
    h = acc / 16 + 128.5 / 16 = (code + 0.5) / 16 exactly; the last column (all 128, bias 255 / 16) is every row's maximum, so the
    hidden slice's range is [0, 255 / 16] -> scale 2^-4, zp 0 and (code + 0.5) / 16 is a tie for every code <= 254.  The grid
    slice's extremes sit in columns 0 and 1, which no tie column reads."""
    from lele_amd._lib import Weight
    w1 = np.full((k1, n1), 128.0, np.float32)
    j = np.arange(n1 - 1)
    w1[2 + j % (k1 - 2), j] = 129.0
    b1 = np.full(n1, 128.5 / 16, np.float32)
    b1[-1] = 255.0 / 16
    W1 = (Weight(w1), Weight(np.array([1.0], np.float32)), Weight(np.array([128.0], np.float32)), Weight(b1))
    return W1, _qw(rng, n1, n2)


def _grid_x(b, m, k, rng):
    """GRID slices (scale 2^-4, zp 128, every value a tie) whose single minimum / maximum sit in columns 0 / 1 of some row"""
    x = ((rng.integers(0, 255, (b, m, k)) + 0.5 - 128) / 16).astype(np.float32)
    s = np.arange(b)
    x[s, (s * 37) % m, 0] = GRID[0]
    x[s, (s * 53 + m - 1) % m, 1] = GRID[1]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("b,m", [(32, 171), (1, 504), (7, 700)])
def test_fused_ffn_hidden_layer_quantised_on_ties(ctx, orc, b, m):
    """fused_ffn_quantized (one-launch form, LELE_HIP_FFN_ONE_LAUNCH=2, and the two launches =0) and fused_ffn_quantized_ln with
    every hidden value on a tie of the hidden slice's quantiser (_ffn_tie_weights): the in-kernel re-quantisation of the hidden
    layer must round half to even like the oracle's SIMD body (n1 = 2048: no tail)"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(b * 3 + m)
    x = _grid_x(b, m, 512, rng)
    W1, W2 = _ffn_tie_weights(512, 2048, 512, rng)
    hid = orc.fused_quantized_linear(x, W1[0].arr, W1[1].arr, W1[2].arr, W1[3].arr, True)
    h16 = hid[..., :-1] * 16
    assert np.array_equal(h16 - np.floor(h16), np.full_like(h16, 0.5)), "hidden values are not all ties"
    want = orc.fused_quantized_linear(hid, W2[0].arr, W2[1].arr, W2[2].arr, W2[3].arr, False)
    xd = ctx.buf().upload(x)
    assert _same(K.fused_quantized_linear(xd, *W1, True, ctx=ctx).numpy(), hid)
    for one in (0, 2):
        with _env(LELE_HIP_FFN_ONE_LAUNCH=one):
            got = K.fused_ffn_quantized(xd, *W1, *W2, False, ctx=ctx).numpy()
            assert _same(got, want), (one, _diff(got, want))
    r1 = rng.standard_normal((b, m, 512)).astype(np.float32)
    g, be = _ln(rng)
    y = want + r1
    got = K.fused_ffn_quantized_ln(xd, *W1, *W2, False, r1, None, g, be, 1e-5, ctx=ctx)
    assert _same(got[0].numpy(), y), _diff(got[0].numpy(), y)
    assert _same(got[1].numpy(), orc.layer_norm(y, g.arr, be.arr, -1, 1e-5))


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(32, 171), (40, 100)])
def test_sanm_out_block_on_adversarial_slices(ctx, orc, b, t):
    """sanm_out_block (one launch at these shapes) on adversarial activations: the projection's quantisation is exact, the FSMN
    memory block within the convolution's 1e-4 (as in tests/test_quant.py)"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    from oracle import plan_ref
    from tests.parity import close_f32
    rng = np.random.default_rng(b * 7 + t)
    av = adversarial_batch(b, t, 512, b + t)
    qkv = rng.standard_normal((b, t, 1536)).astype(np.float32)
    w = _qw(rng, 512, 512)
    fw = Weight((rng.standard_normal((512, 1, 11)) / np.sqrt(11)).astype(np.float32))
    r2 = rng.standard_normal((b, t, 512)).astype(np.float32)
    g, be = _ln(rng)
    got = K.sanm_out_block(ctx.buf().upload(av), *w, False, ctx.buf().upload(qkv), fw, None, 1024, 5, 5, r2, g, be, 1e-5, ctx=ctx)
    o = plan_ref.PlanRef({"statements": [], "weights": {}, "outputs": [], "inputs": []}, {}).call(
        "sanm_out_block", [av, w[0].arr, w[1].arr, w[2].arr, w[3].arr, False, qkv, fw.arr, None, 1024, 5, 5, r2, g.arr, be.arr, 1e-5])
    close_f32(got[0].numpy(), o[0], 1e-4, "x1")
    close_f32(got[1].numpy(), o[1], 1e-4, "layer_norm(x1)")
    # the projection alone: exact (the memory block replaced by a zero residual)
    lin = K.fused_quantized_linear(ctx.buf().upload(av), *w, False, ctx=ctx).numpy()
    assert _same(lin, orc.fused_quantized_linear(av, w[0].arr, w[1].arr, w[2].arr, w[3].arr))


ODD_WEIGHTS = np.array([127.5, 128.5, 2.5, -3.0, 300.0, 0.5, 254.5, 255.5, -0.0, 1.5], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("b,m,k,n", [(1, 93, 560, 1536), (2, 5, 37, 19), (32, 171, 512, 1024), (1, 504, 2048, 512), (1, 33, 100, 130)])
def test_weights_off_the_u8_grid(ctx, orc, b, m, k, n):
    """f32 weights that are not integers or lie outside [0, 255]: the oracle models the reference's cvtps (half even) + saturating
    pack; the weight packers (wpack, wpack_frag, wcolsum) must agree on every route, and mat_mul_integer's B operand too"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(b + m + k + n)
    w = np.clip(np.round(128 + 32 * rng.standard_normal((k, n))), 0, 255).astype(np.float32)
    sel = rng.random((k, n)) < 0.3
    w[sel] = rng.choice(ODD_WEIGHTS, int(sel.sum()))
    ws = (np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32)
    bias = (rng.standard_normal(n) * 0.02).astype(np.float32)
    x = adversarial_batch(b, m, k, 7, kinds=("grid", "near", "zp_tie"))
    want = orc.fused_quantized_linear(x, w, ws, [128.0], bias, False)
    for W in (Weight(w), w):
        got = K.fused_quantized_linear(ctx.buf().upload(x), W, Weight(ws), Weight(np.array([128.0], np.float32)), Weight(bias), False,
                                       ctx=ctx).numpy()
        assert _same(got, want), _diff(got, want)
    a = rng.integers(0, 256, (b, m, k)).astype(np.float32)
    sel = rng.random(a.shape) < 0.2
    a[sel] = rng.choice(ODD_WEIGHTS, int(sel.sum()))
    got = K.mat_mul_integer(a, w, [3.0], [131.0], ctx=ctx).numpy()
    assert _same(got, orc.mat_mul_integer(a, w, [3.0], [131.0]))


@pytest.mark.gpu
def test_prepared_weight_entry_points_on_adversarial_slices(ctx, orc):
    """fused_dq_gemm_prepared quantises the activation like fused_quantized_linear: the adversarial slices through it, against the
    oracle (the u8 weights themselves cannot be off the grid here: they arrive as bytes)"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(17)
    for b, m, k, n in ((1, 93, 512, 512), (2, 9, 37, 19), (3, 171, 512, 96)):
        wu8 = rng.integers(0, 256, (k, n), dtype=np.uint8)
        ws = (np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32)
        bias = (rng.standard_normal(n) * 0.02).astype(np.float32)
        pw = K.prepare_weights(wu8, k, n, ctx=ctx)
        for kinds in (("grid", "near", "zp_tie"), ("pos", "neg", "spike")):
            x = adversarial_batch(b, m, k, k + n, kinds=kinds)
            got = K.fused_dq_gemm_prepared(x, pw, 128, ws, bias, False, ctx=ctx).numpy()
            want = orc.fused_quantized_linear(x, wu8.astype(np.float32), ws, [128.0], bias, False)
            assert _same(got, want), (b, m, k, n, kinds, _diff(got, want))
        pw.close()


@pytest.mark.gpu
def test_conv_integer_from_f32_rounds_ties_half_away(ctx):
    """conv_integer_from_f32 quantises with f32::round(x * inv + zp) (conv2d.rs), half away from zero: on inputs that are all ties
    (the GRID range) half even would give a different code for every even j"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    from oracle import npref
    from oracle import pyoracle as O
    rng = np.random.default_rng(23)
    for shape, pads in (((2, 8, 10, 10), [1, 1, 1, 1]), ((1, 5, 7, 9), [0, 0, 0, 0])):
        x = make_slice("grid", shape, rng, 3, int(np.prod(shape)) - 2)
        w = rng.integers(0, 256, (6, shape[1], 3, 3)).astype(np.float32)
        s, z = npref.dql_params([x])
        assert (s, z) == (F(1 / 16), F(128))
        q = npref.dql_quantize(x, s, z)
        assert not np.array_equal(q, np.clip(round_even(x * 16 + 128), 0, 255)), "no tie rounds differently"
        out, sc = K.conv_integer_from_f32(x, Weight(w), np.array([128.0], np.float32), [1, 1], 1, pads, [1, 1], ctx=ctx)
        assert sc.numpy()[0] == s
        assert _same(out.numpy(), O.conv_integer(q, w, z, 128.0, [1, 1], 1, pads, [1, 1]))


# ------------------------------------------------------------------------------------------------ 3. producer statistics (GPU)


def _spiky(b, m, k, rng, row):
    """activations whose LayerNorm / product has its slice maximum in ONE element: row `row` of every slice carries a spike"""
    x = rng.standard_normal((b, m, k)).astype(np.float32)
    x[:, row, k // 3] = 40.0
    return x


def _consume(ctx, t, w):
    """the consumer linear on t, its route asserted (CONSUMERS: which kernel reads the producer's statistics)"""
    from lele_amd import kernels as K
    got = K.fused_quantized_linear(t, *w, False, ctx=ctx).numpy()
    shp = tuple(t.shape)
    _route_is(ctx, int(np.prod(shp[:-2])), shp[-2], shp[-1], w[0].arr.shape[-1])
    return got


def _want(orc, host, w):
    return orc.fused_quantized_linear(host, w[0].arr, w[1].arr, w[2].arr, w[3].arr, False)


# consumers: (n, LELE_HIP_IGEMM_RS) -> (1024, 1) register-stationary where the rows fill the chip, (1024, 0) the tiled route; on 256 CUs
# the (32, 171) and (3, 1000) activations of K = 512 report CONSUMER_ROUTES (asserted below, every other call through _consume's _route_is)
CONSUMERS = ((1024, 1), (1024, 0))
CONSUMER_ROUTES = {(1024, 1): "q.rs_fq", (1024, 0): "q.tiled/igemm.t128x64"}


def _rewrites(ctx, orc, buf, shape, w, rng):
    """rewrite `buf` (which holds a [b, m, k] tensor with producer statistics) in every way the library offers and check that a
    consumer follows the NEW contents each time"""
    from lele_amd import kernels as K
    from lele_amd._lib import DevTensor
    b, m, k = shape
    t = DevTensor(buf, shape)
    cur = t.numpy()
    # an elementwise op into the same buffer
    y = K.mul(t, np.array([0.25], np.float32), out=buf, ctx=ctx)
    assert _same(_consume(ctx, y, w), _want(orc, cur * F(0.25), w)), "elementwise out="
    # a host upload
    new = (rng.standard_normal(shape) * 0.5).astype(np.float32)
    t = buf.upload(new)
    assert _same(_consume(ctx, t, w), _want(orc, new, w)), "upload"
    # a pitched write into a window: the first image's first half, the window holds the new extreme
    ln = K.layer_norm(t, np.ones(k, np.float32), np.zeros(k, np.float32), -1, 1e-5, out=buf, ctx=ctx)   # statistics again
    half = (rng.standard_normal((1, (m * k) // 2)) * 9).astype(np.float32)
    K.copy_view(half, out=buf, out_window=(0, m * k), ctx=ctx)
    host = DevTensor(buf, shape).numpy()
    assert _same(host.reshape(-1)[:half.size], half.ravel())
    assert _same(_consume(ctx, DevTensor(buf, shape), w), _want(orc, host, w)), "pitched window"
    # an external write through the data pointer, then mark_dirty
    K.layer_norm(DevTensor(buf, shape), np.ones(k, np.float32), np.zeros(k, np.float32), -1, 1e-5, out=buf, ctx=ctx)
    ctx.sync()
    ext = (rng.standard_normal(shape) * 5).astype(np.float32)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(buf.ptr), ext.ctypes.data_as(C.c_void_p), C.c_size_t(ext.nbytes), C.c_int(1)) == 0
    buf.mark_dirty()
    assert _same(_consume(ctx, DevTensor(buf, shape), w), _want(orc, ext, w)), "external write + mark_dirty"
    del ln


@pytest.mark.gpu
@pytest.mark.parametrize("n,rs", CONSUMERS)
@pytest.mark.parametrize("b,m", [(32, 171), (3, 1000)])
def test_layer_norm_statistics_feed_consumers_and_go_stale(ctx, orc, b, m, n, rs):
    """kind 0 (one pair per row, layer_norm): the consumer's result equals the oracle on the tensor as read back; every rewrite of the
    buffer is followed; every reinterpretation of the same pointer as another (batch, m) gives the oracle's result for THAT batching"""
    from lele_amd import kernels as K
    from lele_amd._lib import DevTensor
    rng = np.random.default_rng(b * m + n + rs)
    k = 512
    w = _qw(rng, k, n)
    g, be = _ln(rng, k)
    x = _spiky(b, m, k, rng, m - 1)          # the extreme in a slice's last row (a tile / workgroup boundary for 171 rows)
    buf = ctx.buf()
    with _env(LELE_HIP_IGEMM_RS=rs):
        xn = K.layer_norm(ctx.buf().upload(x), g, be, -1, 1e-5, out=buf, ctx=ctx)
        host = xn.numpy()
        assert _same(_consume(ctx, xn, w), _want(orc, host, w))
        _route_is(ctx, b, m, k, n, CONSUMER_ROUTES[(n, rs)])
        rows = b * m
        for bb in [d for d in (1, 2, 3, 19, b, rows) if rows % d == 0]:   # kind 0 is one pair per row: any batching of the rows
            view = DevTensor(buf, (bb, rows // bb, k))
            assert _same(_consume(ctx, view, w), _want(orc, host.reshape(bb, rows // bb, k), w)), ("reinterpretation", bb)
        _rewrites(ctx, orc, buf, (b, m, k), w, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("n,rs", CONSUMERS)
def test_residual_ln_statistics_feed_consumers_and_go_stale(ctx, orc, n, rs):
    """kind 0 published by the LayerNorm in igemm_as_kernel's epilogue (fused_quantized_linear_residual_ln at (32, 171))"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(5 + n + rs)
    b, m = 32, 171
    x = adversarial_batch(b, m, 512, 3)
    w0 = _qw(rng, 512, 512)
    r1 = _spiky(b, m, 512, rng, 0)
    g, be = _ln(rng)
    w = _qw(rng, 512, n)
    buf = ctx.buf()
    with _env(LELE_HIP_IGEMM_RS=rs):
        _, xn = K.fused_quantized_linear_residual_ln(ctx.buf().upload(x), *w0, False, r1, None, g, be, 1e-5, outs=[ctx.buf(), buf], ctx=ctx)
        assert _same(_consume(ctx, xn, w), _want(orc, xn.numpy(), w))
        _route_is(ctx, b, m, 512, n, CONSUMER_ROUTES[(n, rs)])
        _rewrites(ctx, orc, buf, (b, m, 512), w, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("n,rs", CONSUMERS)
@pytest.mark.parametrize("m,k,h", [(504, 512, 2048), (93, 512, 2048), (7, 512, 2048), (1000, 512, 1024)])
def test_gemm_statistics_feed_consumers_and_go_stale(ctx, orc, m, k, h, n, rs):
    """kind 1 (per-workgroup pairs, one slice): the small-problem GEMM (m = 7, 93) and the register-stationary epilogue (m = 504,
    1000) publish them beside a ReLU hidden layer whose extreme is in one row"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(m + k + h + n + rs)
    w1, w = _qw(rng, k, h), _qw(rng, h, n)
    x = _spiky(1, m, k, rng, m // 2)
    buf = ctx.buf()
    with _env(LELE_HIP_IGEMM_RS=rs):
        hid = K.fused_quantized_linear(ctx.buf().upload(x), *w1, True, out=buf, ctx=ctx)
        host = hid.numpy()
        assert _same(host, orc.fused_quantized_linear(x, w1[0].arr, w1[1].arr, w1[2].arr, w1[3].arr, True))
        assert _same(_consume(ctx, hid, w), _want(orc, host, w))
        _rewrites(ctx, orc, buf, (1, m, h), w, rng)


H, DH = 4, 128
QC = [["slice", 2, 0, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
KC = [["slice", 2, 512, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 3, 1]]]
VC = [["slice", 2, 1024, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,rs", CONSUMERS)
@pytest.mark.parametrize("b,t", [(32, 171), (1, 504)])
def test_attention_statistics_feed_consumers_and_go_stale(ctx, orc, b, t, n, rs):
    """kind 2 (a fixed number of pairs per slice) published by attention_view; one utterance's values spike in one head"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(b * t + n + rs)
    qkv = (rng.standard_normal((b, t, 1536)) * 1.5).astype(np.float32)
    qkv[:, :, 1024 + 300] *= 30          # v of one channel of head 2: the extreme of every slice sits in one column
    scale = Weight(np.array([DH ** -0.5], np.float32))
    w = _qw(rng, 512, n)
    buf = ctx.buf()
    with _env(LELE_HIP_IGEMM_RS=rs):
        qd = ctx.buf().upload(qkv)
        av = K.attention_view(qd, QC, qd, KC, qd, VC, scale, [0, 2, 1, 3], [0, 0, H * DH], out=buf, ctx=ctx)
        host = av.numpy()
        assert _same(_consume(ctx, av, w), _want(orc, host, w))
        if b > 1:   # kind 2 is keyed on (batch, m): other batchings of the same pointer take their own range pass
            from lele_amd._lib import DevTensor
            for bb in (1, 2, 96):      # 5472 rows
                v = DevTensor(buf, (bb, b * t // bb, 512))
                assert _same(_consume(ctx, v, w), _want(orc, host.reshape(bb, -1, 512), w)), bb
        _rewrites(ctx, orc, buf, (b, t, 512), w, rng)


# ------------------------------------------------------------------------------------------------ the recorded-graph case


@pytest.mark.gpu
@pytest.mark.parametrize("producer", ["layer_norm", "attention_view"])
def test_graph_replay_does_not_reuse_statistics_published_before_the_capture(ctx, orc, producer):
    """A buffer carries a producer's statistics (kind 0: layer_norm, kind 2: attention_view) from an eager call; a consumer is recorded
    into a graph; new contents are uploaded into the buffer and the graph replayed.  The replay must quantise the NEW contents with
    their own range.  Then the same with the producer recorded into the graph as well: its statistics are handed over inside."""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(99 + len(producer))
    b, t = 32, 171
    w = _qw(rng, 512, 1024)
    g, be = _ln(rng)
    scale = Weight(np.array([DH ** -0.5], np.float32))
    src = ctx.buf()
    buf = ctx.buf()
    ob = ctx.buf()
    src_t =src.upload(_spiky(b, t, 512, rng, 5) if producer == "layer_norm" else (rng.standard_normal((b, t, 1536)) * 1.5).astype(np.float32))

    def produce():
        if producer == "layer_norm":
            return K.layer_norm(src_t, g, be, -1, 1e-5, out=buf, ctx=ctx)
        return K.attention_view(src_t, QC, src_t, KC, src_t, VC, scale, [0, 2, 1, 3], [0, 0, H * DH], out=buf, ctx=ctx)

    y = produce()                          # eager: statistics beside buf
    first = y.numpy()
    assert _same(K.fused_quantized_linear(y, *w, False, out=ob, ctx=ctx).numpy(), _want(orc, first, w))
    ctx.sync()
    ctx.graph_begin()
    r = K.fused_quantized_linear(y, *w, False, out=ob, ctx=ctx)
    gr = ctx.graph_end()
    try:
        new = (rng.standard_normal((b, t, 512)) * 0.2).astype(np.float32)      # a much narrower range than the producer's output
        new[3, 17, 200] = 0.9
        nt = buf.upload(new)
        gr.launch()
        got = r.numpy()
        assert _same(got, _want(orc, new, w)), "replay quantised the new contents with the old range: " + _diff(got, _want(orc, new, w))
    finally:
        gr.close()
    # the producer inside the graph: the hand-over of its statistics is recorded with it
    y = produce()
    ctx.sync()
    ctx.graph_begin()
    y = produce()
    r = K.fused_quantized_linear(y, *w, False, out=ob, ctx=ctx)
    gr = ctx.graph_end()
    try:
        buf.upload(new)                    # overwritten by the producer on replay
        gr.launch()
        host = y.numpy()
        assert _same(host, first)
        assert _same(r.numpy(), _want(orc, host, w))
    finally:
        gr.close()
    del nt
