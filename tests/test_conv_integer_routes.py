"""Every route of the ConvInteger family on the i8 matrix cores (lele_amd/csrc/conv.hip: ci_run, ci8_pack_kernel, ci8_wfrag_kernel,
ci8_conv_kernel<NJ, KSPLIT>) against the exact integer convolution, bit for bit: one table row per kernel and geometry edge.

The i8 route reports how the image was packed ("ci8.codes": u8 codes as given; "ci8.quant": the from_f32 forms quantise on the way) and
the instantiation that ran: "ci8.nj4" / "ci8.nj2" / "ci8.nj1" (a wave owns 4 / 2 / 1 strips of 32 positions) or "ci8.nj2_ksplit" /
"ci8.nj1_ksplit" (the four waves of a workgroup share the strips and take every fourth (tap, chunk) step).  Which one runs depends on the
CU count, so a row's batch size is a function of kernels.num_cus(): the dispatch is restated here (dispatch) and every row names the route
the library must report.  fused_scale_bias(_silu) reports "fsb.w1"; the f32 form keeps "ci.f32/<the convolution's own route>".

Why bits.  The device sums i8 products in i32 and converts once, so the exact integer convolution (exact_ref: the u8 image padded with
zeros, (x - zx)(w - zw) accumulated per tap in float64, every sum far below 2^53) rounded once to f32 is the reference at every
magnitude.  Where K max|x - zx| max|w - zw| < 2^24 (tests/test_conv_integer.py::_exact) the oracle's f32 sums are exact too and the
device must equal oracle.pyoracle.conv_integer as well.  Rows on the f32 route keep the bar of tests/test_conv_integer.py: equality
when _exact, else 1e-4 (accept_close).

Families, each on every row: "random" (uniform codes, five zero-point pairs), "extreme" (blocks of all-0 and all-255 codes, the four
corner zero points: the largest magnitudes of every sign), "coded" (one lit pixel per image with a distinct code per channel, weights a
function of (oc, c, tap): an output names the tap, channel and output channel it came from), "dirty" (an all-255 call with C rounded up
to 32 and the same N H W immediately before, both images device-resident so that they start at the same arena byte: the bytes under
channels [C, Cp) are then 0xFF and only the weight fragments' zeros keep them out; checked once on an MI355X with a library whose
fragments pad with +1 instead: every output whose window lies inside the image then gained exactly 127 per tap and stale channel).

Not tested: x is trusted to hold u8 codes, as the header says (non-code or NaN activations to conv_integer); NaN into the dynamic
quantisation of the from_f32 forms.

CPU part: name coverage, the rows against the restated dispatch for 64 / 256 / 304 CUs, exact_ref against a brute-force loop and the
oracle, the device's algebra restated (emulate) and eight wrong variants of it that at least one family of each row tells apart (on four
images at the most: the inputs are the same function of the batch size).
GPU part: every row asserts last_route() after a call of another family, then the values."""
import re

import numpy as np
import pytest

from oracle import npref
from oracle import pyoracle as O

CUS = 256
PREFIXES = ("ci8.", "fsb.")
NOT_COVERED = {}   # a key that is a route name would take that name out of the coverage requirement; there is none
CORES = ("ci8.nj4", "ci8.nj2", "ci8.nj1", "ci8.nj2_ksplit", "ci8.nj1_ksplit")
ZPS = ((128.0, 128.0), (0.0, 113.0), (7.0, 0.0), (None, None), (255.0, 255.0))
CORNERS = ((0.0, 0.0), (0.0, 255.0), (255.0, 0.0), (255.0, 255.0))
FAMILIES = ("random", "extreme", "coded", "dirty")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def accept_bits(got, want):
    """"" when got == want bit for bit, else what differs"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, want %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    if not bad.any():
        return ""
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d of %d differ, the first at %s: got %r want %r" % (int(bad.sum()), bad.size, at, got[at], want[at])


def accept_close(got, want, tol=1e-4):
    """tests/test_conv_integer.py::_close as a verdict"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    floor = tol * float(np.sqrt(np.mean(np.square(want)))) + 1e-7
    bad = np.abs(got - want) > tol * np.abs(want) + floor
    return "" if not bad.any() else "%d of %d outside %g (max |diff| %.3e)" % (int(bad.sum()), want.size, tol, float(np.abs(got - want).max()))


def is_exact(x, xz, w, wz):
    """tests/test_conv_integer.py::_exact: no f32 partial sum of the oracle can round"""
    k = w.shape[1] * w.shape[2] * w.shape[3]
    return k * float(np.abs(x - xz).max()) * float(np.abs(w - wz).max()) < 2.0 ** 24


# ================================================================================================= geometry and the dispatch, restated
def geometry(r):
    """a row's output size: pads are [top, left, bottom, right]"""
    (kh, kw), (pt, pl, pb, pr), (sh, sw), (dh, dw) = r["k"], r["pads"], r["strides"], r["dil"]
    oh = (r["H"] + pt + pb - dh * (kh - 1) - 1) // sh + 1
    ow = (r["W"] + pl + pr - dw * (kw - 1) - 1) // sw + 1
    return dict(oh=oh, ow=ow, plane=oh * ow, taps=kh * kw, steps=kh * kw * ((r["C"] + 31) // 32))


def dispatch(N, C, OC, plane, taps, cus):
    """ci_run: the widest wave tile that still gives every CU two workgroups; below that the waves of a workgroup split K"""
    tiles, steps = (OC + 31) // 32, taps * ((C + 31) // 32)
    units, want = N * tiles, 2 * cus
    blocks = lambda nj, ks: (plane + (1 if ks else 4) * 32 * nj - 1) // ((1 if ks else 4) * 32 * nj)   # noqa: E731
    if units * blocks(4, False) >= want:
        return "ci8.nj4"
    if units * blocks(2, False) >= want:
        return "ci8.nj2"
    if units * blocks(1, False) >= want or steps < 8:
        return "ci8.nj1"
    if units * blocks(2, True) >= want:
        return "ci8.nj2_ksplit"
    return "ci8.nj1_ksplit"


def batch_of(r, cus=CUS):
    """a row's N: a number, a function of the CU count, or (None) the smallest batch that `cus` CUs send to the row's kernel"""
    n = r["N"]
    if callable(n):
        return n(cus)
    if n is not None:
        return n
    g = geometry(r)
    for n in range(1, 16 * cus):
        if dispatch(n, r["C"], r["OC"], g["plane"], g["taps"], cus) == r["core"]:
            return n
    raise AssertionError("%s: no batch size reaches %s on %d CUs" % (r["id"], r["core"], cus))


def route_of(r, cus=CUS):
    if r["core"] == "ci.f32":
        return "ci.f32"
    g = geometry(r)
    return "ci8.%s/%s" % (r["form"], dispatch(batch_of(r, cus), r["C"], r["OC"], g["plane"], g["taps"], cus))


# ================================================================================================================ the table
def row(why, core, C=5, OC=40, H=22, W=25, N=None, k=(3, 3), pads=(1, 1, 1, 1), strides=(1, 1), dil=(1, 1), form="codes"):
    r = dict(why=why, core=core, C=C, OC=OC, H=H, W=W, N=N, k=k, pads=pads, strides=strides, dil=dil, form=form)
    r["route"] = "ci.f32" if core == "ci.f32" else "ci8.%s/%s" % (form, core)
    r["id"] = "%s-%s-%s" % (form, core.split(".")[1], re.sub(r"[^a-z0-9]+", "_", why.lower())[:44].strip("_"))
    return r


def eighth(cus):
    return -(-2 * cus // 8)


def sixteenth(cus):
    return -(-2 * cus // 16)


# the five kernels: C = 5, OC = 40 (two tiles, the second ragged), 3 x 3, pad 1: 9 steps; every plane off the multiples of 32 NJ
ROWS = [
    row("plane 2115", "ci8.nj4", H=45, W=47, N=eighth),
    row("plane 1085", "ci8.nj2", H=31, W=35, N=eighth),
    row("plane 550", "ci8.nj1", N=eighth),
    row("plane 550", "ci8.nj2_ksplit", N=sixteenth),
    row("plane 550", "ci8.nj1_ksplit", N=2),
]
# the geometry edges, each on a kernel that splits K and on one that does not (N = None: the smallest batch that reaches the kernel)
for _why, _a, _b, _kw in (
        ("C = 1: one channel of a chunk", "ci8.nj1", "ci8.nj1_ksplit", dict(C=1)),
        ("C = 17: past 16, the second half-wave's channels", "ci8.nj2", "ci8.nj2_ksplit", dict(C=17)),
        ("C = 33: two chunks, 18 steps", "ci8.nj1", "ci8.nj1_ksplit", dict(C=33)),
        ("C = 65: three chunks, 27 steps", "ci8.nj1", "ci8.nj2_ksplit", dict(C=65, H=10, W=13)),
        ("OC = 1: one output channel", "ci8.nj1", "ci8.nj1_ksplit", dict(OC=1)),
        ("OC = 33: one channel in the second tile", "ci8.nj2", "ci8.nj2_ksplit", dict(OC=33)),
        ("pads 2 0 1 3", "ci8.nj1", "ci8.nj1_ksplit", dict(pads=(2, 0, 1, 3))),
        ("stride 2", "ci8.nj1", "ci8.nj2_ksplit", dict(H=43, W=49, strides=(2, 2))),
        ("dilation 2 1", "ci8.nj2", "ci8.nj1_ksplit", dict(dil=(2, 1))),
        ("kernel 5 x 3: 15 steps", "ci8.nj1", "ci8.nj1_ksplit", dict(k=(5, 3), pads=(2, 1, 2, 1))),
        ("plane 20: less than one strip", "ci8.nj4", "ci8.nj1_ksplit", dict(H=4, W=5)),
        ("kernel 4 x 2: 8 steps", "ci8.nj1", "ci8.nj1_ksplit", dict(k=(4, 2), pads=(1, 0, 2, 1))),
):
    ROWS += [row(_why, _a, **_kw), row(_why, _b, **_kw)]
ROWS += [
    row("kernel 7 x 1: 7 steps, too few to split", "ci8.nj1", N=1, k=(7, 1), pads=(3, 0, 3, 0)),
    row("kernel 4 x 2: 8 steps, one image", "ci8.nj1_ksplit", N=1, k=(4, 2), pads=(1, 0, 2, 1)),
]
QUANT_ROWS = [
    row("plane 1085", "ci8.nj2", H=31, W=35, N=eighth, form="quant"),
    row("plane 550", "ci8.nj1_ksplit", N=2, form="quant"),
    row("C = 33 stride 2", "ci8.nj2_ksplit", C=33, H=43, W=49, strides=(2, 2), form="quant"),
]
# the multi form: a 1 x 1 convolution over channel-concatenated sources (one step: never split); `C` lists the sources' channels
MULTI_ROWS = [
    row("sources 4 5 3", "ci8.nj1", C=12, OC=6, H=7, W=9, N=2, k=(1, 1), pads=(0, 0, 0, 0), form="quant"),
    row("sources 5 3", "ci8.nj2", C=8, OC=6, H=31, W=35, k=(1, 1), pads=(0, 0, 0, 0), form="quant"),
]
MULTI_SOURCES = {MULTI_ROWS[0]["id"]: (4, 5, 3), MULTI_ROWS[1]["id"]: (5, 3)}
KBOUND = row("K = 33025, the largest the i8 guard admits", "ci8.nj1_ksplit", C=1321, OC=2, H=6, W=6, N=2, k=(5, 5), pads=(2, 2, 2, 2))
KBEYOND = row("K = 33026", "ci.f32", C=16513, OC=2, H=3, W=3, N=1, k=(2, 1), pads=(0, 0, 0, 0))
FSB_ROUTES = ("fsb.w1",)
ALL_ROWS = ROWS + QUANT_ROWS + MULTI_ROWS + [KBOUND, KBEYOND]
IDS = [r["id"] for r in ALL_ROWS]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)


# ================================================================================================================ references
def conv_core(xp, w, r):
    """xp [N, C, PH, PW] (already padded), w [OC, C, kh, kw], float64 -> [N, OC, oh, ow]: one matrix product per tap"""
    g = geometry(r)
    (kh, kw), (sh, sw), (dh, dw) = r["k"], r["strides"], r["dil"]
    n, c = xp.shape[:2]
    out = np.zeros((n, w.shape[0], g["plane"]), np.float64)
    for a in range(kh):
        for b in range(kw):
            win = xp[:, :, a * dh:a * dh + (g["oh"] - 1) * sh + 1:sh, b * dw:b * dw + (g["ow"] - 1) * sw + 1:sw]
            out += np.matmul(w[None, :, :, a, b], win.reshape(n, c, g["plane"]))
    return out.reshape(n, w.shape[0], g["oh"], g["ow"])


def padded(x, r, value=0.0):
    pt, pl, pb, pr = r["pads"]
    return np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=value)


def exact_ref(x, w, zx, zw, r, pad_value=0.0):
    """the exact integer convolution, rounded once: a padded cell is the u8 code 0"""
    out = conv_core(padded(x, r, pad_value) - (zx or 0.0), np.asarray(w, np.float64) - (zw or 0.0), r)
    assert np.abs(out).max(initial=0.0) < 2.0 ** 53
    return out.astype(np.float32)


def oracle_ref(x, w, zx, zw, r):
    return O.conv_integer(x, w, zx or 0.0, zw or 0.0, list(r["dil"]), 1, list(r["pads"]), list(r["strides"]))


VARIANTS = ("pad_is_zero_point", "drop_last_channel", "zp_exchanged", "k_from_cp", "oc_xor_4", "skip_last_tap", "tail_strip_clamped",
            "stale_pad_code0")


def applicable(variant, r):
    """where a variant cannot change anything: no padded cell / no partner output channel"""
    if variant == "pad_is_zero_point":
        return any(r["pads"])
    if variant == "oc_xor_4":
        return r["OC"] > 4
    return True


def emulate(x, w, zx, zw, r, variant=None):
    """the device's algebra in float64 (conv.hip's section comment): a = x~ - 128 and b = w - 128 multiplied as i8, the zero points
    applied through the window sums of the codes, the weights' sums and K.  `variant`: one of the wrong kernels of VARIANTS"""
    zx, zw = zx or 0.0, zw or 0.0
    if variant == "pad_is_zero_point":
        return exact_ref(x, w, zx, zw, r, pad_value=zx)
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    c, taps = x.shape[1], r["k"][0] * r["k"][1]
    cp, c4, kk = (c + 31) // 32 * 32, (c + 3) // 4 * 4, c * taps
    xa, wb = padded(x, r) - 128.0, w - 128.0
    if variant == "drop_last_channel":
        xa, wb = xa[:, :c - 1], wb[:, :c - 1]
    if variant == "skip_last_tap":
        wb = wb.copy()
        wb[:, :, -1, -1] = 0.0
    acc = conv_core(xa, wb, r)
    sx = conv_core(padded(x, r), np.ones((1, c) + tuple(r["k"])), r)
    wsum = w.sum(axis=(1, 2, 3)).reshape(1, -1, 1, 1)
    if variant == "stale_pad_code0":   # channels [C, C4) were packed as code 0, [C4, Cp) hold 0xFF; the fragment pads with code 0 = -128 as i8
        inside = conv_core(padded(np.ones((x.shape[0], 1) + x.shape[2:]), r), np.ones((1, 1) + tuple(r["k"])), r)
        acc = acc + inside * ((c4 - c) * 16384.0 + (cp - c4) * -16256.0)
    konst = kk * zx * zw - 16384.0 * (cp * taps if variant == "k_from_cp" else kk)
    za, zb = (zx, zw) if variant == "zp_exchanged" else (zw, zx)
    out = acc + (128.0 - za) * sx + (128.0 - zb) * wsum + konst
    if variant == "oc_xor_4":
        o = np.arange(out.shape[1])
        src = np.where((o ^ 4) < out.shape[1], o ^ 4, o)
        out = out[:, src]
    if variant == "tail_strip_clamped":
        flat = out.reshape(out.shape[0], out.shape[1], -1).copy()
        flat[:, :, (flat.shape[2] - 1) // 32 * 32:] = flat[:, :, -1:]
        out = flat.reshape(out.shape)
    return out.astype(np.float32)


# ================================================================================================================ inputs
def codes(rng, shape):
    return rng.integers(0, 256, shape).astype(np.float32)


def coded_weights(oc, c, kh, kw):
    """a u8 code from (oc, c, tap): neighbours along every axis differ"""
    o, ch, t = np.meshgrid(np.arange(oc), np.arange(c), np.arange(kh * kw), indexing="ij")
    return ((o * 7 + ch * 13 + t * 29 + 1) % 256).astype(np.float32).reshape(oc, c, kh, kw)


def cases(r, family, cus=CUS, n=None):
    """[(tag, x, w, zx, zw)] of one family for a row; the same on every machine with `cus` CUs"""
    n = batch_of(r, cus) if n is None else n
    c, oc, h, w_, (kh, kw) = r["C"], r["OC"], r["H"], r["W"], r["k"]
    rng = np.random.default_rng([IDS.index(r["id"]), FAMILIES.index(family)])
    if family == "random":
        x, w = codes(rng, (n, c, h, w_)), codes(rng, (oc, c, kh, kw))
        return [("zp %s %s" % z, x, w) + z for z in ZPS]
    if family == "extreme":
        x = np.zeros((n, c, h, w_), np.float32)
        x[0::2, :, :, :(w_ + 1) // 2] = 255.0
        x[1::2, :, h // 2:, :] = 255.0
        x[2::4, c // 2:] = 255.0 - x[2::4, c // 2:]
        x[3::4, c // 2:] = 255.0 - x[3::4, c // 2:]
        if r["H"] * r["W"] < 64:   # an image too small to hold a whole window of one block: the first is all 255
            x[0] = 255.0
        w = np.zeros((oc, c, kh * kw), np.float32)
        w[0::4] = 255.0
        w[2::4, :, :(kh * kw + 1) // 2] = 255.0
        w[3::4, :(c + 1) // 2] = 255.0
        return [("corner %g %g" % z, x, w.reshape(oc, c, kh, kw)) + z for z in CORNERS]
    if family == "coded":
        x = np.zeros((n, c, h, w_), np.float32)
        i = np.arange(n)
        x[i, :, (i * 5) % h, (i * 3 + w_ - 1) % w_] = (np.arange(c) % 250 + 1).astype(np.float32)[None, :]
        return [("coded", x, coded_weights(oc, c, kh, kw), None, None)]
    return [("dirty", codes(rng, (n, c, h, w_)), codes(rng, (oc, c, kh, kw)), 7.0, 113.0)]


def f32_source(rng, shape, kind):
    """activations for the from_f32 forms: "random", or "ties": every value (j + 0.5 - 128) / 16 with the range -8 .. 7.9375, so that
    scale = 1 / 16, zp = 128 and every code is decided by the rounding of a tie (tests/test_quant_adversarial.py, GRID)"""
    if kind == "random":
        return (rng.standard_normal(shape) * 3).astype(np.float32)
    x = ((rng.integers(0, 255, shape) + 0.5 - 128) / 16).astype(np.float32)
    x.reshape(-1)[3], x.reshape(-1)[-2] = -8.0, 7.9375
    return x


# ================================================================================================================ CPU tests
def test_rows_cover_every_ci8_and_fsb_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}
    assert len(mine) == 8
    used = {lvl for r in ALL_ROWS for lvl in r["route"].split("/") if lvl.startswith(PREFIXES)} | set(FSB_ROUTES)
    named = set(NOT_COVERED) & set(names)
    assert not (used | named) - mine, "routes the library cannot report: %s" % sorted((used | named) - mine)
    assert not used & named
    assert mine - used == named, "routes no row reaches: %s" % sorted(mine - used - named)
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_COVERED.values())
    assert "ci.f32" in names
    # both forms of packing on a kernel that splits K and on a wide one that does not
    assert {(r["form"], r["core"]) for r in ALL_ROWS} >= {("codes", c) for c in CORES} | {("quant", "ci8.nj2"), ("quant", "ci8.nj1_ksplit")}


def test_rows_satisfy_the_dispatch_they_state():
    for r in ALL_ROWS:
        g = geometry(r)
        for cus in (64, CUS, 304):
            assert route_of(r, cus) == r["route"], (r["id"], cus)
        nj = {"ci8.nj4": 4, "ci8.nj2": 2, "ci8.nj2_ksplit": 2}.get(r["core"], 1)
        if "plane 20" not in r["why"] and r["core"] != "ci.f32":   # the tail strip and the tail wave of every variant run
            assert g["plane"] % (32 * nj) and g["plane"] % (128 * nj), r["id"]
        if r["core"].endswith("ksplit"):
            assert g["steps"] >= 8, r["id"]
    head = ROWS[:5]
    assert [(r["core"], geometry(r)["plane"], geometry(r)["steps"]) for r in head] == [
        ("ci8.nj4", 2115, 9), ("ci8.nj2", 1085, 9), ("ci8.nj1", 550, 9), ("ci8.nj2_ksplit", 550, 9), ("ci8.nj1_ksplit", 550, 9)]
    assert [batch_of(r) for r in head] == [64, 64, 64, 32, 2]
    steps = {(geometry(r)["steps"], r["core"].endswith("ksplit")) for r in ROWS}
    assert {(7, False), (8, False), (8, True), (9, False), (9, True)} <= steps          # around steps_lt8
    assert any(s % 4 and ks for s, ks in steps) and {15, 18, 27} <= {s for s, _ in steps}  # waves with unequal step counts
    assert {r["C"] for r in ROWS} == {1, 5, 17, 33, 65} and {r["OC"] for r in ROWS} == {1, 33, 40}
    assert geometry(KBOUND)["taps"] * KBOUND["C"] == 33025 and 33025 * 65025 < 2 ** 31 <= 33026 * 65025
    assert geometry(KBEYOND)["taps"] * KBEYOND["C"] == 33026
    assert all(sum(MULTI_SOURCES[r["id"]]) == r["C"] for r in MULTI_ROWS)


def test_exact_reference_is_the_brute_force_sum():
    r = row("tiny", "ci8.nj1", C=3, OC=5, H=5, W=6, N=2, k=(3, 2), pads=(2, 0, 1, 1), strides=(2, 1), dil=(1, 2))
    g = geometry(r)
    rng = np.random.default_rng(0)
    x, w = codes(rng, (2, 3, 5, 6)).astype(np.int64), codes(rng, (5, 3, 3, 2)).astype(np.int64)
    zx, zw = 9, 200
    want = np.zeros((2, 5, g["oh"], g["ow"]), np.int64)
    for n in range(2):
        for o in range(5):
            for oy in range(g["oh"]):
                for ox in range(g["ow"]):
                    for c in range(3):
                        for a in range(3):
                            for b in range(2):
                                iy, ix = oy * 2 - 2 + a, ox - 0 + 2 * b
                                code = x[n, c, iy, ix] if 0 <= iy < 5 and 0 <= ix < 6 else 0
                                want[n, o, oy, ox] += (code - zx) * (w[o, c, a, b] - zw)
    xf, wf = x.astype(np.float32), w.astype(np.float32)
    assert accept_bits(exact_ref(xf, wf, 9.0, 200.0, r), want.astype(np.float32)) == ""
    assert accept_bits(emulate(xf, wf, 9.0, 200.0, r), want.astype(np.float32)) == ""
    assert accept_bits(oracle_ref(xf, wf, 9.0, 200.0, r), want.astype(np.float32)) == ""


@pytest.mark.parametrize("r", ROWS + [KBOUND], ids=[r["id"] for r in ROWS + [KBOUND]])
def test_row_inputs_tell_wrong_kernels_apart(r):
    """the exact reference equals the device's algebra on every case and the oracle wherever _exact holds; each variant of VARIANTS
    differs from the reference on at least one family's case (on four images at the most)"""
    n = min(batch_of(r), 4)
    fam = {f: cases(r, f, n=n) for f in FAMILIES} if r is not KBOUND else {"extreme": cases(r, "extreme", n=2)}
    refs, exact = {}, 0
    for f, cs in fam.items():
        for tag, x, w, zx, zw in cs:
            want = refs[(f, tag)] = exact_ref(x, w, zx, zw, r)
            assert accept_bits(emulate(x, w, zx, zw, r), want) == "", (f, tag)
            if is_exact(x, zx or 0.0, w, zw or 0.0):
                assert accept_bits(oracle_ref(x, w, zx, zw, r), want) == "", (f, tag)
                exact += 1
    assert exact or r["C"] * geometry(r)["taps"] * 255 * 255 >= 2 ** 24 or r is KBOUND, "no case on which the oracle is exact"
    if r["C"] == 5:
        assert exact >= 5   # C = 5 with 3 x 3 taps: K 255^2 = 2.9e6, every random case is exact
    for v in VARIANTS:
        told = any(accept_bits(emulate(x, w, zx, zw, r, v), refs[(f, tag)]) != "" for f, cs in fam.items() for tag, x, w, zx, zw in cs)
        assert told == applicable(v, r), (v, "not told apart" if not told else "differs where it cannot")
    if r is KBOUND:   # what the epilogue's partial sums reach at the corners: past 2^31 before the constant brings them back
        worst = 0.0
        for tag, x, w, zx, zw in fam["extreme"]:
            kk = r["C"] * geometry(r)["taps"]
            acc = conv_core(padded(x, r) - 128.0, np.asarray(w, np.float64) - 128.0, r)
            sx = conv_core(padded(x, r), np.ones((1, r["C"]) + tuple(r["k"])), r)
            part = acc + (128.0 - zw) * sx
            part2 = part + (128.0 - zx) * np.asarray(w, np.float64).sum(axis=(1, 2, 3)).reshape(1, -1, 1, 1)
            worst = max(worst, float(np.abs(part).max()), float(np.abs(part2).max()))
            assert float(np.abs(part2 + kk * zx * zw - 16384.0 * kk).max()) < 2.0 ** 31
        assert worst >= 2.0 ** 31, worst


# ================================================================================================================ GPU tests
def stale(K, ctx):
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)   # another family's route first: a stale name would show
    assert K.last_route(ctx) and not K.last_route(ctx).startswith(("ci", "fsb"))


def zp(v):
    return None if v is None else np.array([v], np.float32)


def call(K, ctx, r, x, w, zx, zw):
    stale(K, ctx)
    got = K.conv_integer(x, w, zp(zx), zp(zw), list(r["dil"]), 1, list(r["pads"]), list(r["strides"]), ctx=ctx).numpy().copy()
    return got, K.last_route(ctx)


def dirty_arena(K, ctx, r, n):
    """an all-255 image of Cp channels and the same N H W, device-resident like the image of the call that follows: both packed images
    start at the arena's first byte"""
    from lele_amd._lib import Weight
    from lele_amd.tensor import TensorView
    cp = (r["C"] + 31) // 32 * 32
    x = TensorView(ctx.buf().upload(np.full((n, cp, r["H"], r["W"]), 255.0, np.float32)))
    got = K.conv_integer(x, Weight(np.full((1, cp, 1, 1), 255.0, np.float32)), zp(0.0), zp(0.0), ctx=ctx).numpy()
    assert K.last_route(ctx).startswith("ci8.codes/") and np.all(got == cp * 255.0 * 255.0)


def check_codes_row(K, ctx, r, cus):
    from lele_amd._lib import Weight
    from lele_amd.tensor import TensorView
    want_route = route_of(r, cus)
    assert want_route == r["route"], (r["id"], cus)
    n, exact = batch_of(r, cus), 0
    for family in FAMILIES:
        for tag, x, w, zx, zw in cases(r, family, cus):
            wt = Weight(w)
            if family == "dirty":
                dirty_arena(K, ctx, r, n)
                x_in = TensorView(ctx.buf().upload(x))
            else:
                x_in = x
            got, route = call(K, ctx, r, x_in, wt, zx, zw)
            assert route == want_route, (r["id"], family, tag, route)
            want = exact_ref(x, w, zx, zw, r)
            msg = accept_bits(got, want)
            assert msg == "", (r["id"], family, tag, msg)
            if is_exact(x, zx or 0.0, w, zw or 0.0):
                msg = accept_bits(got, oracle_ref(x, w, zx, zw, r))
                assert msg == "", (r["id"], family, tag, "against the oracle", msg)
                exact += 1
            if r["core"].endswith("ksplit"):   # the waves meet in LDS, the channel sums in integer atomics: any order, the same bits
                again, _ = call(K, ctx, r, x_in, wt, zx, zw)
                assert accept_bits(again, got) == "", (r["id"], family, tag, "second run")
    assert exact >= 1, r["id"]
    return want_route


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r["id"] for r in ROWS])
def test_route_and_values(ctx, r):
    from lele_amd import kernels as K
    cus = K.num_cus(ctx)
    print("%d CUs, N = %d: %s" % (cus, batch_of(r, cus), check_codes_row(K, ctx, r, cus)))


@pytest.mark.gpu
def test_largest_k_of_the_i8_guard_and_its_neighbour(ctx):
    """K = 33025 at the four corner zero points on blocks of extreme codes: the epilogue's partial sums pass 2^31 (asserted on the CPU
    in test_row_inputs_tell_wrong_kernels_apart), the result does not.  K = 33026 takes the f32 route"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    cus = K.num_cus(ctx)
    for tag, x, w, zx, zw in cases(KBOUND, "extreme", cus):
        got, route = call(K, ctx, KBOUND, x, Weight(w), zx, zw)
        assert route == route_of(KBOUND, cus) == KBOUND["route"], route
        msg = accept_bits(got, exact_ref(x, w, zx, zw, KBOUND))
        print("K = 33025, %s: %s (|result| up to %.4g)" % (tag, msg or "equal", float(np.abs(got).max())))
        assert msg == "", (tag, msg)
    rng = np.random.default_rng(5)
    r = KBEYOND
    x, w = codes(rng, (1, r["C"], r["H"], r["W"])), codes(rng, (r["OC"], r["C"]) + r["k"])
    got, route = call(K, ctx, r, x, Weight(w), 128.0, 128.0)
    assert route.startswith("ci.f32/"), route
    assert not is_exact(x, 128.0, w, 128.0)
    msg = accept_close(got, oracle_ref(x, w, 128.0, 128.0, r))
    assert msg == "", msg
    assert accept_close(got, exact_ref(x, w, 128.0, 128.0, r)) == ""


SMALL = row("small", "ci8.nj1_ksplit", C=5, OC=8, H=9, W=11, N=1)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [3.5, -1.0, 256.0])
def test_weights_that_are_not_u8_codes_take_the_f32_route_and_the_verdict_is_remembered(ctx, value):
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(11)
    x, w = codes(rng, (1, 5, 9, 11)), codes(rng, (8, 5, 3, 3))
    w[3, 2, 1, 1] = value
    wt = Weight(w)
    first, route1 = call(K, ctx, SMALL, x, wt, 7.0, 3.0)
    second, route2 = call(K, ctx, SMALL, x, wt, 7.0, 3.0)
    assert route1.startswith("ci.f32/") and route2 == route1, (route1, route2)
    assert accept_bits(second, first) == ""
    assert is_exact(x, 7.0, w, 3.0)
    assert accept_bits(first, oracle_ref(x, w, 7.0, 3.0, SMALL)) == ""
    if value == int(value):
        assert accept_bits(first, exact_ref(x, w, 7.0, 3.0, SMALL)) == ""
    # the same values as codes: the i8 route, so the verdict above was the weights' and not the shape's
    w2 = w.copy()
    w2[3, 2, 1, 1] = 4.0
    got, route = call(K, ctx, SMALL, x, Weight(w2), 7.0, 3.0)
    assert route == "ci8.codes/ci8.nj1_ksplit" and accept_bits(got, exact_ref(x, w2, 7.0, 3.0, SMALL)) == ""


@pytest.mark.gpu
def test_mutable_and_device_resident_weights(ctx):
    """a plain host array is packed anew on every call (nothing cached); a device-resident one cannot be scanned: the f32 route"""
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    rng = np.random.default_rng(12)
    x, w = codes(rng, (1, 5, 9, 11)), codes(rng, (8, 5, 3, 3))
    got, route = call(K, ctx, SMALL, x, w, 9.0, 200.0)
    assert route == "ci8.codes/ci8.nj1_ksplit" and accept_bits(got, exact_ref(x, w, 9.0, 200.0, SMALL)) == ""
    before = exact_ref(x, w, 9.0, 200.0, SMALL)
    w[:] = 255.0 - w          # the same array, other values
    got, route = call(K, ctx, SMALL, x, w, 9.0, 200.0)
    after = exact_ref(x, w, 9.0, 200.0, SMALL)
    assert accept_bits(after, before) != "" and route == "ci8.codes/ci8.nj1_ksplit"
    assert accept_bits(got, after) == ""
    w[0, 0, 0, 0] = 0.5       # and no longer codes: this call's route, not a remembered one
    got, route = call(K, ctx, SMALL, x, w, 9.0, 200.0)
    assert route.startswith("ci.f32/") and accept_bits(got, oracle_ref(x, w, 9.0, 200.0, SMALL)) == ""
    w[0, 0, 0, 0] = 1.0
    got, route = call(K, ctx, SMALL, x, w, 9.0, 200.0)
    assert route == "ci8.codes/ci8.nj1_ksplit" and accept_bits(got, exact_ref(x, w, 9.0, 200.0, SMALL)) == ""
    got, route = call(K, ctx, SMALL, x, TensorView(ctx.buf().upload(w)), 9.0, 200.0)
    assert route.startswith("ci.f32/"), route
    assert is_exact(x, 9.0, w, 200.0) and accept_bits(got, oracle_ref(x, w, 9.0, 200.0, SMALL)) == ""


def quant_ref(srcs, w, zw, r):
    s, z = npref.dql_params(srcs)
    q = np.concatenate([npref.dql_quantize(a, s, z) for a in srcs], 1)
    return s, z, q, exact_ref(q, w, float(z), zw, r)


def check_quant(K, ctx, r, srcs, w, zw, want_route, multi, dirty):
    from lele_amd._lib import Weight
    from lele_amd.tensor import TensorView
    s, z, q, want = quant_ref(srcs, w, zw, r)
    wt = Weight(w)
    outs = []
    for _ in range(2):   # twice: integer atomics and (where K is split) the LDS meeting order give the same bits
        if dirty:
            dirty_arena(K, ctx, r, srcs[0].shape[0])
        ins = [TensorView(ctx.buf().upload(a)) for a in srcs] if dirty else srcs
        stale(K, ctx)
        if multi:
            out, sc = K.conv_integer_from_f32_multi(ins, wt, zp(zw), ctx=ctx)
        else:
            out, sc = K.conv_integer_from_f32(ins[0], wt, zp(zw), list(r["dil"]), 1, list(r["pads"]), list(r["strides"]), ctx=ctx)
        assert K.last_route(ctx) == want_route, (r["id"], K.last_route(ctx))
        assert accept_bits(sc.numpy(), np.array([s], np.float32)) == "", r["id"]
        outs.append(out.numpy().copy())
    msg = accept_bits(outs[0], want)
    assert msg == "", (r["id"], msg)
    assert accept_bits(outs[1], outs[0]) == "", (r["id"], "second run")
    if is_exact(q, float(z), w, zw):
        assert accept_bits(outs[0], oracle_ref(q, w, float(z), zw, r)) == "", (r["id"], "against the oracle")
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("r", QUANT_ROWS + MULTI_ROWS, ids=[r["id"] for r in QUANT_ROWS + MULTI_ROWS])
def test_from_f32_route_and_values(ctx, r):
    from lele_amd import kernels as K
    cus = K.num_cus(ctx)
    want_route = route_of(r, cus)
    assert want_route == r["route"]
    n = batch_of(r, cus)
    multi = r["id"] in MULTI_SOURCES
    chans = MULTI_SOURCES.get(r["id"], (r["C"],))
    rng = np.random.default_rng([IDS.index(r["id"]), 9])
    w = codes(rng, (r["OC"], r["C"]) + r["k"])
    for kind, zw, dirty in (("random", 128.0, False), ("ties", 113.0, False), ("random", 0.0, True)):
        if kind == "ties":
            whole = f32_source(rng, (n, r["C"], r["H"], r["W"]), kind)
            srcs = [np.ascontiguousarray(a) for a in np.split(whole, np.cumsum(chans)[:-1], axis=1)]
        else:   # sources of different ranges: the joint range decides
            srcs = [f32_source(rng, (n, c, r["H"], r["W"]), kind) * np.float32(1 + i) + np.float32(i) for i, c in enumerate(chans)]
        z = check_quant(K, ctx, r, srcs, w, zw, want_route, multi, dirty)
        if kind == "ties":
            s, z2 = npref.dql_params(srcs)
            assert (s, z2) == (np.float32(1 / 16), np.float32(128)) and z == z2
    print("%d CUs, N = %d: %s" % (cus, n, want_route))


@pytest.mark.gpu
def test_empty_results_report_no_route(ctx):
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(13)
    for n, oc in ((0, 8), (2, 0)):
        x, w = codes(rng, (n, 5, 9, 11)), codes(rng, (oc, 5, 3, 3))
        got, route = call(K, ctx, SMALL, x, Weight(w) if oc else w, 7.0, 3.0)
        assert route == "" and got.shape == (n, oc, 9, 11), (route, got.shape)
    stale(K, ctx)
    out = K.fused_scale_bias(np.zeros((0, 5, 4, 6), np.float32), 0.5, np.zeros(5, np.float32), ctx=ctx)
    assert K.last_route(ctx) == "" and tuple(out.shape) == (0, 5, 4, 6)


@pytest.mark.gpu
def test_fused_scale_bias_route_and_values(ctx):
    """N = 3, C = 5 with a bias of length 7 (the first five are read): host scale, in place, device scale times scale_mul; the linear
    form bit for bit (one multiplication, one addition, not fused), the SiLU form at the bar of tests/test_conv_integer.py"""
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    rng = np.random.default_rng(14)
    data = (rng.integers(-2 ** 20, 2 ** 20, (3, 5, 4, 6))).astype(np.float32)
    data.reshape(-1)[:4] = [0.0, -0.0, 2.0 ** 31 - 128, -2.0 ** 31]
    bias = rng.standard_normal(7).astype(np.float32)
    scale = np.float32(0.02)
    want = npref.fused_scale_bias(data, scale, bias[:5])
    stale(K, ctx)
    got = K.fused_scale_bias(data, float(scale), bias, ctx=ctx).numpy()
    assert K.last_route(ctx) == "fsb.w1"
    assert accept_bits(got, want) == "", accept_bits(got, want)
    # in place: the result goes where the data was
    buf = ctx.buf()
    dev = TensorView(buf.upload(data))
    stale(K, ctx)
    got = K.fused_scale_bias(dev, float(scale), bias, out=buf, ctx=ctx).numpy().copy()
    assert K.last_route(ctx) == "fsb.w1" and accept_bits(got, want) == "", accept_bits(got, want)
    # the device scale of conv_integer_from_f32 times a weight scale
    sdev = TensorView(ctx.buf().upload(np.array([0.37], np.float32)))
    eff = np.float32(np.float32(0.37) * np.float32(0.02))
    stale(K, ctx)
    got = K.fused_scale_bias(data, sdev, bias, scale_mul=0.02, ctx=ctx).numpy()
    assert K.last_route(ctx) == "fsb.w1"
    assert accept_bits(got, npref.fused_scale_bias(data, eff, bias[:5])) == ""
    small = (data / np.float32(2 ** 14)).astype(np.float32)
    small.reshape(-1)[:4] = [0.0, -0.0, 64.0, -64.0]
    stale(K, ctx)
    got = K.fused_scale_bias_silu(small, sdev, bias, scale_mul=0.02, ctx=ctx).numpy()
    assert K.last_route(ctx) == "fsb.w1"
    assert np.abs(got - npref.fused_scale_bias(small, eff, bias[:5], True)).max() <= 1e-5 * max(1.0, np.abs(got).max())
