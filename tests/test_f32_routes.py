"""Every f32 GEMM and convolution route against a float64 reference, one table row per dispatch branch.

Each case carries the route the library must report (kernels.last_route(): recorded at the launch site, levels joined by '/'), so a
re-tune that moves a shape to another kernel fails here instead of silently leaving that kernel untested.  Two checks per case:

1. Values, against a plain numpy float64 reference (a matrix product; a per-tap tensordot for convolutions):
   * the project bar, parity.close_f32 at 1e-4;
   * a magnitude bound |got - ref| <= c * S with S = |W| (*) |X| + |b| (the same operation on absolute values).
   Derivation of c.  Every route forms each output as a sum of at most K products plus the bias, accumulated in f32 (u = 2^-24):
   a recursive sum of n terms carries at most (n - 1) u sum|t_i| of rounding error whatever the order (Higham, Accuracy and
   Stability, 4.2), and the re-associations the kernels use (split K, LDS passes, a butterfly) are sums of the same kind.  With the
   product itself rounded once: c_f32 = (K + 2) u.  The split-bf16 window kernels (three round-to-nearest bf16 pieces a value, six
   of the nine piece products kept) drop m l + l m + l l <= 3 * 2^-9 * 2^-18 |w x| < 2^-25 |w x| per product and add no rounding of
   their own beyond the f32 accumulation, so c_bf16 = (K + 2) u + 2^-25.  ReLU is exact and 1-Lipschitz, so the bound carries over;
   SiLU (|silu'| <= 1.1) adds its own evaluation error, pinned elsewhere at 1e-5 relative + 1e-7 (test_conv_rnn.py):
   |got - silu(ref)| <= 1.1 c S + 1e-5 |silu(ref)| + 1e-7.
   The table keeps K <= 160, so c <= 9.7e-6, except where the route itself needs more (the direct kernel's several LDS passes at
   stride 1 take at least 27 input channels, K = 243).  In the first half of every input (rows of an image or of A, columns of B)
   a tenth of the values is spread over 2^-40 .. 2^40, so one window holds magnitudes far apart: a dropped middle or low bf16 piece
   shows as an error of 2^-9 or 2^-18 of a large term.  The other half keeps windows without them, where a bias or an edge tap is
   large against c * S.
2. NaN receptive field, exactly.  NaN at inputs where routes change hands (first / last rows and columns, both sides of 8-row,
   32-column and 256-position tile edges, channels 15 / 16 and the last one, the last image; for GEMM the last k of a K tile, A row
   M - 1, B column N - 1).  The set of outputs that must be NaN is built with integer arithmetic from stride, padding, dilation and
   groups; exactly those are NaN and every other output is finite.  For channel views the gaps of the input's pitch are NaN too.

CPU part: the table's labels name every route the library can report, and every case's tolerance rejects emulated wrong variants
(the last k dropped, the last input channel dropped, the right / bottom edge shifted by one, the bias missing on the last block of
output channels) computed in numpy on the same inputs."""
import re

import numpy as np
import pytest

from tests.parity import close_f32

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the table
def G(label, op, m, k, n, batch=(), ta=False, tb=False, c=None, alpha=1.0, beta=1.0, bcast_b=False, view=None):
    """a GEMM case: op in matmul / fused_add / gemm / view; c = C mode (full, row, col, scalar, modulo) for gemm / fused_add"""
    return dict(kind="gemm", label=label, op=op, m=m, k=k, n=n, batch=tuple(batch), ta=ta, tb=tb, c=c, alpha=alpha, beta=beta,
                bcast_b=bcast_b, view=view)


def CV(label, n, c, h, w, oc, kh, kw, group=1, pads=(0, 0, 0, 0), strides=(1, 1), dil=(1, 1), act="none", bias=True, res=False,
       views=False, bf16=False):
    return dict(kind="conv", label=label, n=n, c=c, h=h, w=w, oc=oc, kh=kh, kw=kw, group=group, pads=tuple(pads), strides=tuple(strides),
                dil=tuple(dil), act=act, bias=bias, res=res, views=views, bf16=bf16)


def CT(label, n, c, h, w, oc, kh, kw, strides, pads=(0, 0, 0, 0), bias=True):
    return dict(kind="convt", label=label, n=n, c=c, h=h, w=w, oc=oc, kh=kh, kw=kw, strides=tuple(strides), pads=tuple(pads), bias=bias)


def CI(label, n, c, h, w, oc, k, group, pads, zx, zw):
    return dict(kind="ci", label=label, n=n, c=c, h=h, w=w, oc=oc, kh=k, kw=k, group=group, pads=tuple(pads), zx=zx, zw=zw)


P1 = (1, 1, 1, 1)
CASES = [
    # ---- GEMM: the thin kernels (thin_m needs a k-contiguous B: gemm with trans_b only)
    G("gemm.thin_n", "matmul", 300, 37, 3),
    G("gemm.thin_m", "gemm", 3, 45, 700, tb=True, c="row"),
    # the small (split-K) kernel with each transposition pair, and every C mode
    G("gemm.small", "gemm", 200, 31, 300, c="full", alpha=0.75, beta=-1.5),
    G("gemm.small", "gemm", 200, 17, 301, ta=True, c="row"),
    G("gemm.small", "gemm", 199, 47, 300, tb=True, c="col"),
    G("gemm.small", "gemm", 201, 33, 299, ta=True, tb=True, c="scalar"),
    G("gemm.small", "gemm", 130, 20, 70, c="modulo"),
    G("gemm.small", "fused_add", 150, 40, 96, c="row"),
    G("gemm.small", "fused_add", 150, 40, 96, c="modulo"),
    G("gemm.small", "matmul", 100, 63, 130, batch=(3,), bcast_b=True),
    # the tiled kernels: each tile shape, the four transposition pairs, K < 16 / 17 / 31 (K % 16 = 15), ragged last tiles, N % 4 != 0
    G("gemm.tile64x64", "gemm", 1531, 17, 1538, c="full"),
    G("gemm.tile64x64", "gemm", 1536, 31, 1530, ta=True, c="col"),
    G("gemm.tile64x64", "gemm", 1529, 9, 1536, tb=True, c="scalar"),
    G("gemm.tile64x64", "gemm", 1540, 47, 1535, ta=True, tb=True, c="modulo"),
    G("gemm.tile32x128", "matmul", 96, 17, 6142, batch=(4,)),
    G("gemm.tile128x128", "matmul", 1023, 15, 4097, batch=(3,), bcast_b=True),
    G("gemm.tile64x256", "fused_add", 288, 18, 6144, batch=(4,), c="row"),
    G("gemm.tile256x128", "matmul", 4000, 7, 4100),
    # matmul_view: a base off the 16-byte grid (scalar loads), strided two-level-batch output, on a tiled kernel
    G("gemm.tile64x64", "view", 1536, 20, 1536, view="offset"),
    G("gemm.tile64x64", "view", 640, 17, 643, batch=(2, 3), view="perm"),
    # ---- conv2d, depthwise: each KW on the LDS form (with and without the direct store), the row form, the generic form
    CV("conv.dw_lds_k3", 2, 32, 20, 18, 32, 3, 3, 32, P1, act="silu"),
    CV("conv.dw_lds_k3_direct", 2, 32, 20, 20, 32, 3, 3, 32, (1, 0, 1, 2), act="relu", bias=False),
    CV("conv.dw_lds_k5", 2, 24, 21, 19, 24, 5, 5, 24, (2, 2, 2, 2)),
    CV("conv.dw_lds_k5_direct", 2, 24, 16, 16, 24, 5, 5, 24, (2, 2, 2, 2), act="silu"),
    CV("conv.dw_lds_k7", 1, 40, 23, 22, 40, 7, 7, 40, (3, 3, 3, 3), act="relu"),
    CV("conv.dw_lds_k7_direct", 1, 40, 24, 24, 40, 7, 7, 40, (3, 3, 3, 3), bias=False),
    CV("conv.dw_lds_k11", 1, 16, 30, 27, 16, 11, 11, 16, (5, 5, 5, 5), act="silu"),
    CV("conv.dw_lds_k11_direct", 1, 16, 28, 28, 16, 11, 11, 16, (5, 5, 5, 5)),
    CV("conv.dw_row4_k3", 1, 8, 130, 130, 8, 3, 3, 8, P1, act="silu"),
    CV("conv.dw_row4_k5", 1, 8, 130, 131, 8, 5, 5, 8, (2, 2, 2, 2), act="relu"),
    CV("conv.dw_row4_k7", 1, 8, 131, 130, 8, 7, 7, 8, (3, 3, 3, 3), bias=False),
    CV("conv.dw_row4_k11", 1, 8, 130, 130, 8, 11, 11, 8, (5, 5, 5, 5)),
    CV("conv.dw_generic", 2, 16, 33, 31, 16, 3, 3, 16, P1, strides=(2, 2), act="silu"),
    CV("conv.dw_generic", 2, 16, 20, 21, 16, 3, 3, 16, (2, 2, 2, 2), dil=(2, 2), act="relu"),
    CV("conv.dw_lds_k3_direct", 2, 32, 20, 20, 32, 3, 3, 32, P1, act="silu", res=True),
    # ---- the window kernel (split-bf16), stride 1: 3 x 3 and 1 x 1, each block width with and without osplit; the narrow 5-16 channels
    CV("conv.win3_oct32", 32, 16, 40, 44, 32, 3, 3, 1, P1, act="silu", bf16=True),
    CV("conv.win3_oct32_osplit", 32, 16, 40, 44, 64, 3, 3, 1, (1, 0, 1, 2), act="relu", bf16=True),
    CV("conv.win3_oct64", 128, 16, 24, 40, 64, 3, 3, 1, P1, bf16=True),
    CV("conv.win3_oct64_osplit", 48, 16, 40, 44, 128, 3, 3, 1, P1, act="silu", bias=False, bf16=True),
    CV("conv.win3_oct32", 48, 16, 48, 48, 8, 3, 3, 1, P1, act="silu", bf16=True),
    CV("conv.win1_oct32", 32, 32, 40, 40, 32, 1, 1, act="relu", bf16=True),
    CV("conv.win1_oct32", 32, 32, 40, 40, 8, 1, 1, act="silu", bf16=True),
    CV("conv.win1_oct32_osplit", 32, 32, 40, 40, 64, 1, 1, bf16=True),
    CV("conv.win1_oct64", 80, 32, 40, 40, 64, 1, 1, act="silu", bf16=True),
    CV("conv.win1_oct64_osplit", 38, 32, 40, 40, 128, 1, 1, act="relu", bf16=True),
    CV("conv.win1_oct128", 40, 32, 40, 40, 128, 1, 1, bias=False, bf16=True),
    CV("conv.win1_oct128_osplit", 20, 32, 40, 40, 256, 1, 1, act="silu", bf16=True),
    CV("conv.win3_oct32", 32, 16, 40, 44, 32, 3, 3, 1, P1, act="silu", res=True, views=True, bf16=True),
    CV("conv.win1_oct32", 32, 32, 40, 40, 32, 1, 1, act="relu", views=True, bf16=True),
    # ---- the stride-2 window kernel, odd and even maps
    CV("conv.win3s2_oct64", 48, 16, 80, 80, 64, 3, 3, 1, P1, strides=(2, 2), act="silu", bf16=True),
    CV("conv.win3s2_oct64_osplit", 24, 16, 81, 79, 128, 3, 3, 1, P1, strides=(2, 2), act="relu", bf16=True),
    CV("conv.win3s2_oct32", 48, 16, 79, 80, 32, 3, 3, 1, (0, 1, 1, 0), strides=(2, 2), bf16=True),
    CV("conv.win3s2_oct32_osplit", 24, 16, 80, 80, 96, 3, 3, 1, P1, strides=(2, 2), act="silu", bias=False, bf16=True),
    # ---- the direct kernel (few output channels): ocb 8 / 16, stride 1 / 2, one LDS pass or several
    CV("conv.direct_ocb8_s1", 48, 8, 48, 48, 8, 3, 3, 1, P1, act="silu"),
    CV("conv.direct_ocb16_s1", 90, 8, 37, 45, 13, 3, 3, 1, (0, 2, 1, 0), act="relu"),
    CV("conv.direct_ocb8_s1_passes", 128, 27, 32, 32, 6, 3, 3, 1, P1),
    CV("conv.direct_ocb16_s1_passes", 128, 27, 32, 33, 12, 3, 3, 1, (1, 1, 0, 1), act="silu", bias=False),
    CV("conv.direct_ocb8_s2", 64, 3, 70, 66, 8, 3, 3, 1, P1, strides=(2, 2), act="silu"),
    CV("conv.direct_ocb16_s2", 64, 3, 70, 66, 16, 3, 3, 1, P1, strides=(2, 2), act="relu"),
    CV("conv.direct_ocb8_s2_passes", 176, 12, 40, 36, 5, 3, 3, 1, (1, 0, 1, 2), strides=(2, 2)),
    CV("conv.direct_ocb16_s2_passes", 176, 12, 40, 37, 16, 3, 3, 1, P1, strides=(2, 2), act="silu"),
    CV("conv.direct_ocb8_s1", 48, 8, 48, 48, 8, 3, 3, 1, P1, act="relu", res=True, views=True),
    # ---- the implicit GEMM: pointwise, tap-major K, generic im2col
    CV("conv.gemm_pw/gemm.small", 4, 24, 20, 20, 40, 1, 1, act="silu"),
    CV("conv.gemm_pw/gemm.tile128x128", 64, 24, 20, 20, 200, 1, 1, act="relu", views=True),
    CV("conv.gemm_tap/gemm.small", 8, 12, 12, 12, 200, 3, 3, 1, P1),
    CV("conv.gemm_tap/gemm.tile64x64", 32, 12, 24, 24, 96, 3, 3, 1, (1, 0, 1, 2), act="silu", res=True),
    CV("conv.gemm_tap/gemm.small", 1, 16, 33, 29, 24, 5, 3, 2, (2, 1, 0, 3), strides=(2, 1), dil=(1, 2), act="relu"),
    CV("conv.gemm_generic/gemm.small", 2, 6, 33, 29, 24, 5, 3, 2, (2, 1, 0, 3), strides=(2, 1), dil=(1, 2), act="silu"),
    CV("conv.gemm_generic/gemm.small", 3, 3, 30, 30, 20, 3, 3, 1, P1, bias=False),
    # ---- conv_transpose: kernel == stride (one GEMM), the phase route, a phase no tap reaches (bias only)
    CT("convt.ks/gemm.small", 2, 16, 10, 12, 8, 2, 2, (2, 2)),
    CT("convt.phase", 2, 8, 7, 9, 6, 3, 3, (2, 2), (1, 1, 1, 1)),
    CT("convt.phase_fill", 2, 8, 6, 7, 5, 2, 2, (3, 3)),
    # ---- conv_integer's f32 form (grouped): the codes centred, then the f32 convolution
    CI("ci.f32/conv.gemm_tap/gemm.small", 2, 8, 12, 13, 16, 3, 2, P1, 3.0, 128.0),
]


def case_id(i, case):
    return "%d-%s" % (i, case["label"].replace("/", "+"))


def k_of(case):
    if case["kind"] == "gemm":
        return case["k"]
    if case["kind"] == "convt":
        return case["c"] * -(-case["kh"] // case["strides"][0]) * -(-case["kw"] // case["strides"][1])
    return case["c"] // case["group"] * case["kh"] * case["kw"]


def c_of(case):
    return (k_of(case) + 2) * U + (2.0 ** -25 if case.get("bf16") else 0.0)


# ------------------------------------------------------------------------------------------------------------ inputs
def spread(rng, shape, scale=1.0, axis=-2):
    """standard normal values; in the first half along `axis` (rows of a matrix or an image, columns of a B operand) a tenth of
    them scaled by 2^e with e uniform in [-40, 40].  The other half keeps every window free of them, where a small term (a bias,
    an edge tap) stays visible against c * S."""
    v = rng.standard_normal(shape) * scale
    idx = np.arange(shape[axis]).reshape((-1,) + (1,) * (-axis - 1))
    pick = (rng.random(shape) < 0.1) & (idx < shape[axis] // 2)
    v[pick] *= 2.0 ** rng.integers(-40, 41, int(pick.sum()))
    return v.astype(np.float32)


def conv_geom(case):
    pt, pl, pb, pr = case["pads"]
    sh, sw = case["strides"]
    dh, dw = case["dil"]
    oh = (case["h"] + pt + pb - dh * (case["kh"] - 1) - 1) // sh + 1
    ow = (case["w"] + pl + pr - dw * (case["kw"] - 1) - 1) // sw + 1
    return oh, ow


def convt_geom(case):
    pt, pl, pb, pr = case["pads"]
    sh, sw = case["strides"]
    return (case["h"] - 1) * sh - pt - pb + case["kh"], (case["w"] - 1) * sw - pl - pr + case["kw"]


def make_inputs(i, case):
    rng = np.random.default_rng(1000 + i)
    kind = case["kind"]
    if kind == "gemm":
        m, k, n, batch = case["m"], case["k"], case["n"], case["batch"]
        a = spread(rng, batch + (m, k))
        b = spread(rng, (() if case["bcast_b"] else batch) + (k, n), 0.5, axis=-1)
        cm = case["c"]
        clen = {None: 0, "full": m * n, "row": n, "col": m, "scalar": 1, "modulo": 37}[cm]
        c = (rng.standard_normal(clen) * 4).astype(np.float32) if clen else None
        return dict(a=a, b=b, c=c)
    if kind == "convt":
        x = spread(rng, (case["n"], case["c"], case["h"], case["w"]))
        w = (rng.standard_normal((case["c"], case["oc"], case["kh"], case["kw"])) * 0.3).astype(np.float32)
        b = (rng.standard_normal(case["oc"]) * 2).astype(np.float32) if case["bias"] else None
        return dict(x=x, w=w, b=b)
    if kind == "ci":
        x = rng.integers(0, 256, (case["n"], case["c"], case["h"], case["w"])).astype(np.float32)
        w = rng.integers(0, 256, (case["oc"], case["c"] // case["group"], case["kh"], case["kw"])).astype(np.float32)
        return dict(x=x, w=w, b=None)
    x = spread(rng, (case["n"], case["c"], case["h"], case["w"]))
    w = (rng.standard_normal((case["oc"], case["c"] // case["group"], case["kh"], case["kw"])) * 0.3).astype(np.float32)
    b = (rng.standard_normal(case["oc"]) * 2).astype(np.float32) if case["bias"] else None
    oh, ow = conv_geom(case)
    r = rng.standard_normal((case["n"], case["oc"], oh, ow)).astype(np.float32) if case["res"] else None
    return dict(x=x, w=w, b=b, r=r)


# --------------------------------------------------------------------------------------------------- float64 reference
def gemm_operands(case, inp):
    """logical A [.., M, K], B [.., K, N] in float64"""
    return inp["a"].astype(np.float64), inp["b"].astype(np.float64)


def gemm_c_term(case, inp, m, n, lead):
    """what the C operand / bias adds to the [lead.., M, N] product (float64)"""
    c = inp["c"]
    if c is None:
        return 0.0
    c = c.astype(np.float64)
    cm = case["c"]
    if cm == "full":
        t = c.reshape(m, n)
    elif cm == "row":
        t = c.reshape(1, n)
    elif cm == "col":
        t = c.reshape(m, 1)
    elif cm == "scalar":
        t = c.reshape(1, 1)
    else:
        total = int(np.prod(lead)) * m * n
        t = c[np.arange(total) % c.size].reshape(tuple(lead) + (m, n))
    return t * (case["beta"] if case["op"] == "gemm" else 1.0)


def conv_ref(x, w, b, case, absval=False):
    """float64 convolution as per-tap tensordots; absval: the same on |x|, |w|, |b| (the magnitude S of the bound)"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    if absval:
        x, w = np.abs(x), np.abs(w)
    n, c = x.shape[:2]
    oc, icg, kh, kw = w.shape
    g = c // icg
    ocg = oc // g
    pt, pl, pb, pr = case["pads"]
    sh, sw = case["strides"]
    dh, dw = case["dil"]
    oh, ow = conv_geom(case) if "dil" in case else None
    xp = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)))
    out = np.zeros((n, oc, oh, ow))
    for gi in range(g):
        xs_g = xp[:, gi * icg:(gi + 1) * icg]
        for i in range(kh):
            for j in range(kw):
                xs = xs_g[:, :, i * dh:i * dh + sh * (oh - 1) + 1:sh, j * dw:j * dw + sw * (ow - 1) + 1:sw]
                out[:, gi * ocg:(gi + 1) * ocg] += np.tensordot(w[gi * ocg:(gi + 1) * ocg, :, i, j], xs, axes=([1], [1])).transpose(1, 0, 2, 3)
    if b is not None:
        out += (np.abs(b) if absval else b).astype(np.float64).reshape(1, oc, 1, 1)
    return out


def convt_ref(x, w, b, case, absval=False):
    x, w = x.astype(np.float64), w.astype(np.float64)
    if absval:
        x, w = np.abs(x), np.abs(w)
    n, c, ih, iw = x.shape
    oc, kh, kw = w.shape[1:]
    sh, sw = case["strides"]
    pt, pl = case["pads"][:2]
    oh, ow = convt_geom(case)
    full = np.zeros((n, oc, (ih - 1) * sh + kh, (iw - 1) * sw + kw))
    for i in range(kh):
        for j in range(kw):
            full[:, :, i:i + sh * (ih - 1) + 1:sh, j:j + sw * (iw - 1) + 1:sw] += np.tensordot(w[:, :, i, j], x, axes=([0], [1])).transpose(1, 0, 2, 3)
    out = full[:, :, pt:pt + oh, pl:pl + ow]
    if b is not None:
        out = out + (np.abs(b) if absval else b).astype(np.float64).reshape(1, oc, 1, 1)
    return out


def ci_operands(case, inp):
    pt, pl, pb, pr = case["pads"]
    x = np.pad(inp["x"].astype(np.float64), ((0, 0), (0, 0), (pt, pb), (pl, pr))) - case["zx"]
    return x, inp["w"].astype(np.float64) - case["zw"]


def reference(case, inp):
    """(ref, S): the float64 result before the activation, and the magnitude |W| (*) |X| + |b| (+ |res|)"""
    kind = case["kind"]
    if kind == "gemm":
        a, b = gemm_operands(case, inp)
        m, n = case["m"], case["n"]
        lead = case["batch"]
        alpha = case["alpha"] if case["op"] == "gemm" else 1.0
        ref = alpha * np.matmul(a, b) + gemm_c_term(case, inp, m, n, lead)
        mag = abs(alpha) * np.matmul(np.abs(a), np.abs(b)) + np.abs(gemm_c_term(case, inp, m, n, lead))
        return ref, mag
    if kind == "convt":
        return convt_ref(inp["x"], inp["w"], inp["b"], case), convt_ref(inp["x"], inp["w"], inp["b"], case, True)
    if kind == "ci":
        x, w = ci_operands(case, inp)
        cz = dict(case, pads=(0, 0, 0, 0), strides=(1, 1), dil=(1, 1), h=x.shape[2], w=x.shape[3])
        return conv_ref(x, w, None, cz), conv_ref(x, w, None, cz, True)
    return conv_ref(inp["x"], inp["w"], inp["b"], case), conv_ref(inp["x"], inp["w"], inp["b"], case, True)


def activate(case, v):
    act = case.get("act", "none")
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "silu":
        with np.errstate(over="ignore"):
            return v / (1.0 + np.exp(-v))
    return v


def finish(case, inp, pre):
    out = activate(case, pre)
    if case.get("res"):
        out = out + inp["r"].astype(np.float64)
    return out


def accepts(case, inp, got, ref, mag):
    """the tolerance of check 1: close_f32 at 1e-4 and the magnitude bound (module docstring).  (ok, message)"""
    want = finish(case, inp, ref)
    got = np.asarray(got, np.float64)
    try:
        close_f32(got, want, 1e-4, case["label"])
    except AssertionError as e:
        return False, str(e)
    c = c_of(case)
    if case.get("act") == "silu":
        lim = 1.1 * c * mag + 1e-5 * np.abs(want) + 1e-7
    else:
        lim = c * mag
    if case.get("res"):
        lim = lim + U * np.abs(want)   # the residual's own addition, rounded once
    err = np.abs(got - want)
    bad = ~(err <= lim)
    if bad.any():
        idx = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(lim, 1e-300), 0))), err.shape)
        return False, "%s: %d of %d outside c * S (c = %.3g); worst at %s: got %r want %r S %r" % (
            case["label"], int(bad.sum()), bad.size, c, idx, got[idx], want[idx], mag[idx])
    return True, ""


# --------------------------------------------------------------------------------------------------------- NaN positions
def conv_nan_inputs(case):
    """input positions (img, ch, y, x) that get a NaN: edges, tile edges, channels 15 / 16 / last, the last image"""
    n, c, h, w = case["n"], case["c"], case["h"], case["w"]
    pos = [(n - 1, 0, 0, 0), (0, c - 1, h - 1, w - 1), (0, min(15, c - 1), min(7, h - 1), min(31, w - 1)),
           (n - 1, min(16, c - 1), min(8, h - 1), min(32, w - 1)), (0, c // 2, 255 // w if 255 // w < h else h // 2, 255 % w),
           (n - 1, c - 1, min(256 // w, h - 1), 256 % w), (0, 0, h // 2, w - 1), (n - 1, c // 3, h - 1, 0)]
    return sorted(set(pos))


def axis_hits(p, pad, k, s, d, o):
    """output indices along one axis whose window reads input index p (forward convolution)"""
    out = []
    for t in range(k):
        q = p + pad - t * d
        if q % s == 0 and 0 <= q // s < o:
            out.append(q // s)
    return out


def conv_nan_expected(case, pos):
    oh, ow = conv_geom(case)
    icg, ocg = case["c"] // case["group"], case["oc"] // case["group"]
    pt, pl = case["pads"][:2]
    sh, sw = case["strides"]
    dh, dw = case["dil"]
    mask = np.zeros((case["n"], case["oc"], oh, ow), bool)
    for (img, ch, y, x) in pos:
        g = ch // icg
        ys, xs = axis_hits(y, pt, case["kh"], sh, dh, oh), axis_hits(x, pl, case["kw"], sw, dw, ow)
        for oy in ys:
            mask[img, g * ocg:(g + 1) * ocg, oy, xs] = True
    return mask


def convt_nan_expected(case, pos):
    oh, ow = convt_geom(case)
    pt, pl = case["pads"][:2]
    sh, sw = case["strides"]
    mask = np.zeros((case["n"], case["oc"], oh, ow), bool)
    for (img, ch, y, x) in pos:
        ys = [y * sh - pt + t for t in range(case["kh"]) if 0 <= y * sh - pt + t < oh]
        xs = [x * sw - pl + t for t in range(case["kw"]) if 0 <= x * sw - pl + t < ow]
        for oy in ys:
            mask[img, :, oy, xs] = True
    return mask


def gemm_nan_inputs(case):
    """(a positions, b positions) in the logical [.., M, K] / [.., K, N] operands"""
    m, k, n = case["m"], case["k"], case["n"]
    lb = case["batch"]
    last = tuple(x - 1 for x in lb)
    first = tuple(0 for _ in lb)
    a_pos = [first + (min(m // 2, m - 1), min(15, k - 1)), last + (m - 1, 0), first + (min(31, m - 1), k - 1)]
    bl = () if case["bcast_b"] else last
    b_pos = [bl + (k // 2, n - 1), (() if case["bcast_b"] else first) + (min(16, k - 1), min(256, n - 1))]
    return a_pos, b_pos


def gemm_nan_expected(case, a_pos, b_pos):
    m, n, lb = case["m"], case["n"], case["batch"]
    mask = np.zeros(lb + (m, n), bool)
    for p in a_pos:
        mask[p[:-2] + (p[-2],)] = True
    for p in b_pos:
        if case["bcast_b"]:
            mask[..., p[-1]] = True
        else:
            mask[p[:-2] + (Ellipsis, p[-1])] = True
    return mask


# ---------------------------------------------------------------------------------------------------------------- running
def run(ctx, case, inp):
    """the library's result for the case (numpy)"""
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    kind = case["kind"]
    if kind == "gemm":
        a, b, c = inp["a"], inp["b"], inp["c"]
        op = case["op"]
        if op == "matmul":
            return K.matmul(a, b, ctx=ctx).numpy()
        if op == "fused_add":
            return K.matmul_fused_add(a, b, c, ctx=ctx).numpy()
        if op == "gemm":
            aa = np.ascontiguousarray(a.T) if case["ta"] else a
            bb = np.ascontiguousarray(b.T) if case["tb"] else b
            return K.gemm(aa, bb, c, case["alpha"], case["beta"] if c is not None else 0.0, case["ta"], case["tb"], ctx=ctx).numpy()
        if case["view"] == "offset":   # A = columns [1, K + 1) of a wider tensor whose column 0 is NaN (never read)
            wide = np.full(a.shape[:-1] + (a.shape[-1] + 1,), np.nan, np.float32)
            wide[..., 1:] = a
            return K.matmul_view(wide, [["slice", 1, 1, a.shape[-1]]], b, [], ctx=ctx).numpy()
        # "perm": the product [B0, B1, M, N] stored as [B0, M, B1, N] (rows strided, two-level batch), then read back in order
        got = K.matmul_view(a, [], b, [], out_perm=[0, 2, 1, 3], ctx=ctx).numpy()
        return got.transpose(0, 2, 1, 3)
    if kind == "convt":
        return K.conv_transpose(inp["x"], inp["w"], inp["b"], [1, 1], 1, list(case["pads"]), list(case["strides"]), ctx=ctx).numpy()
    if kind == "ci":
        return K.conv_integer(inp["x"], inp["w"], np.array([case["zx"]], np.float32), np.array([case["zw"]], np.float32), [1, 1],
                              case["group"], list(case["pads"]), [1, 1], ctx=ctx).numpy()
    act = {"none": 0, "relu": 1, "silu": 2}[case["act"]]
    args = (list(case["dil"]), case["group"], list(case["pads"]), list(case["strides"]))
    x, w, b = inp["x"], inp["w"], inp["b"]
    n, c = x.shape[:2]
    oh, ow = conv_geom(case)
    oc = case["oc"]
    if case["views"]:
        # x = channels [3, 3 + C) of a wider tensor whose other channels are NaN; the result (and the residual) windows of others
        wide = np.full((n, c + 5) + x.shape[2:], np.nan, np.float32)
        wide[:, 3:3 + c] = x
        xv = TensorView(ctx.buf().upload(wide)).channels(3, 3 + c)
        tot = oc + 3
        big = ctx.buf()
        big.upload(np.full((n, tot, oh, ow), -3.25, np.float32))
        window = (1 * oh * ow, tot * oh * ow)
        if case["res"]:
            wr = np.full((n, oc + 4, oh, ow), np.nan, np.float32)
            wr[:, 2:2 + oc] = inp["r"]
            rv = TensorView(ctx.buf().upload(wr)).channels(2, 2 + oc)
            got = K.conv2d_res(xv, w, b, rv, *args, act=act, out=big, out_window=window, ctx=ctx).numpy()
        else:
            fn = {0: K.conv2d, 1: lambda *a_, **k_: K.conv2d_fused(*a_, relu=True, **k_), 2: K.conv2d_silu}[act]
            got = fn(xv, w, b, *args, out=big, out_window=window, ctx=ctx).numpy()
        whole = big.to_numpy((n, tot, oh, ow))
        assert np.all(whole[:, :1] == -3.25) and np.all(whole[:, 1 + oc:] == -3.25), "a store outside the output window"
        return got
    if case["res"]:
        return K.conv2d_res(x, w, b, inp["r"], *args, act=act, ctx=ctx).numpy()
    fn = {0: K.conv2d, 1: lambda *a_, **k_: K.conv2d_fused(*a_, relu=True, **k_), 2: K.conv2d_silu}[act]
    return fn(x, w, b, *args, ctx=ctx).numpy()


def with_nans(case, inp):
    """(inputs with NaN placed, expected NaN mask of the result)"""
    out = dict(inp)
    if case["kind"] == "gemm":
        a_pos, b_pos = gemm_nan_inputs(case)
        a, b = inp["a"].copy(), inp["b"].copy()
        for p in a_pos:
            a[p] = np.nan
        for p in b_pos:
            b[p] = np.nan
        out.update(a=a, b=b)
        return out, gemm_nan_expected(case, a_pos, b_pos)
    pos = conv_nan_inputs(case)
    x = inp["x"].copy()
    for p in pos:
        x[p] = np.nan
    out["x"] = x
    if case["kind"] == "convt":
        return out, convt_nan_expected(case, pos)
    if case["kind"] == "ci":
        cz = dict(case, strides=(1, 1), dil=(1, 1))
        return out, conv_nan_expected(cz, pos)
    return out, conv_nan_expected(case, pos)


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_labels_cover_every_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    used = {lvl for case in CASES for lvl in case["label"].split("/")}
    # the attn. names: tests/test_attention_routes.py; the data-movement names: tests/test_manip_routes.py -- the same two assertions
    theirs = ("attn.", "copy.", "resize.", "pool.", "topk.", "cpitch.", "pad.", "gather.", "apool.", "tcp.", "range.", "fill.", "cast.",
              "unary.", "bin.", "binp.", "where.", "clip.", "reduce.", "ln.", "softmax.", "rows.", "rms.", "bn.", "add3.", "hpas.",   # tests/test_eltwise_routes.py
              "rnn.", "rnns.",   # tests/test_rnn_routes.py
              "ci8.", "fsb.",   # tests/test_conv_integer_routes.py
              "fe.",   # tests/test_frontend_routes.py
              "q.", "qffn.", "mmi.", "dql.", "igemm.", "as.", "rs.",   # tests/test_quant_routes.py
              "resample.")   # tests/test_resample.py
    mine = {s for s in names if not s.startswith(theirs)}
    assert not used - mine, "labels the library cannot report: %s" % sorted(used - mine)
    assert not mine - used - {"gemm.k0"}, "routes no case reaches: %s" % sorted(mine - used)   # gemm.k0: test_empty_k


def test_tolerances_stay_within_the_derived_constant():
    for case in CASES:
        stride1_passes = case["label"].endswith("_s1_passes")   # >= 27 input channels: K = 243 is the smallest that reaches it
        assert c_of(case) <= (1e-5 if not stride1_passes else 250 * U), case["label"]


def probe(case, inp):
    """the inputs cut down to what the mutation check needs (first and last image / rows): a wrong variant rejected there is
    rejected on the whole case"""
    if case["kind"] == "gemm":
        out = dict(inp)
        if case["m"] > 96:
            keep = np.r_[0:48, case["m"] - 48:case["m"]]
            out["a"] = inp["a"][..., keep, :]
            if case["c"] in ("full", "col", "modulo"):   # C follows the rows it belongs to (modulo: keep the whole case instead)
                return dict(inp), case
            return out, dict(case, m=len(keep))
        return out, case
    if case["n"] > 2:
        sel = [0, case["n"] - 1]
        out = {k: (v[sel] if isinstance(v, np.ndarray) and k in ("x", "r") else v) for k, v in inp.items()}
        return out, dict(case, n=2)
    return dict(inp), case


def variants(case, inp):
    """emulated wrong kernels: (name, inputs the wrong kernel effectively used)"""
    out = []
    if case["kind"] == "gemm":
        a = inp["a"].copy()
        a[..., -1] = 0.0
        out.append(("last k dropped", dict(inp, a=a)))
        if inp["c"] is not None and case["c"] in ("row", "full", "modulo") and case["n"] > 32:
            c = inp["c"].copy()
            if case["c"] == "row":
                c[(case["n"] - 1) // 32 * 32:] = 0.0
            else:
                c[-32:] = 0.0
            out.append(("C missing on the last block", dict(inp, c=c)))
        return out
    x = inp["x"].copy()
    x[:, -1] = 0.0 if case["kind"] != "ci" else case["zx"]
    out.append(("last input channel dropped", dict(inp, x=x)))
    x = inp["x"].copy()
    x[..., -1] = 0.0 if case["kind"] != "ci" else case["zx"]
    out.append(("right edge shifted by one", dict(inp, x=x)))
    x = inp["x"].copy()
    x[..., -1, :] = 0.0 if case["kind"] != "ci" else case["zx"]
    out.append(("bottom edge shifted by one", dict(inp, x=x)))
    if inp.get("b") is not None:
        b = inp["b"].copy()
        b[(case["oc"] - 1) // 32 * 32:] = 0.0
        out.append(("bias missing on the last block", dict(inp, b=b)))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(i, c) for i, c in enumerate(CASES)])
def test_tolerance_rejects_wrong_variants(i):
    case = CASES[i]
    inp, pc = probe(case, make_inputs(i, case))
    ref, mag = reference(pc, inp)
    want = finish(pc, inp, ref)
    ok, msg = accepts(pc, inp, want.astype(np.float32), ref, mag)
    assert ok, "the reference itself, rounded to f32, fails the tolerance: " + msg
    for name, vin in variants(pc, inp):
        vref, _ = reference(pc, vin)
        wrong = finish(pc, inp, vref)
        ok, _ = accepts(pc, inp, wrong.astype(np.float32), ref, mag)
        assert not ok, "%s: the tolerance cannot tell '%s' from the operation" % (case["label"], name)


# -------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(i, c) for i, c in enumerate(CASES)])
def test_route_values_and_nan_field(ctx, i):
    from lele_amd import kernels as K
    case = CASES[i]
    inp = make_inputs(i, case)
    got = run(ctx, case, inp)
    route = K.last_route(ctx)
    assert route == case["label"], "route moved: the library ran %s, the case covers %s" % (route, case["label"])
    assert set(route.split("/")) <= set(K.route_names())
    ref, mag = reference(case, inp)
    ok, msg = accepts(case, inp, got, ref, mag)
    assert ok, msg
    if case["kind"] == "conv" and case["act"] == "relu":   # ReLU may turn NaN into 0: the NaN field runs without it
        case = dict(case, act="none")
    nin, mask = with_nans(case, inp)
    got = run(ctx, case, nin)
    assert K.last_route(ctx) == route
    isnan = np.isnan(got)
    assert np.array_equal(isnan, mask), "%s: %d outputs NaN that should not be, %d not NaN that should be" % (
        case["label"], int((isnan & ~mask).sum()), int((mask & ~isnan).sum()))
    assert np.isfinite(got[~mask]).all(), "%s: an infinite output" % case["label"]


@pytest.mark.gpu
def test_empty_k(ctx):
    """K = 0 through every entry point: the epilogue alone -- zeros, beta * C, the bias (+ activation) -- as the reference gives, and
    no operand read (gemm.k0)"""
    from lele_amd import kernels as K
    from oracle import pyoracle as O
    a, b = np.zeros((70, 0), np.float32), np.zeros((0, 90), np.float32)
    c = np.linspace(-3, 3, 90).astype(np.float32)
    assert np.array_equal(K.matmul(a, b, ctx=ctx).numpy(), O.matmul(a, b))
    assert K.last_route(ctx) == "gemm.k0"
    assert np.array_equal(K.gemm(a, b, c, 2.0, 0.5, ctx=ctx).numpy(), O.gemm(a, b, c, 2.0, 0.5))
    assert K.last_route(ctx) == "gemm.k0"
    assert np.array_equal(K.matmul_fused_add(a, b, c, ctx=ctx).numpy(), O.matmul_fused_add(a, b, c))
    assert K.last_route(ctx) == "gemm.k0"
    got = K.matmul_view(np.zeros((2, 3, 70, 0), np.float32), [], np.zeros((2, 3, 0, 90), np.float32), [], out_perm=[0, 2, 1, 3], ctx=ctx)
    assert np.array_equal(got.numpy(), np.zeros((2, 70, 3, 90), np.float32))
    assert K.last_route(ctx) == "gemm.k0"
    x, w = np.zeros((2, 0, 9, 11), np.float32), np.zeros((20, 0, 3, 3), np.float32)
    bias = np.linspace(-2, 2, 20).astype(np.float32)
    got = K.conv2d_silu(x, w, bias, [1, 1], 1, [1, 1, 1, 1], [1, 1], ctx=ctx).numpy()
    assert K.last_route(ctx) == "conv.gemm_generic/gemm.k0"
    close_f32(got, O.conv2d(x, w, bias, [1, 1], 1, [1, 1, 1, 1], [1, 1], "silu"), 1e-5, "conv2d C_in = 0")
    got = K.conv1d_fused(np.zeros((2, 0, 17), np.float32), np.zeros((20, 0, 1), np.float32), bias, relu=True, ctx=ctx).numpy()
    assert K.last_route(ctx) == "conv.gemm_pw/gemm.k0"
    assert np.array_equal(got, np.broadcast_to(np.maximum(bias, 0).reshape(1, 20, 1), (2, 20, 17)))
