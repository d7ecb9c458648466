"""The scored greedy decode head: the winner's log-probability out of the i8 GEMM's epilogue (lele_hip_fused_quantized_linear_argmax_logprob,
.._logprob_segments) and the packed token filter that keeps each token's frame and score (lele_hip_token_align_segments).

Reference: oracle.pyoracle.fused_quantized_linear gives the bit-exact logits v (per segment alone for the packed form); ids are
oracle.npref.argmax_last(v), compared as integers; logprob is float64 -log sum_j exp(v_j - v_id) on those logits, and the acceptance is
|got - ref64| <= 1e-5 absolute (BAR).  The bar is derived, not measured: a summation depth of at most 64 additions of positive terms is
64 * 2^-24 = 3.8e-6 relative on the sum; the argument scaling of the exponentials adds at most ~30 * 2^-24 on the terms that still
matter (e^-30 and below do not); the hardware exp and log add about an ulp each of a result of magnitude <= ln 25055 = 10.1: under
6.5e-6 in all.

Input families: the five of tests/test_ctc_greedy.py (restated here: random, ties, spread, negative, flat), whose logits have standard
deviations of tens, so that many rows have logprob ~ 0 and hardly test the sum, plus
  soft           weight_scale and bias of `random` divided by 64: logit std 0.02 .. 0.4, logprob between -3.2 and -9.2
  soft_negative  `soft` with the bias of `negative`: a common offset of -1e4 with that small spread; the cancelling form
                 v_id - (max + ln sum) loses 5e-4 there
`ties` shows that every copy of the maximum is counted: a row's logprob is <= -ln(copies), and within 1e-3 of it where the best other
base column lies far enough below (the generator's logit spread does not put EVERY row there, so that is asserted of the rows whose
gap says so, and that there are such rows).

The CPU part states the families' conditions on the oracle's logits, that an f32 emulation of the blocked algorithm (128-column tile
sums around the tile's maximum, a sequential rescaled merge) stays within a quarter of the bar of float64, and that each of six emulated
wrong kernels exceeds the bar on at least one row of at least one case."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import npref as N  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

BAR = 1e-5
FAMILIES = ("random", "ties", "spread", "negative", "flat", "soft", "soft_negative")
#        batch, m,   K,   n      why
DENSE = [(1, 1, 512, 1),       # score exactly 0.0
         (1, 5, 512, 127),     # one ragged column tile
         (1, 129, 512, 129),   # a second tile holding one column, ragged row tile
         (3, 50, 512, 300),    # three slices in one row tile, 84 masked columns
         (4, 33, 64, 130),     # small K
         (1, 40, 40, 260)]     # K not a multiple of 16
WIDE = (2, 171, 512, 25055)    # the model's width, once: `soft` and `ties` only
PACKED_LENGTHS = [1, 33, 0, 64, 65, 171, 300]


def applies(family, batch, n):
    if family == "flat":
        return batch >= 2
    if family == "ties":
        return n >= 2
    return True


def dense_cases():
    return [(f,) + s for s in DENSE for f in FAMILIES if applies(f, s[0], s[3])]


def weights(family, rng, k, n):
    """(w [k, n] u8 codes as f32, weight_scale [n], weight_zero [1], bias [n])"""
    nb = (n + 2) // 3 if family == "ties" else n
    w = np.clip(np.round(128 + 32 * rng.standard_normal((k, nb))), 0, 255).astype(np.float32)
    ws = (np.abs(rng.standard_normal(nb)) * 0.01 + 0.002).astype(np.float32)
    bias = (rng.standard_normal(nb) * 0.02).astype(np.float32)
    if family == "spread":
        ws = (0.005 * np.exp2(rng.uniform(-3, 3, nb))).astype(np.float32)
        bias = (rng.standard_normal(nb) * 40.0).astype(np.float32)
    if family in ("soft", "soft_negative"):
        ws, bias = (ws / np.float32(64.0)).astype(np.float32), (bias / np.float32(64.0)).astype(np.float32)
    if family in ("negative", "soft_negative"):
        bias = (bias - 1.0e4).astype(np.float32)
    if family == "ties":
        idx = np.arange(n) % nb
        w, ws, bias = np.ascontiguousarray(w[:, idx]), ws[idx].copy(), bias[idx].copy()
    return w, ws, np.array([128.0], np.float32), bias


def slices(family, rng, lengths, k):
    """one f32 [len, k] array per slice; slice i with its own amplitude and offset (`flat`: slice 0 constant)"""
    out = []
    for i, m in enumerate(lengths):
        x = (rng.standard_normal((m, k)) * (1.0 + 0.75 * i) + 0.4 * i).astype(np.float32)
        if family == "flat" and i == 0:
            x = np.full((m, k), 0.5, np.float32)
        out.append(x)
    return out


def ref_logprob(logits):
    """float64 -log sum_j exp(v_j - v_id) over the last axis"""
    v = np.asarray(logits, np.float64)
    return -np.log(np.exp(v - v.max(axis=-1, keepdims=True)).sum(axis=-1))


_cache = {}


def dense_case(family, batch, m, k, n):
    """(x [batch, m, k], (w, ws, wz, bias), oracle logits [batch, m, n], ids [batch, m], float64 logprob [batch, m]) -- computed once,
    shared, never written to"""
    key = (family, batch, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(7 + 1000 * FAMILIES.index(family) + 13 * n + m + k)
        wt = weights(family, rng, k, n)
        x = np.stack(slices(family, rng, [m] * batch, k))
        logits = O.fused_quantized_linear(x, *wt)
        ids, lp = N.argmax_last(logits), ref_logprob(logits)
        for a in (x, logits, ids, lp) + wt:
            a.setflags(write=False)
        _cache[key] = (x, wt, logits, ids, lp)
    return _cache[key]


def packed_case(family, lengths, k, n):
    """(x [R, k], offsets, (w, ws, wz, bias), [oracle logits of segment i alone])"""
    key = (family, tuple(lengths), k, n)
    if key not in _cache:
        rng = np.random.default_rng(99 + 1000 * FAMILIES.index(family) + n + len(lengths))
        wt = weights(family, rng, k, n)
        segs = slices(family, rng, lengths, k)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        logits = [O.fused_quantized_linear(s[None], *wt)[0] if len(s) else np.zeros((0, n), np.float32) for s in segs]
        x = np.concatenate(segs) if off[-1] else np.zeros((0, k), np.float32)
        _cache[key] = (x, off, wt, logits)
    return _cache[key]


def expected_packed(logits):
    ids = np.concatenate([N.argmax_last(lg) if len(lg) else np.zeros(0, np.int32) for lg in logits]).astype(np.int32)
    return ids, np.concatenate([ref_logprob(lg) if len(lg) else np.zeros(0) for lg in logits])


def model_logits(x_slice, wt, params_of=None):
    """the oracle's own pieces with the parameters exposed (tests/test_ctc_greedy.py asserts that dynamic_quantize_linear +
    mat_mul_integer is fused_quantized_linear): a row quantised with its own slice's range and dequantised with another's"""
    w, ws, wz, bias = wt
    y, sc, zp = O.dynamic_quantize_linear(x_slice)
    if params_of is not None:
        _, sc, zp = O.dynamic_quantize_linear(params_of)
    return O.mat_mul_integer(y, w, zp, wz, (sc[0] * ws).astype(np.float32), bias)


# ---- the blocked algorithm in f32, and wrong kernels: per 128-column tile the maximum m_t and S_t = sum exp(v - m_t) added column by
# column, then with M = max m_t the merge S = sum_t S_t * exp(m_t - M) tile by tile and logprob = -ln S; every operation rounded to f32
def blocked_f32(logits, wrong=None):
    f32 = np.float32
    lg = np.ascontiguousarray(logits, f32).reshape(-1, logits.shape[-1])
    rows, n = lg.shape
    tiles, pad = -(-n // 128), -n % 128
    if wrong == "padded":      # padded columns counted as the clamped (last) column
        v = np.concatenate([lg, np.repeat(lg[:, -1:], pad, axis=1)], axis=1)
    else:
        v = np.concatenate([lg, np.full((rows, pad), -np.inf, f32)], axis=1)
    v = v.reshape(rows, tiles, 128)
    if wrong == "dropped" and pad and tiles > 1:   # the ragged last column tile never arrives
        v, tiles = v[:, :-1], tiles - 1
    mt = v.max(axis=2)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((v - mt[:, :, None]).astype(f32)).astype(f32)
    st = np.zeros((rows, tiles), f32)
    for c in range(128):
        st = (st + e[:, :, c]).astype(f32)
    if wrong == "mask_one" and pad:   # a masked column counted as exp(0)
        st[:, -1] = (st[:, -1] + f32(pad)).astype(f32)
    big = mt.max(axis=1)
    s = np.zeros(rows, f32)
    for t in range(tiles):
        scale = f32(1.0) if wrong == "norescale" else np.exp((mt[:, t] - big).astype(f32)).astype(f32)
        s = (s + (st[:, t] * scale).astype(f32)).astype(f32)
    if wrong == "cancel":             # v_id - (max + ln S) in f32
        out = (big - (big + np.log(s).astype(f32)).astype(f32)).astype(f32)
    else:
        out = (f32(0.0) - np.log(s).astype(f32)).astype(f32)
    return out.reshape(logits.shape[:-1])


# ---------------------------------------------------------------------------------------------------- CPU
def test_the_c_abi_declares_the_scored_head():
    from lele_amd._lib import exported_symbols
    fns = ("lele_hip_fused_quantized_linear_argmax_logprob", "lele_hip_fused_quantized_linear_argmax_logprob_segments",
           "lele_hip_token_align_segments")
    assert set(fns) <= set(exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "lele_hip.h")).read()
    for fn in fns:
        doc = hdr[:hdr.index("int " + fn + "(")].rsplit("/*", 1)[1]
        assert "tokenizer.rs:50-71" in doc and "quantization.rs:77-169" in doc, fn
    from lele_amd import kernels as K
    assert all(hasattr(K, fn[len("lele_hip_"):]) for fn in fns)


def test_soft_condition_every_row_is_far_from_certain():
    for family in ("soft", "soft_negative"):
        for s in DENSE[1:]:
            assert (dense_case(family, *s)[4] <= -1.0).all(), (family, s)
        # the packed layout's later segments are louder (amplitude 1 + 0.75 i): most of its rows, not all, are as uncertain
        packed = np.concatenate([ref_logprob(lg) for lg in packed_case(family, PACKED_LENGTHS, 512, 300)[3] if len(lg)])
        assert np.mean(packed <= -1.0) >= 0.9, family
    assert (dense_case("soft", *DENSE[0])[4] == 0.0).all()     # N == 1


def test_negative_condition_every_logit_is_large():
    for family in ("negative", "soft_negative"):
        for s in DENSE:
            assert (np.abs(dense_case(family, *s)[2]) >= 5e3).all(), (family, s)


def test_ties_condition_every_copy_counts():
    sharp = total = 0
    for s in DENSE:
        if not applies("ties", s[0], s[3]):
            continue
        _, _, logits, _, lp = dense_case("ties", *s)
        n = s[3]
        lg = logits.reshape(-1, n).astype(np.float64)
        mx = lg.max(axis=1, keepdims=True)
        copies = (lg == mx).sum(axis=1)
        assert (copies >= 2).all(), s
        assert (lp.reshape(-1) <= -np.log(copies) + 1e-12).all(), s
        # the rows whose best other column lies ln(1e3 * n) below the maximum: everything else adds less than 1e-3 to ln(copies)
        gap = mx[:, 0] - np.where(lg == mx, -np.inf, lg).max(axis=1)
        far = gap >= np.log(1e3 * n)
        assert (np.abs(lp.reshape(-1)[far] + np.log(copies[far])) <= 1e-3).all(), s
        sharp, total = sharp + int(far.sum()), total + len(far)
    assert sharp >= total // 10      # the family pins -ln(copies) on a good part of its rows, not on a handful


def all_cases():
    return dense_cases() + [("soft",) + WIDE, ("ties",) + WIDE]


def test_the_blocked_algorithm_in_f32_is_well_inside_the_bar():
    worst = 0.0
    for case in all_cases():
        _, _, logits, _, lp = dense_case(*case)
        err = float(np.max(np.abs(blocked_f32(logits).astype(np.float64) - lp)))
        assert err <= BAR / 4, (case, err)
        worst = max(worst, err)
    for family in FAMILIES:
        for lg in packed_case(family, PACKED_LENGTHS, 512, 300)[3]:
            if len(lg):
                assert np.max(np.abs(blocked_f32(lg).astype(np.float64) - ref_logprob(lg))) <= BAR / 4, family
    print("worst f32 emulation error %.3g" % worst)


@pytest.mark.parametrize("wrong", ["padded", "dropped", "norescale", "cancel", "mask_one"])
def test_emulated_wrong_kernels_exceed_the_bar(wrong):
    worst = 0.0
    for case in dense_cases():
        _, _, logits, _, lp = dense_case(*case)
        worst = max(worst, float(np.max(np.abs(blocked_f32(logits, wrong).astype(np.float64) - lp))))
    assert worst > BAR, (wrong, worst)
    # ... and by a margin: the bar does not sit at the edge of what a wrong kernel does
    assert worst > 15 * BAR, (wrong, worst)


def test_a_row_dequantised_with_another_segments_scale_exceeds_the_bar():
    worst = 0.0
    for family in ("soft", "random"):
        x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
        own, other = x[off[5]:off[6]], x[off[6]:off[7]]
        worst = max(worst, float(np.max(np.abs(ref_logprob(model_logits(own, wt, params_of=other)) - ref_logprob(logits[5])))))
    assert worst > 15 * BAR, worst


def test_token_times_known_answers():
    from lele_amd import apps
    frames = np.array([[0, 3, 4, 5, 104, -1], [4, 14, -1, -1, -1, -1]], np.int32)
    want = np.array([[0.0, 0.0, 0.0, 0.06, 6.0, -1.0], [0.0, 0.6, -1.0, -1.0, -1.0, -1.0]])
    got = apps.token_times(frames)
    assert got.shape == frames.shape and np.allclose(got, want, rtol=0, atol=1e-12)
    assert np.allclose(apps.token_times([2, 7, -1], prompt_rows=0, lfr_n=1, frame_shift_ms=25.0), [0.05, 0.175, -1.0], rtol=0, atol=1e-12)
    assert apps.token_times(np.zeros((0, 3), np.int32)).shape == (0, 3)


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "ctc_scores_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "ctc_scores_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_ctc_scores_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- GPU
def run_dense(K, ctx, x, wt, **kw):
    return K.fused_quantized_linear_argmax_logprob(x, wt[0], wt[1], wt[2], wt[3], ctx=ctx, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("family,batch,m,k,n", all_cases())
def test_dense_ids_and_scores(ctx, family, batch, m, k, n):
    from lele_amd import kernels as K
    x, wt, logits, want, lp = dense_case(family, batch, m, k, n)
    got_ids, got_lp = run_dense(K, ctx, x, wt)
    ids, sc = got_ids.numpy(), got_lp.numpy()
    assert ids.dtype == np.int32 and sc.dtype == np.float32 and ids.shape == sc.shape == (batch, m) == tuple(got_ids.shape) == tuple(got_lp.shape)
    assert np.array_equal(ids, want)
    assert np.array_equal(ids, K.fused_quantized_linear_argmax(x, *wt, ctx=ctx).numpy())
    err = float(np.max(np.abs(sc.astype(np.float64) - lp)))
    print("%s %s: max |logprob - ref64| = %.3g" % (family, (batch, m, k, n), err))
    assert np.isfinite(sc).all() and (sc <= 0).all() and (sc >= -np.log(n) - BAR).all()
    assert err <= BAR
    if n == 1:
        assert (bits(sc) == 0).all()            # exactly +0.0
    again_ids, again_lp = run_dense(K, ctx, x, wt)
    assert np.array_equal(again_ids.numpy(), ids) and np.array_equal(bits(again_lp.numpy()), bits(sc))


@pytest.mark.gpu
def test_dense_rank_2_and_empty(ctx):
    from lele_amd import kernels as K
    x, wt, _, want, lp = dense_case("soft", 1, 5, 512, 127)
    i2, l2 = run_dense(K, ctx, x[0], wt)
    assert tuple(i2.shape) == tuple(l2.shape) == (5,)
    assert np.array_equal(i2.numpy(), want[0]) and np.max(np.abs(l2.numpy().astype(np.float64) - lp[0])) <= BAR
    ei, el = run_dense(K, ctx, np.zeros((2, 0, 512), np.float32), wt)
    assert tuple(ei.shape) == tuple(el.shape) == (2, 0)
    assert ei.numpy().shape == (2, 0) and ei.numpy().dtype == np.int32 and el.numpy().shape == (2, 0) and el.numpy().dtype == np.float32


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_packed_segments_are_the_dense_call_on_each_alone(ctx, family):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
    got_ids, got_lp = K.fused_quantized_linear_argmax_logprob_segments(x, off, *wt, ctx=ctx)
    ids, sc = got_ids.numpy(), got_lp.numpy()
    rows = int(off[-1])
    assert ids.dtype == np.int32 and sc.dtype == np.float32 and ids.shape == sc.shape == (rows,) == tuple(got_ids.shape) == tuple(got_lp.shape)
    want_ids, want_lp = expected_packed(logits)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(ids, K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx).numpy())
    assert np.max(np.abs(sc.astype(np.float64) - want_lp)) <= BAR
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            ai, al = run_dense(K, ctx, x[off[i]:off[i + 1]], wt)
            assert np.array_equal(ids[off[i]:off[i + 1]], ai.numpy()), i
            assert np.array_equal(bits(sc[off[i]:off[i + 1]]), bits(al.numpy())), i


@pytest.mark.gpu
def test_packed_at_the_models_width(ctx):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("soft", [5, 0, 40], 512, 25055)
    got_ids, got_lp = K.fused_quantized_linear_argmax_logprob_segments(x, off, *wt, ctx=ctx)
    ids, sc = got_ids.numpy(), got_lp.numpy()
    want_ids, want_lp = expected_packed(logits)
    assert np.array_equal(ids, want_ids) and np.max(np.abs(sc.astype(np.float64) - want_lp)) <= BAR
    ai, al = run_dense(K, ctx, x[5:], wt)
    assert np.array_equal(ids[5:], ai.numpy()) and np.array_equal(bits(sc[5:]), bits(al.numpy()))


@pytest.mark.gpu
def test_packed_empty_layouts_and_equal_lengths(ctx):
    from lele_amd import kernels as K
    x, wt, _, want, lp = dense_case("soft", 3, 50, 512, 300)
    for layout in ([0], [0, 0, 0]):
        ei, el = K.fused_quantized_linear_argmax_logprob_segments(np.zeros((0, 512), np.float32), layout, *wt, ctx=ctx)
        assert tuple(ei.shape) == tuple(el.shape) == (0,)
        assert ei.numpy().shape == (0,) and ei.numpy().dtype == np.int32 and el.numpy().shape == (0,) and el.numpy().dtype == np.float32
    pi, pl = K.fused_quantized_linear_argmax_logprob_segments(x.reshape(150, 512), [0, 50, 100, 150], *wt, ctx=ctx)
    di, dl = run_dense(K, ctx, x, wt)
    assert np.array_equal(pi.numpy(), di.numpy().reshape(-1)) and np.array_equal(pi.numpy(), want.reshape(-1))
    assert np.array_equal(bits(pl.numpy()), bits(dl.numpy()).reshape(-1))


def _skip_table(v, rng):
    skip = (rng.uniform(size=v) < 0.3).astype(np.uint8)
    skip[0] = 1
    return skip


def _compaction(ids, sc, off, skip, w):
    """numpy: per segment the kept ids, their frames and scores, padded to w"""
    count = len(off) - 1
    oi, of = np.full((count, w), -1, np.int32), np.full((count, w), -1, np.int32)
    ol, oc = np.zeros((count, w), np.float32), np.zeros(count, np.int32)
    for i in range(count):
        seg = ids[off[i]:off[i + 1]]
        keep = np.array([j for j, t in enumerate(seg) if 0 <= t < len(skip) and not skip[t]], np.int64)
        oc[i] = len(keep)
        oi[i, :len(keep)], of[i, :len(keep)] = seg[keep], keep
        if sc is not None:
            ol[i, :len(keep)] = sc[off[i]:off[i + 1]][keep]
    return oi, of, ol, oc


@pytest.mark.gpu
def test_token_align_segments(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    rng = np.random.default_rng(5)
    v = 300
    skip = _skip_table(v, rng)
    off = np.concatenate([[0], np.cumsum(PACKED_LENGTHS)]).astype(np.int64)
    rows = int(off[-1])
    ids = rng.integers(-3, v + 3, rows).astype(np.int32)        # ids outside [0, V) are dropped
    sc = (-rng.uniform(0.0, 9.0, rows)).astype(np.float32)
    sc[::7] = np.float32(-0.0)                                   # copied bit for bit: the sign of zero survives
    assert (ids < 0).any() and (ids >= v).any()
    for width in (0, 300, 317):
        w = width or 300
        gi, gf, gl, gc = K.token_align_segments(ids, sc, off, skip, width, ctx=ctx)
        fi, fc = K.token_filter_segments(ids, off, skip, width, ctx=ctx)
        assert tuple(gi.shape) == tuple(gf.shape) == tuple(gl.shape) == (len(PACKED_LENGTHS), w) and tuple(gc.shape) == (len(PACKED_LENGTHS),)
        assert gi.numpy().dtype == gf.numpy().dtype == gc.numpy().dtype == np.int32 and gl.numpy().dtype == np.float32
        assert np.array_equal(gi.numpy(), fi.numpy()) and np.array_equal(gc.numpy(), fc.numpy())
        wi, wf, wl, wc = _compaction(ids, sc, off, skip, w)
        assert np.array_equal(gi.numpy(), wi) and np.array_equal(gc.numpy(), wc)
        assert np.array_equal(gf.numpy(), wf)
        assert np.array_equal(bits(gl.numpy()), bits(wl))
        # no scores: the same ids, frames and counts, the score output is not touched
        ol = ctx.buf()
        marker = np.arange(5, dtype=np.float32)
        ol.upload(marker)
        ni, nf, nl, nc = K.token_align_segments(ids, None, off, skip, width, out_logprob=ol, ctx=ctx)
        assert nl is None and np.array_equal(ni.numpy(), wi) and np.array_equal(nf.numpy(), wf) and np.array_equal(nc.numpy(), wc)
        assert _lib.lib().lele_hip_buf_bytes(ol._h) == 20 and np.array_equal(ol.to_numpy((5,), np.float32), marker)
    # a too-small width: the error names the segment, all four outputs stay as they were
    outs = [ctx.buf() for _ in range(4)]
    marker = np.arange(1000, 1007, dtype=np.int32)
    for o in outs:
        o.upload(marker)
    with pytest.raises(_lib.LeleError, match=r"segment 6 has 300 rows"):
        K.token_align_segments(ids, sc, off, skip, 299, out_ids=outs[0], out_frames=outs[1], out_logprob=outs[2], out_counts=outs[3], ctx=ctx)
    with pytest.raises(_lib.LeleError):
        K.token_align_segments(ids, sc[:-1], off, skip, 0, out_ids=outs[0], out_frames=outs[1], out_logprob=outs[2], out_counts=outs[3], ctx=ctx)
    for o in outs:
        assert _lib.lib().lele_hip_buf_bytes(o._h) == 28 and np.array_equal(o.to_numpy((7,), np.int32), marker)
    # empty layouts
    g0 = K.token_align_segments(np.zeros(0, np.int32), np.zeros(0, np.float32), [0, 0], skip, 0, ctx=ctx)
    assert g0[0].numpy().tolist() == [[-1]] and g0[1].numpy().tolist() == [[-1]] and g0[2].numpy().tolist() == [[0.0]] and g0[3].numpy().tolist() == [0]
    gn = K.token_align_segments(np.zeros(0, np.int32), np.zeros(0, np.float32), [0], skip, 0, ctx=ctx)
    assert tuple(gn[0].shape) == tuple(gn[1].shape) == tuple(gn[2].shape) == (0, 1) and tuple(gn[3].shape) == (0,)


def _shifted_device_tensor(ctx, x):
    """x as a dense device tensor that starts 4 bytes past an aligned allocation"""
    from lele_amd import _lib

    class Shifted(_lib.DevTensor):
        is_view = property(lambda self: False)     # dense, only not at the start of its buffer

    flat = np.concatenate([np.zeros(1, np.float32), np.asarray(x, np.float32).reshape(-1)])
    t = Shifted(ctx.buf().upload(flat).buf, x.shape, np.float32, 1, 0)
    assert (t.buf.ptr + 4) % 16 == 4
    return t


@pytest.mark.gpu
def test_views_and_failures_leave_the_outputs_alone(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, _, want, lp = dense_case("soft", 3, 50, 512, 300)
    di, dl = run_dense(K, ctx, x, wt)
    ref_bits = bits(dl.numpy())
    # the input as a device tensor 4 bytes past an aligned start
    si, sl = run_dense(K, ctx, _shifted_device_tensor(ctx, x), wt)
    assert np.array_equal(si.numpy(), want) and np.array_equal(bits(sl.numpy()), ref_bits)
    poff = np.array([0, 50, 100, 150], np.int64)
    pi, pl = K.fused_quantized_linear_argmax_logprob_segments(_shifted_device_tensor(ctx, x.reshape(150, 512)), poff, *wt, ctx=ctx)
    assert np.array_equal(pi.numpy(), want.reshape(-1)) and np.array_equal(bits(pl.numpy()), ref_bits.reshape(-1))
    # failures: raised before anything is launched or resized
    oi, ol = ctx.buf(), ctx.buf()
    marker = np.arange(1000, 1150, dtype=np.int32)
    oi.upload(marker)
    ol.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(oi._h)
    w, ws, wz, bias = wt
    seg = K.fused_quantized_linear_argmax_logprob_segments
    o = dict(out_ids=oi, out_logprob=ol, ctx=ctx)
    for call in (lambda: run_dense(K, ctx, x[:, :, :500], wt, out_ids=oi, out_logprob=ol),                   # K mismatch
                 lambda: K.fused_quantized_linear_argmax_logprob(x, w, ws[:299], wz, bias, **o),              # short weight_scale
                 lambda: K.fused_quantized_linear_argmax_logprob(x, w, ws, wz, bias, out_ids=oi, out_logprob=oi, ctx=ctx),   # one buffer twice
                 lambda: seg(x.reshape(150, 512), [0, 60, 50, 150], *wt, **o),
                 lambda: seg(x.reshape(150, 512), [0, 50, 149], *wt, **o),
                 lambda: seg(x.reshape(150, 512)[:, :500], poff, *wt, **o),
                 lambda: seg(x.reshape(150, 512), poff, w, ws[:299], wz, bias, **o)):
        with pytest.raises(_lib.LeleError):
            call()
        for b in (oi, ol):
            assert _lib.lib().lele_hip_buf_bytes(b._h) == before
            assert np.array_equal(b.to_numpy((150,), np.int32), marker)


@pytest.mark.gpu
def test_graph_replay_reads_the_new_input(ctx):
    from lele_amd import kernels as K
    xa, wt, la, ia, lpa = dense_case("soft", 3, 50, 512, 300)
    xb = dense_case("random", 3, 50, 512, 300)[0]
    wt = tuple(K.Weight(a.copy()) for a in wt)
    lb = O.fused_quantized_linear(xb, *[w.arr for w in wt])
    ib, lpb = N.argmax_last(lb), ref_logprob(lb)
    assert not np.array_equal(ia, ib)
    off = np.array([0, 50, 100, 150], np.int64)
    skip = _skip_table(300, np.random.default_rng(9))
    dskip = K.Weight(skip)                                      # a capture takes no host inputs
    inp, inp2 = ctx.buf(), ctx.buf()
    outs = [ctx.buf() for _ in range(8)]
    da = inp.upload(xa)
    pa = inp2.upload(xa.reshape(150, 512))

    def run():
        K.fused_quantized_linear_argmax_logprob(da, *wt, out_ids=outs[0], out_logprob=outs[1], ctx=ctx)
        pi, pl = K.fused_quantized_linear_argmax_logprob_segments(pa, off, *wt, out_ids=outs[2], out_logprob=outs[3], ctx=ctx)
        K.token_align_segments(pi, pl, off, dskip, 0, out_ids=outs[4], out_frames=outs[5], out_logprob=outs[6], out_counts=outs[7], ctx=ctx)

    run()                                                       # one eager run of the same shape / layout
    ctx.sync()
    ctx.graph_begin()
    run()
    graph = ctx.graph_end()
    for want_ids, want_lp, x in ((ia, lpa, None), (ib, lpb, xb)):
        if x is not None:
            inp.upload(x)
            inp2.upload(x.reshape(150, 512))
        for o in outs[:4]:
            o.upload(np.full(150, -7, np.int32))
        graph.launch()
        d_ids, d_lp = outs[0].to_numpy((3, 50), np.int32), outs[1].to_numpy((3, 50), np.float32)
        p_ids, p_lp = outs[2].to_numpy((150,), np.int32), outs[3].to_numpy((150,), np.float32)
        assert np.array_equal(d_ids, want_ids) and np.array_equal(p_ids, want_ids.reshape(-1))
        assert np.max(np.abs(d_lp.astype(np.float64) - want_lp)) <= BAR and np.array_equal(bits(p_lp), bits(d_lp).reshape(-1))
        wi, wf, wl, wc = _compaction(p_ids, p_lp, off, skip, 50)
        assert np.array_equal(outs[4].to_numpy((3, 50), np.int32), wi) and np.array_equal(outs[5].to_numpy((3, 50), np.int32), wf)
        assert np.array_equal(bits(outs[6].to_numpy((3, 50), np.float32)), bits(wl)) and np.array_equal(outs[7].to_numpy((3,), np.int32), wc)
    graph.close()


@pytest.mark.gpu
def test_no_logits_are_stored(ctx):
    """After the call `out_ids` and `out_logprob` hold rows x 4 bytes each.  Read to confirm that no rows x n workspace exists: the
    reserve / arena_alloc calls on the scored path of quant.hip are those of the ids-only head (tests/test_ctc_greedy.py lists them)
    plus, in run_tiled and fql_segments_impl, the second table of rows x ceil(n / 128) x 4 bytes of tile sums beside the rows x
    ceil(n / 128) x 8 bytes of keys, and the out_logprob->reserve(rows * 4) beside out->reserve(rows * 4); lele_hip_token_align_segments
    reserves count x W ids, frames and scores and count counts."""
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt = dense_case("soft", 3, 50, 512, 300)[:2]
    oi, ol, pi, pl = (ctx.buf() for _ in range(4))
    K.fused_quantized_linear_argmax_logprob(x, *wt, out_ids=oi, out_logprob=ol, ctx=ctx)
    ids, sc = K.fused_quantized_linear_argmax_logprob_segments(x.reshape(150, 512), [0, 50, 100, 150], *wt, out_ids=pi, out_logprob=pl, ctx=ctx)
    for b in (oi, ol, pi, pl):
        assert _lib.lib().lele_hip_buf_bytes(b._h) == 150 * 4
    outs = [ctx.buf() for _ in range(4)]
    K.token_align_segments(ids, sc, [0, 50, 100, 150], np.zeros(300, np.uint8), 64, out_ids=outs[0], out_frames=outs[1], out_logprob=outs[2],
                           out_counts=outs[3], ctx=ctx)
    assert [_lib.lib().lele_hip_buf_bytes(b._h) for b in outs] == [3 * 64 * 4] * 3 + [3 * 4]


@pytest.mark.gpu
def test_encoder_scored_heads_agree_with_the_ids_only_heads(ctx):
    from sensevoice_graph import VOCAB, Encoder
    enc = Encoder(ctx, layers=2, seed=3)
    rng = np.random.default_rng(11)
    feats = ctx.buf().upload(rng.standard_normal((2, 9, 560)).astype(np.float32))
    want = enc.greedy(feats).numpy().copy()
    ids, lp = enc.greedy_scored(feats)
    assert ids.numpy().shape == lp.numpy().shape == (2, 13) and np.array_equal(ids.numpy(), want)
    assert lp.numpy().dtype == np.float32 and np.isfinite(lp.numpy()).all() and (lp.numpy() <= 0).all() and (lp.numpy() >= -np.log(VOCAB) - BAR).all()
    # packed: two utterances of different length
    lens = [7, 21]
    off = np.array([0, 7, 28], np.int64)
    pf = ctx.buf().upload(rng.standard_normal((28, 560)).astype(np.float32))
    skip = np.zeros(VOCAB, np.uint8)
    skip[0] = 1
    skip[::3] = 1
    wi, wc = enc.greedy_segments(pf, off, skip)
    wi, wc = wi.numpy().copy(), wc.numpy().copy()
    gi, gf, gl, gc = (a.numpy() for a in enc.greedy_segments_scored(pf, off, skip))
    assert gi.shape == gf.shape == gl.shape == (2, max(lens) + 4) and np.array_equal(gi, wi) and np.array_equal(gc, wc)
    for i in range(2):
        f = gf[i, :gc[i]]
        assert (f >= 0).all() and (f < lens[i] + 4).all() and (np.diff(f) > 0).all() and (gf[i, gc[i]:] == -1).all()
        assert (gl[i, :gc[i]] <= 0).all() and (bits(gl[i, gc[i]:]) == 0).all()


@pytest.mark.gpu
def test_host_cpp_ctc_scores_demo_matches_python(ctx, tmp_path):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("soft", PACKED_LENGTHS, 512, 300)
    skip = _skip_table(300, np.random.default_rng(8))
    d = str(tmp_path)
    for name, a in (("x.f32", x), ("off.i64", off), ("w.f32", wt[0]), ("ws.f32", wt[1]), ("wz.f32", wt[2]), ("b.f32", wt[3]),
                    ("skip.u8", skip), ("dims.i64", np.array([512, 300], np.int64))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    r = subprocess.run([_build_demo(), "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    rd = lambda n, t: np.fromfile(os.path.join(d, n), t)  # noqa: E731
    ids, lp = K.fused_quantized_linear_argmax_logprob_segments(x, off, *wt, ctx=ctx)
    ki, kf, kl, kc = K.token_align_segments(ids, lp, off, skip, 0, ctx=ctx)
    assert np.array_equal(rd("ids.i32", np.int32), ids.numpy()) and np.array_equal(rd("ids.i32", np.int32), expected_packed(logits)[0])
    assert np.array_equal(rd("lp.f32", np.uint32), bits(lp.numpy()))
    assert np.array_equal(rd("dense_ids.i32", np.int32), rd("ids.i32", np.int32)) and np.array_equal(rd("dense_lp.f32", np.uint32), rd("lp.f32", np.uint32))
    assert np.array_equal(rd("kept.i32", np.int32), ki.numpy().reshape(-1)) and np.array_equal(rd("frames.i32", np.int32), kf.numpy().reshape(-1))
    assert np.array_equal(rd("kept_lp.f32", np.uint32), bits(kl.numpy()).reshape(-1)) and np.array_equal(rd("counts.i32", np.int32), kc.numpy())
