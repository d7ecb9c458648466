"""The greedy decode head: arg-max inside the i8 GEMM (lele_hip_fused_quantized_linear_argmax, .._argmax_segments) and the packed
token filter (lele_hip_token_filter_segments).

Reference: oracle.npref.argmax_last(oracle.pyoracle.fused_quantized_linear(...)) -- per segment for the packed form -- and
pyoracle.decode_greedy_ids for the filter.  Acceptance is EQUALITY OF INTEGERS; there is no tolerance anywhere in this file.

Input families (weights are u8 codes as f32, per-column weight_scale and bias; every batch slice has its own amplitude and offset, so
that two slices never share their dynamic range):
  random    plain draws
  ties      n_base = ceil(n / 3) random base columns, column j copies base j mod n_base (bytes, scale, bias): every row's maximum is
            attained in up to three columns, the expected id is the largest copy < n
  spread    per-column scales over 2^+-3 and biases of several logit standard deviations: the winner by value is not the winner by
            raw accumulator
  negative  a bias that makes every logit negative
  flat      an all-constant slice (degenerate dynamic range) beside a normal one: needs batch >= 2

The CPU part states, on the oracle's logits alone, the conditions that make these families mean something, and that each of seven
emulated wrong kernels is caught by at least one row of at least one case.  The tile-straddling condition of `ties` (the last copy in
another 128-column tile than the first) is geometry: copies lie n_base apart, so it can hold for half of the rows only where
2 * n_base >= 128, i.e. n >= 191; it is asserted on every such case of the table and on the packed layout."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import npref as N  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

FAMILIES = ("random", "ties", "spread", "negative", "flat")
#        batch, m,   K,   n      why
DENSE = [(1, 1, 512, 1),       # smallest
         (1, 5, 512, 127),     # one ragged column tile
         (1, 129, 512, 129),   # ragged row and column tiles
         (3, 50, 512, 300),    # three slices in one row tile
         (4, 33, 64, 130),     # small K
         (1, 40, 40, 260)]     # K not a multiple of 16
WIDE = (2, 171, 512, 25055)    # the model's width, once: `random` and `ties` only
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
    if family == "negative":
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


_cache = {}


def dense_case(family, batch, m, k, n):
    """(x [batch, m, k], (w, ws, wz, bias), oracle logits [batch, m, n]) -- computed once, shared, never written to"""
    key = (family, batch, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(7 + 1000 * FAMILIES.index(family) + 13 * n + m + k)
        wt = weights(family, rng, k, n)
        x = np.stack(slices(family, rng, [m] * batch, k))
        logits = O.fused_quantized_linear(x, *wt)
        for a in (x, logits) + wt:
            a.setflags(write=False)
        _cache[key] = (x, wt, logits)
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
    return np.concatenate([N.argmax_last(lg) if len(lg) else np.zeros(0, np.int32) for lg in logits]).astype(np.int32)


# ---- the oracle's own pieces with the parameters exposed: dynamic_quantize_linear + mat_mul_integer is fused_quantized_linear (the CPU
# part asserts it), which lets an emulated kernel quantise a row with its own slice's range and dequantise it with another's
def model_logits(x_slice, wt, params_of=None, raw=False):
    w, ws, wz, bias = wt
    y, sc, zp = O.dynamic_quantize_linear(x_slice)
    if params_of is not None:
        _, sc, zp = O.dynamic_quantize_linear(params_of)
    if raw:   # the i32 accumulators (as f32)
        return O.mat_mul_integer(y, w, zp, wz, None, None)
    return O.mat_mul_integer(y, w, zp, wz, (sc[0] * ws).astype(np.float32), bias)


def ordered_bits_unsigned(logits):
    """float bits compared as unsigned integers without the sign fix, last of equal maxima"""
    return N.argmax_last(np.ascontiguousarray(logits).view(np.uint32).astype(np.float64))


def argmax_last_any(a):
    a = np.asarray(a)
    return (a.shape[-1] - 1 - np.argmax(a[..., ::-1], axis=-1)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- CPU: conditions
def test_the_parameter_model_is_the_oracle():
    for family, batch, m, k, n in (("random", 3, 50, 512, 300), ("spread", 3, 50, 512, 300)):
        x, wt, logits = dense_case(family, batch, m, k, n)
        for b in range(batch):
            assert np.array_equal(model_logits(x[b], wt).view(np.uint32), logits[b].view(np.uint32))


def test_ties_condition_every_maximum_is_attained_twice_and_straddles_tiles():
    checked_straddle = 0
    cases = [dense_case("ties", *s)[2].reshape(-1, s[3]) for s in DENSE if applies("ties", s[0], s[3])]
    cases.append(np.concatenate(packed_case("ties", PACKED_LENGTHS, 512, 300)[3]))
    for lg in cases:
        n = lg.shape[1]
        mx = lg.max(axis=1, keepdims=True)
        hits = lg == mx
        assert (hits.sum(axis=1) >= 2).all(), n
        first, last = np.argmax(hits, axis=1), N.argmax_last(lg)
        if n >= 191:
            assert np.mean(first // 128 != last // 128) >= 0.5, n
            checked_straddle += 1
        # the expected id is the largest copy < n of the winning base column
        nb = (n + 2) // 3
        assert (last == (first % nb) + nb * ((n - 1 - first % nb) // nb)).all()
    assert checked_straddle >= 3


def test_spread_condition_the_accumulators_pick_another_column():
    for batch, m, k, n in ((3, 50, 512, 300), (1, 129, 512, 129)):
        x, wt, logits = dense_case("spread", batch, m, k, n)
        raw = np.stack([model_logits(x[b], wt, raw=True) for b in range(batch)])
        assert np.mean(argmax_last_any(raw) != N.argmax_last(logits)) >= 0.5, n


def test_negative_condition_every_row_maximum_is_negative():
    for s in DENSE:
        assert (dense_case("negative", *s)[2].max(axis=-1) < 0).all(), s
    assert all((lg.max(axis=-1) < 0).all() for lg in packed_case("negative", PACKED_LENGTHS, 512, 300)[3] if len(lg))


def test_flat_condition_the_constant_slice_has_a_degenerate_range():
    x, wt, logits = dense_case("flat", 3, 50, 512, 300)
    assert np.ptp(x[0]) == 0 and np.ptp(x[1]) > 0
    assert (logits[0] == logits[0][:1]).all()       # every row of the constant slice is the same row


def _differs(emulate):
    """does the emulated kernel give another id than the reference in at least one row of at least one dense case"""
    for family, batch, m, k, n in dense_cases():
        x, wt, logits = dense_case(family, batch, m, k, n)
        if not np.array_equal(emulate(x, wt, logits), N.argmax_last(logits)):
            return True
    return False


def test_emulated_wrong_kernels_are_caught():
    # first of equal maxima wins
    assert _differs(lambda x, wt, lg: np.argmax(lg, axis=-1).astype(np.int32))

    # the ragged last column tile is dropped
    def dropped(x, wt, lg):
        n = lg.shape[-1]
        return N.argmax_last(lg[..., :n - n % 128]) if n >= 128 and n % 128 else N.argmax_last(lg)
    assert _differs(dropped)

    # padded columns take part, with the clamped column's value
    def padded(x, wt, lg):
        n = lg.shape[-1]
        pad = np.repeat(lg[..., -1:], -n % 128, axis=-1)
        return N.argmax_last(np.concatenate([lg, pad], axis=-1))
    assert _differs(padded)
    # accumulators are compared instead of values
    assert _differs(lambda x, wt, lg: argmax_last_any(np.stack([model_logits(xb, wt, raw=True) for xb in x])) if x.shape[2] == 512
                    else N.argmax_last(lg))
    # float bits are compared as unsigned integers without the sign fix
    assert _differs(lambda x, wt, lg: ordered_bits_unsigned(lg))

    # the `split` shortcut gives the third slice of a row tile the second slice's parameters (m = 50: rows 100 .. 127 of tile 0)
    def split_shortcut(x, wt, lg):
        batch, m, _ = x.shape
        out = N.argmax_last(lg).copy()
        if x.shape[2] != 512:
            return out
        for m0 in range(0, batch * m, 128):
            s0 = m0 // m
            for b in range(s0 + 2, batch):
                lo, hi = b * m, min((b + 1) * m, m0 + 128)
                if lo < hi:
                    out[b, lo - b * m:hi - b * m] = N.argmax_last(model_logits(x[b], wt, params_of=x[s0 + 1]))[lo - b * m:hi - b * m]
        return out
    assert _differs(split_shortcut)
    # a row of the packed form reads the parameters of slice row / m (m: the rows of an equal split) instead of its segment's
    caught = False
    for family in ("random", "spread"):
        x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
        count, rows = len(off) - 1, int(off[-1])
        m = -(-rows // count)
        seg_of = np.repeat(np.arange(count), np.diff(off))
        got = np.empty(rows, np.int32)
        for r in range(rows):
            s, t = seg_of[r], min(r // m, count - 1)
            while off[t + 1] == off[t]:
                t -= 1
            got[r] = N.argmax_last(model_logits(x[off[s]:off[s + 1]], wt, params_of=x[off[t]:off[t + 1]]))[r - off[s]] if s != t \
                else N.argmax_last(logits[s])[r - off[s]]
        caught |= not np.array_equal(got, expected_packed(logits))
    assert caught


def test_the_c_abi_declares_the_head():
    from lele_amd._lib import exported_symbols
    names = set(exported_symbols())
    assert {"lele_hip_fused_quantized_linear_argmax", "lele_hip_fused_quantized_linear_argmax_segments", "lele_hip_token_filter_segments"} <= names
    hdr = open(os.path.join(ROOT, "include", "lele_hip.h")).read()
    for fn in ("lele_hip_fused_quantized_linear_argmax(", "lele_hip_fused_quantized_linear_argmax_segments(", "lele_hip_token_filter_segments("):
        doc = hdr[:hdr.index("int " + fn)].rsplit("/*", 1)[1]
        assert "tokenizer.rs:50-71" in doc and "quantization.rs:77-169" in doc, fn
    assert "NaN" in hdr[hdr.index("The greedy decode head"):hdr.index("int lele_hip_fused_quantized_linear_argmax(")]


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "ctc_greedy_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "ctc_greedy_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_ctc_greedy_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- GPU
def run_dense(K, ctx, x, wt, **kw):
    return K.fused_quantized_linear_argmax(x, wt[0], wt[1], wt[2], wt[3], ctx=ctx, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("family,batch,m,k,n", dense_cases() + [("random",) + WIDE, ("ties",) + WIDE])
def test_dense_ids_are_the_oracles_and_the_pairs(ctx, family, batch, m, k, n):
    from lele_amd import kernels as K
    x, wt, logits = dense_case(family, batch, m, k, n)
    want = N.argmax_last(logits)
    got = run_dense(K, ctx, x, wt)
    ids = got.numpy()
    assert ids.dtype == np.int32 and ids.shape == (batch, m) == tuple(got.shape)
    assert np.array_equal(ids, want)
    pair = K.argmax_last(K.fused_quantized_linear(x, *wt, ctx=ctx), ctx=ctx).numpy()
    assert np.array_equal(ids, pair)
    assert np.array_equal(run_dense(K, ctx, x, wt).numpy(), ids)       # the same ids on a second run


@pytest.mark.gpu
def test_dense_rank_2_and_empty(ctx):
    from lele_amd import kernels as K
    x, wt, logits = dense_case("random", 1, 5, 512, 127)
    assert np.array_equal(run_dense(K, ctx, x[0], wt).numpy(), N.argmax_last(logits[0]))
    e = run_dense(K, ctx, np.zeros((2, 0, 512), np.float32), wt)
    assert tuple(e.shape) == (2, 0) and e.numpy().shape == (2, 0) and e.numpy().dtype == np.int32


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in FAMILIES])
def test_packed_segments_are_the_dense_call_on_each_alone(ctx, family):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
    got = K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx)
    ids = got.numpy()
    assert ids.dtype == np.int32 and ids.shape == (int(off[-1]),) == tuple(got.shape)
    assert np.array_equal(ids, expected_packed(logits))
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            alone = run_dense(K, ctx, x[off[i]:off[i + 1]], wt).numpy()
            assert np.array_equal(ids[off[i]:off[i + 1]], alone), i
    assert np.array_equal(K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx).numpy(), ids)


@pytest.mark.gpu
def test_packed_at_the_models_width(ctx):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("ties", [5, 0, 40], 512, 25055)
    ids = K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx).numpy()
    assert np.array_equal(ids, expected_packed(logits))
    assert np.array_equal(ids[5:], run_dense(K, ctx, x[5:], wt).numpy())


@pytest.mark.gpu
def test_packed_empty_layouts_and_equal_lengths(ctx):
    from lele_amd import kernels as K
    x, wt, logits = dense_case("random", 3, 50, 512, 300)
    none = K.fused_quantized_linear_argmax_segments(np.zeros((0, 512), np.float32), [0], *wt, ctx=ctx)
    assert tuple(none.shape) == (0,) and none.numpy().shape == (0,)
    empty = K.fused_quantized_linear_argmax_segments(np.zeros((0, 512), np.float32), [0, 0, 0], *wt, ctx=ctx)
    assert tuple(empty.shape) == (0,) and empty.numpy().dtype == np.int32
    packed = K.fused_quantized_linear_argmax_segments(x.reshape(150, 512), [0, 50, 100, 150], *wt, ctx=ctx).numpy()
    assert np.array_equal(packed, run_dense(K, ctx, x, wt).numpy().reshape(-1))
    assert np.array_equal(packed, N.argmax_last(logits).reshape(-1))


def _skip_table(v, rng):
    skip = (rng.uniform(size=v) < 0.3).astype(np.uint8)
    skip[0] = 1
    return skip


@pytest.mark.gpu
def test_token_filter_segments_is_token_filter_per_segment(ctx):
    from lele_amd import kernels as K
    from lele_amd._lib import LeleError
    rng = np.random.default_rng(5)
    v = 300
    skip = _skip_table(v, rng)
    lengths = [1, 33, 0, 64, 65, 171, 300]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(-3, v + 3, int(off[-1])).astype(np.int32)        # ids outside [0, V) are dropped
    assert (ids < 0).any() and (ids >= v).any()
    for width in (0, 300, 317):
        w = width or 300
        got, cnt = K.token_filter_segments(ids, off, skip, width, ctx=ctx)
        g, c = got.numpy(), cnt.numpy()
        assert g.dtype == np.int32 and c.dtype == np.int32 and g.shape == (len(lengths), w) and c.shape == (len(lengths),)
        for i, n in enumerate(lengths):
            seg = ids[off[i]:off[i + 1]]
            want = np.full(w, -1, np.int32)
            if n:
                a, b = K.token_filter(seg, skip, ctx=ctx)
                a, b = a.numpy(), int(b.numpy().reshape(-1)[0])
                kept = np.array([t for t in seg if 0 <= t < v and not skip[t]], np.int32)
                assert b == len(kept) and np.array_equal(a[:b], kept)
                # the oracle's rule on logits whose arg-max is this segment's in-range ids
                want[:n] = a
            else:
                b = 0
            assert c[i] == b and np.array_equal(g[i], want), (width, i)
    with pytest.raises(LeleError, match=r"segment 6 has 300 rows"):
        K.token_filter_segments(ids, off, skip, 299, ctx=ctx)
    g0, c0 = K.token_filter_segments(np.zeros(0, np.int32), [0, 0], skip, 0, ctx=ctx)
    assert g0.numpy().tolist() == [[-1]] and c0.numpy().tolist() == [0]
    gn, cn = K.token_filter_segments(np.zeros(0, np.int32), [0], skip, 0, ctx=ctx)
    assert tuple(gn.shape) == (0, 1) and tuple(cn.shape) == (0,)


@pytest.mark.gpu
def test_token_filter_segments_against_the_oracle_decoder(ctx):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("random", PACKED_LENGTHS, 512, 300)
    skip = _skip_table(300, np.random.default_rng(6))
    ids = K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx)
    got, cnt = K.token_filter_segments(ids, off, skip, 0, ctx=ctx)
    g, c = got.numpy(), cnt.numpy()
    for i, lg in enumerate(logits):
        if len(lg):
            a, b = O.decode_greedy_ids(lg[None], skip)
            assert c[i] == b[0] and np.array_equal(g[i, :len(lg)], a[0]) and (g[i, len(lg):] == -1).all(), i
        else:
            assert c[i] == 0 and (g[i] == -1).all()


@pytest.mark.gpu
def test_views_and_failures_leave_the_ids_alone(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, logits = dense_case("random", 3, 50, 512, 300)
    want = N.argmax_last(logits)
    # the input as a device tensor 4 bytes past an aligned start
    shifted = _shifted_device_tensor(ctx, x)
    assert np.array_equal(run_dense(K, ctx, shifted, wt).numpy(), want)
    poff = np.array([0, 50, 100, 150], np.int64)
    shifted2 = _shifted_device_tensor(ctx, x.reshape(150, 512))
    assert np.array_equal(K.fused_quantized_linear_argmax_segments(shifted2, poff, *wt, ctx=ctx).numpy(), want.reshape(-1))
    # failures: raised before anything is launched or resized
    out = ctx.buf()
    marker = np.arange(1000, 1150, dtype=np.int32)
    out.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(out._h)
    w, ws, wz, bias = wt
    for call in (lambda: run_dense(K, ctx, x[:, :, :500], wt, out=out),                                        # K mismatch
                 lambda: K.fused_quantized_linear_argmax(x, w, ws[:299], wz, bias, out=out, ctx=ctx),           # short weight_scale
                 lambda: K.fused_quantized_linear_argmax_segments(x.reshape(150, 512), [0, 60, 50, 150], *wt, out=out, ctx=ctx),
                 lambda: K.fused_quantized_linear_argmax_segments(x.reshape(150, 512), [0, 50, 149], *wt, out=out, ctx=ctx),
                 lambda: K.fused_quantized_linear_argmax_segments(x.reshape(150, 512)[:, :500], poff, *wt, out=out, ctx=ctx),
                 lambda: K.fused_quantized_linear_argmax_segments(x.reshape(150, 512), poff, w, ws[:299], wz, bias, out=out, ctx=ctx)):
        with pytest.raises(_lib.LeleError):
            call()
        assert _lib.lib().lele_hip_buf_bytes(out._h) == before
        assert np.array_equal(_lib.DevTensor(out, (150,), np.int32).numpy(), marker)


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
def test_graph_replay_reads_the_new_input(ctx):
    from lele_amd import kernels as K
    xa, wt, la = dense_case("random", 3, 50, 512, 300)
    xb, wtb, lb = dense_case("spread", 3, 50, 512, 300)
    wt = tuple(K.Weight(a.copy()) for a in wt)
    lb_under_wt = O.fused_quantized_linear(xb, *[w.arr for w in wt])
    off = np.array([0, 50, 100, 150], np.int64)
    inp, inp2, out_d, out_p = ctx.buf(), ctx.buf(), ctx.buf(), ctx.buf()
    da = inp.upload(xa)
    pa = inp2.upload(xa.reshape(150, 512))
    K.fused_quantized_linear_argmax(da, *wt, out=out_d, ctx=ctx)                    # one eager run of the same shape / layout
    K.fused_quantized_linear_argmax_segments(pa, off, *wt, out=out_p, ctx=ctx)
    ctx.sync()
    ctx.graph_begin()
    ids_d = K.fused_quantized_linear_argmax(da, *wt, out=out_d, ctx=ctx)
    ids_p = K.fused_quantized_linear_argmax_segments(pa, off, *wt, out=out_p, ctx=ctx)
    graph = ctx.graph_end()
    assert tuple(ids_d.shape) == (3, 50) and tuple(ids_p.shape) == (150,)
    read = lambda: (out_d.to_numpy((3, 50), np.int32), out_p.to_numpy((150,), np.int32))  # noqa: E731  (the buffers themselves: a TensorView caches its host copy)
    out_d.upload(np.full(150, -7, np.int32))
    out_p.upload(np.full(150, -7, np.int32))
    graph.launch()
    got_d, got_p = read()
    assert np.array_equal(got_d, N.argmax_last(la)) and np.array_equal(got_p, N.argmax_last(la).reshape(-1))
    inp.upload(xb)
    inp2.upload(xb.reshape(150, 512))
    graph.launch()
    want = N.argmax_last(lb_under_wt)
    assert not np.array_equal(want, N.argmax_last(la))
    got_d, got_p = read()
    assert np.array_equal(got_d, want) and np.array_equal(got_p, want.reshape(-1))
    graph.close()


@pytest.mark.gpu
def test_no_logits_are_stored(ctx):
    """After the call `out_ids` holds rows x 4 bytes.  Read to confirm that no rows x n workspace exists: the reserve / arena_alloc
    calls on the argmax path of quant.hip -- fql_impl (out->reserve(rows * 4); arena: QParams per slice), launch_range (<= 1024
    {min, max} pairs), run_tiled (arena: rows x kp i8 rows, rows x 4 row sums, rows x ceil(n / 128) x 8 keys), fql_segments_impl (arena: QParams and
    {min, max} pairs per segment, rows x kp, rows x 4, rows x ceil(n / 128) x 8; out->reserve(rows * 4)), packed_weights_of (n x kp weights + n column
    sums, the cache's existing form) -- and lele_hip_token_filter_segments (count x W ids, count counts)."""
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, _ = dense_case("random", 3, 50, 512, 300)
    out, out2 = ctx.buf(), ctx.buf()
    K.fused_quantized_linear_argmax(x, *wt, out=out, ctx=ctx)
    assert _lib.lib().lele_hip_buf_bytes(out._h) == 150 * 4
    K.fused_quantized_linear_argmax_segments(x.reshape(150, 512), [0, 50, 100, 150], *wt, out=out2, ctx=ctx)
    assert _lib.lib().lele_hip_buf_bytes(out2._h) == 150 * 4


@pytest.mark.gpu
def test_encoder_greedy_is_argmax_of_forward(ctx):
    from lele_amd import kernels as K
    from sensevoice_graph import VOCAB, Encoder
    enc = Encoder(ctx, layers=2, seed=3)
    rng = np.random.default_rng(11)
    # dense
    feats = ctx.buf().upload(rng.standard_normal((2, 9, 560)).astype(np.float32))
    want = K.argmax_last(enc.forward(feats), ctx=ctx).numpy()
    got = enc.greedy(feats).numpy()
    assert got.shape == (2, 13) and got.dtype == np.int32 and np.array_equal(got, want)
    # packed: two utterances of different length
    lens = [7, 21]
    off = np.array([0, 7, 28], np.int64)
    pf = ctx.buf().upload(rng.standard_normal((28, 560)).astype(np.float32))
    skip = np.zeros(VOCAB, np.uint8)
    skip[0] = 1
    skip[::3] = 1
    logits, off4 = enc.forward_segments(pf, off)
    lg = logits.numpy()
    ids, counts = enc.greedy_segments(pf, off, skip)
    g, c = ids.numpy(), counts.numpy()
    assert g.shape == (2, max(lens) + 4) and c.shape == (2,)
    for i in range(2):
        seg = lg[off4[i]:off4[i + 1]]
        a, b = O.decode_greedy_ids(seg[None], skip)
        fa, fb = K.token_filter(K.argmax_last(seg, ctx=ctx), skip, ctx=ctx)
        assert np.array_equal(fa.numpy(), a[0]) and int(fb.numpy().reshape(-1)[0]) == b[0]
        assert c[i] == b[0] and np.array_equal(g[i, :len(seg)], a[0]) and (g[i, len(seg):] == -1).all()


@pytest.mark.gpu
def test_host_cpp_ctc_greedy_demo_matches_python(ctx, tmp_path):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("ties", PACKED_LENGTHS, 512, 300)
    skip = _skip_table(300, np.random.default_rng(8))
    d = str(tmp_path)
    for name, a in (("x.f32", x), ("off.i64", off), ("w.f32", wt[0]), ("ws.f32", wt[1]), ("wz.f32", wt[2]), ("b.f32", wt[3]),
                    ("skip.u8", skip), ("dims.i64", np.array([512, 300], np.int64))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    r = subprocess.run([_build_demo(), "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    rd = lambda n: np.fromfile(os.path.join(d, n), np.int32)  # noqa: E731
    ids = K.fused_quantized_linear_argmax_segments(x, off, *wt, ctx=ctx)
    f, c = K.token_filter_segments(ids, off, skip, 0, ctx=ctx)
    assert np.array_equal(rd("ids.i32"), ids.numpy()) and np.array_equal(rd("ids.i32"), expected_packed(logits))
    assert np.array_equal(rd("dense.i32"), rd("ids.i32"))      # the dense call on every segment alone, concatenated
    assert np.array_equal(rd("kept.i32"), f.numpy().reshape(-1)) and np.array_equal(rd("counts.i32"), c.numpy())
