"""LSTM / GRU over a packed batch of independent sequences (include/lele_hip.h: lele_hip_lstm_segments, lele_hip_gru_segments;
lele_amd/csrc/rnn.hip: rnn_seg_kernel): x [R, I] + row_offsets, the layout of the other *_segments calls.

The semantics is "every segment exactly as if it ran alone through lele_hip_lstm / lele_hip_gru", so the yardstick is the EXISTING
single call on the segment alone, never the new code against itself:
  * bit for bit where W x is exact in every summation order (x in k/8, W in k/64, I <= 64: every partial sum is a multiple of 2^-9
    below 2^7) -- the single call's GEMM route moves with T, the packed call's is fixed, and only the recurrence is under test;
  * the oracle per segment at tests/test_conv_rnn.py's element-wise bar (RTOL = 1e-4) on random operands;
  * a segment's bits do not depend on its neighbours, its position or `count` (the M-independent W x route, masking, grouping);
  * chunk-by-chunk calls with the state in place equal one call over the whole sequences, eagerly and replayed as a graph."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4   # tests/test_conv_rnn.py
NAMES = ("lele_hip_lstm_segments", "lele_hip_gru_segments")


def _close(got, want, tol=RTOL, what=""):
    """tests/test_conv_rnn.py::_close: |got - want| <= tol * |want| + tol * rms(want), element by element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not want.size:
        return
    floor = tol * float(np.sqrt(np.mean(np.square(want)))) + 1e-7
    bad = np.abs(got - want) > tol * np.abs(want) + floor
    assert not bad.any(), "%s: %d of %d elements outside %g (max abs diff %.3e, rms %.3e)" % (
        what, int(bad.sum()), want.size, tol, float(np.abs(got - want).max()), float(np.sqrt(np.mean(np.square(want)))))


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def operands(rng, I, H, count, R, exact=False):
    """LSTM-sized operands (the GRU takes the first three gates); exact=True: W x has no rounding in any summation order"""
    sc = np.float32(1.0 / np.sqrt(max(I, H)))
    if exact:
        x = (rng.integers(-8, 9, (R, I)) / 8.0).astype(np.float32)
        w = (rng.integers(-64, 65, (1, 4 * H, I)) / 64.0).astype(np.float32)
    else:
        x = rng.standard_normal((R, I)).astype(np.float32)
        w = (rng.standard_normal((1, 4 * H, I)) * sc).astype(np.float32)
    r = (rng.standard_normal((1, 4 * H, H)) * sc).astype(np.float32)
    b = (rng.standard_normal((1, 8 * H)) * 0.2).astype(np.float32)
    h0 = (rng.standard_normal((1, count, H)) * 0.5).astype(np.float32)
    c0 = (rng.standard_normal((1, count, H)) * 0.5).astype(np.float32)
    return x, w, r, b, h0, c0


def gru_of(w, r, b, H):
    return (np.ascontiguousarray(w[:, :3 * H]), np.ascontiguousarray(r[:, :3 * H]),
            None if b is None else np.ascontiguousarray(np.concatenate([b[:, :3 * H], b[:, 4 * H:7 * H]], axis=1)))


# ---------------------------------------------------------------------------------------------------- CPU: the interface
def test_entry_points_are_declared_exported_and_wrapped():
    from lele_amd import _lib
    from lele_amd import kernels as K
    assert set(NAMES) <= set(_lib.exported_symbols())
    lib = _lib.lib()
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "lele-hip", "src", "ffi.rs")).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert callable(getattr(K, n[len("lele_hip_"):])), n
        assert n + "(" in hpp, n
        assert "pub fn %s(" % n in ffi, n


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "rnn_segments_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "rnn_segments_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_rnn_segments_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- GPU
LENGTHS = [3, 0, 1, 17, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,I,H,form", [("lstm", 24, 128, 1), ("gru", 24, 128, 1), ("lstm", 16, 64, 1), ("lstm", 13, 20, 2), ("gru", 13, 20, 2),
                                           ("lstm", 7, 1, 2), ("gru", 7, 1, 2)])
def test_bit_for_bit_against_the_single_call(ctx, kind, I, H, form):
    from lele_amd import kernels as K
    rng = np.random.default_rng(1000 * H + I)
    off = offsets_of(LENGTHS)
    n = len(LENGTHS)
    x, w, r, b, h0, c0 = operands(rng, I, H, n, int(off[-1]), exact=True)
    for with_state in (True, False):
        bias, hh, cc = (b, h0, c0) if with_state else (None, None, None)
        info = {}
        if kind == "lstm":
            y, h, c = K.lstm_segments(x, off, w, r, bias, hh, cc, info=info, ctx=ctx)
            y, h, c = y.numpy(), h.numpy(), c.numpy()
            assert c.shape == (1, n, H)
        else:
            w3, r3, b3 = gru_of(w, r, bias, H)
            y, h = K.gru_segments(x, off, w3, r3, b3, hh, info=info, ctx=ctx)
            y, h, c = y.numpy(), h.numpy(), None
        assert y.shape == (int(off[-1]), H) and h.shape == (1, n, H)
        assert info == {"form": form, "streams_per_workgroup": 1}
        for i, ln in enumerate(LENGTHS):
            hi = None if hh is None else hh[:, i:i + 1]
            ci = None if cc is None else cc[:, i:i + 1]
            if ln == 0:   # the state comes back exactly (zeros without one)
                assert np.array_equal(h[0, i], np.zeros(H, np.float32) if hi is None else hi[0, 0])
                if c is not None:
                    assert np.array_equal(c[0, i], np.zeros(H, np.float32) if ci is None else ci[0, 0])
                continue
            xi = x[off[i]:off[i + 1]].reshape(ln, 1, I)
            if kind == "lstm":
                yo, ho, co = K.lstm(xi, w, r, bias, None, hi, ci, ctx=ctx)
                assert np.array_equal(c[0, i], co.numpy()[0, 0]), (i, "c")
            else:
                yo, ho = K.gru(xi, w3, r3, b3, hi, False, ctx=ctx)
            assert np.array_equal(y[off[i]:off[i + 1]], yo.numpy().reshape(ln, H)), (i, "y")
            assert np.array_equal(h[0, i], ho.numpy()[0, 0]), (i, "h")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,I,H,lengths", [("lstm", 128, 128, [1, 50, 0, 9]), ("lstm", 300, 517, [4, 2]), ("gru", 64, 128, [9, 1])])
def test_against_the_oracle_per_segment(ctx, kind, I, H, lengths):
    from lele_amd import kernels as K
    rng = np.random.default_rng(7 * H + I)
    off = offsets_of(lengths)
    n = len(lengths)
    x, w, r, b, h0, c0 = operands(rng, I, H, n, int(off[-1]))
    for bias, hh, cc in ((b, h0, c0), (None, None, None)):
        if kind == "lstm":
            y, h, c = (t.numpy() for t in K.lstm_segments(x, off, w, r, bias, hh, cc, ctx=ctx))
        else:
            w3, r3, b3 = gru_of(w, r, bias, H)
            y, h = (t.numpy() for t in K.gru_segments(x, off, w3, r3, b3, hh, ctx=ctx))
        for i, ln in enumerate(lengths):
            if ln == 0:
                continue
            xi = x[off[i]:off[i + 1]].reshape(ln, 1, I)
            hi = None if hh is None else hh[:, i:i + 1]
            if kind == "lstm":
                yo, ho, co = O.lstm(xi, w, r, bias, hi, None if cc is None else cc[:, i:i + 1])
                _close(c[0, i], np.asarray(co).reshape(H), RTOL, "lstm c, segment %d" % i)
            else:
                yo, ho = O.gru(xi, w3, r3, b3, hi)
            _close(y[off[i]:off[i + 1]], np.asarray(yo).reshape(ln, H), RTOL, "%s y, segment %d" % (kind, i))
            _close(h[0, i], np.asarray(ho).reshape(H), RTOL, "%s h, segment %d" % (kind, i))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("H", [128, 20])
def test_a_segment_does_not_depend_on_its_neighbours(ctx, kind, H):
    from lele_amd import kernels as K
    I, V = 40, 5
    cus = K.num_cus(ctx)
    rng = np.random.default_rng(31 + H)
    xv, w, r, b, hv, cv = operands(rng, I, H, 1, V)
    if kind == "gru":
        w, r, b = gru_of(w, r, b, H)

    def run(lengths, at):
        off = offsets_of(lengths)
        n = len(lengths)
        x = rng.standard_normal((int(off[-1]), I)).astype(np.float32)
        h0 = (rng.standard_normal((1, n, H)) * 0.5).astype(np.float32)
        c0 = (rng.standard_normal((1, n, H)) * 0.5).astype(np.float32)
        x[off[at]:off[at + 1]] = xv
        h0[0, at], c0[0, at] = hv[0, 0], cv[0, 0]
        info = {}
        if kind == "lstm":
            y, h, c = (t.numpy() for t in K.lstm_segments(x, off, w, r, b, h0, c0, info=info, ctx=ctx))
            return y[off[at]:off[at + 1]].copy(), h[0, at].copy(), c[0, at].copy(), info
        y, h = (t.numpy() for t in K.gru_segments(x, off, w, r, b, h0, info=info, ctx=ctx))
        return y[off[at]:off[at + 1]].copy(), h[0, at].copy(), None, info

    alone = run([V], 0)
    eight = run([2, 9, 1, V, 0, 4, 30, 3], 3)
    n = 3 * cus + 7
    many_lengths = [[1, 0, 2, 5, 3][i % 5] for i in range(n)]
    many_lengths[100] = V
    many = run(many_lengths, 100)
    n3 = 2 * cus + 5   # NS = 3: an odd member in the pairwise register form, a padding slot in the streamed form's tile of 4
    three = run([[4, 1, 0, 2][i % 4] if i != 7 else V for i in range(n3)], 7)
    assert alone[3]["streams_per_workgroup"] == 1 and eight[3]["streams_per_workgroup"] == 1 and many[3]["streams_per_workgroup"] == 4
    assert three[3]["streams_per_workgroup"] == 3
    for other, name in ((eight, "segment 3 of 8"), (many, "segment 100 of %d" % n), (three, "segment 7 of %d" % n3)):
        assert np.array_equal(alone[0], other[0]), name + ": y"
        assert np.array_equal(alone[1], other[1]), name + ": h"
        if kind == "lstm":
            assert np.array_equal(alone[2], other[2]), name + ": c"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("H", [128, 20])
def test_chunk_after_chunk_in_place_and_as_a_graph(ctx, kind, H):
    from lele_amd import kernels as K
    from lele_amd.tensor import TensorView
    I, N, T = 24, 5, 6
    rng = np.random.default_rng(5 + H)
    x, w, r, b, h0, c0 = operands(rng, I, H, N, N * T)   # packed [N * T, I]: stream i owns rows i * T .. (i + 1) * T
    if kind == "gru":
        w, r, b = gru_of(w, r, b, H)
    dev = lambda a: TensorView(ctx.buf().upload(a))   # noqa: E731
    wd, rd, bd = dev(w), dev(r), dev(b)

    def call(xs, off, hh, cc, outs):
        if kind == "lstm":
            return K.lstm_segments(xs, off, wd, rd, bd, hh, cc, outs=outs, ctx=ctx)
        return K.gru_segments(xs, off, wd, rd, bd, hh, outs=outs[:2], ctx=ctx)

    whole = [t.numpy().copy() for t in call(x, offsets_of([T] * N), h0, c0, [ctx.buf(), ctx.buf(), ctx.buf()])]
    yb, hb, cb, xb = ctx.buf(), ctx.buf(), ctx.buf(), ctx.buf()
    hv, cv = TensorView(hb.upload(h0)), TensorView(cb.upload(c0))
    step = np.arange(N + 1, dtype=np.int64)
    xs = x.reshape(N, T, I)
    for t in range(T):   # one row per stream and call, the state where it was
        res = call(TensorView(xb.upload(xs[:, t])), step, hv, cv, [yb, hb, cb])
        assert np.array_equal(res[0].raw().numpy(), whole[0].reshape(N, T, H)[:, t]), t
    assert np.array_equal(hb.to_numpy((1, N, H)), whole[1])
    if kind == "lstm":
        assert np.array_equal(cb.to_numpy((1, N, H)), whole[2])
    # one more chunk, eagerly from a saved state and replayed as a graph on new x in the same buffer
    x2 = rng.standard_normal((N, I)).astype(np.float32)
    hs, cs = hb.to_numpy((1, N, H)).copy(), cb.to_numpy((1, N, H)).copy()
    xv = TensorView(xb.upload(x2))
    eager = [t.raw().numpy().copy() for t in call(xv, step, hv, cv, [yb, hb, cb])]
    hb.upload(hs), cb.upload(cs), xb.upload(np.zeros((N, I), np.float32))
    ctx.graph_begin()
    call(xv, step, hv, cv, [yb, hb, cb])
    g = ctx.graph_end()
    xb.upload(x2)
    yb.upload(np.zeros((N, H), np.float32))   # the replay writes every value itself
    g.launch()
    assert np.array_equal(yb.to_numpy((N, H)), eager[0])
    assert np.array_equal(hb.to_numpy((1, N, H)), eager[1])
    if kind == "lstm":
        assert np.array_equal(cb.to_numpy((1, N, H)), eager[2])
    g.close()


@pytest.mark.gpu
def test_info_follows_the_documented_rule(ctx):
    from lele_amd import kernels as K
    cus = K.num_cus(ctx)
    rng = np.random.default_rng(3)

    def info_of(kind, H, lengths, I=8):
        off = offsets_of(lengths)
        x, w, r, b, h0, c0 = operands(rng, I, H, len(lengths), int(off[-1]))
        info = {}
        if kind == "lstm":
            K.lstm_segments(x, off, w, r, b, h0, c0, info=info, ctx=ctx)
        else:
            w, r, b = gru_of(w, r, b, H)
            K.gru_segments(x, off, w, r, b, h0, info=info, ctx=ctx)
        return info["form"], info["streams_per_workgroup"]

    for kind in ("lstm", "gru"):
        assert info_of(kind, 128, [2, 1]) == (1, 1)           # S = 2, KS = 64
        assert info_of(kind, 20, [2, 1]) == (2, 1)
        assert info_of(kind, 256, [1]) == (2, 1)              # S = 1, KS = 256: streamed
        assert info_of(kind, 128, [0, 0, 0]) == (0, 1)        # R == 0: nothing launched
        assert info_of(kind, 128, [1] * cus) == (1, 1)
        assert info_of(kind, 128, [1] * (3 * cus + 7)) == (1, 4)
        assert info_of(kind, 20, [1] * (3 * cus + 7)) == (2, 4)
    # empty segments only: the state is handed on exactly
    h0 = rng.standard_normal((1, 3, 16)).astype(np.float32)
    w, r = np.zeros((1, 64, 8), np.float32), np.zeros((1, 64, 16), np.float32)
    y, h, c = K.lstm_segments(np.zeros((0, 8), np.float32), [0, 0, 0, 0], w, r, None, h0, None, ctx=ctx)
    assert y.shape == (0, 16) and np.array_equal(h.numpy(), h0) and np.array_equal(c.numpy(), np.zeros((1, 3, 16), np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_invalid_calls_raise_and_leave_the_outs_untouched(ctx, kind):
    import lele_amd
    from lele_amd import kernels as K
    rng = np.random.default_rng(11)
    I, H, ng = 8, 16, 4 if kind == "lstm" else 3
    x, w, r, b, h0, c0 = operands(rng, I, H, 3, 7)
    if kind == "gru":
        w, r, b = gru_of(w, r, b, H)
    good = dict(off=[0, 3, 3, 7], x=x, w=w, r=r, b=b, h0=h0)
    outs = [ctx.buf(), ctx.buf(), ctx.buf()]

    def call(**kw):
        a = dict(good, **kw)
        if kind == "lstm":
            return K.lstm_segments(a["x"], a["off"], a["w"], a["r"], a["b"], a["h0"], c0 if a["h0"] is h0 else None, outs=outs, ctx=ctx)
        return K.gru_segments(a["x"], a["off"], a["w"], a["r"], a["b"], a["h0"], outs=outs[:2], ctx=ctx)

    res = call()
    before = [t.numpy().copy() for t in res]
    big = 7000 if kind == "lstm" else 8200   # (2H + S G) * 4 bytes with S = 1: 6H * 4 (5H * 4) exceeds 160 KiB; never read, the check comes first
    for kw, msg in (
            (dict(off=[1, 3, 3, 7]), "from 0 to R"), (dict(off=[0, 5, 3, 7]), "decrease"), (dict(off=[0, 3, 3, 6]), "from 0 to R"),
            (dict(x=x.reshape(1, 7, I)), "x must be f32"), (dict(x=x.astype(np.int64)), "x must be f32"),
            (dict(w=np.ascontiguousarray(w[:, :, :I - 1])), "W shape mismatch"), (dict(r=np.ascontiguousarray(r[:, :, :H - 1])), "R shape mismatch"),
            (dict(w=np.concatenate([w, w]), r=np.concatenate([r, r])), "num_directions"),
            (dict(b=np.ascontiguousarray(b[:, :-1])), "bias"), (dict(h0=np.ascontiguousarray(h0[:, :2])), "initial_h"),
            (dict(off=[0, 1], x=np.zeros((1, 1), np.float32), w=np.zeros((1, ng * big, 1), np.float32), r=np.zeros((1, ng * big, big), np.float32),
                  b=np.zeros((1, 2 * ng * big), np.float32), h0=np.zeros((1, 1, big), np.float32)), "hidden_size %d exceeds the LDS" % big)):
        with pytest.raises(lele_amd.LeleError, match=msg):
            call(**kw)
    for t, was in zip(res, before):
        assert np.array_equal(t.raw().buf.to_numpy(was.shape), was)


@pytest.mark.gpu
def test_host_cpp_rnn_segments(tmp_path, ctx):
    from lele_amd import kernels as K
    exe = _build_demo()
    rng = np.random.default_rng(9)
    I, H, lengths = 24, 128, [4, 0, 1, 9]
    off = offsets_of(lengths)
    x, w, r, b, h0, c0 = operands(rng, I, H, len(lengths), int(off[-1]))
    for name, arr in (("dims.i64", np.array([I, H], np.int64)), ("x.f32", x), ("off.i64", off), ("w.f32", w), ("r.f32", r), ("b.f32", b),
                      ("h0.f32", h0), ("c0.f32", c0)):
        arr.tofile(tmp_path / name)
    res = subprocess.run([exe, "run", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("OK"), res.stdout + res.stderr
    li, gi = {}, {}
    ly, lh, lc = K.lstm_segments(x, off, w, r, b, h0, c0, info=li, ctx=ctx)
    w3, r3, b3 = gru_of(w, r, b, H)
    gy, gh = K.gru_segments(x, off, w3, r3, b3, h0, info=gi, ctx=ctx)
    for name, want in (("ly.f32", ly), ("lh.f32", lh), ("lc.f32", lc), ("gy.f32", gy), ("gh.f32", gh)):
        assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(want.shape), want.numpy()), name
    assert list(np.fromfile(tmp_path / "info.i32", np.int32)) == [li["form"], li["streams_per_workgroup"], gi["form"], gi["streams_per_workgroup"]]
