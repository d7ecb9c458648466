"""Variable-length utterances through the encoder as ONE packed batch: x [R, D] + row_offsets, the layout the front-end's
compute_segments / Cmvn.compute_segments hand on (include/lele_hip.h: lele_hip_fused_quantized_linear_segments,
lele_hip_attention_segments, lele_hip_depthwise_conv1d_tlc_segments, lele_hip_segments_prepend; tools/sensevoice_graph.py:
Encoder.forward_segments).

The semantics is "every utterance exactly as if it ran alone" (the reference is batch 1 throughout), so the yardstick of every check is
the EXISTING dense entry point on the segment alone -- never the new code against itself:
  * quantised linear, FSMN stencil, prepend: bit for bit (integer sums are exact, the stencil is the same FMA chain);
  * attention: the two bars and the `close` of tests/test_attention.py (1e-4 against attention_view on the segment alone, 2e-4 against
    the oracle composition) -- the dense call picks 16- / 32- / 128-row kernels by grid size, each with its own summation order, so bits
    cannot be asked for; what IS bitwise: permuting a layout's segments permutes the result, and rewriting one segment changes no other;
  * composed: node by node on the device's own tapped input, end to end against Encoder.forward per utterance at the reference's own
    bar (examples/sensevoice/tests/e2e_test.rs:141-189: mean absolute logit error <= 1.0; arg-max agreement printed), from PCM, and
    recorded into a hipGraph."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conftest import synth_pcm  # noqa: E402

H, DH, D = 4, 128, 512
QC = [["slice", 2, 0, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
KC = [["slice", 2, 512, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 3, 1]]]
VC = [["slice", 2, 1024, 512], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
NAMES = ("lele_hip_fused_quantized_linear_segments", "lele_hip_attention_segments", "lele_hip_depthwise_conv1d_tlc_segments",
         "lele_hip_segments_prepend")
SV_MAX_MAE = 1.0   # e2e_test.rs:141-146, as tests/test_graph_oracle.py uses it


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


def close(a, b, what, rtol=1e-4):
    """tests/test_attention.py's: relative to the element, with rtol x rms of the tensor as the floor"""
    b = np.asarray(b, np.float32)
    floor = rtol * float(np.sqrt(np.mean(np.square(b, dtype=np.float64)))) + 1e-7
    bad = np.abs(a - b) > rtol * np.abs(b) + floor
    assert not bad.any(), "%s: %d of %d elements outside %g (max abs diff %.3g)" % (what, int(bad.sum()), b.size, rtol, float(np.abs(a - b).max()))


def logits_agreement(dev, ref):
    """the two figures examples/sensevoice/tests/e2e_test.rs:126-189 judges the model by"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return {"mae": float(np.abs(dev - ref).mean()), "argmax_agreement": float((dev.argmax(-1) == ref.argmax(-1)).mean())}


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- CPU: the interface
def test_segment_entry_points_are_declared_exported_and_wrapped():
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


def test_forward_segments_is_a_method_of_the_encoder():
    from sensevoice_graph import Encoder
    assert callable(Encoder.forward_segments) and callable(Encoder.layer_segments)


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "encoder_segments_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "encoder_segments_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_encoder_segments_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- GPU: validation
@pytest.mark.gpu
def test_invalid_layouts_raise_and_leave_out_untouched(ctx):
    import lele_amd
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(1)
    x = ctx.buf().upload(rng.standard_normal((40, 1536)).astype(np.float32))
    w = Weight(rng.integers(0, 256, (1536, 64)).astype(np.float32))
    ws, wz, fs = Weight(np.full(64, 0.01, np.float32)), Weight(np.array([128.0], np.float32)), Weight(rng.standard_normal((512, 1, 11)).astype(np.float32))
    good = [0, 10, 40]
    calls = {
        "linear": lambda off, out: K.fused_quantized_linear_segments(x, off, w, ws, wz, None, out=out, ctx=ctx),
        "attention": lambda off, out: K.attention_segments(x, off, H, DH, out=out, ctx=ctx),
        "stencil": lambda off, out: K.depthwise_conv1d_tlc_segments(x, off, fs, None, 5, 5, x_offset=1024, out=out, ctx=ctx),
        "prepend": lambda off, out: K.segments_prepend(x, off, np.ones((4, 1536), np.float32), out=out, ctx=ctx)[0],
    }
    for name, call in calls.items():
        out = ctx.buf()
        shape = call(good, out).shape
        before = out.to_numpy(shape).copy()
        for bad, msg in (([0, 30, 20, 40], "decrease"), ([1, 10, 40], "from 0 to R"), ([0, 10, 39], "from 0 to R"), ([0, 10, 41], "from 0 to R")):
            with pytest.raises(lele_amd.LeleError, match=msg):
                call(bad, out)
        assert np.array_equal(out.to_numpy(shape), before), name
    # the attention's own limits: a 513-row segment (the message names it), a head dimension other than 128, unaligned columns
    big = ctx.buf().upload(rng.standard_normal((3 + 513, 1536)).astype(np.float32))
    out = ctx.buf()
    shape = K.attention_segments(big, [0, 3, 516 - 513 + 512, 516], H, DH, out=out, ctx=ctx).shape
    before = out.to_numpy(shape).copy()
    with pytest.raises(lele_amd.LeleError, match="segment 1 has 513 rows"):
        K.attention_segments(big, [0, 3, 516], H, DH, out=out, ctx=ctx)
    with pytest.raises(lele_amd.LeleError, match="head dimension 64"):
        K.attention_segments(big, [0, 3, 515, 516], 8, 64, out=out, ctx=ctx)
    with pytest.raises(lele_amd.LeleError, match="16-byte"):
        K.attention_segments(big, [0, 3, 515, 516], H, DH, q_offset=2, k_offset=512, v_offset=1024, out=out, ctx=ctx)
    assert np.array_equal(out.to_numpy(shape), before)
    # the stencil keeps every segment's rows: pad_left + pad_right == K - 1
    out = ctx.buf()
    shape = calls["stencil"](good, out).shape
    before = out.to_numpy(shape).copy()
    with pytest.raises(lele_amd.LeleError, match="K - 1"):
        K.depthwise_conv1d_tlc_segments(x, good, fs, None, 5, 4, x_offset=1024, out=out, ctx=ctx)
    assert np.array_equal(out.to_numpy(shape), before)


# ---------------------------------------------------------------------------------------------------- GPU: per operator
Q_LENGTHS = [1, 0, 2, 7, 8, 9, 31, 32, 33, 0, 64, 65, 97, 171, 300, 449, 508]


def _adversarial_rows(rng, lengths, k):
    """segments scaled by 10^(i mod 7 - 3), every third one shifted to be all-positive or all-negative: a row quantised with a
    neighbour's parameters cannot come out right"""
    parts = []
    for i, ln in enumerate(lengths):
        p = rng.standard_normal((ln, k)).astype(np.float32) * np.float32(10.0 ** (i % 7 - 3))
        if i % 3 == 2 and ln:
            shift = np.float32(1.5 * np.abs(p).max())
            p = p + shift if (i // 3) % 2 == 0 else p - shift
            assert (p > 0).all() or (p < 0).all()
        parts.append(p.astype(np.float32))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,relu,bias", [(560, 1536, False, True), (512, 512, False, True), (512, 2048, True, True), (2048, 512, False, True),
                                           (512, 25055, False, True), (13, 24, False, True), (512, 512, False, False)])
def test_quantised_linear_segments_bitwise_per_segment(ctx, orc, k, n, relu, bias):
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(k * 31 + n)
    lengths = [Q_LENGTHS[i] for i in rng.permutation(len(Q_LENGTHS))]
    off = offsets_of(lengths)
    x = _adversarial_rows(rng, lengths, k)
    w = Weight(np.clip(np.round(128 + 32 * rng.standard_normal((k, n))), 0, 255).astype(np.float32))
    ws = Weight((np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32))
    wz = Weight(np.array([128.0], np.float32))
    b = Weight((rng.standard_normal(n) * 0.02).astype(np.float32)) if bias else None
    xd = ctx.buf().upload(x)
    got = K.fused_quantized_linear_segments(xd, off, w, ws, wz, b, relu, ctx=ctx)
    assert got.shape == (len(x), n)
    got = got.numpy()
    for i, ln in enumerate(lengths):
        if ln == 0:
            continue
        seg = x[off[i]:off[i + 1]]
        dense = K.fused_quantized_linear(ctx.buf().upload(seg), w, ws, wz, b, relu, ctx=ctx).numpy()
        assert np.array_equal(got[off[i]:off[i + 1]], dense), "segment %d (%d rows) differs from the dense call on it alone" % (i, ln)
        want = orc.fused_quantized_linear(seg, w.arr, ws.arr, [128.0], b.arr if bias else None, relu)
        assert np.array_equal(got[off[i]:off[i + 1]], want), "segment %d (%d rows) differs from the oracle" % (i, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [3, 11])
@pytest.mark.parametrize("x_offset", [0, 1024])
def test_fsmn_stencil_segments_bitwise_per_segment(ctx, kw, x_offset):
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(kw * 7 + x_offset)
    lengths = [Q_LENGTHS[i] for i in rng.permutation(len(Q_LENGTHS))]
    off = offsets_of(lengths)
    x = rng.standard_normal((int(off[-1]), 1536)).astype(np.float32)
    w = Weight((rng.standard_normal((D, 1, kw)) / np.sqrt(kw)).astype(np.float32))
    bvec = Weight(rng.standard_normal(D).astype(np.float32))
    xd = ctx.buf().upload(x)
    pl = kw // 2
    for bias in (None, bvec):
        for add_input in (False, True):
            got = K.depthwise_conv1d_tlc_segments(xd, off, w, bias, pl, kw - 1 - pl, x_offset=x_offset, add_input=add_input, ctx=ctx)
            assert got.shape == (len(x), D)
            got = got.numpy()
            for i, ln in enumerate(lengths):
                if ln == 0:
                    continue
                seg = ctx.buf().upload(x[off[i]:off[i + 1]][None])
                dense = K.depthwise_conv1d_tlc(seg, w, bias, pl, kw - 1 - pl, x_offset=x_offset, add_input=add_input, ctx=ctx).numpy()[0]
                assert np.array_equal(got[off[i]:off[i + 1]], dense), (i, ln, bias is not None, add_input)


def _oracle_attention(orc, qkv, heads=H):
    t, d = len(qkv), heads * DH
    q = np.ascontiguousarray(qkv[:, :d].reshape(1, t, heads, DH).transpose(0, 2, 1, 3))
    kT = np.ascontiguousarray(qkv[:, d:2 * d].reshape(1, t, heads, DH).transpose(0, 2, 3, 1))
    v = np.ascontiguousarray(qkv[:, 2 * d:].reshape(1, t, heads, DH).transpose(0, 2, 1, 3))
    p = orc.softmax(orc.matmul(q, kT) * np.float32(DH ** -0.5), -1)
    return np.ascontiguousarray(orc.matmul(p, v).transpose(0, 2, 1, 3)).reshape(t, d)


def _chains(heads):
    d = heads * DH
    return ([["slice", 2, 0, d], ["reshape", [0, 0, heads, DH]], ["transpose", [0, 2, 1, 3]]],
            [["slice", 2, d, d], ["reshape", [0, 0, heads, DH]], ["transpose", [0, 2, 3, 1]]],
            [["slice", 2, 2 * d, d], ["reshape", [0, 0, heads, DH]], ["transpose", [0, 2, 1, 3]]])


A_LENGTHS = [1, 8, 33, 0, 64, 65, 100, 171, 257, 300, 449, 504, 512]


def _check_attention_layout(ctx, orc, exact, lengths, heads, rng, victim):
    """per segment against attention_view on it alone (1e-4) and the oracle composition (2e-4); then the two bitwise properties"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    d = heads * DH
    qc, kc, vc = _chains(heads)
    off = offsets_of(lengths)
    qkv = (rng.standard_normal((int(off[-1]), 3 * d)) * 1.5).astype(np.float32)
    scale = Weight(np.array([DH ** -0.5], np.float32))
    qd = ctx.buf().upload(qkv)
    with _env(LELE_HIP_ATTENTION_EXACT=exact):
        got = K.attention_segments(qd, off, heads, DH, scale, ctx=ctx)
        assert got.shape == (len(qkv), d)
        got = got.numpy()
        for i, ln in enumerate(lengths):
            if ln == 0:
                continue
            seg = qkv[off[i]:off[i + 1]]
            sd = ctx.buf().upload(seg[None])
            with _env(LELE_HIP_ATTENTION_MIN_BLOCKS=1):   # the one-launch kernel whatever the grid size
                dense = K.attention_view(sd, qc, sd, kc, sd, vc, scale, [0, 2, 1, 3], [0, 0, d], ctx=ctx).numpy()[0]
            close(got[off[i]:off[i + 1]], dense, "segment %d (%d rows) vs attention_view on it alone" % (i, ln))
            close(got[off[i]:off[i + 1]], _oracle_attention(orc, seg, heads), "segment %d (%d rows) vs oracle composition" % (i, ln), rtol=2e-4)
        # bitwise: the same multiset of segments in another order gives the same segments
        perm = rng.permutation(len(lengths))
        q2 = np.concatenate([qkv[off[i]:off[i + 1]] for i in perm])
        off2 = offsets_of([lengths[i] for i in perm])
        got2 = K.attention_segments(ctx.buf().upload(q2), off2, heads, DH, scale, ctx=ctx).numpy()
        for j, i in enumerate(perm):
            assert np.array_equal(got2[off2[j]:off2[j + 1]], got[off[i]:off[i + 1]]), (j, i)
        # bitwise: rewriting one segment's rows changes no other segment
        q3 = qkv.copy()
        q3[off[victim]:off[victim + 1]] = (rng.standard_normal((lengths[victim], 3 * d)) * 40).astype(np.float32)
        got3 = K.attention_segments(ctx.buf().upload(q3), off, heads, DH, scale, ctx=ctx).numpy()
        keep = np.ones(len(qkv), bool)
        keep[off[victim]:off[victim + 1]] = False
        assert np.array_equal(got3[keep], got[keep])
        assert not np.array_equal(got3[~keep], got[~keep])


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("layout", ["mixed", "32x171"])
def test_attention_segments_per_segment(ctx, orc, exact, layout):
    rng = np.random.default_rng(41 + exact)
    lengths = [A_LENGTHS[i] for i in rng.permutation(len(A_LENGTHS))] if layout == "mixed" else [171] * 32
    _check_attention_layout(ctx, orc, exact, lengths, H, rng, int(np.argmax(lengths)) if layout == "mixed" else 7)


# More heads: a segment takes 16-row workgroups while heads x ceil(len / 32) < CUs / 2 (128 on the MI355X) and the 32-row
# attention_kernel from there on.  The lengths straddle that rule INSIDE one key-tile class (8 heads: 480 | 481 rows in class 8; 16 heads:
# 224 | 225 rows in class 4), so that class has a 16-row and a 32-row work list, and put 32-row segments into further classes -- more
# than 256 workgroups in one launch, where the kernel's wave -> key-tile rotation (a function of the workgroup index) changes.
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("heads,lengths,victim", [(8, [470, 481, 33, 480, 0, 512, 500, 200, 496], 5),
                                                  (16, [200, 225, 224, 1, 256, 240, 300, 512, 64, 449], 7)])
def test_attention_segments_more_heads_both_block_heights(ctx, orc, exact, heads, lengths, victim):
    half = 128   # the rule's threshold on the MI355X; the layouts below are chosen for it
    tall = [ln for ln in lengths if ln and heads * -(-ln // 32) >= half]
    low = [ln for ln in lengths if ln and heads * -(-ln // 32) < half]
    assert tall and low and any(-(-a // 64) == -(-b // 64) for a in tall for b in low)      # one class holds both heights
    assert sum(heads * -(-ln // 32) for ln in tall if -(-ln // 64) == 8) > 256             # the rotation changes inside one launch
    _check_attention_layout(ctx, orc, exact, lengths, heads, np.random.default_rng(heads * 10 + exact), victim)


@pytest.mark.gpu
def test_segments_prepend_matches_numpy(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(5)
    for lengths in ([5, 0, 17, 1, 90, 0], [0, 0], [3]):
        off = offsets_of(lengths)
        x = rng.standard_normal((int(off[-1]), 560)).astype(np.float32)
        prefix = rng.standard_normal((4, 560)).astype(np.float32)
        xd = ctx.buf().upload(x) if len(x) else x   # every segment empty: R == 0, nothing on the device to hand over
        y, off2 = K.segments_prepend(xd, off, prefix, ctx=ctx)
        assert np.array_equal(off2, off + 4 * np.arange(len(off)))
        want = np.concatenate([np.concatenate([prefix, x[off[i]:off[i + 1]]]) for i in range(len(lengths))])
        assert y.shape == want.shape and np.array_equal(y.numpy(), want)


# ---------------------------------------------------------------------------------------------------- GPU: composed
E_LENGTHS = [171, 1, 500, 33, 0, 64, 97, 300]


@pytest.fixture(scope="module")
def enc3(ctx):
    from sensevoice_graph import Encoder, encoder_arrays
    enc = Encoder(ctx, layers=3, damped=True)
    return enc, encoder_arrays(enc)


def _packed_feats(rng, lengths):
    return rng.standard_normal((int(np.sum(lengths)), 560)).astype(np.float32)


@pytest.mark.gpu
def test_forward_segments_node_by_node_on_the_devices_own_inputs(ctx, enc3):
    """every node of every layer: the tapped output against the DENSE operator on each segment of the tapped input alone"""
    from lele_amd import kernels as K
    enc, _ = enc3
    rng = np.random.default_rng(77)
    off = offsets_of(E_LENGTHS)
    feats = ctx.buf().upload(_packed_feats(rng, E_LENGTHS))
    taps = {i: {} for i in range(3)}
    taps["embed"], taps["head"] = {}, {}
    logits, off4 = enc.forward_segments(feats, off, taps)
    assert np.array_equal(off4, off + 4 * np.arange(len(off)))
    assert logits.shape == (int(off4[-1]), 25055)
    up = lambda a: ctx.buf().upload(np.ascontiguousarray(a))   # noqa: E731

    def ql(x, p, relu=False):
        return K.fused_quantized_linear(up(x), p.w, p.scale, p.zero, p.bias, relu, ctx=ctx).numpy()

    for i in range(3):
        t, L = taps[i], enc.layers[i]
        for s in range(len(E_LENGTHS)):
            a, b = int(off4[s]), int(off4[s + 1])
            tag = "layer %d segment %d (%d rows)" % (i, s, b - a)
            seg = lambda name: t[name][a:b]   # noqa: E731
            same = lambda got, want, what: np.testing.assert_array_equal(got, want, err_msg=tag + " " + what)   # noqa: E731
            same(seg("xn"), K.layer_norm(up(seg("x")), L.ln1[0], L.ln1[1], -1, 1e-5, ctx=ctx).numpy(), "layer_norm 1")
            same(seg("qkv"), ql(seg("xn"), L.qkv), "qkv linear")
            qd = up(seg("qkv")[None])
            same(seg("mem"), K.depthwise_conv1d_tlc(qd, L.fsmn, None, 5, 5, x_offset=2 * D, add_input=True, ctx=ctx).numpy()[0], "memory block")
            with _env(LELE_HIP_ATTENTION_MIN_BLOCKS=1):
                av = K.attention_view(qd, QC, qd, KC, qd, VC, enc.scale, [0, 2, 1, 3], [0, 0, D], ctx=ctx).numpy()[0]
            close(seg("av"), av, tag + " attention")
            same(seg("att"), ql(seg("av"), L.out), "output projection")
            if L.d_in == D:
                same(seg("am"), K.add(up(seg("att")), up(seg("mem")), ctx=ctx).numpy(), "add memory")
                same(seg("x1"), K.add(up(seg("am")), up(seg("x")), ctx=ctx).numpy(), "add residual")
            else:
                same(seg("x1"), K.add(up(seg("att")), up(seg("mem")), ctx=ctx).numpy(), "add memory")
            same(seg("xn2"), K.layer_norm(up(seg("x1")), L.ln2[0], L.ln2[1], -1, 1e-5, ctx=ctx).numpy(), "layer_norm 2")
            same(seg("h"), ql(seg("xn2"), L.ffn1, True), "feed-forward 1")
            same(seg("h2"), ql(seg("h"), L.ffn2), "feed-forward 2")
            same(seg("y"), K.add(up(seg("x1")), up(seg("h2")), ctx=ctx).numpy(), "add feed-forward")
    hd = taps["head"]
    for s in range(len(E_LENGTHS)):
        a, b = int(off4[s]), int(off4[s + 1])
        np.testing.assert_array_equal(hd["xn"][a:b], K.layer_norm(up(hd["x"][a:b]), enc.ln_out[0], enc.ln_out[1], -1, 1e-5, ctx=ctx).numpy())
        np.testing.assert_array_equal(hd["logits"][a:b], ql(hd["xn"][a:b], enc.ctc))


@pytest.mark.gpu
def test_forward_segments_end_to_end_against_each_utterance_alone(ctx, enc3):
    from oracle import sensevoice_ref as R
    enc, arrays = enc3
    rng = np.random.default_rng(78)
    off = offsets_of(E_LENGTHS)
    f = _packed_feats(rng, E_LENGTHS)
    logits, off4 = enc.forward_segments(ctx.buf().upload(f), off)
    logits = logits.numpy()
    assert np.isfinite(logits).all()
    for s, ln in enumerate(E_LENGTHS):
        a, b = int(off4[s]), int(off4[s + 1])
        assert b - a == ln + 4
        if ln == 0:
            continue   # exactly its 4 prompt rows (finite, above); Encoder.forward takes no [1, 0, 560]
        alone = enc.forward(ctx.buf().upload(f[off[s]:off[s + 1]][None])).numpy()[0]
        r = logits_agreement(logits[a:b], alone)
        print("utterance %d (%d rows) packed vs alone: mae %.4g, arg-max agreement %.4f" % (s, ln, r["mae"], r["argmax_agreement"]))
        assert r["mae"] <= SV_MAX_MAE, (s, ln, r)
    s = E_LENGTHS.index(97)
    ref = R.encoder_forward(f[off[s]:off[s + 1]][None], arrays)[0]
    r = logits_agreement(logits[int(off4[s]):int(off4[s + 1])], ref)
    print("utterance %d (97 rows) packed vs oracle encoder: mae %.4g, arg-max agreement %.4f" % (s, r["mae"], r["argmax_agreement"]))
    assert r["mae"] <= SV_MAX_MAE, r


@pytest.mark.gpu
def test_forward_segments_from_pcm(ctx, enc3):
    from lele_amd.features import Cmvn, SenseVoiceFrontend
    enc, _ = enc3
    fe = SenseVoiceFrontend(ctx=ctx)
    sr = 16000
    pcm = synth_pcm(70 * sr, seed=31)
    secs = [5.5, 0.3, 30.0, 0.01, 12.25, 1.0]   # one shorter than a frame (160 samples); any order, overlaps allowed
    starts = [3, 20 * sr + 1, 35 * sr, 100, 8 * sr + 2, 66 * sr]
    segs = [(s, s + int(round(t * sr))) for s, t in zip(starts, secs)]
    feats, off = fe.compute_segments(pcm, segs)
    assert 0 in np.diff(off) and int(np.diff(off).max()) == 500
    norm = Cmvn(ctx=ctx).compute_segments(feats, off)
    logits, off4 = enc.forward_segments(norm, off)
    assert np.array_equal(off4, off + 4 * np.arange(len(off)))
    assert logits.shape == (int(off4[-1]), 25055) and np.isfinite(logits.numpy()).all()


@pytest.mark.gpu
def test_graph_capture_of_forward_segments_two_layouts(ctx):
    """recorded after one eager run: replay == eager bit for bit, and again after new features were uploaded into the same buffers,
    for two layouts alive at once (the shape of test_graph_capture_of_segments_cmvn_padding)"""
    from sensevoice_graph import Encoder
    enc = Encoder(ctx, layers=2, damped=True)
    rng = np.random.default_rng(79)
    layouts = [[171, 1, 33, 0, 300], [64, 97, 500]]
    bufs = [ctx.buf() for _ in layouts]
    feats = [b.upload(_packed_feats(rng, ln)) for b, ln in zip(bufs, layouts)]
    offs = [offsets_of(ln) for ln in layouts]
    eager = [enc.forward_segments(f, o)[0].numpy() for f, o in zip(feats, offs)]   # sizes the workspace, uploads both layouts' tables
    eager = [enc.forward_segments(f, o)[0].numpy() for f, o in zip(feats, offs)]   # (the workspace no longer grows)
    graphs = []

    def read(buf, shape):   # the workspace slot is shared by both layouts: its size is the last RECORDED call's, not the last replay's
        buf.reserve(4 * int(np.prod(shape)))   # (within its capacity: nothing moves)
        return buf.to_numpy(shape)

    for f, o in zip(feats, offs):
        ctx.graph_begin()
        res, _ = enc.forward_segments(f, o)
        graphs.append((ctx.graph_end(), (res.raw().buf, res.shape)))   # (a TensorView keeps its first host copy: read the buffer)
    for (g, (buf, shape)), e in zip(graphs, eager):
        buf.upload(np.zeros(shape, np.float32))   # the replay must write every logit itself
        g.launch()
        assert np.array_equal(read(buf, shape), e)
    for b, ln in zip(bufs, layouts):
        b.upload(_packed_feats(rng, ln) * np.float32(0.7))   # new features in the same buffers
    for (g, (buf, shape)), f, o, e in zip(graphs, feats, offs, eager):
        g.launch()
        replay = read(buf, shape)
        assert not np.array_equal(replay, e)
        assert np.array_equal(enc.forward_segments(f, o)[0].numpy(), replay)
    for g, _ in graphs:
        g.close()


@pytest.mark.gpu
def test_host_cpp_encoder_segments(tmp_path, ctx):
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    exe = _build_demo()
    rng = np.random.default_rng(9)
    lengths = [40, 0, 1, 130, 7]
    off = offsets_of(lengths)
    qkv = rng.standard_normal((int(off[-1]), 1536)).astype(np.float32)
    fsmn = (rng.standard_normal((D, 1, 11)) / np.sqrt(11)).astype(np.float32)
    w = np.clip(np.round(128 + 32 * rng.standard_normal((D, D))), 0, 255).astype(np.float32)
    ws = (np.abs(rng.standard_normal(D)) * 0.01 + 0.002).astype(np.float32)
    b = (rng.standard_normal(D) * 0.02).astype(np.float32)
    prefix = rng.standard_normal((4, 1536)).astype(np.float32)
    for name, arr in (("qkv.f32", qkv), ("off.i64", off), ("fsmn.f32", fsmn), ("w.f32", w), ("ws.f32", ws), ("b.f32", b), ("prefix.f32", prefix)):
        arr.tofile(tmp_path / name)
    r = subprocess.run([exe, "run", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    pre, off4 = K.segments_prepend(ctx.buf().upload(qkv), off, prefix, ctx=ctx)
    mem = K.depthwise_conv1d_tlc_segments(pre, off4, Weight(fsmn), None, 5, 5, x_offset=1024, add_input=True, ctx=ctx)
    att = K.attention_segments(pre, off4, H, DH, Weight(np.array([DH ** -0.5], np.float32)), ctx=ctx)
    lin = K.fused_quantized_linear_segments(att, off4, Weight(w), Weight(ws), Weight(np.array([128.0], np.float32)), Weight(b), ctx=ctx)
    assert np.array_equal(np.fromfile(tmp_path / "preoff.i64", np.int64), off4)
    for name, want in (("pre.f32", pre), ("mem.f32", mem), ("att.f32", att), ("lin.f32", lin)):
        assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(want.shape), want.numpy()), name
