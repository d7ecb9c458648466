"""Variable-length audio through the front-end in one launch: SenseVoiceFrontend.compute_segments over (start, end) ranges of one PCM
buffer, the per-segment CMVN after it and the padded [B, T, D] + lengths form (include/lele_hip.h: lele_hip_frontend_compute_segments,
lele_hip_cmvn_segments, lele_hip_segments_to_padded).  Every segment's rows must be what compute() gives for that range alone, bit
for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import synth_pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-4, 1e-6
SR = 16000


def _check_segments(fe, pcm, segs, feats, offsets):
    assert offsets.shape == (len(segs) + 1,) and offsets[0] == 0
    f = feats.numpy() if offsets[-1] > 0 else None
    for i, (s, e) in enumerate(segs):
        rows, cols, _ = fe.out_rows(e - s)
        assert offsets[i + 1] - offsets[i] == rows, (i, s, e)
        if rows == 0:
            continue
        want = fe.compute(pcm[s:e]).numpy()
        assert np.array_equal(f[offsets[i]:offsets[i + 1]], want), (i, s, e)


# ---------------------------------------------------------------------------------------------------- CPU: interface and helpers
def test_segment_entry_points_are_declared_and_exported():
    from lele_amd import _lib
    names = ("lele_hip_frontend_compute_segments", "lele_hip_cmvn_segments", "lele_hip_segments_to_padded")
    assert set(names) <= set(_lib.exported_symbols())
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n


def test_pack_builds_one_buffer_and_its_segments():
    from lele_amd.features import pack
    parts = [np.arange(5, dtype=np.float32), np.zeros(0, np.float32), np.ones(3, np.float32)]
    pcm, segs = pack(parts)
    assert pcm.dtype == np.float32 and pcm.shape == (8,)
    assert segs == [(0, 5), (5, 5), (5, 8)]
    for p, (s, e) in zip(parts, segs):
        assert np.array_equal(pcm[s:e], p)
    pcm, segs = pack([])
    assert pcm.shape == (0,) and segs == []


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def fe(ctx):
    from lele_amd.features import SenseVoiceFrontend
    return SenseVoiceFrontend(ctx=ctx)


@pytest.mark.gpu
def test_segments_bit_identical_to_compute(fe, orc):
    lengths = [0, 1, 399, 400, 401, 559, 560, 561, 1359, 1360, 16000, 48123, 160000]
    rng = np.random.default_rng(3)
    n = 600000
    pcm = synth_pcm(n, seed=11)
    segs = []
    for i, ln in enumerate(lengths):
        base = int(rng.integers(0, n - ln - 8)) & ~3
        segs.append((base + i % 4, base + i % 4 + ln))  # starts = 0, 1, 2, 3 (mod 4)
    order = rng.permutation(len(segs))
    segs = [segs[i] for i in order]
    s0, e0 = segs[-1]
    segs.append((s0 + (e0 - s0) // 2, s0 + (e0 - s0) // 2 + 20000))  # overlaps the last range
    segs.append(segs[3])  # a duplicate
    feats, offsets = fe.compute_segments(pcm, segs)
    _check_segments(fe, pcm, segs, feats, offsets)
    f = feats.numpy()
    for i, (s, e) in enumerate(segs):
        if offsets[i + 1] > offsets[i]:
            ref = orc.frontend_compute(pcm[s:e])
            np.testing.assert_allclose(f[offsets[i]:offsets[i + 1]], ref, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", [(5, 16000), (64, 30 * SR)])
def test_equal_contiguous_segments_equal_compute_batch(fe, batch, n):
    from lele_amd.features import pack
    parts = [synth_pcm(n, seed=100 + b) for b in range(batch)]
    pcm, segs = pack(parts)
    feats, offsets = fe.compute_segments(pcm, segs)
    want = fe.compute_batch(pcm.reshape(batch, n)).numpy()
    t = want.shape[1]
    assert np.array_equal(offsets, np.arange(batch + 1) * t)
    assert np.array_equal(feats.numpy(), want.reshape(batch * t, -1))


def _vad_recording(minutes=10, seed=5):
    """a seeded synthetic recording with speech-like bursts, and Silero-style per-chunk probabilities for it"""
    rng = np.random.default_rng(seed)
    n = minutes * 60 * SR
    chunk = 512
    probs = np.zeros(n // chunk, np.float32)
    i = int(rng.integers(0, 50))
    while i < len(probs):
        speech = int(rng.uniform(0.4, 25.0) * SR / chunk)
        probs[i:i + speech] = rng.uniform(0.5, 1.0, size=len(probs[i:i + speech]))
        i += speech + int(rng.uniform(0.8, 3.0) * SR / chunk)
    pcm = synth_pcm(n, seed=seed) * np.repeat(np.maximum(probs, 0.02), chunk)[:n].astype(np.float32)
    return pcm.astype(np.float32), probs, chunk


@pytest.mark.gpu
def test_vad_shaped_recording_full_size(fe):
    from lele_amd.apps import vad_segments
    pcm, probs, chunk = _vad_recording()
    segs = [(int(s), int(e)) for s, e in vad_segments(probs, chunk, len(probs) * chunk, len(pcm))]
    assert 30 <= len(segs) <= 120, len(segs)
    assert min(e - s for s, e in segs) >= int(0.4 * SR) and max(e - s for s, e in segs) <= 31 * SR
    feats, offsets = fe.compute_segments(pcm, segs)
    _check_segments(fe, pcm, segs, feats, offsets)


@pytest.mark.gpu
def test_empty_and_short_segment_lists(fe):
    pcm = synth_pcm(4000, seed=2)
    feats, offsets = fe.compute_segments(pcm, [])
    assert feats.shape == () and np.array_equal(offsets, [0])
    feats, offsets = fe.compute_segments(pcm, [(0, 0), (10, 409), (100, 399)])
    assert feats.shape == () and np.array_equal(offsets, [0, 0, 0, 0])


@pytest.mark.gpu
def test_invalid_segments_raise_and_leave_out_untouched(ctx, fe):
    import lele_amd
    pcm = synth_pcm(20000, seed=6)
    out = ctx.buf()
    good, _ = fe.compute_segments(pcm, [(0, 16000)], out=out)
    shape = good.shape
    before = out.to_numpy(shape).copy()
    for bad in ([(0, 16000), (-1, 500)], [(100, 50)], [(19000, 20001)], [(0, 16000), (20000, 20001)]):
        with pytest.raises(lele_amd.LeleError, match="outside"):
            fe.compute_segments(pcm, bad, out=out)
    with pytest.raises(lele_amd.LeleError, match="f32"):
        fe.compute_segments(pcm.astype(np.int32), [(0, 16000)], out=out)
    with pytest.raises(lele_amd.LeleError, match="f32"):
        fe.compute_segments(pcm.reshape(2, -1), [(0, 5000)], out=out)
    assert np.array_equal(out.to_numpy(shape), before)


@pytest.mark.gpu
def test_generic_config_segments_equal_per_segment_compute(ctx):
    from lele_amd.features import FeatureConfig, SenseVoiceFrontend
    fe8 = SenseVoiceFrontend(FeatureConfig(sample_rate=8000, n_mels=40), ctx=ctx)
    pcm = synth_pcm(8000 * 20, seed=8)
    segs = [(3, 8000 * 5 + 3), (0, 150), (1001, 1001 + 8000 * 3 + 7), (2, 8000 * 20), (50000, 50000 + 401)]
    feats, offsets = fe8.compute_segments(pcm, segs)
    _check_segments(fe8, pcm, segs, feats, offsets)


@pytest.mark.gpu
def test_cmvn_segments_equal_cmvn_per_segment(ctx, fe):
    from lele_amd.features import Cmvn
    pcm = synth_pcm(200000, seed=9)
    segs = [(0, 48000), (7, 407), (50001, 50001 + 16000), (3, 100), (60000, 60000 + 1359), (1000, 1000 + 33333)]
    feats, offsets = fe.compute_segments(pcm, segs)
    assert 1 in np.diff(offsets) and 0 in np.diff(offsets)
    got = Cmvn(ctx=ctx).compute_segments(feats, offsets).numpy()
    f = feats.numpy()
    for i in range(len(segs)):
        a, b = offsets[i], offsets[i + 1]
        if b > a:
            assert np.array_equal(got[a:b], Cmvn(ctx=ctx).compute(f[a:b]).numpy()), i


@pytest.mark.gpu
@pytest.mark.parametrize("t_max", [0, 120])
def test_segments_to_padded_matches_numpy(ctx, t_max):
    from lele_amd import kernels as K
    rng = np.random.default_rng(4)
    lens = [5, 0, 17, 1, 90]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.standard_normal((int(off[-1]), 560)).astype(np.float32)
    y, lengths = K.segments_to_padded(x, off, t_max=t_max, pad=-7.5, ctx=ctx)
    t = t_max or max(lens)
    want = np.full((len(lens), t, 560), -7.5, np.float32)
    for b, ln in enumerate(lens):
        want[b, :ln] = x[off[b]:off[b + 1]]
    assert np.array_equal(lengths, lens)
    assert np.array_equal(y.numpy(), want)


@pytest.mark.gpu
def test_graph_capture_of_segments_cmvn_padding(ctx, fe):
    from lele_amd import kernels as K
    from lele_amd.features import Cmvn
    rng = np.random.default_rng(12)
    n = 120000
    pcm_buf = ctx.buf()
    pcm = pcm_buf.upload(synth_pcm(n, seed=13))
    cm = Cmvn(ctx=ctx)
    layouts = [[(0, 16000), (20001, 20001 + 48123), (5, 405), (70002, 70002 + 31999)],
               [(3, 3 + 100000), (1, 1 + 1360), (40000, 40000 + 561)]]
    graphs, outs, eager = [], [], []
    for segs in layouts:
        o1, o2, o3 = ctx.buf(), ctx.buf(), ctx.buf()

        def seq(segs=segs, o1=o1, o2=o2, o3=o3):
            f, off = fe.compute_segments(pcm, segs, out=o1)
            c = cm.compute_segments(f, off, out=o2)
            p, _ = K.segments_to_padded(c, off, out=o3, ctx=ctx)
            return p

        e = seq().numpy()  # sizes the buffers and uploads the layout's tables
        ctx.graph_begin()
        res = seq()
        graphs.append((ctx.graph_end(), seq))
        outs.append((o3, res.shape))
        eager.append(e)
    for (g, _), (o3, shape), e in zip(graphs, outs, eager):
        g.launch()
        assert np.array_equal(o3.to_numpy(shape), e)
    pcm_buf.upload((0.5 * rng.standard_normal(n)).astype(np.float32))  # new audio in the same buffer
    for (g, seq), (o3, shape), e in zip(graphs, outs, eager):
        g.launch()
        replay = o3.to_numpy(shape)
        assert not np.array_equal(replay, e)
        assert np.array_equal(seq().numpy(), replay)
    for g, _ in graphs:
        g.close()


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "segments_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "segments_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_segments_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


@pytest.mark.gpu
def test_host_cpp_compute_segments(tmp_path, ctx, fe):
    from lele_amd.features import Cmvn
    exe = _build_demo()
    pcm = synth_pcm(100000, seed=21)
    segs = [(1, 1 + 48000), (30000, 30000 + 16003), (2, 300), (60006, 60006 + 401)]
    paths = [tmp_path / p for p in ("pcm.f32", "segs.i64", "feats.f32", "cmvn.f32", "off.i64")]
    pcm.tofile(paths[0])
    np.asarray(segs, np.int64).tofile(paths[1])
    r = subprocess.run([exe, "run"] + [str(p) for p in paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    want, want_off = fe.compute_segments(pcm, segs)
    off = np.fromfile(paths[4], np.int64)
    assert np.array_equal(off, want_off)
    feats = np.fromfile(paths[2], np.float32).reshape(want.shape)
    assert np.array_equal(feats, want.numpy())
    assert np.array_equal(np.fromfile(paths[3], np.float32).reshape(want.shape), Cmvn(ctx=ctx).compute_segments(want, off).numpy())
