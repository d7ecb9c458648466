"""Chunked streaming of the audio front-end: N live streams pushed chunk by chunk (lele_amd.features.FrontendStream over
lele_hip_frontend_stream_*), bit for bit the whole-utterance front-end.

The expected value for a stream is always the WHOLE-utterance result cut by the closed forms of include/lele_hip.h -- after L samples a
stream has T(L) frames and has emitted E(L) rows -- so there is no streaming oracle:

    CPU   the closed forms (lele_hip_frontend_stream_rows) against brute force on the oracle's shapes; a numpy emulation of the push
          (append / log-mel / emit / compact on the oracle's log-mel rows) that reproduces frontend_compute(concat) exactly for seeded
          random partitions, and five wrong variants of it that do not; the symbols; the route names, which the feature leaves alone.
    GPU   rows == fe.compute(concat) as uint32 for fixed chunk sizes, the LFR edge totals, five streams of different lengths in one
          object (== each stream alone), other configs (table mel loop, scalar emit, other LFR windows, a generic framing), the
          refusals (which leave `out` and the state untouched) and the C++ mirror.  Every push's row count and offsets equal the
          closed forms; on the default config the concatenation also meets the 2-ulp bar of tests/test_frontend_routes.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_frontend_routes import DEFAULT, FAMILIES, Frontends, cfg_of, family, framing, gather, is_fast, meets, truth_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GENERIC_8K = cfg_of(8000, 80)   # 200 / 80 / 512: the fused generic kernel
LFR_WINDOWS = ((1, 1), (4, 2), (5, 3), (7, 6), (3, 7))
# the parent's route names: the feature reports its log-mel launch with these and adds none
FE_ROUTE_NAMES = ["fe.main_std", "fe.main_table", "fe.seg_std", "fe.seg_table", "fe.generic_fused", "fe.generic_four", "fe.tile_dma",
                  "fe.tile_regs", "fe.tile_mixed", "fe.two_kernel"]
# every name the parent listed, in its order (158); families that learned to report their route since are added behind them, under the
# prefixes of LATER_PREFIXES: the resampler's, which reported without being listed, and the quantised linears' (tests/test_quant_routes.py)
PARENT_ROUTE_NAMES = [
    "gemm.thin_n", "gemm.thin_m", "gemm.small", "gemm.tile256x128", "gemm.tile128x128", "gemm.tile64x256", "gemm.tile64x64",
    "gemm.tile32x128", "gemm.k0", "conv.dw_lds_k3", "conv.dw_lds_k5", "conv.dw_lds_k7", "conv.dw_lds_k11", "conv.dw_lds_k3_direct",
    "conv.dw_lds_k5_direct", "conv.dw_lds_k7_direct", "conv.dw_lds_k11_direct", "conv.dw_row4_k3", "conv.dw_row4_k5", "conv.dw_row4_k7",
    "conv.dw_row4_k11", "conv.dw_generic", "conv.win3_oct32", "conv.win3_oct64", "conv.win3_oct32_osplit", "conv.win3_oct64_osplit",
    "conv.win1_oct32", "conv.win1_oct64", "conv.win1_oct128", "conv.win1_oct32_osplit", "conv.win1_oct64_osplit", "conv.win1_oct128_osplit",
    "conv.win3s2_oct32", "conv.win3s2_oct64", "conv.win3s2_oct32_osplit", "conv.win3s2_oct64_osplit", "conv.direct_ocb8_s1",
    "conv.direct_ocb16_s1", "conv.direct_ocb8_s2", "conv.direct_ocb16_s2", "conv.direct_ocb8_s1_passes", "conv.direct_ocb16_s1_passes",
    "conv.direct_ocb8_s2_passes", "conv.direct_ocb16_s2_passes", "conv.gemm_pw", "conv.gemm_tap", "conv.gemm_generic", "convt.ks",
    "convt.phase", "convt.phase_fill", "ci.f32", "ci8.codes", "ci8.quant", "ci8.nj4", "ci8.nj2", "ci8.nj1", "ci8.nj2_ksplit",
    "ci8.nj1_ksplit", "fsb.w1", "attn.flash", "attn.rows16", "attn.rows32", "attn.rows64", "attn.rows16_exact", "attn.rows32_exact",
    "attn.rows64_exact", "attn.nt2", "attn.nt4", "attn.nt6", "attn.nt8", "attn.nt10", "attn.nt12", "attn.nt14", "attn.nt16", "attn.seg",
    "attn.seg_exact", "copy.w4", "copy.w8", "copy.vec16", "copy.tile_w4", "copy.tile_w8", "copy.i64", "resize.up2", "resize.up4",
    "resize.up8", "resize.generic", "pool.lds", "pool.lds_sep", "pool.direct", "pool.direct_i64", "pool.pb1", "pool.pbn", "topk.rank",
    "topk.select_lds", "topk.select_l2", "cpitch.w16", "cpitch.w4", "cpitch.w1", "pad.index", "gather.rows", "gather.elements",
    "apool.window", "tcp.tile32", "range.f32", "range.i64", "fill.words", "cast.convert", "unary.vec4", "unary.w1", "bin.fast",
    "bin.flat_f32", "bin.index_f32", "bin.flat_i64", "bin.index_i64", "binp.vec4", "binp.w1", "where.index", "clip.w1", "reduce.seq",
    "reduce.rows16", "reduce.parts", "ln.reg8", "ln.reg16", "ln.reg32", "ln.stream", "softmax.reg8", "softmax.reg16", "softmax.reg32",
    "softmax.stream", "rows.rpb2", "rows.rpb4", "rows.rpb8", "rms.stream", "bn.w1", "add3.vec4", "add3.w1", "hpas.w1", "rnn.lstm",
    "rnn.gru", "rnns.lstm", "rnns.gru", "rnns.reg16", "rnns.reg32", "rnns.reg64", "rnns.stream1", "rnns.stream2", "rnns.stream4",
    "rnns.stream8", "fe.main_std", "fe.main_table", "fe.seg_std", "fe.seg_table", "fe.generic_fused", "fe.generic_four", "fe.tile_dma",
    "fe.tile_regs", "fe.tile_mixed", "fe.two_kernel"]
LATER_PREFIXES = ("resample.", "q.", "qffn.", "mmi.", "dql.", "igemm.", "as.", "rs.")
NEW_SYMBOLS = ["lele_hip_frontend_stream_rows", "lele_hip_frontend_stream_create", "lele_hip_frontend_stream_destroy",
               "lele_hip_frontend_stream_reset", "lele_hip_frontend_stream_counters", "lele_hip_frontend_stream_push"]


def fcfg(cfg):
    from lele_amd.features import FeatureConfig
    return FeatureConfig(*cfg)


def rows_of(cfg, before, chunk, final=False):
    from lele_amd.features import stream_rows
    return stream_rows(fcfg(cfg), before, chunk, final)


# --------------------------------------------------------------------------------------------------------------------- brute force
def brute_frames(cfg, total):
    """T(L) for L = 0 .. total, from the oracle's own shape function"""
    from oracle import pyoracle as O
    return np.array([O.frontend_shape(n, cfg[0], cfg[2], cfg[3], cfg[5])[1] for n in range(total + 1)], np.int64)


def brute_emitted(t, m, n):
    """rows i whose right-most frame i*n + m-1-pad exists among t frames, by counting"""
    pad = (m - 1) // 2
    return sum(1 for i in range(t + 1) if i * n + (m - 1 - pad) <= t - 1)


def ceil_div(a, b):
    return (a + b - 1) // b


# --------------------------------------------------------------------------------------------------------------------- CPU 1: closed forms
CLOSED_FORM_CONFIGS = [DEFAULT] + [cfg_of(m=m, n=n) for m, n in LFR_WINDOWS if (m, n) != (7, 6)] + [GENERIC_8K]


@pytest.mark.parametrize("cfg", CLOSED_FORM_CONFIGS, ids=lambda c: "x".join(str(v) for v in c))
def test_closed_forms_equal_brute_force(cfg):
    frame_len, hop, _ = framing(cfg)
    m, n = cfg[4], cfg[5]
    pad = (m - 1) // 2
    chunks = (0, 1, hop - 1, hop, hop + 1, frame_len, 1000)
    top = 3000
    T = brute_frames(cfg, top + max(chunks))
    E = np.array([brute_emitted(int(t), m, n) for t in range(int(T.max()) + 1)], np.int64)
    for L in range(top + 1):
        t, e = int(T[L]), int(E[T[L]])
        # the state after L samples, as one push from nothing reports it
        rows, new_frames, pcm_carry, mel_carry = rows_of(cfg, 0, L)
        assert (rows, new_frames) == (e, t), L
        assert pcm_carry == (L if t == 0 else L - t * hop) and 0 <= pcm_carry < frame_len, L
        assert mel_carry == max(0, t - max(0, e * n - pad)) and 0 <= mel_carry <= m - 1, L
        assert e <= ceil_div(t, n), L
        if cfg[4:] == (7, 6):
            assert e == ((t - 4) // 6 + 1 if t >= 4 else 0), L
        # a chunk boundary at L: the push behind it reports the differences, and the carries of the state it leaves
        for c in chunks:
            t2, e2 = int(T[L + c]), int(E[T[L + c]])
            assert rows_of(cfg, L, c) == (e2 - e, t2 - t) + rows_of(cfg, 0, L + c)[2:], (L, c)
        # the flush: what a final push (here an empty one) adds brings the stream to ceil(T/n) rows and leaves nothing behind
        assert rows_of(cfg, L, 0, True) == (ceil_div(t, n) - e, 0, 0, 0), L
        assert rows_of(cfg, 0, L, True) == (ceil_div(t, n), t, 0, 0), L
    # the sum over pushes plus the flush, for a walk through the whole range
    rng = np.random.default_rng(1)
    L = total = 0
    while L < top:
        c = int(rng.integers(0, 700))
        total += rows_of(cfg, L, c)[0]
        L += c
    assert total + rows_of(cfg, L, 0, True)[0] == ceil_div(int(T[L]), n) == ceil_div(rows_of(cfg, 0, L)[1], n)


# --------------------------------------------------------------------------------------------------------------------- CPU 2, 3: emulation
class Emulation:
    """One stream of the push algorithm in numpy: a PCM region (carried samples, then the chunk), a log-mel region (carried rows, then the
    new frames' rows, computed by the oracle from the region alone), the emit gather and the compaction of both -- with the counters
    L, T, E as the closed forms give them.  `wrong` names one deliberate mistake."""

    def __init__(self, cfg, wrong=None):
        self.cfg, self.wrong = cfg, wrong
        self.frame_len, self.hop, _ = framing(cfg)
        self.m, self.n = cfg[4], cfg[5]
        self.pad = (self.m - 1) // 2
        self.reset()

    def reset(self):
        self.L = self.T = self.E = 0
        self.pcm = np.zeros(0, F32)
        self.mel = np.zeros((0, self.cfg[1]), F32)
        self.mel_base = 0   # global index of the frame in row 0 of the log-mel region

    def emitted(self, t):
        k = self.m - 1 - self.pad - (1 if self.wrong == "row one frame early" else 0)
        return (t - 1 - k) // self.n + 1 if t - 1 >= k else 0

    def push(self, chunk, final=False):
        from oracle import pyoracle as O
        cfg = self.cfg
        # append
        region = np.concatenate([self.pcm, np.asarray(chunk, F32)])
        L2 = self.L + len(chunk)
        T2 = 0 if L2 < self.frame_len else (L2 - self.frame_len) // self.hop + 1
        nf = T2 - self.T
        # log-mel of the region's frames (frame j of them at j * hop), behind the carried rows
        if nf:
            new = O.frontend_compute(region, *cfg, return_mel=True)[1]
            assert new.shape[0] == nf
            self.mel = np.concatenate([self.mel, new])
        first_new = self.T
        # emit
        total = ceil_div(T2, self.n)
        E2 = total if final or self.wrong == "right clamp at every push" else min(self.emitted(T2), total)
        out = []
        for i in range(self.E, E2):
            g = i * self.n + np.arange(self.m) - self.pad
            g = np.maximum(g, first_new if self.wrong == "left clamp at every push" else 0)
            if final or self.wrong in ("right clamp at every push", "row one frame early"):
                g = np.minimum(g, T2 - 1)
            assert g.max() <= T2 - 1
            r = np.maximum(g - self.mel_base, 0)   # (a frame that was not carried: only a wrong variant gets here; it reads row 0)
            out.append(self.mel[r].reshape(-1))
        # compact
        if final:
            self.reset()
        else:
            carry = L2 if T2 == 0 else L2 - T2 * self.hop
            self.pcm = region[len(region) - carry:].copy()
            if self.wrong == "frame_len - hop - 1 samples carried":   # the oldest samples beyond that capacity are lost
                lost = max(0, carry - (self.frame_len - self.hop - 1))
                self.pcm[:lost] = 0
            keep = max(0, T2 - max(0, E2 * self.n - self.pad))
            if self.wrong == "m - 2 rows carried":
                keep = min(keep, self.m - 2)
            self.mel_base = T2 - keep
            self.mel = self.mel[len(self.mel) - keep:].copy()
            self.L, self.T, self.E = L2, T2, E2
        return np.stack(out) if out else np.zeros((0, cfg[1] * self.m), F32)


def partitions(total, seed, count=3, top=2500):
    """seeded random cuts of `total` samples into chunks of 0 .. top, zero-length chunks included"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        cuts, at = [], 0
        hi = (400, 1000, top)[k % 3]
        while at < total:
            c = min(int(rng.integers(0, hi + 1)), total - at)
            cuts.append(c)
            at += c
        yield cuts


EMU_CASES = [(DEFAULT, 4000), (DEFAULT, 10641), (cfg_of(m=4, n=2), 3000), (cfg_of(m=5, n=3), 3000), (cfg_of(m=1, n=1), 2000), (cfg_of(m=3, n=7), 5000),
             (GENERIC_8K, 2000), (DEFAULT, 399), (DEFAULT, 1000)]


def emulate(cfg, x, cuts, wrong=None, final_with_last=True):
    emu = Emulation(cfg, wrong)
    got, at = [], 0
    for k, c in enumerate(cuts):
        got.append(emu.push(x[at:at + c], final=final_with_last and k == len(cuts) - 1))
        at += c
    if not final_with_last:
        got.append(emu.push(x[:0], final=True))
    return np.concatenate(got)


@functools.lru_cache(maxsize=None)
def emu_case(cfg, total):
    from oracle import pyoracle as O
    x = family("synth", total, 3)
    want = O.frontend_compute(x, *cfg)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want.reshape(-1, cfg[1] * cfg[4])


def test_emulated_push_reproduces_the_whole_utterance(orc):
    for cfg, total in EMU_CASES:
        x, want = emu_case(cfg, total)
        for k, cuts in enumerate(partitions(total, seed=total)):
            got = emulate(cfg, x, cuts, final_with_last=k % 2 == 0)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cfg, total, cuts)


@pytest.mark.parametrize("wrong", ["row one frame early", "m - 2 rows carried", "right clamp at every push", "left clamp at every push",
                                   "frame_len - hop - 1 samples carried"])
def test_wrong_variants_differ_from_the_whole_utterance(orc, wrong):
    differs = 0
    for cfg, total in EMU_CASES:
        x, want = emu_case(cfg, total)
        for cuts in partitions(total, seed=total):
            got = emulate(cfg, x, cuts, wrong)
            differs += not (got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    assert differs >= 1, wrong


# --------------------------------------------------------------------------------------------------------------------- CPU 4: symbols, routes
def test_new_symbols_are_declared_and_exported():
    import ctypes as C
    from lele_amd import _lib
    declared = _lib.exported_symbols()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    assert "class FrontendStream" in hpp and all(n in hpp for n in NEW_SYMBOLS)


def test_route_names_are_the_parents():
    from lele_amd import kernels as K
    names = K.route_names()
    assert [s for s in names if s.startswith("fe.")] == FE_ROUTE_NAMES
    assert len(PARENT_ROUTE_NAMES) == 158 and not [s for s in PARENT_ROUTE_NAMES if s.startswith(LATER_PREFIXES)]
    assert [s for s in names if not s.startswith(LATER_PREFIXES)] == PARENT_ROUTE_NAMES


def test_stream_rows_refuses_bad_arguments():
    from lele_amd._lib import LeleError
    with pytest.raises(LeleError):
        rows_of(DEFAULT, -1, 10)
    with pytest.raises(LeleError):
        rows_of(DEFAULT, 0, -1)
    with pytest.raises(LeleError):
        rows_of(cfg_of(m=0), 0, 10)


# --------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def fes(ctx):
    return Frontends(ctx)


_whole = {}


def whole(fes, cfg, fam, total, seed=0):
    """(pcm, fe.compute(pcm) or None when it has no frame), once a case; never written again"""
    key = (cfg, fam, total, seed)
    if key not in _whole:
        x = family(fam, total, seed)
        got = fes.get(cfg).compute(x)
        want = None if got.shape == () else got.numpy().copy()
        x.setflags(write=False)
        if want is not None:
            want.setflags(write=False)
        _whole[key] = (x, want)
    return _whole[key]


def expected_route(cfg, lens):
    """lens: carry + chunk of every stream that gained a frame this push (the regions start 16-byte aligned)"""
    if not lens:
        return ""
    if not is_fast(cfg):
        return "fe.generic_fused"
    dma = [ln % 4 == 0 for ln in lens]
    return ("fe.seg_std" if cfg[1] == 80 else "fe.seg_table") + "/" + ("fe.tile_dma" if all(dma) else "fe.tile_mixed" if any(dma) else "fe.tile_regs")


class Driver:
    """pushes a schedule through a FrontendStream and holds every push to the closed forms: its row count, its offsets, its route"""

    def __init__(self, fes, cfg, streams, max_chunk):
        from lele_amd.features import FrontendStream
        self.ctx, self.cfg = fes.ctx, cfg
        self.st = FrontendStream(fes.get(cfg), streams, max_chunk)
        self.seen = [0] * streams
        self.got = [[] for _ in range(streams)]
        self.routes = set()

    def push(self, chunks, final=None, as_device=False):
        from lele_amd import kernels as K
        final = [False] * len(chunks) if final is None else list(final)
        want_rows, lens = [], []
        for i, (c, f) in enumerate(zip(chunks, final)):
            rows, nf, _, _ = rows_of(self.cfg, self.seen[i], len(c), f)
            carry = rows_of(self.cfg, 0, self.seen[i])[2]
            want_rows.append(rows)
            if nf:
                lens.append(carry + len(c))
        if as_device:
            from lele_amd.features import pack
            pcm, segs = pack(chunks)
            dev = self.ctx.buf().upload(pcm if len(pcm) else np.zeros(1, F32))
            arg = (dev, [s for s, _ in segs], [e - s for s, e in segs])
        else:
            arg = list(chunks)
        out, off = self.st.push(arg, final if any(final) else None)
        route = K.last_route(self.ctx)
        assert route == expected_route(self.cfg, lens), (route, lens)
        self.routes.add(route)
        assert list(off) == [0] + list(np.cumsum(want_rows)), (list(off), want_rows)
        if off[-1] == 0:
            assert out.shape == ()
        else:
            rows = out.numpy()
            assert rows.shape == (off[-1], self.cfg[1] * self.cfg[4])
            for i in range(len(chunks)):
                if off[i + 1] > off[i]:
                    self.got[i].append(rows[off[i]:off[i + 1]].copy())
        for i, (c, f) in enumerate(zip(chunks, final)):
            self.seen[i] = 0 if f else self.seen[i] + len(c)
        assert list(self.st.samples_seen) == self.seen
        return out, off

    def rows(self, i):
        return np.concatenate(self.got[i]) if self.got[i] else None


def same_bits(got, want):
    if want is None or got is None:
        return want is None and got is None
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def feed(drv, x, size, final_with_last=True):
    """one stream: x in chunks of `size`"""
    for at in range(0, len(x), size):
        drv.push([x[at:at + size]], [final_with_last and at + size >= len(x)])
    if not final_with_last or len(x) == 0:
        drv.push([x[:0]], [True])


CHUNK_SIZES = (1, 159, 160, 161, 239, 240, 399, 400, 401, 560, 1600, 10640, 20960)


@pytest.mark.gpu
@pytest.mark.parametrize("size", CHUNK_SIZES)
def test_fixed_chunk_sizes_equal_compute(fes, orc, size):
    """one stream, 20960 samples = 129 frames (10640 and 20960 a push span two and three 64-frame blocks); sample by sample for the first
    1000 only.  Every input family of tests/test_frontend_routes.py takes its turn."""
    fam = FAMILIES[CHUNK_SIZES.index(size) % len(FAMILIES)]
    total = 1000 if size == 1 else 20960
    x, want = whole(fes, DEFAULT, fam, total)
    drv = Driver(fes, DEFAULT, 1, size)
    feed(drv, x, size, final_with_last=size % 2 == 0)
    got = drv.rows(0)
    assert same_bits(got, want)
    # the existing bar of the front-end, against the oracle: 2 ulp on the log, the LFR an exact gather of the front-end's own log-mel rows
    _, mel, energy = orc.frontend_compute(x, *DEFAULT, return_energy=True)
    assert meets(got, gather(truth_of(energy), 7, 6))
    assert np.array_equal(got, gather(fes.get(DEFAULT).logmel(x).numpy(), 7, 6))
    if size in (160, 400, 560, 1600):   # carry + chunk stays a multiple of 4 (or not) for the whole run
        assert drv.routes - {""} == {"fe.seg_std/fe.tile_dma"}
    if size in (159, 161, 401):
        assert {"fe.seg_std/fe.tile_dma", "fe.seg_std/fe.tile_regs"} <= drv.routes


@pytest.mark.gpu
@pytest.mark.parametrize("frames", (0, 1, 3, 4, 5, 6, 7, 9, 10, 12, 13))
def test_lfr_edge_totals_equal_compute(fes, frames):
    """few frames: rows that clamp on both sides, a flush that emits every row, a flush that emits none; with samples that complete no
    frame behind the last one"""
    total = 399 if frames == 0 else 400 + (frames - 1) * 160 + 7
    x, want = whole(fes, DEFAULT, "synth", total, seed=frames)
    assert (0 if want is None else want.shape[0]) == ceil_div(frames, 6)
    one = Driver(fes, DEFAULT, 1, total)
    one.push([x], [True])
    assert same_bits(one.rows(0), want)
    assert list(one.st.frames_seen) == [0] and list(one.st.rows_emitted) == [0]   # a final push leaves the stream reset
    many = Driver(fes, DEFAULT, 1, 100)
    feed(many, x, 100, final_with_last=False)
    assert same_bits(many.rows(0), want)


def schedule_of(lengths, seed, top=2500):
    """per stream the chunk lengths of every push (0 .. top, zeros and odd values included; a stream's last chunk is final, after it: 0)"""
    rng = np.random.default_rng(seed)
    left = list(lengths)
    pushes = []
    while any(v is not None for v in left):
        row = []
        for i, v in enumerate(left):
            if v is None:
                row.append((0, False))
                continue
            c = min(int(rng.integers(0, top + 1)), v)
            left[i] = v - c
            done = left[i] == 0 and (v == 0 or rng.integers(0, 2) == 0 or c == 0)
            row.append((c, bool(done)))
            if done:
                left[i] = None
        pushes.append(row)
    return pushes


@pytest.mark.gpu
def test_several_streams_equal_each_stream_alone(fes):
    lengths = (0, 399, 2000, 10641, 20960)
    second = 5000   # slot 1's second utterance, after a reset that abandons the first
    xs = [whole(fes, DEFAULT, "synth", n, seed=10 + i) for i, n in enumerate(lengths)]
    x2, want2 = whole(fes, DEFAULT, "wide", second, seed=2)
    pushes = schedule_of(lengths, seed=7)
    assert len({k for k, row in enumerate(pushes) for c, f in row if f}) >= 3    # streams finish at different pushes
    assert any(c == 0 for row in pushes for c, f in row) and any(c % 2 for row in pushes for c, f in row)
    drv = Driver(fes, DEFAULT, 5, 2500)
    single = [Driver(fes, DEFAULT, 1, 2500) for _ in lengths]
    at = [0] * 5
    at2, reset_at = 0, 2
    rng = np.random.default_rng(8)
    for k, row in enumerate(pushes + [[(0, False)] * 5] * 4):
        chunks, final = [], []
        for i, (c, f) in enumerate(row):
            if i == 1:
                if k < reset_at:          # the first utterance of slot 1: 399 samples, never finished
                    c = min(c, 399 - at[1]) if k + 1 < reset_at else 399 - at[1]
                    chunks.append(xs[1][0][at[1]:at[1] + c])
                    at[1] += c
                    final.append(False)
                else:                      # ... abandoned: the slot takes a second utterance while the others continue
                    c = min(int(rng.integers(0, 2501)), second - at2)
                    chunks.append(x2[at2:at2 + c])
                    at2 += c
                    final.append(k == len(pushes) + 3)   # with the last push of the run, an empty one
                continue
            chunks.append(xs[i][0][at[i]:at[i] + c])
            at[i] += c
            final.append(f)
        if k == reset_at:
            assert drv.st.samples_seen[1] == 399
            drv.st.reset([1])
            drv.seen[1] = 0
            single[1].st.reset()
            single[1].seen[0] = 0
        drv.push(chunks, final, as_device=k % 3 == 1)
        for i in range(5):
            single[i].push([chunks[i]], [final[i]])
    assert at2 == second and at[2:] == list(lengths[2:])
    assert "fe.seg_std/fe.tile_mixed" in drv.routes
    for i in range(5):
        want = want2 if i == 1 else xs[i][1]
        assert same_bits(drv.rows(i), want), i
        assert same_bits(single[i].rows(0), drv.rows(i)), i    # packed == single, bit for bit
    assert xs[0][1] is None and xs[1][1] is None


OTHER_CONFIGS = [
    (cfg_of(nm=40), "fe.seg_table", 10641),        # the table-driven mel loop
    (cfg_of(nm=23), "fe.seg_table", 4000),         # n_mels % 4 != 0: the scalar emit
    (cfg_of(m=1, n=1), "fe.seg_std", 4000),        # no LFR window: nothing is carried in the log-mel region
    (cfg_of(m=4, n=2), "fe.seg_std", 4000),
    (cfg_of(m=3, n=7), "fe.seg_std", 6000),        # a shift longer than the window: frames no row reads
    (cfg_of(nm=40, m=20, n=3), "fe.seg_table", 6000),   # 19 carried rows
    (GENERIC_8K, "fe.generic_fused", 3000),        # another framing: the generic kernels once a stream
    (cfg_of(16000, 40, 20.0, 8.0), "fe.generic_fused", 3001),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,kernel,total", OTHER_CONFIGS, ids=["x".join(str(v) for v in c[0]) for c in OTHER_CONFIGS])
def test_other_configs_equal_compute(fes, cfg, kernel, total):
    xs = [whole(fes, cfg, "synth", total, seed=1), whole(fes, cfg, "wide", total - 161, seed=2)]
    drv = Driver(fes, cfg, 2, 1200)
    at = [0, 0]
    cuts = [list(next(partitions(len(x), seed=5 + i, count=1, top=1200))) for i, (x, _) in enumerate(xs)]
    for k in range(max(len(c) for c in cuts)):
        chunks, final = [], []
        for i, (x, _) in enumerate(xs):
            c = cuts[i][k] if k < len(cuts[i]) else 0
            chunks.append(x[at[i]:at[i] + c])
            at[i] += c
            final.append(k == len(cuts[i]) - 1)
        drv.push(chunks, final)
    for i, (x, want) in enumerate(xs):
        assert want is not None and same_bits(drv.rows(i), want), i
    assert drv.routes - {""} and all(r.split("/")[0] == kernel for r in drv.routes - {""}), drv.routes


@pytest.mark.gpu
def test_refusals_leave_out_and_state_untouched(fes, ctx):
    from lele_amd._lib import LeleError
    x, want = whole(fes, DEFAULT, "synth", 4000, seed=21)
    ref = Driver(fes, DEFAULT, 2, 2100)      # what the valid pushes give without anything refused between them
    drv = Driver(fes, DEFAULT, 2, 2100)
    first = [x[:1000], x[:640]]
    for d in (ref, drv):
        d.push(first)
    before = drv.st._out.to_numpy((int(drv.st._out.nbytes) // 4,), F32)   # the first push's one row
    assert before.shape == (560,)
    state = (list(drv.st.samples_seen), list(drv.st.frames_seen), list(drv.st.rows_emitted))
    assert state == ([1000, 640], [4, 2], [1, 0])

    def out_untouched():
        return drv.st._out.nbytes == 4 * len(before) and np.array_equal(drv.st._out.to_numpy((len(before),), F32).view(np.uint32), before.view(np.uint32))

    def refused(call, read_out=True):
        with pytest.raises(LeleError):
            call()
        assert (list(drv.st.samples_seen), list(drv.st.frames_seen), list(drv.st.rows_emitted)) == state
        assert not read_out or out_untouched()

    refused(lambda: drv.st.push([x[:2101], x[:10]]))                                  # a chunk above max_chunk
    refused(lambda: drv.st.push((x, [0, 3500], [100, 501])))                           # a range outside pcm
    refused(lambda: drv.st.push((x, [-1, 0], [100, 100])))
    refused(lambda: drv.st.push([x[:10]]))                                             # one chunk for two streams
    ctx.graph_begin()
    try:
        refused(lambda: drv.st.push([x[1000:2000], x[640:1000]]), read_out=False)      # a push while the context records a graph
    finally:
        ctx.graph_abort()
    assert out_untouched()   # (read after the recording has ended: reading a buffer back drains the stream)
    # the next valid pushes give what they would have given; a device tensor and a host array as pcm give the same bits
    rest = [([x[1000:2000], x[640:1000]], [False, False]), ([x[2000:3000], x[1000:1999]], [False, False]), ([x[3000:], x[1999:4000]], [True, True])]
    for k, (chunks, final) in enumerate(rest):
        a, _ = ref.push(chunks, final)
        b, _ = drv.push(chunks, final, as_device=True)
        assert a.shape == b.shape and (a.shape == () or np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))), k
    for d in (ref, drv):
        assert same_bits(d.rows(0), want) and same_bits(d.rows(1), want)
    # a frame shift longer than the frame (160 / 400 samples) would have to drop samples between two frames: refused when the stream is made
    from lele_amd.features import FrontendStream
    with pytest.raises(LeleError, match="longer than the frame"):
        FrontendStream(fes.get(cfg_of(16000, 80, 10.0, 25.0)), 1, 1000)


# --------------------------------------------------------------------------------------------------------------------- the C++ mirror
def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "frontend_stream_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "frontend_stream_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_stream_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr
    # the closed forms through the mirror: `rows` prints stream_rows of the default config
    r = subprocess.run([_build_demo(), "rows", "400", "480", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["ROWS"] + [str(v) for v in rows_of(DEFAULT, 400, 480)], r.stdout + r.stderr


@pytest.mark.gpu
def test_host_cpp_stream_demo_equals_python(fes, tmp_path):
    exe = _build_demo()
    x, want = whole(fes, DEFAULT, "synth", 10641, seed=4)
    cuts = np.array([0, 1601, 1601 + 7000, 10641], np.int64)   # three chunks, the last one final
    paths = [tmp_path / n for n in ("pcm.f32", "cuts.i64", "feats.f32", "counts.i64")]
    x.tofile(paths[0])
    cuts.tofile(paths[1])
    r = subprocess.run([exe, "run"] + [str(p) for p in paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    drv = Driver(fes, DEFAULT, 1, 7000)
    counts = []
    for k in range(3):
        _, off = drv.push([x[cuts[k]:cuts[k + 1]]], [k == 2])
        counts.append(int(off[-1]))
    assert list(np.fromfile(paths[3], np.int64)) == counts
    got = np.fromfile(paths[2], F32).reshape(-1, 560)
    assert same_bits(got, drv.rows(0)) and same_bits(got, want)
