"""Audio resampling on the device (include/lele_hip.h "audio resampling", lele_amd/csrc/resample.hip): features.Resampler and
features.ResamplerStream against the host halves in lele_amd/apps.py.

    CPU   the symbols; apps.resample_linear by hand; lele_hip_resampler_out_len against the reference's length and the sinc formula,
          whole and split at every cut; the uploaded table; the filter's quality on the float64 table; the sinc bound rejects wrong
          kernels.
    GPU   linear bit for bit, sinc within gamma_T * sum|h x| + 1 ulp, on a packed layout of awkward lengths in a NaN-filled buffer; live
          equals batch bit for bit for four cuts; validation; Resampler -> front-end end to end, packed and live; graph capture.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["lele_hip_resampler_create", "lele_hip_resampler_destroy", "lele_hip_resampler_table", "lele_hip_resampler_out_len",
               "lele_hip_resample_segments", "lele_hip_resampler_stream_create", "lele_hip_resampler_stream_destroy",
               "lele_hip_resampler_stream_reset", "lele_hip_resampler_stream_counters", "lele_hip_resampler_stream_push"]
LEN_PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (44100, 16000), (48000, 16000), (16000, 8000)]
LENGTHS = list(range(2001)) + [479999, 480000, 480001]
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def host_rs(fr, to, mode, **kw):
    from lele_amd.features import Resampler
    return Resampler(fr, to, mode, device=False, **kw)


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_resample_entry_points_are_declared_exported_wrapped_and_mirrored():
    from lele_amd import _lib, apps, features
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    lib = _lib.lib()
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "lele-hip", "src", "ffi.rs")).read()
    wrapped = open(os.path.join(ROOT, "lele_amd", "features.py")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n + "(" in hpp, n
        assert "pub fn %s(" % n in ffi, n
        assert "lib()." + n + "(" in wrapped, n
    assert "class Resampler {" in hpp and "class ResamplerStream {" in hpp
    for name in ("Resampler", "ResamplerStream"):
        assert isinstance(getattr(features, name), type)
    for name in ("resample_linear", "resample_fir_table", "resample_fir"):
        assert callable(getattr(apps, name))
    assert "resample.hip" in os.listdir(os.path.join(ROOT, "lele_amd", "csrc"))


def test_resample_linear_known_answers():
    from lele_amd import apps
    f32 = np.float32
    assert same_bits(apps.resample_linear(np.arange(10, dtype=f32), 2, 1), np.array([0, 2, 4, 6, 8], f32))
    # 1 -> 2: outputs 4 and 5 sit at idx = 2 = len - 1, the tail rule: the last sample as it is, not an interpolation towards nothing
    assert same_bits(apps.resample_linear(np.array([0, 2, 4], f32), 1, 2), np.array([0, 1, 2, 3, 4, 4], f32))
    assert same_bits(apps.resample_linear(np.arange(9, dtype=f32), 3, 2), np.array([0, 1.5, 3, 4.5, 6, 7.5], f32))
    for fr, to in ((1, 2), (2, 1), (3, 2), (44100, 16000)):
        assert apps.resample_linear(np.zeros(0, f32), fr, to).shape == (0,)
    assert same_bits(apps.resample_linear(np.array([7], f32), 1, 2), np.array([7, 7], f32))      # both by the tail rule
    assert same_bits(apps.resample_linear(np.array([7], f32), 2, 1), np.zeros(0, f32))           # output_len = (1 / 2.0) as usize = 0
    assert same_bits(apps.resample_linear(np.array([7], f32), 3, 2), np.zeros(0, f32))
    x = np.array([1.5, -2.25, np.inf], f32)
    assert same_bits(apps.resample_linear(x, 16000, 16000), x)                                    # from == to: a copy
    assert apps.resample_linear(x, 5, 5) is not x


def test_resample_linear_is_the_loop():
    """the array form is the reference's loop, output for output, on values that exercise the f64 -> f32 rounding"""
    from lele_amd import apps
    rng = np.random.default_rng(1)
    for fr, to in LEN_PAIRS + [(3, 2), (1, 2), (2, 1), (16000, 16000)]:
        for n in (0, 1, 2, 3, 7, 100, 1001):
            x = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 41, n)).astype(np.float32)
            assert same_bits(apps.resample_linear(x, fr, to), apps.resample_linear_loop(x, fr, to)), (fr, to, n)


def test_out_len_is_the_references_length_and_the_sinc_formula():
    """lele_hip_resampler_out_len (host arithmetic) for every length 0 .. 2000 and 479 999 .. 480 001 of six rate pairs.  The lengths
    were also searched for a case where the reference returns FEWER than output_len samples (audio.rs:132 pushing nothing): for these
    rate pairs there is none -- i < floor(len / ratio) keeps floor(i * ratio) below len with room to spare -- so the GPU tests have no
    such named case; the search stays here so that a pair that has one is noticed."""
    from lele_amd import apps
    shortfall = []
    for fr, to in LEN_PAIRS:
        lin, sinc = host_rs(fr, to, "linear"), host_rs(fr, to, "sinc")
        L, M, _ = apps.resample_fir_shape(fr, to)
        ratio = float(fr) / float(to)
        for n in LENGTHS:
            ref = len(apps.resample_linear(np.zeros(n, np.float32), fr, to))
            assert lin.out_len(n) == ref, (fr, to, n)
            if ref < int(float(n) / ratio):
                shortfall.append((fr, to, n))
            assert sinc.out_len(n) == -((-n * L) // M), (fr, to, n)
    assert shortfall == []
    same = host_rs(16000, 16000, "linear")
    assert [same.out_len(n) for n in (0, 1, 77)] == [0, 1, 77]
    assert host_rs(16000, 16000, "sinc").out_len(77, with_carry=True, final=False) == (77, 0)


@pytest.mark.parametrize("mode", ["linear", "sinc"])
def test_out_len_of_the_chunks_sums_to_the_whole(mode):
    """a length split at EVERY cut point (and at two): the per-chunk counts sum to the whole utterance's, the carry stays in its bound
    (linear: ceil(ratio) + 2 samples, sinc: fewer than T) and is what the next chunk's count was computed from"""
    from lele_amd import apps
    for fr, to in LEN_PAIRS:
        rs = host_rs(fr, to, mode)
        bound = math.ceil(fr / to) + 2 if mode == "linear" else apps.resample_fir_shape(fr, to)[2] - 1
        for n in (0, 1, 2, 5, 97, 1000, 2000):
            whole = rs.out_len(n)
            for c in range(n + 1):
                a, carry = rs.out_len(c, 0, final=False, with_carry=True)
                b, zero = rs.out_len(n - c, c, final=True, with_carry=True)
                assert a + b == whole and 0 <= carry <= min(bound, c) and zero == 0, (fr, to, n, c)
        rng = np.random.default_rng(fr + to)
        for n in (1000, 2000):
            whole = rs.out_len(n)
            for _ in range(200):
                c1, c2 = sorted(rng.integers(0, n + 1, 2))
                parts = [rs.out_len(c1, 0, False), rs.out_len(c2 - c1, c1, False), rs.out_len(n - c2, c2, True)]
                assert sum(parts) == whole and min(parts) >= 0


def test_uploaded_table_is_the_float64_table_rounded():
    from lele_amd import apps
    for fr, to, kw in [(48000, 16000, {}), (44100, 16000, {}), (8000, 16000, {}), (22050, 16000, {}), (11025, 16000, {}), (16000, 8000, {}),
                       (48000, 16000, dict(z=5, beta=6.0, rolloff=0.8)), (8000, 16000, dict(z=1, beta=0.0, rolloff=1.0))]:
        tab, L, M = host_rs(fr, to, "sinc", **kw).table()
        ref = apps.resample_fir_table(fr, to, **kw)
        assert (L, M, tab.shape[1]) == apps.resample_fir_shape(fr, to, kw.get("z", 16)) and ref.dtype == np.float64
        assert same_bits(tab, ref.astype(np.float32)), (fr, to, kw)
        assert np.allclose(ref.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert apps.resample_fir_shape(48000, 16000) == (1, 3, 96) and apps.resample_fir_shape(44100, 16000) == (160, 441, 90)
    assert apps.resample_fir_shape(8000, 16000) == (2, 1, 32)
    assert host_rs(8000, 16000, "linear").table()[0].size == 0


def tone_gain(fr, to, hz):
    """amplitude range of a unit complex tone through the float64 table, away from both ends"""
    from lele_amd import apps
    L, M, _ = apps.resample_fir_shape(fr, to)
    tab = apps.resample_fir_table(fr, to)
    t = np.arange(fr // 4) / float(fr)
    a = np.hypot(apps.resample_fir(np.cos(2 * np.pi * hz * t), tab, L, M), apps.resample_fir(np.sin(2 * np.pi * hz * t), tab, L, M))
    k = len(a) // 4
    return float(a[k:-k].min()), float(a[k:-k].max())


def test_filter_quality_on_the_float64_table():
    """Kaiser's formulas for beta = 8.6: stop-band attenuation A = 8.7 + beta / 0.1102 = 86.7 dB, ripple delta = 10^(-A/20) = 4.6e-5,
    transition width 2 pi (A - 8) / (2.285 (T - 1)) of the input rate, centred on the cut-off 0.9 x the narrower Nyquist (where a
    windowed sinc is at exactly one half).  With a 6 dB margin: a stop-band tone is down by at least A - 6 = 80.7 dB and the ripple is
    at most 2 delta.

    Stop band, decimating pairs whose input can hold the tone: 1.5 x the output Nyquist.  Measured 96.8 dB (48 -> 16 kHz), 101.5 dB
    (44.1 -> 16), 95.5 dB (16 -> 8).  (22.05 -> 16 kHz: 12 kHz is above the input's own Nyquist, no such tone exists.)

    Pass band: 0.75 x the narrower Nyquist.  T is fixed by Z, and by the width formula that tone lies just INSIDE the transition band
    for every pair here (48 -> 16 kHz: the band is 5815 .. 8585 Hz, the tone 6000 Hz).  There the response is 1/2 plus the integral
    of the window's main lobe, which is concave up to the pass-band edge, so it lies above the chord from (cut-off, 1/2) to (edge,
    1 - delta): the deviation is at most 2 delta + p / 2 with p the tone's depth into the half band (0 when it is in the pass band).
    That bound is 0.05 .. 0.08 here; measured deviations are 1.66e-3 (48 -> 16), 1.22e-3 (44.1 -> 16), 1.68e-3 (8 -> 16 and
    11.025 -> 16), 0.86e-3 (22.05 -> 16), 1.66e-3 (16 -> 8): the tone keeps its amplitude to 0.015 dB."""
    from lele_amd import apps
    att = 8.7 + 8.6 / 0.1102
    delta = 10.0 ** (-att / 20.0)
    for fr, to in LEN_PAIRS:
        _, _, T = apps.resample_fir_shape(fr, to)
        nyq = min(fr, to) / 2.0
        half = (att - 8.0) / (2.285 * (T - 1)) * fr / (2.0 * math.pi) / 2.0     # Hz, half the transition width
        cut, tone = 0.9 * nyq, 0.75 * nyq
        p = max(0.0, (tone - (cut - half)) / half)
        assert p < 0.25, (fr, to, p)
        lo, hi = tone_gain(fr, to, tone)
        print("pass %d -> %d: deviation -%.3g +%.3g (bound %.3g)" % (fr, to, 1 - lo, hi - 1, 2 * delta + p / 2))
        assert 1.0 - lo <= 2 * delta + p / 2 and hi - 1.0 <= 2 * delta, (fr, to, lo, hi)
        if fr > to and 1.5 * to / 2.0 < fr / 2.0:
            lo, hi = tone_gain(fr, to, 1.5 * to / 2.0)
            print("stop %d -> %d: %.1f dB" % (fr, to, 20 * math.log10(hi)))
            assert 20 * math.log10(hi) <= -(att - 6.0), (fr, to, hi)


# ---- the packed layout of the GPU tests, built once (host only)
SEG_LENGTHS = [0, 1, 2, 3, 5, 255, 256, 257, 4099, 70001]


def hard_values(rng, n):
    x = rng.standard_normal(n)
    k = rng.random(n) < 0.5
    return (x * np.where(k, 2.0 ** rng.integers(-40, 41, n), 1.0)).astype(np.float32)


_LAYOUT = {}


def layout():
    """(parent f32 [N], NaN outside the segments; [(start, end)]): the ten lengths permuted at odd starts (4-byte aligned only), one
    segment overlapping another, one repeated"""
    if not _LAYOUT:
        rng = np.random.default_rng(2024)
        order = [SEG_LENGTHS[i] for i in rng.permutation(len(SEG_LENGTHS))]
        segs, pos = [], 1
        for n in order:
            segs.append((pos, pos + n))
            pos += n + 6 + (n % 2)          # keeps every start odd, NaN between neighbours
        parent = np.full(pos + 8, np.nan, np.float32)
        for s, e in segs:
            parent[s:e] = hard_values(rng, e - s)
        big = next(s for s, e in segs if e - s == 4099)
        segs.insert(3, (big + 1000, big + 1000 + 2001))                          # overlaps the 4099-sample segment
        segs.insert(7, next((s, e) for s, e in segs if e - s == 257))            # a repeat
        assert all(s % 2 == 1 for s, _ in segs) and len(segs) == 12
        _LAYOUT["v"] = (parent, segs)
    return _LAYOUT["v"]


def fir_bound_terms(seg, tab32, L, M):
    """(float64 reference, gamma_T * sum|h x|) of apps.resample_fir on the f32-rounded table"""
    from lele_amd import apps
    T = tab32.shape[1]
    ref = apps.resample_fir(seg, tab32, L, M)
    mag = apps.resample_fir(np.abs(seg.astype(np.float64)), np.abs(tab32), L, M)
    gamma = T * U / (1.0 - T * U)
    return ref, gamma * mag


def within_fir_bound(got, ref, slack):
    got = np.asarray(got)
    if got.shape != ref.shape or got.dtype != np.float32 or not np.all(np.isfinite(got)):
        return False
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= slack + ulp))


def fir_emulated(parent, s, e, tab32, L, M, dphase=0, dbase=0, zero_extend=True):
    """the device kernel's arithmetic on the host (f32 fused multiply-adds emulated in f64: exact products, one rounding a step),
    optionally wrong in one of three ways"""
    T = tab32.shape[1]
    n = e - s
    n_out = (n * L + M - 1) // M
    i = np.arange(n_out, dtype=np.int64)
    base, phase = (i * M) // L + dbase, ((i * M) % L + dphase) % L
    acc = np.zeros(n_out, np.float32)
    for t in range(T):
        j = base - T // 2 + 1 + t
        inside = (j >= 0) & (j < n) if zero_extend else (s + j >= 0) & (s + j < len(parent))
        x = np.where(inside, parent[np.clip(s + j, 0, len(parent) - 1)], np.float32(0))
        acc = (tab32[phase, t].astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("fr,to", [(48000, 16000), (44100, 16000), (8000, 16000)])
def test_the_sinc_bound_rejects_wrong_kernels(fr, to):
    """|err| <= gamma_T * sum|h x| + 1 ulp accepts the kernel's arithmetic emulated on the host and rejects, on at least one segment each,
    a phase off by one, a base off by one and the neighbours' samples in place of the zero extension (on finite neighbours: the
    NaN of the GPU layout would make that one trivial)"""
    parent, segs = layout()
    parent = np.where(np.isnan(parent), np.float32(0.75), parent)
    tab, L, M = host_rs(fr, to, "sinc").table()
    wrong = {"base": dict(dbase=1), "neighbours": dict(zero_extend=False)}
    if L > 1:
        wrong["phase"] = dict(dphase=1)
    rejected = dict.fromkeys(wrong, 0)
    for s, e in segs:
        ref, slack = fir_bound_terms(parent[s:e], tab, L, M)
        assert within_fir_bound(fir_emulated(parent, s, e, tab, L, M), ref, slack), (s, e)
        for k, kw in wrong.items():
            rejected[k] += not within_fir_bound(fir_emulated(parent, s, e, tab, L, M, **kw), ref, slack)
    assert all(v >= 1 for v in rejected.values()), rejected


# ------------------------------------------------------------------------------------------------------------------- GPU

def resampler(ctx, fr, to, mode, **kw):
    from lele_amd.features import Resampler
    return Resampler(fr, to, mode, ctx=ctx, **kw)


def split_packed(tv, segs):
    flat = tv.numpy().reshape(-1)
    assert flat.dtype == np.float32 and (len(segs) == 0 or int(segs[-1][1]) == len(flat))
    return [flat[int(a):int(b)] for a, b in segs]


@pytest.mark.gpu
@pytest.mark.parametrize("fr,to,route", [(8000, 16000, "resample.linear"), (44100, 16000, "resample.linear"), (48000, 16000, "resample.linear"),
                                         (22050, 16000, "resample.linear"), (16000, 16000, "resample.copy")])
def test_linear_packed_is_the_reference_bit_for_bit(ctx, fr, to, route):
    from lele_amd import apps, kernels as K
    parent, segs = layout()
    rs = resampler(ctx, fr, to, "linear")
    got, osegs = rs.compute_segments(parent, segs)
    assert K.last_route(ctx) == route
    assert not np.any(np.isnan(got.numpy()))
    parts = split_packed(got, osegs)
    for (s, e), g in zip(segs, parts):
        assert same_bits(g, apps.resample_linear(parent[s:e], fr, to)), (s, e)
        assert len(g) == rs.out_len(e - s)
    # the same from device memory, and an empty layout
    buf = ctx.buf()
    got2, _ = rs.compute_segments(buf.upload(parent), segs)
    assert same_bits(got2.numpy(), got.numpy())
    none, osegs = rs.compute_segments(parent, [(5, 5), (9, 9)])
    assert none.shape == (0,) and osegs.tolist() == [[0, 0], [0, 0]] and K.last_route(ctx) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("fr,to,route", [(48000, 16000, "resample.fir1"), (44100, 16000, "resample.fir"), (8000, 16000, "resample.fir")])
def test_sinc_packed_within_the_derived_bound(ctx, fr, to, route):
    from lele_amd import kernels as K
    parent, segs = layout()
    rs = resampler(ctx, fr, to, "sinc")
    tab, L, M = rs.table()
    got, osegs = rs.compute_segments(parent, segs)
    assert K.last_route(ctx) == route
    assert not np.any(np.isnan(got.numpy()))
    for (s, e), g in zip(segs, split_packed(got, osegs)):
        ref, slack = fir_bound_terms(parent[s:e], tab, L, M)
        assert within_fir_bound(g, ref, slack), (s, e, float(np.max(np.abs(g - ref) - slack)) if len(g) == len(ref) else len(g))


LIVE_LENGTHS = [1, 1601, 8037]


def live_cuts(kind, max_chunk, rng):
    """per stream, the chunk lengths of every tick; the last chunk of a stream carries `final`"""
    cuts = []
    for n in LIVE_LENGTHS:
        if kind == "ones":
            c = [1] * n
        elif kind == "max":
            c = [max_chunk] * (n // max_chunk) + ([n % max_chunk] if n % max_chunk else [])
        elif kind == "whole":
            c = [n]
        else:
            c, left = [], n
            while left:
                k = 0 if rng.random() < 0.3 else int(min(left, rng.integers(1, max_chunk + 1)))
                c.append(k)
                left -= k
        cuts.append(c)
    return cuts


def run_live(ctx, st, utts, cuts, final_at_end=True):
    """push the utterances tick by tick -> per stream, the concatenated outputs"""
    n = len(utts)
    buf = ctx.buf()
    starts0 = np.cumsum([0] + [len(u) for u in utts[:-1]]).astype(np.int64)
    pcm = buf.upload(np.concatenate(utts).astype(np.float32))
    got = [[] for _ in utts]
    done = [0] * n
    for tick in range(max(len(c) for c in cuts)):
        lengths = np.array([c[tick] if tick < len(c) else 0 for c in cuts], np.int64)
        final = np.array([final_at_end and tick == len(c) - 1 for c in cuts])
        tv, os_, ol = st.push((pcm, starts0 + np.array(done, np.int64), lengths), final=final)
        flat = tv.numpy().reshape(-1)
        assert int(ol.sum()) == len(flat)
        for i in range(n):
            got[i].append(flat[os_[i]:os_[i] + ol[i]])
            done[i] += int(lengths[i])
    buf.close()
    return [np.concatenate(g) for g in got]


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["ones", "max", "random", "whole"])
@pytest.mark.parametrize("mode", ["linear", "sinc"])
@pytest.mark.parametrize("fr,to", [(8000, 16000), (44100, 16000)])
def test_live_equals_batch_bit_for_bit(ctx, fr, to, mode, cut):
    from lele_amd.features import ResamplerStream
    rng = np.random.default_rng(77)
    utts = [hard_values(rng, n) for n in LIVE_LENGTHS]
    rs = resampler(ctx, fr, to, mode)
    parent = np.concatenate(utts)
    ends = np.cumsum(LIVE_LENGTHS)
    batch, osegs = rs.compute_segments(parent, [(int(e - n), int(e)) for e, n in zip(ends, LIVE_LENGTHS)])
    want = split_packed(batch, osegs)
    max_chunk = {"ones": 1, "max": 160, "random": 160, "whole": max(LIVE_LENGTHS)}[cut]
    st = ResamplerStream(rs, len(utts), max_chunk)
    got = run_live(ctx, st, utts, live_cuts(cut, max_chunk, rng))
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), (i, len(g), len(w))
        assert st.counters(i) == (0, 0, 0)          # the final push reset the stream
    st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["linear", "sinc"])
@pytest.mark.parametrize("fr,to", [(8000, 16000), (44100, 16000)])
def test_live_final_without_audio_second_utterance_and_reset(ctx, fr, to, mode):
    """a final push that carries no audio flushes the tail; a second utterance after `final` and one after reset() equal the batch: a
    first utterance ending in NaN leaves nothing behind"""
    from lele_amd.features import ResamplerStream
    rng = np.random.default_rng(5)
    a, b = hard_values(rng, 1601), hard_values(rng, 777)
    a[-120:] = np.nan
    rs = resampler(ctx, fr, to, mode)
    batch, osegs = rs.compute_segments(np.concatenate([a, b]), [(0, len(a)), (len(a), len(a) + len(b))])
    want_a, want_b = split_packed(batch, osegs)
    assert not np.any(np.isnan(want_b)) and np.any(np.isnan(want_a))
    st = ResamplerStream(rs, 2, 400)                         # stream 1 stays silent throughout
    idle = np.zeros(0, np.float32)

    def feed(x, final_with_audio):
        out = []
        for k in range(0, len(x), 400):
            last = k + 400 >= len(x)
            tv, s, n = st.push([x[k:k + 400], idle], final=[last and final_with_audio, False])
            out.append(tv.numpy().reshape(-1)[s[0]:s[0] + n[0]])
            assert n[1] == 0
        return out

    got = feed(a, False)
    seen, emitted, carried = st.counters(0)
    tail = rs.out_len(0, samples_before=len(a), final=True)  # what only `final` releases (none when decimating linearly)
    assert seen == len(a) and emitted == sum(len(g) for g in got) == len(want_a) - tail and carried >= 0
    assert tail >= 1 or (mode, fr) == ("linear", 44100)
    tv, s, n = st.push([idle, idle], final=[True, False])    # final, no audio
    got.append(tv.numpy().reshape(-1)[s[0]:s[0] + n[0]])
    assert n[0] == tail and same_bits(np.concatenate(got), want_a)
    assert same_bits(np.concatenate(feed(b, True)), want_b)  # second utterance after final
    feed(a, False)                                           # NaN tail carried ...
    st.reset([0])                                            # ... and dropped
    assert st.counters(0) == (0, 0, 0)
    assert same_bits(np.concatenate(feed(b, True)), want_b)
    tv, s, n = st.push([idle, idle], final=[True, True])     # final on streams that never had audio
    assert tv.shape == (0,) and n.tolist() == [0, 0]
    st.close()


@pytest.mark.gpu
def test_validation_names_the_offender_and_leaves_out_alone(ctx):
    from lele_amd._lib import LeleError
    from lele_amd.features import Resampler, ResamplerStream
    for fr, to, word in ((0, 16000, "from_rate 0"), (-8000, 16000, "from_rate -8000"), (8000, 0, "to_rate 0"), (8000, -1, "to_rate -1")):
        with pytest.raises(LeleError, match=word):
            Resampler(fr, to, "linear", ctx=ctx)
    with pytest.raises(LeleError, match="z 0"):
        Resampler(48000, 16000, "sinc", ctx=ctx, z=0)
    with pytest.raises(LeleError, match="neither"):
        Resampler(48000, 16000, "cubic", ctx=ctx)
    for mode in ("linear", "sinc"):
        rs = resampler(ctx, 8000, 16000, mode)
        x = np.arange(1000, dtype=np.float32)
        out = ctx.buf()
        good, _ = rs.compute_segments(x, [(0, 1000)], out=out)
        before, nbytes = good.numpy().copy(), out.nbytes
        for segs, word in (([(0, 10), (990, 1001)], "segment 1"), ([(-1, 5)], "segment 0"), ([(7, 3)], "segment 0")):
            with pytest.raises(LeleError, match=word):
                rs.compute_segments(x, segs, out=out)
            assert out.nbytes == nbytes and same_bits(out.to_numpy(before.shape, np.float32), before)
        st = ResamplerStream(rs, 2, 100)
        with pytest.raises(LeleError, match="3 chunks for 2 streams"):
            st.push([x[:5], x[:5], x[:5]], out=out)
        with pytest.raises(LeleError, match="1 final flags for 2 streams"):
            st.push([x[:5], x[:5]], final=[True], out=out)
        with pytest.raises(LeleError, match="stream 1 has 101 samples"):
            st.push([x[:5], x[:101]], out=out)
        with pytest.raises(LeleError, match="stream 0"):
            st.push((x, [995, 0], [10, 5]), out=out)
        with pytest.raises(LeleError, match="id 2"):
            st.reset([2])
        assert st.counters(0) == (0, 0, 0) and st.counters(1) == (0, 0, 0)     # a refused push leaves the streams as they were
        assert out.nbytes == nbytes and same_bits(out.to_numpy(before.shape, np.float32), before)
        st.close()
        out.close()
    with pytest.raises(LeleError, match="without a context"):
        host_rs(8000, 16000, "linear").compute_segments(np.zeros(4, np.float32), [(0, 4)], out=ctx.buf())


def utterance_8k(n=12345):
    rng = np.random.default_rng(8)
    t = np.arange(n) / 8000.0
    return (0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1000 * t) + 0.05 * rng.uniform(-1, 1, n)).astype(np.float32)


@pytest.mark.gpu
def test_end_to_end_packed_8k_utterance_through_the_frontend(ctx):
    from lele_amd import apps
    from lele_amd.features import SenseVoiceFrontend
    x = utterance_8k()
    fe = SenseVoiceFrontend(ctx=ctx)
    rs = resampler(ctx, 8000, 16000, "linear")
    feats, off = fe.compute_segments(*rs.compute_segments(x, [(0, len(x))]))
    want = fe.compute(apps.resample_linear(x, 8000, 16000)).numpy()
    assert want.shape[0] > 20 and off.tolist() == [0, want.shape[0]]
    assert same_bits(feats.numpy(), want)


@pytest.mark.gpu
def test_end_to_end_live_8k_stream_through_the_frontend_stream(ctx):
    from lele_amd import apps
    from lele_amd.features import FrontendStream, ResamplerStream, SenseVoiceFrontend
    x = utterance_8k()
    fe = SenseVoiceFrontend(ctx=ctx)
    rs = resampler(ctx, 8000, 16000, "linear")
    tick = 800                                            # 100 ms at 8 kHz
    st, fs = ResamplerStream(rs, 1, tick), FrontendStream(fe, 1, 2 * tick + 8)
    rows = []
    for k in range(0, len(x), tick):
        final = [k + tick >= len(x)]
        f, off = fs.push(st.push([x[k:k + tick]], final=final), final=final)
        if off[-1]:
            rows.append(f.numpy().copy())
    want = fe.compute(apps.resample_linear(x, 8000, 16000)).numpy()
    assert same_bits(np.concatenate(rows), want)
    fs.close()
    st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fr,to,mode", [(44100, 16000, "linear"), (44100, 16000, "sinc"), (48000, 16000, "sinc")])
def test_graph_capture_of_one_packed_call(ctx, fr, to, mode):
    parent, segs = layout()
    rs = resampler(ctx, fr, to, mode)
    src, out = ctx.buf(), ctx.buf()
    pcm = src.upload(parent)
    eager = rs.compute_segments(pcm, segs, out=out)[0].numpy().copy()       # sizes the buffer, uploads the layout's table
    ctx.graph_begin()
    res, _ = rs.compute_segments(pcm, segs, out=out)
    g = ctx.graph_end()
    for _ in range(2):
        out.upload(np.zeros(len(eager), np.float32))
        g.launch()
        assert same_bits(out.to_numpy(res.shape, np.float32), eager)
    g.close()
    src.close()
    out.close()


TEARDOWN = """
import numpy as np
import lele_amd
from lele_amd.features import FrontendStream, Resampler, ResamplerStream, SenseVoiceFrontend
ctx = lele_amd.default_ctx(0)
fe = SenseVoiceFrontend(ctx=ctx)
fs = FrontendStream(fe, 1, 1700)
rs = Resampler(8000, 16000, "sinc", ctx=ctx)
st = ResamplerStream(rs, 1, 800)
tv, s, n = st.push([np.ones(800, np.float32)])
assert n[0] > 0 and tv.numpy().shape == (n[0],)
rows, off = fs.push((tv, s, n))
assert off[-1] > 0
print("left open", flush=True)
"""


@pytest.mark.gpu
def test_objects_left_open_at_interpreter_exit_are_closed_with_their_context():
    """a Resampler, a ResamplerStream and the front-end objects behind them that nobody closed (an uncaught exception keeps them alive
    in its traceback) are closed when their context is, not after it: the interpreter exits cleanly.  Needs its own interpreter,
    hence the child process."""
    r = subprocess.run([sys.executable, "-c", TEARDOWN], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "left open" in r.stdout, r.stdout
