"""The k-best decode head: every frame's k best tokens with their log-probabilities out of the i8 GEMM's epilogue
(lele_hip_fused_quantized_linear_topk, .._topk_segments; igemm_kernel EM 5) and the host half that consumes them
(lele_amd.apps.ctc_prefix_beam_search).

Reference: oracle.pyoracle.fused_quantized_linear gives the bit-exact logits x (per segment alone for the packed form).  Expected ids
are integers from those logits alone, topk_last below: value descending, of equal values the greater column first (the arg-max head's
rule continued, not the stable order of kernels.topk), padded with -1 where k > n; they are compared exactly, every row.  Expected
log-probabilities are x_j - logsumexp(x) in float64, and the acceptance is |got - ref| <= 1e-5 + 2^-22 |ref| on every slot of every
row: the first term is the bar tests/test_ctc_scores.py holds slot 0 to, the second is two f32 roundings ((v_j - v_0), then + logprob_0)
of a value of that magnitude.  Slot 0 is compared bit for bit with fused_quantized_linear_argmax_logprob.

The input families, shapes and packed layout are those of tests/test_ctc_greedy.py (imported, with its cache of oracle results), plus
one case of this file, `signed_zero`: all-zero rows against weight scales of both signs, so that every logit is +0.0 or -0.0 -- the
oracle's logits of the other families hold no -0.0 at all (a zero sum times a positive scale plus any bias is never -0.0), and the rule
"+0.0 and -0.0 are equal" needs a row that holds both.

Worst |logprob - float64| observed on the MI355X (the GPU tests print it per case): 1.53e-5 for `random`, `spread` and
`flat` (2^-16: two f32 ulps of a value between 64 and 128; the runner-up slots of these families lie 25 to 120 and more below the
winner, and the second term of the bar is 2 ulps of exactly such values), 1.29e-5 `ties`, 4.3e-6 `negative`,
2.8e-6 at the model's width, 2.9e-7 `signed_zero`."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import npref as N  # noqa: E402
from oracle import pyoracle as O  # noqa: E402
from tests.test_ctc_greedy import DENSE, PACKED_LENGTHS, WIDE, dense_case, packed_case, slices, weights  # noqa: E402,F401
from tests.test_ctc_greedy import FAMILIES, applies  # noqa: E402

KS = (1, 2, 4, 8)
BAR_ABS, BAR_REL = 1e-5, 2.0 ** -22
SIGNED_ZERO = ("signed_zero", 1, 3, 512, 130)


def topk_last(x, k):   # value descending; equal values: greater column first
    v = x.shape[-1]
    return (v - 1 - np.argsort(-x[..., ::-1], axis=-1, kind="stable")[..., :k]).astype(np.int32)


def expected(logits, k):
    """(ids int32 [.., k], float64 log-probabilities [.., k]) of the oracle's logits; -1 / -inf where k > n"""
    n = logits.shape[-1]
    kk = min(k, n)
    ids = topk_last(logits, kk)
    v = np.asarray(logits, np.float64)
    mx = v.max(axis=-1, keepdims=True)
    lse = mx + np.log(np.exp(v - mx).sum(axis=-1, keepdims=True))
    lp = np.take_along_axis(v, ids.astype(np.int64), axis=-1) - lse
    pad = [(0, 0)] * (logits.ndim - 1) + [(0, k - kk)]
    return np.pad(ids, pad, constant_values=-1), np.pad(lp, pad, constant_values=-np.inf)


_zero_case = []


def case(family, batch, m, k, n):
    """test_ctc_greedy.dense_case, and this file's own `signed_zero`"""
    if family != "signed_zero":
        return dense_case(family, batch, m, k, n)
    if not _zero_case:
        rng = np.random.default_rng(4)
        w, ws, wz, _ = weights("random", rng, k, n)
        ws = (ws * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)).astype(np.float32)
        bias = np.where(ws < 0, -0.0, 0.0).astype(np.float32)
        x = np.zeros((batch, m, k), np.float32)
        logits = O.fused_quantized_linear(x, w, ws, wz, bias)
        _zero_case.append((x, (w, ws, wz, bias), logits))
    return _zero_case[0]


def dense_table():
    return [(f,) + s for s in DENSE for f in FAMILIES if applies(f, s[0], s[3])] + [SIGNED_ZERO]


def all_cases():
    return dense_table() + [("random",) + WIDE, ("ties",) + WIDE]


def within_bar(got, want):
    """got f32, want float64: |got - want| <= 1e-5 + 2^-22 |want| where want is finite, got == -inf exactly where it is not"""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) - BAR_REL * np.abs(want[fin])
    return bool(np.array_equal(got[~fin], want[~fin]) and (err <= BAR_ABS).all()), float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))


# ---------------------------------------------------------------------------------------------------- CPU: the reference and the families
def test_slot_0_is_argmax_last():
    for c in dense_table():
        logits = case(*c)[2]
        for k in KS:
            assert np.array_equal(expected(logits, k)[0][..., 0], N.argmax_last(logits)), (c, k)
    for family in FAMILIES:
        for lg in packed_case(family, PACKED_LENGTHS, 512, 300)[3]:
            if len(lg):
                assert np.array_equal(topk_last(lg, 4)[..., 0], N.argmax_last(lg)), family


def test_ties_condition_three_equal_values_in_three_tiles():
    logits = dense_case("ties", 3, 50, 512, 300)[2].reshape(-1, 300)
    ids = topk_last(logits, 3)
    v = np.take_along_axis(logits, ids.astype(np.int64), axis=1)
    assert (v[:, 0] == v[:, 1]).all() and (v[:, 1] == v[:, 2]).all()
    assert (ids[:, 0] > ids[:, 1]).all() and (ids[:, 1] > ids[:, 2]).all()
    assert (ids[:, 0] - ids[:, 1] == 100).all() and (ids[:, 1] - ids[:, 2] == 100).all()
    # 100 apart: the first and the third copy never share a 128-column tile, and a good part of the rows has all three in different tiles
    tiles = ids // 128
    assert (tiles[:, 0] != tiles[:, 2]).all()
    assert np.mean((tiles[:, 0] != tiles[:, 1]) & (tiles[:, 1] != tiles[:, 2])) >= 0.25


def test_top_8_condition_two_candidates_share_a_32_column_group():
    for c in dense_table():
        n = c[4]
        if n < 127 or c[0] == "signed_zero":
            continue
        groups = np.sort(topk_last(case(*c)[2].reshape(-1, n), 8) // 32, axis=1)
        share = np.mean((np.diff(groups, axis=1) == 0).any(axis=1))
        assert share >= 0.5, (c, share)


def test_signed_zero_condition_every_row_holds_both_zeros():
    logits = case(*SIGNED_ZERO)[2].reshape(-1, SIGNED_ZERO[4])
    assert (logits == 0).all()
    neg = np.signbit(logits)
    assert neg.any(axis=1).all() and (~neg).any(axis=1).all()
    assert np.array_equal(topk_last(logits, 8), np.tile(np.arange(129, 121, -1, dtype=np.int32), (3, 1)))


# ---- wrong kernels on the oracle's logits [rows, n] -> (ids [rows, k], float64 log-probabilities or None = the reference's)
def _tiles(lg, fill):
    rows, n = lg.shape
    return np.concatenate([lg, np.broadcast_to(fill, (rows, -n % 128))], axis=1).reshape(rows, -1, 128)


def _ordered_key(lg, fold):
    b = np.ascontiguousarray(lg, np.float32).view(np.uint32).astype(np.uint64)
    if fold:
        b = np.where(b == 0x80000000, 0, b)
    b = np.where(b >> np.uint64(31), b ^ np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return (b << np.uint64(32)) | np.arange(lg.shape[1], dtype=np.uint64)


def _by_key(lg, k, fold=True):
    key = _ordered_key(lg, fold)
    return np.argsort(key, axis=1)[:, ::-1][:, :k].astype(np.int32)


def wrong_smaller_column(lg, k):
    return np.argsort(-lg, axis=1, kind="stable")[:, :k].astype(np.int32), None


def wrong_one_per_tile(lg, k):
    t = _tiles(lg, np.float32(-np.inf))
    best = (127 - np.argmax(t[:, :, ::-1], axis=2)) + 128 * np.arange(t.shape[1])       # [rows, tiles], last of equal maxima
    val = np.take_along_axis(lg, best, axis=1)
    order = topk_last(np.where(np.arange(lg.shape[1]) == best[:, :, None], val[:, :, None], -np.inf).max(axis=1), min(k, t.shape[1]))
    return np.pad(order, [(0, 0), (0, k - order.shape[1])], constant_values=-1), None


def wrong_masked_by_value(lg, k):
    v = lg.astype(np.float64).copy()
    out = np.full((lg.shape[0], k), -1, np.int32)
    for j in range(min(k, lg.shape[1])):
        win = N.argmax_last(v)
        top = np.take_along_axis(v, win[:, None].astype(np.int64), axis=1)
        out[:, j] = np.where(np.isfinite(top[:, 0]), win, -1)
        v[v == top] = -np.inf
    return out, None


def wrong_concatenated(lg, k):
    t = _tiles(lg, np.float32(-np.inf))
    per = topk_last(t, min(k, 128)) + 128 * np.arange(t.shape[1], dtype=np.int32)[None, :, None]
    flat = per.reshape(lg.shape[0], -1)
    flat = np.where(flat < lg.shape[1], flat, -1)
    out = np.full((lg.shape[0], k), -1, np.int32)
    for r in range(lg.shape[0]):
        keep = flat[r][flat[r] >= 0][:k]
        out[r, :len(keep)] = keep
    return out, None


def wrong_padded(lg, k):
    ext = _tiles(lg, lg[:, -1:]).reshape(lg.shape[0], -1)
    return topk_last(ext, k), None


def wrong_relative_to_tile_maximum(lg, k):
    ids, lp = expected(lg, k)
    v = lg.astype(np.float64)
    tile_max = _tiles(lg, np.float32(-np.inf)).astype(np.float64).max(axis=2)
    safe = np.maximum(ids, 0).astype(np.int64)
    vj = np.take_along_axis(v, safe, axis=1)
    out = (vj - np.take_along_axis(tile_max, safe // 128, axis=1)) + lp[:, :1]
    return ids, np.where(ids >= 0, out, -np.inf)


def wrong_negative_zero_below(lg, k):
    ids = _by_key(lg, min(k, lg.shape[1]), fold=False)
    return np.pad(ids, [(0, 0), (0, k - ids.shape[1])], constant_values=-1), None


WRONG = {"ties to the smaller column": wrong_smaller_column, "one candidate per tile": wrong_one_per_tile,
         "winners masked by value": wrong_masked_by_value, "tile lists concatenated": wrong_concatenated,
         "padded columns admitted": wrong_padded, "relative to the tile's maximum": wrong_relative_to_tile_maximum,
         "-0.0 below +0.0": wrong_negative_zero_below}


def test_the_key_order_is_topk_last():
    """the 64-bit key the kernel sorts by, emulated, orders every case exactly as topk_last does"""
    for c in dense_table():
        lg = case(*c)[2].reshape(-1, c[4])
        assert np.array_equal(_by_key(lg, min(8, c[4])), topk_last(lg, min(8, c[4]))), c


@pytest.mark.parametrize("name", list(WRONG))
def test_emulated_wrong_kernels_are_caught(name):
    caught = []
    for c in dense_table():
        lg = case(*c)[2].reshape(-1, c[4])
        for k in (4, 8):
            want_ids, want_lp = expected(lg, k)
            ids, lp = WRONG[name](lg, k)
            if not np.array_equal(ids, want_ids) or (lp is not None and not within_bar(lp, want_lp)[0]):
                caught.append((c, k))
    assert caught, name


# ---------------------------------------------------------------------------------------------------- CPU: the host half
def _collapse(path, blank):
    out = []
    for a, b in zip((None,) + path[:-1], path):
        if b != a and b != blank:
            out.append(b)
    return tuple(out)


def _exhaustive(lp, blank):
    """float64 log score of every label sequence: the sum over all V^T alignments"""
    t, v = lp.shape
    tot = {}
    for path in itertools.product(range(v), repeat=t):
        tot.setdefault(_collapse(path, blank), []).append(sum(lp[i, c] for i, c in enumerate(path)))
    return {p: float(np.logaddexp.reduce(s)) for p, s in tot.items()}


def test_ctc_prefix_beam_search_against_exhaustive_enumeration():
    from lele_amd.apps import ctc_prefix_beam_search
    rng = np.random.default_rng(3)
    for t in (1, 2, 3, 4):
        for blank in (0, 2):
            z = rng.standard_normal((t, 4)) * 2.0
            lp = z - np.logaddexp.reduce(z, axis=1, keepdims=True)
            ids = np.argsort(-lp, axis=1, kind="stable")
            cand = np.take_along_axis(lp, ids, axis=1)
            every = sorted(_exhaustive(lp, blank).items(), key=lambda kv: (-kv[1], kv[0]))
            got = ctc_prefix_beam_search(ids, cand, blank=blank, beam=1000, nbest=len(every))
            assert len(got) == len(every)
            assert got[0][0] == every[0][0] and abs(got[0][1] - every[0][1]) <= 1e-9
            assert [p for p, _ in got] == [p for p, _ in every]
            assert all(abs(a[1] - b[1]) <= 1e-9 for a, b in zip(got, every))
            assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))
            # k = 1, beam = 1: the collapsed greedy path, whose one alignment is its whole score
            one = ctc_prefix_beam_search(ids[:, :1], cand[:, :1], blank=blank, beam=1)
            assert one == [(_collapse(tuple(ids[:, 0].tolist()), blank), pytest.approx(float(cand[:, 0].sum()), abs=1e-12))]
            # a candidate of id -1 is ignored, whatever its score says
            ids_pad = np.concatenate([ids[:, :2], np.full((t, 1), -1), ids[:, 2:3]], axis=1)
            lp_pad = np.concatenate([cand[:, :2], np.zeros((t, 1)), cand[:, 2:3]], axis=1)
            assert ctc_prefix_beam_search(ids_pad, lp_pad, blank=blank, beam=1000, nbest=3) == \
                ctc_prefix_beam_search(ids[:, :3], cand[:, :3], blank=blank, beam=1000, nbest=3)
    assert ctc_prefix_beam_search(np.zeros((0, 4), np.int32), np.zeros((0, 4)), beam=2) == [((), 0.0)]


NAMES = ("lele_hip_fused_quantized_linear_topk", "lele_hip_fused_quantized_linear_topk_segments")


def test_the_entry_points_are_declared_and_wrapped():
    from lele_amd._lib import exported_symbols
    assert set(NAMES) <= set(exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "lele_hip.h")).read()
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "lele-hip", "src", "ffi.rs")).read()
    kpy = open(os.path.join(ROOT, "lele_amd", "kernels.py")).read()
    for n in NAMES:
        assert "int " + n + "(" in hdr, n
        assert n + "(" in hpp, n
        assert "pub fn %s(" % n in ffi, n
        assert "def %s(" % n[len("lele_hip_"):] in kpy and "lib()." + n + "(" in kpy, n
    doc = hdr[:hdr.index("int " + NAMES[0] + "(")].rsplit("/*", 1)[1]
    assert "GREATER COLUMN FIRST" in doc and "lele_hip_topk" in doc and "(8 k + 4)" in doc


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "ctc_topk_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "ctc_topk_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_ctc_topk_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- GPU
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_dense(K, ctx, x, wt, k, **kw):
    return K.fused_quantized_linear_topk(x, wt[0], wt[1], wt[2], wt[3], k, ctx=ctx, **kw)


def check_rows(ids, lp, logits, k, what):
    """every assertion a [.., k] result owes the oracle's logits; returns the worst |logprob - float64|"""
    want_ids, want_lp = expected(logits, k)
    assert ids.dtype == np.int32 and lp.dtype == np.float32 and ids.shape == lp.shape == want_ids.shape, what
    assert np.array_equal(ids, want_ids), what
    ok, worst = within_bar(lp, want_lp)
    print("%s k=%d: max |logprob - ref64| = %.3g" % (what, k, worst))
    assert ok, (what, worst)
    flat_ids, flat_lp = ids.reshape(-1, k), lp.reshape(-1, k)
    for j in range(1, k):       # along k: log-probabilities do not increase, real ids are distinct
        assert (flat_lp[:, j] <= flat_lp[:, j - 1]).all(), what
        for i in range(j):
            assert ((flat_ids[:, j] != flat_ids[:, i]) | (flat_ids[:, j] < 0)).all(), what
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("family,batch,m,k,n", all_cases())
def test_dense_ids_and_scores(ctx, family, batch, m, k, n):
    from lele_amd import kernels as K
    x, wt, logits = case(family, batch, m, k, n)
    si, sl = K.fused_quantized_linear_argmax_logprob(x, *wt, ctx=ctx)
    si, sl = si.numpy(), sl.numpy()
    for best in KS:
        got_ids, got_lp = run_dense(K, ctx, x, wt, best)
        assert tuple(got_ids.shape) == tuple(got_lp.shape) == (batch, m, best)
        ids, lp = got_ids.numpy(), got_lp.numpy()
        check_rows(ids, lp, logits, best, "%s %s" % (family, (batch, m, k, n)))
        assert np.array_equal(ids[..., 0], si) and np.array_equal(bits(lp[..., 0]), bits(sl))
        if best > n:
            assert (ids[..., n:] == -1).all() and np.isneginf(lp[..., n:]).all()


@pytest.mark.gpu
def test_dense_rank_2_and_empty(ctx):
    from lele_amd import kernels as K
    x, wt, logits = dense_case("random", 1, 5, 512, 127)
    i2, l2 = run_dense(K, ctx, x[0], wt, 4)
    assert tuple(i2.shape) == tuple(l2.shape) == (5, 4)
    check_rows(i2.numpy(), l2.numpy(), logits[0], 4, "rank 2")
    ei, el = run_dense(K, ctx, np.zeros((2, 0, 512), np.float32), wt, 4)
    assert tuple(ei.shape) == tuple(el.shape) == (2, 0, 4)
    assert ei.numpy().shape == (2, 0, 4) and ei.numpy().dtype == np.int32 and el.numpy().shape == (2, 0, 4) and el.numpy().dtype == np.float32
    pi, pl = K.fused_quantized_linear_topk_segments(np.zeros((0, 512), np.float32), [0, 0, 0], *wt, 4, ctx=ctx)
    assert tuple(pi.shape) == tuple(pl.shape) == (0, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_packed_segments_are_the_dense_call_on_each_alone(ctx, family):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
    got_ids, got_lp = K.fused_quantized_linear_topk_segments(x, off, *wt, 4, ctx=ctx)
    ids, lp = got_ids.numpy(), got_lp.numpy()
    assert tuple(got_ids.shape) == tuple(got_lp.shape) == (int(off[-1]), 4) == ids.shape == lp.shape
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            seg = slice(off[i], off[i + 1])
            check_rows(ids[seg], lp[seg], logits[i], 4, "%s segment %d" % (family, i))
            ai, al = run_dense(K, ctx, x[seg], wt, 4)
            assert np.array_equal(ids[seg], ai.numpy()), i
            assert np.array_equal(bits(lp[seg]), bits(al.numpy())), i


@pytest.mark.gpu
def test_failures_leave_the_outputs_alone(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, _ = dense_case("random", 3, 50, 512, 300)
    oi, ol = ctx.buf(), ctx.buf()
    marker = np.arange(1000, 1150, dtype=np.int32)
    oi.upload(marker)
    ol.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(oi._h)
    seg = K.fused_quantized_linear_topk_segments
    px, poff = x.reshape(150, 512), np.array([0, 50, 100, 150], np.int64)
    o = dict(out_ids=oi, out_logprob=ol, ctx=ctx)
    for call in (lambda: run_dense(K, ctx, x, wt, 0, out_ids=oi, out_logprob=ol),
                 lambda: run_dense(K, ctx, x, wt, 9, out_ids=oi, out_logprob=ol),
                 lambda: run_dense(K, ctx, x, wt, 4, out_ids=oi, out_logprob=oi),                  # one buffer twice
                 lambda: seg(px, poff, *wt, 0, **o),
                 lambda: seg(px, poff, *wt, 9, **o),
                 lambda: seg(px, poff, *wt, 4, out_ids=ol, out_logprob=ol, ctx=ctx),
                 lambda: seg(px, [0, 60, 50, 150], *wt, 4, **o),                                   # offsets that go back
                 lambda: seg(px, [0, 50, 149], *wt, 4, **o),                                       # offsets that do not end at R
                 lambda: run_dense(K, ctx, x[:, :, :500], wt, 4, out_ids=oi, out_logprob=ol)):     # K mismatch
        with pytest.raises(_lib.LeleError):
            call()
        for b in (oi, ol):
            assert _lib.lib().lele_hip_buf_bytes(b._h) == before
            assert np.array_equal(b.to_numpy((150,), np.int32), marker)


@pytest.mark.gpu
def test_graph_replay_reads_the_new_input(ctx):
    from lele_amd import kernels as K
    xa, wt, _ = dense_case("random", 3, 50, 512, 300)
    xb = dense_case("spread", 3, 50, 512, 300)[0]
    xc = dense_case("ties", 3, 50, 512, 300)[0]
    wt = tuple(K.Weight(a.copy()) for a in wt)
    off = np.array([0, 50, 100, 150], np.int64)
    inp, inp2 = ctx.buf(), ctx.buf()
    outs = [ctx.buf() for _ in range(4)]
    eager = {}
    for name, x in (("b", xb), ("c", xc), ("a", xa)):        # the eager results, in buffers of their own; `a` last: its shapes stay staged
        di, dl = run_dense(K, ctx, x, wt, 4)
        pi, pl = K.fused_quantized_linear_topk_segments(x.reshape(150, 512), off, *wt, 4, ctx=ctx)
        eager[name] = (di.numpy().copy(), bits(dl.numpy()).copy(), pi.numpy().copy(), bits(pl.numpy()).copy())
    assert not np.array_equal(eager["a"][0], eager["b"][0]) and not np.array_equal(eager["b"][0], eager["c"][0])
    da, pa = inp.upload(xa), inp2.upload(xa.reshape(150, 512))

    def run():
        run_dense(K, ctx, da, wt, 4, out_ids=outs[0], out_logprob=outs[1])
        K.fused_quantized_linear_topk_segments(pa, off, *wt, 4, out_ids=outs[2], out_logprob=outs[3], ctx=ctx)

    run()                                                     # one eager run of the same shape / layout
    ctx.sync()
    ctx.graph_begin()
    run()
    graph = ctx.graph_end()
    for name, x in (("b", xb), ("c", xc)):                    # two replays, each with fresh input values in the same buffers
        inp.upload(x)
        inp2.upload(x.reshape(150, 512))
        for o in outs:
            o.upload(np.full(600, -7, np.int32))
        graph.launch()
        want = eager[name]
        assert np.array_equal(outs[0].to_numpy((3, 50, 4), np.int32), want[0])
        assert np.array_equal(outs[1].to_numpy((3, 50, 4), np.uint32), want[1])
        assert np.array_equal(outs[2].to_numpy((150, 4), np.int32), want[2])
        assert np.array_equal(outs[3].to_numpy((150, 4), np.uint32), want[3])
    graph.close()


@pytest.mark.gpu
def test_no_logits_are_stored(ctx):
    """After the call the two outputs hold rows x k x 4 bytes each.  Read to confirm that no rows x n workspace exists: on the k-best
    path run_tiled and fql_segments_impl (quant.hip) reserve what the scored head reserves, with k key tables instead of one: rows x
    ceil(n / 128) x (8 k + 4) bytes of keys and tile sums."""
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, _ = dense_case("random", 3, 50, 512, 300)
    oi, ol, pi, pl = (ctx.buf() for _ in range(4))
    run_dense(K, ctx, x, wt, 8, out_ids=oi, out_logprob=ol)
    K.fused_quantized_linear_topk_segments(x.reshape(150, 512), [0, 50, 100, 150], *wt, 8, out_ids=pi, out_logprob=pl, ctx=ctx)
    for b in (oi, ol, pi, pl):
        assert _lib.lib().lele_hip_buf_bytes(b._h) == 150 * 8 * 4


@pytest.mark.gpu
def test_host_cpp_ctc_topk_demo_matches_python(ctx, tmp_path):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case("ties", PACKED_LENGTHS, 512, 300)
    d = str(tmp_path)
    for name, a in (("x.f32", x), ("off.i64", off), ("w.f32", wt[0]), ("ws.f32", wt[1]), ("wz.f32", wt[2]), ("b.f32", wt[3]),
                    ("dims.i64", np.array([512, 300, 4], np.int64))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    r = subprocess.run([_build_demo(), "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    rd = lambda n, t: np.fromfile(os.path.join(d, n), t)  # noqa: E731
    ids, lp = K.fused_quantized_linear_topk_segments(x, off, *wt, 4, ctx=ctx)
    want = np.concatenate([expected(lg, 4)[0] for lg in logits if len(lg)])
    assert np.array_equal(rd("ids.i32", np.int32), ids.numpy().reshape(-1)) and np.array_equal(rd("ids.i32", np.int32), want.reshape(-1))
    assert np.array_equal(rd("lp.f32", np.uint32), bits(lp.numpy()).reshape(-1))
    assert np.array_equal(rd("dense_ids.i32", np.int32), rd("ids.i32", np.int32)) and np.array_equal(rd("dense_lp.f32", np.uint32), rd("lp.f32", np.uint32))


@pytest.mark.gpu
def test_beam_search_on_the_devices_candidates(ctx):
    """End to end on one utterance of a `random` case: the device's [T, 4] candidates through ctc_prefix_beam_search.  The prefix is the
    one the oracle's candidates give; the scores agree within T x the per-frame bar (a score is a log of sums of products of T frame
    probabilities, each within the bar of its float64 value)."""
    from lele_amd import kernels as K
    from lele_amd.apps import ctc_prefix_beam_search
    x, wt, logits = dense_case("random", 3, 50, 512, 300)
    got_ids, got_lp = run_dense(K, ctx, x, wt, 4)
    ids, lp = got_ids.numpy()[1], got_lp.numpy()[1]
    want_ids, want_lp = expected(logits[1], 4)
    got = ctc_prefix_beam_search(ids, lp, blank=0, beam=4, nbest=2)
    ref = ctc_prefix_beam_search(want_ids, want_lp, blank=0, beam=4, nbest=2)
    greedy = float(lp[:, 0].astype(np.float64).sum())
    assert got[0][1] >= greedy - 1e-9
    assert [p for p, _ in got] == [p for p, _ in ref]
    t = len(ids)
    assert all(abs(a[1] - b[1]) <= t * (BAR_ABS + BAR_REL * float(np.max(np.abs(want_lp)))) for a, b in zip(got, ref))


@pytest.mark.gpu
def test_encoder_topk_agrees_with_the_scored_head(ctx):
    from sensevoice_graph import Encoder
    enc = Encoder(ctx, layers=2, seed=3)
    rng = np.random.default_rng(11)
    feats = ctx.buf().upload(rng.standard_normal((2, 9, 560)).astype(np.float32))
    si, sl = enc.greedy_scored(feats)
    si, sl = si.numpy().copy(), sl.numpy().copy()
    ids, lp = enc.topk(feats, 4)
    ids, lp = ids.numpy(), lp.numpy()
    assert ids.shape == lp.shape == (2, 13, 4) and np.array_equal(ids[..., 0], si) and np.array_equal(bits(lp[..., 0]), bits(sl))
    off = np.array([0, 7, 28], np.int64)
    pf = ctx.buf().upload(rng.standard_normal((28, 560)).astype(np.float32))
    pi, pl, off4 = enc.topk_segments(pf, off, 4)
    assert pi.numpy().shape == pl.numpy().shape == (36, 4) and list(np.asarray(off4)) == [0, 11, 36]
    assert (np.diff(pl.numpy().astype(np.float64), axis=1) <= 0).all() and (pi.numpy() >= 0).all()
