"""Forced alignment: the decode head that leaves the log-probabilities of caller-chosen columns (lele_hip_fused_quantized_linear_logprob_at,
.._logprob_at_segments; igemm_kernel EM 6) and the CTC lattice kernel that consumes them (lele_hip_ctc_align_segments).

The head.  Reference: oracle.pyoracle.fused_quantized_linear gives the bit-exact logits v (per segment alone for the packed form).  ids
and logprob must be the scored head's bit for bit; out_at must EQUAL f32(f32(v_c - v_id) + logprob_dev), formed in numpy from the
oracle's logits and the device's own logprob, and lie within AT_BAR(ref) = 1.1e-5 + 2^-23 |ref| of the float64 log-soft-max: the scored
head's bar of 1e-5 on logprob (tests/test_ctc_scores.py derives it) plus two f32 roundings, one of a difference of magnitude at most
|ref| + ln N <= |ref| + 10.2 (2^-24 * 10.2 = 6.1e-7, inside the 1e-6 added to the absolute term) and one of the result.  Families: the
`random`, `ties`, `negative`, `soft`, `soft_negative` of tests/test_ctc_scores.py, restated.

The aligner.  Reference: lele_amd.apps.ctc_forced_align, float64; spans, ok, per-token scores and the path score must be EQUAL.  The
total (the CTC likelihood) passes through exp / log1p on both sides and gets
    |f32 - host f64| <= 2^-24 |s| + C_TOTAL * T * 2^-53 * max(1, A),       C_TOTAL = 40
A the largest finite |alpha| the host met.  Count per frame and state, per side: two logaddexp of (one subtraction, exp and log1p
counted as two roundings each, one addition) = 12, and the emission's addition: 13; logaddexp does not amplify what its arguments carry
(its partial derivatives are positive and sum to 1), so the errors add: 26 a frame for the two sides, and 12 once for the join of the
two end states: 26 T + 12 <= 40 T for T >= 1.  Every rounding is relative to a value of magnitude <= max(1, A) (the log1p is <= ln 2).

The CPU part holds the host function to enumeration of every alignment, states the tie rules on dyadic emissions, and checks a
plain-Python emulation of the kernel's data layout -- 16 states a lane, the values of the lane below handed across the boundary, 2-bit
back-pointers packed a lane a frame -- against the host function, with six deliberately wrong variants that must each differ."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lele_amd.apps import align_results, ctc_forced_align, token_times  # noqa: E402
from oracle import npref as N  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

NINF = -np.inf
C_TOTAL = 40
FAMILIES = ("random", "ties", "negative", "soft", "soft_negative")
#        batch, m,   K,   n,   listed columns            why
DENSE = [(1, 1, 512, 1, (0,)),                         # cols = [0]: the only column, 0.0 exactly
         (1, 5, 512, 127, (0, 3, 64, 126)),            # one ragged tile
         (1, 129, 512, 129, (0, 127, 128)),            # both sides of a tile edge, ragged row tile
         (3, 50, 512, 300, (255, 256, 299)),           # the last tile's first and last column, three slices in one row tile
         (4, 33, 64, 130, (1, 2, 129)),                # small K
         (1, 40, 40, 260, (0, 100, 255, 256, 259))]    # K not a multiple of 16
PACKED_LENGTHS = [1, 33, 0, 64, 65, 171, 300]
PACKED_COLS = (0, 5, 127, 128, 255, 256, 299)


def AT_BAR(ref64):
    return 1.1e-5 + 2.0 ** -23 * np.abs(ref64)


def weights(family, rng, k, n):
    """(w [k, n] u8 codes as f32, weight_scale [n], weight_zero [1], bias [n]) -- the families of tests/test_ctc_scores.py"""
    nb = (n + 2) // 3 if family == "ties" else n
    w = np.clip(np.round(128 + 32 * rng.standard_normal((k, nb))), 0, 255).astype(np.float32)
    ws = (np.abs(rng.standard_normal(nb)) * 0.01 + 0.002).astype(np.float32)
    bias = (rng.standard_normal(nb) * 0.02).astype(np.float32)
    if family in ("soft", "soft_negative"):
        ws, bias = (ws / np.float32(64.0)).astype(np.float32), (bias / np.float32(64.0)).astype(np.float32)
    if family in ("negative", "soft_negative"):
        bias = (bias - 1.0e4).astype(np.float32)
    if family == "ties":
        idx = np.arange(n) % nb
        w, ws, bias = np.ascontiguousarray(w[:, idx]), ws[idx].copy(), bias[idx].copy()
    return w, ws, np.array([128.0], np.float32), bias


def slices(rng, lengths, k):
    return [(rng.standard_normal((m, k)) * (1.0 + 0.75 * i) + 0.4 * i).astype(np.float32) for i, m in enumerate(lengths)]


def dense_cases():
    return [(f,) + s for s in DENSE for f in FAMILIES if f != "ties" or s[3] >= 2]


_cache = {}


def dense_case(family, batch, m, k, n):
    """(x [batch, m, k], (w, ws, wz, bias), oracle logits [batch, m, n]) -- computed once, shared, never written to"""
    key = (family, batch, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(17 + 1000 * FAMILIES.index(family) + 13 * n + m + k)
        wt = weights(family, rng, k, n)
        x = np.stack(slices(rng, [m] * batch, k))
        logits = O.fused_quantized_linear(x, *wt)
        for a in (x, logits) + wt:
            a.setflags(write=False)
        _cache[key] = (x, wt, logits)
    return _cache[key]


def packed_case(family, lengths, k, n):
    """(x [R, k], offsets, (w, ws, wz, bias), oracle logits [R, n]: every segment alone)"""
    key = (family, tuple(lengths), k, n)
    if key not in _cache:
        rng = np.random.default_rng(199 + 1000 * FAMILIES.index(family) + n + len(lengths))
        wt = weights(family, rng, k, n)
        segs = slices(rng, lengths, k)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        logits = np.concatenate([O.fused_quantized_linear(s[None], *wt)[0] if len(s) else np.zeros((0, n), np.float32) for s in segs])
        _cache[key] = (np.concatenate(segs), off, wt, logits)
    return _cache[key]


def log_softmax64(logits):
    v = np.asarray(logits, np.float64)
    mx = v.max(axis=-1, keepdims=True)
    return (v - mx) - np.log(np.exp(v - mx).sum(axis=-1, keepdims=True))


def at_from(logits, ids, logprob, cols):
    """the head's formula in f32: f32(f32(v_c - v_id) + logprob)"""
    v = np.asarray(logits, np.float32)
    v_id = np.take_along_axis(v, np.asarray(ids, np.int64)[..., None], -1)
    return ((v[..., list(cols)] - v_id).astype(np.float32) + np.asarray(logprob, np.float32)[..., None]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the lattice on the host
def collapse(path, blank=0):
    out, prev = [], None
    for x in path:
        if x != prev and x != blank:
            out.append(x)
        prev = x
    return tuple(out)


def table(rng, t, u=6, family="random"):
    """a synthetic `at` table: the f32 log-soft-max of seeded logits over u columns (flat: every emission -0.5, dyadic)"""
    if family == "flat":
        return np.full((t, u), -0.5, np.float32)
    lg = rng.standard_normal((t, u)) * (6.0 if family == "peaky" else 1.0)
    return log_softmax64(lg).astype(np.float32) if t else np.zeros((0, u), np.float32)


def transcript(rng, n, u=6, family="random"):
    """n labels out of 1 .. u - 1 (repeats: runs of equal labels)"""
    if family == "repeats":
        out = []
        while len(out) < n:
            out += [int(rng.integers(1, u))] * int(rng.integers(1, 4))
        return tuple(out[:n])
    return tuple(int(v) for v in rng.integers(1, u, n))


def min_frames(tr):
    return len(tr) + sum(1 for j in range(1, len(tr)) if tr[j] == tr[j - 1])


def emulate(at, cols, tokens, blank=0, skip_rows=0, wrong=None, spl=16):
    """The kernel's algorithm in plain Python: lane l owns states [spl l, spl l + spl), updated in place from its last state down; the
    last two states of lane l - 1 are read BEFORE any lane writes (the cross-lane move; the kernel moves only the topmost, the one a
    correct recurrence reads: a lane's first state is a blank, which takes no skip); the back-pointers of a lane's states of a frame
    are one word of 2 bits a state; lane 0 walks them from the end.  -> (ok, spans, scores, path score).  `wrong` breaks one rule."""
    cols = [int(c) for c in cols]
    bslot, slots, n = cols.index(blank), [cols.index(t) for t in tokens], len(tokens)
    frames = np.asarray(at, np.float32)[skip_rows:]
    nt, ns = len(frames), 2 * n + 1
    lanes = (ns + spl - 1) // spl + 1
    if nt == 0:
        return (True, [], [], 0.0) if n == 0 else (False, [], [], NINF)
    a = [[NINF] * spl for _ in range(lanes)]
    words = []
    for t in range(nt):
        row = frames[t]
        word = [0] * lanes
        if t == 0:
            a[0][0] = float(row[bslot])
            if n:
                a[0][1] = float(row[slots[0]])
        else:
            top = [(a[l][spl - 1], a[l][spl - 2]) for l in range(lanes)]
            for l in range(lanes):
                below = (NINF, NINF) if l == 0 or wrong == "handover" else top[l - 1]
                for i in range(spl - 1, -1, -1):
                    s = spl * l + i
                    j = (s - 1) // 2
                    odd = bool(s & 1)
                    skip = odd and 1 <= j < n and (tokens[j] != tokens[j - 1] or wrong == "skip_equal")
                    if wrong == "skip_blank" and not odd and s >= 2:
                        skip = True
                    em = float(row[slots[j]]) if odd and j < n else float(row[bslot])
                    step = a[l][i - 1] if i >= 1 else below[0]
                    far = a[l][i - 2] if i >= 2 else below[0] if i == 1 else below[1]
                    best, frm = a[l][i], 0
                    if step >= best if wrong == "ties" else step > best:
                        best, frm = step, 1
                    if skip and (far >= best if wrong == "ties" else far > best):
                        best, frm = far, 2
                    a[l][i] = best + em if s < ns else NINF
                    word[l] |= frm << (2 * i)
        words.append(word)
    flat = [v for lane in a for v in lane]
    s = 2 * n if n == 0 or wrong == "end" or flat[2 * n] >= flat[2 * n - 1] else 2 * n - 1
    if flat[s] == NINF:
        return False, [], [], NINF
    score = flat[s]
    first, last, prev = [0] * n, [-1] * n, -1
    for t in range(nt - 1, -1, -1):
        if s < 0:
            break
        if s & 1:
            if s != prev:
                last[s >> 1] = t
            first[s >> 1] = t
        prev = s
        s -= (words[t][s // spl] >> (2 * (s % spl))) & 3
    scores = []
    for j in range(n):
        acc = 0.0
        for t in range(first[j], last[j] + 1):
            acc += float(frames[t][slots[j]])
        scores.append(acc)
    k = 0 if wrong == "spans" else skip_rows
    return True, [(first[j] + k, last[j] + k) for j in range(n)], scores, score


def emulation_cases():
    """(at, cols, tokens, skip_rows): the grid of the GPU test at sizes plain Python can walk, every family"""
    rng = np.random.default_rng(2024)
    cols = [0, 2, 3, 5, 7, 11]
    out = []
    for family in ("random", "repeats", "flat", "peaky"):
        for t in (0, 1, 2, 5, 37):
            for n in (0, 1, 2, 3, 7, 8, 9, 31, 33):
                tr = tuple(cols[v] for v in transcript(rng, n, 6, family))
                out.append((table(rng, t, 6, family), cols, tr, 0))
    for n in (1, 2, 3, 8, 9, 20):                       # exact_fit (the path is unique) and infeasible (one frame short)
        tr = tuple(cols[v] for v in transcript(rng, n, 6, "repeats"))
        for t in (min_frames(tr), min_frames(tr) - 1):
            out.append((table(rng, t, 6), cols, tr, 0))
    for rows, n in ((3, 0), (4, 1), (5, 1), (9, 2), (30, 9)):     # prompt rows in front, segments no longer than them included
        tr = tuple(cols[v] for v in transcript(rng, n, 6))
        out.append((table(rng, rows, 6), cols, tr, 4))
    return out


def test_the_c_abi_declares_the_three_calls():
    from lele_amd import _lib
    from lele_amd import kernels as K
    fns = ("lele_hip_fused_quantized_linear_logprob_at", "lele_hip_fused_quantized_linear_logprob_at_segments", "lele_hip_ctc_align_segments")
    assert set(fns) <= set(_lib.exported_symbols())
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    for fn in fns:
        assert getattr(_lib.lib(), fn) is not None, fn            # exported by the built library
        assert fn + "(" in hpp, fn
        assert hasattr(K, fn[len("lele_hip_"):]), fn


def test_host_function_against_enumeration_of_every_alignment():
    rng = np.random.default_rng(5)
    worst = 0.0
    for t in range(0, 7):
        lp = table(rng, t, 4)
        for tr in [(), (1,), (1, 1), (1, 2), (2, 2, 1), (1, 2, 1), (3, 3, 3)]:
            ok, spans, scores, path_score, total = ctc_forced_align(lp, [0, 1, 2, 3], tr)
            best, tot, feasible = NINF, NINF, False
            for p in itertools.product(range(4), repeat=t):
                if collapse(p) == tr:
                    feasible = True
                    v = math.fsum(float(lp[i, p[i]]) for i in range(t))
                    best, tot = max(best, v), np.logaddexp(tot, v)
            assert ok == feasible == (t >= min_frames(tr)), (t, tr)
            if not ok:
                assert (spans, scores, path_score, total) == ([], [], NINF, NINF)
                continue
            worst = max(worst, abs(best - path_score), abs(tot - total))
            # the path it returns collapses to the transcript and sums to its score
            path = [0] * t
            for j, (f, l) in enumerate(spans):
                assert 0 <= f <= l < t
                path[f:l + 1] = [tr[j]] * (l - f + 1)
            assert collapse(path) == tr and len(spans) == len(tr)
            acc = None
            for i in range(t):
                acc = float(lp[i, path[i]]) if acc is None else acc + float(lp[i, path[i]])
            assert (acc if t else 0.0) == path_score
            for j, (f, l) in enumerate(spans):
                acc = 0.0
                for i in range(f, l + 1):
                    acc += float(lp[i, tr[j]])
                assert acc == scores[j]
    print("worst |host - enumeration| = %.3g" % worst)
    assert worst <= 1e-12


def test_tie_rules_known_answers():
    flat = lambda t, u, v: np.full((t, u), v, np.float32)  # noqa: E731
    ok, spans, scores, path, _ = ctc_forced_align(flat(3, 2, -1.0), [0, 1], (1,))
    assert ok and spans == [(0, 0)] and path == -3.0 and scores == [-1.0]
    ok, spans, _, path, _ = ctc_forced_align(flat(5, 3, -0.5), [0, 1, 2], (2, 2))
    assert ok and spans == [(0, 0), (2, 2)] and path == -2.5
    ok, spans, _, path, _ = ctc_forced_align(flat(5, 4, -0.5), [0, 1, 2, 3], (1, 2, 3))
    assert ok and spans == [(0, 0), (1, 1), (2, 2)] and path == -2.5
    # prompt rows are counted in the spans, and sliced off the frames
    ok, spans, _, path, _ = ctc_forced_align(flat(7, 2, -1.0), [0, 1], (1,), skip_rows=4)
    assert ok and spans == [(4, 4)] and path == -3.0
    for bad in (dict(tokens=(4,)), dict(tokens=(0,)), dict(tokens=(1,), blank=9), dict(tokens=(1,) * 512)):
        with pytest.raises(ValueError):
            ctc_forced_align(flat(3, 2, -1.0), [0, 1], **bad)


def test_the_emulated_kernel_equals_the_host_function():
    for at, cols, tr, skip in emulation_cases():
        want = ctc_forced_align(at, cols, tr, 0, skip)[:4]
        assert emulate(at, cols, tr, 0, skip) == want, (at.shape, tr, skip)
        assert emulate(at, cols, tr, 0, skip, spl=4) == want, (at.shape, tr, skip)


@pytest.mark.parametrize("wrong", ["skip_equal", "skip_blank", "ties", "end", "handover", "spans"])
def test_emulated_wrong_kernels_differ(wrong):
    differ = sum(emulate(at, cols, tr, 0, skip, wrong) != ctc_forced_align(at, cols, tr, 0, skip)[:4] for at, cols, tr, skip in emulation_cases())
    print("%s: differs on %d cases" % (wrong, differ))
    assert differ >= 1


def test_the_heads_formula_in_f32_is_inside_the_bar():
    """(v_c - mx) + lp0 in f32, lp0 the float64 log-probability of the winner moved by nine tenths of the scored head's bar and rounded to
    f32 (that rounding, up to 2^-24 ln N = 6e-7, is part of the bar on the device's logprob)"""
    worst = 0.0
    for family, batch, m, k, n, cols in dense_cases():
        logits = dense_case(family, batch, m, k, n)[2]
        ref = log_softmax64(logits)
        ids = np.argmax(logits, -1)
        lp0 = np.take_along_axis(ref, ids[..., None], -1)[..., 0]
        for shift in (-9e-6, 0.0, 9e-6):
            got = at_from(logits, ids, (lp0 + shift).astype(np.float32), range(n)).astype(np.float64)
            assert (np.abs(got - ref) <= AT_BAR(ref)).all(), (family, n, shift)
            worst = max(worst, float(np.max(np.abs(got - ref) - 2.0 ** -23 * np.abs(ref))))
    print("worst excess over 2^-23 |ref| = %.3g" % worst)


# ---------------------------------------------------------------------------------------------------- GPU: the head
def run_at(K, ctx, x, wt, cols, **kw):
    return K.fused_quantized_linear_logprob_at(x, wt[0], wt[1], wt[2], wt[3], cols, ctx=ctx, **kw)


def check_head(K, ctx, tag, logits, cols, got, scored, topk):
    """got = (ids, logprob, at) of the head, scored = (ids, logprob) of the scored head, topk = (ids, logprob) of the k = 8 head"""
    ids, lp, at = (g.numpy() for g in got)
    n = logits.shape[-1]
    assert ids.dtype == np.int32 and lp.dtype == at.dtype == np.float32
    assert ids.shape == lp.shape == logits.shape[:-1] and at.shape == logits.shape[:-1] + (len(cols),) == tuple(got[2].shape)
    assert np.array_equal(ids, scored[0].numpy()) and np.array_equal(bits(lp), bits(scored[1].numpy())), tag
    assert np.array_equal(at, at_from(logits, ids, lp, cols)), tag
    ref = log_softmax64(logits)[..., list(cols)]
    err = np.abs(at.astype(np.float64) - ref)
    print("%s: max |at - ref64| = %.3g (bar %.3g)" % (tag, float(err.max()) if err.size else 0.0, 1.1e-5))
    assert (err <= AT_BAR(ref)).all(), tag
    # a listed column among the row's 8 best: the k-best head's log-probability bit for bit; the arg-max column: logprob itself
    ti, tl = topk[0].numpy().reshape(-1, 8), topk[1].numpy().reshape(-1, 8)
    flat_at = at.reshape(-1, len(cols))
    hits = 0
    for u, c in enumerate(cols):
        r, j = np.nonzero(ti == c)
        hits += len(r)
        assert np.array_equal(bits(flat_at[r, u]), bits(tl[r, j])), (tag, c)
        win = ids.reshape(-1) == c
        assert np.array_equal(bits(flat_at[win, u]), bits(lp.reshape(-1)[win])), (tag, c)
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize("family,batch,m,k,n,cols", dense_cases())
def test_dense_logprob_at(ctx, family, batch, m, k, n, cols):
    from lele_amd import kernels as K
    x, wt, logits = dense_case(family, batch, m, k, n)
    tag = "%s %s" % (family, (batch, m, k, n))
    scored = K.fused_quantized_linear_argmax_logprob(x, *wt, ctx=ctx)
    topk = K.fused_quantized_linear_topk(x, *wt, 8, ctx=ctx)
    lists = [cols] + ([tuple(range(300))] if n == 300 and family == "random" else [])     # ... and once all 300 columns
    for cl in lists:
        hits = check_head(K, ctx, tag, logits, cl, run_at(K, ctx, x, wt, cl), scored, topk)
        if n <= 8 or len(cl) == n:
            assert hits >= batch * m * min(n, 8)
    if n == 1:
        assert (bits(run_at(K, ctx, x, wt, cols)[2].numpy()) == 0).all()      # exactly +0.0


@pytest.mark.gpu
def test_dense_rank_2_and_empty(ctx):
    from lele_amd import kernels as K
    x, wt, logits = dense_case("soft", 1, 5, 512, 127)
    i2, l2, a2 = run_at(K, ctx, x[0], wt, [0, 126])
    assert tuple(i2.shape) == tuple(l2.shape) == (5,) and tuple(a2.shape) == (5, 2)
    assert np.array_equal(a2.numpy(), at_from(logits[0], i2.numpy(), l2.numpy(), [0, 126]))
    ei, el, ea = run_at(K, ctx, np.zeros((2, 0, 512), np.float32), wt, [0, 126])
    assert tuple(ei.shape) == tuple(el.shape) == (2, 0) and tuple(ea.shape) == (2, 0, 2)
    assert ea.numpy().shape == (2, 0, 2) and ea.numpy().dtype == np.float32
    pi, pl, pa = K.fused_quantized_linear_logprob_at_segments(np.zeros((0, 512), np.float32), [0, 0, 0], *wt, [3], ctx=ctx)
    assert tuple(pi.shape) == (0,) and tuple(pa.shape) == (0, 1) and pa.numpy().shape == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_packed_segments_are_the_dense_call_on_each_alone(ctx, family):
    from lele_amd import kernels as K
    x, off, wt, logits = packed_case(family, PACKED_LENGTHS, 512, 300)
    got = K.fused_quantized_linear_logprob_at_segments(x, off, *wt, PACKED_COLS, ctx=ctx)
    ids, lp, at = (g.numpy().copy() for g in got)
    scored = K.fused_quantized_linear_argmax_logprob_segments(x, off, *wt, ctx=ctx)
    topk = K.fused_quantized_linear_topk_segments(x, off, *wt, 8, ctx=ctx)
    check_head(K, ctx, "packed " + family, logits, PACKED_COLS, got, scored, topk)
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            di, dl, da = run_at(K, ctx, x[off[i]:off[i + 1]], wt, PACKED_COLS)
            assert np.array_equal(ids[off[i]:off[i + 1]], di.numpy()), i
            assert np.array_equal(bits(lp[off[i]:off[i + 1]]), bits(dl.numpy())), i
            assert np.array_equal(bits(at[off[i]:off[i + 1]]), bits(da.numpy())), i


@pytest.mark.gpu
def test_the_models_width(ctx):
    from lele_amd import kernels as K
    batch, m, k, n = 2, 171, 512, 25055
    x, wt, logits = dense_case("soft", batch, m, k, n)
    scored = K.fused_quantized_linear_argmax_logprob(x, *wt, ctx=ctx)
    topk = K.fused_quantized_linear_topk(x, *wt, 8, ctx=ctx)
    rng = np.random.default_rng(3)
    winners = scored[0].numpy().reshape(-1)[::35][:10]
    cols = sorted({0, n - 1} | {int(c) for c in rng.choice(n, 200, replace=False)} | {int(c) for c in winners})
    hits = check_head(K, ctx, "model width", logits, cols, run_at(K, ctx, x, wt, cols), scored, topk)
    assert hits >= 10
    off = np.array([0, 171, 342], np.int64)
    pi, pl, pa = K.fused_quantized_linear_logprob_at_segments(x.reshape(342, 512), off, *wt, cols, ctx=ctx)
    di, dl, da = run_at(K, ctx, x, wt, cols)
    assert np.array_equal(pi.numpy(), di.numpy().reshape(-1)) and np.array_equal(bits(pl.numpy()), bits(dl.numpy()).reshape(-1))
    assert np.array_equal(bits(pa.numpy()), bits(da.numpy()).reshape(342, -1))


@pytest.mark.gpu
def test_head_failures_leave_the_outputs_alone_and_no_logits_are_stored(ctx):
    """After a call the three buffers hold rows x 4, rows x 4 and rows x ncols x 4 bytes.  Read to confirm that no rows x n workspace
    exists: Head::At takes the scored head's reserve / arena_alloc calls in run_tiled and fql_segments_impl (keys rows x ceil(n / 128) x
    8 bytes, sums x 4) plus at->reserve(rows * ncols * 4); its column -> slot map (4 n bytes) is part of the call's layout table."""
    from lele_amd import _lib
    from lele_amd import kernels as K
    x, wt, _ = dense_case("soft", 3, 50, 512, 300)
    xp, poff = x.reshape(150, 512), np.array([0, 50, 100, 150], np.int64)
    bufs = [ctx.buf() for _ in range(6)]
    run_at(K, ctx, x, wt, [255, 256, 299], out_ids=bufs[0], out_logprob=bufs[1], out_at=bufs[2])
    K.fused_quantized_linear_logprob_at_segments(xp, poff, *wt, [255, 256, 299], out_ids=bufs[3], out_logprob=bufs[4], out_at=bufs[5], ctx=ctx)
    assert [_lib.lib().lele_hip_buf_bytes(b._h) for b in bufs] == [150 * 4, 150 * 4, 150 * 3 * 4] * 2
    oi, ol, oa = ctx.buf(), ctx.buf(), ctx.buf()
    marker = np.arange(1000, 1150, dtype=np.int32)
    for b in (oi, ol, oa):
        b.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(oi._h)
    o = dict(out_ids=oi, out_logprob=ol, out_at=oa)
    seg = K.fused_quantized_linear_logprob_at_segments
    calls = []
    for cols in ([5, 3], [3, 3], [0, 300], [-1, 4], [], list(range(300)) + [300]):           # unsorted, repeated, out of range, none, too many
        calls.append((lambda cols=cols: run_at(K, ctx, x, wt, cols, **o), cols))
        calls.append((lambda cols=cols: seg(xp, poff, *wt, cols, ctx=ctx, **o), cols))
    for alias in (dict(out_ids=oi, out_logprob=ol, out_at=oi), dict(out_ids=oi, out_logprob=ol, out_at=ol), dict(out_ids=oi, out_logprob=oi, out_at=oa)):
        calls.append((lambda alias=alias: run_at(K, ctx, x, wt, [1, 2], **alias), alias))
        calls.append((lambda alias=alias: seg(xp, poff, *wt, [1, 2], ctx=ctx, **alias), alias))
    calls.append((lambda: seg(xp, [0, 60, 50, 150], *wt, [1, 2], ctx=ctx, **o), "offsets"))
    for call, what in calls:
        with pytest.raises(_lib.LeleError):
            call()
        for b in (oi, ol, oa):
            assert _lib.lib().lele_hip_buf_bytes(b._h) == before, what
            assert np.array_equal(b.to_numpy((150,), np.int32), marker), what
    with pytest.raises(_lib.LeleError, match=r"cols\[1\]"):                                      # the error names the index
        run_at(K, ctx, x, wt, [5, 3], **o)
    with pytest.raises(_lib.LeleError, match=r"cols\[2\]"):
        run_at(K, ctx, x, wt, [0, 1, 300], **o)


# ---------------------------------------------------------------------------------------------------- GPU: the aligner
def aligner_batch(rng, family, pairs, u=6, skip_rows=0):
    """a packed batch of (frames, labels) segments of one family -> (at [R, u], offsets, transcripts)"""
    tabs, trs = [], []
    for t, n in pairs:
        trs.append(transcript(rng, n, u, family))
        tabs.append(table(rng, t + skip_rows if t >= 0 else 0, u, family))
    off = np.concatenate([[0], np.cumsum([len(a) for a in tabs])]).astype(np.int64)
    return (np.concatenate(tabs) if off[-1] else np.zeros((0, u), np.float32)), off, trs


def check_aligner(K, ctx, tag, at, off, trs, skip_rows=0, width=0, cols=None):
    cols = list(range(at.shape[1])) if cols is None else cols
    want = [ctc_forced_align(at[off[i]:off[i + 1]], cols, trs[i], 0, skip_rows, return_bound=True) for i in range(len(trs))]
    w = width or max([len(t) for t in trs] + [1])
    worst, worst_diff = 0.0, 0.0
    for with_total in (True, False):
        outs = K.ctc_align_segments(at, cols, off, trs, 0, skip_rows, width, total=with_total, ctx=ctx)
        spans, scores, path, total, ok = (None if o is None else o.numpy() for o in outs)
        assert spans.shape == (len(trs), w, 2) and scores.shape == (len(trs), w) and path.shape == ok.shape == (len(trs),)
        assert spans.dtype == ok.dtype == np.int32 and scores.dtype == path.dtype == np.float32 and (total is None) == (not with_total)
        got = align_results(spans, scores, path, total, ok, [len(t) for t in trs])
        for i, (g, h) in enumerate(zip(got, want)):
            n = len(trs[i]) if h[0] else 0
            assert g[0] == h[0] and g[1] == h[1], (tag, i, trs[i], g[:2], h[:2])
            assert g[2] == [float(np.float32(v)) for v in h[2]], (tag, i)
            assert g[3] == float(np.float32(h[3])), (tag, i, g[3], h[3])
            assert (spans[i, n:] == -1).all() and (bits(scores[i, n:]) == 0).all(), (tag, i)          # unused slots: -1 and +0.0
            if with_total:
                frames = max(int(off[i + 1] - off[i]) - skip_rows, 0)
                if np.isinf(h[4]):
                    assert g[4] == h[4], (tag, i)
                else:
                    diff = abs(g[4] - h[4])
                    bound = 2.0 ** -24 * abs(h[4]) + C_TOTAL * frames * 2.0 ** -53 * max(1.0, h[5])
                    worst, worst_diff = max(worst, diff - 2.0 ** -24 * abs(h[4])), max(worst_diff, diff)
                    assert diff <= bound, (tag, i, g[4], h[4], bound)
    print("%s: %d segments, worst |total - host| = %.3g, beyond its own f32 rounding %.3g" % (tag, len(trs), worst_diff, max(worst, 0.0)))
    return want


GRID = [(t, n) for t in (0, 1, 2, 5, 37, 171) for n in (0, 1, 2, 3, 31, 32, 33, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["random", "repeats", "flat", "peaky"])
def test_aligner_grid(ctx, family):
    from lele_amd import kernels as K
    rng = np.random.default_rng(31 + len(family))
    at, off, trs = aligner_batch(rng, family, GRID)
    want = check_aligner(K, ctx, family, at, off, trs)
    assert sum(1 for h in want if h[0]) >= 12 and sum(1 for h in want if not h[0]) >= 10
    # 16 states a lane: the same segments beside one transcript of more than 127 labels
    at2, off2, trs2 = aligner_batch(rng, family, GRID[8:] + [(300, 130)])
    check_aligner(K, ctx, family + " (16 states a lane)", at2, off2, trs2)


@pytest.mark.gpu
def test_aligner_exact_fit_and_infeasible(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(77)
    trs = [transcript(rng, n, 6, fam) for fam in ("random", "repeats") for n in (1, 2, 3, 31, 32, 33, 100)]
    for name, short in (("exact_fit", 0), ("infeasible", 1)):
        tabs = [table(rng, min_frames(tr) - short, 6) for tr in trs]
        off = np.concatenate([[0], np.cumsum([len(a) for a in tabs])]).astype(np.int64)
        want = check_aligner(K, ctx, name, np.concatenate(tabs), off, trs)
        assert all(h[0] == (not short) for h in want)


@pytest.mark.gpu
def test_aligner_packed_batch_with_prompt_rows(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(78)
    lengths = (0, 3, 4, 5, 40, 9, 17, 1)                      # rows, prompt rows included: four segments no longer than skip_rows
    labels = (0, 1, 0, 1, 12, 2, 20, 0)
    tabs = [table(rng, t, 6) for t in lengths]
    trs = [transcript(rng, n, 6) for n in labels]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    want = check_aligner(K, ctx, "packed, skip_rows 4", np.concatenate(tabs), off, trs, skip_rows=4, width=24)
    assert [h[0] for h in want] == [True, False, True, True, True, True, False, True]
    assert want[3][1] == [(4, 4)] and min(f for f, _ in want[4][1]) >= 4
    # other columns than 0 .. U - 1, the blank not the first of them
    cols = [2, 3, 5, 7, 11, 13]
    trs2 = [tuple(cols[v] for v in tr) for tr in trs]
    w = [ctc_forced_align(np.concatenate(tabs)[off[i]:off[i + 1]], cols, trs2[i], 2, 4) for i in range(len(trs))]
    outs = K.ctc_align_segments(np.concatenate(tabs), cols, off, trs2, 2, 4, 0, ctx=ctx)
    got = align_results(*(o.numpy() for o in outs), [len(t) for t in trs2])
    assert [g[:2] for g in got] == [h[:2] for h in w]
    # no segments at all
    outs = K.ctc_align_segments(np.zeros((0, 6), np.float32), list(range(6)), [0], [], ctx=ctx)
    assert outs[0].numpy().shape == (0, 1, 2) and outs[4].numpy().shape == (0,)


@pytest.mark.gpu
def test_aligner_longest_transcript_and_the_lds_threshold(ctx):
    """L = 511 at T = 600 (16 states a lane, back-pointers in the scratch block); 16 SPL T bytes of back-pointers against 56 KiB:
    SPL 4 fits at T = 896 and not at 897, SPL 16 fits at T = 224 and not at 225"""
    from lele_amd import kernels as K
    rng = np.random.default_rng(79)
    for tag, pairs in (("L 511", [(600, 511), (5, 2)]), ("SPL 4 in LDS", [(896, 40), (7, 3)]), ("SPL 4 beyond", [(897, 40), (7, 3)]),
                       ("SPL 16 in LDS", [(224, 130), (7, 3)]), ("SPL 16 beyond", [(225, 130), (7, 3)])):
        at, off, trs = aligner_batch(rng, "random", pairs)
        trs[0] = tuple(1 + (j + j // 5) % 5 for j in range(len(trs[0])))       # no adjacent equal labels: feasible in L frames
        want = check_aligner(K, ctx, tag, at, off, trs)
        assert want[0][0] and want[1][0]


@pytest.mark.gpu
def test_aligner_bad_transcripts_leave_the_outputs_alone(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    rng = np.random.default_rng(80)
    at, off = table(rng, 30, 6), np.array([0, 10, 30], np.int64)
    cols = [0, 2, 3, 5, 7, 11]
    bufs = [ctx.buf() for _ in range(5)]
    marker = np.arange(1000, 1064, dtype=np.int32)
    for b in bufs:
        b.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(bufs[0]._h)
    o = dict(out_spans=bufs[0], out_scores=bufs[1], out_path=bufs[2], out_total=bufs[3], out_ok=bufs[4], ctx=ctx)
    bad = [(dict(transcripts=[(2, 3), (4,)]), r"segment 1, position 0"),                       # a label that is not listed
           (dict(transcripts=[(2, 0), (3,)]), r"segment 0, position 1"),                       # a label equal to the blank
           (dict(transcripts=[(2,), (2, 3) * 256]), r"segment 1 .* more than 511"),            # L = 512
           (dict(transcripts=[(2,), (2, 3, 5)], width=2), r"segment 1 .* width"),              # longer than the given width
           (dict(transcripts=[(2,), (3,)], blank=1), r"blank"),                                # the blank is not listed
           (dict(transcripts=[(2,), (3,)], cols=[0, 3, 2, 5, 7, 11]), r"cols\[2\]"),
           (dict(transcripts=[(2,), (3,)], out_spans=bufs[1]), r"distinct")]
    for kw, pattern in bad:
        args = dict(o, cols=cols, blank=0, width=0)
        args.update(kw)
        with pytest.raises(_lib.LeleError, match=pattern):
            K.ctc_align_segments(at, args.pop("cols"), off, args.pop("transcripts"), args.pop("blank"), 0, args.pop("width"), **args)
        for b in bufs:
            assert _lib.lib().lele_hip_buf_bytes(b._h) == before and np.array_equal(b.to_numpy((64,), np.int32), marker), pattern
    K.ctc_align_segments(at, cols, off, [(2,), (2, 3) * 255 + (5,)], ctx=ctx)                  # L = 511 is accepted


@pytest.mark.gpu
def test_graph_replay_reads_the_new_input(ctx):
    from lele_amd import kernels as K
    xa, wt, la = dense_case("soft", 3, 50, 512, 300)
    xb = dense_case("random", 3, 50, 512, 300)[0]
    wt = tuple(K.Weight(a.copy()) for a in wt)
    lb = O.fused_quantized_linear(xb, *[w.arr for w in wt])
    off = np.array([0, 50, 100, 150], np.int64)
    cols = [0, 255, 256, 299]
    trs = [(255, 256), (299, 299, 255), ()]
    inp, inp2 = ctx.buf(), ctx.buf()
    outs = [ctx.buf() for _ in range(11)]
    da, pa = inp.upload(xa), inp2.upload(xa.reshape(150, 512))

    def run():
        K.fused_quantized_linear_logprob_at(da, *wt, cols, out_ids=outs[0], out_logprob=outs[1], out_at=outs[2], ctx=ctx)
        _, _, at = K.fused_quantized_linear_logprob_at_segments(pa, off, *wt, cols, out_ids=outs[3], out_logprob=outs[4], out_at=outs[5], ctx=ctx)
        K.ctc_align_segments(at, cols, off, trs, 0, 4, 0, out_spans=outs[6], out_scores=outs[7], out_path=outs[8], out_total=outs[9],
                             out_ok=outs[10], ctx=ctx)

    run()                                                       # one eager run of the same layout, columns and transcripts
    ctx.sync()
    ctx.graph_begin()
    run()
    graph = ctx.graph_end()
    seen = []
    for logits, x in ((la, None), (lb, xb)):
        if x is not None:
            inp.upload(x)
            inp2.upload(x.reshape(150, 512))
        for o in outs[:2] + outs[3:5]:
            o.upload(np.full(150, -7, np.int32))
        graph.launch()
        ids, lp, at = outs[0].to_numpy((3, 50), np.int32), outs[1].to_numpy((3, 50), np.float32), outs[2].to_numpy((3, 50, 4), np.float32)
        assert np.array_equal(ids, N.argmax_last(logits))
        assert np.array_equal(at, at_from(logits, ids, lp, cols))
        assert np.array_equal(bits(outs[5].to_numpy((150, 4), np.float32)), bits(at).reshape(150, 4))
        got = align_results(outs[6].to_numpy((3, 3, 2), np.int32), outs[7].to_numpy((3, 3), np.float32), outs[8].to_numpy((3,), np.float32),
                            outs[9].to_numpy((3,), np.float32), outs[10].to_numpy((3,), np.int32), [2, 3, 0])
        for i in range(3):
            h = ctc_forced_align(at.reshape(150, 4)[off[i]:off[i + 1]], cols, trs[i], 0, 4)
            assert got[i][:2] == h[:2] and got[i][2] == [float(np.float32(v)) for v in h[2]] and got[i][3] == float(np.float32(h[3]))
        seen.append(at.copy())
    assert not np.array_equal(seen[0], seen[1])
    graph.close()


@pytest.mark.gpu
def test_encoder_align_segments_end_to_end(ctx):
    from sensevoice_graph import VOCAB, Encoder
    enc = Encoder(ctx, layers=2, seed=3)
    rng = np.random.default_rng(11)
    off = np.array([0, 7, 28], np.int64)
    pf = ctx.buf().upload(rng.standard_normal((28, 560)).astype(np.float32))
    # the arg-max transcript of every utterance: its greedy path behind the prompt rows, collapsed
    skip = np.zeros(VOCAB, np.uint8)
    skip[0] = 1
    gi, gf, _, gc = (a.numpy().copy() for a in enc.greedy_segments_scored(pf, off, skip))
    trs, where = [], []
    for i in range(2):
        ids, frames = gi[i, :gc[i]], gf[i, :gc[i]]
        ids, frames = ids[frames >= 4], frames[frames >= 4]
        runs = []                                             # (label, its frames): equal ids at adjacent frames are one label
        for v, f in zip(ids.tolist(), frames.tolist()):
            if runs and runs[-1][0] == v and runs[-1][1][-1] == f - 1:
                runs[-1][1].append(f)
            else:
                runs.append((v, [f]))
        trs.append(tuple(v for v, _ in runs))
        where.append([fr for _, fr in runs])
    long = max(trs, key=len)
    assert len(long) >= 2
    outs = tuple(o.numpy().copy() for o in enc.align_segments(pf, off, trs))
    got = align_results(*outs, [len(t) for t in trs])
    # the reference: the oracle's logits of the projection's input, their float64 log-soft-max columns rounded to f32
    cols = enc.align_cols(trs)
    _, xn, off4 = enc.trunk_segments(pf, off)
    xn, off4, p = xn.numpy().copy(), np.asarray(off4), enc.ctc
    assert list(off4) == [0, 11, 36]
    for i in range(2):
        logits = O.fused_quantized_linear(xn[off4[i]:off4[i + 1]][None], p.w.arr, p.scale.arr, p.zero.arr, p.bias.arr)[0]
        ok, spans, _, _, _ = ctc_forced_align(log_softmax64(logits)[:, cols].astype(np.float32), cols, trs[i], 0, 4)
        assert ok and got[i][0] and got[i][1] == spans, i
        # the span of a label contains the frames at which greedy decoding emitted it
        for j, (f, l) in enumerate(got[i][1]):
            assert f <= where[i][j][0] and where[i][j][-1] <= l, (i, j, f, l, where[i][j])
        assert (token_times(np.array([s[0] for s in got[i][1]])) >= 0).all()
    # the dense form: both utterances of one length
    df = ctx.buf().upload(rng.standard_normal((2, 9, 560)).astype(np.float32))
    dense = align_results(*(o.numpy().copy() for o in enc.align(df, [long[:1], long[:2]])), [1, 2])
    assert len(dense) == 2 and all(len(d[1]) == n for d, n in zip(dense, (1, 2)) if d[0])
