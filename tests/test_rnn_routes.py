"""Every LSTM / GRU route (lele_amd/csrc/rnn.hip) against the oracle bit for bit: one table row per dispatch branch and threshold side.

The single calls (rnn_kernel) report "rnn.lstm" / "rnn.gru" and the GEMM kernel that computed W x; the packed calls (rnn_seg_kernel) report
"rnns.lstm" / "rnns.gru" and the kernel form: recurrent weights in registers in slices of 16 / 32 / 64 ("rnns.reg16" ...), or streamed with
1 / 2 / 4 / 8 members a register tile ("rnns.stream1" ...).  Every row names the route the library must report (kernels.last_route()) and
the shape that selects it, so a re-tune that moves a shape to another kernel fails here instead of leaving that kernel untested.

Why bits.  oracle/simd_math.cpp::orc_lstm / orc_gru take each dot product in float64, round it once and run the reference's AVX2 gate
code, so the device equals the oracle bit for bit, at every step and for any bias and initial state, whenever both dot products are
exact in every summation order:
  * W x: x in k/8, W in k/64, I <= 64 -- every partial sum is an integer multiple of 2^-9 below 2^7;
  * R h: every row of R has at most one nonzero, from {-2, -1, 1, 2} -- the product is an exact scaling, every other fma of the chain,
    every join (a0 + a1) + (a2 + a3) and every slice sum adds a zero.
Which k a row reads is chosen so that every slice, each of the four accumulators, the remainder loop and the first and last k of every
slice are read (routing_gaps): a wrong slice bound, a dropped or doubled k is an O(1) error, a wrong association or activation a bit.
Hidden elements k >= (H & ~7), the tail, go through libm, the device's own: rows of body elements read body k only, so the body stays
exact over all steps; tail elements are judged at 16 ulp on a probe step 0 (x_0 = 0, input and output gates held open by the bias, a
cell-gate pre-activation of 1e-4 .. 3e-4 chosen where the polynomial tanh and libm's are 3e-5 relative apart or more: probe_values) and
at the 1e-4 bar after it.  Measured on an MI355X: the device's tail is at most 2 ulp from glibc's on the probe step, 6e-8 absolute after.

Families per row: "exact" (above), "random" (ordinary random R, the 1e-4 bar of tests/test_conv_rnn.py; packed == single bit for bit),
"saturate" (biases +-30, +-88, +-100, +-1e4 on the exact operands, bit for bit; the tail's gates at -+1e4, where body and tail give exact
zeros and ones), and on a few rows a NaN / an infinity in one x row (classes from that step on).

Oracle against float64 (test_oracle_against_float64): measured over all rows of the table on the exact family, the oracle stays within
5.6e-7 (y) and 6.2e-6 (c; the T = 40 row, where |c| reaches 24 -- 7.0e-7 on every other row) absolute of the plain float64 LSTM / GRU
below; the bounds Y_BOUND / C_BOUND are four times that, for rows not yet seen.

CPU part: name coverage, every row against the dispatch restated in Python for 256 CUs, which (kind, KS) pairs any H can select, the
operands' exactness, the routing coverage, the oracle against float64, emulated wrong kernels against the acceptance functions.
GPU part: every row asserts last_route() and then the values."""
import functools
import os
import re

import numpy as np
import pytest

CUS = 256
RTOL = 1e-4          # tests/test_conv_rnn.py
PROBE_ULP = 16       # the tail on the probe step: 2e-6 relative, fifteen times under the 3.1e-5 that part the polynomial and libm
Y_BOUND, C_BOUND = 4 * 5.6e-7, 4 * 6.2e-6
PREFIXES = ("rnn.", "rnns.")
THREADS = 1024
LDS_LIMIT = 160 * 1024
POOL = 13            # a packed row draws its segments from at most 5 * POOL distinct ones: the 8 members of a workgroup are always distinct

# what no row asserts, and why (a key that is a route name takes that name out of the coverage requirement; there is none)
NOT_COVERED = {
    "hidden_size beyond the LDS limit": "an error, not a route: tests/test_rnn_segments.py::test_invalid_calls_raise_and_leave_the_outs_untouched",
    "R > 65535 * 64 rows / count >= 2^28": "the size guards of the packed call need a 4-million-row batch",
    "LELE_HIP_RNN_SEG_FORM=2": "the A/B switch of tools/rnn_segments_bench.py sends the register shapes to the streamed kernels the H = 20 rows pin",
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def accept_bits(got, want):
    """tests/test_eltwise_routes.py::accept_bits: "" when got == want bit for bit (any NaN where the reference yields a NaN, the NaN
    masks equal), else what differs; no element is dropped"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, want %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (bits(got) != bits(want)))
    if not bad.any():
        return ""
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d of %d differ, the first at %s: got %r want %r" % (int(bad.sum()), bad.size, at, got[at], want[at])


def accept_close(got, want, tol=RTOL):
    """tests/test_conv_rnn.py::_close as a verdict: |got - want| <= tol |want| + tol rms(want) + 1e-7, element by element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    if not want.size:
        return ""
    floor = tol * float(np.sqrt(np.mean(np.square(want)))) + 1e-7
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= tol * np.abs(want) + floor)
    return "" if not bad.any() else "%d of %d outside %g (max |diff| %.3e)" % (int(bad.sum()), want.size, tol, float(np.nanmax(np.abs(got - want))))


def accept_ulp(got, want, ulps=PROBE_ULP):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    dist = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return "" if not want.size or np.all(dist <= ulps) else "the probe step's tail is %.1f ulp from libm's (bar %d)" % (float(dist.max()), ulps)


def klass(v):
    """NaN 0, +inf 1, -inf 2, finite 3"""
    v = np.asarray(v, np.float32)
    return np.where(np.isnan(v), 0, np.where(np.isinf(v), np.where(v > 0, 1, 2), 3))


def accept_rnn(H, got, want, family):
    """one sequence: got / want = (y [T, H], h [H], c [H] or None).  "exact": body by bits, tail at PROBE_ULP on step 0 and at RTOL
    behind it; "saturate": every element by bits; "random": every element at RTOL.  "" or what is wrong"""
    body = H & ~7
    (gy, gh, gc), (wy, wh, wc) = got, want
    T = wy.shape[0]
    if gy.shape != wy.shape or gh.shape != wh.shape:
        return "shapes %s %s, want %s %s" % (gy.shape, gh.shape, wy.shape, wh.shape)
    if T:   # the final h is the last y
        msg = accept_bits(gh, gy[-1])
        if msg:
            return "h is not the last y: " + msg
    pairs = [("y", gy, wy), ("h", gh[None], wh[None])] + ([] if wc is None else [("c", gc[None], wc[None])])
    for name, g, w in pairs:
        if family == "random":
            msg = accept_close(g, w)
        elif family == "saturate":
            msg = accept_bits(g, w)
        else:
            msg = accept_bits(g[:, :body], w[:, :body])
            if not msg and body < H and w.shape[0]:
                first = name == "y" or T == 1   # h and c are step 0's only when there is no other step
                if first and T:
                    msg = accept_ulp(g[0, body:], w[0, body:])
                if not msg and g.shape[0] > 1:
                    msg = accept_close(g[1:, body:], w[1:, body:])
                if not msg and not first:
                    msg = accept_close(g[:, body:], w[:, body:])
        if msg:
            return "%s: %s" % (name, msg)
    return ""


def accept_classes(got, want, H, t0):
    """a NaN / an infinity enters at step t0: bits in the body before it, the same classes (NaN / +inf / -inf / finite) from it on"""
    body = H & ~7
    (gy, gh, gc), (wy, wh, wc) = got, want
    msg = accept_bits(gy[:t0, :body], wy[:t0, :body])
    if msg:
        return "before the special value: " + msg
    for name, g, w in (("y", gy[t0:], wy[t0:]), ("h", gh, wh)) + (() if wc is None else (("c", gc, wc),)):
        if g.shape != w.shape or not np.array_equal(klass(g), klass(w)):
            return "%s: classes differ: got %s want %s" % (name, klass(g).reshape(-1)[:16], klass(w).reshape(-1)[:16])
    return ""


# ================================================================================================= the dispatch, restated
def ng_of(kind):
    return 4 if kind == "lstm" else 3


def slices_of(kind, H):
    """S of rnn_kernel / rnn_seg_kernel: thread (s, g) sums k in [s H / S, (s + 1) H / S)"""
    G = ng_of(kind) * H
    return min(H, max(1, THREADS // G))


def ks_of(kind, H, restricted=True):
    """the register-stationary slice length, 0 = streamed; restricted=False: the rule before the per-kind list of instantiations"""
    G, S = ng_of(kind) * H, slices_of(kind, H)
    ks = H // S if H % S == 0 and S * G <= THREADS else 0
    allowed = ((16 if kind == "lstm" else 32), 64) if restricted else (16, 32, 64)
    return ks if ks in allowed else 0


def seg_bytes(kind, H):
    return (2 * H + slices_of(kind, H) * ng_of(kind) * H) * 4


def ns_of(kind, H, count, cus=CUS):
    if count <= cus:
        return 1
    return min(8, (count + cus - 1) // cus, LDS_LIMIT // seg_bytes(kind, H))


def packed_route(kind, H, lengths, cus=CUS):
    if sum(lengths) == 0:
        return ""
    ks, ns = ks_of(kind, H), ns_of(kind, H, len(lengths), cus)
    form = "reg%d" % ks if ks else "stream%d" % (1 if ns == 1 else 2 if ns == 2 else 4 if ns <= 4 else 8)
    return "rnns.%s/rnns.%s" % (kind, form)


def gemm_route(M, N, K, cus=CUS):
    """gemm::launch for two k-contiguous operands, no statistics, batch 1"""
    if M <= 0 or N <= 0:
        return ""
    if K <= 0:
        return "gemm.k0"
    if K >= 8 and M <= 4 and N >= 8:
        return "gemm.thin_m"
    if K >= 8 and N <= 4 and M >= 8:
        return "gemm.thin_n"
    if ((M + 63) // 64) * ((N + 63) // 64) < 2 * cus and K >= 16:
        return "gemm.small"
    best, best_score = None, -1.0
    for bm, bn, base in ((128, 128, 1.0), (64, 256, 0.92), (64, 64, 0.70), (32, 128, 0.55), (256, 128, 1.10)):
        tm, tn = float((M + bm - 1) // bm), float((N + bn - 1) // bn)
        eff = (float(M) * N) / (tm * bm * tn * bn)
        blocks = tm * tn
        score = eff * base * (1.0 if blocks >= 2.0 * cus else blocks / (2.0 * cus))
        if score > best_score:
            best, best_score = "gemm.tile%dx%d" % (bm, bn), score
    return best


def single_route(kind, H, I, T, cus=CUS):
    core = gemm_route(T, ng_of(kind) * H, I, cus)
    return "rnn.%s" % kind + ("/" + core if core else "")


# ================================================================================================================ the table
def row(kind, entry, H, I, lengths, given, route, why):
    """lengths: the step count of a single call, the list of segment lengths of a packed one, or a function of the CU count"""
    return dict(kind=kind, entry=entry, H=H, I=I, lengths=lengths, given=given, route=route, why=why,
                id="%s-%s-H%d-I%d-%s" % (kind, entry, H, I, re.sub(r"[^a-z0-9]+", "_", why.lower())[:40].strip("_")))


def mixed(count, longest=5):
    """count lengths that mix 0, 1, 2 and one longer segment: the same five-cycle whatever the count"""
    return [[1, 0, 2, 1, longest][i % 5] for i in range(count)]


ROWS = []
for _k in ("lstm", "gru"):
    ROWS += [
        row(_k, "single", 1, 7, 3, True, "rnn.%s/gemm.tile64x64" % _k, "H = 1: one gate element, all tail; I = 7 the scalar loader"),
        row(_k, "single", 7, 16, 4, True, "rnn.%s/gemm.thin_m" % _k, "H = 7: all tail, slices of one k"),
        row(_k, "single", 8, 0, 3, True, "rnn.%s/gemm.k0" % _k, "H = 8: no tail; I = 0, W x is the epilogue alone"),
        row(_k, "single", 20, 64, 5, True, "rnn.%s/gemm.small" % _k, "H = 20: unequal slices (LSTM S = 12, GRU S = 17), a tail of 4; I = 64 vector loader"),
        row(_k, "single", 72, 16, 4, False, "rnn.%s/gemm.thin_m" % _k, "H = 72: LSTM slices of 24, GRU slices of 18 (four rounds and a remainder of 2); no bias, no state"),
        row(_k, "single", 128, 16, 6, True, "rnn.%s/gemm.small" % _k, "H = 128: the VAD size, S = 2"),
        row(_k, "single", 264, 7, 3, True, "rnn.%s/gemm.tile64x64" % _k, "H = 264: S = 1; LSTM G = 1056 > 1024, the strided GEMV loop"),
        row(_k, "single", 1029, 16, 3, True, "rnn.%s/gemm.thin_m" % _k, "H = 1029: the second gate pass is all tail"),
        row(_k, "single", 1040, 7, 3, False, "rnn.%s/gemm.tile64x64" % _k, "H = 1040: the second gate pass has body elements; no bias, no state"),
        row(_k, "single", 128, 64, 40, True, "rnn.%s/gemm.small" % _k, "T = 40: drift over many steps"),
        row(_k, "single", 20, 16, 0, True, "rnn.%s" % _k, "T = 0: no step, the state comes back"),
    ]
ROWS.append(row("gru", "single", 344, 16, 3, True, "rnn.gru/gemm.thin_m", "H = 344: GRU G = 1032 > 1024, the strided GEMV loop"))
for _k, _h in (("lstm", 64), ("lstm", 128), ("gru", 96), ("gru", 128)):
    _form = "rnns.%s/rnns.reg%d" % (_k, {("lstm", 64): 16, ("gru", 96): 32}.get((_k, _h), 64))
    ROWS += [
        row(_k, "packed", _h, 16, lambda cus: mixed(5), True, _form, "register form, ns = 1: count 5"),
        row(_k, "packed", _h, 16, lambda cus: mixed(cus + 1), True, _form, "register form, ns = 2: count = cus + 1, one pair"),
        row(_k, "packed", _h, 16, lambda cus: mixed(2 * cus + 1), _h != 128, _form, "register form, ns = 3: count = 2 cus + 1, the odd member of the pairwise walk"),
    ]
for _k in ("lstm", "gru"):
    for _n, _c, _f, _w in ((1, lambda cus: cus, 1, "count = cus"), (2, lambda cus: cus + 1, 2, "count = cus + 1"), (2, lambda cus: 2 * cus, 2, "count = 2 cus"),
                           (3, lambda cus: 2 * cus + 1, 4, "count = 2 cus + 1: a padding slot in the tile of 4"), (4, lambda cus: 4 * cus, 4, "count = 4 cus"),
                           (5, lambda cus: 4 * cus + 1, 8, "count = 4 cus + 1: three padding slots in the tile of 8"),
                           (7, lambda cus: 7 * cus, 8, "count = 7 cus"), (8, lambda cus: 7 * cus + 1, 8, "count = 7 cus + 1: the cap of 8")):
        ROWS.append(row(_k, "packed", 20, 16, (lambda c: lambda cus: mixed(c(cus)))(_c), True, "rnns.%s/rnns.stream%d" % (_k, _f), "streamed, ns = %d: %s" % (_n, _w)))
ROWS += [
    row("lstm", "packed", 1029, 7, lambda cus: mixed(7 * cus + 1, 3), True, "rnns.lstm/rnns.stream8", "streamed, ns = 6: count = 7 cus + 1 asks for 8, 160 KiB of LDS hold 6"),
    row("gru", "packed", 20, 0, lambda cus: mixed(5), True, "rnns.gru/rnns.stream1", "I = 0 packed: W x is the epilogue alone"),
    row("lstm", "packed", 128, 0, lambda cus: mixed(3), False, "rnns.lstm/rnns.reg64", "I = 0 packed, register form; no bias, no state"),
    row("lstm", "packed", 20, 16, lambda cus: [0, 0, 0], True, "", "R = 0: nothing launched, the state is handed on"),
    row("gru", "packed", 128, 16, lambda cus: [0, 0], True, "", "R = 0: nothing launched, the state is handed on"),
]
IDS = [r["id"] for r in ROWS]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)
SPECIAL_ROWS = [r for r in ROWS if (r["entry"], r["H"], r["I"]) in (("single", 20, 64), ("single", 128, 16)) or (r["entry"] == "packed" and r["H"] == 20 and "ns = 3" in r["why"])]


def lengths_of(r, cus=CUS):
    return r["lengths"](cus) if callable(r["lengths"]) else r["lengths"]


def route_of(r, cus=CUS):
    if r["entry"] == "single":
        return single_route(r["kind"], r["H"], r["I"], r["lengths"], cus)
    return packed_route(r["kind"], r["H"], lengths_of(r, cus), cus)


# ================================================================================================================= operands
def slice_bounds(kind, H):
    S = slices_of(kind, H)
    return [(s * H // S, (s + 1) * H // S) for s in range(S)]


def wanted_k(kind, H):
    """the k that a routing must read: per slice the first and the last, one of each accumulator of the unrolled rounds, one of the
    remainder loop"""
    need = set()
    for k0, k1 in slice_bounds(kind, H):
        rounds = (k1 - k0) // 4
        need |= {k0, k1 - 1}
        if rounds:
            need |= {k0 + 4 * (rounds - 1) + a for a in range(4)}
        if (k1 - k0) % 4:
            need.add(k0 + 4 * rounds)
    return need


def routing_gaps(kind, H, r):
    """what the nonzeros of r [G, H] leave unread: "" or the missing cases; rows of body elements may read body k only"""
    body, gaps = H & ~7, []
    g, k = np.nonzero(r)
    if len(g) and np.bincount(g).max() > 1:
        gaps.append("a row with two nonzeros")
    if not set(np.unique(np.abs(r[g, k])).tolist()) <= {1.0, 2.0}:
        gaps.append("a value outside {-2, -1, 1, 2}")
    if np.any((g % H < body) & (k >= body)):
        gaps.append("a body row reads a tail k")
    read = set(k.tolist())
    for s, (k0, k1) in enumerate(slice_bounds(kind, H)):
        rounds = (k1 - k0) // 4
        if not read & set(range(k0, k1)):
            gaps.append("slice %d unread" % s)
        if k0 not in read or k1 - 1 not in read:
            gaps.append("slice %d: first / last k unread" % s)
        for a in range(4 if rounds else 0):
            if not read & {k0 + 4 * j + a for j in range(rounds)}:
                gaps.append("slice %d: accumulator %d unread" % (s, a))
        if (k1 - k0) % 4 and not read & set(range(k0 + 4 * rounds, k1)):
            gaps.append("slice %d: remainder unread" % s)
    return "; ".join(gaps)


def routing(rng, kind, H):
    """R [G, H] with one nonzero a row at most.  The tail's cell-gate rows (LSTM c, GRU h) stay zero: the probe step wants their
    pre-activation from the bias alone"""
    NG, body = ng_of(kind), H & ~7
    G = NG * H
    r = np.zeros((G, H), np.float32)
    col = np.full(G, -1, np.int64)
    elem = np.arange(G) % H
    cell = NG - 1
    tail_rows = [g for g in range(G) if elem[g] >= body and g // H != cell]
    body_rows = rng.permutation([g for g in range(G) if elem[g] < body]).tolist()
    need = sorted(wanted_k(kind, H))
    need_tail, need_body = [k for k in need if k >= body], [k for k in need if k < body]
    assert len(need_tail) <= len(tail_rows) and len(need_body) <= len(body_rows), (kind, H)
    for g, k in zip(tail_rows, need_tail):
        col[g] = k
    for g, k in zip(body_rows, need_body):
        col[g] = k
    free_tail = tail_rows[len(need_tail):]
    free_body = np.array(body_rows[len(need_body):], np.int64)
    if len(free_tail):
        col[free_tail] = rng.integers(0, H, len(free_tail))
    if len(free_body):
        pick = rng.integers(0, body, len(free_body))
        col[free_body] = np.where(rng.random(len(free_body)) < 0.1, -1, pick)   # one row in ten stays zero
    live = np.nonzero(col >= 0)[0]
    r[live, col[live]] = rng.choice(np.float32([-2, -1, 1, 2]), len(live))
    return r


SEPARATION = 3e-5   # what parts the polynomial tanh from libm's on the probe step, relative: probe_values keeps nothing closer


def tanh_gap(u, twice):
    """the oracle's polynomial tanh against float64's at u (and again at the result: the LSTM's h = o tanh(c)), relative"""
    from oracle import pyoracle as orc
    poly = lambda v: orc.unary("tanh", np.concatenate([v, np.zeros(-len(v) % 8, np.float32)]))[:len(v)]   # noqa: E731
    u = np.asarray(u, np.float32)
    t1 = np.tanh(u.astype(np.float64))
    p1 = poly(u)
    gap = np.abs(p1 - t1) / t1
    if twice:
        t2 = np.tanh(t1.astype(np.float32).astype(np.float64))
        gap = np.minimum(gap, np.abs(poly(p1) - t2) / t2)
    return gap


def probe_values(rng, n, twice):
    """n cell-gate pre-activations in 1e-4 .. 3e-4.  The polynomial's error there is its rounding noise, 3.7e-5 of the value in the
    median and next to nothing at one value in thirteen: only values where it is SEPARATION or more are kept"""
    out = np.zeros(0, np.float32)
    while len(out) < n:
        u = rng.uniform(1e-4, 3e-4, 4 * n + 8).astype(np.float32)
        out = np.concatenate([out, u[tanh_gap(u, twice) >= SEPARATION]])
    return out[:n]


SATURATING = np.float32([30, -30, 88, -88, 100, -100, 1e4, -1e4])


def operands(r, family, cus=CUS):
    """everything one row needs, the same on every machine with `cus` CUs: x [R, I], w [1, G, I], r [1, G, H], b [1, 2G] or None, the pool
    of distinct segments {length, h0, c0, first row in x} and which pool member each segment is.  A single call is one segment"""
    kind, H, I = r["kind"], r["H"], r["I"]
    NG, body = ng_of(kind), r["H"] & ~7
    G = NG * H
    rng = np.random.default_rng([ROWS.index(r), ("exact", "random", "saturate").index(family)])
    lengths = [r["lengths"]] if r["entry"] == "single" else lengths_of(r, cus)
    count = len(lengths)
    period = 5 * POOL if count > 5 * POOL else count   # lengths repeat with period 5: pool member i % period keeps segment i's length
    member = np.arange(count) % period
    plen = lengths[:period]
    w = (rng.integers(-64, 65, (1, G, I)) / 64.0).astype(np.float32)
    if family == "random":
        rr = (rng.standard_normal((G, H)) / np.sqrt(H)).astype(np.float32)
    else:
        rr = routing(rng, kind, H)
    b = None
    if r["given"]:
        b = (rng.standard_normal((2, NG, H)) * 2).astype(np.float32)
        if family == "saturate":
            b[0] = SATURATING[(np.arange(NG)[:, None] * 3 + np.arange(H)[None, :]) % len(SATURATING)]
            if kind == "lstm":
                b[0, :3, body:] = -1e4    # the tail's i, o, f: exact zeros through libm, c_t = h_t = +-0
            else:
                b[0, 2] = np.where(b[0, 2] < -30, -b[0, 2], b[0, 2])   # the reference's polynomial tanh is NaN below -44.5: h would be NaN from step 0 on
                b[0, 0, body:] = 1e4      # the tail's z: exactly one, h_t = h_{t-1}
        elif family == "exact" and body < H:
            u = probe_values(rng, H - body, kind == "lstm")
            b[:, NG - 1, body:] = [u, np.zeros_like(u)]            # the cell gate's pre-activation on the probe step
            if kind == "lstm":
                b[:, :2, body:] = np.float32([[[30.0]], [[0.0]]])    # i, o open: 1 / (1 + expf(-26 or more)) == 1
            else:
                b[:, 0, body:] = np.float32([[-100.0], [0.0]])       # z shut: 1 / (1 + expf(96 or more)) == 0
        b = b.reshape(1, 2 * G)
    assert family != "exact" or body == H or r["given"], "a row with a tail needs the bias for its probe step"
    pool = []
    for ln in plen:
        x = (rng.integers(-8, 9, (ln, I)) / 8.0).astype(np.float32)
        if family == "exact" and body < H and ln:
            x[0] = 0   # the probe step
        h0 = c0 = None
        if r["given"]:
            h0 = np.clip(rng.standard_normal(H) * 0.5, -2, 2).astype(np.float32)
            c0 = (rng.standard_normal(H) * 0.5).astype(np.float32)
            if family == "exact":
                c0[body:] = 0
        pool.append(dict(length=ln, h0=h0, c0=c0 if kind == "lstm" else None, x=x))
    x = np.concatenate([pool[m]["x"] for m in member]) if count else np.zeros((0, I), np.float32)
    return dict(x=x.reshape(sum(lengths), I), w=w, r=rr.reshape(1, G, H), b=b, pool=pool, member=member, lengths=lengths)


def oracle_run(orc, kind, op, p, x=None, r=None, b="same", h0="same"):
    """the oracle on one segment: (y [T, H], h [H], c [H] or None)"""
    x = p["x"] if x is None else x
    r = op["r"] if r is None else r
    b = op["b"] if isinstance(b, str) else b
    h0 = p["h0"] if isinstance(h0, str) else h0
    H = r.shape[2]
    x3 = x.reshape(len(x), 1, x.shape[1])
    hh = None if h0 is None else h0.reshape(1, 1, H)
    if kind == "lstm":
        y, h, c = orc.lstm(x3, op["w"], r, b, hh, None if p["c0"] is None else p["c0"].reshape(1, 1, H))
        return y.reshape(-1, H), h.reshape(H), c.reshape(H)
    y, h = orc.gru(x3, op["w"], r, b, hh)
    return y.reshape(-1, H), h.reshape(H), None


def float64_run(kind, op, p):
    """a plain float64 LSTM (gates i, o, f, c) / GRU (z, r, h; the linear-before-reset form): (y, h, c or None)"""
    H = op["r"].shape[2]
    NG = ng_of(kind)
    w, r = op["w"][0].astype(np.float64), op["r"][0].astype(np.float64)
    b = np.zeros((2, NG, H)) if op["b"] is None else op["b"].astype(np.float64).reshape(2, NG, H)
    h = np.zeros(H) if p["h0"] is None else p["h0"].astype(np.float64)
    c = np.zeros(H) if p["c0"] is None else p["c0"].astype(np.float64)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))   # noqa: E731
    ys = []
    for xt in p["x"].astype(np.float64):
        wc, rc = (w @ xt).reshape(NG, H), (r @ h).reshape(NG, H)
        if kind == "lstm":
            g = wc + rc + b[0] + b[1]
            c = sig(g[2]) * c + sig(g[0]) * np.tanh(g[3])
            h = sig(g[1]) * np.tanh(c)
        else:
            z, rg = sig(wc[0] + rc[0] + b[0, 0] + b[1, 0]), sig(wc[1] + rc[1] + b[0, 1] + b[1, 1])
            h = (1.0 - z) * np.tanh(wc[2] + b[0, 2] + rg * (rc[2] + b[1, 2])) + z * h
        ys.append(h.copy())
    return np.array(ys).reshape(-1, H), h, c if kind == "lstm" else None


@functools.lru_cache(maxsize=12)
def reference(index, family, cus):
    """a row's operands and the oracle's result for every pool member: computed once, shared, never written to"""
    from oracle import pyoracle as orc
    r = ROWS[index]
    op = operands(r, family, cus)
    want = [oracle_run(orc, r["kind"], op, p) for p in op["pool"]]
    for a in [op["x"], op["w"], op["r"]] + [v for t in want for v in t if v is not None]:
        a.setflags(write=False)
    return op, want


# ================================================================================================================ CPU tests
def test_rows_cover_every_rnn_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}
    assert len(mine) == 11
    used = {lvl for r in ROWS for lvl in r["route"].split("/") if lvl.startswith(PREFIXES)}
    named = set(NOT_COVERED) & set(names)
    assert not (used | named) - mine, "routes the library cannot report: %s" % sorted((used | named) - mine)
    assert mine - used == named, "routes no row reaches: %s" % sorted(mine - used - named)
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_COVERED.values())
    # the W x levels of the single calls are the GEMM's own names
    assert {r["route"].split("/")[1] for r in ROWS if r["route"].count("/") and r["entry"] == "single"} <= set(names)


def test_rows_satisfy_the_dispatch_they_state():
    for r in ROWS:
        assert route_of(r) == r["route"], r["id"]
        if r["entry"] == "packed":   # the rule in terms of the CU count holds on a smaller and a larger device as well
            assert packed_route(r["kind"], r["H"], lengths_of(r, 64), 64) == r["route"] == packed_route(r["kind"], r["H"], lengths_of(r, 304), 304), r["id"]
    at = lambda kind, H, count: (ks_of(kind, H), ns_of(kind, H, count))   # noqa: E731
    # the shapes the issue names
    assert (slices_of("lstm", 20), slices_of("gru", 20)) == (12, 17) and slice_bounds("lstm", 72)[0] == (0, 24) and slice_bounds("gru", 72)[1] == (18, 36)
    assert slices_of("lstm", 7) == 7 and slices_of("gru", 7) == 7 and slices_of("lstm", 264) == 1 and slices_of("gru", 1) == 1
    assert len({b - a for a, b in slice_bounds("lstm", 20)}) > 1 and len({b - a for a, b in slice_bounds("gru", 20)}) > 1   # unequal slices
    assert 4 * 264 > THREADS and 3 * 344 > THREADS and 3 * 1029 > 2 * THREADS and slices_of("gru", 344) == 1   # G > 1024: the GEMV loop's second and third pass
    assert 1029 > THREADS and (1029 & ~7) == 1024 and (1040 & ~7) == 1040   # the gate loop's second pass: all tail / body
    assert (ks_of("lstm", 64), ks_of("lstm", 128), ks_of("gru", 96), ks_of("gru", 128), ks_of("lstm", 20), ks_of("lstm", 256)) == (16, 64, 32, 64, 0, 0)
    # every ns the streamed rows state, on both sides of every boundary
    seen = {}
    for r in ROWS:
        if r["entry"] == "packed" and r["route"]:
            seen.setdefault((r["kind"], r["route"].split(".")[-1]), set()).add(ns_of(r["kind"], r["H"], len(lengths_of(r))))
    for kind in ("lstm", "gru"):
        assert seen[(kind, "stream1")] >= {1} and seen[(kind, "stream2")] == {2} and seen[(kind, "stream4")] == {3, 4}
        assert seen[(kind, "stream8")] >= {5, 7, 8}
        assert [ns_of(kind, 20, c) for c in (CUS, CUS + 1, 2 * CUS, 2 * CUS + 1, 4 * CUS, 4 * CUS + 1, 7 * CUS, 7 * CUS + 1, 100 * CUS)] == [1, 2, 2, 3, 4, 5, 7, 8, 8]
    assert seen[("lstm", "reg16")] == seen[("lstm", "reg64")] == seen[("gru", "reg32")] == seen[("gru", "reg64")] == {1, 2, 3}
    # the LDS clamp decides on exactly one row: 8 asked for, 6 fit
    assert at("lstm", 1029, 7 * CUS + 1) == (0, 6) and LDS_LIMIT // seg_bytes("lstm", 1029) == 6 and 6 in seen[("lstm", "stream8")]
    assert all(LDS_LIMIT // seg_bytes(r["kind"], r["H"]) >= 8 for r in ROWS if r["entry"] == "packed" and r["H"] != 1029)
    # the W x routes of the single calls: k0, the scalar and the vector loader, three GEMM kernels
    assert {r["I"] for r in ROWS if r["entry"] == "single"} == {0, 7, 16, 64}
    assert {r["route"].split("/")[-1] for r in ROWS if r["entry"] == "single"} >= {"gemm.k0", "gemm.thin_m", "gemm.small", "gemm.tile64x64"}
    assert all(r["I"] <= 64 for r in ROWS)


def test_which_register_forms_any_hidden_size_can_select():
    """S = min(H, max(1, 1024 / G)) and H = S * KS leave four (kind, KS) pairs: the LSTM never has slices of 32, the GRU never slices of
    16 -- the dispatch holds no such instantiation"""
    got = {}
    for kind in ("lstm", "gru"):
        for H in range(1, 7001):
            ks = ks_of(kind, H, restricted=False)
            if ks:
                got.setdefault((kind, ks), []).append(H)
            assert ks_of(kind, H) == ks, (kind, H)   # the per-kind list drops nothing any H selects
    assert got == {("lstm", 16): [64], ("lstm", 64): [128], ("gru", 32): [96], ("gru", 64): [128]}
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lele_amd", "csrc", "rnn.hip")).read()
    assert "ks != (MODE == 0 ? 16 : 32) && ks != 64" in src and "LELE_RNN_SEG(2, 32)" not in src and "LELE_RNN_SEG(2, 16)" not in src


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_operands_are_exact_and_the_routing_reads_every_case(r, orc):
    """W x and R h recomputed in float64 in two summation orders and in f32: identical; the routing's coverage asserted"""
    kind, H, I = r["kind"], r["H"], r["I"]
    for family in ("exact", "saturate"):
        op, want = reference(ROWS.index(r), family, CUS)
        assert routing_gaps(kind, H, op["r"][0]) == "", (family, routing_gaps(kind, H, op["r"][0]))
        x, w, rr = op["x"], op["w"][0], op["r"][0]
        assert np.array_equal(x * 8, np.round(x * 8)) and np.array_equal(w * 64, np.round(w * 64)) and I <= 64
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        fwd = x64 @ w64.T
        rev = x64[:, ::-1] @ w64[:, ::-1].T
        assert np.array_equal(fwd, rev) and np.array_equal(fwd, (x @ w.T).astype(np.float64)) and np.array_equal(fwd, fwd.astype(np.float32))
        states = [p["h0"] for p in op["pool"] if p["h0"] is not None] + [y for y, _, _ in want if len(y)]
        if states:
            h = np.concatenate([s.reshape(-1, H) for s in states])
            h64, r64 = h.astype(np.float64), rr.astype(np.float64)
            fwd = h64 @ r64.T
            rev = h64[:, ::-1] @ r64[:, ::-1].T
            assert np.array_equal(fwd, rev) and np.array_equal(fwd, (h @ rr.T).astype(np.float64)) and np.array_equal(fwd, fwd.astype(np.float32))
    if H & 7 and r["lengths"] != 0:   # the probe step: what parts the polynomial tanh from libm's is many times the bar
        op, want = reference(ROWS.index(r), "exact", CUS)
        body = H & ~7
        for p, (y, h, c) in zip(op["pool"], want):
            if p["length"]:
                u = op["b"].reshape(2, ng_of(kind), H)[0, -1, body:]
                assert np.all((u >= np.float32(1e-4)) & (u <= np.float32(3e-4)))
                assert accept_ulp(y[0, body:], np.tanh(np.tanh(u.astype(np.float64)) if kind == "lstm" else u.astype(np.float64)).astype(np.float32), 4) == ""
                assert np.all(tanh_gap(u, kind == "lstm") >= SEPARATION) and SEPARATION > 15 * PROBE_ULP * 2.0 ** -24


def test_oracle_against_float64():
    """the oracle within Y_BOUND / C_BOUND (absolute) of the float64 recurrence on every row's exact operands; the measured maxima are
    5.6e-7 on y (GRU H = 128, packed) and 6.2e-6 on c (LSTM H = 128, T = 40, |c| up to 24; 7.0e-7 on the rows of at most six steps)"""
    worst_y = worst_c = 0.0
    for i, r in enumerate(ROWS):
        op, want = reference(i, "exact", CUS)
        for p, (y, h, c) in zip(op["pool"], want):
            if not p["length"]:
                continue
            fy, fh, fc = float64_run(r["kind"], op, p)
            worst_y = max(worst_y, float(np.abs(y - fy).max()), float(np.abs(h - fh).max()))
            if c is not None:
                worst_c = max(worst_c, float(np.abs(c - fc).max()))
    print("oracle against float64: y %.3e, c %.3e" % (worst_y, worst_c))
    assert worst_y <= Y_BOUND and worst_c <= C_BOUND, (worst_y, worst_c)


def fma32(a, b, c):
    """one fused multiply-add on f32 arrays: the product is exact in float64"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def find_row(kind, entry, H, why=""):
    return next(r for r in ROWS if (r["kind"], r["entry"], r["H"]) == (kind, entry, H) and why in r["why"])


def test_acceptance_rejects_emulated_wrong_kernels(orc):
    """each variant is the oracle on altered operands (no device emulator): it differs from the reference in at least one bit on the
    inputs the GPU part uses, and the acceptance the GPU part applies rejects it"""
    seen = set()

    def told(name, want, wrong, verdict):
        assert any(accept_bits(a, b) != "" for a, b in zip(wrong, want) if b is not None), "%s: the variant gives the reference's bits" % name
        assert verdict != "", "%s: the acceptance lets the variant pass" % name
        seen.add(name)

    for kind in ("lstm", "gru"):
        for H in (8, 20, 128):
            r = find_row(kind, "single", H)
            op, want = reference(ROWS.index(r), "exact", CUS)
            p, G = op["pool"][0], ng_of(kind) * H
            assert accept_rnn(H, want[0], want[0], "exact") == ""
            # the two bias vectors added first: in the LSTM body ((wc + rc) + bw) + br becomes (wc + rc) + (bw + br)
            b = op["b"].reshape(2, G)
            pre = np.concatenate([b[0] + b[1], np.zeros(G, np.float32)]).reshape(1, 2 * G)
            wrong = oracle_run(orc, kind, op, p, b=pre)
            if kind == "lstm":
                body = H & ~7
                assert accept_bits(wrong[0][:, :body], want[0][0][:, :body]) != "", "the bias family does not tell the association"
                told("bias_pre_added.%s.%d" % (kind, H), want[0], wrong, accept_rnn(H, wrong, want[0], "exact"))
            # the routing shifted by one k
            wrong = oracle_run(orc, kind, op, p, r=np.ascontiguousarray(np.roll(op["r"], 1, axis=2)))
            told("routing_shifted.%s.%d" % (kind, H), want[0], wrong, accept_rnn(H, wrong, want[0], "exact"))
        # the initial h of two segments exchanged
        r = find_row(kind, "packed", 20, "ns = 3")
        op, want = reference(ROWS.index(r), "exact", CUS)
        a, bq = [i for i, p in enumerate(op["pool"]) if p["length"]][:2]
        wrong = oracle_run(orc, kind, op, op["pool"][a], h0=op["pool"][bq]["h0"])
        told("h0_exchanged." + kind, want[a], wrong, accept_rnn(20, wrong, want[a], "exact"))
        # body and tail exchanged: hidden elements 0..3 and 16..19 of H = 20 trade places (the same pre-activations on step 0), so the
        # oracle runs the polynomial on the tail's and libm on the body's
        r = find_row(kind, "single", 20)
        op, want = reference(ROWS.index(r), "exact", CUS)
        p, H, NG = op["pool"][0], 20, ng_of(kind)
        perm = np.arange(H)
        perm[:4], perm[16:] = np.arange(16, 20), np.arange(4)
        rows = (np.arange(NG)[:, None] * H + perm[None, :]).reshape(-1)
        op2 = dict(op, w=np.ascontiguousarray(op["w"][:, rows]), r=np.ascontiguousarray(op["r"][:, rows][:, :, perm]),
                   b=np.ascontiguousarray(op["b"].reshape(2, NG * H)[:, rows].reshape(1, -1)))
        p2 = dict(p, h0=p["h0"][perm], c0=None if p["c0"] is None else p["c0"][perm])
        swapped = [None if v is None else v[..., np.argsort(perm)] for v in oracle_run(orc, kind, op2, p2)]
        for name, sl in (("tail_takes_the_body_value", slice(16, 20)), ("body_takes_the_tail_value", slice(0, 4))):
            wrong = [None if v is None else v.copy() for v in want[0]]
            for dst, src in zip(wrong, swapped):
                if dst is not None:
                    dst[..., sl] = src[..., sl]
            wrong[1] = wrong[0][-1].copy()
            told("%s.%s" % (name, kind), want[0], wrong, accept_rnn(H, wrong, want[0], "exact"))
        rel = np.abs(swapped[0][0, 16:].astype(np.float64) - want[0][0][0, 16:]) / np.abs(want[0][0][0, 16:])
        assert np.all(rel >= 0.99 * SEPARATION), rel   # the separation the probe step relies on
    # c_t = fg * c + ig * cg in two roundings where the reference fuses, one step from the oracle's own pieces: ig * cg is the c_t of a
    # zero cell state, fg the oracle's sigmoid of the forget gate's pre-activation
    r = find_row("lstm", "single", 128)
    op, want = reference(ROWS.index(r), "exact", CUS)
    p, H = op["pool"][0], 128
    one = dict(p, x=p["x"][:1])
    y1, h1, c1 = oracle_run(orc, "lstm", op, one)
    _, _, prod = oracle_run(orc, "lstm", op, dict(one, c0=np.zeros(H, np.float32)))
    b = op["b"].reshape(2, 4, H)
    wc, rc = (op["w"][0] @ one["x"][0]).reshape(4, H), (op["r"][0] @ p["h0"]).reshape(4, H)
    gate = ((wc + rc) + b[0]) + b[1]
    fg, og = orc.unary("sigmoid", gate[2]), orc.unary("sigmoid", gate[1])
    assert accept_bits(fma32(fg, p["c0"], prod), c1) == "" and accept_bits(og * orc.unary("tanh", c1), h1) == ""   # the pieces are the oracle's
    c_wrong = fg * p["c0"] + prod
    h_wrong = og * orc.unary("tanh", c_wrong)
    told("c_unfused", (y1, h1, c1), (h_wrong[None], h_wrong, c_wrong), accept_rnn(H, (h_wrong[None], h_wrong, c_wrong), (y1, h1, c1), "exact"))
    assert len(seen) == 3 + 6 + 2 + 4 + 1, sorted(seen)
    # the class acceptance: a NaN that the reference does not have, and one it has
    y = want[0][0]
    bad = y.copy()
    bad[2, 5] = np.nan
    assert accept_classes((bad, bad[-1], want[0][2]), want[0], H, 2) != "" and accept_classes(want[0], want[0], H, 2) == ""


# ================================================================================================================ GPU tests
def device_single(K, ctx, kind, op, p, dev):
    """the single call on one segment -> (y [T, H], h [H], c [H] or None)"""
    H = op["r"].shape[2]
    x3 = p["x"].reshape(len(p["x"]), 1, p["x"].shape[1])
    hh = None if p["h0"] is None else p["h0"].reshape(1, 1, H)
    if kind == "lstm":
        y, h, c = K.lstm(x3, dev["w"], dev["r"], dev["b"], None, hh, None if p["c0"] is None else p["c0"].reshape(1, 1, H), ctx=ctx)
        return y.numpy().reshape(-1, H).copy(), h.numpy().reshape(H).copy(), c.numpy().reshape(H).copy()
    y, h = K.gru(x3, dev["w"], dev["r"], dev["b"], hh, False, ctx=ctx)
    return y.numpy().reshape(-1, H).copy(), h.numpy().reshape(H).copy(), None


def device_packed(K, ctx, kind, op, dev, x=None):
    """the packed call -> (y [R, H], h [count, H], c [count, H] or None, info)"""
    H = op["r"].shape[2]
    off = np.concatenate([[0], np.cumsum(op["lengths"])]).astype(np.int64)
    given = op["pool"][0]["h0"] is not None
    h0 = np.stack([op["pool"][m]["h0"] for m in op["member"]])[None] if given else None
    info = {}
    x = op["x"] if x is None else x
    if kind == "lstm":
        c0 = np.stack([op["pool"][m]["c0"] for m in op["member"]])[None] if given else None
        y, h, c = K.lstm_segments(x, off, dev["w"], dev["r"], dev["b"], h0, c0, info=info, ctx=ctx)
        return y.numpy().copy(), h.numpy()[0].copy(), c.numpy()[0].copy(), info
    y, h = K.gru_segments(x, off, dev["w"], dev["r"], dev["b"], h0, info=info, ctx=ctx)
    return y.numpy().copy(), h.numpy()[0].copy(), None, info


def on_device(ctx, op):
    from lele_amd.tensor import TensorView
    return {k: op[k] if op[k] is None or not op[k].size else TensorView(ctx.buf().upload(op[k])) for k in ("w", "r", "b")}   # (I = 0: W is empty)


def check_row(K, ctx, r, family, cus):
    kind, H = r["kind"], r["H"]
    op, want = reference(ROWS.index(r), family, cus)
    dev = on_device(ctx, op)
    if r["entry"] == "single":
        got = device_single(K, ctx, kind, op, op["pool"][0], dev)
        assert K.last_route(ctx) == route_of(r, cus), (r["id"], family)
        msg = accept_rnn(H, got, want[0], family)
        assert msg == "", (r["id"], family, msg)
        if r["lengths"] == 0 and r["given"]:   # no step: the state comes back exactly
            assert accept_bits(got[1], op["pool"][0]["h0"]) == "" and (kind == "gru" or accept_bits(got[2], op["pool"][0]["c0"]) == "")
        return
    y, h, c, info = device_packed(K, ctx, kind, op, dev)
    assert K.last_route(ctx) == route_of(r, cus) == r["route"], (r["id"], family)
    ns = ns_of(kind, H, len(op["lengths"]), cus)
    assert info == {"form": 0 if not r["route"] else 1 if "reg" in r["route"] else 2, "streams_per_workgroup": ns}, info
    assert y.shape == (sum(op["lengths"]), H) and h.shape == (len(op["lengths"]), H)
    off = np.concatenate([[0], np.cumsum(op["lengths"])])
    alone = {}
    for i, m in enumerate(op["member"]):
        p = op["pool"][m]
        got = (y[off[i]:off[i + 1]], h[i], None if c is None else c[i])
        if not p["length"]:   # an empty segment hands its state on exactly (zeros without one)
            zero = np.zeros(H, np.float32)
            assert accept_bits(got[1], zero if p["h0"] is None else p["h0"]) == "", (r["id"], family, i)
            assert c is None or accept_bits(got[2], zero if p["c0"] is None else p["c0"]) == "", (r["id"], family, i)
            continue
        msg = accept_rnn(H, got, want[m], family)
        assert msg == "", (r["id"], family, "segment %d" % i, msg)
        if family != "saturate":   # every segment bit for bit the single call on it alone
            if m not in alone:
                alone[m] = device_single(K, ctx, kind, op, p, dev)
            for name, a, b in zip("yhc", got, alone[m]):
                assert a is None or accept_bits(a, b) == "", (r["id"], family, "segment %d against the single call" % i, name, accept_bits(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_route_and_values(ctx, r):
    from lele_amd import kernels as K
    cus = K.num_cus(ctx)
    for family in ("exact", "random", "saturate"):
        if family == "saturate" and not r["given"]:
            continue   # no bias to saturate with
        check_row(K, ctx, r, family, cus)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("r", SPECIAL_ROWS, ids=[r["id"] for r in SPECIAL_ROWS])
def test_a_nan_or_an_infinity_in_one_x_row(ctx, orc, r, value):
    """the special value enters one x row in the middle of the longest segment: classes as the oracle's from that step on, the steps
    before it and every other segment untouched"""
    from lele_amd import kernels as K
    special_case(K, ctx, orc, r, value, K.num_cus(ctx))


def special_case(K, ctx, orc, r, value, cus):
    kind, H = r["kind"], r["H"]
    op, want = reference(ROWS.index(r), "exact", cus)
    dev = on_device(ctx, op)
    m = int(np.argmax([p["length"] for p in op["pool"]]))
    p = op["pool"][m]
    t0 = p["length"] // 2
    xs = p["x"].copy()
    xs[t0, min(3, r["I"] - 1)] = value
    hit = dict(p, x=xs)
    ref = oracle_run(orc, kind, op, hit)
    if r["entry"] == "single":
        msg = accept_classes(device_single(K, ctx, kind, op, hit, dev), ref, H, t0)
        assert msg == "", (r["id"], msg)
        return
    off = np.concatenate([[0], np.cumsum(op["lengths"])])
    i = int(np.nonzero(op["member"] == m)[0][1])   # the second segment drawn from that pool member
    x = op["x"].copy()
    x[off[i]:off[i + 1]] = xs
    y, h, c, _ = device_packed(K, ctx, kind, op, dev, x=x)
    msg = accept_classes((y[off[i]:off[i + 1]], h[i], None if c is None else c[i]), ref, H, t0)
    assert msg == "", (r["id"], msg)
    for j, mj in enumerate(op["member"]):   # its neighbours see nothing of it
        if j != i and op["pool"][mj]["length"]:
            msg = accept_rnn(H, (y[off[j]:off[j + 1]], h[j], None if c is None else c[j]), want[mj], "exact")
            assert msg == "", (r["id"], "segment %d" % j, msg)
