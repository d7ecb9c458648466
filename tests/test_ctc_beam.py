"""CTC prefix beam search on the device (lele_hip_ctc_beam_search_segments, ctc_beam_seg_kernel of csrc/app.hip) against the host
function it moves to the device, lele_amd.apps.ctc_prefix_beam_search, which stays the reference exactly as it stands.

Inputs are candidate tables [T, k] as the k-best head gives them: the f32 log-soft-max of seeded logits, the k greatest of a frame in
stable order, ids distinct per frame, -1 / -inf where the vocabulary has fewer than k labels.  Families: `small_vocab` (6 labels, the
blank favoured: repeats, merges and re-entries nearly every frame), `wide` (ids up to 25054), `peaky` (blank near 0 on most frames),
`repeats` (runs of one label with and without a blank between), `padded` (slots dropped to -1 / -inf), `padded_dead` (the same with
one frame whose every slot is -1: the host's beam dies there and the result is no hypothesis at all), `twins` (frame 0 holds labels 3
and 5 with bit-equal scores, the greater id in the earlier slot, no later frame uses either: every prefix that starts with one has a
twin with a bit-identical total, which only the tuple order separates).

The margin condition (checked on the CPU, for every case): `host_margin` below restates the host search and looks at every pair of
totals whose order decides anything -- the beam-th and (beam + 1)-th entry of each frame, and neighbours in the final list up to the
nbest-th and its successor.  Each such pair is either exactly equal -- and then the two are `twins` partners, or both totals are -inf,
which any arithmetic reproduces -- or at least 1e-9 * max(1, |total|) apart, four orders of magnitude above the arithmetic bar.

Bars.  Sequences, lengths and counts equal the host's exactly.  Scores: |f32 score - host float64| <= 2^-24 |s| + 16 T 2^-53 max(1, |s|):
the f32 rounding of the output, then at most four roundings and two libm calls of at most 2 ulp a frame on values no larger than |s|,
host and device together.  The GPU tests print the worst difference per case; on the MI355X: 1.16e-5 for `wide` at
171 frames, k = 8, beam 8 (score -377: the f32 rounding alone allows 2.2e-5), 1.07e-5 for `peaky` at 900 frames (score -259), at most
3.7e-6 for every other case.

The CPU half also runs a plain-Python emulation of the kernel's algorithm (slots, trie nodes, merge detection by content, ranking by
counting, the tie walk) with numpy's float64 logaddexp: it must equal the host function on every case, scores bit for bit, and each of
seven deliberately wrong variants of it must differ on at least one case -- which shows that the inputs can tell."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lele_amd.apps import ctc_prefix_beam_search  # noqa: E402

NINF = -np.inf
VOCAB_WIDE = 25055
MARGIN = 1e-9
TWIN_A, TWIN_B = 3, 5


# ---------------------------------------------------------------------------------------------------- inputs
def log_softmax32(x):
    x = np.asarray(x, np.float32)
    m = x.max(axis=-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32))).astype(np.float32)


def topk_table(logits, k, names=None):
    """the k-best head's output for these logits: (ids int32 [T, k], logprob f32 [T, k]), stable top-k, -1 / -inf past the vocabulary"""
    lsm = log_softmax32(logits)
    t, v = lsm.shape
    kk = min(k, v)
    order = np.argsort(-lsm, axis=1, kind="stable")[:, :kk]
    ids = order if names is None else np.asarray(names)[order]
    ids = np.pad(ids.astype(np.int32), [(0, 0), (0, k - kk)], constant_values=-1)
    lp = np.pad(np.take_along_axis(lsm, order, axis=1), [(0, 0), (0, k - kk)], constant_values=NINF).astype(np.float32)
    return ids, lp


def make(family, t, k, seed):
    rng = np.random.default_rng([seed, t, k, sum(map(ord, family))])
    if family in ("small_vocab", "padded", "padded_dead"):
        lg = rng.normal(0.0, 1.5, (t, 6))
        lg[:, 0] += 1.5
        ids, lp = topk_table(lg, k)
        if family != "small_vocab":
            for f in range(t):
                if k > 1 and rng.uniform() < 0.4:
                    drop = int(rng.integers(1, k))
                    ids[f, k - drop:] = -1
                    lp[f, k - drop:] = NINF
            if family == "padded_dead":
                ids[t // 2] = -1
                lp[t // 2] = NINF
        return ids, lp
    if family == "wide":
        lg = rng.normal(0.0, 3.0, (t, VOCAB_WIDE)).astype(np.float32)
        lg[:, 0] += np.where(rng.uniform(size=t) < 0.5, 9.0, 0.0).astype(np.float32)
        lg[:, VOCAB_WIDE - 1] += np.where(rng.uniform(size=t) < 0.3, 12.0, 0.0).astype(np.float32)
        return topk_table(lg, k)
    if family == "peaky":
        lg = rng.normal(0.0, 1.0, (t, 40))
        lg[:, 0] += np.where(rng.uniform(size=t) < 0.85, 14.0, 0.0)
        return topk_table(lg, k)
    if family == "repeats":
        pat = []
        while len(pat) < t:
            pat += [int(rng.integers(1, 4))] * int(rng.integers(1, 4))
            if rng.uniform() < 0.5:
                pat += [0] * int(rng.integers(1, 3))
        lg = rng.normal(0.0, 0.5, (t, 8))
        lg[np.arange(t), pat[:t]] += 4.0
        return topk_table(lg, k)
    if family == "twins":
        assert t >= 1 and k >= 2
        rest = [0, 1, 2, 4, 6, 7]
        ids, lp = topk_table(rng.normal(0.0, 1.5, (t, 6)), k, rest)
        lg0 = np.minimum(rng.normal(0.0, 1.0, 8), 2.0)
        lg0[TWIN_A] = lg0[TWIN_B] = 3.0
        i0, l0 = topk_table(lg0[None], k)
        assert list(i0[0, :2]) == [TWIN_A, TWIN_B] and l0[0, 0] == l0[0, 1]
        i0[0, :2] = [TWIN_B, TWIN_A]        # the head's tie rule: the greater column first
        ids[0], lp[0] = i0[0], l0[0]
        return ids, lp
    raise KeyError(family)


# (family, T, k, beam, nbest): T in {0, 1, 2, 5, 37, 171}, k in {1, 3, 4, 8}, beam in {1, 2, 4, 8} and 3 for twins, nbest in {1, 3, beam}
CASES = [
    ("small_vocab", 0, 4, 4, 1), ("small_vocab", 1, 4, 4, 3), ("small_vocab", 2, 3, 2, 2), ("small_vocab", 5, 4, 4, 4),
    ("small_vocab", 37, 4, 4, 3), ("small_vocab", 37, 8, 8, 8), ("small_vocab", 37, 1, 1, 1), ("small_vocab", 37, 3, 2, 1),
    ("small_vocab", 171, 4, 8, 3), ("small_vocab", 171, 3, 4, 4),
    ("wide", 5, 8, 8, 8), ("wide", 37, 4, 4, 1), ("wide", 37, 3, 4, 3), ("wide", 171, 8, 8, 8),
    ("peaky", 37, 4, 4, 3), ("peaky", 171, 4, 4, 1), ("peaky", 37, 8, 2, 2),
    ("repeats", 37, 3, 4, 4), ("repeats", 37, 4, 8, 3), ("repeats", 171, 4, 4, 3),
    ("padded", 37, 4, 4, 3), ("padded", 5, 8, 2, 2), ("padded", 37, 3, 8, 8), ("padded_dead", 37, 4, 4, 3),
    ("twins", 37, 4, 1, 1), ("twins", 37, 4, 3, 3), ("twins", 5, 4, 3, 3), ("twins", 2, 3, 1, 1), ("twins", 37, 8, 8, 8),
]
# the kernel keeps its prefix trie in LDS while (1 + beam * frames) * 8 bytes <= 56 KiB, else in global memory: one segment just under
# that threshold (7161 nodes), one just over it (7201)
LONG = [("peaky", 895, 4, 8, 1), ("peaky", 900, 4, 8, 3)]
SEED = 1
PACKED_LENGTHS = (0, 3, 4, 5, 40, 9, 17, 1)
PACKED = ("small_vocab", 4, 4, 3)   # family, k, beam, nbest

_tables, _refs = {}, {}


def table(family, t, k):
    key = (family, t, k)
    if key not in _tables:
        ids, lp = make(family, t, k, SEED)
        ids.setflags(write=False)
        lp.setflags(write=False)
        _tables[key] = (ids, lp)
    return _tables[key]


def reference(case):
    """the host function's answer, computed once per case"""
    if case not in _refs:
        family, t, k, beam, nbest = case
        ids, lp = table(family, t, k)
        _refs[case] = ctc_prefix_beam_search(ids, lp, 0, beam, nbest)
    return _refs[case]


def packed_table():
    family, k = PACKED[0], PACKED[1]
    parts = [make(family, n, k, 100 + i) for i, n in enumerate(PACKED_LENGTHS)]
    off = np.concatenate([[0], np.cumsum(PACKED_LENGTHS)]).astype(np.int64)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), off


def packed_reference(ids, lp, off, skip_rows, beam, nbest):
    return [ctc_prefix_beam_search(ids[min(off[i] + skip_rows, off[i + 1]):off[i + 1]], lp[min(off[i] + skip_rows, off[i + 1]):off[i + 1]],
                                   0, beam, nbest) for i in range(len(off) - 1)]


def twin_partner(p):
    if p and p[0] in (TWIN_A, TWIN_B):
        return (TWIN_A + TWIN_B - p[0],) + tuple(p[1:])
    return None


# ---------------------------------------------------------------------------------------------------- the margin condition
def host_margin(ids, lp, blank, beam, nbest):
    """apps.ctc_prefix_beam_search restated with a watch on every comparison that decides something -> (its result, the smallest relative
    gap seen among those comparisons, the offending pairs: exact ties that are neither twins partners nor two -inf, and gaps below MARGIN,
    the number of exact ties between twins partners)"""
    ids, lp = np.asarray(ids, np.int64), np.asarray(lp, np.float64)
    beams = {(): (0.0, NINF)}
    total = lambda s: np.logaddexp(s[0], s[1])  # noqa: E731
    smallest, bad, twin_ties = [np.inf], [], []

    def watch(a, b, where):
        (pa, sa), (pb, sb) = a, b
        ta, tb = float(total(sa)), float(total(sb))
        if ta == tb:
            if ta != NINF and twin_partner(pa) == pb:
                twin_ties.append(where)
            elif ta != NINF:
                bad.append((where, pa, pb, ta, tb))
            return
        gap = abs(ta - tb) / max(1.0, abs(ta)) if np.isfinite(ta) and np.isfinite(tb) else np.inf
        smallest[0] = min(smallest[0], gap)
        if gap < MARGIN:
            bad.append((where, pa, pb, ta, tb))

    for t in range(ids.shape[0]):
        nxt = {}

        def add(prefix, which, v):
            s = nxt.setdefault(prefix, [NINF, NINF])
            s[which] = np.logaddexp(s[which], v)

        for prefix, (pb, pnb) in beams.items():
            for c, v in zip(ids[t].tolist(), lp[t].tolist()):
                if c < 0:
                    continue
                if c == blank:
                    add(prefix, 0, np.logaddexp(pb, pnb) + v)
                elif prefix and prefix[-1] == c:
                    add(prefix, 1, pnb + v)
                    add(prefix + (c,), 1, pb + v)
                else:
                    add(prefix + (c,), 1, np.logaddexp(pb, pnb) + v)
        ranked = sorted(nxt.items(), key=lambda kv: (-total(kv[1]), kv[0]))
        if len(ranked) > beam:
            watch(ranked[beam - 1], ranked[beam], "frame %d" % t)
        beams = {p: (s[0], s[1]) for p, s in ranked[:beam]}
    ranked = sorted(beams.items(), key=lambda kv: (-total(kv[1]), kv[0]))
    for i in range(min(nbest, len(ranked) - 1)):
        watch(ranked[i], ranked[i + 1], "final %d" % i)
    return [(p, float(total(s))) for p, s in ranked[:nbest]], smallest[0], bad, len(twin_ties)


# ---------------------------------------------------------------------------------------------------- the kernel's algorithm, emulated
BUGS = ("repeat_from_total", "duplicate_entry", "tie_by_slot", "prune_by_pnb", "minus_one_counted", "prompt_not_skipped", "next_row_read")


def emulate_one(ids, lp, blank, beam, nbest, bug=None):
    """ctc_beam_seg_kernel's steps for one segment, lane by lane, in float64 with numpy's logaddexp -> the host function's list.  Slots
    hold (node, parent, last, depth, pb, pnb, tot); the trie holds (parent, label) per node, node 0 the empty prefix; frame t's new
    prefixes are nodes 1 + t * beam + rank."""
    ids, lp = np.asarray(ids, np.int64), np.asarray(lp, np.float64)
    frames, k = ids.shape
    trie = {0: (0, -1)}
    la = np.logaddexp

    def same_prefix(a, b, d):
        for _ in range(d):
            if a == b:
                break
            (pa, ca), (pb_, cb) = trie[a], trie[b]
            if ca != cb:
                return False
            a, b = pa, pb_
        return a == b

    def less(x, y, lim, ix, iy):   # (rest node, last label, length) each; x before y in tuple order?  Equal prefixes: by entry index
        (ra, ca, na), (rb, cb, nb_) = x, y
        if na == 0 or nb_ == 0:
            return na < nb_ if na != nb_ else ix < iy
        shorter, same_length = na < nb_, na == nb_
        while na > nb_:
            ra, ca = trie[ra]
            na -= 1
        while nb_ > na:
            rb, cb = trie[rb]
            nb_ -= 1
        res = 0
        for _ in range(lim):
            if ca != cb:
                res = -1 if ca < cb else 1
            if ra == rb:
                break
            (ra, ca), (rb, cb) = trie[ra], trie[rb]
        return res < 0 if res else (ix < iy if same_length else shorter)

    def no_nan(v):                 # a NaN total would compare false with everything; the kernel ranks it as -inf
        return NINF if v != v else v

    slots = [dict(node=0, parent=0, last=-1, depth=0, pb=0.0, pnb=NINF, tot=0.0)]
    for t in range(frames):
        cand = [(int(ids[t, j]), float(lp[t, j])) for j in range(k)]
        valid = [c >= 0 or bug == "minus_one_counted" for c, _ in cand]
        jb = next((j for j in range(k) if valid[j] and cand[j][0] == blank), None)
        ext_v, rep_v, entries = {}, {}, []   # an entry: (lane index, key, handle, payload)
        for s, S in enumerate(slots):
            for j, (c, v) in enumerate(cand):
                if not valid[j] or c == blank:
                    continue
                rep = c == S["last"]
                e = no_nan((S["pb"] if rep and bug != "repeat_from_total" else S["tot"]) + v)
                fresh = True
                if bug != "duplicate_entry":
                    for q, Q in enumerate(slots):
                        if Q["depth"] == S["depth"] + 1 and Q["last"] == c and same_prefix(Q["parent"], S["node"], S["depth"]):
                            ext_v[q] = e
                            fresh = False
                if rep:
                    rep_v[s] = S["pnb"] + v
                if fresh:
                    entries.append((s * 8 + j, e, (S["node"], c, S["depth"] + 1),
                                    dict(node=None, parent=S["node"], last=c, depth=S["depth"] + 1, pb=NINF, pnb=e, tot=e)))
        for q, Q in enumerate(slots):
            if jb is None and q not in rep_v and q not in ext_v:
                continue
            npb = no_nan(Q["tot"] + cand[jb][1] if jb is not None else NINF)
            npnb = no_nan(la(rep_v.get(q, NINF), ext_v.get(q, NINF)))
            tot = no_nan(la(npb, npnb))
            entries.append((64 + q, npnb if bug == "prune_by_pnb" else tot, (Q["parent"], Q["last"], Q["depth"]),
                            dict(node=Q["node"], parent=Q["parent"], last=Q["last"], depth=Q["depth"], pb=npb, pnb=npnb, tot=tot)))
        nxt = [None] * min(beam, len(entries))
        for m, key, h, new in entries:
            rank = 0
            for m2, key2, h2, _ in entries:
                if m2 == m:
                    continue
                if key2 > key or (key2 == key and (m2 < m if bug == "tie_by_slot" else less(h2, h, t + 2, m2, m))):
                    rank += 1
            if rank < len(nxt):
                if new["node"] is None:
                    new["node"] = 1 + t * beam + rank
                    trie[new["node"]] = (new["parent"], new["last"])
                nxt[rank] = new
        # (total, tuple order, entry index) is a strict total order, so the ranks are a permutation and every slot is written -- also
        # for duplicate ids or NaN scores, where the result is unspecified; only `tie_by_slot` beside `duplicate_entry` could leave a hole
        assert bug is not None or None not in nxt, "a rank was taken twice"
        slots = [s for s in nxt if s is not None]
    out = []
    for S in slots[:nbest]:
        seq, rest, lab = [], S["parent"], S["last"]
        for _ in range(S["depth"]):
            seq.append(lab)
            rest, lab = trie[rest]
        out.append((tuple(reversed(seq)), float(S["tot"])))
    return out


def emulate_segments(ids, lp, off, skip_rows, blank, beam, nbest, bug=None):
    res = []
    for i in range(len(off) - 1):
        r0 = off[i] if bug == "prompt_not_skipped" else min(off[i] + skip_rows, off[i + 1])
        r1 = min(off[i + 1] + 1, len(ids)) if bug == "next_row_read" else off[i + 1]
        res.append(emulate_one(ids[r0:r1], lp[r0:r1], blank, beam, nbest, bug))
    return res


# ---------------------------------------------------------------------------------------------------- CPU tests
NAME = "lele_hip_ctc_beam_search_segments"


def test_the_entry_point_is_declared_exported_and_wrapped():
    from lele_amd import _lib
    from lele_amd import apps
    from lele_amd import kernels as K
    assert NAME in _lib.exported_symbols() and hasattr(_lib.lib(), NAME)
    hdr = open(os.path.join(ROOT, "include", "lele_hip.h")).read()
    hpp = open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "lele-hip", "src", "ffi.rs")).read()
    kpy = open(os.path.join(ROOT, "lele_amd", "kernels.py")).read()
    assert "int " + NAME + "(" in hdr and NAME + "(" in hpp and "pub fn %s(" % NAME in ffi
    assert "def ctc_beam_search_segments(" in kpy and "lib()." + NAME + "(" in kpy
    assert callable(K.ctc_beam_search_segments) and callable(apps.beam_results)
    from sensevoice_graph import Encoder
    assert callable(Encoder.beam_segments) and callable(Encoder.beam)


def test_beam_results_gives_the_host_functions_format():
    from lele_amd.apps import beam_results
    tokens = np.array([[[7, 9, -1], [7, -1, -1]], [[-1, -1, -1], [-1, -1, -1]]], np.int32)
    lengths = np.array([[2, 1], [0, 0]], np.int32)
    scores = np.array([[-0.5, -1.25], [0.0, NINF]], np.float32)
    assert beam_results(tokens, lengths, scores, np.array([2, 1], np.int32)) == [[((7, 9), -0.5), ((7,), -1.25)], [((), 0.0)]]
    assert beam_results(tokens, lengths, scores, np.array([0, 0], np.int32)) == [[], []]
    with pytest.raises(ValueError):
        beam_results(tokens, lengths[:, :1], scores, np.array([2, 1]))


def _build_demo():
    libdir = os.path.join(ROOT, "lele_amd")
    src = os.path.join(ROOT, "tests", "host_cpp", "ctc_beam_demo.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "ctc_beam_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                           src, "-L", libdir, "-llele_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_host_cpp_ctc_beam_demo_builds():
    r = subprocess.run([_build_demo(), "probe"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("PROBE"), r.stdout + r.stderr


def test_the_tables_are_what_the_head_gives():
    sizes = {"t": set(), "k": set(), "beam": set(), "nbest": set()}
    for family, t, k, beam, nbest in CASES + LONG:
        ids, lp = table(family, t, k)
        assert ids.dtype == np.int32 and lp.dtype == np.float32 and ids.shape == lp.shape == (t, k)
        assert 1 <= nbest <= beam <= 8
        for f in range(t):
            real = ids[f][ids[f] >= 0]
            assert len(set(real.tolist())) == len(real)                      # distinct per frame
            assert np.isneginf(lp[f][ids[f] < 0]).all()
            assert (np.diff(lp[f][ids[f] >= 0]) <= 0).all()                  # best first
        if t <= 171:
            sizes["t"].add(t), sizes["k"].add(k), sizes["beam"].add(beam), sizes["nbest"].add(nbest if nbest in (1, 3) else "beam")
    assert sizes == {"t": {0, 1, 2, 5, 37, 171}, "k": {1, 3, 4, 8}, "beam": {1, 2, 3, 4, 8}, "nbest": {1, 3, "beam"}}   # beam 3: twins
    assert table("wide", 171, 8)[0].max() == VOCAB_WIDE - 1
    assert (table("padded_dead", 37, 4)[0][18] == -1).all() and (table("padded", 37, 4)[0] == -1).any()
    ids, lp = table("twins", 37, 4)
    assert list(ids[0, :2]) == [TWIN_B, TWIN_A] and lp[0, 0] == lp[0, 1] and not np.isin(ids[1:], (TWIN_A, TWIN_B)).any()
    assert reference(("padded_dead", 37, 4, 4, 3)) == []
    assert reference(("small_vocab", 0, 4, 4, 1)) == [((), 0.0)]


def test_the_margin_condition_holds_for_every_case():
    smallest = np.inf
    for case in CASES + LONG:
        family, t, k, beam, nbest = case
        got, gap, bad, _ = host_margin(*table(family, t, k), 0, beam, nbest)
        assert got == reference(case), case                                   # the restatement is the host function
        assert not bad, (case, bad[:3])
        smallest = min(smallest, gap)
    ids, lp, off = packed_table()
    for skip in (0, 4):
        for i in range(len(off) - 1):
            lo = min(off[i] + skip, off[i + 1])
            assert not host_margin(ids[lo:off[i + 1]], lp[lo:off[i + 1]], 0, PACKED[2], PACKED[3])[2], (skip, i)
    print("smallest deciding relative gap over the table: %.3g" % smallest)
    assert smallest >= MARGIN


def test_twins_ties_fall_on_the_beam_boundary():
    """at beam 1 and 3 the beam-th and (beam + 1)-th entries of some frame are twins partners with bit-equal totals"""
    for beam in (1, 3):
        assert host_margin(*table("twins", 37, 4), 0, beam, beam)[3] > 0, beam
        assert reference(("twins", 37, 4, beam, beam))[0][0][0] == TWIN_A    # of two equal twins the smaller tuple is first


def test_the_emulated_kernel_equals_the_host_function():
    for case in CASES + LONG:
        family, t, k, beam, nbest = case
        assert emulate_one(*table(family, t, k), 0, beam, nbest) == reference(case), case
    ids, lp, off = packed_table()
    for skip in (0, 4):
        assert emulate_segments(ids, lp, off, skip, 0, PACKED[2], PACKED[3]) == packed_reference(ids, lp, off, skip, PACKED[2], PACKED[3])


@pytest.mark.parametrize("bug", BUGS)
def test_an_emulated_wrong_kernel_is_told_apart(bug):
    if bug in ("prompt_not_skipped", "next_row_read"):
        ids, lp, off = packed_table()
        assert emulate_segments(ids, lp, off, 4, 0, PACKED[2], PACKED[3], bug) != packed_reference(ids, lp, off, 4, PACKED[2], PACKED[3])
        return
    for case in sorted(CASES, key=lambda c: c[1]):
        family, t, k, beam, nbest = case
        if emulate_one(*table(family, t, k), 0, beam, nbest, bug) != reference(case):
            return
    pytest.fail("no case of the table tells `%s` from the reference" % bug)


def malformed_tables():
    """inputs whose result is unspecified but must stay inside its buffers: duplicate ids with bit-equal scores (two entries of equal
    content and total), a frame of one id eight times, NaN and +inf scores"""
    rng = np.random.default_rng(77)
    ids, lp = (a.copy() for a in make("small_vocab", 12, 4, 9))
    ids[:, 1], lp[:, 1] = ids[:, 0], lp[:, 0]
    one = (np.array([[5, 5]], np.int32), np.array([[-0.7, -0.7]], np.float32))
    same = (np.full((6, 8), 3, np.int32), np.full((6, 8), -1.5, np.float32))
    nid, nlp = (a.copy() for a in make("small_vocab", 12, 4, 10))
    nlp[rng.uniform(size=nlp.shape) < 0.3] = np.nan
    nlp[3, 0], nlp[5, 1] = np.inf, -np.inf
    return [("twice", ids, lp), ("one_frame", *one), ("eight_times", *same), ("nan", nid, nlp), ("all_nan", nid, np.full_like(nlp, np.nan))]


def test_the_emulated_kernel_takes_every_rank_once_on_malformed_frames():
    """duplicate ids or NaN scores: the result is unspecified, but no slot of the next beam may stay unwritten (emulate_one asserts that
    the ranks are a permutation) and what comes out is well formed"""
    for name, ids, lp in malformed_tables():
        for beam, nbest in ((4, 2), (8, 8), (1, 1)):
            with np.errstate(invalid="ignore"):
                res = emulate_one(ids, lp, 0, beam, nbest)
            assert 1 <= len(res) <= nbest, name
            for seq, _ in res:
                assert len(seq) <= len(ids) and set(seq) <= set(ids.reshape(-1).tolist()), name
    assert len(emulate_one(np.array([[5, 5]]), np.array([[-0.7, -0.7]]), 0, 4, 4)) == 2      # two entries, two slots: no hole


# ---------------------------------------------------------------------------------------------------- GPU
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def search(ctx, ids, lp, off, **kw):
    from lele_amd import kernels as K
    out = K.ctc_beam_search_segments(np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lp, np.float32), off, ctx=ctx, **kw)
    assert tuple(out[1].shape) == tuple(out[2].shape) == tuple(out[0].shape)[:2] and tuple(out[3].shape) == tuple(out[0].shape)[:1]
    return tuple(o.numpy().copy() for o in out)


def check_against_host(got, want, frames, what):
    """got: the four device arrays; want: the host lists; frames: per segment.  Returns the worst |score - host|"""
    from lele_amd.apps import beam_results
    tokens, lengths, scores, counts = got
    assert tokens.dtype == lengths.dtype == counts.dtype == np.int32 and scores.dtype == np.float32
    lists = beam_results(tokens, lengths, scores, counts)
    worst = 0.0
    assert len(lists) == len(want), what
    for i, (g, w) in enumerate(zip(lists, want)):
        assert [p for p, _ in g] == [p for p, _ in w], (what, i)
        for (_, sg), (_, sw) in zip(g, w):
            if not np.isfinite(sw):
                assert sg == sw, (what, i)
                continue
            err = abs(sg - sw)
            worst = max(worst, err)
            assert err <= 2.0 ** -24 * abs(sw) + 16 * frames[i] * 2.0 ** -53 * max(1.0, abs(sw)), (what, i, sg, sw, err)
        n = len(w)
        assert (lengths[i, n:] == 0).all() and np.isneginf(scores[i, n:]).all() and (tokens[i, n:] == -1).all(), (what, i)
        for h in range(n):
            assert (tokens[i, h, lengths[i, h]:] == -1).all(), (what, i, h)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + LONG, ids=lambda c: "-".join(map(str, c)))
def test_every_case_against_the_host_function(ctx, case):
    family, t, k, beam, nbest = case
    ids, lp = table(family, t, k)
    got = search(ctx, ids, lp, [0, t], beam=beam, nbest=nbest)
    assert got[0].shape == (1, nbest, max(t, 1))
    worst = check_against_host(got, [reference(case)], [t], case)
    print("%s: max |score - host float64| = %.3g" % (case, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, 4])
def test_packed_equals_every_segment_alone(ctx, skip):
    ids, lp, off = packed_table()
    _, k, beam, nbest = PACKED
    got = search(ctx, ids, lp, off, beam=beam, nbest=nbest, skip_rows=skip)
    frames = [max(int(off[i + 1] - off[i]) - skip, 0) for i in range(len(off) - 1)]
    w = max(max(frames), 1)
    assert got[0].shape == (len(frames), nbest, w)
    worst = check_against_host(got, packed_reference(ids, lp, off, skip, beam, nbest), frames, "packed skip %d" % skip)
    print("packed skip %d: max |score - host float64| = %.3g" % (skip, worst))
    for i in range(len(frames)):
        seg = slice(off[i], off[i + 1])
        one = search(ctx, ids[seg], lp[seg], [0, off[i + 1] - off[i]], beam=beam, nbest=nbest, skip_rows=skip, width=w)
        assert np.array_equal(one[0][0], got[0][i]) and np.array_equal(one[1][0], got[1][i]), i
        assert np.array_equal(bits(one[2][0]), bits(got[2][i])) and one[3][0] == got[3][i], i
    dense = search(ctx, np.tile(ids[off[4]:off[5]], (3, 1)), np.tile(lp[off[4]:off[5]], (3, 1)), np.arange(4) * 40, beam=beam, nbest=nbest)
    for b in range(3):                                                        # a dense [3, 40, k] batch is off[i] = i * 40
        assert all(np.array_equal(bits(dense[j][b]) if j == 2 else dense[j][b], bits(dense[j][0]) if j == 2 else dense[j][0]) for j in range(4))


@pytest.mark.gpu
def test_empty_batch_and_empty_segments(ctx):
    none = search(ctx, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), [0], beam=4, nbest=2)
    assert none[0].shape == (0, 2, 1) and none[1].shape == none[2].shape == (0, 2) and none[3].shape == (0,)
    hollow = search(ctx, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), [0, 0, 0], beam=4, nbest=2)
    assert hollow[0].shape == (2, 2, 1) and (hollow[0] == -1).all() and list(hollow[3]) == [1, 1]
    assert np.array_equal(hollow[1], np.zeros((2, 2), np.int32))
    assert np.array_equal(bits(hollow[2]), bits(np.array([[0.0, NINF], [0.0, NINF]], np.float32)))  # +0.0, not -0.0
    ids, lp = table("small_vocab", 5, 4)
    short = search(ctx, ids, lp, [0, 2, 5], beam=4, nbest=2, skip_rows=3)     # 0 frames (2 rows <= 3), 0 frames (3 rows <= 3)
    assert list(short[3]) == [1, 1] and (short[1] == 0).all() and short[0].shape == (2, 2, 1)


@pytest.mark.gpu
def test_width_pads_and_a_width_too_small_is_refused(ctx):
    from lele_amd import _lib
    ids, lp, off = packed_table()
    _, k, beam, nbest = PACKED
    tight = search(ctx, ids, lp, off, beam=beam, nbest=nbest)
    wide = search(ctx, ids, lp, off, beam=beam, nbest=nbest, width=64)
    assert tight[0].shape[2] == 40 and wide[0].shape == (len(off) - 1, nbest, 64)
    assert np.array_equal(wide[0][:, :, :40], tight[0]) and (wide[0][:, :, 40:] == -1).all()
    assert all(np.array_equal(bits(wide[j]) if j == 2 else wide[j], bits(tight[j]) if j == 2 else tight[j]) for j in (1, 2, 3))
    exact = search(ctx, ids, lp, off, beam=beam, nbest=nbest, skip_rows=4, width=36)   # the longest segment has 40 - 4 frames
    assert exact[0].shape[2] == 36
    with pytest.raises(_lib.LeleError, match="segment 4"):
        search(ctx, ids, lp, off, beam=beam, nbest=nbest, skip_rows=4, width=35)


@pytest.mark.gpu
def test_bad_arguments_leave_the_outputs_alone(ctx):
    from lele_amd import _lib
    from lele_amd import kernels as K
    ids, lp, off = packed_table()
    ids, lp = np.ascontiguousarray(ids), np.ascontiguousarray(lp)
    outs = [ctx.buf() for _ in range(4)]
    marker = np.arange(500, 620, dtype=np.int32)
    for b in outs:
        b.upload(marker)
    before = _lib.lib().lele_hip_buf_bytes(outs[0]._h)
    names = ("out_tokens", "out_lengths", "out_scores", "out_counts")
    o = dict(zip(names, outs), ctx=ctx)
    run = K.ctc_beam_search_segments
    wide9 = (np.tile(ids[:, :1], (1, 9)), np.tile(lp[:, :1], (1, 9)))
    calls = [lambda: run(ids, lp, off, beam=0, nbest=1, **o), lambda: run(ids, lp, off, beam=9, nbest=1, **o),
             lambda: run(ids, lp, off, beam=4, nbest=5, **o), lambda: run(ids, lp, off, beam=4, nbest=0, **o),
             lambda: run(wide9[0], wide9[1], off, beam=4, nbest=1, **o),                                    # k = 9
             lambda: run(ids.astype(np.float32), lp, off, beam=4, nbest=1, **o),                            # wrong dtypes
             lambda: run(ids, lp.view(np.int32), off, beam=4, nbest=1, **o),
             lambda: run(ids, lp[:, :3].copy(), off, beam=4, nbest=1, **o),                                 # shapes that differ
             lambda: run(ids.reshape(-1), lp.reshape(-1), off * 4, beam=4, nbest=1, **o),                   # rank 1
             lambda: run(ids, lp, off, beam=4, nbest=1, skip_rows=-1, **o), lambda: run(ids, lp, off, blank=-1, beam=4, nbest=1, **o),
             lambda: run(ids, lp, off, beam=4, nbest=1, width=-1, **o),
             lambda: run(ids, lp, [0, 50, 40, off[-1]], beam=4, nbest=1, **o),                              # offsets that go back
             lambda: run(ids, lp, [0, 50, off[-1] - 1], beam=4, nbest=1, **o),                              # ... that do not end at R
             lambda: run(ids, lp, [1, 50, off[-1]], beam=4, nbest=1, **o)]                                  # ... that do not start at 0
    for a in range(4):                                                                                      # aliased outputs
        for b in range(a + 1, 4):
            alias = dict(o)
            alias[names[b]] = outs[a]
            calls.append(lambda alias=alias: run(ids, lp, off, beam=4, nbest=1, **alias))
    for i, call in enumerate(calls):
        with pytest.raises(_lib.LeleError):
            call()
        for b in outs:
            assert _lib.lib().lele_hip_buf_bytes(b._h) == before, i
            assert np.array_equal(b.to_numpy((120,), np.int32), marker), i


@pytest.mark.gpu
def test_graph_replay_reads_the_new_candidates(ctx):
    from lele_amd import kernels as K
    t, k, beam, nbest = 37, 4, 4, 3
    tabs = {n: make("small_vocab", 2 * t, k, s) for n, s in (("a", 31), ("b", 32), ("c", 33))}
    off = np.array([0, t, 2 * t], np.int64)
    eager = {n: search(ctx, i, l, off, beam=beam, nbest=nbest, skip_rows=4) for n, (i, l) in tabs.items()}
    assert not np.array_equal(eager["a"][0], eager["b"][0]) and not np.array_equal(eager["b"][0], eager["c"][0])
    bi, bl = ctx.buf(), ctx.buf()
    di, dl = bi.upload(tabs["a"][0]), bl.upload(tabs["a"][1])
    outs = [ctx.buf() for _ in range(4)]

    def run():
        K.ctc_beam_search_segments(di, dl, off, 0, beam, nbest, 4, 0, out_tokens=outs[0], out_lengths=outs[1], out_scores=outs[2],
                                   out_counts=outs[3], ctx=ctx)

    run()                                                     # one eager run of the same layout
    ctx.sync()
    ctx.graph_begin()
    run()
    graph = ctx.graph_end()
    w = t - 4
    for n in ("b", "c"):                                      # fresh candidates in the same buffers, stale bytes in the outputs
        bi.upload(tabs[n][0])
        bl.upload(tabs[n][1])
        for o in outs:
            o.upload(np.full(2 * nbest * w, -7, np.int32))
        graph.launch()
        want = eager[n]
        assert np.array_equal(outs[0].to_numpy((2, nbest, w), np.int32), want[0])
        assert np.array_equal(outs[1].to_numpy((2, nbest), np.int32), want[1])
        assert np.array_equal(outs[2].to_numpy((2, nbest), np.uint32), bits(want[2]))
        assert np.array_equal(outs[3].to_numpy((2,), np.int32), want[3])
    graph.close()


@pytest.mark.gpu
def test_malformed_frames_stay_inside_the_buffers(ctx):
    """duplicate ids, NaN and +inf scores: unspecified results, well-formed outputs -- counts within nbest, lengths within the frames,
    tokens from the frame's ids, then -1.  The order of entries is strict and total whatever comes in, so every slot of a beam is
    written before it is read (and both slot sets start as the empty prefix)."""
    for name, ids, lp in malformed_tables():
        t = len(ids)
        labels = set(ids.reshape(-1).tolist())
        for beam, nbest in ((4, 2), (8, 8), (1, 1)):
            tokens, lengths, scores, counts = search(ctx, np.tile(ids, (2, 1)), np.tile(lp, (2, 1)), [0, t, 2 * t], beam=beam, nbest=nbest)
            assert tokens.shape == (2, nbest, t) and ((1 <= counts) & (counts <= nbest)).all(), (name, beam)
            assert ((0 <= lengths) & (lengths <= t)).all(), (name, beam)
            for i in range(2):
                for h in range(nbest):
                    n = lengths[i, h]
                    assert (tokens[i, h, n:] == -1).all() and set(tokens[i, h, :n].tolist()) <= labels, (name, beam, i, h)
                    assert n == 0 or h < counts[i]
            assert np.array_equal(tokens[0], tokens[1]) and np.array_equal(lengths[0], lengths[1])   # deterministic


@pytest.mark.gpu
def test_global_trie_packed_and_captured(ctx):
    """Past 895 frames at beam 8 the trie leaves LDS for the context's scratch block, one stride of nodes per segment: two segments, the
    long one second, against the host and against each alone, then the same call captured and replayed on new candidates."""
    from lele_amd import kernels as K
    beam, nbest, k = 8, 3, 4
    tabs = {n: [make("peaky", 37, k, s), make("peaky", 900, k, s + 1)] for n, s in (("a", 41), ("b", 43))}
    off = np.array([0, 37, 937], np.int64)
    packed = {n: (np.concatenate([p[0] for p in v]), np.concatenate([p[1] for p in v])) for n, v in tabs.items()}
    eager = {}
    for n in ("b", "a"):
        for part in tabs[n]:
            assert not host_margin(part[0], part[1], 0, beam, nbest)[2]
        got = search(ctx, *packed[n], off, beam=beam, nbest=nbest)
        check_against_host(got, [ctc_prefix_beam_search(p[0], p[1], 0, beam, nbest) for p in tabs[n]], [37, 900], "global trie " + n)
        for i, part in enumerate(tabs[n]):
            one = search(ctx, part[0], part[1], [0, len(part[0])], beam=beam, nbest=nbest, width=900)
            assert np.array_equal(one[0][0], got[0][i]) and np.array_equal(bits(one[2][0]), bits(got[2][i])) and one[3][0] == got[3][i]
        eager[n] = got
    assert not np.array_equal(eager["a"][0], eager["b"][0])
    bi, bl = ctx.buf(), ctx.buf()
    di, dl = bi.upload(packed["a"][0]), bl.upload(packed["a"][1])
    outs = [ctx.buf() for _ in range(4)]

    def run():
        K.ctc_beam_search_segments(di, dl, off, 0, beam, nbest, 0, 0, out_tokens=outs[0], out_lengths=outs[1], out_scores=outs[2],
                                   out_counts=outs[3], ctx=ctx)

    run()                                                     # one eager run: the scratch block has its size
    ctx.sync()
    ctx.graph_begin()
    run()
    graph = ctx.graph_end()
    bi.upload(packed["b"][0])
    bl.upload(packed["b"][1])
    for o, n in zip(outs, (2 * nbest * 900, 2 * nbest, 2 * nbest, 2)):   # stale bytes, each buffer at the size it has
        o.upload(np.full(n, -7, np.int32))
    graph.launch()
    want = eager["b"]
    assert np.array_equal(outs[0].to_numpy((2, nbest, 900), np.int32), want[0])
    assert np.array_equal(outs[1].to_numpy((2, nbest), np.int32), want[1])
    assert np.array_equal(outs[2].to_numpy((2, nbest), np.uint32), bits(want[2]))
    assert np.array_equal(outs[3].to_numpy((2,), np.int32), want[3])
    graph.close()


@pytest.mark.gpu
def test_host_cpp_ctc_beam_demo_matches_python(ctx, tmp_path):
    ids, lp, off = packed_table()
    _, k, beam, nbest = PACKED
    d = str(tmp_path)
    for name, a in (("ids.i32", ids), ("lp.f32", lp), ("off.i64", off), ("dims.i64", np.array([k, 4, 0, beam, nbest, 48], np.int64))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    r = subprocess.run([_build_demo(), "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    rd = lambda n, t: np.fromfile(os.path.join(d, n), t)  # noqa: E731
    got = search(ctx, ids, lp, off, beam=beam, nbest=nbest, skip_rows=4, width=48)
    assert list(rd("shape.i64", np.int64)) == [len(off) - 1, nbest, 48]
    assert np.array_equal(rd("tokens.i32", np.int32), got[0].reshape(-1)) and np.array_equal(rd("lengths.i32", np.int32), got[1].reshape(-1))
    assert np.array_equal(rd("scores.f32", np.uint32), bits(got[2]).reshape(-1)) and np.array_equal(rd("counts.i32", np.int32), got[3])


@pytest.mark.gpu
def test_encoder_beam_segments_end_to_end(ctx):
    from lele_amd.apps import beam_results
    from sensevoice_graph import VOCAB, Encoder
    enc = Encoder(ctx, layers=2, seed=3)
    rng = np.random.default_rng(11)
    off = np.array([0, 7, 28], np.int64)
    pf = ctx.buf().upload(rng.standard_normal((28, 560)).astype(np.float32))
    got = tuple(o.numpy().copy() for o in enc.beam_segments(pf, off, 4, 4, 2))
    ci, cl, off4 = enc.topk_segments(pf, off, 4)
    ci, cl, off4 = ci.numpy().copy(), cl.numpy().copy(), np.asarray(off4)
    assert list(off4) == [0, 11, 36] and got[0].shape == (2, 2, 21)
    want = []
    for i in range(2):
        res, _, bad, _ = host_margin(ci[off4[i] + 4:off4[i + 1]], cl[off4[i] + 4:off4[i + 1]], 0, 4, 2)
        assert not bad and res == ctc_prefix_beam_search(ci[off4[i] + 4:off4[i + 1]], cl[off4[i] + 4:off4[i + 1]], 0, 4, 2)
        want.append(res)
    check_against_host(got, want, [7, 21], "encoder")
    # beam 1 over the single best candidate is the greedy path, collapsed
    one = tuple(o.numpy().copy() for o in enc.beam_segments(pf, off, 1, 1, 1))
    frame_ids, counts = enc.greedy_segments(pf, off, np.zeros(VOCAB, np.uint8))       # nothing skipped: every frame's id, prompt rows too
    frame_ids, counts = frame_ids.numpy(), counts.numpy()
    assert list(counts) == [11, 25]
    for i, lists in enumerate(beam_results(*one)):
        path = frame_ids[i, 4:counts[i]]
        keep = np.concatenate([[True], path[1:] != path[:-1]]) & (path != 0)
        assert len(lists) == 1 and lists[0][0] == tuple(int(v) for v in path[keep]), i
    # the dense form: both utterances of one length
    df = ctx.buf().upload(rng.standard_normal((2, 9, 560)).astype(np.float32))
    dense = tuple(o.numpy().copy() for o in enc.beam(df, 4, 4, 2))
    di, dl = enc.topk(df, 4)
    di, dl = di.numpy(), dl.numpy()
    assert dense[0].shape == (2, 2, 9)
    check_against_host(dense, [ctc_prefix_beam_search(di[b, 4:], dl[b, 4:], 0, 4, 2) for b in range(2)], [9, 9], "encoder dense")
