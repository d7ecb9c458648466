"""lele_hip_attention_segments_long: the packed attention without the 512-row limit (utterances over 30 s in one batch).

A segment of at most 512 rows must come out of the new call exactly as lele_hip_attention_segments gives it; a longer one runs the
one-pass kernel (attention_flash_kernel<SEG>) on its own length and is held to the float64 reference under the derived bound of
tests/test_attention_routes.py with that file's C_BOUND, not re-fitted.  The new call reports the existing route attn.seg.

Lengths (t_q == t_k == the segment's length), the smallest at which the long form can go wrong:
    513   one key in the last tile; the smallest long segment          544   a multiple of 32: no masked tile
    545   one key past a full tile                                      640   a multiple of 128: only full query blocks
    641   one live row in the last block, three idle compute waves      1025  33 tiles: the producers' six-step loop wraps five times

CPU part: the symbol in all four bindings, the route names unchanged, and the three conditions tests/test_attention_routes.py states for
its own table, on these lengths: the oracle's f32 composition inside C_BOUND / 4, the bound inside the project's 1e-4 bar on the
moderate families, every emulated wrong kernel rejected at 4 x the bound in at least one family.

GPU part: every family in a mixed layout; short segments bit for bit attention_segments'; a long segment's bits independent of order,
neighbours and batch; Q | K | V as column slices of a wider NaN row; the errors; 8 heads; the encoder on utterances over 30 s, eager
and recorded into a graph."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_attention_routes import (C_BOUND, DH, FAMILIES, H, MODERATE, NOT_REACHABLE, SEG_LENGTHS, TABLE, VARIANTS, _env, case, check,  # noqa: E402
                                   check_family, heads, merged, outside, scale_operand, worst)
from test_encoder_segments import SV_MAX_MAE, _packed_feats, logits_agreement, offsets_of  # noqa: E402

NAME = "lele_hip_attention_segments_long"
LONG = [513, 544, 545, 640, 641, 1025]
LAYOUT = [513, 33, 544, 0, 545, 171, 1025, 640, 641]
FAMS = [name for name, _ in FAMILIES]


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_symbol_is_declared_exported_and_wrapped_in_all_four_bindings():
    from lele_amd import _lib
    from lele_amd import kernels as K
    assert NAME in set(_lib.exported_symbols())
    assert hasattr(_lib.lib(), NAME) and callable(K.attention_segments_long)
    assert "int %s(LeleCtx* ctx" % NAME in open(os.path.join(ROOT, "include", "lele_hip.h")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "lele_amd", "host", "lele.hpp")).read()
    assert "pub fn %s(" % NAME in open(os.path.join(ROOT, "rust", "lele-hip", "src", "ffi.rs")).read()
    assert "attention_segments_long" in K.attention_segments.__doc__


def test_route_names_are_the_ones_the_route_table_covers():
    from lele_amd import kernels as K
    mine = {s for s in K.route_names() if s.startswith("attn.")}
    assert mine == {lvl for row in TABLE for lvl in row["route"].split("/")} | NOT_REACHABLE


def test_layout_holds_every_length_and_short_segments_of_two_classes():
    assert set(LONG) <= set(LAYOUT) and 0 in LAYOUT and sum(1 for n in LAYOUT if 0 < n <= 512) >= 2
    assert all(n > 512 for n in LONG) and 544 % 32 == 0 and 640 % 128 == 0 and 641 % 128 == 1 and 513 % 32 == 1 and 545 % 32 == 1
    assert -(-1025 // 32) == 33 > 5 * 6


@pytest.mark.parametrize("n", LONG)
def test_oracle_composition_within_a_quarter_of_the_bound(orc, n):
    ratios = {}
    for fam in FAMS:
        inp = case(fam, 1, n, n, True)
        s = orc.matmul(inp["q"], np.ascontiguousarray(inp["k"].transpose(0, 1, 3, 2)))
        o = orc.matmul(orc.softmax(s * inp["scale"], -1), inp["v"])
        ratios[fam] = worst(o, inp)
    print("%d rows: oracle composition / bound(C_BOUND = 1): " % n + "   ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= C_BOUND / 4, ratios


@pytest.mark.parametrize("n", LONG)
def test_bound_is_never_looser_than_the_project_bar_on_moderate_inputs(n):
    for fam in MODERATE:
        inp = case(fam, 1, n, n, True)
        o = inp["o"]
        bar = 1e-4 * (np.abs(o) + np.sqrt(np.mean(np.square(o))))
        loose = C_BOUND * inp["bound1"] > bar
        assert not loose.any(), "%d rows %s: bound up to %.3g of the 1e-4 bar" % (n, fam, float(np.max(C_BOUND * inp["bound1"] / bar)))


@pytest.mark.parametrize("n", LONG)
def test_tolerance_rejects_wrong_variants(n):
    seen = {name: False for name, _, applies in VARIANTS if applies(n, n, True)}
    if n % 64:
        assert len(seen) == len(VARIANTS)
    for fam in FAMS:
        inp = case(fam, 1, n, n, True)
        q, k, v, sc = inp["q"], inp["k"], inp["v"], inp["scale"]
        assert not outside(inp["o"].astype(np.float32), inp, 1).any(), "the reference itself, rounded to f32, fails the bound"
        for name, emul, _ in VARIANTS:
            if name in seen and not seen[name]:
                seen[name] = bool(outside(emul(q, k, v, sc), inp, 4).any())
    missed = [name for name, hit in seen.items() if not hit]
    assert not missed, "%d rows: no family tells %s from the operation" % (n, missed)


# -------------------------------------------------------------------------------------------------------------------- GPU
def packed(cases, key=lambda c: (c["q"], c["k"]), nh=H):
    """the cases' Q | K | V as packed rows [R, 3 * nh * DH]; a case is [n, H, t, DH] with n * H == nh heads"""
    def m(a):
        a = a.reshape((1, nh) + a.shape[2:])
        return np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(a.shape[2], nh * DH)
    parts = [np.concatenate([m(key(c)[0]), m(key(c)[1]), m(c["v"])], -1) for c in cases if c is not None]
    return np.concatenate(parts, 0)


def run_long(ctx, qkv, lengths, sc, nh=H, **kw):
    from lele_amd import kernels as K
    got = K.attention_segments_long(ctx.buf().upload(qkv), offsets_of(lengths), nh, DH, scale=scale_operand(sc), ctx=ctx, **kw).numpy()
    assert got.shape == (int(np.sum(lengths)), nh * DH)
    assert K.last_route(ctx) == "attn.seg"
    return got


def segs(got, lengths):
    off = offsets_of(lengths)
    return [got[off[i]:off[i + 1]] for i in range(len(lengths))]


@pytest.fixture(scope="module")
def random_layout(ctx):
    """the `random` family on LAYOUT: (qkv, scale, the new call's result), shared and read only"""
    cases = [case("random", 1, n, n, True) if n else None for n in LAYOUT]
    qkv = packed(cases)
    got = run_long(ctx, qkv, LAYOUT, cases[0]["scale"])
    qkv.setflags(write=False)
    got.setflags(write=False)
    return qkv, cases[0]["scale"], got


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
def test_every_family_in_a_mixed_layout(ctx, fam):
    cases = [case(fam, 1, n, n, True) if n else None for n in LAYOUT]
    sc = cases[0]["scale"]
    got = segs(run_long(ctx, packed(cases), LAYOUT, sc), LAYOUT)
    got0 = segs(run_long(ctx, packed(cases, lambda c: c["unshifted"]), LAYOUT, sc), LAYOUT) if fam.startswith("shift") else [None] * len(LAYOUT)
    ratios, failures = [], []
    for n, c, g, g0 in zip(LAYOUT, cases, got, got0):
        if not n:
            continue
        try:
            ratios.append("%d: %.2f" % (n, check_family(fam, c, heads(g)[None], None if g0 is None else heads(g0)[None], "segment of %d rows" % n)))
        except AssertionError as e:
            failures.append(str(e))
    print("%s: worst |got - f64| / bound by length  %s" % (fam, "  ".join(ratios)))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_short_segments_are_attention_segments_bit_for_bit(ctx, random_layout):
    from lele_amd import kernels as K
    qkv, sc, got = random_layout
    short = [n if n <= 512 else 0 for n in LAYOUT]
    rows = np.concatenate([np.full(n, n <= 512) for n in LAYOUT])
    want = K.attention_segments(ctx.buf().upload(qkv[rows]), offsets_of(short), H, DH, scale=scale_operand(sc), ctx=ctx).numpy()
    assert rows.sum() == 33 + 171 and np.array_equal(got[rows], want)
    # no long segment in the layout: the old call's array
    cases = [case("random", 1, n, n, True) if n else None for n in SEG_LENGTHS]
    q2 = packed(cases)
    want = K.attention_segments(ctx.buf().upload(q2), offsets_of(SEG_LENGTHS), H, DH, scale=scale_operand(sc), ctx=ctx).numpy()
    assert np.array_equal(run_long(ctx, q2, SEG_LENGTHS, sc), want)


@pytest.mark.gpu
def test_a_segment_depends_on_its_own_rows_only(ctx, random_layout):
    qkv, sc, got = random_layout
    parts, res = segs(qkv, LAYOUT), segs(got, LAYOUT)
    rng = np.random.default_rng(5)
    # the same multiset of segments in another order
    perm = [int(i) for i in rng.permutation(len(LAYOUT))]
    assert perm != sorted(perm)
    l2 = [LAYOUT[i] for i in perm]
    for j, g in zip(perm, segs(run_long(ctx, np.concatenate([parts[i] for i in perm]), l2, sc), l2)):
        assert np.array_equal(g, res[j]), "segment %d (%d rows) moved with the order" % (j, LAYOUT[j])
    # one segment alone: a long one and a short one
    for j in (LAYOUT.index(641), LAYOUT.index(171)):
        assert np.array_equal(run_long(ctx, parts[j], [LAYOUT[j]], sc), res[j]), "segment of %d rows alone" % LAYOUT[j]
    # a victim's rows 40 x larger: no other row changes
    off = offsets_of(LAYOUT)
    for victim in (LAYOUT.index(1025), LAYOUT.index(171)):
        q3 = qkv.copy()
        q3[off[victim]:off[victim + 1]] = (rng.standard_normal((LAYOUT[victim], qkv.shape[1])) * 40).astype(np.float32)
        got3 = run_long(ctx, q3, LAYOUT, sc)
        keep = np.ones(len(qkv), bool)
        keep[off[victim]:off[victim + 1]] = False
        assert np.array_equal(got3[keep], got[keep]), "victim of %d rows" % LAYOUT[victim]
        assert np.isfinite(got3).all() and not np.array_equal(got3[~keep], got[~keep])


@pytest.mark.gpu
def test_views_of_a_wider_nan_row(ctx, random_layout):
    """V | gap | Q | gap | K inside a wider row that is NaN everywhere else: no NaN out, the bits of the tight copy"""
    qkv, sc, got = random_layout
    d = H * DH
    vo, qo, ko = 4, 4 + d + 8, 4 + d + 8 + d + 12
    wide = np.full((len(qkv), ko + d + 4), np.nan, np.float32)
    wide[:, qo:qo + d], wide[:, ko:ko + d], wide[:, vo:vo + d] = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    res = run_long(ctx, wide, LAYOUT, sc, q_offset=qo, k_offset=ko, v_offset=vo)
    assert not np.isnan(res).any(), "%d results are NaN: the kernel read outside its columns" % int(np.isnan(res).sum())
    assert np.array_equal(res, got)


@pytest.mark.gpu
def test_both_work_lists_survive_the_store_dropping_unused_tables(random_layout):
    """The call takes two layout tables, and a miss drops every table no capture has used once 64 of them are around.  In a context
    of its own 63 layouts leave 63 such tables; the call's short lists are the 64th, its long list finds the store full and drops
    them all, the short lists among them: they must be fetched again, not read where they were"""
    from lele_amd import _lib
    from lele_amd import kernels as K
    qkv, sc, got = random_layout
    own = _lib.Ctx(0)
    try:
        x = own.buf().upload(qkv[:64])
        for i in range(63):
            K.attention_segments(x, [0, i + 1, 64], H, DH, ctx=own)
        assert np.array_equal(run_long(own, qkv, LAYOUT, sc), got)
        assert np.array_equal(run_long(own, qkv, LAYOUT, sc), got)
    finally:
        own.close()


@pytest.mark.gpu
def test_errors_leave_out_untouched(ctx):
    import lele_amd
    from lele_amd import kernels as K
    rng = np.random.default_rng(1)
    big = ctx.buf().upload(rng.standard_normal((3 + 513, 1536)).astype(np.float32))
    out = ctx.buf()
    good = [0, 3, 516]
    shape = K.attention_segments_long(big, good, H, DH, out=out, ctx=ctx).shape
    before = out.to_numpy(shape).copy()
    assert shape == (516, 512) and np.isfinite(before).all()
    with _env(LELE_HIP_ATTENTION_EXACT=1):
        with pytest.raises(lele_amd.LeleError, match="segment 1 has 513 rows.*LELE_HIP_ATTENTION_EXACT"):
            K.attention_segments_long(big, good, H, DH, out=out, ctx=ctx)
        assert np.array_equal(out.to_numpy(shape), before)
        # short segments behave as today
        a = K.attention_segments_long(big, [0, 3, 4, 516], H, DH, ctx=ctx).numpy()
        assert K.last_route(ctx) == "attn.seg_exact"
        assert np.array_equal(a, K.attention_segments(big, [0, 3, 4, 516], H, DH, ctx=ctx).numpy())
    for bad, msg in (([0, 30, 20, 516], "decrease"), ([1, 10, 516], "from 0 to R"), ([0, 10, 515], "from 0 to R"), ([0, 10, 517], "from 0 to R")):
        with pytest.raises(lele_amd.LeleError, match=msg):
            K.attention_segments_long(big, bad, H, DH, out=out, ctx=ctx)
    with pytest.raises(lele_amd.LeleError, match="head dimension 64"):
        K.attention_segments_long(big, good, 8, 64, out=out, ctx=ctx)
    with pytest.raises(lele_amd.LeleError, match="16-byte"):
        K.attention_segments_long(big, good, H, DH, q_offset=2, k_offset=512, v_offset=1024, out=out, ctx=ctx)
    assert np.array_equal(out.to_numpy(shape), before)
    # the old call still refuses, and says so as before
    with pytest.raises(lele_amd.LeleError, match="segment 1 has 513 rows, at most 512"):
        K.attention_segments(big, good, H, DH, out=out, ctx=ctx)
    assert np.array_equal(out.to_numpy(shape), before)


L8 = [513, 0, 700, 33]


@pytest.mark.gpu
def test_eight_heads(ctx):
    """8 heads = two batch elements of a 4-head case side by side; every family against the bound, then the bitwise properties"""
    def as8(c):
        return {k: (v.reshape((1, 8) + v.shape[2:]) if isinstance(v, np.ndarray) else
                    tuple(a.reshape((1, 8) + a.shape[2:]) for a in v) if isinstance(v, tuple) else v) for k, v in c.items()}
    failures = []
    for fam in FAMS:
        cases = [as8(case(fam, 2, n, n, True)) if n else None for n in L8]
        sc = cases[0]["scale"]
        h8 = lambda g: g.reshape(len(g), 8, DH).swapaxes(0, 1)[None]   # noqa: E731
        got = segs(run_long(ctx, packed(cases, nh=8), L8, sc, nh=8), L8)
        got0 = segs(run_long(ctx, packed(cases, lambda c: c["unshifted"], nh=8), L8, sc, nh=8), L8) if fam.startswith("shift") else [None] * len(L8)
        for n, c, g, g0 in zip(L8, cases, got, got0):
            if n:
                try:
                    check_family(fam, c, h8(g), None if g0 is None else h8(g0), "%s, segment of %d rows" % (fam, n))
                except AssertionError as e:
                    failures.append(str(e))
    assert not failures, "\n".join(failures)
    cases = [as8(case("random", 2, n, n, True)) if n else None for n in L8]
    qkv, sc = packed(cases, nh=8), cases[0]["scale"]
    got = run_long(ctx, qkv, L8, sc, nh=8)
    parts, res = segs(qkv, L8), segs(got, L8)
    perm = [2, 3, 0, 1]
    l2 = [L8[i] for i in perm]
    for j, g in zip(perm, segs(run_long(ctx, np.concatenate([parts[i] for i in perm]), l2, sc, nh=8), l2)):
        assert np.array_equal(g, res[j])
    assert np.array_equal(run_long(ctx, parts[2], [700], sc, nh=8), res[2])
    off = offsets_of(L8)
    for victim in (2, 3):
        q3 = qkv.copy()
        q3[off[victim]:off[victim + 1]] *= np.float32(40)
        got3 = run_long(ctx, q3, L8, sc, nh=8)
        keep = np.ones(len(qkv), bool)
        keep[off[victim]:off[victim + 1]] = False
        assert np.array_equal(got3[keep], got[keep]) and not np.array_equal(got3[~keep], got[~keep])


E_LONG = [171, 520, 33, 0, 700]


@pytest.fixture(scope="module")
def enc3(ctx):
    from sensevoice_graph import Encoder, encoder_arrays
    enc = Encoder(ctx, layers=3, damped=True)
    return enc, encoder_arrays(enc)


@pytest.mark.gpu
def test_encoder_takes_utterances_over_30_s(ctx, enc3, monkeypatch):
    from oracle import pyoracle as O
    from oracle import sensevoice_ref as R
    enc, arrays = enc3
    rng = np.random.default_rng(80)
    off = offsets_of(E_LONG)
    f = _packed_feats(rng, E_LONG)
    logits, off4 = enc.forward_segments(ctx.buf().upload(f), off)
    logits = logits.numpy().copy()
    assert np.array_equal(off4, off + 4 * np.arange(len(off))) and np.isfinite(logits).all()
    # every utterance alone through the same call: its bits
    for s, ln in enumerate(E_LONG):
        alone, _ = enc.forward_segments(ctx.buf().upload(f[off[s]:off[s + 1]]) if ln else f[:0], [0, ln])
        assert np.array_equal(alone.numpy(), logits[off4[s]:off4[s + 1]]), "utterance %d (%d rows) alone" % (s, ln)
    # greedy ids of the packed batch: the host decode of each utterance's logits
    skip = np.zeros(logits.shape[1], np.uint8)
    skip[0] = 1
    skip[::3] = 1
    ids, counts = enc.greedy_segments(ctx.buf().upload(f), off, skip)
    g, c = ids.numpy(), counts.numpy()
    assert g.shape == (len(E_LONG), max(E_LONG) + 4)
    for s in range(len(E_LONG)):
        seg = logits[off4[s]:off4[s + 1]]
        a, b = O.decode_greedy_ids(seg[None], skip)
        assert c[s] == b[0] and np.array_equal(g[s, :len(seg)], a[0]) and (g[s, len(seg):] == -1).all(), s
    # a long utterance against the oracle's forward, at the bar of tests/test_encoder_segments.py's end-to-end comparison
    s = E_LONG.index(520)
    r = logits_agreement(logits[off4[s]:off4[s + 1]], R.encoder_forward(f[off[s]:off[s + 1]][None], arrays)[0])
    print("utterance of 520 rows packed vs oracle encoder: mae %.4g, arg-max agreement %.4f" % (r["mae"], r["argmax_agreement"]))
    assert r["mae"] <= SV_MAX_MAE, r
    # the short utterances: the bits of the path without the new call (layer_segments on attention_segments)
    monkeypatch.setattr(enc.K, "attention_segments_long", enc.K.attention_segments)
    short = [ln if ln <= 512 else 0 for ln in E_LONG]
    rows = np.concatenate([np.full(ln, ln <= 512) for ln in E_LONG])
    old, o4 = enc.forward_segments(ctx.buf().upload(f[rows]), offsets_of(short))
    old = old.numpy()
    for s, ln in enumerate(E_LONG):
        if ln <= 512:
            assert np.array_equal(old[o4[s]:o4[s + 1]], logits[off4[s]:off4[s + 1]]), "utterance %d (%d rows)" % (s, ln)


@pytest.mark.gpu
def test_graph_capture_with_a_long_utterance(ctx):
    """recorded after one eager run: the replay equals eager bit for bit, again after new features went into the same buffer"""
    from sensevoice_graph import Encoder
    enc = Encoder(ctx, layers=2, damped=True)
    rng = np.random.default_rng(81)
    layout = [171, 520, 0, 33]
    off = offsets_of(layout)
    buf = ctx.buf()
    feats = buf.upload(_packed_feats(rng, layout))
    eager = enc.forward_segments(feats, off)[0].numpy()   # sizes the workspace, uploads the layout's tables
    eager = enc.forward_segments(feats, off)[0].numpy()
    ctx.graph_begin()
    res, _ = enc.forward_segments(feats, off)
    g, out, shape = ctx.graph_end(), res.raw().buf, res.shape
    out.upload(np.zeros(shape, np.float32))   # the replay must write every logit itself
    g.launch()
    assert np.array_equal(out.to_numpy(shape), eager)
    buf.upload(_packed_feats(rng, layout) * np.float32(0.7))
    g.launch()
    replay = out.to_numpy(shape).copy()
    assert not np.array_equal(replay, eager)
    assert np.array_equal(enc.forward_segments(feats, off)[0].numpy(), replay)
    g.close()
