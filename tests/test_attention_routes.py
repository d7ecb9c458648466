"""Every attention route against a float64 reference, one table row per dispatch branch and key-tile class.

lele_hip_attention_view picks one of three kernels by grid size (16, 32 or 64 query rows per workgroup on LDS score tiles; the
one-pass kernel with producer waves), each of the first three in eight key-tile classes and with LELE_HIP_ATTENTION_EXACT on and off;
lele_hip_attention_segments runs the 16- / 32-row kernels behind a work list.  Every row of TABLE names the route the library must
report (kernels.last_route()), so a re-tune that moves a shape to another kernel fails here instead of leaving that kernel untested.

Reference: plain numpy float64 per (batch, head) on the same f32 inputs -- s = scale * Q K^T, a max-subtracted softmax, P V.

Acceptance: per output element, derived (u = 2^-24, E[i, j] = scale * sum_d |q[i, d]| |k[j, d]|):
    rel[i, j]   = C_BOUND * u * (2 max_j E[i, j] + 2 E[i, j] + |s[i, j] - max_j s[i, j]| + 8)
    bound[i, d] = sum_j p[i, j] * rel[i, j] * |v[j, d]|
The E terms: a score's rounding in any summation order, the cross terms the split-bf16 products drop, the one-pass kernel's single
rounding of q * scale * log2 e (the maximum's own error moves every exponent of the row: 2 max E).  |s - max|: the rounding of the
exponential's argument.  8: the exponential itself, the sum, the division.  C_BOUND is measured on the oracle's f32 composition,
never on a kernel (see C_BOUND below).

Input families (FAMILIES): except `random` and `wide` the scores are small integers (or multiples of 2^-10) on a few dimensions with a
query operand of at most 8 significant bits and scale 0.125 or none, so they are exact in f32 in any order and through the three-piece
bf16 split: the softmax and P V stages are tested on exactly known scores.

CPU part: name coverage, the oracle composition inside C_BOUND / 4, the bound never looser than the project's 1e-4 on the moderate
families, and every row's tolerance rejecting emulated wrong kernels (VARIANTS) by 4 x the bound in at least one family.

GPU part: per row, the route and every family inside the bound (Q in its own buffer, K and V column slices of a second, t_q != t_k);
per kernel, the operands as views of parents that are NaN everywhere else (no NaN out, the bits of tight copies), the {min, max}
statistics feeding the quantised projection, and the [b, H, t_q, 128] output form against the merged one, bit for bit."""
import functools
import os
import re

import numpy as np
import pytest

H, DH = 4, 128
U = 2.0 ** -24
LOG2E = np.float32(1.44269504088896341)
FLT_MAX = np.float32(3.40282347e+38)

# C_BOUND.  Measured on the CPU: the worst |orc.matmul -> orc.softmax -> orc.matmul  -  float64| / bound(C_BOUND = 1) over every
# (row, family) of TABLE (test_oracle_composition_within_a_quarter_of_the_bound prints them with -s):
#     random 0.105   ramp_under8 0.183   ramp_over8 0.167   ramp_3 0.350   ramp_down 0.195   shift_pos 0.000   shift_neg 0.000
#     two_peak 0.002   wide 0.205
# (the shifted scores are exact integers and their bound carries E = 30000; two_peak's weights are exactly 1/2).  Four times the
# worst ratio, 1.40 (the margin for the three roundings a product the split-bf16 routes add to the f32 composition), rounded up to
# a power of two.  One constant for all routes.
C_BOUND = 2.0

QC = [["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
KC = [["slice", 2, 0, H * DH], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 3, 1]]]
VC = [["slice", 2, H * DH, H * DH], ["reshape", [0, 0, H, DH]], ["transpose", [0, 2, 1, 3]]]
SEG_LENGTHS = [1, 33, 0, 64, 65, 171, 512, 300]


# ---------------------------------------------------------------------------------------------------------------- the table
def R(route, b, tq, tk, exact=0, scaled=True):
    return dict(route=route, b=b, tq=tq, tk=tk, exact=exact, scaled=scaled)


def _nt(tk):
    return "attn.nt%d" % (2 * ((tk + 63) // 64))


# the dispatch on a 256-CU device, fb = 4 b:  rows16 if fb * ceil(tq / 32) < 128;  flash if (not exact and) fb * ceil(tq / 128) >= 128;
# 64 rows if fb * ceil(tq / 64) >= 768;  else 32 rows
TK_CLASSES = [1, 33, 64, 65, 129, 193, 257, 321, 385, 449, 512]   # classes 1, 1, 1, 2 .. 8, 8
TABLE = []
# rows16: b = 1 -> fb * ceil(tq / 32) = 4, 8 (tq = 17, 40), 64 (tq = 512) < 128
TABLE += [R("attn.rows16/" + _nt(tk), 1, (17, 40)[i & 1], tk) for i, tk in enumerate(TK_CLASSES)]
TABLE += [R("attn.rows16/attn.nt16", 1, 1, 512), R("attn.rows16/attn.nt2", 1, 512, 1)]
# rows32: b = 16, tq in 33 .. 64 -> 64 * 2 = 128 blocks of 32 rows (not rows16), 64 * 1 blocks of 128 (not flash), 64 of 64 rows (< 768)
TABLE += [R("attn.rows32/" + _nt(tk), 16, 40, tk) for tk in TK_CLASSES]
TABLE += [R("attn.rows32/attn.nt6", 16, 33, 171), R("attn.rows32/attn.nt10", 16, 64, 300)]
# flash: b = 32 -> 128 * ceil(tq / 32) >= 128 and 128 * ceil(tq / 128) >= 128;  b = 16, tq = 129 -> 64 * 2 = 128: the second workgroup
# of a head has one live row and three idle compute waves
TABLE += [R("attn.flash", 32, 1, 33), R("attn.flash", 32, 1, 512), R("attn.flash", 32, 97, 1), R("attn.flash", 32, 97, 31),
          R("attn.flash", 32, 97, 100), R("attn.flash", 32, 97, 511), R("attn.flash", 32, 128, 32), R("attn.flash", 32, 128, 64),
          R("attn.flash", 32, 128, 512), R("attn.flash", 16, 129, 33), R("attn.flash", 16, 129, 171), R("attn.flash", 16, 129, 511),
          R("attn.flash", 32, 171, 171)]   # the last: t_q == t_k
# the f32 replicas, classes 1, 3, 8 (EXACT never takes the one-pass kernel)
TABLE += [R("attn.rows16_exact/" + _nt(tk), 1, tq, tk, exact=1) for tq, tk in ((40, 33), (17, 129), (40, 449))]
TABLE += [R("attn.rows32_exact/" + _nt(tk), 16, 40, tk, exact=1) for tk in (33, 129, 449)]
# 64 rows: fb * ceil(tq / 64) = 768 * 1 >= 768.  The view chain (slice, reshape, transpose) cannot give K and V a zero batch stride,
# so the class-8 row uploads 192 x 449 x 1024 floats a family: the slowest row of the table
TABLE += [R("attn.rows64_exact/" + _nt(tk), 192, 40, tk, exact=1) for tk in (33, 171, 449)]
# no scale operand (integer-score families only)
TABLE += [R("attn.rows16/attn.nt8", 1, 40, 193, scaled=False), R("attn.flash", 32, 97, 100, scaled=False)]
# the packed form: every segment (t_q == t_k == its length) on the 16-row kernel of its class, one launch per class
TABLE += [R("attn.seg", 0, 0, 0), R("attn.seg", 0, 0, 0, exact=1)]
TABLE[-1]["route"] = "attn.seg_exact"

# attention_kernel<NT, 2, false> is instantiated but no product call reaches it: two row tiles need fb * ceil(tq / 64) >= 3 CUs, and
# then fb * ceil(tq / 128) >= fb * ceil(tq / 64) / 2 >= 1.5 CUs >= CUs / 2 and fb * ceil(tq / 32) >= CUs / 2, which is the one-pass
# kernel's condition unless the output view is off the 16-byte grid -- and kernels.attention_view / plan_runner.hpp build the output
# view from row-major strides of dimensions that end in the head dimension (multiples of 128) at offset 0 of an allocation
NOT_REACHABLE = {"attn.rows64"}


def row_id(i, row):
    return "%d-%s-b%d-q%d-k%d%s" % (i, row["route"].replace("/", "+"), row["b"], row["tq"], row["tk"], "" if row["scaled"] else "-noscale")


ROW_IDS = [row_id(i, r) for i, r in enumerate(TABLE)]


def shapes_of(row):
    """(unique batch elements, t_q, t_k) of every attention problem of the row (the packed form: one per non-empty segment).  A dense
    row's batch repeats min(b, 3) distinct elements: 3 is coprime to the 8 heads' worth of workgroups the one-pass kernel regroups"""
    if row["route"].startswith("attn.seg"):
        return [(1, n, n) for n in SEG_LENGTHS if n]
    return [(min(row["b"], 3), row["tq"], row["tk"])]


# ------------------------------------------------------------------------------------------------------------ input families
# a family: f(rng, n, tq, tk, scaled) -> dict(q, k, v [n, H, t, DH] f32, scale (np.float32 or None), + what its extra checks need)
def _spread_v(rng, n, tk):
    """V: standard normal, half of the entries scaled by 2^e, e uniform in [-40, 40] (as tests/test_f32_routes.py spreads its operands):
    a dropped middle or low bf16 piece of P or V shows as 2^-9 or 2^-18 of a large term"""
    v = rng.standard_normal((n, H, tk, DH))
    pick = rng.random(v.shape) < 0.5
    v[pick] *= 2.0 ** rng.integers(-40, 41, int(pick.sum()))
    return v.astype(np.float32)


def fam_random(rng, n, tq, tk, scaled):
    """N(0, 1.5^2) everywhere, scale 128^-0.5: the baseline (what tests/test_attention.py feeds every kernel)"""
    mk = lambda t: (rng.standard_normal((n, H, t, DH)) * 1.5).astype(np.float32)
    return dict(q=mk(tq), k=mk(tk), v=mk(tk), scale=np.float32(DH ** -0.5))


def fam_wide(rng, n, tq, tk, scaled):
    """N(0, 6^2) Q and K, scale 128^-0.5: |s| reaches tens, rows are near one-hot with near-ties -- the rounding of the exponential's
    argument and of the scores themselves.  Held to the derived bound only"""
    mk = lambda t, s: (rng.standard_normal((n, H, t, DH)) * s).astype(np.float32)
    return dict(q=mk(tq, 6.0), k=mk(tk, 6.0), v=mk(tk, 1.0), scale=np.float32(DH ** -0.5))


def _ramp(rise, down):
    def fam(rng, n, tq, tk, scaled):
        qm = 8.0 if scaled else 1.0
        pos = np.arange(tk)[::-1] if down else np.arange(tk)
        step = rise * np.log(2.0) / 32.0   # nats per key
        q = np.zeros((n, H, tq, DH), np.float32)
        k = np.zeros((n, H, tk, DH), np.float32)
        # the ramp proper over the top 64 nats (11 tiles at 8.2 units a tile), flat below (a key 64 nats under the maximum weighs
        # nothing in float64 either), centred: |s| <= 32 keeps E, and with it the bound, inside the project's 1e-4 (condition (a))
        ramp = np.maximum((pos - (tk - 1)) * step, -64.0)
        k[..., 0] = np.round((ramp - ramp.min() / 2.0) * 1024.0) / 1024.0
        q[..., 0] = qm
        k[..., 1] = rng.integers(0, 2, (n, H, tk)) / 16.0    # 0.09 log2 units on half of the rows: rows differ, the tile rise keeps its side of 8
        q[..., 1] = qm * rng.integers(0, 2, (n, H, tq))
        return dict(q=q, k=k, v=_spread_v(rng, n, tk), scale=np.float32(0.125) if scaled else None)
    fam.__doc__ = """scores %s with the key index by %.1f log2 units per 32-key tile, so the maximum is the %s valid key: the one-pass
    kernel's lazy offset (it moves when a tile's maximum exceeds it by more than 8), a rescale applied to l but not O or to O but not l,
    a maximum taken over the first tile only""" % ("fall" if down else "rise", rise, "first" if down else "last")
    return fam


def _shift(sign):
    def fam(rng, n, tq, tk, scaled):
        qm = 8.0 if scaled else 1.0
        q = np.zeros((n, H, tq, DH), np.float32)
        k = np.zeros((n, H, tk, DH), np.float32)
        for d in (0, 1):
            q[..., d] = qm * rng.integers(-2, 3, (n, H, tq))
            k[..., d] = rng.integers(-3, 4, (n, H, tk))
        q0, k0 = q.copy(), k.copy()
        q[..., 2] = qm * 30.0
        k[..., 2] = sign * 1000.0
        v = rng.standard_normal((n, H, tk, DH)).astype(np.float32)
        return dict(q=q, k=k, v=v, scale=np.float32(0.125) if scaled else None, unshifted=(q0, k0))
    fam.__doc__ = """every score carries the common offset %+d (one shared dimension) over integer differences in [-12, 12]; the result
    must be the unshifted one: a missing or late max subtraction, padded keys scored as 0""" % (sign * 30000)
    return fam


def peak_positions(tk):
    """the second peak of head h (the first is key tk - 1); a position that is not a key before the last gives a single peak"""
    return [p if p < tk - 1 else tk - 1 for p in (0, 31, 32, tk // 3)]


def fam_two_peak(rng, n, tq, tk, scaled):
    """two keys tie for the maximum 100+ nats above the rest: key t_k - 1 and, by head, key 0, 31, 32 or t_k / 3 (a position at or past
    the last key: a single peak).  O must be the mean of the two V rows: an unmasked re-read of the last key gives weights 1/3 and 2/3,
    a dropped last key weight 1; the rest sits near exp(-104), where v_exp_f32's result is denormal"""
    qm = 8.0 if scaled else 1.0
    q = np.zeros((n, H, tq, DH), np.float32)
    k = np.zeros((n, H, tk, DH), np.float32)
    q[..., 0] = qm * rng.integers(-1, 2, (n, H, tq))
    k[..., 0] = rng.integers(-3, 4, (n, H, tk))
    q[..., 3] = qm * 8.0
    v = _spread_v(rng, n, tk)
    mean = np.empty((n, H, 1, DH), np.float64)
    for h, p in enumerate(peak_positions(tk)):
        for key in (p, tk - 1):
            k[:, h, key, 0] = 0.0
            k[:, h, key, 3] = 13.0   # 0.125 * 64 * 13 = 104
        mean[:, h, 0] = (v[:, h, p].astype(np.float64) + v[:, h, tk - 1].astype(np.float64)) / 2
    return dict(q=q, k=k, v=v, scale=np.float32(0.125) if scaled else None, mean=mean)


FAMILIES = [("random", fam_random), ("ramp_under8", _ramp(7.8, False)), ("ramp_over8", _ramp(8.2, False)), ("ramp_3", _ramp(3.0, False)),
            ("ramp_down", _ramp(8.2, True)), ("shift_pos", _shift(1)), ("shift_neg", _shift(-1)), ("two_peak", fam_two_peak), ("wide", fam_wide)]
MODERATE = ("random", "ramp_under8", "ramp_over8", "ramp_3", "ramp_down")
INTEGER_SCORES = tuple(name for name, _ in FAMILIES if name not in ("random", "wide"))


def families_of(row):
    return [name for name, _ in FAMILIES if row["scaled"] or name in INTEGER_SCORES]


# --------------------------------------------------------------------------------------------------- float64 reference
def reference(q, k, v, scale):
    """(o, bound at C_BOUND = 1), both [n, H, tq, DH] float64"""
    q, k, v = q.astype(np.float64), k.astype(np.float64), v.astype(np.float64)
    sc = 1.0 if scale is None else float(scale)
    s = sc * np.matmul(q, k.transpose(0, 1, 3, 2))
    e = sc * np.matmul(np.abs(q), np.abs(k).transpose(0, 1, 3, 2))
    d = s - s.max(-1, keepdims=True)
    p = np.exp(d)
    p /= p.sum(-1, keepdims=True)
    rel = U * (2 * e.max(-1, keepdims=True) + 2 * e + np.abs(d) + 8)
    return np.matmul(p, v), np.matmul(p * rel, np.abs(v))


@functools.lru_cache(maxsize=None)
def case(fam, n, tq, tk, scaled):
    """inputs and reference of one (family, shape), computed once and shared (read only) by every test and row that needs it"""
    idx = [name for name, _ in FAMILIES].index(fam)
    inp = FAMILIES[idx][1](np.random.default_rng([idx, n, tq, tk, int(scaled)]), n, tq, tk, scaled)
    inp["o"], inp["bound1"] = reference(inp["q"], inp["k"], inp["v"], inp["scale"])
    for a in inp.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp


def outside(got, inp, factor):
    """elements of got [.., n, H, tq, DH] that are not finite or further than factor * bound from the reference"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(got - inp["o"]) <= factor * C_BOUND * inp["bound1"])


def worst(got, inp):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - inp["o"]) / inp["bound1"]
    r = np.where(np.abs(got - inp["o"]) == 0, 0.0, r)
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


# ------------------------------------------------------------------------------------------------- emulated wrong kernels
def _scores(q, k, scale):
    s = np.matmul(q, k.transpose(0, 1, 3, 2))
    return s if scale is None else s * scale


def _softmax_pv(s, v):
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(s - s.max(-1, keepdims=True))
        return np.matmul(p, v) / p.sum(-1, keepdims=True)


def _neighbour(a):
    """the next (batch, head)'s operand"""
    n, h = a.shape[:2]
    return np.roll(a.reshape((n * h,) + a.shape[2:]), -1, axis=0).reshape(a.shape)


def _online(q, k, v, scale, skip):
    """the one-pass kernel's scheme in numpy f32: 32-key tiles, scores in log2 units, the lazy offset; skip = "O" / "l" leaves that
    rescale out, None is the scheme itself"""
    sc = LOG2E if scale is None else np.float32(scale * LOG2E)
    s = np.matmul(q * sc, k.transpose(0, 1, 3, 2))
    m = np.full(s.shape[:-1] + (1,), -FLT_MAX, np.float32)
    l = np.zeros_like(m)
    o = np.zeros(q.shape[:3] + (DH,), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for t0 in range(0, s.shape[-1], 32):
            st = s[..., t0:t0 + 32]
            mt = st.max(-1, keepdims=True)
            m_new = np.where(mt > m + np.float32(8), mt, m)
            alpha = np.exp2(m - m_new)
            if skip != "l":
                l = l * alpha
            if skip != "O":
                o = o * alpha
            m = m_new
            p = np.exp2(st - m)
            l = l + p.sum(-1, keepdims=True)
            o = o + np.matmul(p, v[..., t0:t0 + 32, :])
        return o / l


def v_drop_last(q, k, v, sc):
    return _softmax_pv(_scores(q, k[..., :-1, :], sc), v[..., :-1, :])


def v_last_twice(q, k, v, sc):
    return _softmax_pv(_scores(q, np.concatenate([k, k[..., -1:, :]], -2), sc), np.concatenate([v, v[..., -1:, :]], -2))


def v_pad_zero(q, k, v, sc):
    s = _scores(q, k, sc)
    return _softmax_pv(np.concatenate([s, np.zeros_like(s[..., :1])], -1), np.concatenate([v, v[..., -1:, :]], -2))


def v_pad_neighbour(q, k, v, sc):
    return _softmax_pv(_scores(q, np.concatenate([k, _neighbour(k)[..., :1, :]], -2), sc), np.concatenate([v, _neighbour(v)[..., :1, :]], -2))


def v_max_first_tile(q, k, v, sc):
    s = _scores(q, k, sc)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(s - s[..., :32].max(-1, keepdims=True))
        return np.matmul(p, v) / p.sum(-1, keepdims=True)


def v_no_scale(q, k, v, sc):
    return _softmax_pv(_scores(q, k, None), v)


def v_last_row(q, k, v, sc):
    o = _softmax_pv(_scores(q, k, sc), v).copy()
    o[..., -1, :] = o[..., -2, :]
    return o


# (name, emulation, applies(tq, tk, scaled)).  Keys are padded to a multiple of 64 (32 in the one-pass kernel): a padded key exists
# unless tk % 64 == 0; with one key a repeat or a zero-scored re-read of it changes nothing (both carry the same V row), nor do the scale and the query row
VARIANTS = [
    ("last key dropped", v_drop_last, lambda tq, tk, sc: tk > 1),
    ("last key counted twice", v_last_twice, lambda tq, tk, sc: tk > 1),
    ("one padded key scored 0", v_pad_zero, lambda tq, tk, sc: tk > 1 and tk % 64 != 0),
    ("one padded key scored as the neighbouring batch element's first key", v_pad_neighbour, lambda tq, tk, sc: tk % 64 != 0),
    ("maximum from the first 32 keys only", v_max_first_tile, lambda tq, tk, sc: tk > 32),
    ("online softmax without the O rescale", lambda q, k, v, sc: _online(q, k, v, sc, "O"), lambda tq, tk, sc: tk > 32),
    ("online softmax without the l rescale", lambda q, k, v, sc: _online(q, k, v, sc, "l"), lambda tq, tk, sc: tk > 32),
    ("scale not applied", v_no_scale, lambda tq, tk, sc: sc and tk > 1),
    ("last query row computed from row t_q - 2", v_last_row, lambda tq, tk, sc: tq > 1 and tk > 1),
]


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_rows_cover_every_attention_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith("attn.")}   # every other name: tests/test_f32_routes.py
    used = {lvl for row in TABLE for lvl in row["route"].split("/")}
    assert not (used | NOT_REACHABLE) - mine, "routes the library cannot report: %s" % sorted((used | NOT_REACHABLE) - mine)
    assert not used & NOT_REACHABLE
    assert not mine - used - NOT_REACHABLE, "routes no row reaches: %s" % sorted(mine - used - NOT_REACHABLE)
    # every kernel with classes is paired with each class it is listed for: the 16- and 32-row kernels with all eight
    for kern in ("attn.rows16", "attn.rows32"):
        assert {r["route"] for r in TABLE if r["route"].startswith(kern + "/")} == {"%s/attn.nt%d" % (kern, 2 * c) for c in range(1, 9)}


def test_rows_satisfy_the_dispatch_conditions_they_state():
    """the dispatch of lele_hip_attention_view restated for 256 CUs: every dense row names the route it computes"""
    cus = 256
    for row in TABLE:
        if row["route"].startswith("attn.seg"):
            assert all(H * -(-n // 32) < cus // 2 for n in SEG_LENGTHS)   # every segment on the 16-row kernel
            continue
        fb, tq, tk = H * row["b"], row["tq"], row["tk"]
        rows16 = fb * -(-tq // 32) < cus // 2
        flash = not row["exact"] and not rows16 and fb * -(-tq // 128) >= cus // 2
        two = fb * -(-tq // 64) >= 3 * cus
        want = "attn.flash" if flash else "attn.rows%d%s/%s" % (16 if rows16 else 64 if two else 32, "_exact" if row["exact"] else "", _nt(tk))
        assert want == row["route"], row
        assert (tq != tk) or (row["b"], tq) == (32, 171)


def test_oracle_composition_within_a_quarter_of_the_bound(orc):
    """the measurement behind C_BOUND (printed per family), and the assertion that the oracle's f32 composition keeps four times clear of it"""
    ratios, done = {}, set()
    for row in TABLE:
        for fam in families_of(row):
            for n, tq, tk in shapes_of(row):
                if (fam, n, tq, tk, row["scaled"]) in done:   # rows of several routes share a shape
                    continue
                done.add((fam, n, tq, tk, row["scaled"]))
                inp = case(fam, n, tq, tk, row["scaled"])
                inp = {k: v[:1] if isinstance(v, np.ndarray) and v.ndim == 4 else v for k, v in inp.items()}   # the first batch element: the oracle's GEMM is slow
                s = orc.matmul(inp["q"], np.ascontiguousarray(inp["k"].transpose(0, 1, 3, 2)))
                if inp["scale"] is not None:
                    s = s * inp["scale"]
                o = orc.matmul(orc.softmax(s, -1), inp["v"])
                ratios[fam] = max(ratios.get(fam, 0.0), worst(o, inp))
    print("oracle composition / bound(C_BOUND = 1): " + "   ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= C_BOUND / 4, ratios


def test_bound_is_never_looser_than_the_project_bar_on_moderate_inputs():
    """condition (a): on `random` and the ramps, bound <= 1e-4 (|o| + rms(o)) at every element"""
    for row in TABLE:
        for fam in families_of(row):
            if fam not in MODERATE:
                continue
            for n, tq, tk in shapes_of(row):
                inp = case(fam, n, tq, tk, row["scaled"])
                o = inp["o"]
                bar = 1e-4 * (np.abs(o) + np.sqrt(np.mean(np.square(o))))
                loose = C_BOUND * inp["bound1"] > bar
                assert not loose.any(), "%s %s: bound up to %.3g of the 1e-4 bar" % (row, fam, float(np.max(C_BOUND * inp["bound1"] / bar)))


@pytest.mark.parametrize("i", range(len(TABLE)), ids=ROW_IDS)
def test_tolerance_rejects_wrong_variants(i):
    row = TABLE[i]
    for n, tq, tk in shapes_of(row):
        seen = {name: False for name, _, applies in VARIANTS if applies(tq, tk, row["scaled"])}
        if tk > 32 and tk % 64 and tq > 1 and row["scaled"]:
            assert len(seen) == len(VARIANTS)
        for fam in families_of(row):
            inp = case(fam, n, tq, tk, row["scaled"])
            q, k, v, sc = inp["q"], inp["k"], inp["v"], inp["scale"]
            assert not outside(inp["o"].astype(np.float32), inp, 1).any(), "the reference itself, rounded to f32, fails the bound"
            assert not outside(_softmax_pv(_scores(q, k, sc), v), inp, 1).any(), "numpy's f32 composition fails the bound (%s)" % fam
            for name, emul, _ in VARIANTS:
                if name in seen and not seen[name]:
                    seen[name] = bool(outside(emul(q, k, v, sc), inp, 4).any())
        missed = [name for name, hit in seen.items() if not hit]
        assert not missed, "t_q %d, t_k %d: no family tells %s from the operation" % (tq, tk, missed)


# -------------------------------------------------------------------------------------------------------------------- GPU
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


def merged(a):
    """[n, H, t, DH] -> [n, t, H * DH], the layout the projections write and read"""
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(a.shape[0], a.shape[2], H * DH)


def heads(a):
    """[.., t, H * DH] -> [.., H, t, DH]"""
    return a.reshape(a.shape[:-1] + (H, DH)).swapaxes(-2, -3)


def scale_operand(sc):
    from lele_amd._lib import Weight
    return None if sc is None else Weight(np.array([sc], np.float32))


def run_dense(ctx, row, q, k, v, sc, out_perm=(0, 2, 1, 3), out_reshape=(0, 0, H * DH)):
    """the library's result for the row's batch (the n distinct elements repeated), Q in its own buffer, K | V column slices of a second;
    returns (device result, route)"""
    from lele_amd import kernels as K
    rep = np.arange(row["b"]) % q.shape[0]
    qd = ctx.buf().upload(merged(q)[rep])
    kvd = ctx.buf().upload(np.concatenate([merged(k), merged(v)], -1)[rep])
    with _env(LELE_HIP_ATTENTION_MIN_BLOCKS=1, LELE_HIP_ATTENTION_EXACT=row["exact"]):
        got = K.attention_view(qd, QC, kvd, KC, kvd, VC, scale_operand(sc), None if out_perm is None else list(out_perm),
                               None if out_reshape is None else list(out_reshape), ctx=ctx)
    return got, K.last_route(ctx)


def check(got, inp, what):
    """got [b, H, tq, DH] (the n distinct elements of the case repeated) against the reference, element by element: finite and inside
    the bound; returns the worst |got - ref| / bound"""
    n = inp["o"].shape[0]
    rep = np.arange(got.shape[0]) % n
    assert np.isfinite(got).all(), "%s: %d results are NaN or infinite" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got.astype(np.float64) - inp["o"][rep])
    lim = C_BOUND * inp["bound1"][rep]
    bad = ~(err <= lim)
    if bad.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            at = np.unravel_index(int(np.argmax(np.where(bad, err / lim, 0))), err.shape)
        raise AssertionError("%s: %d of %d outside the bound; worst at %s: got %r want %r bound %.3g (%.1f x)" % (
            what, int(bad.sum()), bad.size, at, got[at], inp["o"][rep][at], lim[at], err[at] / lim[at]))
    return float(np.max(np.where(err == 0, 0.0, err / np.where(lim == 0, 1.0, lim))))


def run_segments(ctx, row, fam, key):
    """the packed layout of SEG_LENGTHS: (per-segment results [1, H, len, DH], route); key picks each segment's (q, k) pair"""
    from lele_amd import kernels as K
    cases = [case(fam, 1, n, n, row["scaled"]) if n else None for n in SEG_LENGTHS]
    parts = []
    for c in cases:
        if c is not None:
            q, k = key(c)
            parts.append(np.concatenate([merged(q)[0], merged(k)[0], merged(c["v"])[0]], -1))
    off = np.concatenate([[0], np.cumsum(SEG_LENGTHS)])
    sc = next(c for c in cases if c is not None)["scale"]
    with _env(LELE_HIP_ATTENTION_EXACT=row["exact"]):
        got = K.attention_segments(ctx.buf().upload(np.concatenate(parts, 0)), [int(x) for x in off], H, DH, scale=scale_operand(sc), ctx=ctx).numpy()
    assert got.shape == (int(off[-1]), H * DH)
    return [(c, heads(got[off[j]:off[j + 1]])[None]) for j, c in enumerate(cases) if c is not None], K.last_route(ctx)


def check_family(fam, inp, got, got0, what):
    """check, and the family's own property: two_peak -- the mean of the two V rows (the float64 reference to exp(-100)); shift -- the
    same call with the offset removed (got0), under the same bound.  Returns the worst |got - ref| / bound"""
    ratio = check(got, inp, what)
    rep = np.arange(got.shape[0]) % inp["o"].shape[0]
    lim = C_BOUND * inp["bound1"][rep]
    if fam == "two_peak":
        bad = ~(np.abs(got - inp["mean"][rep]) <= lim)
        assert not bad.any(), "%s: %d results are not the mean of the two peaks' V rows" % (what, int(bad.sum()))
    if fam.startswith("shift"):
        diff = np.abs(got.astype(np.float64) - got0)
        bad = ~(diff <= lim)
        assert not bad.any(), "%s: %d results differ from the unshifted call's by more than the bound (worst %.3g x)" % (
            what, int(bad.sum()), float(np.max(diff / lim)))
    return ratio


def run_family(ctx, row, fam):
    """one family through the row's route: the worst |got - ref| / bound over its problems"""
    from lele_amd import kernels as K
    shifted = fam.startswith("shift")
    if row["route"].startswith("attn.seg"):
        res, route = run_segments(ctx, row, fam, lambda c: (c["q"], c["k"]))
        assert route == row["route"], "route moved: the library ran %s, the row covers %s" % (route, row["route"])
        plain = run_segments(ctx, row, fam, lambda c: c["unshifted"])[0] if shifted else [(None, None)] * len(res)
        return max(check_family(fam, inp, got, got0, "segment of %d rows" % got.shape[2]) for (inp, got), (_, got0) in zip(res, plain))
    n, tq, tk = shapes_of(row)[0]
    inp = case(fam, n, tq, tk, row["scaled"])
    dev, route = run_dense(ctx, row, inp["q"], inp["k"], inp["v"], inp["scale"])
    assert route == row["route"], "route moved: the library ran %s, the row covers %s" % (route, row["route"])
    assert set(route.split("/")) <= set(K.route_names())
    assert dev.shape == (row["b"], tq, H * DH)
    got0 = None
    if shifted:
        dev0, route0 = run_dense(ctx, row, inp["unshifted"][0], inp["unshifted"][1], inp["v"], inp["scale"])
        assert route0 == route
        got0 = heads(dev0.numpy())
    return check_family(fam, inp, heads(dev.numpy()), got0, "t_q %d, t_k %d" % (tq, tk))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TABLE)), ids=ROW_IDS)
def test_route_values(ctx, i):
    row = TABLE[i]
    ratios, failures = [], []
    for fam in families_of(row):   # every family runs, so a failure names all the families that see it
        try:
            ratios.append("%s %.2f" % (fam, run_family(ctx, row, fam)))
        except AssertionError as e:
            failures.append("%s: %s" % (fam, e))
    print("%s: worst |got - f64| / bound  %s" % (ROW_IDS[i], "  ".join(ratios)))
    assert not failures, "\n".join(failures)


def _row(route, **kw):
    for r in TABLE:
        if r["route"].startswith(route) and all(r[k] == v for k, v in kw.items()):
            return r
    raise KeyError(route)


# one row per kernel: 16 rows (class 8, 40 of 48 rows live in the last blocks), 32 rows, the one-pass kernel, an f32 replica
KERNEL_ROWS = [_row("attn.rows16/", tq=40, tk=449), _row("attn.rows32/", tq=33, tk=171), _row("attn.flash", tq=97, tk=100, scaled=True),
               _row("attn.rows32_exact/", tk=129)]
KERNEL_IDS = [row_id(TABLE.index(r), r) for r in KERNEL_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("row", KERNEL_ROWS, ids=KERNEL_IDS)
def test_poisoned_neighbours(ctx, row):
    """the operands as row and column slices of parents that are NaN everywhere else -- the rows before a batch element's first
    query / key and after its last, the pitch gaps left and right: no NaN in the result, and the bits of the call on tight copies"""
    from lele_amd import kernels as K
    b, tq, tk = row["b"], row["tq"], row["tk"]
    n = min(b, 3)
    inp = case("random", n, tq, tk, True)
    rep = np.arange(b) % n
    g, pad_q, pad_kv = 3, 4, 8   # guard rows; pitch gaps (multiples of 4 floats: the fused path needs 16-byte aligned rows)
    qp = np.full((b, g + tq + g, pad_q + H * DH + pad_q), np.nan, np.float32)
    qp[:, g:g + tq, pad_q:pad_q + H * DH] = merged(inp["q"])[rep]
    kvp = np.full((b, g + tk + g, pad_kv + 2 * H * DH + pad_kv), np.nan, np.float32)
    kvp[:, g:g + tk, pad_kv:pad_kv + H * DH] = merged(inp["k"])[rep]
    kvp[:, g:g + tk, pad_kv + H * DH:pad_kv + 2 * H * DH] = merged(inp["v"])[rep]
    qc = [["slice", 1, g, tq], ["slice", 2, pad_q, H * DH]] + QC
    kc = [["slice", 1, g, tk], ["slice", 2, pad_kv, H * DH]] + KC[1:]
    vc = [["slice", 1, g, tk], ["slice", 2, pad_kv + H * DH, H * DH]] + VC[1:]
    for chain, shape in ((qc, qp.shape), (kc, kvp.shape), (vc, kvp.shape)):
        _, st, off = K._walk_chain(list(shape), chain)
        assert off % 4 == 0 and all(s % 4 == 0 for s in st if s != 1), (st, off)
    qd, kvd = ctx.buf().upload(qp), ctx.buf().upload(kvp)
    with _env(LELE_HIP_ATTENTION_MIN_BLOCKS=1, LELE_HIP_ATTENTION_EXACT=row["exact"]):
        got = K.attention_view(qd, qc, kvd, kc, kvd, vc, scale_operand(inp["scale"]), [0, 2, 1, 3], [0, 0, H * DH], ctx=ctx).numpy()
    assert K.last_route(ctx) == row["route"]
    assert not np.isnan(got).any(), "%d results are NaN: the kernel read outside its views" % int(np.isnan(got).sum())
    tight, route = run_dense(ctx, row, inp["q"], inp["k"], inp["v"], inp["scale"])
    assert route == row["route"]
    assert np.array_equal(got, tight.numpy()), "views of padded parents and tight copies give different bits"
    check(heads(got), inp, "poisoned parents")


# the statistics a call leaves for the output projection, after t_q != t_k calls on each kernel and after the one-pass row whose last
# workgroup of a head has one live row
STAT_ROWS = [_row("attn.rows16/", tq=40, tk=193, scaled=True), _row("attn.rows32/", tq=40, tk=129), _row("attn.flash", tq=97, tk=100, scaled=True),
             _row("attn.flash", tq=129, tk=171)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", STAT_ROWS, ids=[row_id(TABLE.index(r), r) for r in STAT_ROWS])
def test_statistics_feed_the_output_projection(ctx, orc, row):
    """fused_quantized_linear of the result (its range from the {min, max} pairs the kernel left) == the oracle on a host copy"""
    from lele_amd import kernels as K
    from lele_amd._lib import Weight
    rng = np.random.default_rng(17)
    w = (Weight(np.clip(np.round(128 + 32 * rng.standard_normal((512, 512))), 0, 255).astype(np.float32)),
         Weight((np.abs(rng.standard_normal(512)) * 0.01 + 0.002).astype(np.float32)), Weight(np.array([128.0], np.float32)),
         Weight((rng.standard_normal(512) * 0.02).astype(np.float32)))
    n, tq, tk = shapes_of(row)[0]
    inp = case("random", n, tq, tk, True)
    av, route = run_dense(ctx, row, inp["q"], inp["k"], inp["v"], inp["scale"])
    assert route == row["route"]
    got = K.fused_quantized_linear(av, *w, False, ctx=ctx).numpy()
    want = orc.fused_quantized_linear(av.numpy(), w[0].arr, w[1].arr, [128.0], w[3].arr, False)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("row", KERNEL_ROWS, ids=KERNEL_IDS)
def test_output_without_out_perm(ctx, row):
    """[b, H, t_q, 128] (no out_perm, no statistics): the bits of the merged form, transposed on the host"""
    n, tq, tk = shapes_of(row)[0]
    inp = case("random", n, tq, tk, True)
    plain, route = run_dense(ctx, row, inp["q"], inp["k"], inp["v"], inp["scale"], out_perm=None, out_reshape=None)
    assert route == row["route"] and plain.shape == (row["b"], H, tq, DH)
    mrg, route = run_dense(ctx, row, inp["q"], inp["k"], inp["v"], inp["scale"])
    assert route == row["route"]
    assert np.array_equal(plain.numpy(), heads(mrg.numpy()))
