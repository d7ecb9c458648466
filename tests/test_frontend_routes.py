"""Every kernel route of the audio front-end, named by the library and held to the contract of frontend.hip's header.

The contract: the power spectrum and the mel sums are the reference's bit for bit, only `ln` may differ, by at most 2 ulp.  The oracle hands
out the f32 mel sums themselves (`frontend_compute(..., return_energy=True)`), so the bar is stated on them, per log-mel cell:

    truth = float64 ln(max(E_oracle, 1e-5f))        |device - truth| <= 2 * ulp32(max(|truth|, 1))

For |truth| >= 1 this is the 2 ulp of the contract; below 1 the bound stays at 2^-22 absolute (an error d in ln is a relative error d of
the energy, and the contract promises the energy no finer than that).  Floor cells (E <= 1e-5f) are cells like any other: their truth is
ln(1e-5f).  The LFR features are compared with the gather (lfr.rs: left pad (m - 1) / 2, indices clamped) of the same front-end's log-mel
rows by array_equal.

`ROWS` names, for every row, the config, the entry point, the lengths, the input family and the route the library must report
(`kernels.last_route`): the kernel (`fe.main_std`, `fe.main_table`, `fe.seg_std`, `fe.seg_table`, `fe.generic_fused`, `fe.generic_four`)
and, for the main and segment kernels, how the PCM tile was staged (`fe.tile_dma`, `fe.tile_regs`, `fe.tile_mixed`).  A row that lands
on another route fails before its numbers are looked at; `route_of` restates the dispatch conditions and is checked against the table
without a GPU.  The CPU half also checks the condition each input family states on the oracle, that the oracle's energies are exactly
what its log-mel is the logf of, and that the bar has teeth: models built from oracle pieces that are accurate but not the reference
(a float64 pipeline, energies off by 2^-18, a shifted LFR pad) fail it.

Worst |device - truth| per route, measured on an MI355X: profiles/frontend_routes.json (tools/frontend_routes_profile.py)."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import synth_pcm

PREFIXES = ("fe.",)
# what no row asserts, and why (a key that is a route name takes that name out of the coverage requirement)
NOT_COVERED = {
    "fe.two_kernel": "lab only: LELE_HIP_FE_FUSED=0 is read by the lab library alone (tests/test_frontend_gpu.py::test_kernel_variants_are_identical)",
    "n_fft = 2048 / 4096": "frontend_create derives n_fft from the frame (512 up to 400 samples, 1024 beyond) and refuses a frame longer than "
                           "its n_fft, so no FeatureConfig reaches the one-frame-a-workgroup form of the fused generic kernel",
    "LELE_HIP_FE_DPP=0 / LELE_HIP_FE_GENERIC_MEL=1": "lab only: the __shfl neighbour exchange and the forced table-driven mel loop; the table-driven "
                                                     "kernel itself is reached here by every n_mels other than 80",
}

F32, F64 = np.float32, np.float64
FLOOR = F32(1e-5)
DEFAULT = (16000, 80, 25.0, 10.0, 7, 6)   # sample_rate, n_mels, frame_length_ms, frame_shift_ms, lfr_m, lfr_n
FAMILIES = ("synth", "tone", "nyquist", "impulse", "tiny", "ramp", "wide")
FAMILY_LEN = 10640   # the length the family conditions are stated at (65 frames of the default framing)
MAX_GRID_Y = 65535


# --------------------------------------------------------------------------------------------------------------------- inputs
def family(name, n, seed=0):
    """PCM of family `name`, n samples.  What each is for, as conditions on the oracle: test_families_meet_their_conditions"""
    i = np.arange(n)
    if name == "synth":      # the suite's standard input: two tones and noise
        return synth_pcm(n, seed)
    if name == "tone":       # a pure tone: most filters hold leakage only, a tenth of the cells have |ln E| < 1 (the clamp of the bar)
        return (0.3 * np.sin(2 * np.pi * 1000 * i / 16000.0)).astype(F32)
    if name == "nyquist":    # all the energy in the last bin
        return (0.25 * (1 - 2 * (i % 2))).astype(F32)
    if name == "impulse":    # one nonzero sample every 977: frames of zeros (E == 0, the floor) between frames with a flat spectrum
        x = np.zeros(n, F32)
        x[(seed * 131) % 977::977] = 0.5
        return x
    if name == "tiny":       # mel energies on both sides of the 1e-5 floor
        return (synth_pcm(n, seed) * F32(3e-7)).astype(F32)
    if name == "ramp":       # eight decades of amplitude in one utterance
        return (synth_pcm(n, seed).astype(F64) * np.logspace(-8, 0, n)).astype(F32)
    if name == "wide":       # subnormal samples to 3e4, by the frame and sample by sample (tests/test_frontend_tile_dma.py)
        from test_frontend_tile_dma import chain_inputs
        return np.roll(np.resize(chain_inputs()["wide"], n), 160 * seed)
    raise KeyError(name)


# --------------------------------------------------------------------------------------------------------------------- the bar
def ulp32(v):
    """spacing of f32 at the (float64, positive) magnitude v"""
    return 2.0 ** (np.floor(np.log2(v)) - 23)


def truth_of(energy):
    return np.log(np.maximum(energy, FLOOR).astype(F64))


def ulps(d, truth):
    """|d - truth| in units of ulp32(max(|truth|, 1)); the bar is 2"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(d, F32).astype(F64) - truth) / ulp32(np.maximum(np.abs(truth), 1.0))


def meets(d, truth):
    d = np.asarray(d)
    return d.shape == truth.shape and bool(np.all(ulps(d, truth) <= 2.0))   # (a NaN compares false)


def meets_old(d, ref):
    """the 1e-4 bar of tests/test_frontend_gpu.py"""
    return d.shape == ref.shape and bool(np.all(np.abs(d - ref) <= 1e-4 * np.abs(ref) + 1e-6))


def lfr_index(nf, m, n, pad=None):
    """[t_lfr, m] frame indices of lfr.rs:18-54"""
    pad = (m - 1) // 2 if pad is None else pad
    t = (nf + n - 1) // n
    return np.clip(np.arange(t)[:, None] * n + np.arange(m)[None, :] - pad, 0, nf - 1)


def gather(rows, m, n, pad=None):
    idx = lfr_index(rows.shape[0], m, n, pad)
    return rows[idx].reshape(idx.shape[0], m * rows.shape[1])


# --------------------------------------------------------------------------------------------------------------------- the dispatch, restated
def framing(cfg):
    sr, nm, fl, fs, m, n = cfg
    frame_len = int(F32(sr) * F32(fl) / F32(1000.0))   # pipeline.rs:39, in f32
    hop = int(F32(sr) * F32(fs) / F32(1000.0))
    return frame_len, hop, (1024 if frame_len > 400 else 512)


def frames_of(cfg, n):
    frame_len, hop, _ = framing(cfg)
    return 0 if n < frame_len else (n - frame_len) // hop + 1


def is_fast(cfg):
    return framing(cfg) == (400, 160, 512) and cfg[1] <= 128


def frames_per_workgroup(cfg):
    n_fft = framing(cfg)[2]
    return 64 if is_fast(cfg) else 4 if n_fft <= 512 else 2 if n_fft <= 1024 else 1


def route_of(row):
    """the route frontend.hip reports for `row`, from the conditions its launch sites test (buffers start 16-byte aligned)"""
    cfg = row["cfg"]
    lengths = row["lengths"]
    if row["entry"] == "segments":
        starts = np.cumsum([row["lead"]] + list(lengths))[:-1]
        live = [(s, ln) for s, ln in zip(starts, lengths) if frames_of(cfg, ln)]
        if not live:
            return ""
        if not is_fast(cfg):
            return "fe.generic_fused"
        dma = [s % 4 == 0 and ln % 4 == 0 and not row["forced_regs"] for s, ln in live]
        return ("fe.seg_std" if cfg[1] == 80 else "fe.seg_table") + "/" + ("fe.tile_dma" if all(dma) else "fe.tile_mixed" if any(dma) else "fe.tile_regs")
    n = lengths[0]
    assert all(ln == n for ln in lengths)
    if frames_of(cfg, n) == 0 or row["batch"] == 0:
        return ""
    if not is_fast(cfg):
        return "fe.generic_fused" if row["batch"] <= MAX_GRID_Y else "fe.generic_four"
    return ("fe.main_std" if cfg[1] == 80 else "fe.main_table") + "/" + ("fe.tile_dma" if n % 4 == 0 and not row["forced_regs"] else "fe.tile_regs")


# --------------------------------------------------------------------------------------------------------------------- the table
ROWS = []


def add(route, cfg, entry, lengths, fam, why, lead=0, forced_regs=False, batch=None):
    lengths = tuple(lengths)
    batch = len(lengths) if batch is None else batch
    rid = "%s-%s-%s-%s-%s%s%s" % (route.replace("fe.", "").replace("/", "+") or "none", "x".join(str(v) for v in cfg), entry,
                                  "_".join(str(v) for v in lengths), fam, "-lead%d" % lead if entry == "segments" else "", "-regs" if forced_regs else "")
    if any(r["id"] == rid for r in ROWS):   # (a case two groups share is one row)
        return
    ROWS.append(dict(id=rid, route=route, cfg=tuple(cfg), entry=entry, lengths=lengths, family=fam, why=why, lead=lead, forced_regs=forced_regs,
                     batch=batch))


def cfg_of(sr=16000, nm=80, fl=25.0, fs=10.0, m=7, n=6):
    return (sr, nm, fl, fs, m, n)


def tile(n):
    return "fe.tile_dma" if n % 4 == 0 else "fe.tile_regs"


# the default config: one frame; exactly 64 frames with pcm_len % 4 zero (10480, 10484) and not (10482); 65 frames = a second workgroup of
# one frame, aligned and not (10640, 10641); 129 frames = three workgroups
for _n in (400, 10480, 10482, 10484, 10640, 10641, 20960):
    for _f in FAMILIES:
        add("fe.main_std/" + tile(_n), DEFAULT, "compute", (_n,), _f, "default config, %d frames" % frames_of(DEFAULT, _n))
# aligned runs through the registers: the product switch LELE_HIP_FE_TILE_DMA=0
for _n in (10480, 20960):
    for _f in ("synth", "wide"):
        add("fe.main_std/fe.tile_regs", DEFAULT, "compute", (_n,), _f, "aligned, register staging by the switch", forced_regs=True)
# the table-driven mel loop: 23 (a partial round), 40, 96, 128 mels (all eight rounds)
for _nm in (23, 40, 96, 128):
    for _n in (10640, 10641):
        for _f in FAMILIES:
            add("fe.main_table/" + tile(_n), cfg_of(nm=_nm), "compute", (_n,), _f, "%d mels: %d rounds" % (_nm, (_nm + 15) // 16))
# LFR settings with both clamps live (m > 1: the left pad; n not dividing the frame count: the right), one frame included
for _m, _l in ((7, 6), (5, 3), (1, 1), (4, 7)):
    for _nm in (80, 40):
        for _n in (400, 10640):
            add(("fe.main_std/" if _nm == 80 else "fe.main_table/") + tile(_n), cfg_of(nm=_nm, m=_m, n=_l), "compute", (_n,), "synth", "lfr %d / %d" % (_m, _l))
# a batch whose utterances touch (the halo of one ends in the next): every utterance of it is a cell-by-cell row of its own
for _nm in (80, 40):
    for _n in (10640, 10482):
        add(("fe.main_std/" if _nm == 80 else "fe.main_table/") + tile(_n), cfg_of(nm=_nm), "batch", (_n,) * 3, "wide", "three utterances a launch")
# segments of one buffer: three utterances behind 0, 1 and 3 leading samples -- every segment aligned, none, and both kinds in one launch
# (behind 3 samples the first, of 10641, ends where the second starts 16-byte aligned); a segment too short for a frame between them
for _nm in (80, 40):
    _k = "fe.seg_std/" if _nm == 80 else "fe.seg_table/"
    for _f in ("synth", "wide", "tiny"):
        add(_k + "fe.tile_dma", cfg_of(nm=_nm), "segments", (10640, 4000, 20960), _f, "every segment aligned", lead=0)
        add(_k + "fe.tile_regs", cfg_of(nm=_nm), "segments", (10640, 4000, 20960), _f, "no segment aligned", lead=1)
        add(_k + "fe.tile_mixed", cfg_of(nm=_nm), "segments", (10641, 10640, 4000), _f, "unaligned, then two aligned", lead=3)
    add(_k + "fe.tile_mixed", cfg_of(nm=_nm), "segments", (10640, 396, 10642, 10640), "synth", "a frameless segment; aligned, unaligned (length), unaligned (start)", lead=0)
    add(_k + "fe.tile_regs", cfg_of(nm=_nm), "segments", (10640, 20960), "synth", "aligned segments, register staging by the switch", lead=0, forced_regs=True)
# every other framing: the fused generic kernel, 4 frames a workgroup at n_fft 512 and 2 at 1024; 8 frames fill workgroups, 7 do not
GENERIC = (cfg_of(8000, 80), cfg_of(22050, 80), cfg_of(32000, 64), cfg_of(16000, 40, 20.0, 8.0), cfg_of(16000, 80, 32.0, 16.0), cfg_of(40000, 128))
for _c in GENERIC:
    _fl, _hop, _ = framing(_c)
    for _k in (8, 7):
        for _f in ("synth", "tiny", "wide"):
            add("fe.generic_fused", _c, "compute", (_fl + (_k - 1) * _hop + 3,), _f, "%d frames, %d a workgroup" % (_k, frames_per_workgroup(_c)))
    add("fe.generic_fused", _c, "batch", (_fl + 6 * _hop,) * 3, "ramp", "three utterances, 7 frames each")
add("fe.generic_fused", GENERIC[0], "segments", (1003, 150, 2000), "synth", "the generic kernels once a segment", lead=1)
add("fe.generic_fused", GENERIC[4], "segments", (5000, 9001), "wide", "the generic kernels once a segment", lead=0)
# nothing to launch
add("", DEFAULT, "compute", (399,), "synth", "shorter than a frame")
add("", GENERIC[0], "compute", (199,), "synth", "shorter than a frame")
add("", DEFAULT, "segments", (399, 10), "synth", "no segment holds a frame", lead=0)

# the launches past the grid's 65535 rows (their own tests below: 65536 utterances each)
BIG_GENERIC = cfg_of(8000, 23, 25.0, 10.0, 1, 1)
BIG_ROWS = [
    dict(id="generic_four", route="fe.generic_four", cfg=BIG_GENERIC, entry="batch", lengths=(200,) * (MAX_GRID_Y + 1), batch=MAX_GRID_Y + 1, forced_regs=False,
         why="one-frame utterances at 8 kHz: two passes of 65535 + 1 through the four kernels"),
    dict(id="generic_fused_65535", route="fe.generic_fused", cfg=BIG_GENERIC, entry="batch", lengths=(200,) * MAX_GRID_Y, batch=MAX_GRID_Y, forced_regs=False,
         why="one utterance fewer: the fused kernel"),
    dict(id="main_chunks", route="fe.main_std/fe.tile_dma", cfg=DEFAULT, entry="batch", lengths=(400,) * (MAX_GRID_Y + 1), batch=MAX_GRID_Y + 1, forced_regs=False,
         why="the fast kernel in two launches of 65535 + 1 utterances"),
]
BIG_PROBES = (0, 1, MAX_GRID_Y - 1, MAX_GRID_Y)


def all_routes():
    return {lvl for r in ROWS + BIG_ROWS for lvl in r["route"].split("/") if lvl}


# --------------------------------------------------------------------------------------------------------------------- the oracle, once a case
@functools.lru_cache(maxsize=None)
def case(cfg, fam, n, seed):
    """-> (pcm, LFR features, log-mel, energy, truth) of the oracle; truth is None for an input shorter than a frame"""
    from oracle import pyoracle as O
    sr, nm, fl, fs, m, l = cfg
    x = family(fam, n, seed)
    out, mel, energy = O.frontend_compute(x, sr, nm, fl, fs, m, l, return_energy=True)
    for a in (x, out, mel, energy):
        a.setflags(write=False)
    if mel.size == 0:
        return x, out, mel, energy, None
    return x, out, mel, energy, truth_of(energy)


def cases_of(row):
    return [case(row["cfg"], row["family"], n, i) for i, n in enumerate(row["lengths"])]


# --------------------------------------------------------------------------------------------------------------------- CPU
def test_oracle_energies_are_what_its_log_mel_is_the_logf_of(orc):
    seen = set()
    for row in ROWS:
        for i, n in enumerate(row["lengths"]):
            key = (row["cfg"], row["family"], n, i)
            if key in seen:
                continue
            seen.add(key)
            x, out, mel, energy, truth = case(*key)
            assert energy.shape == mel.shape == ((frames_of(row["cfg"], n), row["cfg"][1]) if truth is not None else (0,)), key
            assert energy.dtype == F32 and np.array_equal(orc.log_compress(energy).view(np.uint32), mel.view(np.uint32)), key
            # the existing signature is untouched and gives the same bits
            o2, m2 = orc.frontend_compute(x, *row["cfg"], return_mel=True)
            assert np.array_equal(o2.view(np.uint32), out.view(np.uint32)) and np.array_equal(m2.view(np.uint32), mel.view(np.uint32)), key
            if truth is not None:   # the oracle's own logf meets the bar everywhere (it is correctly rounded or nearly: within 1 ulp), and
                assert meets(mel, truth), (key, float(ulps(mel, truth).max()))   # its LFR is the gather of its rows
                assert np.array_equal(out, gather(mel, row["cfg"][4], row["cfg"][5])), key
    assert len({k[0] for k in seen}) == len({r["cfg"] for r in ROWS}) >= 17


def test_rows_cover_every_front_end_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}
    assert len(mine) == 10
    used = all_routes()
    named = set(NOT_COVERED) & set(names)
    assert not (used | named) - mine, "routes the library cannot report: %s" % sorted((used | named) - mine)
    assert not used & named
    assert mine - used == named, "routes no row reaches: %s" % sorted(mine - used - named)
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_COVERED.values())
    # every fast kernel with every staging it can have; every entry point on the fast and on the generic side
    got = {r["route"] for r in ROWS}
    assert {"fe.%s/fe.tile_%s" % (k, t) for k in ("main_std", "main_table") for t in ("dma", "regs")} <= got
    assert {"fe.%s/fe.tile_%s" % (k, t) for k in ("seg_std", "seg_table") for t in ("dma", "regs", "mixed")} <= got
    assert {(r["entry"], is_fast(r["cfg"])) for r in ROWS} == {(e, f) for e in ("compute", "batch", "segments") for f in (True, False)}
    assert len({r["id"] for r in ROWS}) == len(ROWS)


def test_other_route_tables_count_what_they_counted():
    """the fe. names are nobody else's: the prefix counts the other route tables assert are those of the names without them"""
    from lele_amd import kernels as K
    import test_conv_integer_routes as ci
    import test_eltwise_routes as el
    import test_manip_routes as mp
    import test_rnn_routes as rn
    names = K.route_names()
    others = [s for s in names if not s.startswith(PREFIXES)]
    for mod, count in ((el, 30), (rn, 11), (ci, 8)):
        assert sum(s.startswith(mod.PREFIXES) for s in names) == sum(s.startswith(mod.PREFIXES) for s in others) == count
    assert sum(s.startswith(mp.PREFIXES) for s in names) == sum(s.startswith(mp.PREFIXES) for s in others)
    assert sum(s.startswith("attn.") for s in names) == 17 and not any(p.startswith("fe") for m in (el, rn, ci, mp) for p in m.PREFIXES)


def test_rows_satisfy_the_dispatch_they_state():
    for r in ROWS + BIG_ROWS:
        assert route_of(r) == r["route"], r["id"]
        assert max(r["lengths"]) <= 20960                      # at most 129 frames, three workgroups of the fast kernels
    for c in GENERIC + (BIG_GENERIC,):
        assert not is_fast(c)
    assert [framing(c) for c in GENERIC] == [(200, 80, 512), (551, 220, 1024), (800, 320, 1024), (320, 128, 512), (512, 256, 1024), (1000, 400, 1024)]
    assert {frames_per_workgroup(c) for c in GENERIC} == {4, 2} and framing(BIG_GENERIC) == (200, 80, 512)
    for r in ROWS:   # the frame counts the rows were chosen for
        if r["route"] == "fe.generic_fused" and r["entry"] == "compute":
            assert frames_of(r["cfg"], r["lengths"][0]) in (7, 8)
    assert {frames_of(DEFAULT, n) for n in (400, 10480, 10482, 10484, 10640, 10641, 20960)} == {1, 64, 65, 129}
    assert [n % 4 for n in (10480, 10482, 10484, 10640, 10641, 20960)] == [0, 2, 0, 0, 1, 0]
    # the launches past the grid: 65536 utterances are two passes of the four kernels (the scratch of 65535 one-frame utterances
    # stays under its 256 MiB), and one launch more of the fast kernel
    per_utt = 4 + 512 * 4 + 257 * 4 + 23 * 4
    assert min(MAX_GRID_Y, (1 << 28) // per_utt) == MAX_GRID_Y and frames_of(BIG_GENERIC, 200) == 1 and frames_of(DEFAULT, 400) == 1
    assert 200 % 4 == 0 and 400 % 4 == 0   # every chunk of the batch starts 16-byte aligned


def test_families_meet_their_conditions():
    share = {}
    for fam in FAMILIES:
        x, out, mel, energy, truth = case(DEFAULT, fam, FAMILY_LEN, 0)
        assert np.all(np.isfinite(energy)) and np.all(energy >= 0), fam
        share[fam] = (float(np.mean(energy <= FLOOR)), float(np.mean(np.abs(truth) < 1)), float(truth.min()), float(truth.max()))
    floor = {f: s[0] for f, s in share.items()}
    assert floor["synth"] == 0 and floor["tone"] == 0 and floor["nyquist"] == 0, floor
    assert share["tone"][1] >= 0.05, share["tone"]             # the family that exercises the clamp of the bar
    assert 0.5 <= floor["impulse"] <= 0.65, floor              # (0.60: the frames between two impulses are zeros)
    assert 0.2 <= floor["tiny"] <= 0.5, floor                  # (0.37)
    assert 0 < floor["ramp"] <= 0.25 and share["ramp"][3] - share["ramp"][2] >= 30, share["ramp"]
    # wide, as tests/test_frontend_tile_dma.py records it: frames of subnormal samples alone (their energy underflows to the floor) up to
    # samples of 3e4, whose energies lie far above anything audio reaches
    assert np.count_nonzero(np.abs(case(DEFAULT, "wide", FAMILY_LEN, 0)[0][:1200]) < np.finfo(F32).tiny) == 1200
    assert 0.2 <= floor["wide"] <= 0.5 and share["wide"][3] > 45, share["wide"]
    x, out, mel, energy, truth = case(DEFAULT, "tiny", FAMILY_LEN, 0)
    assert energy[energy > FLOOR].min() < 2 * FLOOR and energy[energy <= FLOOR].max() > FLOOR / 2   # cells close to the floor on both sides


def float64_front_end(x, cfg):
    """the front-end in float64: np.fft.rfft, the oracle's window and its dense mel bank -- accurate, and nobody's roundings"""
    from oracle import pyoracle as O
    sr, nm = cfg[0], cfg[1]
    frame_len, hop, n_fft = framing(cfg)
    nf = frames_of(cfg, len(x))
    fr = np.stack([x[i * hop:i * hop + frame_len] for i in range(nf)]).astype(F64) * 32768.0
    fr = fr - fr.mean(axis=1, keepdims=True)
    fr[:, 1:] = fr[:, 1:] - 0.97 * fr[:, :-1]
    power = np.abs(np.fft.rfft(fr * O.hann_window(frame_len).astype(F64), n_fft, axis=1)) ** 2
    energy = power @ O.mel_filterbank(sr, n_fft, nm, 20.0).astype(F64).T
    return np.log(np.maximum(energy, F64(FLOOR))).astype(F32)


def test_the_bar_has_teeth(orc):
    x, out, mel, energy, truth = case(DEFAULT, "synth", FAMILY_LEN, 0)
    # accurate arithmetic that is not the reference's passes the 1e-4 bar in every cell and fails this one
    d = float64_front_end(x, DEFAULT)
    assert meets_old(d, mel) and not meets(d, truth)
    assert float(np.mean(ulps(d, truth) <= 2.0)) < 0.95 and float(ulps(d, truth).max()) > 10
    # energies off by 2^-18 (a quarter of what the 1e-4 bar allows at ln E = 10 would be 2^-12)
    d = np.log(energy.astype(F64) * (1 + 2.0 ** -18)).astype(F32)
    assert meets_old(d, mel) and not meets(d, truth)
    # the floor.  Its neighbour nextafter(1e-5f) moves ln by 9.1e-8 = 0.095 ulp of 11.5 -- the two round to the same f32, below
    # anything a bound on ln can show; the bar does see a floor that is off by 2^-18, and a missing one
    xt, _, melt, et, tt = case(DEFAULT, "tiny", FAMILY_LEN, 0)
    near = np.nextafter(FLOOR, F32(1))
    assert np.array_equal(np.log(np.maximum(et, near).astype(F64)).astype(F32), np.log(np.maximum(et, FLOOR).astype(F64)).astype(F32))
    assert not meets(np.log(np.maximum(et, FLOOR * F32(1 + 2.0 ** -18)).astype(F64)).astype(F32), tt)
    assert not meets(np.log(np.maximum(et, F32(1e-30)).astype(F64)).astype(F32), tt)
    # a left LFR pad that is off by one fails the gather
    for m, n in ((7, 6), (5, 3), (4, 7)):
        good = gather(mel, m, n)
        assert np.array_equal(good, orc.lfr(mel, m, n))
        assert not np.array_equal(gather(mel, m, n, pad=(m - 1) // 2 + 1), good) and not np.array_equal(gather(mel, m, n, pad=(m - 1) // 2 - 1), good)
    # and the oracle's own log-mel passes (every case of the table: test_oracle_energies_are_what_its_log_mel_is_the_logf_of)
    assert meets(mel, truth) and meets(melt, tt)
    # a NaN, an infinity and a missing row fail
    bad = mel.copy()
    bad[3, 5] = np.nan
    assert not meets(bad, truth) and not meets(mel[:-1], truth)
    bad[3, 5] = np.inf
    assert not meets(bad, truth)


# --------------------------------------------------------------------------------------------------------------------- GPU
class Frontends:
    """one SenseVoiceFrontend per (config, staging switch) of a context"""

    def __init__(self, ctx):
        self.ctx, self.made = ctx, {}

    def get(self, cfg, forced_regs=False):
        from lele_amd.features import FeatureConfig, SenseVoiceFrontend
        key = (cfg, forced_regs)
        if key not in self.made:
            old = os.environ.get("LELE_HIP_FE_TILE_DMA")
            if forced_regs:
                os.environ["LELE_HIP_FE_TILE_DMA"] = "0"
            try:
                self.made[key] = SenseVoiceFrontend(FeatureConfig(*cfg), ctx=self.ctx)
            finally:
                if forced_regs:
                    if old is None:
                        del os.environ["LELE_HIP_FE_TILE_DMA"]
                    else:
                        os.environ["LELE_HIP_FE_TILE_DMA"] = old
        return self.made[key]


@pytest.fixture(scope="module")
def fes(ctx):
    return Frontends(ctx)


def routed(ctx, route, call):
    """`call()` after a call of another route (a stale name would show); its result, once the library has named `route`"""
    from lele_amd import kernels as K
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)
    assert K.last_route(ctx) == "fill.words"
    got = call()
    took = K.last_route(ctx)
    assert took == route, "route moved: the library ran %r, the row covers %r" % (took, route)
    assert set(filter(None, took.split("/"))) <= set(K.route_names())
    return got


def run_row(fes, row, worst=None):
    """runs `row` on the device -> list of what failed (empty: the row holds).  worst: dict route -> largest |d - truth| in ulps seen"""
    ctx, route, cfg = fes.ctx, row["route"], row["cfg"]
    m, n = cfg[4], cfg[5]
    fe = fes.get(cfg, row["forced_regs"])
    cs = cases_of(row)
    bad = []

    def hold(d, truth, what):
        u = ulps(d, truth) if d.shape == truth.shape else np.array([np.inf])
        if worst is not None:
            worst[route] = max(worst.get(route, 0.0), float(np.max(u)))
        if not meets(d, truth):
            bad.append("%s: %d of %d cells miss the bar, worst %.2f ulp" % (what, int(np.sum(~(u <= 2.0))), u.size, float(np.nanmax(u))))

    if route == "":
        if row["entry"] == "segments":
            pcm = np.concatenate([c[0] for c in cs])
            ends = np.cumsum(row["lengths"])
            out, off = routed(ctx, "", lambda: fe.compute_segments(pcm, list(zip(ends - row["lengths"], ends))))
            assert out.shape == () and not off.any()
        else:
            assert routed(ctx, "", lambda: fe.compute(cs[0][0])).shape == ()
            assert routed(ctx, "", lambda: fe.logmel(cs[0][0])).shape == ()
        return bad
    if row["entry"] == "compute":
        x, _, _, _, truth = cs[0]
        lm = routed(ctx, route, lambda: fe.logmel(x)).numpy()
        hold(lm, truth, "logmel")
        out = routed(ctx, route, lambda: fe.compute(x)).numpy()
        if not (lm.shape == truth.shape and np.array_equal(out, gather(lm, m, n))):
            bad.append("compute is not the LFR gather of logmel's rows")
    elif row["entry"] == "batch":
        xs = np.stack([c[0] for c in cs])
        lm = routed(ctx, route, lambda: fe.logmel(xs)).numpy()
        out = routed(ctx, route, lambda: fe.compute_batch(xs)).numpy()
        for i, c in enumerate(cs):
            hold(lm[i], c[4], "logmel of utterance %d" % i)
            if not np.array_equal(out[i], gather(lm[i], m, n)):
                bad.append("utterance %d of compute_batch is not the LFR gather of logmel's rows" % i)
            if not np.array_equal(out[i], fe.compute(c[0]).numpy()):
                bad.append("utterance %d of compute_batch differs from its own compute" % i)
    else:
        pcm = np.concatenate([np.zeros(row["lead"], F32)] + [c[0] for c in cs])
        ends = row["lead"] + np.cumsum(row["lengths"])
        segs = [(int(e - ln), int(e)) for e, ln in zip(ends, row["lengths"])]
        out, off = routed(ctx, route, lambda: fe.compute_segments(pcm, segs))
        out = out.numpy()
        want = [0] + list(np.cumsum([c[1].shape[0] if c[4] is not None else 0 for c in cs]))
        assert list(off) == want, (list(off), want)
        for i, c in enumerate(cs):
            got = out[off[i]:off[i + 1]]
            if c[4] is None:
                continue
            hold(got, gather(c[4], m, n), "segment %d" % i)
            if not np.array_equal(got, fe.compute(c[0]).numpy()):
                bad.append("segment %d differs from its own compute" % i)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_row_takes_its_route_and_meets_the_bar(fes, row):
    bad = run_row(fes, row)
    assert not bad, (row["why"], bad)


def big_batch(n):
    """65536 utterances of n samples, every one different"""
    x = synth_pcm((MAX_GRID_Y + 1) * n, 5).reshape(MAX_GRID_Y + 1, n)
    x.setflags(write=False)
    return x


def run_big(fes, row, worst=None):
    from oracle import pyoracle as O
    ctx, cfg, route = fes.ctx, row["cfg"], row["route"]
    fe = fes.get(cfg)
    xs = big_batch(row["lengths"][0])[:row["batch"]]
    out = routed(ctx, route, lambda: fe.compute_batch(xs)).numpy()
    lm = routed(ctx, route, lambda: fe.logmel(xs)).numpy()
    assert out.shape == (row["batch"], 1, cfg[1] * cfg[4]) and lm.shape == (row["batch"], 1, cfg[1])
    bad = []
    for i in [p for p in BIG_PROBES if p < row["batch"]]:
        _, mel, energy = O.frontend_compute(xs[i], *cfg, return_energy=True)
        truth = truth_of(energy)
        u = ulps(lm[i], truth)
        if worst is not None:
            worst[route] = max(worst.get(route, 0.0), float(u.max()))
        if not meets(lm[i], truth):
            bad.append("utterance %d: worst %.2f ulp" % (i, float(np.nanmax(u))))
        if not (np.array_equal(out[i], fe.compute(xs[i]).numpy()) and np.array_equal(lm[i], fe.logmel(xs[i]).numpy())
                and np.array_equal(out[i], gather(lm[i], cfg[4], cfg[5]))):
            bad.append("utterance %d differs from its single call" % i)
    # no utterance was left out or written twice: the one-frame rows are all different, none is the buffer's fill
    if not (np.all(np.isfinite(lm)) and len(np.unique(lm[::257, 0, :4].view(np.uint32), axis=0)) == len(lm[::257])):
        bad.append("rows of the batch repeat or were not written")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("row", BIG_ROWS, ids=[r["id"] for r in BIG_ROWS])
def test_batches_past_the_grid_run_in_passes(fes, row):
    bad = run_big(fes, row)
    assert not bad, (row["why"], bad)


@pytest.mark.gpu
def test_cmvn_of_65536_utterances_runs_in_chunks(ctx, orc):
    from lele_amd.features import Cmvn
    x = (np.random.default_rng(9).standard_normal((MAX_GRID_Y + 1, 1, 8)) * 3 + 10).astype(F32)
    got = Cmvn(ctx=ctx).compute(x).numpy()
    assert got.shape == x.shape
    for i in BIG_PROBES:
        assert np.array_equal(got[i], Cmvn(ctx=ctx).compute(x[i]).numpy()) and np.array_equal(got[i], orc.cmvn(x[i])), i
    # (one frame an utterance: x - mean is 0 or a rounding of it, over sqrt(eps): every row finite, and the next test of more frames)
    assert np.all(np.isfinite(got))
    x = (np.random.default_rng(10).standard_normal((MAX_GRID_Y + 1, 3, 2)) * 3 + 10).astype(F32)
    got = Cmvn(ctx=ctx).compute(x).numpy()
    for i in BIG_PROBES + (12345,):
        assert np.array_equal(got[i], orc.cmvn(x[i])), i
