"""Phase A on real and conjugate values (kFeConjA, lele_amd/csrc/frontend.hip), on the device.

It changes no rounding: the conjugate form keeps half of the complex registers as (re, -im) and reads conjugated twiddles for them
(tests/test_fe_core_conj.py has the CPU proof).  So `LELE_HIP_FE_CONJ_A=0` (the pass as it was, still built) must give the same BYTES
as the default from fe_main_kernel, fe_seg_main_kernel and fe_stream_main_kernel -- on the entry points and shapes of
tests/test_frontend_lean_lds.py: 1, 63 and 64 frames, 65 frames (block 1's tile crosses the utterance's end), 130 frames (two whole
blocks and a partial third), a sample count that is no multiple of 4 (register staging), an odd-offset segment, a chunked stream,
lfr_n = 2, tones, impulses and all-zero PCM.  Hooks and routes must read as before.  The tile has one direct-to-LDS addressing
(LELE_HIP_FE_TILE_DMA=1), so there is no second one to compare.
"""
import numpy as np
import pytest

from conftest import synth_pcm
from test_frontend_lean_lds import FAMILIES as LEAN_FAMILIES
from test_frontend_lean_lds import LENGTHS, cfg_lfr2, form, frames, hook, is_lean, make_fe, run_entry, same_bytes

FAMILIES = dict(LEAN_FAMILIES, zero=lambda n, seed=0: np.zeros(n, np.float32))
# the forms a build holds, by the switch that selects them
VARIANTS = {
    "new": dict(LELE_HIP_FE_CONJ_A="1"),
    "conj_off": dict(LELE_HIP_FE_CONJ_A="0"),
}
OLD = ("conj_off",)


def is_conj(fe):
    return hook("lele_hip_frontend_conj_a", fe)


@pytest.fixture(scope="module")
def fes(ctx):
    """front-ends of every variant for the default config and for lfr_n = 2, and the plain default"""
    out = {name: {v: make_fe(ctx, cfg, **env) for v, env in VARIANTS.items()} for name, cfg in (("default", None), ("lfr2", cfg_lfr2()))}
    out["default"]["default"] = make_fe(ctx)
    return out


def compare(fes_cfg, ctx, entry, x, what, route=None):
    got, r1 = run_entry(fes_cfg["new"], ctx, entry, x)
    assert sum(a.size for a in got) > 0, what
    for old in OLD:
        want, r0 = run_entry(fes_cfg[old], ctx, entry, x)
        same_bytes(got, want, (what, old))
        assert r1 == r0, (what, old, r1, r0)
    if route is not None:
        assert r1 == route, (what, r1)
    return got, r1


@pytest.mark.gpu
def test_the_switches_select_the_forms_and_the_other_hooks_read_as_before(ctx, fes):
    for name in ("default", "lfr2"):
        f = fes[name]
        assert is_conj(f["new"]) == 1 and is_conj(f["conj_off"]) == 0, name
        for v in VARIANTS:
            assert form(f[v]) == 3 and is_lean(f[v]) == 1, (name, v)   # what both hooks reported before
    d = fes["default"]["default"]
    assert is_conj(d) == 1 and form(d) == 3 and is_lean(d) == 1   # the default takes the conjugate form
    # the conjugate form is a form of the lean constant-table pass only
    assert is_conj(make_fe(ctx, LELE_HIP_FE_CONST_TW="0")) == 0
    assert is_conj(make_fe(ctx, LELE_HIP_FE_CONST_TW="mismatch")) == 0
    assert is_conj(make_fe(ctx, LELE_HIP_FE_LDS_TABLES="0")) == 0
    off = make_fe(ctx, LELE_HIP_FE_LEAN_LDS="0")
    assert is_conj(off) == 0 and is_lean(off) == 0 and form(off) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("cfg", ["default", "lfr2"])
def test_batch_and_logmel_give_the_bytes_of_the_earlier_forms(ctx, fes, cfg, fam):
    for n in LENGTHS:
        x = FAMILIES[fam](n, n % 7)
        for entry in ("batch", "logmel"):
            compare(fes[cfg], ctx, entry, x, (cfg, fam, n, entry), "fe.main_std/fe.tile_dma")
    # a sample count that is no multiple of 4: the register-staged tile
    x = FAMILIES[fam](frames(65) + 2, 5)
    for entry in ("batch", "logmel"):
        compare(fes[cfg], ctx, entry, x, (cfg, fam, "unaligned", entry), "fe.main_std/fe.tile_regs")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("cfg", ["default", "lfr2"])
def test_segments_and_streams_give_the_bytes_of_the_earlier_forms(ctx, fes, cfg, fam):
    x = FAMILIES[fam](frames(65), 3)
    for entry, route in (("segments3", "fe.seg_std/fe.tile_mixed"), ("segments3_unaligned", "fe.seg_std/fe.tile_regs"), ("stream", None)):
        _, r = compare(fes[cfg], ctx, entry, x, (cfg, fam, entry), route)
        if route is None:
            assert all(s.startswith("fe.seg_std/fe.tile_") for s in r.split("|")), r


@pytest.mark.gpu
def test_a_batch_of_utterances_gives_the_bytes_of_the_earlier_form(ctx, fes):
    """four utterances of 130 frames in one launch: two whole blocks each and a third whose tile crosses the utterance's end"""
    n = frames(130)
    x = np.stack([synth_pcm(n, 20 + i) for i in range(4)])
    got = fes["default"]["new"].compute_batch(x).numpy()
    for old in OLD:
        assert got.tobytes() == fes["default"][old].compute_batch(x).numpy().tobytes(), old
    for i in range(4):   # and each utterance is what it is alone
        assert got[i].tobytes() == fes["default"]["new"].compute_batch(x[i][None, :]).numpy()[0].tobytes(), i


@pytest.mark.gpu
def test_new_forms_meet_the_oracle(fes, orc):
    """the comparisons above are build against build; this one ties the default to the reference restatement (the suite's bar)"""
    x = synth_pcm(frames(130), 130)
    ref = orc.frontend_compute(x)
    got = fes["default"]["default"].compute_batch(x[None, :]).numpy()[0]
    assert got.shape == ref.shape
    err = np.abs(got - ref) - (1e-4 * np.abs(ref) + 1e-6)   # RTOL, ATOL of tests/test_frontend_gpu.py
    assert np.all(err <= 0), float(err.max())
