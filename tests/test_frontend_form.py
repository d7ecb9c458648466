"""Which fused front-end kernel runs: the form is decided once (fe::select_form, lele_amd/csrc/fe_core.h) and one dispatcher
(fe_dispatch, lele_amd/csrc/frontend.hip) turns it into the template arguments of fe_main_kernel, fe_seg_main_kernel and
fe_stream_main_kernel.

Every form gives the same bytes, so no output can tell whether the dispatcher launched the form that frontend_create selected.  The
test hook lele_hip_frontend_last_launch reports the tuple the dispatcher recorded from the constants it launched with, packed as
mode | std_mel << 1 | fused << 2 | opt << 3 (-1 before any fused launch).

CPU: select_form on all 384 combinations of its eight inputs against the rule restated here, the product forms, the hooks' views.
GPU: one frame through every entry point under every product switch; what can go wrong is the choice of kernel, not its arithmetic.
"""
import itertools

import numpy as np
import pytest

from conftest import synth_pcm
from test_frontend_conj import is_conj
from test_frontend_lean_lds import form, frames, hook, is_lean, make_fe
from test_frontend_tables import emu, ptr  # noqa: F401  (emu, a fixture: tests/emu/fe_tables_emu.cpp built with g++)

CONST_TW, LDS_MEL, LEAN_LDS, CONJ_A = 1, 2, 4, 8


def pack(mode, std, fused, opt):
    return mode | std << 1 | fused << 2 | opt << 3


def rule(std, match, const_tw, lds_tables, lean, conj, dpp, fused):
    """the selection as the fields of LeleFrontend used to hold it -> (mode, std, fused, opt, (form hook, lean hook, conj hook))"""
    opt2 = 0
    if match and const_tw and std and fused and dpp == 1:
        opt2 = CONST_TW | (LDS_MEL if lds_tables else 0)
    is_lean_ = opt2 == (CONST_TW | LDS_MEL) and lean
    is_conj_ = is_lean_ and conj
    opt = opt2 | (LEAN_LDS if is_lean_ else 0) | (CONJ_A if is_conj_ else 0)
    return 1 if dpp == 1 else 0, int(std), int(fused), opt, (opt2, int(is_lean_), int(is_conj_))


def test_select_form_is_the_rule_on_every_input(emu):
    product = {(1, s, 1, 0) for s in (0, 1)} | {(1, 1, 1, o) for o in (1, 3, 7, 15)}
    seen, cases = set(), 0
    out = np.zeros(4, np.int32)
    for std, match, ctw, lds, lean, conj, fused in itertools.product((0, 1), repeat=7):
        for dpp in (0, 1, 2):
            emu.fe_select_form(std, match, ctw, lds, lean, conj, dpp, fused, ptr(out))
            got = tuple(int(v) for v in out)
            what = (std, match, ctw, lds, lean, conj, dpp, fused)
            mode, s, f, opt, views = rule(*what)
            assert got == (mode, s, f, opt), what
            assert (got[3] & 3, got[3] >> 2 & 1, got[3] >> 3 & 1) == views, what   # kernel_form, lean_lds, conj_a
            if dpp == 1 and fused == 1:   # the lab values at their defaults: nothing but the product library's kernels
                assert got in product, what
                seen.add(got)
            cases += 1
    assert cases == 384 and seen == product


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def cfg_64_mels():
    from lele_amd.features import FeatureConfig
    return FeatureConfig(n_mels=64)


# name -> (config, switches, opt, std_mel) of the launch
SETTINGS = {
    "default": (None, {}, 15, 1),
    "conj_off": (None, dict(LELE_HIP_FE_CONJ_A="0"), 7, 1),
    "lean_off": (None, dict(LELE_HIP_FE_LEAN_LDS="0"), 3, 1),
    "lds_tables_off": (None, dict(LELE_HIP_FE_LDS_TABLES="0"), 1, 1),
    "const_tw_off": (None, dict(LELE_HIP_FE_CONST_TW="0"), 0, 1),
    # the switch counts as on here: only create's own tw_const_matches, on a table one ulp off, sends this one to opt 0
    "const_tw_mismatch": (None, dict(LELE_HIP_FE_CONST_TW="mismatch"), 0, 1),
    "other_bank": (cfg_64_mels, {}, 0, 0),
}


def last_launch(fe):
    return hook("lele_hip_frontend_last_launch", fe)


def run(fe, entry, x):
    """one entry point on x; -> number of values it returned (an input shorter than one frame gives the empty view, shape ())"""
    from lele_amd.features import FrontendStream
    if entry == "batch":
        o = fe.compute_batch(x[None, :])
    elif entry == "logmel":
        o = fe.logmel(x)
    elif entry == "segments":
        o, _ = fe.compute_segments(x, [(0, len(x))])
    else:
        st = FrontendStream(fe, 1, 400)
        try:
            o, _ = st.push([x], final=[1])
            return o.numpy().size if o.shape != () else 0
        finally:
            st.close()
    return o.numpy().size if o.shape != () else 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_every_entry_point_launches_the_selected_form(ctx, name):
    config, env, opt, std = SETTINGS[name]
    config = config() if config else None
    want = pack(1, std, 1, opt)
    assert SETTINGS["default"][2:] == (15, 1) and pack(1, 1, 1, 15) == 1 | 2 | 4 | 15 << 3
    x = synth_pcm(frames(1), 7)
    assert len(x) == 400
    shared = make_fe(ctx, config, **env)
    assert (form(shared), is_lean(shared), is_conj(shared)) == (opt & 3, opt >> 2 & 1, opt >> 3 & 1)
    for entry in ("batch", "logmel", "segments", "stream"):
        fe = make_fe(ctx, config, **env)
        assert last_launch(fe) == -1, entry                  # a fresh front-end
        assert run(fe, entry, x[:399]) == 0 and last_launch(fe) == -1, entry   # shorter than one frame: nothing is launched
        assert run(fe, entry, x) > 0, entry
        assert last_launch(fe) == want, (entry, last_launch(fe), want)
        assert run(fe, entry, x[:399]) == 0 and last_launch(fe) == want, entry   # ... and the value stays
        # the same front-end through every entry point in turn
        assert run(shared, entry, x) > 0 and last_launch(shared) == want, (entry, last_launch(shared), want)
