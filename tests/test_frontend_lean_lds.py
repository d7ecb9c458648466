"""The lean pass of the default front-end kernels (kFeLeanLds, lele_amd/csrc/frontend.hip): the exchange's eight-byte LDS accesses as
single ds_write_b64 / ds_read_b64 and the next pass's sample pointer carried from pass to pass.

Neither changes an operation or an address, so `LELE_HIP_FE_LEAN_LDS=0` (today's pass loop, still built) and the default must give the
same BYTES from fe_main_kernel, fe_seg_main_kernel and fe_stream_main_kernel -- on one frame, on both sides of a 64-frame block
boundary, on a partial third block (the tail clamp of the carried pointer: lanes past the last frame read frame 0), on unaligned
segments (the register-staged tile), on a chunked stream, and with lfr_n = 2 (the division branch of the carried LFR targets).  The
kernels must also report the routes they reported before.

The issue's other lever -- phase A without its sign flips -- is not in the tree (docs/experiments.md: the compiler folds an element's
negation into an operand modifier only for a broadcast scalar), so fe_core.h is unchanged and there is no CPU comparison to make.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import synth_pcm


def frames(f):
    return 400 + 160 * (f - 1)


def impulse(n, seed=0):
    """the impulse family of tests/test_frontend_routes.py: frames of zeros between frames with a flat spectrum"""
    x = np.zeros(n, np.float32)
    x[(seed * 131) % 977::977] = 0.5
    return x


FAMILIES = {"synth": synth_pcm, "impulse": impulse}
LENGTHS = [frames(1), frames(63), frames(64), frames(65), frames(130)]   # S = 400, 400 + 160 * {62, 63, 64, 129}


def make_fe(ctx, config=None, **env):
    from lele_amd.features import SenseVoiceFrontend
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return SenseVoiceFrontend(config=config, ctx=ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def hook(name, fe):
    from lele_amd import _lib
    fn = getattr(_lib.lib(), name)
    fn.restype = C.c_int
    return fn(fe._h)


def is_lean(fe):
    return hook("lele_hip_frontend_lean_lds", fe)


def form(fe):
    return hook("lele_hip_frontend_kernel_form", fe)


def cfg_lfr2():
    from lele_amd.features import FeatureConfig
    return FeatureConfig(lfr_m=7, lfr_n=2)


@pytest.fixture(scope="module")
def pairs(ctx):
    """(lean, plain) front-ends for the default config and for lfr_n = 2"""
    return {name: (make_fe(ctx, cfg), make_fe(ctx, cfg, LELE_HIP_FE_LEAN_LDS="0")) for name, cfg in (("default", None), ("lfr2", cfg_lfr2()))}


def run_entry(fe, ctx, entry, x):
    """-> (arrays, route) of one entry point on one input"""
    from lele_amd import kernels as K
    from lele_amd.features import FrontendStream
    if entry == "batch":
        out = [fe.compute_batch(x[None, :]).numpy().copy()]
    elif entry == "logmel":
        out = [fe.logmel(x).numpy().copy()]
    elif entry == "segments3":
        # three segments of unequal lengths in one buffer, the second starting at an odd sample offset: the register-staged tile
        n = len(x)
        segs = [(0, n), (n + 1, n + 1 + frames(3)), (n + 1 + frames(3) + 3, n + 1 + frames(3) + 3 + frames(66) + 2)]
        buf = np.concatenate([x, FAMILIES["synth"](segs[2][1] - n, 9)])
        assert segs[1][0] % 2 == 1 and len({e - s for s, e in segs}) == 3
        o, off = fe.compute_segments(buf, segs)
        out = [o.numpy().copy(), np.asarray(off)]
    elif entry == "segments3_unaligned":
        segs = [(1, 1 + frames(3)), (1 + frames(3) + 2, 1 + frames(3) + 2 + frames(65) + 1), (3, 3 + frames(130))]
        buf = np.resize(x, max(e for _, e in segs))
        assert all(s % 4 for s, _ in segs) and segs[0][0] % 2 == 1
        o, off = fe.compute_segments(buf, segs)
        out = [o.numpy().copy(), np.asarray(off)]
    elif entry == "stream":
        st = FrontendStream(fe, 1, 2000)
        out, routes = [], []
        pos = 0
        for k, n in enumerate((560, 160, 2000)):
            o, off = st.push([x[pos:pos + n]], final=[1 if k == 2 else 0])
            pos += n
            routes.append(K.last_route(ctx))
            out += [o.numpy().copy() if off[-1] else np.zeros((0,), np.float32), np.asarray(off)]
        st.close()
        return out, "|".join(routes)
    else:
        raise KeyError(entry)
    return out, K.last_route(ctx)


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        assert a.tobytes() == b.tobytes(), (what, i)


@pytest.mark.gpu
def test_the_switch_selects_the_lean_pass_and_nothing_else_does(ctx, pairs):
    for name, (lean, plain) in pairs.items():
        assert is_lean(lean) == 1 and is_lean(plain) == 0, name
        assert form(lean) == form(plain) == 3, name   # kFeConstTw | kFeLdsMel: what the form hook reported before
    # the lean pass is a form of the constant-table kernel only
    assert is_lean(make_fe(ctx, LELE_HIP_FE_CONST_TW="0")) == 0
    assert is_lean(make_fe(ctx, LELE_HIP_FE_LDS_TABLES="0")) == 0
    assert is_lean(make_fe(ctx, LELE_HIP_FE_LEAN_LDS="1")) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("cfg", ["default", "lfr2"])
def test_lean_pass_gives_the_bytes_of_the_plain_pass(ctx, pairs, cfg, fam):
    lean, plain = pairs[cfg]
    for n in LENGTHS:
        x = FAMILIES[fam](n, n % 7)
        for entry, route in (("batch", "fe.main_std/fe.tile_dma"), ("logmel", "fe.main_std/fe.tile_dma")):
            got, r1 = run_entry(lean, ctx, entry, x)
            want, r0 = run_entry(plain, ctx, entry, x)
            assert got[0].size > 0, (n, entry)
            same_bytes(got, want, (cfg, fam, n, entry))
            assert r1 == r0 == route, (n, entry, r1, r0)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("cfg", ["default", "lfr2"])
def test_segments_and_streams_give_the_bytes_of_the_plain_pass(ctx, pairs, cfg, fam):
    lean, plain = pairs[cfg]
    x = FAMILIES[fam](frames(65), 3)
    for entry, route in (("segments3", "fe.seg_std/fe.tile_mixed"), ("segments3_unaligned", "fe.seg_std/fe.tile_regs"), ("stream", None)):
        got, r1 = run_entry(lean, ctx, entry, x)
        want, r0 = run_entry(plain, ctx, entry, x)
        assert sum(a.size for a in got) > 0, entry
        same_bytes(got, want, (cfg, fam, entry))
        assert r1 == r0, (entry, r1, r0)
        if route is not None:
            assert r1 == route, (entry, r1)
        else:
            assert all(r.startswith("fe.seg_std/fe.tile_") for r in r1.split("|")), r1


@pytest.mark.gpu
def test_lean_pass_meets_the_oracle(pairs, orc):
    """the comparison above is build against build; this one ties the lean pass to the reference restatement (the suite's bar)"""
    lean, _ = pairs["default"]
    x = synth_pcm(frames(130), 130)
    ref = orc.frontend_compute(x)
    got = lean.compute_batch(x[None, :]).numpy()[0]
    assert got.shape == ref.shape
    err = np.abs(got - ref) - (1e-4 * np.abs(ref) + 1e-6)   # RTOL, ATOL of tests/test_frontend_gpu.py
    assert np.all(err <= 0), float(err.max())
