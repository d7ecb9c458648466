"""The default front-end kernels' compiled-in tables: phase A's twiddles as constants, the mel weights as an LDS image.

fe_main_kernel / fe_seg_main_kernel / fe_stream_main_kernel of the default bank read the 27 wave-uniform twiddles of FFT stages 2..5
as literals (fe::TwConst, lele_amd/csrc/fe_core.h) and the lane's 40 mel weights from an LDS copy laid out by fe::mel_lds_index.
`LELE_HIP_FE_CONST_TW=0` keeps the kernels that read every twiddle from the table -- which is also what frontend_create selects by
itself when the table it has just built differs from the constants in any bit -- and `LELE_HIP_FE_LDS_TABLES=0` keeps the weights in
global memory.  None of it may move a bit.

CPU (tests/emu/fe_tables_emu.cpp, the shared fe_core.h on the host):
* the constants are the reference's table (the oracle's, and the one the host's libm gives) at the 27 entries, bit for bit;
* phase_a_fast over the constants equals phase_a_fast over the table on random frames, bit for bit;
* the mel image is a permutation of the 640 weights, and every 16-byte request of a frame's 16 lanes covers the 64 banks once.
GPU: the default build against the table-reading kernels on the lengths at which the kernel takes another path, and the create-time
check's own way into the table-reading kernels.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-4, 1e-6   # the front-end's bar (tests/test_frontend_gpu.py)
FORM_CONST_TW, FORM_LDS_MEL = 1, 2   # lele_hip_frontend_kernel_form


def frames(f):
    return 400 + 160 * (f - 1)


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(HERE, "emu", "fe_tables_emu.cpp")
    so = os.path.join(HERE, "emu", "libfe_tables_emu.so")
    hdr = os.path.join(HERE, "..", "lele_amd", "csrc", "fe_core.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_constants_are_the_reference_table(emu, orc):
    n = emu.fe_tw_const_n()
    used = [i for i in range(n) if emu.fe_tw_const_used(i)]
    # tw_off(2)+1; tw_off(3)+0..3; tw_off(4)+1..7; tw_off(5)+1..15
    assert used == [2] + list(range(3, 7)) + list(range(8, 15)) + list(range(16, 31)) and len(used) == 27
    cre, cim = np.empty(n, np.float32), np.empty(n, np.float32)
    emu.fe_tw_const(ptr(cre), ptr(cim))
    ore, oim, _ = orc.precompute_twiddles(512)
    hre, him = np.empty(511, np.float32), np.empty(511, np.float32)
    emu.fe_host_twiddles512(ptr(hre), ptr(him))
    for name, (tre, tim) in {"oracle": (ore, oim), "libm": (hre, him)}.items():
        assert np.array_equal(bits(cre)[used], bits(tre)[used]), name
        assert np.array_equal(bits(cim)[used], bits(tim)[used]), name
        assert emu.fe_tw_const_matches(ptr(np.ascontiguousarray(tre, np.float32)), ptr(np.ascontiguousarray(tim, np.float32))) == 1, name
    # one ulp in one used entry is a mismatch; an entry phase_a_fast never reads is not looked at
    for i in used:
        for part in (0, 1):
            t = [hre.copy(), him.copy()]
            t[part][i] = np.nextafter(t[part][i], np.float32(2.0))
            assert emu.fe_tw_const_matches(ptr(t[0]), ptr(t[1])) == 0, (i, part)
    t = hre.copy()
    t[7] = np.float32(0.5)
    t[100] = np.float32(0.5)
    assert emu.fe_tw_const_matches(ptr(t), ptr(him)) == 1


def test_phase_a_over_constants_equals_phase_a_over_the_table(emu, orc):
    ore, oim, _ = orc.precompute_twiddles(512)
    ore, oim = np.ascontiguousarray(ore, np.float32), np.ascontiguousarray(oim, np.float32)
    rng = np.random.default_rng(5)
    rev5 = [int("{:05b}".format(r)[::-1], 2) for r in range(32)]
    for trial in range(200):
        x = (rng.standard_normal(32) * 10 ** rng.uniform(-6, 6)).astype(np.float32)
        if trial % 4 == 0:
            x[rng.integers(0, 32, 8)] = 0.0
        if trial % 5 == 0:
            x *= np.float32(1e-38)   # subnormal products
        x[[r for r in range(32) if rev5[r] >= 25]] = 0.0   # the zero padding phase_a_fast counts on
        a, b = np.empty(64, np.float32), np.empty(64, np.float32)
        emu.fe_phase_a_fast_both(ptr(x), ptr(ore), ptr(oim), ptr(a), ptr(b))
        assert np.array_equal(bits(a), bits(b)), trial


def test_mel_image_is_a_permutation_and_conflict_free(emu):
    nw, nc = emu.fe_mel_lds_weights(), emu.fe_mel_lds_chunks()
    assert (nw, nc) == (40, 10)
    idx = np.array([[emu.fe_mel_lds_index(s, p) for p in range(16)] for s in range(nw)])
    assert sorted(idx.ravel().tolist()) == list(range(640))   # the 640 weights of the table [step][lane], each once
    for j in range(nc):
        base = idx[4 * j]   # the lane's 16-byte request: four consecutive words from here
        assert np.all(base % 4 == 0)
        for k in range(4):
            assert np.array_equal(idx[4 * j + k], base + k)   # a lane's weights of the chunk are contiguous
        banks = sorted(((base[:, None] + np.arange(4)[None, :]) % 64).ravel().tolist())
        assert banks == list(range(64)), j   # the 16 lanes of a frame: every bank exactly once


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def make_fe(ctx, **env):
    from lele_amd.features import SenseVoiceFrontend
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return SenseVoiceFrontend(ctx=ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def form(fe):
    from lele_amd import _lib
    fn = _lib.lib().lele_hip_frontend_kernel_form
    fn.restype = C.c_int
    return fn(fe._h)


@pytest.fixture(scope="module")
def fe_default(ctx):
    return make_fe(ctx)


@pytest.fixture(scope="module")
def fe_tables(ctx):
    """the table-reading kernels by the switches"""
    return make_fe(ctx, LELE_HIP_FE_CONST_TW="0", LELE_HIP_FE_LDS_TABLES="0")


@pytest.fixture(scope="module")
def fe_mismatch(ctx):
    """the table-reading kernels by the create-time check: it is handed a table one ulp off in one entry"""
    return make_fe(ctx, LELE_HIP_FE_CONST_TW="mismatch")


def run_all(fe, case):
    """every entry point of the fused kernels on one case -> list of arrays"""
    from conftest import synth_pcm
    from lele_amd.features import FrontendStream, pack
    out = []
    if case == "batch3x400":
        xs = np.stack([synth_pcm(400, 40 + s) for s in range(3)])
        out.append(fe.compute_batch(xs).numpy().copy())
        out += [fe.logmel(x).numpy().copy() for x in xs]
        pcm, segs = pack(list(xs))
        o, off = fe.compute_segments(pcm, segs)
        out += [o.numpy().copy(), np.asarray(off)]
    elif case == "segments123":
        z = np.zeros(1, np.float32)
        parts = [z, synth_pcm(frames(65), 1), z, synth_pcm(frames(3), 2), z, synth_pcm(frames(64) + 1, 3)]
        ends = np.cumsum([len(q) for q in parts])
        pcm = np.concatenate(parts)
        segs = [(int(ends[i] - len(parts[i])), int(ends[i])) for i in (1, 3, 5)]
        assert [s % 4 for s, _ in segs] == [1, 2, 3]
        o, off = fe.compute_segments(pcm, segs)
        out += [o.numpy().copy(), np.asarray(off)]
    elif case == "stream":
        st = FrontendStream(fe, 2, 12000)
        o, off = st.push([synth_pcm(frames(70), 7), synth_pcm(5001, 8)], final=[1, 0])
        out += [o.numpy().copy(), np.asarray(off)]
        st.close()
    else:
        x = synth_pcm(frames(case), case)
        out.append(fe.compute_batch(x[None, :]).numpy().copy())
        out.append(fe.logmel(x).numpy().copy())
        o, off = fe.compute_segments(x, [(0, len(x))])
        out += [o.numpy().copy(), np.asarray(off)]
    return out


CASES = ["batch3x400", 63, 64, 65, 257, "segments123", "stream"]


@pytest.fixture(scope="module")
def default_results(fe_default):
    return {c: run_all(fe_default, c) for c in CASES}


@pytest.mark.gpu
def test_forms_are_what_the_switches_and_the_check_select(fe_default, fe_tables, fe_mismatch, ctx):
    assert form(fe_default) == FORM_CONST_TW | FORM_LDS_MEL
    assert form(fe_tables) == 0
    assert form(fe_mismatch) == 0   # the check refused the constants: the table-reading kernels, whatever else is switched on
    assert form(make_fe(ctx, LELE_HIP_FE_LDS_TABLES="0")) == FORM_CONST_TW
    assert form(make_fe(ctx, LELE_HIP_FE_CONST_TW="0")) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_default_build_equals_the_table_reading_kernels(fe_tables, default_results, case):
    got, want = default_results[case], run_all(fe_tables, case)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.size > 0, (case, i)
        assert a.tobytes() == b.tobytes(), (case, i)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_refused_constants_fall_back_and_keep_the_bits(fe_mismatch, default_results, case):
    got, want = run_all(fe_mismatch, case), default_results[case]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (case, i)


@pytest.mark.gpu
def test_constants_only_form_and_the_oracle(ctx, fe_default, default_results, orc):
    """the form with the weights left in global memory (LELE_HIP_FE_LDS_TABLES=0) gives the same bytes, and they meet the oracle"""
    from conftest import synth_pcm
    fe_c = make_fe(ctx, LELE_HIP_FE_LDS_TABLES="0")
    for case in (65, "segments123"):
        for a, b in zip(run_all(fe_c, case), default_results[case]):
            assert a.tobytes() == b.tobytes(), case
    x = synth_pcm(frames(65), 65)
    ref = orc.frontend_compute(x)
    got = default_results[65][0][0]
    assert got.shape == ref.shape
    err = np.abs(got - ref) - (RTOL * np.abs(ref) + ATOL)
    assert np.all(err <= 0), float(err.max())
