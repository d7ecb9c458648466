"""Phase A on real and conjugate values (lele_amd/csrc/fe_core.h: phase_a_conj, tw_conj_image), on the CPU.

The per-lane code the HIP kernel runs is compiled for the host and driven by a 16-lane emulator (tests/emu/fe_emulate_conj.cpp):
phase_a_conj, the exchange, phase_b on the conjugated table image.  A lane of class primed(16 * rho + c) holds (re, -im); un-primed by
that class, the 257 bins must equal the oracle's restatement of the reference FFT -- `re` equal, `im` equal -- and the power the
kernel computes from the STORED pair must be the bits of fe::power on the oracle's pair.  (Equal as numbers: the folds drop zeros whose
sign the reference computes, fe_core.h's "alike zeros"; the power is compared bit for bit.)  Non-finite frames are out of scope, as
fe_core.h states for the existing folds.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(HERE, "emu", "fe_emulate_conj.cpp")
    so = os.path.join(HERE, "emu", "libfe_emu_conj.so")
    hdr = os.path.join(HERE, "..", "lele_amd", "csrc", "fe_core.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bin_is_primed(emu):
    """class of bin j = (2 v + rho) * 16 + c: primed(16 * rho + c); bin 256 is real"""
    j = np.arange(257)
    cls = np.array([emu.fe_conj_primed(int(16 * ((x >> 4) & 1) + (x & 15))) for x in j], bool)
    cls[256] = False
    return cls


def frames():
    rng = np.random.default_rng(0)
    out = []
    for trial in range(64):   # the frames of tests/test_fe_core_emulation.py
        fr = np.zeros(512, np.float32)
        fr[:400] = (rng.standard_normal(400) * 10 ** rng.uniform(-3, 4)).astype(np.float32)
        if trial % 3 == 0:
            fr[:400] += np.float32(1e4) * np.sin(0.3 * np.arange(400)).astype(np.float32)
        out.append(("random%d" % trial, fr))
    for n in (0, 15, 16, 255, 399):
        fr = np.zeros(512, np.float32)
        fr[n] = 1.0
        out.append(("impulse%d" % n, fr))
    out.append(("zero", np.zeros(512, np.float32)))
    fr = np.zeros(512, np.float32)
    fr[37] = np.float32(1e-41)   # subnormal
    assert 0 < fr[37] < np.finfo(np.float32).tiny
    out.append(("subnormal", fr))
    return out


def test_primed_is_the_stated_set(emu):
    want = [r == 8 or r % 16 in (1, 2, 4, 5, 9, 10, 13) for r in range(32)]
    assert [bool(emu.fe_conj_primed(r)) for r in range(32)] == want
    assert not emu.fe_conj_primed(0) and not emu.fe_conj_primed(16)   # the real registers: bins 0 and 256 come from them


def test_image_conjugates_exactly_the_primed_lanes_entries(emu, orc):
    twr, twi, _ = orc.precompute_twiddles(512)
    twr, twi = np.ascontiguousarray(twr[:511]), np.ascontiguousarray(twi[:511])
    img = np.empty(2 * 511, np.float32)
    emu.fe_conj_tw_image(ptr(twr), ptr(twi), C.c_int(511), ptr(img))
    got = img.view(np.uint32).reshape(511, 2)
    sign = np.uint32(0x80000000)
    n_conj = 0
    for i in range(511):
        conj = i >= 31 and bool(emu.fe_conj_primed((i + 1) & 31))
        n_conj += conj
        assert got[i, 0] == twr[i:i + 1].view(np.uint32)[0], i
        assert got[i, 1] == (twi[i:i + 1].view(np.uint32)[0] ^ (sign if conj else np.uint32(0))), i
    assert n_conj == 15 * 15   # 15 primed classes of 32, in the 15 groups of 32 entries of stages 6..9


def test_conjugate_form_is_bit_exact(emu, orc):
    twr, twi, _ = orc.precompute_twiddles(512)
    twr, twi = np.ascontiguousarray(twr), np.ascontiguousarray(twi)
    primed = bin_is_primed(emu)
    assert primed.sum() > 100 and not primed[0] and not primed[16] and not primed[256]
    for name, fr in frames():
        re, im = orc.rfft(fr, 2)
        re, im = np.ascontiguousarray(re, np.float32), np.ascontiguousarray(im, np.float32)
        ore, oim, opw = np.empty(257, np.float32), np.empty(257, np.float32), np.empty(257, np.float32)
        emu.fe_emulate_conj_fft512(ptr(fr), ptr(twr), ptr(twi), ptr(ore), ptr(oim), ptr(opw))
        assert np.all(np.isfinite(ore)) and np.all(np.isfinite(oim)), name
        assert np.array_equal(ore, re), name
        assert np.array_equal(np.where(primed, -oim, oim), im), name
        want_pw = np.empty(257, np.float32)
        emu.fe_conj_power(ptr(re), ptr(im), C.c_int(257), ptr(want_pw))
        assert opw.tobytes() == want_pw.tobytes(), name
        if name.startswith("impulse"):
            assert np.any(opw > 0), name
