"""The fused front-end kernels' PCM tile: direct-to-LDS staging, raw samples, fused multiply-add sum chain.

fe_main_kernel / fe_seg_main_kernel copy a block's 10 560-sample run into LDS with direct-to-LDS loads where the run is 16-byte
aligned and through registers where it is not (`LELE_HIP_FE_TILE_DMA=0` forces the registers everywhere), and the 400-step frame sum
reads the raw samples as `fma(x, 32768, sum)`.  None of it may move a bit:

* lengths at which the tile's edge is the utterance's edge: both stagings agree bit for bit and meet the oracle;
* a batch whose utterances touch (the halo rows of one end in the next, the last ends the tensor) equals the single calls;
* the same utterances as segments, unaligned (register staging) and aligned (direct-to-LDS inside fe_seg_main_kernel);
* the chain against RECORDED output: `tests/golden/frontend_parent_lfr_*.npy` are the LFR features the library built from commit
  75e90d1 (the parent of this change: samples scaled on the way into the tile, plain adds) gave on an MI355X for the two inputs of
  `chain_inputs()`.  Equality with them is what pins fma(x, 2^15, sum) == (x * 2^15) + sum on the device, subnormal samples and
  sums included.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL = 1e-4, 1e-6   # the front-end's bar (tests/test_frontend_gpu.py)
EDGE_LENGTHS = [400, 10480, 10484, 10640, 20960]   # 1 frame; exactly 64; 64 + 4 samples; 65 = a second block of one frame; 129


def synth(n, seed):
    from conftest import synth_pcm
    return synth_pcm(n, seed)


def chain_inputs():
    """name -> PCM of the recorded cases"""
    import bench
    n = 10640
    rng = np.random.default_rng(20240607)
    # magnitudes from subnormal (x * 2^15 is then barely normal) to 3e4, in stretches longer than a frame and mixed sample by sample
    mags = np.array([1e-42, 1e-20, 1.0, 3e4], np.float64)
    pick = rng.integers(0, 4, n)
    pick[:1200] = 0          # frames that hold subnormals only
    pick[1200:2400] = 1      # ... 1e-20 only
    pick[2400:3600] = rng.integers(0, 2, 1200)
    x = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * mags[pick]).astype(np.float32)
    assert np.count_nonzero(np.abs(x[:1200]) < np.finfo(np.float32).tiny) == 1200
    return {"wide": x, "synth": np.ascontiguousarray(bench.synth_batch(1, 30 * 16000, 0)[0][:20960])}


@pytest.fixture(scope="module")
def fe(ctx):
    from lele_amd.features import SenseVoiceFrontend
    return SenseVoiceFrontend(ctx=ctx)


@pytest.fixture(scope="module")
def fe_regs(ctx):
    """the same front-end with the tile staged through registers for aligned runs too"""
    from lele_amd.features import SenseVoiceFrontend
    old = os.environ.get("LELE_HIP_FE_TILE_DMA")
    os.environ["LELE_HIP_FE_TILE_DMA"] = "0"
    try:
        return SenseVoiceFrontend(ctx=ctx)
    finally:
        if old is None:
            del os.environ["LELE_HIP_FE_TILE_DMA"]
        else:
            os.environ["LELE_HIP_FE_TILE_DMA"] = old


@pytest.fixture(scope="module")
def three():
    return [synth(10640, 20 + s) for s in range(3)]


@pytest.fixture(scope="module")
def three_single(fe, three):
    return [fe.compute(x).numpy() for x in three]


@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_tile_edge_is_the_utterance_edge(fe, fe_regs, orc, n):
    x = synth(n, n % 11)
    ref = orc.frontend_compute(x)
    dma, regs = fe.compute(x).numpy(), fe_regs.compute(x).numpy()
    assert dma.shape == ref.shape
    assert np.array_equal(dma, regs)
    err = np.abs(dma - ref) - (RTOL * np.abs(ref) + ATOL)
    assert np.all(err <= 0), float(err.max())


def test_batch_whose_utterances_touch_equals_the_single_calls(fe, fe_regs, three, three_single):
    xs = np.stack(three)
    got = fe.compute_batch(xs).numpy()
    got_regs = fe_regs.compute_batch(xs).numpy()
    for i in range(3):
        assert np.array_equal(got[i], three_single[i]), i
        assert np.array_equal(got_regs[i], three_single[i]), i


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_segments_equal_compute(fe, fe_regs, three, three_single, lead):
    """lead 0: every segment starts 16-byte aligned (direct-to-LDS inside fe_seg_main_kernel); 1, 3: none does (register staging)"""
    from lele_amd.features import pack
    pcm, segs = pack([np.zeros(lead, np.float32)] + three)
    segs = segs[1:]
    assert all(s % 4 == lead for s, _ in segs)
    for f in (fe, fe_regs):
        out, off = f.compute_segments(pcm, segs)
        out = out.numpy()
        assert list(off) == [0, 11, 22, 33]
        for i in range(3):
            assert np.array_equal(out[off[i]:off[i + 1]], three_single[i]), (lead, i)


@pytest.mark.parametrize("name", ["wide", "synth"])
def test_sum_chain_reproduces_the_recorded_parent_output(fe, fe_regs, name):
    x = chain_inputs()[name]
    want = np.load(os.path.join(GOLDEN, "frontend_parent_lfr_%s.npy" % name))
    got = fe.compute(x).numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want)
    assert np.array_equal(fe_regs.compute(x).numpy(), want)
    # the unaligned form of the same samples (register staging, scalar loads) through compute_segments
    pcm = np.concatenate([np.zeros(1, np.float32), x])
    out, _ = fe.compute_segments(pcm, [(1, 1 + len(x))])
    assert np.array_equal(out.numpy(), want)
