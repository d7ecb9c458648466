"""The fused front-end kernels' LFR scatter: where a frame's log-mel row is stored.

fe_main_kernel / fe_seg_main_kernel divide once per block to find a lane's first LFR target (block b of row i with
n*i + b - pad == frame) and carry (b, i) and the target's byte offset from pass to pass: b += 4, then one compare-subtract where
lfr_n >= 4, a division where it is smaller.  Stores are the utterance's base plus a 32-bit offset.  None of it may move a row:

* (lfr_m, lfr_n) on both sides of the lfr_n >= 4 switch, with n > m (rows that skip frames) and m up to 9 (clamps of several
  blocks at both ends), all on the default 80-filter mel bank, i.e. the unrolled kernel the benchmark times (the front-end reports
  no kernel route through lele_hip_last_route, so there is none to assert);
* 1, 63, 64, 65 and 129 frames: a single frame (every block of every row is a clamp), a block's last frame, a full block, one frame
  into a second block, one frame into a third;
* a batch of three through compute_batch and the same three as touching segments through compute_segments -- the first 16-byte
  aligned (direct-to-LDS tile), the second one sample longer than its frames need (its length is no multiple of four: register
  staging), which leaves the third starting 4 bytes past a 16-byte boundary -- agree bit for bit and meet the oracle at the
  front-end's bar (tests/test_frontend_gpu.py);
* the default (7, 6) cases equal `tests/golden/frontend_lfr_targets_parent_<frames>.npy` bit for bit: what compute_batch gave on an
  MI355X for the same three utterances with the library built from commit e04314a (a division per pass, 64-bit store addresses).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL = 1e-4, 1e-6   # the front-end's bar (tests/test_frontend_gpu.py)
LFR = [(7, 6), (1, 1), (5, 1), (7, 2), (4, 3), (9, 4), (3, 5)]
FRAMES = [1, 63, 64, 65, 129]


def utterances(frames):
    """three utterances of exactly `frames` frames"""
    from conftest import synth_pcm
    n = 400 + 160 * (frames - 1)
    return [synth_pcm(n, 100 * frames + s) for s in range(3)]


@pytest.fixture(scope="module")
def frontends(ctx):
    from lele_amd.features import FeatureConfig, SenseVoiceFrontend
    return {mn: SenseVoiceFrontend(FeatureConfig(lfr_m=mn[0], lfr_n=mn[1]), ctx=ctx) for mn in LFR}


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("m,n", LFR)
def test_batch_and_segments_store_every_row_where_the_oracle_does(frontends, orc, m, n, frames):
    fe = frontends[(m, n)]
    xs = utterances(frames)
    rows = (frames + n - 1) // n
    batch = fe.compute_batch(np.stack(xs)).numpy()
    assert batch.shape == (3, rows, 80 * m)
    for i, x in enumerate(xs):
        ref = orc.frontend_compute(x, lfr_m=m, lfr_n=n)
        assert ref.shape == batch[i].shape
        err = np.abs(batch[i] - ref) - (RTOL * np.abs(ref) + ATOL)
        assert np.all(err <= 0), (i, float(err.max()))
    # the same utterances as touching segments; the extra sample after the second belongs to no frame
    L = len(xs[0])
    pcm = np.concatenate([xs[0], xs[1], np.zeros(1, np.float32), xs[2]])
    segs = [(0, L), (L, 2 * L + 1), (2 * L + 1, 3 * L + 1)]
    assert L % 4 == 0 and segs[2][0] % 4 == 1
    out, off = fe.compute_segments(pcm, segs)
    assert list(off) == [0, rows, 2 * rows, 3 * rows]
    out = out.numpy()
    for i in range(3):
        assert np.array_equal(out[off[i]:off[i + 1]], batch[i]), i
    if (m, n) == (7, 6):
        want = np.load(os.path.join(GOLDEN, "frontend_lfr_targets_parent_%d.npy" % frames))
        assert want.shape == batch.shape and want.dtype == batch.dtype
        assert np.array_equal(batch, want)
