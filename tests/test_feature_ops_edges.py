"""The small feature operators (lele_amd/csrc/features_ops.hip: lfr, cmvn, cmvn_segments, segments_to_padded, cmvn_apply_with_stats,
rfft, stft, stft_power_spectrum) at every edge of their loops, bit for bit.

The bar is the CPU oracle (oracle/pyoracle.py), or a few lines of numpy for the pure copies, compared with parity.same_bits_f32:
equal 32-bit patterns, or NaN on both sides.  That sees what np.array_equal cannot -- the sign of a zero, a denormal flushed to zero
-- and admits inputs that hold NaN and infinities.  Where a case only means something while its expected array holds such values,
the test asserts that on the expected array.  The oracle is a restatement too: the CPU-only tests at the top tie it to float64 on
the input families used below."""
import numpy as np
import pytest

from parity import holds, same_bits_f32

EPS32 = float(np.finfo(np.float32).eps)
SPECIALS = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-40], np.float32)   # 1e-40: an f32 denormal

# (n_fft, hop, win_length, len) of the STFT cases
STFT_CASES = [(2, 1, 2, 5), (4, 3, 3, 10), (8, 8, 5, 40), (64, 16, 64, 64), (64, 16, 64, 63), (64, 100, 40, 500), (4096, 512, 4096, 6000),
              (512, 160, 400, 1)]
STFT_LEN_EDGES = [(64, 16, 40, n) for n in (39, 40, 55, 56, 57)]    # frames 1, 1, 1, 2, 2
CMVN_T, CMVN_D = (1, 7, 8, 9, 15, 16, 17), (1, 63, 64, 65, 129)
CMVN_EPS = (0.0, 1e-5, 1.0)
RFFT_N = (2, 4, 8, 16, 32, 4096)
# the overflow row of rfft: seeded standard-normal values times this scale.  Chosen on the CPU (1.2 to 1.5 times FLT_MAX over the
# row's largest float64 bin) so that every input is finite and the oracle's bins hold finite values beside infinities
RFFT_OVERFLOW_SCALE = {2: 2.18e38, 4: 1.2766e38, 8: 7.73e37, 16: 5.34e37, 32: 2.51e37, 4096: 2.44e36}


# ------------------------------------------------------------------------------------------------ inputs, shared by CPU and GPU tests
def with_specials(x):
    """x with -0.0, NaN, +inf, -inf and a denormal in its first elements (row 0 where a row holds five)"""
    x = np.array(x, np.float32)
    k = min(len(SPECIALS), x.size)
    x.reshape(-1)[:k] = SPECIALS[:k]
    return x


def stft_signal(n_fft, length):
    return np.random.default_rng(1000 * n_fft + length).standard_normal(length).astype(np.float32)


def cmvn_data(t, d, seed=0):
    return (np.random.default_rng(10007 * t + d + seed).standard_normal((t, d)) * 3 + 10).astype(np.float32)


CONSTANTS = (10.1, 7.7, 0.1)
SPECIAL_COLUMNS = ("c10.1", "c7.7", "c0.1", "zero", "tiny", "huge", "denormal", "nan", "inf", "plain0", "plain1", "plain2")


def cmvn_special(t):
    """[t, 12]: the columns a well-conditioned draw never holds (SPECIAL_COLUMNS)"""
    rng = np.random.default_rng(31 * t)
    x = (rng.standard_normal((t, len(SPECIAL_COLUMNS))) * 3 + 10).astype(np.float32)
    for k, c in enumerate(CONSTANTS):
        x[:, k] = c                                                      # one-pass f32 variance of a constant: about 0, either sign
    x[:, 3] = 0.0
    x[:, 4] = (rng.standard_normal(t) * 1e-20).astype(np.float32)        # squares underflow
    # squares overflow (9e38 and more), the mean's square does not (alternating signs): sum of squares inf, variance inf, sd inf
    x[:, 5] = (3e19 * rng.uniform(1.0, 1.5, t) * np.where(np.arange(t) % 2, -1.0, 1.0)).astype(np.float32)
    x[:, 6] = (rng.standard_normal(t) * 1e-40).astype(np.float32)        # denormal in
    x[t // 2, 7] = np.nan
    x[t // 3, 8] = np.inf
    return x


def one_pass_variance(column):
    """cmvn.rs:28-50 on one column in sequential f32, before the clamp: (variance, mean)"""
    s = q = np.float32(0.0)
    for v in np.asarray(column, np.float32):
        s = np.float32(s + v)
        q = np.float32(q + np.float32(v * v))
    tf = np.float32(len(column))
    mean = np.float32(s / tf)
    return np.float32(np.float32(q / tf) - np.float32(mean * mean)), mean


def rfft_rows(n):
    """[67, n]: ordinary | +0 | -0 | impulses at 0, 1, 2 | denormal scale | overflow scale | one +inf | one NaN | ordinary .."""
    rng = np.random.default_rng(50 + n)
    x = rng.standard_normal((67, n)).astype(np.float32)
    x[1] = 0.0
    x[2] = -0.0
    for r, p in ((3, 0), (4, 1), (5, 2)):
        x[r] = 0.0
        x[r, p % n] = 1.5
    x[6] = (rng.standard_normal(n) * 1e-40).astype(np.float32)
    x[7] = (np.random.default_rng(700 + n).standard_normal(n).astype(np.float32) * np.float32(RFFT_OVERFLOW_SCALE[n])).astype(np.float32)
    x[8, n // 3] = np.inf
    x[9, n // 2] = np.nan
    return x


def oracle_rfft_rows(orc, x):
    out = [orc.rfft(row, 2) for row in x]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def oracle_default_window(orc, n_fft, win):
    """The periodic Hann window the oracle's stft applies when none is given, exactly: a unit impulse under hop 1 leaves window[i] * 1.0
    alone in frame win - 1 - i, and a frame with one non-zero sample has that sample as its bin 0 (every other term is an exact zero)"""
    impulse = np.zeros(2 * win - 1, np.float32)
    impulse[win - 1] = 1.0
    return np.ascontiguousarray(orc.stft(impulse, n_fft, 1, win)[::-1, 0, 0])


def frames_of(sig, n_fft, hop, win, window):
    """the windowed, zero-extended frames [frames, n_fft] of math.rs:2343-2351, in f32 (one rounded product a sample)"""
    nfr = 1 if len(sig) < win else (len(sig) - win) // hop + 1
    fr = np.zeros((nfr, n_fft), np.float32)
    for f in range(nfr):
        seg = sig[f * hop:f * hop + win]
        fr[f, :len(seg)] = seg * window[:len(seg)]
    return fr


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


SEG_LENGTHS = [0, 7, 0, 0, 8, 9, 1, 16, 0]
MANY = 65538                                     # segments: two launches of 65535 and 3, lengths cycling 0, 1, 2, 3


def padded_reference(x, off, t_max, pad):
    count, d = len(off) - 1, x.shape[1]
    out = np.full((count, t_max, d), pad, np.float32)
    for b in range(count):
        out[b, :off[b + 1] - off[b]] = x[off[b]:off[b + 1]]
    return out


# ------------------------------------------------------------------------------------------------ CPU: the oracle against float64
def test_oracle_stft_is_anchored_to_float64(orc):
    """Every (n_fft, hop, win, len) of the GPU cases on finite ordinary input: each complex bin of the oracle within
    eps_f32 * log2(n_fft) * sum|windowed frame| of numpy's float64 rfft of the same f32 frame (log2(n_fft) butterfly levels, each adding
    at most one rounding of a partial sum that the frame's absolute sum bounds).
    Measured on these signals, |error| / (eps_f32 * sum|frame|) at its largest bin: 0.00 at (2, 1, 2, 5) and (512, 160, 400, 1), 0.38 at
    (4, 3, 3, 10), 0.35 at (8, 8, 5, 40), 0.57 / 0.65 at (64, 16, 64, 64 / 63), 0.77 at (64, 100, 40, 500), 0.25 at (4096, 512, 4096,
    6000), and 1.14 / 0.86 / 0.97 / 0.75 / 0.80 at (64, 16, 40, 39 / 40 / 55 / 56 / 57): the largest is 1.14 against a bound of 6, and
    no case uses more than 0.19 of its bound.
    The default window itself: within 8 eps_f32 of the float64 periodic Hann (the f32 angle 2 pi i / win carries three roundings of a
    value up to 2 pi: 1.1e-6, halved by the 0.5; cosf and the two remaining operations add under 2 eps)."""
    worst = 0.0
    for n_fft, hop, win, length in STFT_CASES + STFT_LEN_EDGES:
        sig = stft_signal(n_fft, length)
        w = oracle_default_window(orc, n_fft, win)
        assert w.shape == (win,)
        hann64 = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(win) / win))
        assert np.abs(w.astype(np.float64) - hann64).max() <= 8 * EPS32, (n_fft, win)
        fr = frames_of(sig, n_fft, hop, win, w)
        want = np.fft.rfft(fr.astype(np.float64), axis=1)
        got = orc.stft(sig, n_fft, hop, win).astype(np.float64)
        assert got.shape == want.shape + (2,), (n_fft, hop, win, length)
        err = np.abs((got[..., 0] + 1j * got[..., 1]) - want)
        scale = EPS32 * np.abs(fr.astype(np.float64)).sum(axis=1, keepdims=True)
        ratio = float((err / np.where(scale > 0, scale, 1.0)).max())     # a frame of zeros (len = 1 under Hann): error 0 required
        assert (err <= np.log2(n_fft) * scale).all(), (n_fft, hop, win, length, ratio)
        print("stft oracle vs float64 at %r: |error| <= %.3f eps_f32 sum|frame| (bound %d)" % ((n_fft, hop, win, length), ratio, np.log2(n_fft)))
        worst = max(worst, ratio / np.log2(n_fft))
        # the power form is the same bins squared and added in f32 (math.rs:2423-2428)
        p = orc.stft_power(sig, n_fft, hop, win)
        g32 = orc.stft(sig, n_fft, hop, win)
        same_bits_f32(p, g32[..., 0] * g32[..., 0] + g32[..., 1] * g32[..., 1], "power of %r" % ((n_fft, hop, win, length),))
    print("largest share of the bound used: %.3f" % worst)


def test_oracle_rfft_rows_hold_what_the_cases_need(orc):
    """the special rows of rfft_rows keep their meaning: denormal bins, an overflow row with finite and infinite bins and no NaN input,
    NaN rows; ordinary rows within the float64 bound of the STFT anchor"""
    minus_zero_bins = 0
    for n in RFFT_N:
        x = rfft_rows(n)
        re, im = oracle_rfft_rows(orc, x)
        assert np.isfinite(x[7]).all() and holds(re[7], "finite") and (np.isinf(re[7]).any() or np.isinf(im[7]).any()), n
        assert holds(np.concatenate([re[6], im[6]]), "denormal"), n
        assert not np.isfinite(re[8]).all() and np.isnan(re[9]).all(), n
        assert not np.signbit(im[:, 0]).any() and not np.signbit(im[:, -1]).any(), n     # bins 0 and n/2: imaginary part +0.0
        assert not re[1:3].any() and not im[1:3].any() and not np.signbit(re[1]).any(), n      # zero rows: zeros out, +0.0 in: +0.0 out
        minus_zero_bins += int(np.signbit(re[2]).sum() + np.signbit(im[2]).sum())
        for r in (0, 10, 66):
            want = np.fft.rfft(x[r].astype(np.float64))
            err = np.abs(re[r].astype(np.float64) + 1j * im[r].astype(np.float64) - want)
            assert (err <= EPS32 * np.log2(n) * np.abs(x[r].astype(np.float64)).sum()).all(), (n, r)
        # float64 keeps the denormal scale too: the oracle's row 6 is the float64 transform to within a few denormal steps
        want6 = np.fft.rfft(x[6].astype(np.float64))
        assert np.abs(re[6].astype(np.float64) - want6.real).max() <= np.log2(n) * n * 1.5e-45, n
    assert minus_zero_bins > 0        # the -0.0 rows leave bins of -0.0 that a comparison by value could not tell from +0.0


def test_oracle_cmvn_is_anchored_to_float64(orc):
    """Well-conditioned data (standard_normal * 3 + 10): the oracle's one-pass f32 statistics against the float64 two-pass formula.
    Measured: 1.34e-5 absolute at (93, 65) and 1.97e-5 at the worst point of the T x D grid of the GPU test (a column whose few frames
    lie close together: small variance, large normalised values).  The bound is 4 x the larger measured value.  Not applied to the ill-conditioned columns of cmvn_special: there the one-pass f32
    formula is the contract."""
    def err(x):
        x64 = x.astype(np.float64)
        want = (x64 - x64.mean(axis=0)) / np.sqrt(x64.var(axis=0) + 1e-5)
        return float(np.abs(orc.cmvn(x).astype(np.float64) - want).max())
    e93 = err(cmvn_data(93, 65))
    grid = max(err(cmvn_data(t, d)) for t in CMVN_T for d in CMVN_D if t > 1)   # T = 1: variance 0, output 0 / sqrt(eps) exactly
    print("cmvn oracle vs float64: %.3g at (93, 65), %.3g over the grid" % (e93, grid))
    assert e93 <= 4 * 1.97e-5 and grid <= 4 * 1.97e-5
    x1 = cmvn_data(1, 65)
    assert not orc.cmvn(x1).any()


def test_one_pass_variance_goes_negative_on_constant_columns(orc):
    """the clamp var = max(var, 0) is reached: sequential f32 moments of a constant column leave a negative variance at T = 9 and at
    T = 333, and with eps = 0 the oracle then divides by sqrt(0): infinities, not the NaN of sqrt(negative)"""
    for t in (7, 8, 9, 17, 333):
        var = [float(one_pass_variance(np.full(t, c, np.float32))[0]) for c in CONSTANTS]
        assert min(var) < 0.0, (t, var)
    for t in (9, 333):
        x = cmvn_special(t)
        got = orc.cmvn(x, 0.0)
        negative = 0
        for k in range(3):
            var, mean = one_pass_variance(x[:, k])
            if var < 0:
                negative += 1
                assert mean != x[0, k] and np.isinf(got[:, k]).all(), (t, k)      # (x - mean) / 0: signed infinity
            # the emulation is the oracle's arithmetic: the same column under eps = 1 from (variance, mean)
            sd = np.sqrt(np.float32(max(var, np.float32(0.0)) + np.float32(1.0)))
            same_bits_f32(orc.cmvn(x, 1.0)[:, k], ((x[:, k] - mean) / sd).astype(np.float32), "emulated column %d at T = %d" % (k, t))
        assert negative >= 1, t
        assert np.isnan(got[:, 3]).all()                                            # all-zero column, eps = 0: 0 / 0
        assert not got[:, 5].any() and holds(got[:, 5], "+0", "-0"), t              # sd = inf: signed zeros
        assert np.isnan(got[:, 7]).all() and holds(got[:, 8], "nan", "-inf"), t
        assert holds(orc.cmvn(x, 1.0)[:, 6], "denormal"), t


def test_numpy_restatements_of_the_copies():
    x = with_specials(np.arange(12, dtype=np.float32).reshape(4, 3) + 1)
    off = offsets_of([0, 3, 0, 1])
    out = padded_reference(x, off, 3, np.float32(-0.0))
    assert out.shape == (4, 3, 3) and np.signbit(out[0]).all() and not out[0].any()
    same_bits_f32(out[1], x[:3])
    same_bits_f32(out[3, 0], x[3])
    assert np.signbit(out[3, 1:]).all()
    assert holds(x, "-0", "nan", "+inf", "-inf", "denormal")
    with pytest.raises(AssertionError):
        same_bits_f32(np.zeros(2, np.float32), np.array([0.0, -0.0], np.float32))
    with pytest.raises(AssertionError):
        same_bits_f32(np.array([1e-40], np.float32), np.zeros(1, np.float32))
    with pytest.raises(AssertionError):
        same_bits_f32(np.array([np.nan, 1.0], np.float32), np.array([1.0, np.nan], np.float32))
    assert same_bits_f32(np.array([np.nan, -0.0], np.float32), -np.array([np.nan, 0.0], np.float32))   # NaN sign is free, zero's is not


def test_real_fft_refuses_another_length():
    """RealFft(length).process asserts input.len() == n upstream (features/fft.rs:24); raised before any device is touched"""
    import lele_amd
    from lele_amd.features import RealFft
    with pytest.raises(lele_amd.LeleError, match=r"8.*16|16.*8"):
        RealFft(8).process(np.zeros(16, np.float32))
    with pytest.raises(lele_amd.LeleError, match="last dimension is 4, not 16"):
        RealFft(16).process(np.zeros((3, 4), np.float32))


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("t,d,m,n", [(1, 3, 1, 1), (2, 3, 8, 1), (5, 2, 4, 9), (3, 1, 7, 6), (13, 5, 2, 3), (6000, 80, 7, 6)])
def test_lfr_is_a_bit_transparent_gather(ctx, orc, t, d, m, n):
    """m = 1, even m (pad = (m - 1) / 2 floors), n > T, m > T (every block clamps), n = 1; (6000, 80, 7, 6): 560 000 outputs, a second
    trip through the grid-stride loop (2048 x 256 threads)"""
    from lele_amd.features import Lfr
    x = with_specials(np.random.default_rng(t * 100 + d).standard_normal((t, d)))
    want = orc.lfr(x, m, n)
    placed = {3: ("-0", "nan", "+inf"), 5: ("-0", "nan", "+inf", "-inf", "denormal")}[min(5, x.size)]
    assert holds(want, *placed), "the expected gather lost its special values"
    if t == 6000:
        assert want.size > 2048 * 256
    same_bits_f32(Lfr(m, n, ctx).compute(x).numpy(), want, "lfr [T, D]")
    same_bits_f32(Lfr(m, n, ctx).compute(x.reshape(1, t, d)).numpy(), want, "lfr [1, T, D]")


@gpu
def test_lfr_empty_and_refused_shapes(ctx):
    import lele_amd
    from lele_amd.features import Lfr
    got = Lfr(7, 6, ctx).compute(np.zeros((0, 5), np.float32))
    assert got.shape == (0, 35) and got.numpy().size == 0
    with pytest.raises(lele_amd.LeleError, match="expects"):
        Lfr(7, 6, ctx).compute(np.zeros((2, 4, 5), np.float32))


@gpu
@pytest.mark.parametrize("eps", CMVN_EPS)
def test_cmvn_loop_edges(ctx, orc, eps):
    """T around the 8-frame unrolled body and its tail, D around the 64-thread block of the moments kernel"""
    from lele_amd.features import Cmvn
    for t in CMVN_T:
        for d in CMVN_D:
            x = cmvn_data(t, d)
            same_bits_f32(Cmvn(eps, ctx).compute(x).numpy(), orc.cmvn(x, eps), "cmvn (%d, %d) eps %g" % (t, d, eps))
    x = cmvn_data(9, 65)
    same_bits_f32(Cmvn(eps, ctx).compute(x.reshape(1, 9, 65)).numpy(), orc.cmvn(x, eps).reshape(1, 9, 65), "cmvn [1, T, D]")
    xb = np.stack([cmvn_data(9, 65, seed=s) for s in range(3)])          # the [B, T, D] extension: every utterance on its own
    got = Cmvn(eps, ctx).compute(xb).numpy()
    assert got.shape == (3, 9, 65)
    for b in range(3):
        same_bits_f32(got[b], orc.cmvn(xb[b], eps), "cmvn utterance %d of [3, 9, 65]" % b)


@gpu
def test_cmvn_apply_takes_a_second_grid_stride_trip(ctx, orc):
    from lele_amd.features import Cmvn
    x = cmvn_data(600, 560)
    assert x.size > 1024 * 256
    same_bits_f32(Cmvn(ctx=ctx).compute(x).numpy(), orc.cmvn(x), "cmvn (600, 560)")


@gpu
@pytest.mark.parametrize("t", [9, 333])
@pytest.mark.parametrize("eps", CMVN_EPS)
def test_cmvn_special_columns(ctx, orc, t, eps):
    """constant columns (negative one-pass variance: the clamp), zeros, underflowing and overflowing squares, denormals, NaN, +inf"""
    from lele_amd.features import Cmvn
    x = cmvn_special(t)
    want = orc.cmvn(x, eps)
    assert min(float(one_pass_variance(x[:, k])[0]) for k in range(3)) < 0.0
    if eps == 0.0:
        for k in range(3):
            if one_pass_variance(x[:, k])[0] < 0:
                assert np.isinf(want[:, k]).all(), k           # a kernel without the clamp gives NaN here
    if eps == 1.0:
        assert holds(want[:, 6], "denormal")
    assert not want[:, 5].any() and holds(want[:, 5], "+0", "-0") and np.isnan(want[:, 7]).all() and holds(want[:, 8], "nan", "-inf")
    got = Cmvn(eps, ctx).compute(x).numpy()
    for k, name in enumerate(SPECIAL_COLUMNS):
        same_bits_f32(got[:, k], want[:, k], "column %s at T = %d, eps %g" % (name, t, eps))


@gpu
def test_cmvn_empty_inputs_keep_their_shape(ctx):
    from lele_amd.features import Cmvn
    for shape in ((0, 5), (4, 0), (1, 0, 5)):
        got = Cmvn(ctx=ctx).compute(np.zeros(shape, np.float32))
        assert got.shape == shape and got.numpy().size == 0


@gpu
def test_cmvn_apply_with_stats_edges(ctx, orc):
    import lele_amd
    from lele_amd.features import Cmvn
    rng = np.random.default_rng(5)
    eps = np.float32(1e-5)
    x = cmvn_data(9, 65)
    mean, std = rng.standard_normal(65).astype(np.float32), rng.uniform(0.5, 2, 65).astype(np.float32)
    std[7] = -eps                    # std + eps == 0: +-inf
    mean[11] = np.nan
    want = orc.cmvn_apply_with_stats(x, mean, std)
    assert np.isinf(want[:, 7]).all() and np.isnan(want[:, 11]).all() and np.isfinite(np.delete(want, (7, 11), axis=1)).all()
    same_bits_f32(Cmvn(ctx=ctx).apply_with_stats(x, mean, std).numpy(), want, "[T, D]")
    same_bits_f32(Cmvn(ctx=ctx).apply_with_stats(x.reshape(1, 9, 65), mean, std).numpy(), want.reshape(1, 9, 65), "[1, T, D]")
    big = cmvn_data(1000, 560)        # 560 000 elements: past 2048 x 256 threads
    assert big.size > 2048 * 256
    mean, std = rng.standard_normal(560).astype(np.float32), rng.uniform(0.5, 2, 560).astype(np.float32)
    same_bits_f32(Cmvn(ctx=ctx).apply_with_stats(big, mean, std).numpy(), orc.cmvn_apply_with_stats(big, mean, std), "(1000, 560)")
    with pytest.raises(lele_amd.LeleError, match="Mean dimension mismatch"):
        Cmvn(ctx=ctx).apply_with_stats(x, mean[:64], std[:65])
    with pytest.raises(lele_amd.LeleError, match="Std dimension mismatch"):
        Cmvn(ctx=ctx).apply_with_stats(x, mean[:65], std[:64])


@gpu
@pytest.mark.parametrize("eps", (0.0, 1e-5))
def test_cmvn_segments_is_the_oracle_on_every_segment(ctx, orc, eps):
    """empty segments first, last and adjacent; the 9-row segment carries the special columns"""
    from lele_amd.features import Cmvn
    off = offsets_of(SEG_LENGTHS)
    x = cmvn_data(int(off[-1]), 65)
    x[off[5]:off[6], :len(SPECIAL_COLUMNS)] = cmvn_special(9)
    got = Cmvn(eps, ctx).compute_segments(x, off).numpy()
    assert got.shape == x.shape
    for b, n in enumerate(SEG_LENGTHS):
        if n:
            same_bits_f32(got[off[b]:off[b + 1]], orc.cmvn(x[off[b]:off[b + 1]], eps), "segment %d (%d rows)" % (b, n))
    want5 = orc.cmvn(x[off[5]:off[6]], eps)
    assert holds(want5, "nan", "-inf", "-0") and (eps != 0.0 or np.isinf(want5[:, 1]).all())


@gpu
def test_cmvn_segments_past_the_grid_limit(ctx, orc):
    """65 538 segments: two launches (65 535 + 3), whose offsets, statistics and rows must line up across the chunk boundary"""
    from lele_amd.features import Cmvn
    lengths = np.arange(MANY) % 4
    off = offsets_of(lengths)
    x = cmvn_data(int(off[-1]), 3)
    got = Cmvn(ctx=ctx).compute_segments(x, off).numpy()
    assert got.shape == x.shape
    pick = [0, 1] + list(range(65533, MANY)) + sorted(np.random.default_rng(9).choice(np.arange(2, 65533), 64, replace=False).tolist())
    assert sum(1 for b in pick if lengths[b]) >= 40
    for b in pick:
        if lengths[b]:
            same_bits_f32(got[off[b]:off[b + 1]], orc.cmvn(x[off[b]:off[b + 1]]), "segment %d" % b)
    # every row of every segment was written by its own segment's launch: the device's own dense call on a [B, T, D] view of the
    # 3-row segments agrees with the packed call everywhere
    three = np.flatnonzero(lengths == 3)
    dense = Cmvn(ctx=ctx).compute(np.stack([x[off[b]:off[b] + 3] for b in three])).numpy()
    same_bits_f32(np.stack([got[off[b]:off[b] + 3] for b in three]), dense, "3-row segments against the dense [B, 3, D] call")


@gpu
@pytest.mark.parametrize("pad", [-0.0, float("nan"), 1.5])
def test_segments_to_padded_is_a_bit_transparent_copy(ctx, pad):
    from lele_amd import kernels as K
    off = offsets_of(SEG_LENGTHS)
    x = with_specials(cmvn_data(int(off[-1]), 65))
    assert holds(x, "-0", "nan", "+inf", "-inf", "denormal")
    for t_max, t_out in ((0, 16), (20, 20)):
        got, lengths = K.segments_to_padded(x, off, t_max, pad, ctx=ctx)
        assert lengths.tolist() == SEG_LENGTHS
        want = padded_reference(x, off, t_out, np.float32(pad))
        assert holds(want, "nan") and (pad != 0 or holds(want, "-0"))
        same_bits_f32(got.numpy(), want, "t_max %d pad %r" % (t_max, pad))


@gpu
def test_segments_to_padded_past_the_grid_limit(ctx):
    from lele_amd import kernels as K
    lengths = np.arange(MANY) % 4
    off = offsets_of(lengths)
    x = cmvn_data(int(off[-1]), 3)
    got, _ = K.segments_to_padded(x, off, 0, -0.0, ctx=ctx)
    same_bits_f32(got.numpy(), padded_reference(x, off, 3, np.float32(-0.0)), "65 538 segments")


@gpu
def test_segment_layout_errors(ctx):
    import lele_amd
    from lele_amd import kernels as K
    from lele_amd.features import Cmvn
    x = cmvn_data(10, 4)
    for call in (lambda off: Cmvn(ctx=ctx).compute_segments(x, off), lambda off: K.segments_to_padded(x, off, ctx=ctx)):
        with pytest.raises(lele_amd.LeleError, match="row_offsets must run from 0 to R = 10"):
            call([1, 5, 10])
        with pytest.raises(lele_amd.LeleError, match="row_offsets must run from 0 to R = 10"):
            call([0, 5, 9])
        with pytest.raises(lele_amd.LeleError, match="row_offsets decrease at segment 1"):
            call([0, 6, 4, 10])
    with pytest.raises(lele_amd.LeleError, match="t_max 5 is shorter than the longest segment \\(6 rows\\)"):
        K.segments_to_padded(x, [0, 6, 10], 5, ctx=ctx)


@gpu
@pytest.mark.parametrize("n", RFFT_N)
def test_rfft_rows_bit_for_bit(ctx, orc, n):
    """the scalar-to-FMA butterfly switch at half-size 4 (n = 8 is the first to take it), the LDS limit n = 4096; signed zeros, denormals
    (the device keeps them: the oracle does, and float64 agrees), overflow, +inf, NaN -- and ordinary rows beside them that nothing
    may leak into"""
    from lele_amd.features import RealFft
    x = rfft_rows(n)
    want_re, want_im = oracle_rfft_rows(orc, x)
    assert holds(np.concatenate([want_re[6], want_im[6]]), "denormal")
    assert holds(want_re[7], "finite") and (np.isinf(want_re[7]).any() or np.isinf(want_im[7]).any())
    assert not np.isfinite(want_re[8]).all() and np.isnan(want_re[9]).all()
    assert np.isfinite(want_re[10:]).all() and np.isfinite(want_im[10:]).all()
    re, im = RealFft(n, ctx).process(x)
    re, im = re.numpy(), im.numpy()
    assert re.shape == (67, n // 2 + 1) and im.shape == re.shape
    for r in range(67):
        same_bits_f32(re[r], want_re[r], "re of row %d, n = %d" % (r, n))
        same_bits_f32(im[r], want_im[r], "im of row %d, n = %d" % (r, n))
    r1, i1 = RealFft(n, ctx).process(x[0])                      # the [n] form
    same_bits_f32(r1.numpy().reshape(-1), want_re[0]) and same_bits_f32(i1.numpy().reshape(-1), want_im[0])


@gpu
def test_rfft_refused_lengths(ctx):
    import lele_amd
    from lele_amd.features import RealFft
    for n, msg in ((6, "length 6 is not a power of two"), (1, "length 1 is not a power of two"), (8192, "n_fft=8192 exceeds the device limit")):
        with pytest.raises(lele_amd.LeleError, match=msg):
            RealFft(n, ctx).process(np.zeros((2, n), np.float32))
    with pytest.raises(lele_amd.LeleError, match="last dimension is 16, not 8"):    # fft.rs:24; used to return a 16-point transform
        RealFft(8, ctx).process(np.zeros((1, 16), np.float32))


def check_stft(K, ctx, orc, sig, n_fft, hop, win, window=None, what=""):
    want, want_p = orc.stft(sig, n_fft, hop, win, window), orc.stft_power(sig, n_fft, hop, win, window)
    for shape in ((len(sig),), (1, len(sig))):
        lead = shape[:-1]
        s = K.stft(sig.reshape(shape), n_fft, hop, win, window, ctx=ctx)
        p = K.stft_power_spectrum(sig.reshape(shape), n_fft, hop, win, window, ctx=ctx)
        assert s.shape == lead + want.shape and p.shape == lead + want_p.shape, (what, s.shape, p.shape)
        same_bits_f32(s.numpy().reshape(want.shape), want, "stft %s %r" % (what, shape))
        same_bits_f32(p.numpy().reshape(want_p.shape), want_p, "stft_power_spectrum %s %r" % (what, shape))
    return want, want_p


@gpu
@pytest.mark.parametrize("n_fft,hop,win,length", STFT_CASES + STFT_LEN_EDGES + [(64, 16, 40, 1)])
def test_stft_configurations(ctx, orc, n_fft, hop, win, length):
    """n_fft from 2 to 4096, hop below, at and above the window, win_length < n_fft, and the frame-count rule (len - win) / hop + 1 at
    len == win, win - 1, win + hop - 1, win + hop and len = 1; default periodic-Hann window, [L] and [1, L]"""
    from lele_amd import kernels as K
    want, _ = check_stft(K, ctx, orc, stft_signal(n_fft, length), n_fft, hop, win, what=str((n_fft, hop, win, length)))
    frames = {39: 1, 40: 1, 55: 1, 56: 2, 57: 2}.get(length) if (n_fft, hop, win) == (64, 16, 40) and length > 1 else None
    assert frames is None or want.shape[0] == frames


@gpu
def test_stft_windows_empty_signal_and_nan(ctx, orc):
    import lele_amd
    from lele_amd import kernels as K
    sig = stft_signal(64, 200)
    w = np.random.default_rng(8).standard_normal(50).astype(np.float32)      # longer than win_length: its first 40 entries count
    w[3] = 0.0
    w[4] = -0.0
    assert (w[:40] < 0).any()
    want, _ = check_stft(K, ctx, orc, sig, 64, 16, 40, w, "explicit window")
    same_bits_f32(want, orc.stft(sig, 64, 16, 40, w[:40].copy()))
    with pytest.raises(lele_amd.LeleError, match="window shorter than win_length"):
        K.stft(sig, 64, 16, 40, w[:39].copy(), ctx=ctx)
    # one NaN sample: only the frames that overlap it are NaN (11 frames; sample 100 lies in frames 4, 5, 6)
    bad = sig.copy()
    bad[100] = np.nan
    want, want_p = check_stft(K, ctx, orc, bad, 64, 16, 40, what="one NaN sample")
    assert want.shape[0] == 11
    assert [f for f in range(11) if np.isnan(want[f]).any()] == [4, 5, 6] and np.isnan(want_p[4:7]).all()
    assert not np.isnan(want_p[:4]).any() and not np.isnan(want_p[7:]).any()
    # the empty signal: math.rs:2313-2316
    e = np.zeros(0, np.float32)
    assert K.stft(e, 64, 16, 40, ctx=ctx).shape == (0, 0, 33, 2) and K.stft_power_spectrum(e, 64, 16, 40, ctx=ctx).shape == (0, 0, 33)


@gpu
def test_stft_refused_arguments(ctx):
    import lele_amd
    from lele_amd import kernels as K
    sig = stft_signal(64, 400)
    for fn in (K.stft, K.stft_power_spectrum):
        with pytest.raises(lele_amd.LeleError, match="length 48 is not a power of two"):
            fn(sig, 48, 16, 48, ctx=ctx)
        with pytest.raises(lele_amd.LeleError, match="n_fft=8192 exceeds the device limit"):
            fn(np.zeros(9000, np.float32), 8192, 512, 8192, ctx=ctx)
        with pytest.raises(lele_amd.LeleError, match="need 0 < win_length <= n_fft and hop > 0"):
            fn(sig, 64, 16, 65, ctx=ctx)
        with pytest.raises(lele_amd.LeleError, match="need 0 < win_length <= n_fft and hop > 0"):
            fn(sig, 64, 0, 64, ctx=ctx)
        # [B, L] with B > 1: upstream transforms the flattened data once, shapes the result [B, ..] and panics in
        # TensorView::from_slice (tensor.rs:66).  The device used to report [2, frames, ..] over a buffer of half those bytes.
        with pytest.raises(lele_amd.LeleError, match="Data length mismatch"):
            fn(np.stack([sig, sig]), 64, 16, 64, ctx=ctx)
        with pytest.raises(lele_amd.LeleError, match="Data length mismatch"):
            fn(np.zeros((2, 1, 400), np.float32), 64, 16, 64, ctx=ctx)
