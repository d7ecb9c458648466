"""What the convolution entries of lele_amd/csrc/conv.hip answer to a geometry they cannot run, word for word, and the two pad
conventions their shared geometry builder must keep apart.

Every entry resolves its own attribute conventions and reports its own wording (the ConvInteger family mirrors the reference's
"conv2d_with_zero_points: ..."): conv2d / conv2d_res / conv2d_pitched, conv1d, conv_integer, conv_integer_from_f32, each on x
[1, 4, 5, 5] ([1, 4, 5] for conv1d) with group = 3, a weight whose C_in/g is wrong, a 7 x 7 (7-tap) kernel without padding, a stride
of 0 and -- where the entry takes a bias -- a bias one element short.  The messages are copied from the source: the test fails when a
refactor rewords one or lets another check answer first.

Pads: conv1d takes [left, right] (conv1d.rs:886-887), the 2-D entries [top, left, bottom, right] or two values [h, w] used on both
sides (conv2d.rs:246-273).  (2, 0) on conv1d and (1, 2) on conv2d / conv_integer are the cases one convention would misread as the
other: the output shapes differ, and the values (small integers: every f32 sum is exact, so equality is the bar) are held to
oracle.pyoracle, the convolution oracle.npref's ConvInteger section names."""
import numpy as np
import pytest

from oracle import pyoracle as O

OC = 8
X2 = np.arange(100, dtype=np.float32).reshape(1, 4, 5, 5) % 7 - 3
X1 = np.arange(20, dtype=np.float32).reshape(1, 4, 5) % 7 - 3


def w2(icg=4, k=3, oc=OC):
    return (np.arange(oc * icg * k * k, dtype=np.float32).reshape(oc, icg, k, k) % 5 - 2)


def w1(icg=4, k=3, oc=OC):
    return (np.arange(oc * icg * k, dtype=np.float32).reshape(oc, icg, k) % 5 - 2)


BIAS = np.arange(OC, dtype=np.float32)
SHORT = BIAS[:OC - 1]

# (what, weight shape arguments, group, strides, bias)
BAD = (
    ("group", dict(), 3, 1, BIAS),
    ("cin", dict(icg=3), 1, 1, BIAS),
    ("k7", dict(k=7), 1, 1, BIAS),
    ("stride0", dict(), 1, 0, BIAS),
    ("bias", dict(), 1, 1, SHORT),
)
CONV2D = {"group": "conv2d: channels not divisible by group",
          "cin": "conv2d: weight C_in/g = 3 but input has 4 channels per group",
          "k7": "conv2d: output dimensions must be positive",
          "stride0": "conv2d: output dimensions must be positive",
          "bias": "conv2d: bias has 7 entries for 8 channels"}
CONV1D = {"group": "conv1d: channels not divisible by group",
          "cin": "conv1d: weight C_in/g mismatch",
          "k7": "conv1d: output length must be positive",
          "stride0": "conv1d: output length must be positive",
          "bias": "conv1d: bias shorter than C_out"}
CONVI = {"group": "conv_integer: channels not divisible by group",
         "cin": "conv_integer: weight C_in/g mismatch",
         "k7": "conv2d_with_zero_points: output dimensions must be positive",
         "stride0": "conv2d_with_zero_points: output dimensions must be positive"}


def message(call):
    from lele_amd._lib import LeleError
    with pytest.raises(LeleError) as e:
        call()
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["conv2d", "conv2d_res", "conv2d_pitched"])
@pytest.mark.parametrize("what,wkw,group,stride,bias", BAD, ids=[b[0] for b in BAD])
def test_conv2d_entries(ctx, entry, what, wkw, group, stride, bias):
    from lele_amd import kernels as K
    w, s = w2(**wkw), [stride, stride]
    if entry == "conv2d":
        call = lambda: K.conv2d(X2, w, bias, [], group, [], s, ctx=ctx)  # noqa: E731
    elif entry == "conv2d_res":
        res = np.zeros((1, OC, 3, 3), np.float32)
        call = lambda: K.conv2d_res(X2, w, bias, res, [], group, [], s, ctx=ctx)  # noqa: E731
    else:
        call = lambda: K.conv2d(X2, w, bias, [], group, [], s, out=ctx.buf(), out_window=(0, 4 * OC * 9), ctx=ctx)  # noqa: E731
    assert message(call) == CONV2D[what]


@pytest.mark.gpu
@pytest.mark.parametrize("what,wkw,group,stride,bias", BAD, ids=[b[0] for b in BAD])
def test_conv1d(ctx, what, wkw, group, stride, bias):
    from lele_amd import kernels as K
    assert message(lambda: K.conv1d(X1, w1(**wkw), bias, [], group, [], [stride], ctx=ctx)) == CONV1D[what]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["conv_integer", "conv_integer_from_f32"])
@pytest.mark.parametrize("what,wkw,group,stride,bias", BAD[:4], ids=[b[0] for b in BAD[:4]])
def test_conv_integer_entries(ctx, entry, what, wkw, group, stride, bias):
    from lele_amd import kernels as K
    w, s = np.abs(w2(**wkw)), [stride, stride]
    if entry == "conv_integer":
        call = lambda: K.conv_integer(np.abs(X2), w, None, None, [], group, [], s, ctx=ctx)  # noqa: E731
    else:
        call = lambda: K.conv_integer_from_f32(X2, w, None, [], group, [], s, ctx=ctx)  # noqa: E731
    assert message(call) == CONVI[what]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


@pytest.mark.gpu
def test_conv1d_pads_are_left_right(ctx):
    from lele_amd import kernels as K
    got = K.conv1d(X1, w1(), BIAS, [], 1, [2, 0], [], ctx=ctx).numpy()
    assert got.shape == (1, OC, 5)   # 5 + 2 + 0 - 2; read as [h, w] = both sides it would be 7 (or 3)
    same_bits(got, O.conv1d(X1, w1(), BIAS, [], 1, [2, 0], []))
    xp = np.pad(X1, ((0, 0), (0, 0), (2, 0)))
    same_bits(got, O.conv1d(xp, w1(), BIAS, [], 1, [0, 0], []))


@pytest.mark.gpu
def test_two_value_pads_are_height_width_on_both_sides(ctx):
    from lele_amd import kernels as K
    got = K.conv2d(X2, w2(), BIAS, [], 1, [1, 2], [], ctx=ctx).numpy()
    assert got.shape == (1, OC, 5, 7)   # 5 + 1 + 1 - 2 rows, 5 + 2 + 2 - 2 columns; read as [left, right] the rows would be 3
    same_bits(got, O.conv2d(X2, w2(), BIAS, [], 1, [1, 2], []))
    same_bits(got, O.conv2d(X2, w2(), BIAS, [], 1, [1, 2, 1, 2], []))
    codes, wc = np.abs(X2), np.abs(w2())
    zx, zw = np.array([2.0], np.float32), np.array([1.0], np.float32)
    got = K.conv_integer(codes, wc, zx, zw, [], 1, [1, 2], [], ctx=ctx).numpy()
    assert got.shape == (1, OC, 5, 7)
    same_bits(got, O.conv_integer(codes, wc, 2.0, 1.0, [], 1, [1, 2, 1, 2], []))
