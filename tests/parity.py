"""The f32 parity bar of BASELINE.json ("mel and NN ops within 1e-4 relative f32"), in one place.

close_f32: element by element, |got - want| <= tol * |want| + tol * rms(want) + 1e-7.  The rms term is the round-off floor of a sum
of products: an output that cancels to ~0 carries the error of its terms, which scale with the tensor's typical magnitude.  No
max(1, .) slack and no scaling by the tensor's largest element."""
import numpy as np


def same_bits_f32(got, want, what=""):
    """The bit-for-bit bar of two float32 arrays: equal shapes and, element by element, equal 32-bit patterns or NaN on both sides.
    So -0.0 is not +0.0, a denormal is not 0.0 and a NaN must sit where the other has one; a NaN's sign and payload are free (x86
    produces the negative default NaN, the GPU the positive one)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (0x%08x), want %r (0x%08x)" % (
            what, int(bad.sum()), g.size, np.unravel_index(i, got.shape), float(g[i]), int(g.view(np.uint32)[i]), float(w[i]),
            int(w.view(np.uint32)[i])))
    return True


def holds(a, *kinds):
    """a float32 array holds at least one value of each kind: 'nan', '+inf', '-inf', 'denormal', '-0', '+0', 'finite'"""
    a = np.asarray(a, np.float32).reshape(-1)
    mag = np.abs(a)
    tests = {"nan": np.isnan(a), "+inf": a == np.inf, "-inf": a == -np.inf, "denormal": (mag > 0) & (mag < np.finfo(np.float32).tiny),
             "-0": (a == 0) & np.signbit(a), "+0": (a == 0) & ~np.signbit(a), "finite": np.isfinite(a) & (a != 0)}
    return all(bool(tests[k].any()) for k in kinds)


def close_f32(got, want, tol=1e-4, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not want.size:
        return
    rms = float(np.sqrt(np.mean(np.square(want))))
    bad = np.abs(got - want) > tol * np.abs(want) + tol * rms + 1e-7
    assert not bad.any(), "%s: %d of %d elements outside %g (max abs diff %.3e, rms %.3e)" % (
        what, int(bad.sum()), want.size, tol, float(np.abs(got - want).max()), rms)
