"""A queue of images of different sizes, one call each way: kernels.image_preprocess_batch (bit for bit image_preprocess per image) and
kernels.yolo_seg_postprocess_sized (equal to yolo_seg_postprocess per image at its own size), whose mask comes from bit tables of the
reference's exact predicates instead of the pixel x detection loop.

CPU: the helpers, and a numpy restatement of the bit-table scheme against a numpy restatement of the direct loop -- with every cell bit
outside a box's cell rectangle poisoned, and three wrong variants that the same inputs must reject.  GPU: equality with the per-image
calls and the oracle."""
import ctypes as C

import numpy as np
import pytest

F = np.float32

# (image width, image height) and the mask grid (rows, columns) of the scheme test
SCHEME_CASES = [((96, 72), (40, 40)), ((33, 47), (16, 16)), ((1, 1), (40, 40)), ((500, 375), (160, 160)), ((7, 300), (40, 40)),
                ((96, 72), (24, 40))]
BATCH_SIZES = [(96, 72), (33, 47), (1, 1), (500, 375), (640, 640), (7, 300)]  # (w, h)


# ---------------------------------------------------------------------------------------------------------------- helpers
def test_pack_images_and_unpack_masks_round_trip():
    from lele_amd import apps
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((17, 5), (1, 1), (33, 47))]
    queue = [imgs[0], imgs[1], imgs[0], imgs[2]]          # one image listed twice
    data, off, hs, ws = apps.pack_images(queue)
    assert data.dtype == np.uint8 and data.ndim == 1 and off.dtype == np.int64 and hs.dtype == np.int32 and ws.dtype == np.int32
    assert hs.tolist() == [17, 1, 17, 33] and ws.tolist() == [5, 1, 5, 47]
    assert off[0] == off[2] and data.size == sum(i.size for i in imgs)    # stored once
    for img, o, h, w in zip(queue, off, hs, ws):
        assert np.array_equal(data[o:o + 3 * h * w].reshape(h, w, 3), img)
    data, off, hs, ws = apps.pack_images([])
    assert data.shape == (0,) and data.dtype == np.uint8 and off.shape == hs.shape == ws.shape == (0,)
    with pytest.raises(ValueError):
        apps.pack_images([np.zeros((4, 4), np.uint8)])
    sizes = [(5, 17), (1, 1), (47, 33)]                   # (w, h)
    masks = [rng.integers(0, 2, (h, w), dtype=np.uint8) * 255 for w, h in sizes]
    flat = np.concatenate([m.reshape(-1) for m in masks])
    moff = np.concatenate([[0], np.cumsum([m.size for m in masks])]).astype(np.int64)
    back = apps.unpack_masks(flat, moff, sizes)
    assert len(back) == 3 and all(b.shape == m.shape and np.array_equal(b, m) for b, m in zip(back, masks))
    assert apps.unpack_masks(np.zeros(0, np.uint8), np.zeros(1, np.int64), []) == []
    with pytest.raises(ValueError):
        apps.unpack_masks(flat, moff, [(5, 17), (1, 1), (33, 47)][:2])


# ------------------------------------------------------------------------------------------------ the scheme, in numpy
def _cell_of(v, scale, side):
    """the mask cell a pixel coordinate reads: min(floor((v + 0.5f) * scale), side - 1) in f32, as yolo_mask_kernel has it"""
    m = np.floor((np.asarray(v, F) + F(0.5)) * F(scale)).astype(np.int64)
    return np.minimum(m, side - 1)


def _edge_boxes(rng, w, h, n):
    """n boxes in image space (x1, y1, x2, y2), f32, as the detections carry them (x1, y1 >= 0; x2 <= w, y2 <= h): first the edge
    cases -- the whole image, one that starts on the last column, one wholly beyond the image (x1 > x2 = w after the clamp), two that are
    empty after the clamps (no integer between the bounds; x2 < 0) -- then boxes with fractional bounds all over the image"""
    edge = [(0, 0, w, h), (max(w - 1.5, 0), 0.25 * h, w, 0.75 * h), (1.09375 * w, 0, w, h), (int(0.2 * w) + 0.2, int(0.2 * h) + 0.2, int(0.2 * w) + 0.8, h),
            (0, 0, -0.0625 * w, h)]
    out = np.zeros((n, 4), F)
    for i in range(n):
        if i < len(edge):
            out[i] = edge[i]
            continue
        x1, y1 = rng.random() * w * 0.8, rng.random() * h * 0.8
        out[i] = [x1, y1, min(x1 + (0.05 + 0.4 * rng.random()) * w, w), min(y1 + (0.05 + 0.4 * rng.random()) * h, h)]
    return out


def _direct_mask(boxes, pred, w, h):
    """image.rs:213-262 pixel by detection: pred[d, cy, cx] stands for `mv > 0.5 && mv * score > 0.5` of detection d at that cell"""
    hm, wm = pred.shape[1:]
    ix, iy = np.arange(w, dtype=F), np.arange(h, dtype=F)
    mx, my = _cell_of(ix, F(wm) / F(w), wm), _cell_of(iy, F(hm) / F(h), hm)
    mask = np.zeros((h, w), bool)
    for d, (x1, y1, x2, y2) in enumerate(boxes):
        inx, iny = (ix >= x1) & (ix <= x2), (iy >= y1) & (iy <= y2)
        mask |= (iny[:, None] & inx[None, :]) & pred[d][my[:, None], mx[None, :]]
    return mask


def _scheme_mask(boxes, pred, w, h, first=np.ceil, short=0, max_words=None):
    """(b) cell bits inside the rectangle the box's pixels map to -- POISONED with 1 outside it --, (c) column / row bits of the pixel
    range first(x1) .. min(floor(x2), w - 1), (d) a pixel is set iff the AND of its three words is non-zero over the ceil(n / 32) words.
    first / short / max_words are the mutation hooks: the real scheme is ceil, 0, None."""
    hm, wm = pred.shape[1:]
    n = len(boxes)
    words = (n + 31) // 32
    sx, sy = F(wm) / F(w), F(hm) / F(h)
    ix, iy = np.arange(w, dtype=F), np.arange(h, dtype=F)
    cellb, colb, rowb = np.zeros((words, hm, wm), np.uint32), np.zeros((words, w), np.uint32), np.zeros((words, h), np.uint32)
    cyy, cxx = np.mgrid[0:hm, 0:wm]
    for d, (x1, y1, x2, y2) in enumerate(boxes):
        bit = np.uint32(1 << (d & 31))
        xlo, xhi = first(x1), min(np.floor(x2), F(w - 1))
        ylo, yhi = first(y1), min(np.floor(y2), F(h - 1))
        inside = np.zeros((hm, wm), bool)
        if xlo <= xhi and ylo <= yhi:
            cx0, cx1 = int(_cell_of(xlo, sx, wm)), int(_cell_of(xhi, sx, wm)) - short
            cy0, cy1 = int(_cell_of(ylo, sy, hm)), int(_cell_of(yhi, sy, hm)) - short
            inside = (cxx >= cx0) & (cxx <= cx1) & (cyy >= cy0) & (cyy <= cy1)
            colb[d >> 5][(ix >= xlo) & (ix <= xhi)] |= bit
            rowb[d >> 5][(iy >= ylo) & (iy <= yhi)] |= bit
        cellb[d >> 5][np.where(inside, pred[d], True)] |= bit
    mx, my = _cell_of(ix, sx, wm), _cell_of(iy, sy, hm)
    hit = np.zeros((h, w), np.uint32)
    for wd in range(words if max_words is None else min(words, max_words)):
        hit |= colb[wd][None, :] & rowb[wd][:, None] & cellb[wd][my[:, None], mx[None, :]]
    return hit != 0


def _scheme_inputs():
    rng = np.random.default_rng(20)
    for (w, h), (hm, wm) in SCHEME_CASES:
        n = 40                                            # crosses a 32-bit word
        boxes = _edge_boxes(rng, w, h, n)
        pred = rng.random((n, hm, wm)) < 0.5
        yield (w, h), boxes, pred


def test_bit_table_scheme_equals_the_direct_loop_with_poison_outside_the_rectangles():
    """Column bits are written here as the pixel RANGE ceil(x1) .. min(floor(x2), w - 1); the kernel writes them as the reference's
    comparison pair -- the same set, asserted below for every box."""
    for (w, h), boxes, pred in _scheme_inputs():
        want = _direct_mask(boxes, pred, w, h)
        assert np.array_equal(_scheme_mask(boxes, pred, w, h), want), (w, h)
        ix = np.arange(w, dtype=F)
        for x1, _, x2, _ in boxes:
            assert np.array_equal((ix >= x1) & (ix <= x2), (ix >= np.ceil(x1)) & (ix <= min(np.floor(x2), F(w - 1))))
    assert any(_direct_mask(b, p, w, h).any() and not _direct_mask(b, p, w, h).all() for (w, h), b, p in _scheme_inputs())


def test_the_same_inputs_reject_three_wrong_variants():
    variants = {"floor for the first pixel": dict(first=np.floor), "cell rectangle one short at the high end": dict(short=1),
                "only the first 32 detections' words": dict(max_words=1)}
    for name, kw in variants.items():
        differs = [not np.array_equal(_scheme_mask(b, p, w, h, **kw), _direct_mask(b, p, w, h)) for (w, h), b, p in _scheme_inputs()]
        assert sum(differs) >= 3, (name, differs)         # not by one lucky pixel of one case


# ---------------------------------------------------------------------------------------------------------------- GPU: preprocess
def _packed(rng, shapes, order):
    """images of `shapes` (h, w), stored in `order` with odd gaps of noise between them; entry i of the returned lists is image i"""
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    parts, off, at = [], [0] * len(imgs), 0
    for k, i in enumerate(order):
        gap = rng.integers(0, 256, 2 * k + 1, dtype=np.uint8)
        parts += [gap, imgs[i].reshape(-1)]
        off[i] = at + gap.size
        at += gap.size + imgs[i].size
    return imgs, np.concatenate(parts), off


def _check_batch(ctx, imgs, data, off, target, listed):
    from lele_amd import kernels as K
    from oracle import pyoracle as O
    hs, ws = [imgs[i].shape[0] for i in listed], [imgs[i].shape[1] for i in listed]
    out = ctx.buf()
    out.upload(np.full(len(listed) * 3 * target * target, np.nan, F))
    got = K.image_preprocess_batch(data, [off[i] for i in listed], hs, ws, target, out=out, ctx=ctx).numpy()
    assert got.shape == (len(listed), 3, target, target) and got.dtype == F
    for k, i in enumerate(listed):
        assert np.array_equal(got[k], O.image_preprocess(imgs[i], target)[0]), (k, imgs[i].shape, target)
        assert np.array_equal(got[k], K.image_preprocess(imgs[i], target, ctx=ctx).numpy()[0]), (k, imgs[i].shape, target)


@pytest.mark.gpu
def test_device_preprocess_batch_bit_for_bit(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(31)
    shapes = [(17, 5), (1, 1), (33, 47), (480, 640), (375, 500), (2, 40000)]   # the wide strip: the f32 product rounds
    imgs, data, off = _packed(rng, shapes, [3, 0, 5, 2, 4, 1])
    assert any(o % 2 for o in off) and any(o % 4 == 1 or o % 4 == 3 for o in off)
    _check_batch(ctx, imgs, data, off, 32, [0, 1, 2, 3, 4, 5, 2])                 # image 2 listed twice
    imgs, data, off = _packed(rng, [(375, 500), (1, 1), (720, 1280)], [2, 0, 1])
    _check_batch(ctx, imgs, data, off, 640, [0, 1, 2])
    imgs, data, off = _packed(rng, [(17, 5), (33, 47), (375, 500)], [1, 2, 0])
    _check_batch(ctx, imgs, data, off, 30, [0, 1, 2])                             # target % 4 != 0: the scalar store
    empty = K.image_preprocess_batch(data, [], [], [], 32, ctx=ctx)
    assert tuple(empty.shape) == (0, 3, 32, 32) and empty.numpy().shape == (0, 3, 32, 32)


@pytest.mark.gpu
def test_device_preprocess_batch_refusals_leave_out_alone(ctx):
    import lele_amd
    from lele_amd import _lib
    rng = np.random.default_rng(32)
    data = ctx.buf().upload(rng.integers(0, 256, 1000, dtype=np.uint8))
    out = ctx.buf()
    before = rng.standard_normal(64).astype(F)
    out.upload(before)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def call(off, hs, ws, count, target, nulls=()):
        keep = []
        a = [np.array(v, dt) for v, dt in ((off, np.int64), (hs, np.int32), (ws, np.int32))]
        sh = _lib.OutShape()
        sh.rank.value = 7
        args = {"ctx": ctx._h, "bytes": _lib.as_tensor(data, keep), "off": a[0].ctypes.data_as(i64p), "hs": a[1].ctypes.data_as(i32p),
                "ws": a[2].ctypes.data_as(i32p), "out": out._h}
        for name in nulls:
            args[name] = None
        rc = _lib.lib().lele_hip_image_preprocess_batch(args["ctx"], args["bytes"], args["off"], args["hs"], args["ws"], C.c_int64(count),
                                                        C.c_int32(target), args["out"], sh.shape, C.byref(sh.rank))
        msg = _lib.lib().lele_hip_last_error().decode()
        assert rc != 0 and sh.rank.value == 7, (msg, nulls)
        assert out.nbytes == before.nbytes and np.array_equal(out.to_numpy((64,), F), before)
        return msg

    ok = ([0, 300], [10, 10], [10, 10])                   # 300 bytes each
    for name in ("ctx", "bytes", "off", "hs", "ws", "out"):
        assert "NULL" in call(*ok, 2, 32, nulls=(name,)), name
    assert "count" in call(*ok, -1, 32)
    assert "target" in call(*ok, 2, 0)
    assert "image 1" in call([0, 300], [10, 0], [10, 10], 2, 32)
    assert "image 1" in call([0, 300], [10, 10], [10, -3], 2, 32)
    assert "image 0" in call([-1, 300], [10, 10], [10, 10], 2, 32)
    assert "image 1" in call([0, 701], [10, 10], [10, 10], 2, 32)          # 701 + 300 > 1000
    assert "image 1" in call([0, 2 ** 62], [10, 10], [10, 10], 2, 32)      # (no overflow in the check itself)
    from lele_amd import kernels as K
    with pytest.raises(lele_amd.LeleError, match="image 1"):
        K.image_preprocess_batch(data, [0, 701], [10, 10], [10, 10], 32, out=out, ctx=ctx)
    got = K.image_preprocess_batch(data, [0, 700], [10, 10], [10, 10], 32, out=out, ctx=ctx)   # the last byte of the buffer is legal
    assert tuple(got.shape) == (2, 3, 32, 32)


# -------------------------------------------------------------------------------------------------------------- GPU: postprocess
def _batch_inputs(seed, sizes, keeps, mask_shape):
    """logits [N, 300, 38] whose image n keeps keeps[n] queries at threshold 0.5 -- their boxes _edge_boxes in image space, carried
    back to the network's 640-space -- and features [N, 32, *mask_shape]"""
    rng = np.random.default_rng(seed)
    logits = np.zeros((len(sizes), 300, 38), F)
    for n, ((w, h), keep) in enumerate(zip(sizes, keeps)):
        logits[n, :, 4] = rng.random(300) * 0.2
        rows = np.sort(rng.choice(300, keep, replace=False))
        boxes = _edge_boxes(rng, w, h, keep)
        for i, b in zip(rows, boxes):
            logits[n, i, :4] = b * np.array([640.0 / w, 640.0 / h, 640.0 / w, 640.0 / h])
            if b[2] < 0:                                  # x2 < 0 behind the clamp of x1 to 0: both raw bounds left of the image
                logits[n, i, 0] = logits[n, i, 2] - 40.0
            if logits[n, i, 2] <= logits[n, i, 0]:        # an inverted box is dropped by the filter: keep it a kept, empty one
                logits[n, i, 2] = logits[n, i, 0] + F(0.01)
            logits[n, i, 4] = 0.55 + rng.random() * 0.45
            logits[n, i, 5] = float(rng.integers(0, 90))
            logits[n, i, 6:] = rng.standard_normal(32)
    feat = (rng.standard_normal((len(sizes), 32) + tuple(mask_shape)) * 0.5).astype(F)
    return logits, feat


BATCHES = {"square": (41, BATCH_SIZES, [300, 33, 1, 4, 12, 0], (40, 40)), "oblong": (42, BATCH_SIZES, [33, 300, 4, 0, 1, 12], (24, 40))}


@pytest.fixture(scope="module")
def per_image(ctx):
    """the existing call and the oracle, image by image at the image's own size: computed once, read by the tests below"""
    from lele_amd import kernels as K
    from oracle import pyoracle as O
    ref = {}
    for name, (seed, sizes, keeps, mshape) in BATCHES.items():
        logits, feat = _batch_inputs(seed, sizes, keeps, mshape)
        rows = []
        for n, (w, h) in enumerate(sizes):
            d, c, m = K.yolo_seg_postprocess(logits[n:n + 1], feat[n:n + 1], w, h, 0.5, 80, ctx=ctx)
            od, om = O.yolo_seg_postprocess(logits[n:n + 1], feat[n:n + 1], w, h, 0.5)
            rows.append((d.numpy().copy(), c.numpy().copy(), m.numpy().copy(), od, om))
            assert int(rows[-1][1][0]) == keeps[n], (name, n)
        ref[name] = (logits, feat, sizes, rows)
    return ref


def _assert_equal_per_image(got, rows, sizes, order=None):
    from lele_amd import apps
    dets, count, mask, moff = got
    d, c = dets.numpy(), count.numpy()
    masks = apps.unpack_masks(mask, moff, [sizes[i] for i in (order or range(len(sizes)))])
    assert moff.tolist() == np.concatenate([[0], np.cumsum([m.size for m in masks])]).tolist()
    for k, i in enumerate(order or range(len(sizes))):
        rd, rc, rm, od, om = rows[i]
        assert c[k] == rc[0] and np.array_equal(d[k], rd), (k, i)           # kept rows and the zero rows behind them
        assert not d[k, c[k]:].any() and np.array_equal(d[k, :c[k]], od), (k, i)
        assert masks[k].shape == rm.shape and np.array_equal(masks[k], rm), (k, i, int((masks[k] != rm).sum()))
        assert not ((masks[k] != om) & (rm == om)).any(), (k, i)            # no disagreement with the oracle beyond the existing call's


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_device_postprocess_sized_equals_the_per_image_call(ctx, per_image, name):
    from lele_amd import kernels as K
    logits, feat, sizes, rows = per_image[name]
    got = K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.5, 80, ctx=ctx)
    assert tuple(got[0].shape) == (len(sizes), 300, 38) and tuple(got[1].shape) == (len(sizes),)
    _assert_equal_per_image(got, rows, sizes)
    assert sum(r[2].any() and not r[2].all() for r in rows) >= 3              # the masks are neither empty nor full
    order = list(range(len(sizes)))[::-1]                                     # the batch reversed: every image the same bytes
    rev = K.yolo_seg_postprocess_sized(logits[order], feat[order], [sizes[i] for i in order], 0.5, 80, ctx=ctx)
    _assert_equal_per_image(rev, rows, sizes, order)


@pytest.mark.gpu
def test_device_postprocess_sized_without_masks_and_with_nothing_kept(ctx, per_image):
    from lele_amd import kernels as K
    logits, feat, sizes, rows = per_image["square"]
    total = sum(w * h for w, h in sizes)
    om = ctx.buf()
    stamp = np.arange(total, dtype=np.int64).astype(np.uint8)
    om.upload(stamp)
    dets, count, mask, moff = K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.5, 80, out_mask=om, masks=False, ctx=ctx)
    assert mask is None and moff[-1] == total
    assert np.array_equal(dets.numpy(), np.stack([r[0] for r in rows])) and np.array_equal(count.numpy(), np.concatenate([r[1] for r in rows]))
    assert np.array_equal(om.to_numpy((total,), np.uint8), stamp)             # the mask buffer was not touched
    dets, count, mask, moff = K.yolo_seg_postprocess_sized(logits, feat, sizes, 1.5, 80, out_mask=om, ctx=ctx)   # nothing passes
    assert not count.numpy().any() and not dets.numpy().any() and mask.numpy().shape == (total,) and not mask.numpy().any()


@pytest.mark.gpu
def test_device_postprocess_sized_with_tables_beyond_the_arena(ctx):
    """66 images over a 160 x 160 mask need 40 * 66 * (25600 + w + h) > 64 MiB of bit tables: they live in the context's scratch block,
    not in its staging arena.  Constant features make a detection's sigmoid the same in every cell, so its mask is its whole box or nothing."""
    from lele_amd import kernels as K
    sizes = [[(33, 47), (96, 72), (7, 300)][i % 3] for i in range(66)]
    assert 40 * sum(160 * 160 + w + h for w, h in sizes) > 64 << 20
    logits, _ = _batch_inputs(61, sizes, [(5 * i) % 41 for i in range(66)], (1, 1))
    feat_host = np.full((66, 32, 160, 160), 0.5, F)
    feat = ctx.buf().upload(feat_host)
    dets, count, mask, moff = K.yolo_seg_postprocess_sized(logits, feat, sizes, 0.5, 80, ctx=ctx)
    from lele_amd import apps
    masks = apps.unpack_masks(mask, moff, sizes)
    assert count.numpy().tolist() == [(5 * i) % 41 for i in range(66)]
    some = 0
    for n in range(66):
        d, c, m = K.yolo_seg_postprocess(logits[n:n + 1], feat_host[n:n + 1], sizes[n][0], sizes[n][1], 0.5, 80, ctx=ctx)
        assert np.array_equal(dets.numpy()[n], d.numpy()) and np.array_equal(masks[n], m.numpy()), n
        some += bool(m.numpy().any() and not m.numpy().all())
    assert some >= 10                                     # masks that are neither empty nor full
    feat.buf.close()


@pytest.mark.gpu
def test_device_postprocess_sized_refusals(ctx, per_image):
    import lele_amd
    from lele_amd import kernels as K
    logits, feat, sizes, _ = per_image["square"]
    for bad, what in ((sizes[:-1], "sizes"), (sizes[:2] + [(0, 5)] + sizes[3:], "image 2"), (sizes[:4] + [(7, -1)] + sizes[5:], "image 4"),
                      ([(46341, 46341)] + sizes[1:], "image 0"), ([(40000, 40000), (30000, 20000)] + sizes[2:], "image 1")):
        with pytest.raises(lele_amd.LeleError, match=what):
            K.yolo_seg_postprocess_sized(logits, feat, bad, 0.5, 80, ctx=ctx)
    with pytest.raises(lele_amd.LeleError, match="NULL"):
        K.yolo_seg_postprocess_sized(logits, None, sizes, 0.5, 80, ctx=ctx)


@pytest.mark.gpu
def test_both_calls_replay_from_a_graph_on_new_data(ctx):
    from lele_amd import kernels as K
    rng = np.random.default_rng(51)
    shapes = [(33, 47), (375, 500), (17, 5)]
    imgs_a, data_a, off = _packed(rng, shapes, [1, 2, 0])
    data_b = rng.integers(0, 256, data_a.size, dtype=np.uint8)
    hs, ws = [s[0] for s in shapes], [s[1] for s in shapes]
    sizes = [(96, 72), (33, 47), (500, 375)]
    la, fa = _batch_inputs(52, sizes, [33, 4, 12], (40, 40))
    lb, fb = _batch_inputs(53, sizes, [1, 40, 7], (40, 40))
    bufs = {k: ctx.buf() for k in ("bytes", "x", "logits", "feat", "dets", "count", "mask")}

    def run(dev):
        x = K.image_preprocess_batch(dev[0], off, hs, ws, 32, out=bufs["x"], ctx=ctx)
        return x, K.yolo_seg_postprocess_sized(dev[1], dev[2], sizes, 0.5, 80, out_dets=bufs["dets"], out_count=bufs["count"],
                                               out_mask=bufs["mask"], ctx=ctx)

    def read():
        total = sum(w * h for w, h in sizes)
        return (bufs["x"].to_numpy((3, 3, 32, 32), F), bufs["dets"].to_numpy((3, 300, 38), F), bufs["count"].to_numpy((3,), np.int32),
                bufs["mask"].to_numpy((total,), np.uint8))

    dev = [bufs["bytes"].upload(data_a), bufs["logits"].upload(la), bufs["feat"].upload(fa)]
    run(dev)                                              # the layouts' tables and the buffers exist from here on
    ctx.sync()
    want_a = read()
    ctx.graph_begin()
    run(dev)
    graph = ctx.graph_end()
    for b in ("x", "dets", "mask"):
        bufs[b].upload(np.zeros(bufs[b].nbytes, np.uint8))
    graph.launch()
    assert all(np.array_equal(g, w) for g, w in zip(read(), want_a))
    bufs["bytes"].upload(data_b)
    bufs["logits"].upload(lb)
    bufs["feat"].upload(fb)
    graph.launch()
    got_b = read()
    fresh = {k: ctx.buf() for k in ("x", "dets", "count", "mask")}
    x = K.image_preprocess_batch(data_b, off, hs, ws, 32, out=fresh["x"], ctx=ctx)
    d, c, m, _ = K.yolo_seg_postprocess_sized(lb, fb, sizes, 0.5, 80, out_dets=fresh["dets"], out_count=fresh["count"], out_mask=fresh["mask"],
                                              ctx=ctx)
    want_b = (x.numpy(), d.numpy(), c.numpy(), m.numpy())
    assert all(np.array_equal(g, w) for g, w in zip(got_b, want_b))
    assert not np.array_equal(want_b[0], want_a[0]) and not np.array_equal(want_b[3], want_a[3]) and want_b[3].any()
    graph.close()
