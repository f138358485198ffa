"""migan_pipeline_batch_post_samples (several completions per image, written out of place by one kernel that tiles the IMAGE) run on
the CPU through the fiber emulator.  The yardstick of every byte comparison is the existing in-place path on copies:
migan_pipeline_batch_post applied to a copy of image i with y row i * S + s.  The generator is not under test: y is seeded random,
N(0, 0.6), or the oracle generator's output for the goldens."""
import os

import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from oracle import migan_torch_cpu as torc
from tests.emu_util import emu_lib, ptr
from tests.pipeline_batch_case import five_items
from tests.test_emu_pipeline_batch import GAUSS, GOLDENS, TILE_H, TILE_W, batch_pre, items_of

FILL = 0xA5                                  # every destination starts as this: a byte the kernel does not write shows


def random_y(rng, n, samples, res):
    return (rng.standard_normal((n * samples, 3, res, res)) * 0.6).astype(np.float32)


def post_samples(lib, items, scratch, bbox, images, y, samples, res, gauss=None):
    outs = [np.full((samples,) + img.shape, FILL, dtype=np.uint8) for img in images]
    lib.pipeline_batch_post_samples(items, samples, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(o) for o in outs], gauss25=gauss)
    return outs


def post_on_copies(lib, images, masks, scratch, bbox, y, samples, res, gauss=None):
    """-> want[i][s]: migan_pipeline_batch_post on a copy of every image, once per sample, with y rows s, S + s, 2 S + s, ..."""
    want = [[None] * samples for _ in images]
    for s in range(samples):
        copies = [np.array(img, copy=True) for img in images]
        ys = np.ascontiguousarray(y[s::samples])
        lib.pipeline_batch_post(items_of(copies, masks), res, ptr(ys), ptr(bbox), ptr(scratch), gauss25=gauss)
        for i, c in enumerate(copies):
            want[i][s] = c
    return want


def check_against_copies(lib, images, masks, y, samples, res, padding, gausses=(None, GAUSS)):
    """every destination == the in-place path on copies, whole arrays; images, boxes and x untouched.  Returns boxes and outputs."""
    originals = [np.array(img, copy=True) for img in images]
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, padding)
    bbox0, x0 = bbox.copy(), x.copy()
    outs = None
    for gauss in gausses:
        outs = post_samples(lib, items, scratch, bbox, images, y, samples, res, gauss)
        want = post_on_copies(lib, images, masks, scratch, bbox, y, samples, res, gauss)
        for i in range(len(images)):
            for s in range(samples):
                np.testing.assert_array_equal(outs[i][s], want[i][s], err_msg=f"item {i}, sample {s}")
            np.testing.assert_array_equal(images[i], originals[i], err_msg=f"source image {i} was written")
        np.testing.assert_array_equal(bbox, bbox0)
        np.testing.assert_array_equal(x, x0)
    return bbox, outs


def test_five_items_three_samples(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(41)
    res, padding, samples = 64, 8, 3
    images, masks = five_items(rng)
    y = random_y(rng, 5, samples, res)
    boxes, outs = check_against_copies(lib, images, masks, y, samples, res, padding)
    for i, mask in enumerate(masks):
        assert list(boxes[i]) == list(po.masked_bbox(mask, res, padding)), f"item {i}"
    # one item whose box starts and ends off the tile grid of the IMAGE in both directions, spans several tiles, and leaves
    # whole tiles of the image outside
    off_grid = []
    for (x0, x1, y0, y1), img in zip(boxes, images):
        h, w = img.shape[1:]
        tiles_y, tiles_x = -(-h // TILE_H), -(-w // TILE_W)
        met_y, met_x = -(-y1 // TILE_H) - y0 // TILE_H, -(-x1 // TILE_W) - x0 // TILE_W      # tile rows / columns the box meets
        off_grid.append(x0 % TILE_W != 0 and x1 % TILE_W != 0 and y0 % TILE_H != 0 and y1 % TILE_H != 0
                        and met_y > 1 and met_x > 1 and met_y * met_x < tiles_y * tiles_x)
    assert any(off_grid), [list(b) for b in boxes]
    # the samples of an item differ inside its box (different y) and are the image outside it
    x0, x1, y0, y1 = boxes[4]
    assert (outs[4][0][:, y0:y1, x0:x1] != outs[4][1][:, y0:y1, x0:x1]).any()
    outside = np.ones(masks[4].shape, dtype=bool)
    outside[y0:y1, x0:x1] = False
    for s in range(samples):
        np.testing.assert_array_equal(outs[4][s][:, outside], images[4][:, outside])


def test_one_sample(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(42)
    images, masks = five_items(rng)
    check_against_copies(lib, images, masks, random_y(rng, 5, 1, 64), 1, 64, 8)


def test_smallest_images(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(43)
    res, samples = 8, 2
    images = [rng.integers(0, 256, (3, 3, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)]
    masks = [np.full((3, 3), 255, dtype=np.uint8), np.full((5, 7), 255, dtype=np.uint8)]
    masks[0][1, 1] = 0
    masks[1][1:4, 2:6] = 0
    _, outs = check_against_copies(lib, images, masks, random_y(rng, 2, samples, res), samples, res, 0)
    assert (outs[1][0] != outs[1][1]).any()           # (the 3 x 3 image's pooled mask is 255 everywhere: it stays as it is)


def test_masks_of_another_size_are_resized_first(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(44)
    res, padding, samples = 64, 8, 2
    sizes = [(96, 80), (50, 70), (64, 48)]
    msizes = [(37, 53), (128, 128), (64, 48)]                         # half size / odd aspect, larger, same
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = []
    for mh, mw in msizes:
        m = np.full((mh, mw), 255, dtype=np.uint8)
        m[mh // 3:mh // 3 * 2, mw // 4:mw // 2] = 0
        m[rng.random((mh, mw)) > 0.97] = 0
        masks.append(m)
    y = random_y(rng, 3, samples, res)
    resized = [np.ascontiguousarray(po.tv_resize(torch.from_numpy(m)[None, None], s, "nearest")[0, 0].numpy()) for m, s in zip(masks, sizes)]
    abox, a = check_against_copies(lib, images, masks, y, samples, res, padding, gausses=(None,))
    bbox, b = check_against_copies(lib, images, resized, y, samples, res, padding, gausses=(None,))
    np.testing.assert_array_equal(abox, bbox)
    for i in range(3):
        np.testing.assert_array_equal(a[i], b[i], err_msg=f"item {i}")
        assert (a[i][0] != images[i]).any() and (a[i][0] != a[i][1]).any()


def test_more_items_than_one_launch_carries(pkg):
    """35 items, two samples each: more than one launch, and the y rows of the second launch start at 2 * (items of the first)"""
    lib = emu_lib()
    rng = np.random.default_rng(45)
    res, n, samples = 8, 35, 2
    sizes = [(3 + i % 10, 3 + (i * 3) % 7) for i in range(n)]        # 3 x 3 ... 12 x 9
    assert (3, 3) in sizes and (12, 9) in sizes
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.ascontiguousarray((rng.random(s) > 0.3).astype(np.uint8) * 255) for s in sizes]
    _, outs = check_against_copies(lib, images, masks, random_y(rng, n, samples, res), samples, res, 1, gausses=(None,))
    assert (outs[34][0] != outs[34][1]).any()


def test_a_box_that_does_not_fit_its_image_gives_plain_copies(pkg):
    """The boxes reach the kernel through device memory, so the host cannot refuse one.  Where the in-place form leaves such an item
    alone, the out-of-place form defines its output: S copies of the image.  The good item of the batch is processed."""
    lib = emu_lib()
    rng = np.random.default_rng(46)
    res, padding, samples = 8, 2, 2
    sizes = [(20, 24), (17, 40), (31, 23)]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m in masks:
        m[5:12, 6:15] = 0
    y = random_y(rng, 3, samples, res)
    items, scratch, bbox, _ = batch_pre(lib, images, masks, res, padding)
    bbox[0] = (4, 24 + 5, 0, 20)                                      # x_max beyond the 24 columns
    bbox[1] = (6, 8, 5, 7)                                            # 2 x 2
    outs = post_samples(lib, items, scratch, bbox, images, y, samples, res)
    want = post_on_copies(lib, images, masks, scratch, bbox, y, samples, res)
    for s in range(samples):
        np.testing.assert_array_equal(outs[0][s], images[0])
        np.testing.assert_array_equal(outs[1][s], images[1])
        np.testing.assert_array_equal(outs[2][s], want[2][s])
        assert (outs[2][s] != images[2]).any()


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[9:-4] for p in GOLDENS])
def test_goldens_as_one_item_of_a_batch(pkg, path):
    """sample 0 of the middle item gets the oracle generator's output: its bytes are the REFERENCE module's result"""
    g = np.load(path)
    res, seed, padding = int(g["resolution"]), int(g["seed"]), int(g["padding"])
    sd = pkg.synth.make_state_dict(res, seed=seed, regime="export")
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    lib = emu_lib()
    rng = np.random.default_rng(47)
    samples = 2
    _, want_bbox, want_x = po.pipeline(g["image"], g["mask"], lambda t: torch.zeros((1, 3, res, res)), res, padding)
    y = random_y(rng, 3, samples, res)
    y[1 * samples + 0] = np.asarray(torc.generator(want_x, sd, res), dtype=np.float32)[0]
    images = [rng.integers(0, 256, (3, 45, 61), dtype=np.uint8), np.array(g["image"], copy=True), rng.integers(0, 256, (3, 33, 19), dtype=np.uint8)]
    masks = [np.full((45, 61), 255, dtype=np.uint8), np.ascontiguousarray(g["mask"][0]), np.zeros((33, 19), dtype=np.uint8)]
    masks[0][10:30, 5:50] = 0
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, padding)
    outs = post_samples(lib, items, scratch, bbox, images, y, samples, res, GAUSS)
    assert list(bbox[1]) == [int(v) for v in g["bbox"]] == list(want_bbox)
    np.testing.assert_array_equal(outs[1][0], g["result"])
    np.testing.assert_array_equal(images[1], g["image"])
    x0, x1, y0, y1 = want_bbox
    assert (outs[1][1][:, y0:y1, x0:x1] != outs[1][0][:, y0:y1, x0:x1]).any()


def test_argument_errors(pkg):
    lib = emu_lib()
    res = 64
    img, mask = np.zeros((3, 32, 32), dtype=np.uint8), np.zeros((32, 32), dtype=np.uint8)
    ok = items_of([img], [mask])
    scratch = np.zeros(lib.pipeline_batch_scratch_bytes(ok), dtype=np.uint8)
    x, y = np.zeros((1, 4, res, res), dtype=np.float32), np.zeros((2, 3, res, res), dtype=np.float32)
    bbox = np.zeros((1, 4), dtype=np.int32)
    out = np.full((2, 3, 32, 32), FILL, dtype=np.uint8)
    lib.pipeline_batch_pre(ok, res, 8, ptr(x), ptr(bbox), ptr(scratch))
    with pytest.raises(ValueError, match="samples"):
        lib.pipeline_batch_post_samples(ok, 0, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)])           # samples = 0
    with pytest.raises(ValueError, match="outs"):
        lib.pipeline_batch_post_samples(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), None)                 # null outs
    with pytest.raises(ValueError, match="destination"):
        lib.pipeline_batch_post_samples(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), [0])                  # a null entry
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_samples(ok, 2, 48, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)])            # resolution not a power of two
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_samples([(0,) + ok[0][1:]], 2, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)])   # null image pointer
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_samples(ok, 2, res, ptr(y), None, ptr(scratch), [ptr(out)])                # null box table
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_samples([], 2, res, ptr(y), ptr(bbox), ptr(scratch), [])                   # n = 0
    assert (out == FILL).all()                                                                            # nothing was launched
    lib.pipeline_batch_post_samples(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)])               # and the good call goes through
    assert list(bbox[0]) == [0, 32, 0, 32] and not (out == FILL).any()
