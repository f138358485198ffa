"""The batch form of the deployed pipeline (migan_pipeline_batch_pre / _post: N images of different sizes, boxes on the device,
one fused LDS-tiled post kernel) run on the CPU through the fiber emulator, against the single-image path it must reproduce byte
for byte (migan_pipeline_bbox / _pre / _post), the oracle's boxes and the reference goldens.  The generator is not under test:
y is seeded random, N(0, 0.6), or the oracle generator's output for the goldens."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from oracle import migan_torch_cpu as torc
from tests.emu_util import emu_lib, ptr
from tests.pipeline_batch_case import five_items

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN, "pipeline_r256_*.npz"))) + [os.path.join(GOLDEN, "pipeline_r64_freeform.npz")]
GAUSS = po.gaussian_kernel().flatten().tolist()
TILE_W, TILE_H = 32, 8                       # pipe_post_batch_kernel's tile (migan_pipeline.hpp: kPostTW, kPostTH)


def items_of(images, masks):
    return [(ptr(img), ptr(m), img.shape[1], img.shape[2], m.shape[0], m.shape[1]) for img, m in zip(images, masks)]


def batch_pre(lib, images, masks, res, padding):
    """-> items, scratch, bbox [n, 4], x [n, 4, R, R]; host buffers stand in for device memory under the emulator"""
    items = items_of(images, masks)
    scratch = np.zeros(lib.pipeline_batch_scratch_bytes(items), dtype=np.uint8)
    bbox = np.full((len(items), 4), -7, dtype=np.int32)
    x = np.zeros((len(items), 4, res, res), dtype=np.float32)
    lib.pipeline_batch_pre(items, res, padding, ptr(x), ptr(bbox), ptr(scratch))
    return items, scratch, bbox, x


def run_batch(lib, images, masks, y, res, padding, gauss=None):
    """images [3, H, W] uint8 each (modified in place), masks [h, w] uint8 each, y [n, 3, R, R]"""
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, padding)
    lib.pipeline_batch_post(items, res, ptr(y), ptr(bbox), ptr(scratch), gauss25=gauss)
    return bbox, x


def run_single(lib, image, mask, y1, res, padding, gauss=None):
    """the existing migan_pipeline_bbox / _pre / _post sequence on one image (modified in place); y1 [1, 3, R, R]"""
    h, w = mask.shape
    scratch = np.zeros(lib.pipeline_scratch_bytes(h, w), dtype=np.uint8)
    bbox = lib.pipeline_bbox(ptr(mask), h, w, res, padding, ptr(scratch))
    x = np.zeros((1, 4, res, res), dtype=np.float32)
    lib.pipeline_pre(ptr(image), ptr(mask), h, w, bbox, res, ptr(x))
    lib.pipeline_post(ptr(image), ptr(mask), h, w, bbox, res, ptr(np.ascontiguousarray(y1)), ptr(scratch), gauss25=gauss)
    return bbox, x


def check_against_single(lib, images, masks, y, res, padding):
    """boxes = oracle's = pipeline_bbox's; x = pipeline_pre's; every byte = the single-image sequence with the same y, with the
    built-in gaussian and with the oracle's weights; pixels outside each box unchanged.  Returns the boxes."""
    boxes = None
    for gauss in (None, GAUSS):
        got = [np.array(img, copy=True) for img in images]
        bbox, x = run_batch(lib, got, masks, y, res, padding, gauss=gauss)
        for i, (img, mask) in enumerate(zip(images, masks)):
            want = np.array(img, copy=True)
            wbox, wx = run_single(lib, want, mask, y[i:i + 1], res, padding, gauss=gauss)
            _, obox, _ = po.pipeline(img, mask[None], lambda t: torch.from_numpy(y[i:i + 1]), res, padding)
            assert list(bbox[i]) == list(wbox) == list(obox), f"item {i}"
            np.testing.assert_array_equal(x[i:i + 1], wx, err_msg=f"item {i}")
            np.testing.assert_array_equal(got[i], want, err_msg=f"item {i}")
            x0, x1, y0, y1 = wbox
            outside = np.ones(mask.shape, dtype=bool)
            outside[y0:y1, x0:x1] = False
            np.testing.assert_array_equal(got[i][:, outside], img[:, outside], err_msg=f"item {i}")
        boxes = bbox
    return boxes


def test_batch_is_byte_identical_to_the_single_image_path(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(21)
    res, padding = 64, 8
    images, masks = five_items(rng)
    y = (rng.standard_normal((5, 3, res, res)) * 0.6).astype(np.float32)
    boxes = check_against_single(lib, images, masks, y, res, padding)
    x0, x1, y0, y1 = boxes[4]
    assert (x1 - x0) % TILE_W != 0 and (y1 - y0) % TILE_H != 0
    assert (x1 - x0) > TILE_W and (y1 - y0) > TILE_H                  # more than one tile each way


def test_smallest_images(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(22)
    res = 8
    images = [rng.integers(0, 256, (3, 3, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)]
    masks = [np.full((3, 3), 255, dtype=np.uint8), np.full((5, 7), 255, dtype=np.uint8)]
    masks[0][1, 1] = 0
    masks[1][1:4, 2:6] = 0
    y = (rng.standard_normal((2, 3, res, res)) * 0.6).astype(np.float32)
    check_against_single(lib, images, masks, y, res, 0)


def test_masks_of_another_size_are_resized_first(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(23)
    res, padding = 64, 8
    sizes = [(96, 80), (50, 70), (64, 48)]
    msizes = [(37, 53), (128, 128), (64, 48)]                         # half size / odd aspect, larger, same
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = []
    for mh, mw in msizes:
        m = np.full((mh, mw), 255, dtype=np.uint8)
        m[mh // 3:mh // 3 * 2, mw // 4:mw // 2] = 0
        m[rng.random((mh, mw)) > 0.97] = 0
        masks.append(m)
    y = (rng.standard_normal((3, 3, res, res)) * 0.6).astype(np.float32)
    resized = [np.ascontiguousarray(po.tv_resize(torch.from_numpy(m)[None, None], s, "nearest")[0, 0].numpy()) for m, s in zip(masks, sizes)]
    a = [np.array(img, copy=True) for img in images]
    b = [np.array(img, copy=True) for img in images]
    abox, ax = run_batch(lib, a, masks, y, res, padding)
    bbox, bx = run_batch(lib, b, resized, y, res, padding)
    np.testing.assert_array_equal(abox, bbox)
    np.testing.assert_array_equal(ax, bx)
    for i in range(3):
        np.testing.assert_array_equal(a[i], b[i], err_msg=f"item {i}")
        assert (a[i] != images[i]).any()


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[9:-4] for p in GOLDENS])
def test_goldens_as_one_item_of_a_batch(pkg, path):
    g = np.load(path)
    res, seed, padding = int(g["resolution"]), int(g["seed"]), int(g["padding"])
    sd = pkg.synth.make_state_dict(res, seed=seed, regime="export")
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    lib = emu_lib()
    rng = np.random.default_rng(24)
    # the generator is not under test: y of the golden item is the oracle generator's output for the ORACLE's x
    _, want_bbox, want_x = po.pipeline(g["image"], g["mask"], lambda t: torch.zeros((1, 3, res, res)), res, padding)
    y = (rng.standard_normal((3, 3, res, res)) * 0.6).astype(np.float32)
    y[1] = np.asarray(torc.generator(want_x, sd, res), dtype=np.float32)[0]
    images = [rng.integers(0, 256, (3, 45, 61), dtype=np.uint8), np.array(g["image"], copy=True), rng.integers(0, 256, (3, 33, 19), dtype=np.uint8)]
    masks = [np.full((45, 61), 255, dtype=np.uint8), np.ascontiguousarray(g["mask"][0]), np.zeros((33, 19), dtype=np.uint8)]
    masks[0][10:30, 5:50] = 0
    bbox, x = run_batch(lib, images, masks, y, res, padding, gauss=GAUSS)
    assert list(bbox[1]) == [int(v) for v in g["bbox"]] == list(want_bbox)
    np.testing.assert_array_equal(x[1:2, :, ::7, ::5], g["x_strided"])
    np.testing.assert_array_equal(images[1], g["result"])


def test_more_items_than_one_launch_carries(pkg):
    """35 items through the C ABI (launches of 32 + 3) == 35 single-image calls"""
    lib = emu_lib()
    rng = np.random.default_rng(25)
    res, n = 8, 35
    sizes = [(3 + i % 10, 3 + (i * 3) % 7) for i in range(n)]        # 3 x 3 ... 12 x 9
    assert (3, 3) in sizes and (12, 9) in sizes
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.ascontiguousarray((rng.random(s) > 0.3).astype(np.uint8) * 255) for s in sizes]
    y = (rng.standard_normal((n, 3, res, res)) * 0.6).astype(np.float32)
    got = [np.array(img, copy=True) for img in images]
    bbox, x = run_batch(lib, got, masks, y, res, 1)
    for i in range(n):
        want = np.array(images[i], copy=True)
        wbox, wx = run_single(lib, want, masks[i], y[i:i + 1], res, 1)
        assert list(bbox[i]) == list(wbox), f"item {i}"
        np.testing.assert_array_equal(x[i:i + 1], wx, err_msg=f"item {i}")
        np.testing.assert_array_equal(got[i], want, err_msg=f"item {i}")


def test_a_box_that_does_not_fit_its_image_is_left_alone(pkg):
    """CPU only.  The boxes reach _post through device memory, so the host cannot refuse one: an item whose row lies outside its
    image, or is smaller than 3 x 3, stays unchanged, and the other item of the batch is processed normally."""
    lib = emu_lib()
    rng = np.random.default_rng(26)
    res, padding = 8, 2
    sizes = [(20, 24), (17, 40), (31, 23)]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m in masks:
        m[5:12, 6:15] = 0
    y = (rng.standard_normal((3, 3, res, res)) * 0.6).astype(np.float32)
    got = [np.array(img, copy=True) for img in images]
    items, scratch, bbox, _ = batch_pre(lib, got, masks, res, padding)
    good = [int(v) for v in bbox[2]]
    bbox[0] = (4, 24 + 5, 0, 20)                                      # x_max beyond the 24 columns
    bbox[1] = (6, 8, 5, 7)                                            # 2 x 2
    lib.pipeline_batch_post(items, res, ptr(y), ptr(bbox), ptr(scratch))
    np.testing.assert_array_equal(got[0], images[0])
    np.testing.assert_array_equal(got[1], images[1])
    want = np.array(images[2], copy=True)
    wbox, _ = run_single(lib, want, masks[2], y[2:3], res, padding)
    assert list(wbox) == good
    np.testing.assert_array_equal(got[2], want)
    assert (want != images[2]).any()


def test_batch_argument_errors(pkg):
    lib = emu_lib()
    res = 64
    img, mask = np.zeros((3, 32, 32), dtype=np.uint8), np.zeros((32, 32), dtype=np.uint8)
    ok = items_of([img], [mask])
    scratch = np.zeros(lib.pipeline_batch_scratch_bytes(ok), dtype=np.uint8)
    x, y = np.zeros((1, 4, res, res), dtype=np.float32), np.zeros((1, 3, res, res), dtype=np.float32)
    bbox = np.zeros((1, 4), dtype=np.int32)
    thin_img, thin_mask = np.zeros((3, 2, 32), dtype=np.uint8), np.zeros((2, 32), dtype=np.uint8)
    with pytest.raises(ValueError):
        lib.pipeline_batch_scratch_bytes([])                                                 # n = 0
    with pytest.raises(ValueError):
        lib.pipeline_batch_pre([], res, 8, ptr(x), ptr(bbox), ptr(scratch))
    with pytest.raises(ValueError):
        lib.pipeline_batch_pre(items_of([thin_img], [thin_mask]), res, 8, ptr(x), ptr(bbox), ptr(scratch))   # a 2 x 32 image
    with pytest.raises(ValueError):
        lib.pipeline_batch_scratch_bytes(items_of([thin_img], [thin_mask]))
    with pytest.raises(ValueError):
        lib.pipeline_batch_pre(ok, 48, 8, ptr(x), ptr(bbox), ptr(scratch))                   # resolution not a power of two
    with pytest.raises(ValueError):
        lib.pipeline_batch_post(ok, 48, ptr(y), ptr(bbox), ptr(scratch))
    with pytest.raises(ValueError):
        lib.pipeline_batch_pre(ok, res, -1, ptr(x), ptr(bbox), ptr(scratch))                 # negative padding
    null_image = [(0,) + ok[0][1:]]
    with pytest.raises(ValueError):
        lib.pipeline_batch_pre(null_image, res, 8, ptr(x), ptr(bbox), ptr(scratch))          # null image pointer
    with pytest.raises(ValueError):
        lib.pipeline_batch_post(null_image, res, ptr(y), ptr(bbox), ptr(scratch))
    with pytest.raises(ValueError):
        lib.pipeline_batch_post(ok, res, ptr(y), None, ptr(scratch))                         # null box table
    lib.pipeline_batch_pre(ok, res, 8, ptr(x), ptr(bbox), ptr(scratch))                      # and the good call goes through
    assert list(bbox[0]) == [0, 32, 0, 32]
