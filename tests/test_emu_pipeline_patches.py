"""migan_pipeline_batch_post_patches (the completions of every photo as box-sized patches, written by one kernel that tiles the CROP)
run on the CPU through the fiber emulator, product kernel source.  The yardstick of every byte comparison is
migan_pipeline_batch_post_samples' output for the same arguments, cropped to the box.  The generator is not under test: y is
seeded random, N(0, 0.6).  Every destination starts as FILL and has GUARD more bytes behind its capacity."""

import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests.emu_util import emu_lib, ptr
from tests.pipeline_patches_case import (BAD_BOXES, FILL, GUARD, TILE_H, TILE_W, case_clipped, case_five, case_resized_masks, case_smallest,
                                         case_three, case_two_launches, crop, patch_bytes, patch_view, random_y)
from tests.test_emu_pipeline_batch import GAUSS, batch_pre, items_of
from tests.test_emu_pipeline_samples import post_samples


def post_patches(lib, items, scratch, bbox, y, samples, res, gauss=None, sizes=None, capacities=None):
    """-> flat destinations of sizes[i] + GUARD bytes, all FILL before the call (sizes: by default exactly each patch; capacities:
    what the call is told, by default the sizes)"""
    sizes = [patch_bytes(b, samples) for b in bbox] if sizes is None else sizes
    bufs = [np.full(n + GUARD, FILL, dtype=np.uint8) for n in sizes]
    lib.pipeline_batch_post_patches(items, samples, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(b) for b in bufs],
                                    sizes if capacities is None else capacities, gauss25=gauss)
    return bufs


class Unchanged:
    """images, masks, bbox and x before a call; check() after it"""

    def __init__(self, images, masks, bbox, x):
        self.now = list(images) + list(masks) + [bbox, x]
        self.then = [np.array(a, copy=True) for a in self.now]

    def check(self):
        for k, (a, b) in enumerate(zip(self.now, self.then)):
            np.testing.assert_array_equal(a, b, err_msg=f"input {k} of images + masks + [bbox, x] was written")


def check_against_samples(lib, case, y, gausses=(None, GAUSS)):
    """every patch == the samples form's destination cropped to the box, whole arrays; the bytes behind the capacity, the images, the
    masks, the boxes and x untouched.  Returns the boxes and the patches."""
    images, masks, res, samples = case["images"], case["masks"], case["res"], case["samples"]
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, case["padding"])
    same = Unchanged(images, masks, bbox, x)
    patches = None
    for gauss in gausses:
        want = post_samples(lib, items, scratch, bbox, images, y, samples, res, gauss)
        bufs = post_patches(lib, items, scratch, bbox, y, samples, res, gauss)
        patches = [patch_view(b, box, samples) for b, box in zip(bufs, bbox)]
        for i in range(len(images)):
            np.testing.assert_array_equal(patches[i], crop(want[i], bbox[i]), err_msg=f"item {i}")
            assert (bufs[i][-GUARD:] == FILL).all(), f"item {i}: bytes behind the capacity were written"
        same.check()
    return bbox, patches


def test_five_items_three_samples(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(61)
    case = case_five(rng)
    boxes, patches = check_against_samples(lib, case, random_y(rng, 5, case["samples"], case["res"]))
    for i, mask in enumerate(case["masks"]):
        assert list(boxes[i]) == list(po.masked_bbox(mask, case["res"], case["padding"])), f"item {i}"
    # the case holds a crop that is no multiple of the tile in either direction and spans several tiles each way (item 4, 66 x 66),
    # and one of several tile columns whose last is partial (item 3, 150 x 40); the boxes of the other three are 64 x 64
    x0, x1, y0, y1 = (int(v) for v in boxes[4])
    assert (x1 - x0) % TILE_W != 0 and (y1 - y0) % TILE_H != 0 and x1 - x0 > TILE_W and y1 - y0 > TILE_H
    x0, x1, y0, y1 = (int(v) for v in boxes[3])
    assert (x1 - x0) % TILE_W != 0 and x1 - x0 > TILE_W and y1 - y0 > TILE_H
    assert (patches[4][0] != patches[4][1]).any() and (patches[4][1] != patches[4][2]).any()      # different y: different patches


def test_one_sample(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(62)
    case = dict(case_five(rng), samples=1)
    check_against_samples(lib, case, random_y(rng, 5, 1, case["res"]))


def test_smallest_images(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(63)
    case = case_smallest(rng)
    boxes, patches = check_against_samples(lib, case, random_y(rng, 2, case["samples"], case["res"]))
    assert [list(b) for b in boxes] == [[0, 3, 0, 3], [0, 7, 0, 5]]
    assert (patches[1][0] != patches[1][1]).any()     # (the 3 x 3 image's pooled mask is 255 everywhere: its patches are the image)


def test_masks_of_another_size_are_resized_first(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(64)
    case = case_resized_masks(rng)
    sizes = [img.shape[1:] for img in case["images"]]
    y = random_y(rng, 3, case["samples"], case["res"])
    resized = [np.ascontiguousarray(po.tv_resize(torch.from_numpy(m)[None, None], s, "nearest")[0, 0].numpy())
               for m, s in zip(case["masks"], sizes)]
    abox, a = check_against_samples(lib, case, y, gausses=(None,))
    bbox, b = check_against_samples(lib, dict(case, masks=resized), y, gausses=(None,))
    np.testing.assert_array_equal(abox, bbox)
    for i in range(3):
        np.testing.assert_array_equal(a[i], b[i], err_msg=f"item {i}")
        assert (a[i][0] != a[i][1]).any()


def test_more_items_than_one_launch_carries(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(65)
    case = case_two_launches(rng)
    assert len(case["images"]) == 33
    _, patches = check_against_samples(lib, case, random_y(rng, 33, case["samples"], case["res"]), gausses=(None,))
    assert (patches[32][0] != patches[32][1]).any()


def test_a_box_clipped_at_an_image_corner(pkg):
    lib = emu_lib()
    rng = np.random.default_rng(66)
    case = case_clipped(rng)
    boxes, patches = check_against_samples(lib, case, random_y(rng, 2, case["samples"], case["res"]))
    assert [list(b) for b in boxes] == [[0, 34, 0, 27], [0, 25, 16, 45]]          # at (0, 0); ending at (W, H) = (25, 45); not square
    for i, mask in enumerate(case["masks"]):
        assert list(boxes[i]) == list(po.masked_bbox(mask, case["res"], case["padding"])), f"item {i}"
        assert (patches[i][0] != patches[i][1]).any()


def test_a_box_that_does_not_fit_its_image_is_skipped(pkg):
    """The boxes reach the kernel through device memory, so the host cannot refuse one.  An item whose row lies outside its image, or
    is smaller than 3 x 3, has no patch: its destination (sized by the bound S * 3 * H * W) keeps every byte.  The good item of the
    batch is processed."""
    lib = emu_lib()
    rng = np.random.default_rng(67)
    case = case_three(rng)
    images, masks, res, samples = case["images"], case["masks"], case["res"], case["samples"]
    y = random_y(rng, 3, samples, res)
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, case["padding"])
    for i, row in BAD_BOXES.items():
        bbox[i] = row
    same = Unchanged(images, masks, bbox, x)
    sizes = [samples * img.size for img in images[:2]] + [patch_bytes(bbox[2], samples)]
    bufs = post_patches(lib, items, scratch, bbox, y, samples, res, sizes=sizes)
    want = post_samples(lib, items, scratch, bbox, images, y, samples, res)
    assert (bufs[0] == FILL).all() and (bufs[1] == FILL).all()
    np.testing.assert_array_equal(patch_view(bufs[2], bbox[2], samples), crop(want[2], bbox[2]))
    assert (bufs[2][-GUARD:] == FILL).all()
    assert (crop(want[2], bbox[2]) != crop(np.stack([images[2]] * samples), bbox[2])).any()
    same.check()


def test_a_capacity_one_byte_short_skips_the_item(pkg):
    """the middle item is told one byte less than its patches take: nothing of it is written, not even the bytes that fit"""
    lib = emu_lib()
    rng = np.random.default_rng(68)
    case = case_three(rng)
    images, masks, res, samples = case["images"], case["masks"], case["res"], case["samples"]
    y = random_y(rng, 3, samples, res)
    items, scratch, bbox, x = batch_pre(lib, images, masks, res, case["padding"])
    same = Unchanged(images, masks, bbox, x)
    sizes = [patch_bytes(b, samples) for b in bbox]
    capacities = [sizes[0], sizes[1] - 1, sizes[2]]
    bufs = post_patches(lib, items, scratch, bbox, y, samples, res, sizes=sizes, capacities=capacities)
    want = post_samples(lib, items, scratch, bbox, images, y, samples, res)
    assert (bufs[1] == FILL).all()
    for i in (0, 2):
        np.testing.assert_array_equal(patch_view(bufs[i], bbox[i], samples), crop(want[i], bbox[i]), err_msg=f"item {i}")
        assert (bufs[i][-GUARD:] == FILL).all()
    same.check()
    # and a capacity of 0 with a null destination is such an item too
    out0, out2 = np.full(sizes[0], FILL, dtype=np.uint8), np.full(sizes[2], FILL, dtype=np.uint8)
    lib.pipeline_batch_post_patches(items, samples, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out0), 0, ptr(out2)], [sizes[0], 0, sizes[2]])
    np.testing.assert_array_equal(out0, bufs[0][:sizes[0]])
    np.testing.assert_array_equal(out2, bufs[2][:sizes[2]])


def test_exact_capacity_leaves_the_guard_intact(pkg):
    """capacity == S * 3 * ch * cw exactly: every byte of it is written once (two different fills agree), none behind it"""
    lib = emu_lib()
    rng = np.random.default_rng(69)
    case = case_five(rng)
    images, masks, res, samples = case["images"], case["masks"], case["res"], case["samples"]
    y = random_y(rng, 5, samples, res)
    items, scratch, bbox, _ = batch_pre(lib, images, masks, res, case["padding"])
    sizes = [patch_bytes(b, samples) for b in bbox]
    got = []
    for fill in (FILL, 0x5A):
        bufs = [np.full(n + GUARD, fill, dtype=np.uint8) for n in sizes]
        lib.pipeline_batch_post_patches(items, samples, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(b) for b in bufs], sizes)
        for i, b in enumerate(bufs):
            assert (b[sizes[i]:] == fill).all(), f"item {i}: the guard behind the capacity was written"
        got.append([b[:n] for b, n in zip(bufs, sizes)])
    for i in range(5):
        np.testing.assert_array_equal(got[0][i], got[1][i], err_msg=f"item {i}: a byte inside the capacity was not written")


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
        lib.pipeline_batch_post_patches(ok, 0, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)], [out.size])          # samples = 0
    with pytest.raises(ValueError, match="outs"):
        lib.pipeline_batch_post_patches(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), None, [out.size])                # null outs
    with pytest.raises(ValueError, match="out_bytes"):
        lib.pipeline_batch_post_patches(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)], None)                # null out_bytes
    with pytest.raises(ValueError, match="destination"):
        lib.pipeline_batch_post_patches(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), [0], [out.size])                 # null entry, capacity > 0
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_patches(ok, 2, 48, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)], [out.size])           # resolution not a power of two
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_patches([(0,) + ok[0][1:]], 2, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)], [out.size])   # null image pointer
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_patches(ok, 2, res, ptr(y), None, ptr(scratch), [ptr(out)], [out.size])               # null box table
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_patches(ok, 2, res, None, ptr(bbox), ptr(scratch), [ptr(out)], [out.size])            # null y
    with pytest.raises(ValueError):
        lib.pipeline_batch_post_patches([], 2, res, ptr(y), ptr(bbox), ptr(scratch), [], [])                          # n = 0
    assert (out == FILL).all()                                                                                       # nothing was launched
    lib.pipeline_batch_post_patches(ok, 2, res, ptr(y), ptr(bbox), ptr(scratch), [ptr(out)], [out.size])              # and the good call goes through
    assert list(bbox[0]) == [0, 32, 0, 32] and not (out == FILL).any()
