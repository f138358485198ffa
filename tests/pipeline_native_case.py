"""The cases and the oracle shared by tests/test_emu_pipeline_native.py and tests/test_gpu_pipeline_native.py (crops at native size:
include/migan_pipeline_native_hip.h, MIGAN_Pipeline.forward_native).  Test infrastructure only.

The oracle needs nothing new.  The network input is the closed form in numpy float32 -- x = (m - 0.5, (image * 2 / 255 - 1) * m) with
m = mask / 255 inside the box, (-0.5, 0, 0, 0) in the rest of the window -- and the result is po.postprocess(crop, crop mask, y) of
the pipeline oracle, whose resize of y to the crop's size is the identity when y has that size already, pasted where the label map
equals the row's label.  Every comparison is byte for byte (x: bit for bit against the existing kernels, value for value against the
closed form).  The generator is not under test at this level: y is seeded random.

Every check takes (lib, bufs): the library under test and where its buffers live (pipeline_regions_case.Buffers)."""
import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests import pipeline_regions_case as rc

RES, PADDING, GAUSS = rc.RES, rc.PADDING, rc.GAUSS
Buffers = rc.Buffers


def random_y(rng, rows, hc, wc):
    return (rng.standard_normal((rows, 3, hc, wc)) * 0.6).astype(np.float32)


def photo(seed, h, w, holes, gray=False):
    """a seeded random photo [3, h, w] and its mask: 255 but for the `holes` (y0, y1, x0, x1), which are 0 (gray: 0 ... 254).

    The photo's bytes are 1 ... 254.  The kernels sum the 25 products of the blur in fp64 and round once (the definition, shared with
    every post kernel); the oracle's blur is ATen's fp32 conv2d, whose order of summation is its own, and the two feathered masks
    can differ in the last bit.  That reaches a byte only where the blend is an integer in exact arithmetic, image == output, which
    for a random y means a saturated output (0 or 255) over a photo byte of the same value: 255 mk + 255 (1 - mk) is 255 or
    254.99998.  It says nothing about these kernels, so the photos here keep off the two values."""
    rng = np.random.default_rng(seed)
    image = rng.integers(1, 255, (3, h, w), dtype=np.uint8)
    mask = np.full((h, w), 255, dtype=np.uint8)
    for y0, y1, x0, x1 in holes:
        mask[y0:y1, x0:x1] = rng.integers(0, 255, (y1 - y0, x1 - x0), dtype=np.uint8) if gray else 0
    return image, mask


def oracle_x(image, mask, box, hc, wc):
    """the closed form: [4, hc, wc] float32"""
    x0, x1, y0, y1 = box
    m = mask[y0:y1, x0:x1].astype(np.float32) / np.float32(255)
    rgb = image[:, y0:y1, x0:x1].astype(np.float32) * np.float32(2) / np.float32(255) - np.float32(1)
    x = np.zeros((4, hc, wc), dtype=np.float32)
    x[0] = -0.5
    x[0, :y1 - y0, :x1 - x0] = m - np.float32(0.5)
    x[1:, :y1 - y0, :x1 - x0] = rgb * m
    return x


def oracle_post(image, mask, labels, rows, y, out=None):
    """-> the image after every row (label, box) with its y row [3, hc, wc]: po.postprocess of the crop with the part of y that lies
    over it, every crop taken from the ORIGINAL image, pasted where labels == label (everywhere in the box for label 0) into `out`
    (default: a copy of the image)"""
    out = np.array(image, copy=True) if out is None else out
    for (label, (x0, x1, y0, y1)), yr in zip(rows, y):
        ci = torch.from_numpy(image[None, :, y0:y1, x0:x1].copy())
        cm = torch.from_numpy(mask[None, None, y0:y1, x0:x1].copy())
        part = np.ascontiguousarray(yr[None, :, :y1 - y0, :x1 - x0])
        assert not np.isnan(part).any()
        done = po.postprocess(ci, cm, torch.from_numpy(part))[0].numpy()
        sel = np.ones((y1 - y0, x1 - x0), dtype=bool) if label == 0 else labels[y0:y1, x0:x1] == label
        out[:, y0:y1, x0:x1][:, sel] = done[:, sel]
    return out


class Scene:
    """one photo on the device: image (a fresh copy), mask and, when given, the label map"""

    def __init__(self, bufs, image, mask, labels=None):
        self.bufs, self.image0, self.mask, self.labels = bufs, image, mask, labels
        self.image_dev, self.mask_dev = bufs.to_dev(image), bufs.to_dev(mask)
        self.labels_dev = None if labels is None else bufs.to_dev(labels)

    def row(self, label, box):
        h, w = self.mask.shape
        return (self.bufs.ptr(self.image_dev), self.bufs.ptr(self.mask_dev), None if self.labels_dev is None else self.bufs.ptr(self.labels_dev),
                h, w, label, tuple(box))

    def image(self):
        return self.bufs.to_np(self.image_dev)


def run_pre(lib, bufs, scenes, rows, hc, wc, x_fill=7.0):
    """native_pre of rows [(scene index, label, box), ...] in one call -> x [m, 4, hc, wc] (it began as x_fill)"""
    x_dev = bufs.to_dev(np.full((len(rows), 4, hc, wc), x_fill, dtype=np.float32))
    lib.pipeline_native_pre([scenes[i].row(label, box) for i, label, box in rows], hc, wc, bufs.ptr(x_dev), bufs.stream)
    return bufs.to_np(x_dev)


def run_post(lib, bufs, scenes, rows, hc, wc, y):
    y_dev = bufs.to_dev(y)
    lib.pipeline_native_post([scenes[i].row(label, box) for i, label, box in rows], hc, wc, bufs.ptr(y_dev), GAUSS, bufs.stream)


def run_native(lib, bufs, scenes, rows, hc, wc, y):
    """both, one call each -> x"""
    x = run_pre(lib, bufs, scenes, rows, hc, wc)
    run_post(lib, bufs, scenes, rows, hc, wc, y)
    return x


def check_against_the_oracle(lib, bufs, image, mask, rows, hc, wc, labels=None, seed=3, nan_padding=False):
    """rows [(label, box), ...] of ONE photo in one call of each entry point: x against the closed form, every image byte against the oracle"""
    scene = Scene(bufs, image, mask, labels)
    y = random_y(np.random.default_rng(seed), len(rows), hc, wc)
    if nan_padding:
        for r, (_, (x0, x1, y0, y1)) in enumerate(rows):
            y[r, :, y1 - y0:, :] = np.nan
            y[r, :, :, x1 - x0:] = np.nan
    x = run_native(lib, bufs, [scene], [(0, label, box) for label, box in rows], hc, wc, y)
    for r, (_, box) in enumerate(rows):
        np.testing.assert_array_equal(x[r], oracle_x(image, mask, box, hc, wc), err_msg=f"x of row {r}")
    got = scene.image()
    np.testing.assert_array_equal(got, oracle_post(image, mask, labels, rows, y))
    return x, y, got


# ---- 1. anchor: an R x R window with an R x R box gives the bits of migan_pipeline_regions_pre / _post ---------------------------------
def check_anchor(lib, bufs):
    case = rc.CASES["three_blobs"]()
    image, mask = case["images"][0], case["full"][0]
    labels_np, count, boxes, _ = rc.run_find(lib, bufs, case, [bufs.to_dev(image)], [bufs.to_dev(case["masks"][0])])
    assert count[0] == 3
    k = 2
    box = tuple(int(v) for v in boxes[0, k])
    assert (box[1] - box[0], box[3] - box[2]) == (RES, RES) and image.shape[1:] == (157, 203)
    y = random_y(np.random.default_rng(11), 1, RES, RES)
    for label in (0, k):
        a, b = Scene(bufs, image, mask, labels_np[0]), Scene(bufs, image, mask, labels_np[0])
        x = run_native(lib, bufs, [a], [(0, label, box)], RES, RES, y)
        x_dev = bufs.to_dev(np.full((1, 4, RES, RES), 7.0, dtype=np.float32))
        lib.pipeline_regions_pre([b.row(label, box)], RES, bufs.ptr(x_dev), bufs.stream)
        y_dev = bufs.to_dev(y)
        lib.pipeline_regions_post([b.row(label, box)], RES, bufs.ptr(y_dev), GAUSS, bufs.stream)
        np.testing.assert_array_equal(x.view(np.uint32), bufs.to_np(x_dev).view(np.uint32), err_msg=f"label {label}: x bits")
        np.testing.assert_array_equal(a.image(), b.image(), err_msg=f"label {label}: image bytes")
        assert (a.image() != image).any(), "something was completed"
        np.testing.assert_array_equal(a.image(), oracle_post(image, mask, labels_np[0], [(label, box)], y))


# ---- 2. inside: a 48 x 80 window at an odd offset, the hole on the box's left border ------------------------------------------------------
def check_inside(lib, bufs):
    box = (31, 111, 23, 71)
    image, mask = photo(21, 157, 203, [(33, 53, 31, 56), (60, 71, 90, 100)], gray=True)
    assert (mask[23:71, 31] != 255).any() and (mask[70, 31:111] != 255).any(), "the hole touches the box's left and bottom borders"
    _, _, got = check_against_the_oracle(lib, bufs, image, mask, [(0, box)], 48, 80)
    outside = np.ones(mask.shape, dtype=bool)
    outside[23:71, 31:111] = False
    np.testing.assert_array_equal(got[:, outside], image[:, outside])
    assert (got != image).any()


# ---- 3. padded: the photo is smaller than the window ---------------------------------------------------------------------------------------
def check_padded(lib, bufs):
    image, mask = photo(22, 40, 50, [(10, 30, 20, 50), (36, 40, 3, 9)])
    x, _, got = check_against_the_oracle(lib, bufs, image, mask, [(0, (0, 50, 0, 40))], 48, 64, nan_padding=True)
    pad = np.ones((48, 64), dtype=bool)
    pad[:40, :50] = False
    assert (x[0, 0][pad] == -0.5).all() and (x[0, 1:][:, pad] == 0).all()
    assert (got != image).any()


# ---- 4. edges: boxes that are no multiple of the post tile, a 3 x 3 box, a width that is no multiple of 4, an x off the 16-byte grid -----
def check_edges(lib, bufs):
    image, mask = photo(23, 157, 203, [(105, 130, 20, 60), (155, 157, 200, 203)])
    # a 3 x 3 box in a 16 x 16 window at the photo's bottom right corner
    check_against_the_oracle(lib, bufs, image, mask, [(0, (200, 203, 154, 157))], 16, 16, nan_padding=True)
    # 45 x 70 in 48 x 72: four columns per thread, and the quad at columns 68 ... 71 straddles the box's border
    check_against_the_oracle(lib, bufs, image, mask, [(0, (5, 75, 100, 145))], 48, 72, nan_padding=True)
    # 45 x 67 in 47 x 70: one column per thread
    check_against_the_oracle(lib, bufs, image, mask, [(0, (5, 72, 100, 145))], 47, 70, nan_padding=True)
    # 33 x 65 in 33 x 65: the box is the window, one column past two tiles, one row past four
    check_against_the_oracle(lib, bufs, image, mask, [(0, (10, 75, 100, 133))], 33, 65)
    # a width that is a multiple of 4 with x one float off the 16-byte grid: one column per thread
    scene = Scene(bufs, image, mask)
    box, hc, wc = (5, 75, 100, 145), 48, 72
    flat = bufs.to_dev(np.full(4 * hc * wc + 4, 7.0, dtype=np.float32))
    assert bufs.ptr(flat) % 16 == 0
    lib.pipeline_native_pre([scene.row(0, box)], hc, wc, bufs.ptr(flat) + 4, bufs.stream)
    out = bufs.to_np(flat)
    np.testing.assert_array_equal(out[1:1 + 4 * hc * wc].reshape(4, hc, wc), oracle_x(image, mask, box, hc, wc))
    assert out[0] == 7.0 and (out[1 + 4 * hc * wc:] == 7.0).all()


# ---- 5. labels: two rows of one photo with overlapping boxes ---------------------------------------------------------------------------
def check_labels(lib, bufs):
    case = rc.CASES["overlapping_crops"]()
    image, mask, labels = case["images"][0], case["full"][0], case["found"][0]["labels"]
    rows = [(1, (3, 83, 2, 66)), (2, (28, 108, 5, 69))]                  # 64 x 80 windows; either covers a part of the other's region
    for (label, (x0, x1, y0, y1)), other in zip(rows, (2, 1)):
        inside = labels[y0:y1, x0:x1]
        assert (inside == label).any() and (inside == other).any()
    y = random_y(np.random.default_rng(5), 2, 64, 80)
    want = oracle_post(image, mask, labels, rows, y)
    both = Scene(bufs, image, mask, labels)
    run_native(lib, bufs, [both], [(0, label, box) for label, box in rows], 64, 80, y)
    np.testing.assert_array_equal(both.image(), want)
    for label in (1, 2):                                                 # each row stores only where its label is
        alone = Scene(bufs, image, mask, labels)
        run_native(lib, bufs, [alone], [(0,) + rows[label - 1]], 64, 80, y[label - 1:label])
        np.testing.assert_array_equal(alone.image()[:, labels != label], image[:, labels != label])
        np.testing.assert_array_equal(alone.image()[:, labels == label], want[:, labels == label])
    rev = Scene(bufs, image, mask, labels)
    run_native(lib, bufs, [rev], [(0, label, box) for label, box in rows[::-1]], 64, 80, np.ascontiguousarray(y[::-1]))
    np.testing.assert_array_equal(rev.image(), want)
    two = Scene(bufs, image, mask, labels)
    for r in (1, 0):
        run_native(lib, bufs, [two], [(0,) + rows[r]], 64, 80, y[r:r + 1])
    np.testing.assert_array_equal(two.image(), want)


# ---- 6. more rows than one launch carries ----------------------------------------------------------------------------------------------
def check_forty_rows(lib, bufs):
    case = rc.CASES["many_rows"]()
    hc, wc = 64, 68
    rows = []
    for i, found in enumerate(case["found"]):
        for r, (x0, x1, y0, y1) in enumerate(found["boxes"]):
            rows.append((i, r + 1, (x0, min(x1 + (r % 5), 160, x0 + wc), y0, y1 - (r % 3))))     # boxes of several sizes, all <= the window
    assert len(rows) == 40 and all(b[1] - b[0] <= wc and b[3] - b[2] <= hc for _, _, b in rows)
    y = random_y(np.random.default_rng(6), 40, hc, wc)
    scenes = [Scene(bufs, case["images"][i], case["full"][i], case["found"][i]["labels"]) for i in range(2)]
    x = run_native(lib, bufs, scenes, rows, hc, wc, y)
    singles = [Scene(bufs, case["images"][i], case["full"][i], case["found"][i]["labels"]) for i in range(2)]
    for r, row in enumerate(rows):                                       # (every input is formed before any result is stored)
        np.testing.assert_array_equal(x[r].view(np.uint32), run_pre(lib, bufs, singles, [row], hc, wc)[0].view(np.uint32), err_msg=f"row {r}")
    for r, row in enumerate(rows):
        run_post(lib, bufs, singles, [row], hc, wc, y[r:r + 1])
    for a, b, img in zip(scenes, singles, case["images"]):
        np.testing.assert_array_equal(a.image(), b.image())
        assert (a.image() != img).any()


# ---- 7. refusals: MIGAN_EINVAL with nothing launched -----------------------------------------------------------------------------------
def check_refusals(lib, bufs):
    image, mask = photo(24, 60, 70, [(20, 40, 20, 40)])
    labels = np.ones((60, 70), dtype=np.uint8)
    scene = Scene(bufs, image, mask, labels)
    hc, wc, box = 48, 64, (2, 66, 5, 53)
    x_dev = bufs.to_dev(np.full((1, 4, hc, wc), 3.0, dtype=np.float32))
    y_dev = bufs.to_dev(np.zeros((1, 3, hc, wc), dtype=np.float32))
    good = scene.row(1, box)
    bad_rows = [(0,) + good[1:],                                          # null image
                good[:1] + (0,) + good[2:],                               # null mask
                good[:2] + (0,) + good[3:],                               # label above 0 without a label map
                good[:3] + (2, 70, 1, box),                               # image below 3 x 3
                good[:3] + (1 << 15, 1 << 15, 1, box),                    # 2^30 pixels
                good[:5] + (65, box), good[:5] + (-1, box),               # label outside 0 ... 64
                good[:6] + ((0, 71, 5, 53),), good[:6] + ((-1, 60, 5, 53),), good[:6] + ((2, 66, 5, 61),),      # box outside the image
                good[:6] + ((5, 7, 5, 53),), good[:6] + ((2, 66, 5, 7),),                                       # box below 3 x 3
                good[:6] + ((2, 67, 5, 53),), good[:6] + ((2, 66, 5, 54),)]                                     # box wider / taller than the window
    calls = [([bad], hc, wc, False) for bad in bad_rows]
    calls += [([], hc, wc, False), (None, hc, wc, False), ([good], hc, wc, True),                               # no rows, null table, null tensor
              ([good], 0, wc, False), ([good], hc, 0, False), ([good], -1, wc, False), ([good], 1 << 14, 1 << 14, False)]   # the window
    for rows, h, w, null in calls:
        with pytest.raises(ValueError):
            lib.pipeline_native_pre(rows, h, w, None if null else bufs.ptr(x_dev), bufs.stream)
        with pytest.raises(ValueError):
            lib.pipeline_native_post(rows, h, w, None if null else bufs.ptr(y_dev), GAUSS, bufs.stream)
    assert (bufs.to_np(x_dev) == 3.0).all() and (scene.image() == image).all()
    lib.pipeline_native_pre([good[:2] + (0,) + good[3:5] + (0, box)], hc, wc, bufs.ptr(x_dev), bufs.stream)      # label 0 needs no label map
    assert not (bufs.to_np(x_dev) == 3.0).any()


CHECKS = {f.__name__[6:]: f for f in (check_anchor, check_inside, check_padded, check_edges, check_labels, check_forty_rows, check_refusals)}


# ---- the window rule ---------------------------------------------------------------------------------------------------------------------
# (box, H, W) -> (in-photo box, (Hc, Wc)) at R = 64, q = 16; boxes are {x_min, x_max, y_min, y_max}
WINDOW_TABLE = [
    (((60, 130, 50, 120), 157, 203), ((55, 135, 45, 125), (80, 80))),        # centred growth: 70 -> 80, 5 either side
    (((60, 131, 50, 121), 157, 203), ((56, 136, 46, 126), (80, 80))),        # odd growth, 71 -> 80: 4 before, 5 behind
    (((2, 72, 0, 70), 157, 203), ((0, 80, 0, 80), (80, 80))),                # clamped left / at the top
    (((133, 203, 87, 157), 157, 203), ((123, 203, 77, 157), (80, 80))),      # clamped right / at the bottom
    (((0, 50, 0, 40), 40, 50), ((0, 50, 0, 40), (48, 64))),                  # the photo is smaller than the window
    (((0, 70, 10, 74), 100, 70), ((0, 70, 10, 74), (64, 80))),               # narrower only: columns padded, rows kept
    (((10, 74, 20, 84), 157, 203), ((10, 74, 20, 84), (64, 64))),            # exact multiples unchanged: R x R stays R x R
    (((7, 103, 3, 51), 60, 110), ((7, 103, 3, 51), (48, 96))),               # exact multiples unchanged, non-square
    (((31, 64, 9, 52), 61, 67), ((19, 67, 7, 55), (48, 48))),                # odd sizes, 33 x 43: 24 clamped to 67 - 48; 9 - 2
    (((0, 67, 0, 61), 61, 67), ((0, 67, 0, 61), (64, 80))),                  # the box is the odd-sized photo
]


def check_window_properties(pipe, box, h, w):
    (x0, x1, y0, y1), (hc, wc) = pipe.native_window(box, h, w)
    q = pipe.res // 4
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h, "the box lies inside the photo"
    assert x1 - x0 <= wc and y1 - y0 <= hc and hc % q == 0 and wc % q == 0 and hc >= q and wc >= q
    assert x0 <= box[0] and box[1] <= x1 and y0 <= box[2] and box[3] <= y1, "it contains the input box"
    assert wc - (box[1] - box[0]) < q and hc - (box[3] - box[2]) < q, "no more than the rounding"
    assert (x1 - x0 == wc or (x0 == 0 and x1 == w)) and (y1 - y0 == hc or (y0 == 0 and y1 == h)), "padding only where the photo ends"
