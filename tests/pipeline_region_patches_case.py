"""The helpers and the oracle shared by tests/test_emu_pipeline_region_patches.py and tests/test_gpu_pipeline_region_patches.py
(S completions per hole region as patches, and the paste back: include/migan_pipeline_region_patches_hip.h,
MIGAN_Pipeline.forward_region_patches / paste_patches).  Test infrastructure only.

The cases, the region oracle and the buffer abstraction are tests/pipeline_regions_case.py's, unchanged.  The oracle for patch (r, s)
is the crop at row r's box of oracle_post(image, full mask, labels, [row r], y[r * S + s : r * S + s + 1]): the existing oracle
applied with that row alone to the ORIGINAL photo.  Every destination starts as FILL and has GUARD more bytes behind its capacity.
The generator is not under test: y is seeded random."""
import functools

import numpy as np

from tests import pipeline_regions_case as rc
from tests.pipeline_regions_case import CASES, GAUSS, Buffers, host_rows, oracle_post, random_y, run_find   # noqa: F401 (re-exported)

FILL = 0xA5                                  # every destination starts as this: an unwritten or over-written byte shows
GUARD = 64                                   # bytes behind every destination's capacity, FILL before and after the call
TILE_W, TILE_H = 32, 8                       # pipe_post_rows_patches_kernel's tile (migan_pipeline.hpp: kPostTW, kPostTH)
Y_SEED = 11


def flat_rows(case):
    """[(image index, label, box)] of all images, by the oracle's "when not to split" rule"""
    return [(i, label, box) for i, found in enumerate(case["found"]) for label, box in rc.rows_of(found)]


def patch_bytes(box, samples):
    x0, x1, y0, y1 = box
    return samples * 3 * (y1 - y0) * (x1 - x0)


@functools.lru_cache(maxsize=None)
def reference(name, samples, y_seed=Y_SEED):
    """-> y [rows * S, 3, R, R] and, per row, the oracle's patches uint8 [S, 3, ch, cw].  Computed once per (case, S, seed) and
    shared by the tests: treat both as read-only."""
    case = CASES[name]()
    flat = flat_rows(case)
    y = random_y(np.random.default_rng(y_seed), len(flat) * samples)
    want = []
    for r, (i, label, (x0, x1, y0, y1)) in enumerate(flat):
        per = []
        for s in range(samples):
            at = r * samples + s
            done = oracle_post(case["images"][i], case["full"][i], case["found"][i]["labels"], [(label, (x0, x1, y0, y1))], y[at:at + 1])
            per.append(done[:, y0:y1, x0:x1])
        want.append(np.stack(per))
    return y, want


class Prepared:
    """a case on the buffers of `bufs`, through migan_pipeline_regions_find: images, masks at the images' sizes, label maps, the flat
    row list [(image index, label, box)] (checked against the oracle's) and the rows' table for the C ABI"""

    def __init__(self, lib, bufs, case):
        self.lib, self.bufs, self.case = lib, bufs, case
        self.images_dev = [bufs.to_dev(a) for a in case["images"]]
        self.full_dev = [bufs.to_dev(m) for m in case["full"]]
        masks_dev = [bufs.to_dev(m) for m in case["masks"]]
        self.labels, count, boxes, self.labels_dev = run_find(lib, bufs, case, self.images_dev, masks_dev)
        rows = host_rows(case, count, boxes)
        self.flat = [(i, label, box) for i, rs in enumerate(rows) for label, box in rs]
        assert self.flat == flat_rows(case)
        self.table = [self.row(r) for r in range(len(self.flat))]

    def row(self, r, image=None):
        i, label, box = self.flat[r]
        img = self.images_dev[i] if image is None else image
        return (self.bufs.ptr(img), self.bufs.ptr(self.full_dev[i]), self.bufs.ptr(self.labels_dev[i]), self.case["images"][i].shape[1],
                self.case["images"][i].shape[2], label, box)

    def assert_inputs_untouched(self):
        for i, img in enumerate(self.case["images"]):
            np.testing.assert_array_equal(self.bufs.to_np(self.images_dev[i]), img, err_msg=f"image {i} was written")
            np.testing.assert_array_equal(self.bufs.to_np(self.full_dev[i]), self.case["full"][i], err_msg=f"mask {i} was written")
            np.testing.assert_array_equal(self.bufs.to_np(self.labels_dev[i]), self.labels[i], err_msg=f"label map {i} was written")


def post_patches(prep, y_dev, samples, rows=None, sizes=None, capacities=None, gauss=GAUSS, fill=FILL):
    """migan_pipeline_regions_post_patches on rows (default: all) -> flat destinations of sizes[r] + GUARD bytes, all `fill` before"""
    rows = list(range(len(prep.flat))) if rows is None else rows
    sizes = [patch_bytes(prep.flat[r][2], samples) for r in rows] if sizes is None else sizes
    outs = [prep.bufs.to_dev(np.full(n + GUARD, fill, dtype=np.uint8)) for n in sizes]
    prep.lib.pipeline_regions_post_patches([prep.table[r] for r in rows], samples, prep.case["res"], prep.bufs.ptr(y_dev),
                                           [prep.bufs.ptr(o) for o in outs], sizes if capacities is None else capacities, gauss,
                                           prep.bufs.stream)
    return outs


def patch_view(buf_np, box, samples):
    x0, x1, y0, y1 = box
    return buf_np[:patch_bytes(box, samples)].reshape(samples, 3, y1 - y0, x1 - x0)


def check_case(lib, bufs, name, samples, y_seed=Y_SEED):
    """every patch of every row against the oracle, whole arrays; the guard bytes, the photos, masks, label maps and y untouched.
    Returns dict(prep, y, y_dev, outs (the device destinations), patches (numpy, per row [S, 3, ch, cw]))"""
    case = CASES[name]()
    y, want = reference(name, samples, y_seed)
    prep = Prepared(lib, bufs, case)
    y_dev = bufs.to_dev(y)
    outs = post_patches(prep, y_dev, samples) if prep.flat else []
    patches = []
    for r, (i, label, box) in enumerate(prep.flat):
        got = bufs.to_np(outs[r])
        n = patch_bytes(box, samples)
        np.testing.assert_array_equal(patch_view(got, box, samples), want[r], err_msg=f"{name} row {r} (image {i}, label {label})")
        assert (got[n:] == FILL).all() and got.size == n + GUARD, f"{name} row {r}: bytes behind the capacity were written"
        patches.append(patch_view(got, box, samples))
    prep.assert_inputs_untouched()
    np.testing.assert_array_equal(bufs.to_np(y_dev), y, err_msg="y was written")
    return dict(prep=prep, y=y, y_dev=y_dev, outs=outs, patches=patches)


def empty_tile(name):
    """-> (row index, (ty0, tx0)) of a kernel tile of a row's crop that holds NO pixel of the row's label but a hole pixel (of another
    region): pipe_post_rows_kernel leaves such a tile at once, the patches kernel must still write all of it, with the photo's bytes.
    Found on the oracle alone; a case without one fails here, when the test is built."""
    case = CASES[name]()
    for r, (i, label, (x0, x1, y0, y1)) in enumerate(flat_rows(case)):
        if label == 0:
            continue
        lab, hole = case["found"][i]["labels"][y0:y1, x0:x1], case["full"][i][y0:y1, x0:x1] != 255
        for ty0 in range(0, y1 - y0, TILE_H):
            for tx0 in range(0, x1 - x0, TILE_W):
                tile = (slice(ty0, ty0 + TILE_H), slice(tx0, tx0 + TILE_W))
                if not (lab[tile] == label).any() and hole[tile].any():
                    assert (lab == label).any()                      # (the row itself is not empty)
                    return r, (ty0, tx0)
    raise AssertionError(f"{name}: no row has a tile without a pixel of its label and with a hole pixel of another region")


def paste_rows(prep, outs, samples, choice, images):
    """the paste table: row r takes sample choice[r] of outs[r] (None / -1: not listed) into images[image of r]"""
    table = []
    for r, (i, label, box) in enumerate(prep.flat):
        pick = choice[r]
        if pick is None or pick < 0:
            continue
        img = prep.case["images"][i]
        table.append((prep.bufs.ptr(images[i]), prep.bufs.ptr(prep.labels_dev[i]), prep.bufs.ptr(outs[r]) + pick * patch_bytes(box, 1),
                      img.shape[1], img.shape[2], label, box))
    return table


def oracle_paste(case, flat, y, samples, choice):
    """-> per image the photo after pasting sample choice[r] of every listed row: oracle_post given the chosen y rows"""
    want = []
    for i, img in enumerate(case["images"]):
        mine = [(r, label, box) for r, (j, label, box) in enumerate(flat) if j == i and choice[r] is not None and choice[r] >= 0]
        rows = [(label, box) for _, label, box in mine]
        ys = [y[r * samples + choice[r]] for r, _, _ in mine]
        want.append(oracle_post(img, case["full"][i], case["found"][i]["labels"], rows, ys))
    return want


def mixed_choice(flat, samples):
    """a different sample per row where S allows, cycling 0, 1, ..., S - 1 down the row list: at least two distinct choices in any photo
    with two rows or more (for S >= 2)"""
    return [r % samples for r in range(len(flat))]
