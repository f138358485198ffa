"""One crop per hole region (include/migan_pipeline_regions_hip.h: migan_pipeline_regions_find / _pre / _post) run on the CPU through
the fiber emulator: the product's kernels (mi-gan_amd/csrc/migan_pipeline_regions.inc) and host code against the scipy / pipeline
oracle of tests/pipeline_regions_case.py.  Every comparison is exact: label map, counts, boxes, x and image bytes.  The generator
is not under test: y is seeded random."""

import numpy as np
import pytest

from tests import pipeline_regions_case as rc
from tests.emu_util import emu_lib, ptr
from tests.test_emu_pipeline_batch import batch_pre, items_of

BUFS = rc.Buffers(to_dev=lambda a: np.array(a, copy=True), ptr=ptr, to_np=lambda a: np.array(a, copy=True))


@pytest.fixture(scope="module")
def lib():
    """the emulator library WITH the regions kernels (tests/emu/build_emu.py rebuilds a library older than any source)"""
    lib = emu_lib()
    assert hasattr(lib.lib, "migan_pipeline_regions_find"), "the emulator library lacks the regions entry points"
    return lib


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_case_against_the_oracle(lib, name):
    rc.run_case(lib, BUFS, rc.CASES[name]())


def test_three_blobs_are_numbered_in_raster_order(lib):
    """region 1 is the blob whose first pixel comes first in raster order (the rightmost one), and every box is masked_bbox of its blob alone"""
    case = rc.CASES["three_blobs"]()
    out = rc.run_case(lib, BUFS, case)
    lab = out["labels"][0]
    assert lab[15, 160] == 1 and lab[65, 30] == 2 and lab[130, 130] == 3
    assert [label for _, label, _ in out["flat"]] == [1, 2, 3]


def test_a_crop_shows_the_other_regions_holes_and_stores_only_its_own(lib):
    """overlapping_crops: x row 1 shows region 2's hole pixels inside box 1 as hole; the bytes inside region 2 are row 2's alone"""
    case = rc.CASES["overlapping_crops"]()
    out = rc.run_case(lib, BUFS, case)
    img, mask, lab = case["images"][0], case["full"][0], out["labels"][0]
    x0, x1, y0, y1 = out["flat"][0][2]
    assert (x1 - x0, y1 - y0) == (64, 64)                          # not resized: x row 1's mask plane is the crop's mask
    np.testing.assert_array_equal(out["x"][0, 0], mask[y0:y1, x0:x1].astype(np.float32) / 255 - 0.5)
    assert (out["x"][0, 0][lab[y0:y1, x0:x1] == 2] == -0.5).any()
    only2 = rc.oracle_post(img, mask, lab, [out["rows"][0][1]], out["y"][1:2])
    np.testing.assert_array_equal(out["images"][0][:, lab == 2], only2[:, lab == 2])


def test_fallback_rows_give_the_batch_pipelines_bytes(lib):
    """rule6: nine regions with max_regions = 8 report 9 and run as ONE row with the single box, whose bytes are
    migan_pipeline_batch_post's for the same y row; so do one region and two regions whose single box is R x R; no hole: count 0, no
    row, image untouched"""
    case = rc.CASES["rule6"]()
    out = rc.run_case(lib, BUFS, case)
    assert list(out["count"]) == [9, 1, 0, 2]
    assert [len(r) for r in out["rows"]] == [1, 1, 0, 1] and all(label == 0 for _, label, _ in out["flat"])
    np.testing.assert_array_equal(out["images"][2], case["images"][2])
    keep = [0, 1, 3]
    images = [np.array(case["images"][i], copy=True) for i in keep]
    items, scratch, bbox, x = batch_pre(lib, images, [case["masks"][i] for i in keep], case["res"], case["padding"])
    lib.pipeline_batch_post(items, case["res"], ptr(out["y"]), ptr(bbox), ptr(scratch), gauss25=rc.GAUSS)
    for j, i in enumerate(keep):
        assert tuple(bbox[j]) == out["flat"][j][2]
        np.testing.assert_array_equal(x[j], out["x"][j])
        np.testing.assert_array_equal(out["images"][i], images[j])


def test_rows_may_come_in_any_order_and_in_separate_calls(lib):
    """no pixel has two writers: the rows of many_rows reversed, and posted in two calls, give the same bytes"""
    case = rc.CASES["many_rows"]()
    first = rc.run_case(lib, BUFS, case)
    assert len(first["flat"]) == 40
    images = [np.array(img, copy=True) for img in case["images"]]
    labels = first["labels"]
    table = [(ptr(images[i]), ptr(case["full"][i]), ptr(labels[i]), images[i].shape[1], images[i].shape[2], label, box)
             for i, label, box in first["flat"]]
    order = list(range(len(table)))[::-1]
    y = np.ascontiguousarray(first["y"][order])
    lib.pipeline_regions_post([table[r] for r in order[:7]], case["res"], ptr(y[:7]), rc.GAUSS)
    lib.pipeline_regions_post([table[r] for r in order[7:]], case["res"], ptr(y[7:]), rc.GAUSS)
    for got, want in zip(images, first["images"]):
        np.testing.assert_array_equal(got, want)


def test_more_items_than_one_launch_of_find_carries(lib):
    """17 items, kRegionsFindMax = 16: one call gives the bytes of 17 calls with one item each"""
    rc.check_find_splits_like_single_calls(lib, BUFS)


def test_twice_the_same(lib):
    """the labelling uses atomics, the label map does not depend on their order: two runs, the same bytes everywhere"""
    case = rc.CASES["serpentine"]()
    a, b = rc.run_case(lib, BUFS, case), rc.run_case(lib, BUFS, case)
    np.testing.assert_array_equal(a["labels"][0], b["labels"][0])
    np.testing.assert_array_equal(a["boxes"], b["boxes"])
    np.testing.assert_array_equal(a["images"][0], b["images"][0])


def test_wide_gap(lib):
    """gap = 64, the widest: both dilation kernels use their whole halo; two dots 129 apart are one region, 130 apart two"""
    rng = np.random.default_rng(5)
    masks = []
    for dist in (129, 130):
        m = np.full((150, 300), 255, dtype=np.uint8)
        m[70, 80] = 0
        m[75, 80 + dist] = 0
        masks.append(m)
    tall = [np.ascontiguousarray(m.T) for m in masks]
    case = rc._case("wide_gap", rng, [(150, 300)] * 2 + [(300, 150)] * 2, masks + tall, 64, 4, [1, 2, 1, 2], [False, True, False, True])
    rc.run_case(lib, BUFS, case)


def test_arguments_are_checked_before_anything_is_launched(lib):
    case = rc.CASES["three_blobs"]()
    img, mask = np.array(case["images"][0], copy=True), case["masks"][0]
    h, w = mask.shape
    items = items_of([img], [mask])
    scratch = np.full(lib.pipeline_regions_scratch_bytes(items, 3, 8), 0xA5, dtype=np.uint8)
    labels = np.full((h, w), 0xEE, dtype=np.uint8)
    count, boxes = np.full(1, -7, dtype=np.int32), np.full((1, 9, 4), -7, dtype=np.int32)

    def find(items=items, res=64, padding=8, gap=3, max_regions=8, label_ptrs=(ptr(labels),), count=ptr(count), boxes=ptr(boxes), scratch=ptr(scratch)):
        lib.pipeline_regions_find(items, res, padding, gap, max_regions, None if label_ptrs is None else list(label_ptrs), count, boxes, scratch)

    for bad in (dict(gap=1), dict(gap=65), dict(max_regions=0), dict(max_regions=65), dict(res=48), dict(padding=-1), dict(label_ptrs=None),
                dict(label_ptrs=(0,)), dict(count=None), dict(boxes=None), dict(scratch=None), dict(items=[]),
                dict(items=[(ptr(img), 0, h, w, h, w)]), dict(items=[(ptr(img), ptr(mask), 2, w, h, w)])):
        with pytest.raises(ValueError):
            find(**bad)
    for gap, cap in ((1, 8), (3, 0)):
        with pytest.raises(ValueError):
            lib.pipeline_regions_scratch_bytes(items, gap, cap)
    assert (labels == 0xEE).all() and (count == -7).all() and (boxes == -7).all() and (scratch == 0xA5).all()
    find()
    assert count[0] == 3

    x = np.full((1, 4, 64, 64), 3.0, dtype=np.float32)
    y = np.zeros((1, 3, 64, 64), dtype=np.float32)
    box = tuple(int(v) for v in boxes[0, 1])
    good = (ptr(img), ptr(mask), ptr(labels), h, w, 1, box)
    for bad in ((0,) + good[1:], good[:1] + (0,) + good[2:], good[:2] + (0,) + good[3:], good[:5] + (65, box), good[:5] + (-1, box),
                good[:6] + ((0, w + 1, 0, 64),), good[:6] + ((5, 7, 0, 64),), good[:3] + (2, w, 1, box)):
        with pytest.raises(ValueError):
            lib.pipeline_regions_pre([bad], 64, ptr(x))
        with pytest.raises(ValueError):
            lib.pipeline_regions_post([bad], 64, ptr(y), rc.GAUSS)
    for rows, res, buf in (([], 64, ptr(x)), (None, 64, ptr(x)), ([good], 48, ptr(x)), ([good], 64, None)):
        with pytest.raises(ValueError):
            lib.pipeline_regions_pre(rows, res, buf)
        with pytest.raises(ValueError):
            lib.pipeline_regions_post(rows, res, buf, rc.GAUSS)
    assert (x == 3.0).all() and (img == case["images"][0]).all()
    lib.pipeline_regions_pre([good[:2] + (0,) + good[3:5] + (0, box)], 64, ptr(x))        # label 0 needs no label map
    assert not (x == 3.0).all()
