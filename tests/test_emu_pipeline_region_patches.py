"""S completions per hole region as patches, and the paste back (include/migan_pipeline_region_patches_hip.h:
migan_pipeline_regions_post_patches / _paste) run on the CPU through the fiber emulator: the product's kernels
(mi-gan_amd/csrc/migan_pipeline_region_patches.inc) and host code against the oracle of tests/pipeline_region_patches_case.py.
Every comparison is byte for byte.  The generator is not under test: y is seeded random."""

import numpy as np
import pytest

from tests import pipeline_region_patches_case as pc
from tests.emu_util import emu_lib, ptr
from tests.test_emu_pipeline_batch import batch_pre

BUFS = pc.Buffers(to_dev=lambda a: np.array(a, copy=True), ptr=ptr, to_np=lambda a: np.array(a, copy=True))


@pytest.fixture(scope="module")
def lib():
    """the emulator library WITH the region patches kernels (tests/emu/build_emu.py rebuilds a library older than any source)"""
    lib = emu_lib()
    assert hasattr(lib.lib, "migan_pipeline_regions_post_patches"), "the emulator library lacks the region patches entry points"
    return lib


# many_rows (40 rows) runs at S = 2 to stay at seconds; every other case at S = 3
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_against_the_oracle(lib, name):
    out = pc.check_case(lib, BUFS, name, 2 if name == "many_rows" else 3)
    if name == "many_rows":
        assert len(out["prep"].flat) == 40                           # a launch carries 32 rows: the last 8 are the second launch's
    if name == "rule6":
        assert [label for _, label, _ in out["prep"].flat] == [0, 0, 0]
    if name == "three_blobs":                                        # different y: different patches
        assert [label for _, label, _ in out["prep"].flat] == [1, 2, 3]
        assert (out["patches"][0][0] != out["patches"][0][1]).any() and (out["patches"][0][1] != out["patches"][0][2]).any()


@pytest.mark.parametrize("name", ["three_blobs", "borders", "rule6"])
def test_one_sample(lib, name):
    pc.check_case(lib, BUFS, name, 1)


def test_the_crops_are_off_the_tile_grid_and_clipped():
    """what the cases are relied on for: a crop that is no multiple of the tile, and boxes clipped at an image border"""
    boxes = [box for _, _, box in pc.flat_rows(pc.CASES["borders"]())]
    img = pc.CASES["borders"]()["images"][0]
    assert any(b[0] == 0 and b[2] == 0 for b in boxes) and any(b[1] == img.shape[2] and b[3] == img.shape[1] for b in boxes)
    sizes = [(b[1] - b[0], b[3] - b[2]) for name in pc.CASES for _, _, b in pc.flat_rows(pc.CASES[name]())]
    assert any(w % pc.TILE_W and h % pc.TILE_H and w > pc.TILE_W and h > pc.TILE_H for w, h in sizes)


def test_a_patch_holds_the_photo_where_another_region_lies(lib):
    """overlapping_crops: box 1 covers a part of region 2; there patch 1 holds the photo's bytes in every sample"""
    out = pc.check_case(lib, BUFS, "overlapping_crops", 3)
    case, prep = out["prep"].case, out["prep"]
    assert [label for _, label, _ in prep.flat] == [1, 2, 3]
    x0, x1, y0, y1 = prep.flat[0][2]
    sel = prep.labels[0][y0:y1, x0:x1] == 2
    assert sel.any() and (case["full"][0][y0:y1, x0:x1][sel] != 255).any()
    for s in range(3):
        np.testing.assert_array_equal(out["patches"][0][s][:, sel], case["images"][0][:, y0:y1, x0:x1][:, sel])
    own = prep.labels[0][y0:y1, x0:x1] == 1
    assert (out["patches"][0][0][:, own] != case["images"][0][:, y0:y1, x0:x1][:, own]).any()


def test_a_tile_without_a_pixel_of_its_label_is_still_written(lib):
    """the in-place kernel leaves such a tile at once; here all of it is written, with the photo's bytes, in every sample"""
    r, (ty0, tx0) = pc.empty_tile("overlapping_crops")
    out = pc.check_case(lib, BUFS, "overlapping_crops", 3)
    i, _, (x0, x1, y0, y1) = out["prep"].flat[r]
    photo = out["prep"].case["images"][i][:, y0:y1, x0:x1]
    for s in range(3):
        np.testing.assert_array_equal(out["patches"][r][s][:, ty0:ty0 + pc.TILE_H, tx0:tx0 + pc.TILE_W],
                                      photo[:, ty0:ty0 + pc.TILE_H, tx0:tx0 + pc.TILE_W])


def test_every_byte_is_written_whatever_the_fill(lib):
    """two different fills agree inside the capacity, and neither guard is touched"""
    case = pc.CASES["overlapping_crops"]()
    y, _ = pc.reference("overlapping_crops", 3)
    prep = pc.Prepared(lib, BUFS, case)
    a, b = pc.post_patches(prep, y, 3, fill=pc.FILL), pc.post_patches(prep, y, 3, fill=0x5A)
    for r, (_, _, box) in enumerate(prep.flat):
        n = pc.patch_bytes(box, 3)
        np.testing.assert_array_equal(a[r][:n], b[r][:n], err_msg=f"row {r}: a byte inside the capacity was not written")
        assert (a[r][n:] == pc.FILL).all() and (b[r][n:] == 0x5A).all()


def test_label_0_rows_give_the_batch_patches_bytes(lib):
    """rule6: the rows that are not split hold migan_pipeline_batch_post_patches' bytes for the same y"""
    out = pc.check_case(lib, BUFS, "rule6", 3)
    case, prep = out["prep"].case, out["prep"]
    keep = [i for i, _, _ in prep.flat]
    assert keep == [0, 1, 3] and all(label == 0 for _, label, _ in prep.flat)
    images = [np.array(case["images"][i], copy=True) for i in keep]
    items, scratch, bbox, _ = batch_pre(lib, images, [case["masks"][i] for i in keep], case["res"], case["padding"])
    sizes = [pc.patch_bytes(box, 3) for _, _, box in prep.flat]
    bufs = [np.full(n, pc.FILL, dtype=np.uint8) for n in sizes]
    lib.pipeline_batch_post_patches(items, 3, case["res"], ptr(out["y"]), ptr(bbox), ptr(scratch), [ptr(b) for b in bufs], sizes, gauss25=pc.GAUSS)
    for r, (_, _, box) in enumerate(prep.flat):
        assert tuple(bbox[r]) == box
        np.testing.assert_array_equal(pc.patch_view(bufs[r], box, 3), out["patches"][r], err_msg=f"row {r}")


# ---- paste ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overlapping_crops", "three_blobs", "borders"])
def test_paste_a_different_sample_per_region(lib, name):
    """the chosen sample of every region -> the photo: oracle_post given the chosen y rows; rows reversed, or pasted in two calls,
    give the same bytes; the patches are only read"""
    out = pc.check_case(lib, BUFS, name, 3)
    prep, case = out["prep"], out["prep"].case
    choice = pc.mixed_choice(prep.flat, 3)
    assert len(set(choice)) >= 2
    want = pc.oracle_paste(case, prep.flat, out["y"], 3, choice)
    before = [np.array(o, copy=True) for o in out["outs"]]
    for order in ("forward", "reversed", "two calls"):
        images = [np.array(a, copy=True) for a in case["images"]]
        table = pc.paste_rows(prep, out["outs"], 3, choice, images)
        if order == "two calls":
            lib.pipeline_regions_paste(table[1:])
            lib.pipeline_regions_paste(table[:1])
        else:
            lib.pipeline_regions_paste(table if order == "forward" else table[::-1])
        for got, w in zip(images, want):
            np.testing.assert_array_equal(got, w, err_msg=f"{name}, {order}")
    assert (want[0] != case["images"][0]).any()
    for o, b in zip(out["outs"], before):
        np.testing.assert_array_equal(o, b)
    prep.assert_inputs_untouched()


def test_an_unlisted_region_keeps_the_photos_bytes(lib):
    out = pc.check_case(lib, BUFS, "overlapping_crops", 3)
    prep, case = out["prep"], out["prep"].case
    for choice in ([2, None, 1], [-1, 0, -1]):
        images = [np.array(a, copy=True) for a in case["images"]]
        lib.pipeline_regions_paste(pc.paste_rows(prep, out["outs"], 3, choice, images))
        np.testing.assert_array_equal(images[0], pc.oracle_paste(case, prep.flat, out["y"], 3, choice)[0])
        for r, pick in enumerate(choice):
            sel = prep.labels[0] == r + 1
            assert (images[0][:, sel] == case["images"][0][:, sel]).all() == (pick is None or pick < 0)


def test_pasting_the_one_sample_is_the_in_place_post(lib):
    """S = 1, choice 0: what migan_pipeline_regions_post leaves for the same y; with the 40 rows of many_rows across a launch of 32"""
    for name in ("many_rows", "rule6"):
        out = pc.check_case(lib, BUFS, name, 1)
        prep, case = out["prep"], out["prep"].case
        pasted = [np.array(a, copy=True) for a in case["images"]]
        lib.pipeline_regions_paste(pc.paste_rows(prep, out["outs"], 1, [0] * len(prep.flat), pasted))
        posted = [np.array(a, copy=True) for a in case["images"]]
        lib.pipeline_regions_post([prep.row(r, posted[prep.flat[r][0]]) for r in range(len(prep.flat))], case["res"], ptr(out["y"]), pc.GAUSS)
        for i, (a, b) in enumerate(zip(pasted, posted)):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} image {i}")
        assert (pasted[0] != case["images"][0]).any()


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_anything_is_launched(lib):
    case = pc.CASES["three_blobs"]()
    prep = pc.Prepared(lib, BUFS, case)
    h, w = case["images"][0].shape[1:]
    good, box = prep.table[0], prep.flat[0][2]
    S, res = 2, case["res"]
    y = np.zeros((S, 3, res, res), dtype=np.float32)
    n = pc.patch_bytes(box, S)
    out = np.full(n + pc.GUARD, pc.FILL, dtype=np.uint8)

    def post(rows=(good,), samples=S, res=res, y=ptr(y), outs=(ptr(out),), caps=(n,)):
        lib.pipeline_regions_post_patches(None if rows is None else list(rows), samples, res, y, None if outs is None else list(outs),
                                          None if caps is None else list(caps), pc.GAUSS)

    bad_rows = ((0,) + good[1:], good[:1] + (0,) + good[2:], good[:2] + (0,) + good[3:],          # null image, mask, labels with label 1
                good[:5] + (65, box), good[:5] + (-1, box),                                      # label out of range
                good[:6] + ((0, w + 1, 0, 64),), good[:6] + ((5, 7, 0, 64),), good[:6] + ((0, 64, -1, 63),),      # bad boxes
                good[:3] + (2, w, 1, box))                                                       # an image below 3 x 3
    for bad in ([dict(samples=0), dict(samples=-1), dict(outs=None), dict(caps=None), dict(outs=(0,)), dict(caps=(n - 1,)), dict(res=48),
                 dict(y=None), dict(rows=None, outs=(), caps=()), dict(rows=(), outs=(), caps=())] + [dict(rows=(b,)) for b in bad_rows]):
        with pytest.raises(ValueError):
            post(**bad)
    assert (out == pc.FILL).all()
    prep.assert_inputs_untouched()
    post()                                                           # and the good call goes through, exactly into its capacity
    assert not (out[:n] == pc.FILL).all() and (out[n:] == pc.FILL).all()
    post(rows=(good[:2] + (0,) + good[3:5] + (0, box),))             # label 0 needs no label map

    img = np.array(case["images"][0], copy=True)
    pgood = (ptr(img), ptr(prep.labels_dev[0]), ptr(out), h, w, 1, box)
    for bad in ((0,) + pgood[1:], pgood[:1] + (0,) + pgood[2:], pgood[:2] + (0,) + pgood[3:],     # null image, labels with label 1, patch
                pgood[:5] + (65, box), pgood[:5] + (-1, box), pgood[:6] + ((0, w + 1, 0, 64),), pgood[:6] + ((5, 7, 0, 64),),
                pgood[:3] + (2, w, 1, box)):
        with pytest.raises(ValueError):
            lib.pipeline_regions_paste([bad])
        with pytest.raises(ValueError):
            lib.pipeline_regions_paste([pgood, bad])                 # a bad row behind a good one: the good one is not pasted either
    for rows in ([], None):
        with pytest.raises(ValueError):
            lib.pipeline_regions_paste(rows)
    np.testing.assert_array_equal(img, case["images"][0])
    lib.pipeline_regions_paste([pgood])
    assert (img != case["images"][0]).any()
    lib.pipeline_regions_paste([pgood[:1] + (0,) + pgood[2:5] + (0, box)])                        # label 0 needs no label map
