"""The cases and the oracle shared by tests/test_emu_pipeline_regions.py and tests/test_gpu_pipeline_regions.py (one crop per hole
region: include/migan_pipeline_regions_hip.h, MIGAN_Pipeline.forward_regions).  Test infrastructure only.

The oracle restates the definition with scipy and the pipeline oracle: D = maximum_filter of the hole indicator, regions =
ndimage.label(D, 8-connectivity) (numbered in raster order of their first pixel), box k = po.masked_bbox of a mask that holds region
k's hole pixels alone, x = po.preprocess of the crop with the FULL mask, result = po.postprocess of the crop with the full mask,
pasted where label == k.  Every case builder asserts, on the oracle alone, that the case yields the K it was built for and that the
"do not split" rule triggers or not as intended: a case that degenerates fails when it is built, not vacuously later."""
import functools

import numpy as np
import torch
from scipy import ndimage

from oracle import migan_pipeline_oracle as po

RES, PADDING = 64, 8
GAUSS = po.gaussian_kernel().flatten().tolist()
TILE = 32                                    # regions_label_tile_kernel's tile (migan_pipeline_regions.inc: kRegTile)


def random_y(rng, rows, res=RES):
    return (rng.standard_normal((rows, 3, res, res)) * 0.6).astype(np.float32)


def resized_mask(mask, h, w):
    """the mask at the image's size: tvF.resize(mask, (h, w), NEAREST)"""
    if mask.shape == (h, w):
        return mask
    return np.ascontiguousarray(po.tv_resize(torch.from_numpy(mask)[None, None], (h, w), "nearest")[0, 0].numpy())


def oracle_find(mask, gap, max_regions, res=RES, padding=PADDING):
    """mask [H, W] at the image's size -> dict(labels uint8 [H, W], K, single box, boxes [K][4], split)"""
    hole = mask != 255
    d = ndimage.maximum_filter(hole.astype(np.uint8), size=2 * gap + 1, mode="constant", cval=0) > 0
    lab, k = ndimage.label(d, structure=np.ones((3, 3), dtype=int))
    single = tuple(int(v) for v in po.masked_bbox(mask, res, padding))
    boxes = []
    for r in range(1, k + 1):
        alone = np.full_like(mask, 255)
        sel = hole & (lab == r)
        alone[sel] = mask[sel]
        boxes.append(tuple(int(v) for v in po.masked_bbox(alone, res, padding)))
    fits = single[1] - single[0] <= res and single[3] - single[2] <= res
    split = 2 <= k <= max_regions and not fits
    return dict(labels=lab.astype(np.uint8) if k <= 255 else None, K=int(k), single=single, boxes=boxes, split=split, hole=bool(hole.any()))


def rows_of(found):
    """the (label, box) rows of one image by the "when not to split" rule"""
    if not found["hole"]:
        return []
    if found["split"]:
        return [(r + 1, box) for r, box in enumerate(found["boxes"])]
    return [(0, found["single"])]


def oracle_x(image, mask, box, res=RES):
    x0, x1, y0, y1 = box
    ci = torch.from_numpy(image[None, :, y0:y1, x0:x1].copy())
    cm = torch.from_numpy(mask[None, None, y0:y1, x0:x1].copy())
    return po.preprocess(ci, cm, res)[0].numpy()


def oracle_post(image, mask, labels, rows, y):
    """-> the image after every row (label, box) with its y row: the post-processing of the crop with the full mask, every crop
    taken from the ORIGINAL image, pasted where labels == label (everywhere in the crop for label 0)"""
    out = np.array(image, copy=True)
    for (label, (x0, x1, y0, y1)), yr in zip(rows, y):
        ci = torch.from_numpy(image[None, :, y0:y1, x0:x1].copy())
        cm = torch.from_numpy(mask[None, None, y0:y1, x0:x1].copy())
        done = po.postprocess(ci, cm, torch.from_numpy(yr[None]))[0].numpy()
        sel = np.ones((y1 - y0, x1 - x0), dtype=bool) if label == 0 else labels[y0:y1, x0:x1] == label
        out[:, y0:y1, x0:x1][:, sel] = done[:, sel]
    return out


def _case(name, rng, sizes, masks, gap, max_regions, want_k, want_split):
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    case = dict(name=name, images=images, masks=[np.ascontiguousarray(m) for m in masks], gap=gap, max_regions=max_regions, res=RES,
                padding=PADDING)
    case["full"] = [resized_mask(m, h, w) for m, (h, w) in zip(case["masks"], sizes)]
    case["found"] = [oracle_find(m, gap, max_regions) for m in case["full"]]
    got_k = [f["K"] for f in case["found"]]
    got_split = [f["split"] for f in case["found"]]
    assert got_k == list(want_k), f"{name}: built for K = {list(want_k)}, the oracle finds {got_k}"
    assert got_split == list(want_split), f"{name}: built for split = {list(want_split)}, the oracle says {got_split}"
    return case


def _blank(h, w):
    return np.full((h, w), 255, dtype=np.uint8)


def case_three_blobs():
    """three blobs well apart; the raster order of their first pixels is not the order of their columns"""
    rng = np.random.default_rng(101)
    m = _blank(157, 203)
    m[10:22, 150:170] = 0
    m[60:75, 20:45] = 0
    m[120:140, 118:151] = 0
    return _case("three_blobs", rng, [(157, 203)], [m], 3, 8, [3], [True])


def case_corner_touch():
    """two single hole pixels whose dilated squares touch at one corner only: one region under 8-connectivity; one pixel further
    apart: two"""
    rng = np.random.default_rng(102)
    gap, masks = 2, []
    for extra in (0, 1):
        m = _blank(75, 90)
        m[20, 30] = 0
        m[20 + 2 * gap + 1 + extra, 30 + 2 * gap + 1 + extra] = 0
        masks.append(m)
    return _case("corner_touch", rng, [(75, 90)] * 2, masks, gap, 8, [1, 2], [False, False])


def case_merge_boundary():
    """two single hole pixels at Chebyshev distance 2 gap + 1 (one region) and 2 gap + 2 (two), along x and along y, across a tile border"""
    rng = np.random.default_rng(103)
    gap, masks, want = 3, [], []
    for axis in (0, 1):
        for dist, k in ((2 * gap + 1, 1), (2 * gap + 2, 2)):
            m = _blank(71, 93)
            a = [28, 27]                                             # the pair straddles row / column 32
            b = list(a)
            b[axis] += dist
            m[a[0], a[1]] = 0
            m[b[0], b[1]] = 0
            masks.append(m)
            want.append(k)
    return _case("merge_boundary", rng, [(71, 93)] * 4, masks, gap, 8, want, [False] * 4)


def case_serpentine():
    """a one-pixel-wide serpentine through 5 x 4 labelling tiles (gap = 2): vertical runs joined alternately at the top and at the
    bottom, so the component's label must travel down, across a tile border, up again ... and a second blob between two runs that
    must stay separate.  A single sweep of merges along the tile borders does not finish this one."""
    rng = np.random.default_rng(104)
    h, w = 141, 123
    m = _blank(h, w)
    xs = list(range(8, 113, 16))                                     # 8, 24, ..., 104
    for j, x in enumerate(xs):
        m[8:131, x] = 0
        if j + 1 < len(xs):
            m[8 if j % 2 == 0 else 130, x:xs[j + 1] + 1] = 0
    m[60:63, 47:50] = 0                                              # between the runs at x = 40 and x = 56
    assert h > 4 * TILE and w > 3 * TILE
    return _case("serpentine", rng, [(h, w)], [m], 2, 8, [2], [True])


def case_borders():
    """regions in two corners and on the right border: the dilation and the boxes are clipped"""
    rng = np.random.default_rng(105)
    h, w = 97, 83
    m = _blank(h, w)
    m[0:6, 0:9] = 0
    m[h - 5:h, w - 7:w] = 0
    m[40:47, w - 3:w] = 0
    m[h - 1, 0] = 0
    return _case("borders", rng, [(h, w)], [m], 3, 8, [4], [True])


def case_overlapping_crops():
    """regions 1 and 2 are 20 pixels apart: box 1 (64 wide) covers part of region 2, and the other way round; region 3 is far away"""
    rng = np.random.default_rng(106)
    m = _blank(170, 200)
    m[30:40, 30:40] = 0
    m[33:45, 60:72] = 0
    m[150:160, 180:190] = 0
    case = _case("overlapping_crops", rng, [(170, 200)], [m], 2, 8, [3], [True])
    (x0, x1, y0, y1), lab = case["found"][0]["boxes"][0], case["found"][0]["labels"]
    inside = (lab[y0:y1, x0:x1] == 2) & (m[y0:y1, x0:x1] != 255)
    assert inside.any() and inside.sum() < ((lab == 2) & (m != 255)).sum(), "box 1 must cover a part of region 2's hole pixels"
    return case


def case_gray():
    """mask values 1 ... 254 inside the regions: anything but 255 is a hole pixel for labels and boxes, pre / post use the bytes"""
    rng = np.random.default_rng(107)
    m = _blank(120, 180)
    m[20:40, 15:50] = rng.integers(1, 255, (20, 35), dtype=np.uint8)
    m[80:100, 130:160] = rng.integers(0, 255, (20, 30), dtype=np.uint8)
    m[85:90, 140:150] = 254
    return _case("gray", rng, [(120, 180)], [m], 3, 8, [2], [True])


def case_rule6():
    """when not to split: nine dots with max_regions = 8, one region, no hole at all, two blobs whose single box is R x R"""
    rng = np.random.default_rng(108)
    dots = _blank(140, 140)
    for y in (20, 60, 100):
        for x in (25, 65, 105):
            dots[y:y + 3, x:x + 3] = 0
    one = _blank(99, 130)
    one[30:70, 40:110] = 0
    none = _blank(77, 91)
    near = _blank(110, 120)
    near[40:46, 40:46] = 0
    near[60:66, 70:76] = 0
    return _case("rule6", rng, [(140, 140), (99, 130), (77, 91), (110, 120)], [dots, one, none, near], 3, 8, [9, 1, 0, 2],
                 [False, False, False, False])


def case_resized_masks():
    """masks of another size than their image (half size, odd aspect; larger): the nearest-resize path"""
    rng = np.random.default_rng(109)
    a = _blank(60, 75)
    a[5:12, 6:15] = 0
    a[45:55, 55:70] = 0
    b = _blank(200, 170)
    b[20:45, 20:40] = 0
    b[150:180, 120:160] = 0
    return _case("resized_masks", rng, [(120, 150), (131, 97)], [a, b], 3, 8, [2, 2], [True, True])


def case_many_rows():
    """two images of 20 regions each with max_regions = 32: 40 rows, so the rows of the second image straddle a launch of 32 rows
    (and a chunk of forward_regions)"""
    rng = np.random.default_rng(110)
    masks = []
    for shift in (0, 3):
        m = _blank(130, 160)
        for y in range(10 + shift, 130, 32):
            for x in range(12 + shift, 160, 31):
                m[y:y + 4 + shift, x:x + 5] = 0                         # (a hole narrower than 3 vanishes in the 3x3 max-pool)
        masks.append(m)
    return _case("many_rows", rng, [(130, 160)] * 2, masks, 2, 32, [20, 20], [True, True])


CASES = {f.__name__[5:]: functools.lru_cache(maxsize=None)(f) for f in (
    case_three_blobs, case_corner_touch, case_merge_boundary, case_serpentine, case_borders, case_overlapping_crops, case_gray, case_rule6,
    case_resized_masks, case_many_rows)}


class Buffers:
    """what the two test files differ in: where the buffers live.  to_dev(numpy array) -> a buffer, ptr(buffer) -> its address,
    to_np(buffer) -> a numpy copy, stream"""

    def __init__(self, to_dev, ptr, to_np, stream=0):
        self.to_dev, self.ptr, self.to_np, self.stream = to_dev, ptr, to_np, stream


def run_find(lib, bufs, case, images_dev, masks_dev):
    """migan_pipeline_regions_find on the case -> labels (list of uint8 [H, W]), count [n], boxes [n, max_regions + 1, 4], and the label
    buffers.  Every output starts as a fill value."""
    n, cap = len(case["images"]), case["max_regions"] + 1
    items = [(bufs.ptr(i), bufs.ptr(m), img.shape[1], img.shape[2], msk.shape[0], msk.shape[1])
             for i, m, img, msk in zip(images_dev, masks_dev, case["images"], case["masks"])]
    scratch = bufs.to_dev(np.full(lib.pipeline_regions_scratch_bytes(items, case["gap"], case["max_regions"]), 0xA5, dtype=np.uint8))
    labels = [bufs.to_dev(np.full(img.shape[1:], 0xEE, dtype=np.uint8)) for img in case["images"]]
    count = bufs.to_dev(np.full(n, -7, dtype=np.int32))
    boxes = bufs.to_dev(np.full((n, cap, 4), -7, dtype=np.int32))
    lib.pipeline_regions_find(items, case["res"], case["padding"], case["gap"], case["max_regions"], [bufs.ptr(b) for b in labels],
                              bufs.ptr(count), bufs.ptr(boxes), bufs.ptr(scratch), bufs.stream)
    return [bufs.to_np(b) for b in labels], bufs.to_np(count), bufs.to_np(boxes), labels


def seventeen_items():
    """more items than one launch of regions_find carries (kRegionsFindMax = 16): 17 tiny images of different sizes between 8 x 8 and
    14 x 14 with one or two holes each, two of them with a mask of another size, one all known, one all hole.  No oracle: the test
    compares one call with 17 calls."""
    rng = np.random.default_rng(111)
    sizes = [(8 + i % 7, 8 + (2 * i + i // 7) % 7) for i in range(17)]
    assert len(set(sizes)) == 17 and all(8 <= s <= 14 for hw in sizes for s in hw)
    masks = []
    for i, (h, w) in enumerate(sizes):
        mh, mw = {3: (2 * h, 2 * w), 11: (h + 3, w - 2)}.get(i, (h, w))
        m = _blank(mh, mw)
        m[1:3, 1:3] = 0
        if i % 2:
            m[mh - 3:mh - 1, mw - 3:mw - 1] = 0
        masks.append(m)
    masks[5][...] = 255
    masks[9][...] = 0
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    return dict(name="seventeen_items", images=images, masks=masks, gap=2, max_regions=4, res=8, padding=2)


def check_find_splits_like_single_calls(lib, bufs):
    """labels, counts and boxes of ONE regions_find over 17 items (two launches of every kernel; counts and boxes of the second
    begin at item 16) are, byte for byte, those of 17 calls with one item each"""
    case = seventeen_items()

    def find(sub):
        images_dev = [bufs.to_dev(img) for img in sub["images"]]
        masks_dev = [bufs.to_dev(m) for m in sub["masks"]]
        return run_find(lib, bufs, sub, images_dev, masks_dev)[:3]

    labels, count, boxes = find(case)
    assert sorted(set(count.tolist())) == [0, 1, 2], "the case must hold images without a region, with one and with two"
    assert count[5] == 0 and count[9] == 1 and not (labels[5] != 0).any() and (labels[9] == 1).all()
    for i in range(17):
        one = dict(case, images=case["images"][i:i + 1], masks=case["masks"][i:i + 1])
        labels1, count1, boxes1 = find(one)
        np.testing.assert_array_equal(labels[i], labels1[0], err_msg=f"item {i}")
        assert count[i] == count1[0], f"item {i}"
        np.testing.assert_array_equal(boxes[i], boxes1[0], err_msg=f"item {i}")


def check_find(case, labels, count, boxes):
    """label map, counts and boxes against the oracle"""
    cap = case["max_regions"] + 1
    for i, found in enumerate(case["found"]):
        what = f"{case['name']} item {i}"
        k = found["K"]
        assert count[i] == min(k, cap), what
        assert tuple(boxes[i, 0]) == found["single"], what
        if k < cap:
            np.testing.assert_array_equal(labels[i], found["labels"], err_msg=what)
            assert [tuple(b) for b in boxes[i, 1:k + 1]] == found["boxes"], what
            assert not boxes[i, k + 1:].any(), what
        else:
            assert not boxes[i, 1:].any(), what


def host_rows(case, count, boxes):
    """the "when not to split" rule on the host copy of counts and boxes, as forward_regions applies it -> per image [(label, box)]"""
    rows, res = [], case["res"]
    for i, found in enumerate(case["found"]):
        k, single = int(count[i]), tuple(int(v) for v in boxes[i, 0])
        fits = single[1] - single[0] <= res and single[3] - single[2] <= res
        if k == 0:
            rows.append([])
        elif k < 2 or k > case["max_regions"] or fits:
            rows.append([(0, single)])
        else:
            rows.append([(r, tuple(int(v) for v in boxes[i, r])) for r in range(1, k + 1)])
        assert rows[-1] == rows_of(found), f"{case['name']} item {i}"
    return rows


def run_case(lib, bufs, case, y_seed=7):
    """find -> check -> rows -> pre -> check x -> post with seeded y -> check every image byte.  Returns what a test may look at
    further: dict(labels, count, boxes, rows, x, y, images)"""
    images_dev = [bufs.to_dev(img) for img in case["images"]]
    masks_dev = [bufs.to_dev(m) for m in case["masks"]]
    labels, count, boxes, labels_dev = run_find(lib, bufs, case, images_dev, masks_dev)
    check_find(case, labels, count, boxes)
    rows = host_rows(case, count, boxes)
    full_dev = []
    for m_dev, m, full, img in zip(masks_dev, case["masks"], case["full"], case["images"]):
        h, w = img.shape[1:]
        if m.shape != (h, w):                                        # the rows take the mask at the image's size
            resized = bufs.to_dev(np.zeros((h, w), dtype=np.uint8))
            lib.pipeline_mask_resize(bufs.ptr(m_dev), m.shape[0], m.shape[1], bufs.ptr(resized), h, w, bufs.stream)
            np.testing.assert_array_equal(bufs.to_np(resized), full)
            m_dev = resized
        full_dev.append(m_dev)
    flat = [(i, label, box) for i, rs in enumerate(rows) for label, box in rs]
    table = [(bufs.ptr(images_dev[i]), bufs.ptr(full_dev[i]), bufs.ptr(labels_dev[i]), case["images"][i].shape[1], case["images"][i].shape[2],
              label, box) for i, label, box in flat]
    res = case["res"]
    x_dev = bufs.to_dev(np.zeros((len(flat), 4, res, res), dtype=np.float32))
    lib.pipeline_regions_pre(table, res, bufs.ptr(x_dev), bufs.stream)
    x = bufs.to_np(x_dev)
    for r, (i, label, box) in enumerate(flat):
        np.testing.assert_array_equal(x[r], oracle_x(case["images"][i], case["full"][i], box), err_msg=f"{case['name']} row {r}")
    y = random_y(np.random.default_rng(y_seed), len(flat))
    y_dev = bufs.to_dev(y)
    lib.pipeline_regions_post(table, res, bufs.ptr(y_dev), GAUSS, bufs.stream)
    images = [bufs.to_np(b) for b in images_dev]
    at = 0
    for i, rs in enumerate(rows):
        want = oracle_post(case["images"][i], case["full"][i], case["found"][i]["labels"], rs, y[at:at + len(rs)])
        at += len(rs)
        np.testing.assert_array_equal(images[i], want, err_msg=f"{case['name']} item {i}")
        if case["found"][i]["split"]:                                # outside every label: the input image
            np.testing.assert_array_equal(images[i][:, labels[i] == 0], case["images"][i][:, labels[i] == 0])
    return dict(labels=labels, count=count, boxes=boxes, rows=rows, flat=flat, x=x, y=y, images=images)

