"""The numpy restatement of Pillow's uint8 BICUBIC / NEAREST resize (tests/photo_case.py) against Pillow's own bytes: the goldens
(tests/golden/photo_*.npz, tests/golden/make_golden_photo.py: Image.resize, and the reference's resize / read_mask / preprocess of
scripts/demo.py) and, where Pillow is installed, the live library.  0 differing bytes everywhere."""
import glob
import os

import numpy as np
import pytest

from tests import photo_case as pc

GOLDENS = sorted(glob.glob(os.path.join(pc.GOLDEN, "photo_*.npz")))


def test_goldens_exist():
    assert [os.path.basename(p) for p in GOLDENS] == ["photo_batch.npz", "photo_bicubic.npz", "photo_flows.npz", "photo_nearest.npz"]
    assert all(os.path.getsize(p) < 512 * 1024 for p in GOLDENS) and sum(os.path.getsize(p) for p in GOLDENS) < 768 * 1024


def test_inputs_are_the_seeded_ones():
    g = pc.golden("bicubic")
    for name in pc.BICUBIC_CASES:
        assert np.array_equal(g[f"{name}.src"], pc.bicubic_source(name)) and g[f"{name}.src"].shape[:2] == pc.BICUBIC_CASES[name][0]
        assert g[f"{name}.out"].shape[:2] == pc.BICUBIC_CASES[name][1]
    photos, masks = pc.flow_inputs()
    got_p, got_m = pc.flow_sources()
    assert all(np.array_equal(a, b) for a, b in zip(photos + masks, got_p + got_m))
    assert [p.shape[:2] for p in photos] == list(pc.FLOW_PHOTOS) and [m.shape for m in masks] == list(pc.FLOW_MASKS)
    assert max(max(m.shape) for m in masks) > 512 and all(m.shape != p.shape[:2] for p, m in zip(photos, masks))
    assert any(((m != 0) & (m != 255)).any() for m in masks)


@pytest.mark.parametrize("name", sorted(pc.BICUBIC_CASES))
def test_bicubic_restatement(name):
    g = pc.golden("bicubic")
    _, (h, w) = pc.BICUBIC_CASES[name]
    assert pc.differing(pc.pil_bicubic(g[f"{name}.src"], (w, h)), g[f"{name}.out"]) == 0


def test_tap_counts_and_the_accumulator():
    """1023 -> 16 has a ksize of 257 and outputs that use 256 taps; no left-to-right partial sum of any table the cases build leaves int32"""
    ksize, _, ns, _ = pc.coeffs(1023, 16)
    assert ksize == 257 and ns.max() == 256
    pairs = set()
    for (sh, sw), (dh, dw) in pc.BICUBIC_CASES.values():
        pairs |= {(sh, dh), (sw, dw)}
    pairs |= {(4000, 512), (3000, 512), (1024, 512), (768, 512), (16384, 1), (1, 4096)}
    for in_size, out_size in sorted(pairs):
        if in_size != out_size:
            assert pc.worst_partial_sum(in_size, out_size) < 2 ** 31, (in_size, out_size)


@pytest.mark.parametrize("name", sorted(pc.NEAREST_CASES))
def test_nearest_restatement(name):
    g = pc.golden("nearest")
    (sh, sw), (h, w), closed_form_misses = pc.NEAREST_CASES[name]
    assert pc.differing(pc.pil_nearest(g[f"{name}.src"], (w, h)), g[f"{name}.out"]) == 0
    if closed_form_misses is not None:
        iy, ix = pc.nearest_index(sh, h), pc.nearest_index(sw, w)
        cy, cx = pc.closed_form_index(sh, h), pc.closed_form_index(sw, w)
        picked_elsewhere = (iy[:, None] != cy[:, None]) | (ix[None, :] != cx[None, :])
        assert int(picked_elsewhere.sum()) == closed_form_misses
        src = g[f"{name}.src"]
        assert (src[cy][:, cx] != g[f"{name}.out"]).sum() > 0             # ... and gives other bytes than Pillow on this very mask


def test_checkerboard_overshoots():
    """the upscaled checkerboard's sums leave 0 .. 255 on both sides, so both clamps decide bytes of the golden"""
    src = pc.checkerboard(40, 40)[:, :, :1].astype(np.int64)
    _, xmins, ns, kk = pc.coeffs(40, 64)
    acc = np.stack([(1 << 21) + (src[:, xmins[x]:xmins[x] + ns[x], 0] * kk[x, :ns[x]]).sum(axis=1) for x in range(64)], axis=1) >> pc.PRECISION_BITS
    assert acc.min() < 0 and acc.max() > 255


def test_flag_restatement():
    g = pc.golden("nearest")
    for flags in (pc.INVERT, pc.THRESHOLD, pc.INVERT | pc.THRESHOLD):
        for size in ((10, 12), (7, 17)):
            assert np.array_equal(pc.pil_nearest(g["flags.src"], size, flags), g[f"flags.{flags}.{size[0]}x{size[1]}"])


def test_batch_restatement():
    g = pc.golden("batch")
    for name, sizes in (("b5", pc.BATCH5_SIZES), ("b33", pc.batch33_sizes())):
        for i, size in enumerate(sizes):
            assert np.array_equal(pc.pil_bicubic(g[f"{name}.src{i}"], size), g[f"{name}.out{i}"]), (name, i)
    assert len({g[f"b33.src{i}"].shape for i in range(33)}) > 8 and len(set(pc.batch33_sizes())) > 8
    for i, size in enumerate(pc.batch33_sizes()):
        assert np.array_equal(pc.pil_nearest(g[f"m33.src{i}"], size, pc.THRESHOLD), g[f"m33.out{i}"])


@pytest.mark.parametrize("r", pc.FLOW_RESOLUTIONS)
def test_flow_restatements(r):
    photos, masks = pc.flow_sources()
    want = pc.flow_golden("eval", r)
    for i, (p, m) in enumerate(zip(photos, masks)):
        img, mask = pc.eval_flow(p, m, r)
        assert np.array_equal(img, want[0][i]) and np.array_equal(mask, want[1][i]), f"eval {i}"
    for invert in (False, True):
        want = pc.flow_golden("demo", r, invert)
        for i, (p, m) in enumerate(zip(photos, masks)):
            img, mask = pc.demo_flow(p, m, r, invert)
            assert np.array_equal(img, want[0][i]) and np.array_equal(mask, want[1][i]), f"demo {i} invert {invert}"
        assert set(np.unique(want[1])) == {0, 255}


def test_against_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    shapes = [((37, 53), (16, 16)), ((16, 16), (37, 53)), ((7, 5), (16, 16)), ((64, 64), (64, 31)), ((129, 127), (128, 128)), ((1023, 40), (16, 16)),
              ((75, 100), (12, 16)), ((300, 400), (64, 64)), ((31, 64), (64, 31)), ((2, 50), (9, 3))]
    for (sh, sw), (dh, dw) in shapes:
        src = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        assert np.array_equal(pc.pil_bicubic(src, (dw, dh)), np.array(Image.fromarray(src).resize((dw, dh), Image.BICUBIC))), ((sh, sw), (dh, dw))
        m = np.ascontiguousarray(src[:, :, 0])
        assert np.array_equal(pc.pil_nearest(m, (dw, dh)), np.array(Image.fromarray(m).resize((dw, dh), Image.NEAREST))), ((sh, sw), (dh, dw))
