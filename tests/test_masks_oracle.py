"""The numpy restatement of the reference's RandomMask (tests/masks_case.py) against what the reference's own functions returned
(tests/golden/masks_*.npz, tests/golden/make_golden_masks.py) and, where Pillow is installed, ImageDraw itself; then the C++ draws
of the library (migan_masks_draw: host code only, loaded through the CPU emulator build as the other host tests load theirs) against
numpy's own RandomState: plans and final state.  Every comparison is equality."""
import glob
import importlib
import os

import numpy as np
import pytest

from tests import masks_case as mc
from tests.emu_util import emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def hb():
    return importlib.import_module("mi-gan_amd").hipbind


def test_goldens_exist():
    paths = sorted(glob.glob(os.path.join(mc.GOLDEN, "masks_*.npz")))
    assert sorted(os.path.basename(p) for p in paths) == sorted(mc.golden_name(s, r, h) for s, r, h, _ in mc.GOLDENS)
    assert all(os.path.getsize(p) < 64 * 1024 for p in paths)
    # the numbers of candidates the reference drew: the rejection path is covered, at 32 by all-hole candidates
    assert [mc.golden(s, r, h)[2] for s, r, h, _ in mc.GOLDENS] == [197, 184, 77, 230, 576, 4, 2]
    for s, r, h, n in mc.GOLDENS:
        masks = mc.golden(s, r, h)[0]
        assert masks.shape == (n, r, r) and set(np.unique(masks)) <= {0, 255}


@pytest.mark.parametrize("entry", mc.GOLDENS, ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_restatement_equals_the_reference(entry):
    """draw order, raster, rejection and the generator's final state (with its cached Gaussian)"""
    seed, r, hole_range, n = entry
    want, state, candidates = mc.golden(seed, r, hole_range)
    rng = np.random.RandomState(seed)
    got, drawn, _ = mc.random_masks(n, r, hole_range, rng)
    assert np.array_equal(got, want) and drawn == candidates
    assert mc.same_state(rng.get_state(), state)


def test_the_global_generator_is_the_default_one():
    want, state, _ = mc.golden(0, 64, (0, 1))
    keep = np.random.get_state()
    try:
        np.random.seed(0)
        got, _, _ = mc.random_masks(3, 64, (0, 1), np.random)
        assert np.array_equal(got, want[:3])
    finally:
        np.random.set_state(keep)


def test_segments_against_imagedraw():
    """Pillow's wide line on a few thousand random segments: vertical, horizontal, zero-length and on-the-border ones among them"""
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    from PIL import Image
    r = np.random.RandomState(1)
    bad = []
    for i in range(3000):
        s = int(r.choice([16, 37, 64]))
        x0, y0, x1, y1 = (int(v) for v in r.randint(0, s + 1, 4))
        if i % 10 == 0:
            x1 = x0
        if i % 10 == 1:
            y1 = y0
        if i % 50 == 2:
            x1, y1 = x0, y0
        if i % 25 == 3:
            x0 = x1 = s
        if i % 25 == 4:
            y0 = y1 = s
        w = int(r.randint(12, 48))
        im = Image.new("L", (s, s), 0)
        ImageDraw.Draw(im).line([(x0, y0), (x1, y1)], fill=1, width=w)
        got = mc.raster(mc.make_plan(quads=[mc.quad_of_segment(x0, y0, x1, y1, w)]), s)
        if not np.array_equal(got == 0, np.asarray(im) > 0):
            bad.append((s, x0, y0, x1, y1, w))
    assert not bad, bad[:5]


def test_discs_against_imagedraw():
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    from PIL import Image
    assert len(mc.DIAMETERS) == 18 and {2 * (w // 2) for w in range(12, 48)} == set(mc.DIAMETERS)
    for d in mc.DIAMETERS:
        hw = mc.disc_half_widths(d)
        assert len(hw) == d // 2 + 1 and hw[0] == d // 2 and all(a >= b for a, b in zip(hw, hw[1:]))
        for c in ((30, 30), (0, 0), (64, 5), (3, 64), (64, 64)):
            im = Image.new("L", (64, 64), 0)
            ImageDraw.Draw(im).ellipse((c[0] - d // 2, c[1] - d // 2, c[0] + d // 2, c[1] + d // 2), fill=1)
            got = mc.raster(mc.make_plan(discs=[(c[0], c[1], d)]), 64)
            assert np.array_equal(got == 0, np.asarray(im) > 0), (d, c)


def test_capacities_follow_from_the_text():
    assert (mc.MAX_RECTS, mc.MAX_QUADS, mc.MAX_DISCS, mc.PLAN_WORDS_MAX) == (9 + 4, 19 * 17, 19 * 18, 4958)
    assert len(mc.capacity_plan(32)) == mc.PLAN_WORDS_MAX


# ---- the library's host code: numpy's legacy stream and RandomMask's draws in C++ ------------------------------------------------
@pytest.mark.parametrize("entry", mc.GOLDENS, ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_cpp_draws_equal_numpys(lib, hb, entry):
    """40 candidates: every plan word and the state behind every candidate -- MT19937 over several regenerations, random_sample, uniform, the polar
    Gaussian with its cached value, randint's masked rejection"""
    seed, r, hole_range, _ = entry
    coef = mc.coef_of(hole_range)
    rng = np.random.RandomState(seed)
    state = hb.MasksRng.from_state(rng.get_state())
    k = 40
    buf = np.full(k + 1 + k * mc.PLAN_WORDS_MAX, -1, np.int32)
    states = (hb.MasksRng * k)()
    used = lib.masks_draw(state, r, coef, k, buf.ctypes.data, buf.size, states)
    assert used == buf[k] and buf[0] == k + 1 and (buf[used:] == -1).all()
    for c in range(k):
        want = mc.draw_plan(rng, r, coef)
        assert np.array_equal(buf[buf[c]:buf[c + 1]], want), f"candidate {c}"
        assert mc.same_state(states[c].to_state(), rng.get_state()), f"the generator behind candidate {c}"
    assert mc.same_state(state.to_state(), rng.get_state())
    assert rng.get_state()[2] != 624 and k * 100 > 624                   # (the key was regenerated on the way)


def test_cpp_draws_without_a_buffer_advance_the_same(lib, hb):
    rng = np.random.RandomState(7)
    rng.normal()                                                     # a cached Gaussian in the incoming state
    a, b = hb.MasksRng.from_state(rng.get_state()), hb.MasksRng.from_state(rng.get_state())
    assert a.has_gauss == 1
    buf = np.empty(9 + 1 + 9 * mc.PLAN_WORDS_MAX, np.int32)
    lib.masks_draw(a, 48, 0.6, 9, buf.ctypes.data, buf.size)
    assert lib.masks_draw(b, 48, 0.6, 9) == 0
    for _ in range(9):
        mc.draw_plan(rng, 48, 0.6)
    assert mc.same_state(a.to_state(), b.to_state()) and mc.same_state(a.to_state(), rng.get_state())


def test_cpp_draw_argument_errors(lib, hb):
    rng = np.random.RandomState(3)
    state = hb.MasksRng.from_state(rng.get_state())
    buf = np.empty(2 + 1 + 2 * mc.PLAN_WORDS_MAX, np.int32)
    for kw in (dict(r=15), dict(r=1025), dict(k=0), dict(k=65537), dict(coef=0.19), dict(coef=1.5), dict(coef=float("nan")), dict(cap=buf.size - 1)):
        a = dict(r=32, k=2, coef=1.0, cap=buf.size)
        a.update(kw)
        with pytest.raises(ValueError):
            lib.masks_draw(state, a["r"], a["coef"], a["k"], buf.ctypes.data, a["cap"])
    bad = hb.MasksRng.from_state(rng.get_state())
    bad.pos = 625
    with pytest.raises(ValueError, match="pos"):
        lib.masks_draw(bad, 32, 1.0, 1)
    assert mc.same_state(state.to_state(), rng.get_state())              # a refused call leaves the generator alone
    with pytest.raises(TypeError, match="MT19937"):
        hb.MasksRng.from_state(("PCG64", None, 0, 0, 0.0))
