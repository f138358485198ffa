"""Random hole masks (include/migan_masks_hip.h) on the CPU emulator: the kernel of mi-gan_amd/csrc/migan_masks.hpp and the host code
behind migan_masks_draw / migan_masks_raster on host memory, driven by mi-gan_amd/masks.py's own acceptance loop, against the masks
the reference's RandomMask returned (tests/golden/masks_*.npz).  Every comparison is equality of bytes.  The same cases run on the
device in tests/test_gpu_masks.py."""
import os
import re

import numpy as np
import pytest

from tests import masks_case as mc
from tests.emu_util import ROOT, emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def mem():
    return mc.HostMem()


@pytest.mark.parametrize("entry", mc.SMALL, ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_goldens(pkg, lib, entry):
    seed, r, hole_range, n = entry
    want, state, candidates = mc.golden(seed, r, hole_range)
    rng = np.random.RandomState(seed)
    got, ratios, backend = mc.emu_random_masks(pkg, lib, n, r, hole_range, rng)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert mc.same_state(rng.get_state(), state)
    assert np.array_equal(ratios, [mc.hole_ratio(m) for m in want])
    assert backend.launches <= 4 < candidates                              # chunks, one read-back each


@pytest.mark.parametrize("entry", (mc.SMALL[1], mc.SMALL[3]), ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_chunk_sizes_give_the_same_masks_and_state(pkg, lib, entry):
    seed, r, hole_range, n = entry
    n = min(n, 12)
    want, _, _ = mc.golden(seed, r, hole_range)
    ref = np.random.RandomState(seed)
    _, drawn, _ = mc.random_masks(n, r, hole_range, ref)                   # the state behind the n-th mask, from numpy itself
    for chunk in (1, 7, drawn, drawn + 5):
        rng = np.random.RandomState(seed)
        got, _, backend = mc.emu_random_masks(pkg, lib, n, r, hole_range, rng, chunk=chunk)
        assert np.array_equal(got, want[:n]), f"chunk {chunk}"
        assert mc.same_state(rng.get_state(), ref.get_state()), f"chunk {chunk}"
        assert backend.launches == -(-drawn // chunk)
    # a caller interleaves its own draws: two calls are one
    rng = np.random.RandomState(seed)
    a, _, _ = mc.emu_random_masks(pkg, lib, 5, r, hole_range, rng)
    b, _, _ = mc.emu_random_masks(pkg, lib, n - 5, r, hole_range, rng)
    assert np.array_equal(np.concatenate([a, b]), want[:n]) and mc.same_state(rng.get_state(), ref.get_state())


def test_no_rejection_and_the_global_generator(pkg, lib):
    """hole_range None: every candidate of the [0, 1] stream, rasterised straight into `out`"""
    keep = np.random.get_state()
    try:
        np.random.seed(0)
        out = np.full((9, 32, 32), 99, np.uint8)
        got, ratios, backend = mc.emu_random_masks(pkg, lib, 9, 32, None, None, out=out)
        state = np.random.get_state()
    finally:
        np.random.set_state(keep)
    ref = np.random.RandomState(0)
    want = np.stack([mc.raster(mc.draw_plan(ref, 32, 1.0), 32) for _ in range(9)])
    assert got is out and np.array_equal(out, want) and backend.launches == 1
    assert (ratios == 1.0).any() and np.array_equal(ratios, [mc.hole_ratio(m) for m in want])      # all-hole candidates are kept
    assert mc.same_state(state, ref.get_state())
    rng = np.random.RandomState(0)
    got, _, backend = mc.emu_random_masks(pkg, lib, 9, 32, None, rng, chunk=4)
    assert np.array_equal(got, want) and backend.launches == 3 and mc.same_state(rng.get_state(), ref.get_state())


@pytest.mark.parametrize("r", (32, 37, 64))
def test_edge_plans(lib, mem, r):
    """both flip bits, segments along x = s and y = s, zero-length segments, every diameter, empty and full, from aligned and odd
    addresses (R = 32 and 64 take the 16-byte stores when aligned)"""
    mc.run_edge_plans(lib, mem, r)


@pytest.mark.parametrize("r", (37, 64))
def test_plan_at_every_capacity_limit(lib, mem, r):
    mc.run_capacity_plan(lib, mem, r)


def test_plans_beyond_the_capacities_are_refused_by_the_kernel(lib, mem):
    mc.run_refused_plans(lib, mem, 32)


def test_more_than_one_band(lib, mem):
    """R = 70: three bands, the last of 6 rows; flipped rows cross the bands"""
    plans = [p for _, p in mc.edge_plans(70)]
    got, holes = mc.raster_plans(lib, mem, plans, 70)
    for g, h, p in zip(got, holes, plans):
        want = mc.raster(p, 70)
        assert np.array_equal(g, want) and h == int((want == 0).sum())


def test_error_paths(pkg, lib):
    rng = np.random.RandomState(11)
    start = rng.get_state()
    for n, r, hr in ((0, 32, (0, 1)), (4, 15, (0, 1)), (4, 1025, (0, 1)), (4, 32, (0.05, 0.1)), (True, 32, (0, 1)), (4, 32.0, (0, 1)), (4, 32, (0, 1, 2))):
        with pytest.raises(ValueError):
            mc.emu_random_masks(pkg, lib, n, r, hr, rng)
    with pytest.raises(ValueError, match="at least 0.2"):
        pkg.masks.check_arguments(4, 32, (0.0, 0.19))
    assert pkg.masks.check_arguments(4, 32, (0.1, 0.1)) == 0.2 and pkg.masks.check_arguments(4, 32, None) == 1.0
    assert mc.same_state(rng.get_state(), start)                           # refused before any draw
    # a range nothing falls into: max_candidates ends it, the generator back at the call's start
    with pytest.raises(RuntimeError, match="40 candidates gave 0 of 2"):
        mc.emu_random_masks(pkg, lib, 2, 32, (0.9995, 1), rng, max_candidates=40)
    assert mc.same_state(rng.get_state(), start)
    with pytest.raises(RuntimeError, match="candidates gave 1 of 3"):
        mc.emu_random_masks(pkg, lib, 3, 32, (0, 1), rng, max_candidates=2, chunk=1)
    assert mc.same_state(rng.get_state(), start)
    with pytest.raises(TypeError, match="RandomState"):
        mc.emu_random_masks(pkg, lib, 2, 32, (0, 1), np.random.default_rng(0))
    with pytest.raises(ValueError, match="max_candidates"):
        mc.emu_random_masks(pkg, lib, 2, 32, (0, 1), rng, max_candidates=0)
    assert pkg.masks.default_max_candidates(1) == 10000 and pkg.masks.default_max_candidates(64) == 64000
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.masks.random_masks(2, 32, rng=rng)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.masks.random_masks(2, 32, rng=rng, out=torch.zeros((2, 32, 32), dtype=torch.uint8))
    assert mc.same_state(rng.get_state(), start)


def test_raster_argument_errors(lib):
    mc.run_arg_errors(lib)


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "mi-gan_amd", "csrc", "migan_masks.hpp")).read()
    assert re.search(r"kMkBand = (\d+)", text).group(1) == str(mc.BAND)
    assert re.search(r"kMkResMin = (\d+), kMkResMax = (\d+)", text).groups() == (str(mc.R_MIN), str(mc.R_MAX))
    assert re.search(r"kMkRects = (\d+), kMkStrokes = (\d+), kMkPoints = (\d+)", text).groups() == (str(mc.MAX_RECTS), str(mc.MAX_STROKES), str(mc.MAX_POINTS))
    # the row formula runs with contraction off; the only atomics are the integer ones on LDS
    assert text.count("#pragma clang fp contract(off)") >= 3
    assert set(re.findall(r"MIGAN_ATOMIC_[A-Z0-9_]+", text)) == {"MIGAN_ATOMIC_OR_U32", "MIGAN_ATOMIC_ADD_I32"}
    host = open(os.path.join(ROOT, "mi-gan_amd", "csrc", "migan_masks_host.hpp")).read()
    assert "rt::" not in host and "MIGAN_GLOBAL" not in host                # the draws make no GPU call


def test_exports(pkg):
    """the header against the binding: tests/test_abi_headers.py; here the case module against the binding"""
    hb = pkg.hipbind
    assert hb.MASKS_PLAN_WORDS_MAX == mc.PLAN_WORDS_MAX and hb.MASKS_BAND == mc.BAND
    assert pkg.masks.R_MIN == mc.R_MIN and pkg.masks.R_MAX == mc.R_MAX
    assert "masks" in pkg.__all__
