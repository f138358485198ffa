"""Random hole masks on the MI355X: the cases of tests/masks_case.py (those of tests/test_emu_masks.py) through
mi-gan_amd.masks.random_masks and migan_masks_raster on device memory.  Only the goldens are read (tests/golden/masks_*.npz: what the
reference's RandomMask returned, and the state it left numpy's generator in); every comparison is equality of bytes."""
import os

import numpy as np
import pytest
import torch

from tests import masks_case as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def mem():
    return mc.CudaMem(DEV)


def _t(a):
    return torch.from_numpy(np.array(a))                          # (a writable copy: the goldens are read-only)


@pytest.mark.parametrize("entry", mc.GOLDENS, ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_goldens(pkg, entry):
    """the reference's masks for the seed, and `rng` advanced exactly as the golden's stored state says"""
    seed, r, hole_range, n = entry
    want, state, _ = mc.golden(seed, r, hole_range)
    rng = np.random.RandomState(seed)
    got, ratios = pkg.masks.random_masks(n, r, hole_range, rng=rng, device=DEV, return_hole_ratio=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, r, r) and got.is_cuda and got.is_contiguous()
    assert torch.equal(got.cpu(), _t(want)), f"{int((got.cpu() != _t(want)).sum())} bytes differ"
    assert mc.same_state(rng.get_state(), state)
    assert ratios.dtype == torch.float64 and np.array_equal(ratios.numpy(), [mc.hole_ratio(m) for m in want])


@pytest.mark.parametrize("entry", (mc.SMALL[1], mc.SMALL[3]), ids=lambda e: f"r{e[1]}_{e[2][0]}_{e[2][1]}")
def test_chunk_sizes_give_the_same_masks_and_state(pkg, entry):
    seed, r, hole_range, n = entry
    n = min(n, 12)
    want, _, _ = mc.golden(seed, r, hole_range)
    ref = np.random.RandomState(seed)
    _, drawn, _ = mc.random_masks(n, r, hole_range, ref)
    for chunk in (1, 7, drawn):
        rng = np.random.RandomState(seed)
        got = pkg.masks.random_masks(n, r, hole_range, rng=rng, device=DEV, chunk=chunk)
        assert torch.equal(got.cpu(), _t(want[:n])), f"chunk {chunk}"
        assert mc.same_state(rng.get_state(), ref.get_state()), f"chunk {chunk}"


def test_out_no_rejection_and_the_global_generator(pkg):
    keep = np.random.get_state()
    try:
        np.random.seed(0)
        out = torch.full((9, 32, 32), 99, dtype=torch.uint8, device=DEV)
        got = pkg.masks.random_masks(9, 32, None, out=out)
        state = np.random.get_state()
    finally:
        np.random.set_state(keep)
    ref = np.random.RandomState(0)
    want = np.stack([mc.raster(mc.draw_plan(ref, 32, 1.0), 32) for _ in range(9)])
    assert got is out and torch.equal(out.cpu(), _t(want)) and mc.same_state(state, ref.get_state())
    # `out` with rejection: the accepted candidates are gathered into it
    want, state, _ = mc.golden(0, 64, (0.2, 0.4))
    rng = np.random.RandomState(0)
    out = torch.full((16, 64, 64), 99, dtype=torch.uint8, device=DEV)
    assert pkg.masks.random_masks(16, 64, (0.2, 0.4), rng=rng, out=out) is out
    assert torch.equal(out.cpu(), _t(want)) and mc.same_state(rng.get_state(), state)


def test_non_default_stream(pkg):
    want, state, _ = mc.golden(0, 37, (0, 1))
    stream = torch.cuda.Stream(device=DEV)
    rng = np.random.RandomState(0)
    with torch.cuda.stream(stream):
        got = pkg.masks.random_masks(64, 37, (0, 1), rng=rng, device=DEV)
    stream.synchronize()
    assert torch.equal(got.cpu(), _t(want)) and mc.same_state(rng.get_state(), state)


@pytest.mark.parametrize("r", (32, 37, 64))
def test_edge_plans(lib, mem, r):
    mc.run_edge_plans(lib, mem, r)


@pytest.mark.parametrize("r", (37, 64))
def test_plan_at_every_capacity_limit(lib, mem, r):
    mc.run_capacity_plan(lib, mem, r)


def test_plans_beyond_the_capacities_are_refused_by_the_kernel(lib, mem):
    mc.run_refused_plans(lib, mem, 32)


def test_more_than_one_band_and_the_largest_size(lib, mem):
    for r in (70, 1024):
        plans = [p for _, p in mc.edge_plans(r)] + ([mc.capacity_plan(r)] if r == 70 else [])
        got, holes = mc.raster_plans(lib, mem, plans, r)
        for g, h, p in zip(got, holes, plans):
            want = mc.raster(p, r)
            assert np.array_equal(g, want) and h == int((want == 0).sum())


def test_two_runs_give_the_same_bytes(pkg):
    a = pkg.masks.random_masks(6, 512, (0, 1), rng=np.random.RandomState(5), device=DEV)
    b = pkg.masks.random_masks(6, 512, (0, 1), rng=np.random.RandomState(5), device=DEV)
    assert torch.equal(a, b) and bool(((a == 0) | (a == 255)).all())


def test_forward_uint8_takes_the_masks_unchanged(pkg):
    """Generator(16): forward_uint8(img, random_masks(...)) is forward_uint8 of the same bytes from the host, known pixels kept"""
    m = pkg.Generator(resolution=16)
    sd = pkg.synth.make_state_dict(16, seed=13)
    m.load_state_dict({k: _t(v.copy()) for k, v in sd.items()})
    m = m.to(DEV).eval()
    rng = np.random.RandomState(2)
    masks = pkg.masks.random_masks(5, 16, (0.1, 0.9), rng=rng, device=DEV)
    ref = np.random.RandomState(2)
    want_masks, _, _ = mc.random_masks(5, 16, (0.1, 0.9), ref)
    assert torch.equal(masks.cpu(), _t(want_masks)) and mc.same_state(rng.get_state(), ref.get_state())
    img = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (5, 16, 16, 3)).astype(np.uint8)).to(DEV)
    with torch.no_grad():
        got = m.forward_uint8(img, masks)
        want = m.forward_uint8(img, _t(want_masks).to(DEV))
    assert torch.equal(got, want) and bool((got[masks == 255] == img[masks == 255]).all())
    # the training formatters' form
    f = (masks / 255).float()[:, None]
    assert tuple(f.shape) == (5, 1, 16, 16) and set(f.unique().tolist()) <= {0.0, 1.0}


def test_error_paths(pkg):
    rng = np.random.RandomState(11)
    start = rng.get_state()
    rm = pkg.masks.random_masks
    for n, r, hr in ((0, 32, (0, 1)), (4, 15, (0, 1)), (4, 1025, (0, 1)), (4, 32, (0.05, 0.1))):
        with pytest.raises(ValueError):
            rm(n, r, hr, rng=rng, device=DEV)
    with pytest.raises(RuntimeError, match="40 candidates gave 0 of 2"):
        rm(2, 32, (0.9995, 1), rng=rng, device=DEV, max_candidates=40)
    assert mc.same_state(rng.get_state(), start)
    with pytest.raises(TypeError, match="RandomState"):
        rm(2, 32, rng=np.random.default_rng(0), device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rm(2, 32, rng=rng, device="cpu")
    with pytest.raises(RuntimeError, match="out must be"):
        rm(2, 32, rng=rng, out=torch.zeros((2, 32, 33), dtype=torch.uint8, device=DEV))
    assert mc.same_state(rng.get_state(), start)


def test_raster_argument_errors(lib):
    mc.run_arg_errors(lib)


def test_exports_in_the_built_libraries(pkg, lib):
    assert lib.backend() == "hip:gfx950"
    for path in (pkg.library_path(), os.path.join(os.path.dirname(pkg.library_path()), "libmigan_hip_nanclamp.so")):
        loaded = pkg.hipbind.MiganLib(path)
        for name in pkg.hipbind.exports("migan_masks_hip.h"):
            assert hasattr(loaded.lib, name), f"{path} does not export {name}"
