"""Crops at native size (include/migan_pipeline_native_hip.h: migan_pipeline_native_pre / _post) run on the CPU through the fiber
emulator: the product's kernels (mi-gan_amd/csrc/migan_pipeline_native.inc) and host code against the closed form and the pipeline
oracle of tests/pipeline_native_case.py, and against migan_pipeline_regions_pre / _post where the two must agree bit for bit.  Also
the window rule of MIGAN_Pipeline.forward_native, which is plain integers.  The generator is not under test: y is seeded random."""
import numpy as np
import pytest
import torch

from tests import pipeline_native_case as nc
from tests.emu_util import emu_lib, ptr

BUFS = nc.Buffers(to_dev=lambda a: np.array(a, copy=True), ptr=ptr, to_np=lambda a: np.array(a, copy=True))


@pytest.fixture(scope="module")
def lib():
    lib = emu_lib()
    assert hasattr(lib.lib, "migan_pipeline_native_pre"), "the emulator library lacks the native entry points"
    return lib


@pytest.mark.parametrize("name", sorted(nc.CHECKS))
def test_kernels(lib, name):
    nc.CHECKS[name](lib, BUFS)


@pytest.fixture(scope="module")
def pipe(pkg):
    """the window rule reads the resolution and nothing else: no generator, no device"""
    return pkg.pipeline.MIGAN_Pipeline(torch.nn.Identity(), nc.RES, padding=nc.PADDING, device="cpu")


@pytest.mark.parametrize("args,want", nc.WINDOW_TABLE)
def test_window_rule_table(pipe, args, want):
    box, h, w = args
    assert pipe.native_window(box, h, w) == want
    nc.check_window_properties(pipe, box, h, w)


def test_window_rule_always(pipe):
    """every reference box of a seeded sweep of photo sizes and holes: inside the photo, no larger than the window, both multiples of
    q, containing the box; an R x R box stays R x R"""
    rng = np.random.default_rng(31)
    seen_padded = seen_clamped = seen_same = 0
    for n in range(400):
        h, w = (int(v) for v in rng.integers(3, 260, 2))
        y0, x0 = int(rng.integers(0, h - 2)), int(rng.integers(0, w - 2))
        y1, x1 = int(rng.integers(y0 + 3, h + 1)), int(rng.integers(x0 + 3, w + 1))
        if n % 4 == 0:                                                   # a box whose sides are multiples of q already
            x1, y1 = min(w, x0 + 16 * max(1, (x1 - x0) // 16)), min(h, y0 + 16 * max(1, (y1 - y0) // 16))
        box = (x0, x1, y0, y1)
        nc.check_window_properties(pipe, box, h, w)
        got, (hc, wc) = pipe.native_window(box, h, w)
        seen_padded += wc > w or hc > h
        seen_clamped += wc <= w and (got[0] == 0 or got[1] == w) and got[:2] != box[:2]
        seen_same += got == box
    assert seen_padded and seen_clamped and seen_same
    assert pipe.native_window((100, 164, 30, 94), 157, 203) == ((100, 164, 30, 94), (64, 64))
