"""PSNR / SSIM of completions against the photo (include/migan_metrics_hip.h) on the CPU emulator: the kernels of
mi-gan_amd/csrc/migan_metrics.hpp and the host code behind migan_metrics_batch, on host memory, against the float64 yardstick of
tests/metrics_case.py within 4 rulers (the reference's own float32 error on the same image pair), the MSE exactly (uint8) or within
the bound of a reordered fp64 sum (float32).  The same cases run on the device in tests/test_gpu_metrics.py."""
import os
import re

import numpy as np
import pytest

from tests import metrics_case as mc
from tests.emu_util import ROOT, emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def mem():
    return mc.HostMem()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case(lib, mem, name):
    mse, ssim = mc.run_case(lib, mem, name)
    c = mc.CASES[name]
    if c.get("nohole"):
        # the item without a hole pixel gets NaN in both outputs, the rows around it are right (run_case checked them)
        assert np.isnan(mse[1]).all() and np.isnan(ssim[1]).all()
        assert np.isfinite(mse[[0, 2]]).all() and np.isfinite(ssim[[0, 2]]).all()


def test_hole_straddles_a_tile_border():
    for h, w in mc.SMALL_SIZES:
        mc.assert_straddles(mc.hole_rect(h, w), h, w)
    y0, y1, x0, x1 = mc.hole_rect(2 * mc.TILE_H + 3, 3 * mc.TILE_W + 1)
    assert y0 < mc.TILE_H < y1 and x0 < mc.TILE_W < x1
    y0, y1, x0, x1 = mc.hole_rect(33, 41)
    assert y0 < mc.TILE_H < y1 and x0 < mc.TILE_W < x1


@pytest.mark.parametrize("name", ["small_u8_hwc_s3_mask", "small_f32_chw_s3"])
def test_sample_alone_is_bit_equal(lib, mem, name):
    mc.run_samples_alone(lib, mem, name)


@pytest.mark.parametrize("dtype,layout", [(mc.U8, mc.HWC), (mc.F32, mc.CHW)])
def test_identity(lib, mem, dtype, layout):
    mc.run_identity(lib, mem, dtype, layout)


def test_two_launches(lib, mem):
    mc.run_two_launches(lib, mem)


def test_argument_errors(lib, mem):
    mc.run_arg_errors(lib, mem)


def test_tile_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "mi-gan_amd", "csrc", "migan_metrics.hpp")).read()
    assert re.search(r"kMetTW = (\d+), kMetTH = (\d+)", text).groups() == (str(mc.TILE_W), str(mc.TILE_H))
    assert re.search(r"kMetItemsMax = (\d+)", text).group(1) == str(mc.ITEMS_PER_LAUNCH)
    assert re.search(r"kMetR = (\d+)", text).group(1) == str(mc.HALO)
    # the taps in the kernel text are the reference's float32 values
    taps = [float.fromhex(t) for t in re.search(r"#define MIGAN_MET_TAPS \{(.*?)\}", text, flags=re.S).group(1).replace("\\", " ").replace("f,", ",")
            .rstrip("f").split(",")]
    assert np.array_equal(np.asarray(taps, dtype=np.float32), mc.taps32().numpy()) and len(taps) == 11


def test_exports(pkg):
    """the header against the binding: tests/test_abi_headers.py; here the case module's codes against the binding's"""
    hb = pkg.hipbind
    assert (mc.U8, mc.F32, mc.CHW, mc.HWC) == (hb.METRICS_U8, hb.METRICS_F32, hb.METRICS_CHW, hb.METRICS_HWC)
