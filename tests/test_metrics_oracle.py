"""The yardsticks of the PSNR / SSIM tests (tests/metrics_case.py) against the reference's own results (tests/golden/metrics_*.npz,
tests/golden/make_golden_metrics.py): the float32 restatement gives what lib/evaluator/eva_ssim.py::compute_ssim gave, the float64
restatement lies within the ruler of the float32 one, and the MSE expression gives eva_psnr.py:34-56's PSNR."""
import glob
import os

import numpy as np
import pytest

from tests import metrics_case as mc

GOLDENS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_*.npz")))


def test_goldens_exist():
    assert len(GOLDENS) == 4 and all(os.path.getsize(p) < 64 * 1024 for p in GOLDENS)


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[8:-4])
def test_restatements_against_the_reference(path):
    z = np.load(path)
    gt, pred, vr = z["gt"], z["pred"], tuple(float(v) for v in z["value_range"])
    assert np.array_equal(mc.taps32().numpy(), z["window"])           # bit for bit the reference's gaussian(11, 1.5)
    e = mc.expected(gt, pred, value_range=vr)
    # float32 rounding of a value <= 1 (torch's convolution may pick another summation order on another machine)
    np.testing.assert_allclose(e["ssim32"], z["ssim"].astype(np.float64), rtol=0, atol=2e-7)
    print(os.path.basename(path), "float32 restatement vs reference", np.abs(e["ssim32"] - z["ssim"]).max(), "rulers", e["ruler"])
    # |mean(a) - mean(b)| <= mean|a - b|: the ruler bounds the distance of the two restatements, and it is float32-sized
    assert (np.abs(e["ssim"] - e["ssim32"]) <= e["ruler"]).all() and (e["ruler"] < 2e-5).all() and (e["ruler"] > 0).all()
    # eva_psnr.py:56 on a float32 mean of 3 H W terms: a relative error of a few 2^-24 in the mse is 4.3 * that in dB
    np.testing.assert_allclose(-10.0 * np.log10(e["mse"]), z["psnr_none"].astype(np.float64), rtol=0, atol=2e-5)
    e8 = mc.expected(gt, pred, shave=8, value_range=vr)
    assert e8["count"] == 3 * (gt.shape[1] - 16) * (gt.shape[2] - 16)
    np.testing.assert_allclose(-10.0 * np.log10(e8["mse"]), z["psnr_div2k"].astype(np.float64), rtol=0, atol=2e-5)


def test_regions():
    mask = np.full((20, 24), 255, dtype=np.uint8)
    mask[2:12, 3:9] = 7
    p, s = mc.regions(20, 24, mask, 4)
    assert s.sum() == 60 and p.sum() == 8 * 5 and not p[:4].any() and p[4:12, 4:9].all()
    p, s = mc.regions(20, 24, None, 0)
    assert p.all() and s.all()
