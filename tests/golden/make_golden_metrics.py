#!/usr/bin/env python3
"""Goldens of the PSNR / SSIM evaluators (include/migan_metrics_hip.h): seeded uint8 / float32 image pairs with

  ssim        the reference's own lib/evaluator/eva_ssim.py::compute_ssim(pred, gt, size_average=False) on the normalised float32
              images, on the CPU, and the window gaussian(11, 1.5) it is built from
  psnr_none   the expression of lib/evaluator/eva_psnr.py:34-56 for for_dataset=None    (the line references are in psnr_lines below;
  psnr_div2k  ... and for for_dataset='div2k', scale=2                                   the evaluator CLASS cannot run here: its
              sync() moves tensors to a GPU rank)

Stored per case (tests/golden/metrics_*.npz, a few KB): gt [3,H,W], pred [S,3,H,W], value_range, and the three results [S].
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MIGAN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from lib.evaluator.eva_ssim import compute_ssim, gaussian      # noqa: E402  (the reference's)
from tests import metrics_case as mc                           # noqa: E402  (images and normalisation only)


def psnr_lines(pred, gt, for_dataset, scale=2, rgb_range=1):
    """eva_psnr.py:34-56 on numpy float32 [S,3,H,W] (add_batch's arguments after the shape checks)"""
    diff = (pred - gt) / rgb_range                             # :34
    if for_dataset is None:                                    # :36
        valid = diff                                           # :37
    elif for_dataset == 'div2k':                               # :45
        shave = scale + 6                                      # :46
        valid = diff[:, :, shave:-shave, shave:-shave]         # :47
    mse = (valid**2).mean(axis=(1, 2, 3))                      # :54
    return -10*np.log10(mse)                                   # :56


def main():
    cases = {
        "u8_noise": ("noise", 20, 24, mc.U8, (0.0, 1.0)),
        "u8_smooth": ("smooth", 23, 19, mc.U8, (0.0, 1.0)),
        "f32_smooth": ("smooth", 20, 24, mc.F32, (0.0, 1.0)),
        "f32_noise_pm1": ("noise", 19, 21, mc.F32, (-1.0, 1.0)),
    }
    for name, (kind, h, w, dtype, vr) in cases.items():
        gt, pred, _ = mc.make_item(kind, h, w, 2, dtype, 11, with_mask=False, value_range=vr)
        pred = pred.copy()
        pred[1] = mc.image("smooth" if kind == "noise" else "noise", h, w, 12, dtype, vr)       # one completion differs everywhere
        g = mc.normalise(gt[None], vr).expand(2, -1, -1, -1).contiguous()
        p = mc.normalise(pred, vr)
        ssim = compute_ssim(p, g, size_average=False).numpy()
        out = dict(gt=gt, pred=pred, value_range=np.asarray(vr, dtype=np.float32), ssim=ssim, window=gaussian(11, 1.5).numpy(),
                   psnr_none=psnr_lines(p.numpy(), g.numpy(), None), psnr_div2k=psnr_lines(p.numpy(), g.numpy(), 'div2k'))
        path = os.path.join(HERE, f"metrics_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes", "ssim", ssim, "psnr", out["psnr_none"], out["psnr_div2k"])


if __name__ == "__main__":
    main()
