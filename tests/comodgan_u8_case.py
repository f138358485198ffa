"""Shared by tests/test_emu_comodgan_u8.py and tests/test_gpu_comodgan_u8.py (include/comodgan_u8_hip.h): the configurations that
reach every form of the two uint8 kernels, and the uint8 inputs.  Test infrastructure only."""
import importlib

import numpy as np

pkg = importlib.import_module("mi-gan_amd")
cs = importlib.import_module("mi-gan_amd.comodgan_schema")


def config(r, ch_base, ch_max):
    return cs.Config(resolution=r, ch_base=ch_base, ch_max=ch_max, num_ws=cs.default_num_ws(r))


# name -> (config, images, samples, forward options, fp16 (before_res, after_res, storage) or None)
#   lpp4    64 channels at R (4 lanes per pixel); N = 2, S = 3: the smallest case where b / S is neither b nor 0
#   lpp8    128 channels (8 lanes per pixel); the plain forward, with a truncation cutoff
#   lpp16   256 channels (16 lanes per pixel) at the smallest resolution a handle takes; an odd batch, 3 * 64 pixels, S = 2
#   fp16    the top blocks half precision with fp16 storage: the fp16-output FromRGB and the fp16-input last ToRGB
CASES = {
    "lpp4": (config(16, 1024, 64), 2, 3, {}, None),
    "lpp8": (config(32, 4096, 128), 1, 1, dict(truncation_psi=0.6, truncation_cutoff=3), None),
    "lpp16": (config(8, 2048, 256), 3, 2, {}, None),
    "fp16": (config(16, 1024, 64), 2, 2, {}, (8, 8, True)),
}


def noise_floats(r):
    """comodgan_noise_floats: per image, 16 + 2 res^2 for res = 8 ... R"""
    return 16 + sum(2 * res * res for res in (1 << k for k in range(3, r.bit_length())))


def make_u8(batch, r, seed):
    """synth.make_uint8_input with a few mask bytes at 128 (a hole by the == 255 rule) and, where the drawn strokes cover less, rows
    punched out from the bottom until a quarter of the pixels are holes.  -> img [N,R,R,3], mask [N,R,R], both uint8, contiguous"""
    img, mask = pkg.synth.make_uint8_input(batch, r, seed)
    img, mask = np.ascontiguousarray(img), np.ascontiguousarray(mask)
    mask[0, :2, :3] = 128
    mask[-1, r // 2, r // 2:] = 128
    row = r
    while (mask != 255).mean() < 0.25:
        row -= 1
        mask[:, row, :] = 0
    assert (mask != 255).mean() >= 0.25 and (mask == 255).mean() >= 0.25, ((mask != 255).mean(), (mask == 255).mean())
    assert ((mask != 255) & (mask != 0)).any()
    return img, mask
