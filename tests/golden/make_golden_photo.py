#!/usr/bin/env python3
"""Goldens of the photo-loading tests (include/migan_photo_hip.h): seeded uint8 inputs with the bytes Pillow and the reference's own
functions make of them (tests/golden/photo_*.npz, a few hundred KB in all).

  photo_bicubic / photo_nearest / photo_batch   Image.resize((w, h), Image.BICUBIC | Image.NEAREST) as scripts/evaluate_fid_lpips.py:143 /
                                                :149 call it; the flag cases apply demo.py:42-44's two lines to Pillow's result
  photo_flows   eval   lines :142-149 of scripts/evaluate_fid_lpips.py (that script cannot be imported without lpips)
                demo   the reference's own resize, read_mask and preprocess of scripts/demo.py, imported with cv2 stubbed (the front
                       half never calls it); the mask reaches read_mask as a PNG file, as it does in the script

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_photo.py
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MIGAN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests import photo_case as pc                              # noqa: E402  (cases and inputs only)


def load_demo_script():
    cv2 = types.ModuleType("cv2")                               # (not installed; demo.py's front half never calls it)
    cv2.INTER_CUBIC = 2
    sys.modules.setdefault("cv2", cv2)
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_demo_photo", os.path.join(REF, "scripts", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pil_resize(a, size, resample):
    return np.array(Image.fromarray(a).resize(size, resample))


def save(name, out):
    path = os.path.join(HERE, f"photo_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, len(out), "arrays", os.path.getsize(path), "bytes")


def main():
    out = {}
    for name, (_, (h, w)) in pc.BICUBIC_CASES.items():
        src = pc.bicubic_source(name)
        out[f"{name}.src"], out[f"{name}.out"] = src, pil_resize(src, (w, h), Image.BICUBIC)
    save("bicubic", out)

    out = {}
    for name, (_, (h, w), _) in pc.NEAREST_CASES.items():
        src = pc.nearest_source(name)
        out[f"{name}.src"], out[f"{name}.out"] = src, pil_resize(src, (w, h), Image.NEAREST)
    src = pc.flag_mask()
    out["flags.src"] = src
    for flags in (pc.INVERT, pc.THRESHOLD, pc.INVERT | pc.THRESHOLD):
        for size in ((10, 12), (7, 17)):
            mask = pil_resize(src, size, Image.NEAREST)
            if flags & pc.INVERT:
                mask = 255 - mask                               # demo.py:43
            if flags & pc.THRESHOLD:
                mask[mask < 255] = 0                            # demo.py:44
            out[f"flags.{flags}.{size[0]}x{size[1]}"] = mask
    save("nearest", out)

    out = {}
    for name, srcs, sizes in (("b5", pc.batch5_sources(), pc.BATCH5_SIZES), ("b33", pc.batch33_sources(), pc.batch33_sizes())):
        for i, (s, size) in enumerate(zip(srcs, sizes)):
            out[f"{name}.src{i}"], out[f"{name}.out{i}"] = s, pil_resize(s, size, Image.BICUBIC)
    for i, (s, size) in enumerate(zip(pc.batch33_sources(), pc.batch33_sizes())):
        m = np.ascontiguousarray(s[:, :, 1])
        m[m > 128] = 255
        o = pil_resize(m, size, Image.NEAREST)
        o[o < 255] = 0
        out[f"m33.src{i}"], out[f"m33.out{i}"] = m, o
    save("batch", out)

    demo = load_demo_script()
    photos, masks = pc.flow_inputs()
    out = {}
    for i, (p, m) in enumerate(zip(photos, masks)):
        out[f"photo{i}"], out[f"mask{i}"] = p, m
    with tempfile.TemporaryDirectory() as tmp:
        for i, m in enumerate(masks):
            Image.fromarray(m).save(os.path.join(tmp, f"{i}.png"))
        for r in pc.FLOW_RESOLUTIONS:
            imgs, msks = [], []
            for p, m in zip(photos, masks):
                img = Image.fromarray(p).convert("RGB")                                 # evaluate_fid_lpips.py:141
                if img.size[0] != r or img.size[1] != r:                                # :142
                    img = img.resize((r, r), Image.BICUBIC)                             # :143
                mask = Image.fromarray(m).convert("L")                                  # :148
                mask = mask.resize((r, r), Image.NEAREST)                               # :149
                imgs.append(np.array(img))
                msks.append(np.array(mask))
            out[f"eval.r{r}.img"], out[f"eval.r{r}.mask"] = np.stack(imgs), np.stack(msks)
            for invert in (False, True):
                imgs, msks = [], []
                for i, p in enumerate(photos):
                    img = Image.fromarray(p).convert("RGB")                             # demo.py:125
                    img_resized = demo.resize(img, max_size=r)                          # :126
                    mask = demo.read_mask(os.path.join(tmp, f"{i}.png"), invert=invert)  # :127
                    mask_resized = demo.resize(mask, max_size=r, interpolation=Image.NEAREST)      # :128
                    x = demo.preprocess(img_resized, mask_resized, r).numpy()           # :130
                    # preprocess keeps the photo only where the mask is 1: its two resizes (:57-58) again, and x must agree with them
                    img8 = np.array(img_resized.resize((r, r), Image.BICUBIC))
                    mask8 = np.array(mask_resized.resize((r, r), Image.NEAREST))
                    m01 = (mask8 // 255).astype(np.float32)
                    assert set(np.unique(mask8)) <= {0, 255}
                    assert np.array_equal(x[0, 0], m01 - 0.5)
                    assert np.array_equal(x[0, 1:], (img8.astype(np.float32) * 2 / 255 - 1).transpose(2, 0, 1) * m01[None])
                    imgs.append(img8)
                    msks.append(mask8)
                key = f"demo.r{r}" + (".inv" if invert else "")
                out[f"{key}.img"], out[f"{key}.mask"] = np.stack(imgs), np.stack(msks)
    save("flows", out)


if __name__ == "__main__":
    main()
