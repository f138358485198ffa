#!/usr/bin/env python3
"""Goldens of the random-mask tests (include/migan_masks_hip.h): what the reference's own RandomMask (scripts/generate_masks.py:16-93,
with the installed numpy and Pillow) returns for a seed, bit-packed, with the state of numpy's legacy generator after the run and the
number of candidates it drew (tests/golden/masks_*.npz, 5 - 20 KB each).  lib/data_factory/ds_ffhq.py's
copy of the function is run for the first masks of every entry and must agree.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masks.py
"""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MIGAN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests import masks_case as mc                              # noqa: E402  (the list of entries and the file names only)


def load_generate_masks():
    if importlib.util.find_spec("tqdm") is None:                # (only main() uses it)
        tqdm = types.ModuleType("tqdm")
        tqdm.tqdm = lambda it, **kw: it
        sys.modules["tqdm"] = tqdm
    spec = importlib.util.spec_from_file_location("ref_generate_masks", os.path.join(REF, "scripts", "generate_masks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_ffhq_copy():
    """RandomBrush / RandomMask of lib/data_factory/ds_ffhq.py:148-225, without the module around them (it imports the training stack)"""
    text = open(os.path.join(REF, "lib", "data_factory", "ds_ffhq.py")).read()
    start = text.index("def RandomBrush(")
    after = text.index("\n", text.index("def RandomMask(")) + 1
    end = re.search(r"^\S", text[after:], flags=re.M)                # the first unindented line behind RandomMask
    body = text[start:] if end is None else text[start:after + end.start()]
    import math
    from PIL import Image, ImageDraw
    scope = {"np": np, "math": math, "Image": Image, "ImageDraw": ImageDraw, "PIL": PIL}
    exec(compile(body, "ds_ffhq_masks", "exec"), scope)
    return scope["RandomMask"]


def main():
    ref = load_generate_masks()
    ffhq = load_ffhq_copy()
    calls = [0]
    brush = ref.RandomBrush

    def counted(*a, **kw):
        calls[0] += 1
        return brush(*a, **kw)
    ref.RandomBrush = counted
    for seed, r, hole_range, n in mc.GOLDENS:
        np.random.seed(seed)
        calls[0] = 0
        masks = np.stack([ref.RandomMask(r, list(hole_range)) for _ in range(n)])
        state = np.random.get_state()
        assert masks.dtype == np.uint8 and set(np.unique(masks)) <= {0, 255}
        np.random.seed(seed)
        k = min(n, 4)
        again = np.stack([ffhq(r, list(hole_range)) for _ in range(k)])
        assert np.array_equal(np.asarray(again).reshape(k, r, r) > 0, masks[:k] > 0), "ds_ffhq.py's copy disagrees"
        path = os.path.join(HERE, mc.golden_name(seed, r, hole_range))
        np.savez_compressed(path, bits=np.packbits(masks.reshape(-1) // 255), n=n, key=state[1], pos=state[2], has_gauss=state[3], gauss=state[4],
                            candidates=calls[0], numpy=np.__version__, pillow=PIL.__version__)
        print(os.path.basename(path), n, "masks", calls[0], "candidates", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
