"""Photo loading on the device: mi-gan_amd/photo.py::load_eval at R = 512 (-> migan_photo_resize_batch) against the two yardsticks
it has to be read against, in one process:

  byte floor   source bytes + the uint8 intermediate written and read + destination bytes, photo and mask, over 6.3 TB/s
  the forward  Generator(512).forward_uint8 on what load_eval returned, the call it feeds

    python scripts/photo_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/photo_timing.py --reps 3 --load-only

Workloads: 32 photos of 1024 x 768 (the workload of profiles/pipeline_batch.md) and one photo of 4000 x 3000, masks of the photo's
size.  Before anything is timed the loader's bytes are compared with Pillow's where Pillow is installed (otherwise with the numpy
restatement of tests/photo_case.py), on the timed shapes.  Times are device events around each call, after a warm-up, the two calls
alternating; the spread of the repetitions is reported.  Pillow's own time for the same photo is taken on this host's CPU when it is
installed.  Seeded images: no files, no network.  Needs an MI355X; there is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def timed(fn, warmup, reps, other):
    """milliseconds of `reps` calls of fn and of other, alternating, by device events"""
    out = ([], [])
    for r in range(warmup + reps):
        for k, f in enumerate((fn, other)):
            if f is None:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def stats(ms):
    q = statistics.quantiles(ms, n=10) if len(ms) >= 10 else [min(ms)] * 9
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "p10_ms": q[0], "p90_ms": q[-1]}


def floor_bytes(n, h, w, r):
    """what load_eval has to move for n photos of h x w with masks of h x w: the photo read, [h][r][3] written and read, [r][r][3]
    written; the mask gathered ([r][r] read at most, [r][r] written)"""
    photo = h * w * 3 + 2 * h * r * 3 + r * r * 3
    mask = 2 * r * r
    return n * (photo + mask)


def make_photo(h, w, seed):
    rng = np.random.default_rng(seed)
    small = rng.random((h // 8 + 2, w // 8 + 2, 3))
    img = np.kron(small, np.ones((8, 8, 1)))[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2      # some structure, some noise
    return np.rint(img * 255).astype(np.uint8)


def make_mask(h, w):
    m = np.full((h, w), 255, np.uint8)
    m[h // 4:h // 4 * 3, w // 8:w // 8 * 5] = 0
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--load-only", action="store_true", help="only load_eval (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photo_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    r = a.resolution
    try:
        from PIL import Image
    except ImportError:
        Image = None
    model = None
    if not a.load_only:
        model = pkg.Generator(resolution=r)
        sd = pkg.synth.make_state_dict(r, seed=3)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        model = model.to(dev).eval()
    result = {"device": torch.cuda.get_device_name(0), "resolution": r, "reps": a.reps, "warmup": a.warmup, "pillow": Image is not None, "cases": []}
    for name, n, h, w in (("32 photos of 1024 x 768", 32, 768, 1024), ("one photo of 4000 x 3000", 1, 3000, 4000)):
        photos = [make_photo(h, w, 10 + i) for i in range(min(n, 2))]
        mask = make_mask(h, w)
        d_img = [torch.from_numpy(photos[i % len(photos)]).to(dev) for i in range(n)]
        d_mask = [torch.from_numpy(mask).to(dev) for _ in range(n)]
        entry = {"workload": name, "photos": n, "height": h, "width": w}
        img, msk = pkg.photo.load_eval(d_img, d_mask, r)
        if Image is not None:
            want_img = np.array(Image.fromarray(photos[0]).resize((r, r), Image.BICUBIC))
            want_msk = np.array(Image.fromarray(mask).resize((r, r), Image.NEAREST))
            entry["compared_with"] = "Pillow " + importlib.import_module("PIL").__version__
        else:
            from tests import photo_case as pc
            want_img, want_msk = pc.pil_bicubic(photos[0], (r, r)), pc.pil_nearest(mask, (r, r))
            entry["compared_with"] = "the numpy restatement of tests/photo_case.py"
        entry["differing_bytes"] = int((img[0].cpu().numpy() != want_img).sum() + (msk[0].cpu().numpy() != want_msk).sum())
        if entry["differing_bytes"] or not torch.equal(img[0], img[n - 1 - (n - 1) % len(photos)]):
            raise SystemExit(f"{name}: the loader's bytes differ: {entry}")

        def load():
            return pkg.photo.load_eval(d_img, d_mask, r)

        def forward():
            with torch.no_grad():
                return model.forward_uint8(img, msk)

        tl, tf = timed(load, a.warmup, a.reps, None if a.load_only else forward)
        entry["load_eval"] = stats(tl)
        entry["floor_bytes"] = floor_bytes(n, h, w, r)
        entry["floor_ms"] = entry["floor_bytes"] / HBM_BYTES_PER_S * 1e3
        entry["load_over_floor"] = entry["load_eval"]["median_ms"] / entry["floor_ms"]
        entry["load_gbytes_per_s"] = entry["floor_bytes"] / (entry["load_eval"]["median_ms"] * 1e-3) / 1e9
        if tf:
            entry["forward_uint8"] = stats(tf)
            entry["load_over_forward"] = entry["load_eval"]["median_ms"] / entry["forward_uint8"]["median_ms"]
        if Image is not None:                                          # this host's CPU, one photo and its mask, best of 3
            best = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                Image.fromarray(photos[0]).resize((r, r), Image.BICUBIC)
                Image.fromarray(mask).resize((r, r), Image.NEAREST)
                best = min(best, time.perf_counter() - t0)
            entry["pillow_cpu_ms_per_photo"] = best * 1e3
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
        del d_img, d_mask, img, msk
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
