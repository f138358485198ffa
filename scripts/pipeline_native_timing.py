"""Deployed pipeline, crops at native size: what the larger forward costs, on 8 photos of 2048 x 1536 with one hole of about
600 x 600 each.

    python scripts/pipeline_native_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pipeline_native_timing.py --reps 3 --skip-end-to-end

  * the window the rule gives every photo.
  * migan_pipeline_native_pre / _post on the windows against migan_pipeline_regions_pre / _post (pipe_pre_rows_kernel,
    pipe_post_rows_kernel) on the reference's boxes of the same photos, each on seeded y rows of its own size, alternating in one
    process; with the box pixels, ns per box pixel of the two post kernels and the bytes per second of the two pre kernels.  Under
    rocprofv3 the kernels' own times are in the trace; here a repetition is one launch between device events.
  * the generator at R x R (model(x), 8 rows) against the window size (forward_any_size, 8 rows).
  * forward_native against forward_regions, whole calls, on the same photos.

Synthetic weights, seeded smooth photos: no files, no network, and nothing here says anything about image quality.  Every repetition
runs between device events and a synchronise; the paths alternate, so that a drift of the machine hits both.  Needs an MI355X; there
is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_photo(height, width, hole, seed, dev):
    """a smooth seeded photo (low-frequency noise upsampled) and a mask with the (y, x, h, w) rectangle"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, height // 50 + 2, width // 50 + 2), generator=g)
    photo = (torch.nn.functional.interpolate(low, size=(height, width), mode="bicubic", align_corners=False).clamp(0, 1) * 255).to(torch.uint8)
    mask = np.full((1, 1, height, width), 255, dtype=np.uint8)
    y, x, h, w = hole
    mask[0, 0, y:y + h, x:x + w] = 0
    return photo.to(dev).contiguous(), torch.from_numpy(mask).to(dev)


def event_ms(fn, reset=None):
    if reset:
        reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def alternate(fns, warmup, reps, reset=None):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(event_ms(fn, reset))
    return {name: stats(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--height", type=int, default=1536)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--photos", type=int, default=8)
    ap.add_argument("--hole", type=int, default=600, help="side of the square hole of every photo")
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_native_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    res, h, w, s, n = a.resolution, a.height, a.width, a.hole, a.photos
    sd = pkg.synth.make_state_dict(res, seed=1, regime="export")
    model = pkg.Generator(resolution=res)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    pipe = pkg.pipeline.MIGAN_Pipeline(model, res, padding=a.padding, device=dev)
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    # the holes wander over the photo, by odd steps: the boxes begin at any column
    holes = [((37 + 97 * i) % (h - s - 1), (53 + 211 * i) % (w - s - 1), s, s - 3 * (i % 3)) for i in range(n)]
    photos, masks = zip(*[make_photo(h, w, hole, 11 + i, dev) for i, hole in enumerate(holes)])
    work = [p.clone() for p in photos]

    def reset():
        for wk, p in zip(work, photos):
            wk.copy_(p)

    # ---- boxes and windows: one box per photo (the holes are single regions), through the pipeline's own host code ----
    _, calls = pipe.forward_native(work, masks, return_rows=True)
    reset()
    _, used, _ = pipe.forward_regions(work, masks, return_regions=True)
    reset()
    assert len(calls) == 1 and len(calls[0][2]) == n, f"the photos were built for one call of {n} rows, got {[(c[0], c[1], len(c[2])) for c in calls]}"
    hc, wc, listed = calls[0]
    boxes_ref = [u[0].tolist() for u in used]
    boxes_win = [list(box) for _, _, box in listed]
    result = {"device": torch.cuda.get_device_name(0), "resolution": res, "size": [h, w], "photos": n, "holes": holes, "padding": a.padding,
              "reps": a.reps, "warmup": a.warmup, "window": [hc, wc], "boxes_reference": boxes_ref, "boxes_window": boxes_win}
    rows_ref = [(wk.data_ptr(), m.data_ptr(), None, h, w, 0, b) for wk, m, b in zip(work, masks, boxes_ref)]
    rows_win = [(wk.data_ptr(), m.data_ptr(), None, h, w, 0, b) for wk, m, b in zip(work, masks, boxes_win)]
    px_ref = sum((b[1] - b[0]) * (b[3] - b[2]) for b in boxes_ref)
    px_win = sum((b[1] - b[0]) * (b[3] - b[2]) for b in boxes_win)

    # ---- the stages around the generator, through the C ABI, on seeded y ----
    rng = np.random.default_rng(3)
    y_r = torch.from_numpy((rng.standard_normal((n, 3, res, res)) * 0.6).astype(np.float32)).to(dev)
    y_n = torch.from_numpy((rng.standard_normal((n, 3, hc, wc)) * 0.6).astype(np.float32)).to(dev)
    x_r = torch.empty((n, 4, res, res), dtype=torch.float32, device=dev)
    x_n = torch.empty((n, 4, hc, wc), dtype=torch.float32, device=dev)
    stages = {"regions_pre": lambda: lib.pipeline_regions_pre(rows_ref, res, x_r.data_ptr(), stream),
              "native_pre": lambda: lib.pipeline_native_pre(rows_win, hc, wc, x_n.data_ptr(), stream),
              "regions_post": lambda: lib.pipeline_regions_post(rows_ref, res, y_r.data_ptr(), gauss25=pipe._gauss, stream=stream),
              "native_post": lambda: lib.pipeline_native_post(rows_win, hc, wc, y_n.data_ptr(), gauss25=pipe._gauss, stream=stream)}
    result["stages_ms"] = alternate(stages, a.warmup, a.reps, reset)
    med = {k: v["median"] for k, v in result["stages_ms"].items()}
    result["post_box_pixels"] = {"regions": px_ref, "native": px_win}
    result["post_ns_per_box_pixel"] = {"regions": med["regions_post"] * 1e6 / px_ref, "native": med["native_post"] * 1e6 / px_win}
    # bytes the algorithm needs: 4 read per pixel of the source (regions: four taps of three planes and the mask, from the box; counted
    # as the box's 4 bytes per pixel once) and 16 written per pixel of x
    result["pre_bytes"] = {"regions": 4 * px_ref + 16 * n * res * res, "native": 4 * px_win + 16 * n * hc * wc}
    result["pre_gb_per_s"] = {"regions": result["pre_bytes"]["regions"] / (med["regions_pre"] * 1e6),
                              "native": result["pre_bytes"]["native"] / (med["native_pre"] * 1e6)}

    # ---- the generator at R x R and at the window size, n rows each ----
    gen = {"generator_RxR": lambda: model(x_r), "generator_window": lambda: model.forward_any_size(x_n)}
    result["generator_ms"] = alternate(gen, a.warmup, a.reps)

    # ---- whole calls ----
    if not a.skip_end_to_end:
        ends = {"forward_regions": lambda: pipe.forward_regions(work, masks), "forward_native": lambda: pipe.forward_native(work, masks)}
        result["end_to_end_ms"] = alternate(ends, a.warmup, a.reps, reset)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
