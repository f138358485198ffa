"""Deployed pipeline, one crop per hole region: what splitting costs and what surrounds it, on one large photo with three marked
objects far apart.

    python scripts/pipeline_regions_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pipeline_regions_timing.py --reps 3

  * migan_pipeline_regions_find + _pre + _post (three rows) against migan_pipeline_batch_pre + _post (one box) on the same photo,
    with the same seeded y rows, alternating in one process.  The batch entry points are the parent's, unchanged.
  * the generator at batch 3 against batch 1.
  * forward_regions against forward_batch end to end, and metrics.psnr_ssim of both over the hole against the photo.  With synthetic
    weights the quality figures show that the plumbing works, nothing about completions.

Synthetic weights, a seeded smooth photo: no files, no network.  Every repetition runs between device events and a synchronise;
the paths alternate, so that a drift of the machine hits both.  Needs an MI355X; there is no CPU path."""
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


def make_photo(height, width, holes, seed, dev):
    """a smooth seeded photo (low-frequency noise upsampled) and a mask with the given (y, x, h, w) rectangles"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, height // 50 + 2, width // 50 + 2), generator=g)
    photo = (torch.nn.functional.interpolate(low, size=(height, width), mode="bicubic", align_corners=False).clamp(0, 1) * 255).to(torch.uint8)
    mask = np.full((1, 1, height, width), 255, dtype=np.uint8)
    for y, x, h, w in holes:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--hole", type=int, default=160, help="side of the three square holes")
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--gap", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_regions_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    res, h, w, s = a.resolution, a.height, a.width, a.hole
    sd = pkg.synth.make_state_dict(res, seed=1, regime="export")
    model = pkg.Generator(resolution=res)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    pipe = pkg.pipeline.MIGAN_Pipeline(model, res, padding=a.padding, device=dev)
    gap = max(2, a.padding // 4) if a.gap is None else a.gap
    holes = [(h // 10, w // 12, s, s), (h // 2, w - w // 8 - s, s, s), (h - h // 9 - s, w // 3, s, s)]
    photo, mask = make_photo(h, w, holes, 11, dev)
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "resolution": res, "size": [h, w], "holes": holes, "padding": a.padding, "gap": gap,
              "reps": a.reps, "warmup": a.warmup}

    # ---- the stages around the generator, through the C ABI, on seeded y ----
    img_r, img_b = photo.clone(), photo.clone()
    items = [(img_r.data_ptr(), mask.data_ptr(), h, w, h, w)]
    cap = 8 + 1
    scratch_r = torch.empty(lib.pipeline_regions_scratch_bytes(items, gap, 8), dtype=torch.uint8, device=dev)
    labels = torch.empty((h, w), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    boxes = torch.empty((1, cap, 4), dtype=torch.int32, device=dev)

    def find():
        lib.pipeline_regions_find(items, res, a.padding, gap, 8, [labels.data_ptr()], count.data_ptr(), boxes.data_ptr(), scratch_r.data_ptr(), stream)

    find()
    k = int(count.cpu()[0])
    host_boxes = boxes.cpu()[0].tolist()
    assert k == 3, f"the photo was built for three regions, found {k}"
    rows = [(img_r.data_ptr(), mask.data_ptr(), labels.data_ptr(), h, w, r, host_boxes[r]) for r in range(1, k + 1)]
    result["boxes"] = {"single": host_boxes[0], "regions": host_boxes[1:k + 1]}
    rng = np.random.default_rng(3)
    y3 = torch.from_numpy((rng.standard_normal((3, 3, res, res)) * 0.6).astype(np.float32)).to(dev)
    x3 = torch.empty((3, 4, res, res), dtype=torch.float32, device=dev)
    x1 = torch.empty((1, 4, res, res), dtype=torch.float32, device=dev)
    items_b = [(img_b.data_ptr(), mask.data_ptr(), h, w, h, w)]
    scratch_b = torch.empty(lib.pipeline_batch_scratch_bytes(items_b), dtype=torch.uint8, device=dev)
    bbox = torch.empty((1, 4), dtype=torch.int32, device=dev)

    def pre_r():
        lib.pipeline_regions_pre(rows, res, x3.data_ptr(), stream)

    def post_r():
        lib.pipeline_regions_post(rows, res, y3.data_ptr(), gauss25=pipe._gauss, stream=stream)

    def pre_b():
        lib.pipeline_batch_pre(items_b, res, a.padding, x1.data_ptr(), bbox.data_ptr(), scratch_b.data_ptr(), stream)

    def post_b():
        lib.pipeline_batch_post(items_b, res, y3.data_ptr(), bbox.data_ptr(), scratch_b.data_ptr(), gauss25=pipe._gauss, stream=stream)

    def all_r():
        find(); pre_r(); post_r()

    def all_b():
        pre_b(); post_b()

    stages = {"regions_find": find, "regions_pre": pre_r, "regions_post": post_r, "regions_find_pre_post": all_r,
              "batch_pre": pre_b, "batch_post": post_b, "batch_pre_post": all_b}
    for _ in range(a.warmup):
        for fn in stages.values():
            fn()
    torch.cuda.synchronize()
    assert bbox.cpu()[0].tolist() == host_boxes[0], "slot 0 must be the batch pipeline's box"
    ts = {name: [] for name in stages}
    for _ in range(a.reps):
        for name, fn in stages.items():
            ts[name].append(event_ms(fn, reset=lambda: (img_r.copy_(photo), img_b.copy_(photo))))
    result["stages_ms"] = {name: stats(v) for name, v in ts.items()}

    # ---- the generator at batch 1 and at batch 3 ----
    gen = {"generator_batch1": lambda: model(x1), "generator_batch3": lambda: model(x3)}
    for _ in range(a.warmup):
        for fn in gen.values():
            fn()
    tg = {name: [] for name in gen}
    for _ in range(a.reps):
        for name, fn in gen.items():
            tg[name].append(event_ms(fn))
    result["generator_ms"] = {name: stats(v) for name, v in tg.items()}

    # ---- end to end, and the metrics over the hole ----
    e_r, e_b = [photo.clone()], [photo.clone()]
    ends = {"forward_regions": lambda: pipe.forward_regions(e_r, [mask], gap=gap), "forward_batch": lambda: pipe.forward_batch(e_b, [mask])}
    for _ in range(a.warmup):
        for fn in ends.values():
            fn()
    te = {name: [] for name in ends}
    for _ in range(a.reps):
        for name, fn in ends.items():
            te[name].append(event_ms(fn, reset=lambda: (e_r[0].copy_(photo), e_b[0].copy_(photo))))
    result["end_to_end_ms"] = {name: stats(v) for name, v in te.items()}
    e_r[0].copy_(photo)
    e_b[0].copy_(photo)
    _, used, _ = pipe.forward_regions(e_r, [mask], gap=gap, return_regions=True)
    pipe.forward_batch(e_b, [mask])
    result["rows_used"] = used[0].tolist()
    quality = {}
    for name, out in (("forward_regions", e_r[0]), ("forward_batch", e_b[0])):
        p, q = pkg.metrics.psnr_ssim(out, photo, mask, layout="chw")
        quality[name] = {"psnr_hole": float(p[0]), "ssim_hole": float(q[0])}
    result["quality_synthetic_weights"] = quality
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
