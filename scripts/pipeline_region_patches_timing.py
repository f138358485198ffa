"""Deployed pipeline, S completions per hole region as patches: what the out-of-place post kernel and the paste kernel cost, on one
large photo with three marked objects far apart (the photo of scripts/pipeline_regions_timing.py).

    python scripts/pipeline_region_patches_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python scripts/pipeline_region_patches_timing.py --reps 3 --samples 4 --skip-end-to-end

  * migan_pipeline_regions_post_patches at S = 1, 4, 8 against migan_pipeline_regions_post (in place, the parent's, unchanged) on the
    same three rows, with seeded y rows, alternating in one process.
  * migan_pipeline_regions_paste of one sample per row against a device-to-device copy of the same number of bytes.
  * forward_region_patches + paste_patches(choice=0) against forward_regions end to end, around the MI-GAN generator (S = 1).

Synthetic weights, a seeded smooth photo: no files, no network.  A timed window is `--inner` back-to-back calls between device events
and a synchronise, divided by `--inner` (one call is tens of microseconds: a window of one would measure the event pair); the paths
alternate, so that a drift of the machine hits all of them.  Such a window cannot be shorter than the host needs to enqueue its calls:
for the kernel's own time take the second command, one S per run (the trace names the kernel, not its S).  Needs an MI355X; there is
no CPU path."""
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

from scripts.pipeline_regions_timing import make_photo, stats  # noqa: E402


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(paths, warmup, reps, inner):
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            ts[name].append(window_ms(fn, inner))
    return {name: stats(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--hole", type=int, default=160, help="side of the three square holes")
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-end-to-end", action="store_true", help="the operators alone: what a kernel trace of one S should hold")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_region_patches_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    res, h, w, s = a.resolution, a.height, a.width, a.hole
    sd = pkg.synth.make_state_dict(res, seed=1, regime="export")
    model = pkg.Generator(resolution=res)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    pipe = pkg.pipeline.MIGAN_Pipeline(model, res, padding=a.padding, device=dev)
    gap = max(2, a.padding // 4)
    holes = [(h // 10, w // 12, s, s), (h // 2, w - w // 8 - s, s, s), (h - h // 9 - s, w // 3, s, s)]
    photo, mask = make_photo(h, w, holes, 11, dev)
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "resolution": res, "size": [h, w], "holes": holes, "padding": a.padding, "gap": gap,
              "reps": a.reps, "warmup": a.warmup, "inner": a.inner}

    # ---- the rows ----
    image = photo.clone()
    items = [(image.data_ptr(), mask.data_ptr(), h, w, h, w)]
    scratch = torch.empty(lib.pipeline_regions_scratch_bytes(items, gap, 8), dtype=torch.uint8, device=dev)
    labels = torch.empty((h, w), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    boxes = torch.empty((1, 9, 4), dtype=torch.int32, device=dev)
    lib.pipeline_regions_find(items, res, a.padding, gap, 8, [labels.data_ptr()], count.data_ptr(), boxes.data_ptr(), scratch.data_ptr(), stream)
    k = int(count.cpu()[0])
    host_boxes = boxes.cpu()[0].tolist()
    assert k == 3, f"the photo was built for three regions, found {k}"
    rows = [(image.data_ptr(), mask.data_ptr(), labels.data_ptr(), h, w, r, host_boxes[r]) for r in range(1, k + 1)]
    result["boxes"] = host_boxes[1:k + 1]
    crop_pixels = [(b[3] - b[2]) * (b[1] - b[0]) for b in host_boxes[1:k + 1]]
    result["label_pixels"] = [int((labels == r).sum()) for r in range(1, k + 1)]
    s_max = max(a.samples)
    rng = np.random.default_rng(3)
    y = torch.from_numpy((rng.standard_normal((3 * s_max, 3, res, res)) * 0.6).astype(np.float32)).to(dev)

    # ---- the post kernels: in place (the parent's) and out of place at each S; y rows r * S + s of the same buffer ----
    paths = {"regions_post_in_place": lambda: lib.pipeline_regions_post(rows, res, y.data_ptr(), gauss25=pipe._gauss, stream=stream)}
    outs = {}
    for S in a.samples:
        sizes = [S * 3 * n for n in crop_pixels]
        outs[S] = ([torch.empty(n, dtype=torch.uint8, device=dev) for n in sizes], sizes)
        paths[f"regions_post_patches_S{S}"] = (lambda S=S: lib.pipeline_regions_post_patches(
            rows, S, res, y.data_ptr(), [o.data_ptr() for o in outs[S][0]], outs[S][1], gauss25=pipe._gauss, stream=stream))
    result["post_ms"] = measure(paths, a.warmup, a.reps, a.inner)
    result["patch_bytes_per_sample"] = [3 * n for n in crop_pixels]

    # ---- paste of one sample per row against a device-to-device copy of the same bytes ----
    first = a.samples[0]
    target = photo.clone()
    paste_rows = [(target.data_ptr(), labels.data_ptr(), outs[first][0][r].data_ptr(), h, w, r + 1, host_boxes[r + 1]) for r in range(3)]
    total = sum(3 * n for n in crop_pixels)
    src, dst = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    result["paste_ms"] = measure({"regions_paste": lambda: lib.pipeline_regions_paste(paste_rows, stream), "d2d_copy_same_bytes": lambda: dst.copy_(src)},
                                 a.warmup, a.reps, a.inner)
    result["paste_bytes"] = {"patch_bytes_offered": total, "bytes_written": 3 * sum(result["label_pixels"])}

    if not a.skip_end_to_end:
        # ---- end to end around the MI-GAN generator (S = 1) ----
        e_r, e_p = [photo.clone()], [photo.clone()]

        def patches_and_paste():
            p, b, lab = pipe.forward_region_patches(e_p, [mask], gap=gap)
            pipe.paste_patches(e_p, p, b, lab, 0)

        result["end_to_end_ms"] = measure({"forward_regions": lambda: pipe.forward_regions(e_r, [mask], gap=gap),
                                           "forward_region_patches_and_paste": patches_and_paste}, a.warmup, a.reps, 1)
        e_r[0].copy_(photo)
        e_p[0].copy_(photo)
        pipe.forward_regions(e_r, [mask], gap=gap)
        patches_and_paste()
        result["end_to_end_same_bytes"] = bool(torch.equal(e_r[0], e_p[0]))
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
