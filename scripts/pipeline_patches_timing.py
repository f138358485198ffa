"""Deployed pipeline, the completions of every photo as box-sized patches: MIGAN_Pipeline.forward_patches (the crop of every
completion, one host synchronisation per chunk to size the result) against MIGAN_Pipeline.forward_samples (S whole copies of every
photo, no synchronisation), and the post stage alone on the same y: one migan_pipeline_batch_post_patches against one
migan_pipeline_batch_post_samples, each with the allocation of its destinations.

    python scripts/pipeline_patches_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pipeline_patches_timing.py --reps 3 --post-only

Two photo sizes, 4000 x 3000 and 1024 x 768 by default.  Synthetic weights, seeded images and rectangular holes: no files, no network.
forward_samples is the parent commit's code, so timing it here stands in for a run of the parent.  Before anything is timed the
defining property is checked on the inputs: patches[i] == forward_samples(...)[i] cropped to box i, byte for byte.  Each repetition
runs between torch.cuda.synchronize() calls and the two paths alternate, so that a drift of the machine hits both.  Needs an MI355X;
there is no CPU path."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.pipeline_batch_timing import make_batch  # noqa: E402
from scripts.pipeline_samples_timing import alternate  # noqa: E402


def size_arg(text):
    w, h = (int(v) for v in text.lower().split("x"))
    return w, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sizes", type=size_arg, nargs="+", default=[(4000, 3000), (1024, 768)], help="photo sizes as WIDTHxHEIGHT")
    ap.add_argument("--hole", type=int, nargs=2, default=(100, 400))
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--post-only", action="store_true", help="only the post stage, on a seeded random y (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_patches_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    n, s, res = a.images, a.samples, a.resolution
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "resolution": res, "images": n, "samples": s, "hole": list(a.hole),
              "padding": a.padding, "reps": a.reps, "warmup": a.warmup, "sizes": []}

    pipe, z, gauss = None, None, None
    if not a.post_only:
        cs, cm = pkg.comodgan_schema, pkg.comodgan
        cfg = cs.Config(resolution=res, num_ws=cs.default_num_ws(res))
        gen = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=res), cm.Synthesis(resolution=res))
        sd = pkg.synth.make_comodgan_state_dict(cfg, 1)
        gen.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        pipe = pkg.pipeline.MIGAN_Pipeline(gen, res, padding=a.padding, device=dev)
        z = torch.from_numpy(pkg.synth.make_latent(n * s, cfg.z_dim, 1)).to(dev).reshape(n, s, cfg.z_dim)
        gauss = pipe._gauss

    for width, height in a.sizes:
        images, masks = make_batch(n, height, width, a.hole[0], a.hole[1], 7, dev)
        entry = {"size": [width, height]}
        kept = {}

        # ---- the defining property, on these inputs, before any timing ---------------------------------------------------------------
        if pipe is not None:
            wholes, whole_boxes = pipe.forward_samples(images, masks, z, noise_mode="const", return_bbox=True)
            patches, boxes = pipe.forward_patches(images, masks, z, noise_mode="const")
            same = bool(torch.equal(boxes, whole_boxes.cpu())) and all(
                bool(torch.equal(patches[i], wholes[i][:, :, y0:y1, x0:x1])) for i, (x0, x1, y0, y1) in enumerate(boxes.tolist()))
            if not same:
                raise SystemExit(f"{width} x {height}: forward_patches differs from forward_samples cropped to the boxes")
            entry["byte_identical"] = same
            del wholes, patches

        # ---- the post stage alone, on the same y -------------------------------------------------------------------------------------
        items = [(t.data_ptr(), m.data_ptr(), height, width, height, width) for t, m in zip(images, masks)]
        scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=dev)
        bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
        x = torch.empty((n, 4, res, res), dtype=torch.float32, device=dev)
        lib.pipeline_batch_pre(items, res, a.padding, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), stream)
        if pipe is not None:
            with torch.no_grad():
                y = pipe.model.forward_samples(x, z, noise_mode="const").reshape(n * s, 3, res, res).contiguous()
        else:
            y = torch.randn((n * s, 3, res, res), generator=torch.Generator().manual_seed(3)).mul_(0.6).to(dev)
        rows = bbox.cpu().tolist()
        crops = [(x1 - x0, y1 - y0) for x0, x1, y0, y1 in rows]
        sizes = [s * 3 * cw * ch for cw, ch in crops]
        entry["crops"] = crops
        entry["crop_share"] = sum(cw * ch for cw, ch in crops) / (n * width * height)
        entry["result_bytes"] = {"forward_samples": s * n * 3 * height * width, "forward_patches": sum(sizes)}

        def post_samples():
            outs = [torch.empty((s, 3, height, width), dtype=torch.uint8, device=dev) for _ in images]
            lib.pipeline_batch_post_samples(items, s, res, y.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), [o.data_ptr() for o in outs],
                                            gauss25=gauss, stream=stream)
            kept["wholes"] = outs

        def post_patches():
            outs = [torch.empty(size, dtype=torch.uint8, device=dev) for size in sizes]
            lib.pipeline_batch_post_patches(items, s, res, y.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), [o.data_ptr() for o in outs], sizes,
                                            gauss25=gauss, stream=stream)
            kept["patches"] = outs

        tw, tp, ratio = alternate(post_samples, post_patches, a.warmup, a.reps)
        same = all(bool(torch.equal(kept["patches"][i].view(s, 3, y1 - y0, x1 - x0), kept["wholes"][i][:, :, y0:y1, x0:x1]))
                   for i, (x0, x1, y0, y1) in enumerate(rows))
        entry["post_stage"] = {"batch_post_samples_ms": tw, "batch_post_patches_ms": tp, "speedup_median": ratio, "byte_identical": same}
        kept.clear()

        # ---- the whole call ----------------------------------------------------------------------------------------------------------
        if pipe is not None:
            def samples_call():
                kept["samples"] = pipe.forward_samples(images, masks, z, noise_mode="const")

            def patches_call():
                kept["patches"] = pipe.forward_patches(images, masks, z, noise_mode="const")

            tw, tp, ratio = alternate(samples_call, patches_call, a.warmup, a.reps)
            entry["whole_call"] = {"forward_samples_ms": tw, "forward_patches_ms": tp, "speedup_median": ratio}
            kept.clear()
        result["sizes"].append(entry)
        del images, masks, y
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
