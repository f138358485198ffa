"""Deployed pipeline: N sequential MIGAN_Pipeline.forward calls against one forward_batch, on the same GPU in one process, and the
fused post-processing kernel of the batch path against the two-kernel pair of the single-image path on one large crop.

    python scripts/pipeline_batch_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pipeline_batch_timing.py --reps 3 --post-only

Synthetic weights, seeded images and rectangular holes: no files, no network.  The sequential path is the parent's code unchanged,
so timing it here stands in for a run of the parent.  Each repetition runs between torch.cuda.synchronize() calls and the two paths
alternate, so that a drift of the machine hits both.  Needs an MI355X; there is no CPU path."""
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


def make_batch(n, height, width, lo, hi, seed, dev):
    rng = np.random.default_rng(seed)
    images, masks = [], []
    for _ in range(n):
        images.append(torch.from_numpy(rng.integers(0, 256, (1, 3, height, width), dtype=np.uint8)).to(dev))
        m = np.full((1, 1, height, width), 255, dtype=np.uint8)
        hh, hw = (int(v) for v in rng.integers(lo, hi + 1, 2))
        y0, x0 = int(rng.integers(0, height - hh + 1)), int(rng.integers(0, width - hw + 1))
        m[0, 0, y0:y0 + hh, x0:x0 + hw] = 0
        masks.append(torch.from_numpy(m).to(dev))
    return images, masks


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def post_kernels(pkg, pipe, side, reps, dev):
    """the pair pipe_maxpool_kernel + pipe_post_kernel against pipe_post_batch_kernel on one side x side crop (an all-0 mask: the box is
    the whole image); device-event times here, kernel times from a rocprofv3 --kernel-trace --stats run of this script"""
    lib = pkg.load_library()
    rng = np.random.default_rng(5)
    res = pipe.res
    image = torch.from_numpy(rng.integers(0, 256, (3, side, side), dtype=np.uint8)).to(dev)
    mask = torch.zeros((side, side), dtype=torch.uint8, device=dev)
    mask[::7, ::5] = 255                                             # (not flat: the pooled mask has structure)
    mask[0, 0] = 0
    mask[side - 1, side - 1] = 0
    y = torch.from_numpy((rng.standard_normal((1, 3, res, res)) * 0.6).astype(np.float32)).to(dev)
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    items = [(0, mask.data_ptr(), side, side, side, side)]
    s1 = torch.empty(lib.pipeline_scratch_bytes(side, side), dtype=torch.uint8, device=dev)
    sb = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=dev)
    box = lib.pipeline_bbox(mask.data_ptr(), side, side, res, pipe.padding, s1.data_ptr(), stream)
    assert box == (0, side, 0, side), box
    a, b = image.clone(), image.clone()
    items_b = [(b.data_ptr(),) + items[0][1:]]
    bbox = torch.tensor([list(box)], dtype=torch.int32, device=dev)

    def pair():
        lib.pipeline_post(a.data_ptr(), mask.data_ptr(), side, side, box, res, y.data_ptr(), s1.data_ptr(), gauss25=pipe._gauss, stream=stream)

    def fused():
        lib.pipeline_batch_post(items_b, res, y.data_ptr(), bbox.data_ptr(), sb.data_ptr(), gauss25=pipe._gauss, stream=stream)

    pair()
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b))
    out = {"crop": [side, side], "byte_identical": same}
    for name, fn, img in (("pair_ms", pair, a), ("fused_ms", fused, b)):
        ts = []
        for _ in range(reps):
            img.copy_(image)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out[name] = {"median": statistics.median(ts), "min": min(ts)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--hole", type=int, nargs=2, default=(100, 400))
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--crop", type=int, default=2048)
    ap.add_argument("--post-only", action="store_true", help="only the post-kernel comparison (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_batch_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    sd = pkg.synth.make_state_dict(a.resolution, seed=1, regime="export")
    model = pkg.Generator(resolution=a.resolution)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    pipe = pkg.pipeline.MIGAN_Pipeline(model, a.resolution, padding=a.padding, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "resolution": a.resolution, "images": a.images, "size": [a.height, a.width],
              "hole": list(a.hole), "padding": a.padding, "reps": a.reps, "warmup": a.warmup}
    if not a.post_only:
        images, masks = make_batch(a.images, a.height, a.width, a.hole[0], a.hole[1], 7, dev)
        seq_imgs = [t.clone() for t in images]
        bat_imgs = [t.clone() for t in images]

        def reset():
            for s, b, t in zip(seq_imgs, bat_imgs, images):
                s.copy_(t)
                b.copy_(t)

        def seq():
            for t, m in zip(seq_imgs, masks):
                pipe(t, m)

        def bat():
            pipe.forward_batch(bat_imgs, masks)

        for _ in range(a.warmup):
            reset()
            seq()
            bat()
        torch.cuda.synchronize()
        # the two paths agree to the fp32 rounding between a batch-1 and a batched generator forward
        d = torch.stack([(s.to(torch.int16) - b.to(torch.int16)).abs().max() for s, b in zip(seq_imgs, bat_imgs)]).max()
        off = sum(int((s != b).sum()) for s, b in zip(seq_imgs, bat_imgs)) / sum(s.numel() for s in seq_imgs)
        ts, tb = [], []
        for _ in range(a.reps):
            reset()
            ts.append(timed(seq))
            tb.append(timed(bat))
        n = float(a.images)
        result.update({"sequential_ms_per_image": {"median": statistics.median(ts) / n, "min": min(ts) / n},
                       "batch_ms_per_image": {"median": statistics.median(tb) / n, "min": min(tb) / n},
                       "speedup_median": statistics.median(ts) / statistics.median(tb),
                       "max_byte_difference": int(d), "share_of_bytes_that_differ": off})
    result["post_kernels"] = post_kernels(pkg, pipe, a.crop, max(3, a.reps), dev)
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
