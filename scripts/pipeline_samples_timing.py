"""Deployed pipeline, several completions per photo: MIGAN_Pipeline.forward_samples (boxes and network input once per image, the
Co-Mod-GAN encoder once per image, one out-of-place post kernel) against what a caller had to do before it: S copies of every photo
through forward_batch.  And the post stage alone on the same y: S device copies per image + migan_pipeline_batch_post over N * S
items against one migan_pipeline_batch_post_samples.

    python scripts/pipeline_samples_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pipeline_samples_timing.py --reps 3 --post-only

Synthetic weights, seeded images and rectangular holes: no files, no network.  Both baselines are built from calls of the parent
commit only, so timing them here stands in for a run of the parent.  Each repetition runs between torch.cuda.synchronize() calls
and the two paths alternate, so that a drift of the machine hits both.  Needs an MI355X; there is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.pipeline_batch_timing import make_batch, timed  # noqa: E402


class FixedLatents(torch.nn.Module):
    """the Co-Mod-GAN as forward_batch sees a model: y = model(x), here with row k's z fixed and the noise constant"""

    def __init__(self, generator, z_rows):
        super().__init__()
        self.generator, self.z_rows = generator, z_rows

    def forward(self, x):
        return self.generator(x, z=self.z_rows[:x.shape[0]], noise_mode="const")


def alternate(a, b, warmup, reps):
    for _ in range(warmup):
        a()
        b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a))
        tb.append(timed(b))
    return ({"median": statistics.median(ta), "min": min(ta)}, {"median": statistics.median(tb), "min": min(tb)},
            statistics.median(ta) / statistics.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--hole", type=int, nargs=2, default=(100, 400))
    ap.add_argument("--padding", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--post-only", action="store_true", help="only the post stage, on a seeded random y (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_samples_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    n, s, res = a.images, a.samples, a.resolution
    images, masks = make_batch(n, a.height, a.width, a.hole[0], a.hole[1], 7, dev)
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "resolution": res, "images": n, "samples": s, "size": [a.height, a.width],
              "hole": list(a.hole), "padding": a.padding, "reps": a.reps, "warmup": a.warmup}

    pipe = None
    if a.post_only:
        y = torch.randn((n * s, 3, res, res), generator=torch.Generator().manual_seed(3)).mul_(0.6).to(dev)
        gauss = None
    else:
        cs, cm = pkg.comodgan_schema, pkg.comodgan
        cfg = cs.Config(resolution=res, num_ws=cs.default_num_ws(res))
        gen = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=res), cm.Synthesis(resolution=res))
        sd = pkg.synth.make_comodgan_state_dict(cfg, 1)
        gen.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        pipe = pkg.pipeline.MIGAN_Pipeline(gen, res, padding=a.padding, device=dev)
        z = torch.from_numpy(pkg.synth.make_latent(n * s, cfg.z_dim, 1)).to(dev).reshape(n, s, cfg.z_dim)
        gauss = pipe._gauss

    # ---- the post stage alone, on the same y -----------------------------------------------------------------------------------------
    items = [(t.data_ptr(), m.data_ptr(), a.height, a.width, a.height, a.width) for t, m in zip(images, masks)]
    scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    x = torch.empty((n, 4, res, res), dtype=torch.float32, device=dev)
    lib.pipeline_batch_pre(items, res, a.padding, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), stream)
    if pipe is not None:
        with torch.no_grad():
            y = pipe.model.forward_samples(x, z, noise_mode="const").reshape(n * s, 3, res, res).contiguous()
    bbox_rows = bbox.repeat_interleave(s, 0).contiguous()           # row i * S + s = the box of image i
    scratch_rows = torch.empty(lib.pipeline_batch_scratch_bytes([it for it in items for _ in range(s)]), dtype=torch.uint8, device=dev)
    kept = {}

    def post_on_copies():
        copies = [t.clone() for t in images for _ in range(s)]
        rows = [(c.data_ptr(),) + items[k // s][1:] for k, c in enumerate(copies)]
        lib.pipeline_batch_post(rows, res, y.data_ptr(), bbox_rows.data_ptr(), scratch_rows.data_ptr(), gauss25=gauss, stream=stream)
        kept["copies"] = copies

    def post_samples():
        outs = [torch.empty((s, 3, a.height, a.width), dtype=torch.uint8, device=dev) for _ in images]
        lib.pipeline_batch_post_samples(items, s, res, y.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), [o.data_ptr() for o in outs],
                                        gauss25=gauss, stream=stream)
        kept["outs"] = outs

    tc, tn, ratio = alternate(post_on_copies, post_samples, a.warmup, a.reps)
    same = all(bool(torch.equal(kept["outs"][i][k], kept["copies"][i * s + k][0])) for i in range(n) for k in range(s))
    crop = [(int(b[1] - b[0]), int(b[3] - b[2])) for b in bbox.cpu().tolist()]
    result["post_stage"] = {"copies_then_batch_post_ms": tc, "batch_post_samples_ms": tn, "speedup_median": ratio, "byte_identical": same,
                            "crops": crop}

    # ---- the whole call --------------------------------------------------------------------------------------------------------------
    if pipe is not None:
        plain = pkg.pipeline.MIGAN_Pipeline(FixedLatents(pipe.model, z.reshape(n * s, -1)), res, padding=a.padding, device=dev)
        masks_rows = [m for m in masks for _ in range(s)]

        def batch_on_copies():
            kept["batch"] = plain.forward_batch([t.clone() for t in images for _ in range(s)], masks_rows)

        def samples_call():
            kept["samples"] = pipe.forward_samples(images, masks, z, noise_mode="const")

        tc, tn, ratio = alternate(batch_on_copies, samples_call, a.warmup, a.reps)
        # the generator of the two paths is the same network at the same batch, the encoder run N * S times against N times:
        # INTEGRATION section 6 bounds that difference, here it is counted in result bytes
        d = max(int((kept["samples"][i][k].to(torch.int16) - kept["batch"][i * s + k][0].to(torch.int16)).abs().max())
                for i in range(n) for k in range(s))
        result["whole_call"] = {"forward_batch_on_copies_ms": tc, "forward_samples_ms": tn, "speedup_median": ratio, "max_byte_difference": d}
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
