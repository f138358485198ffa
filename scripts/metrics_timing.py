"""PSNR / SSIM on the device: one fused call (mi-gan_amd/metrics.py::psnr_ssim -> migan_metrics_batch) against the reference's torch
formulation (lib/evaluator/eva_ssim.py:21-41 and eva_psnr.py:34-56: five depthwise 121-tap F.conv2d, float32 copies of the images,
once per sample) on the same device tensors.

    python scripts/metrics_timing.py [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/metrics_timing.py --reps 3 --fused-only

Default shapes: Co-Mod-GAN-512 at batch 16 with S = 4 -- uint8 [16, 4, 512, 512, 3] against [16, 512, 512, 3], and float32
[16, 4, 3, 512, 512] against [16, 3, 512, 512] -- each with and without a mask.  The torch formulation is what a user of the parent
commit has to run, so timing it here stands in for the parent.  Before anything is timed the two are compared on the inputs.  Times
are device events around each call, after a warm-up, the two paths alternating in one process; the spread of the repetitions is
reported.  Seeded images: no files, no network.  Needs an MI355X; there is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_formulation(pred, gt, mask, hwc, value_range, shave):
    """(psnr, ssim) [N, S] as the reference computes them, in float32 on the device; the hole-only means through a 0 / 1 weight"""
    n, s = pred.shape[:2]
    if hwc:
        pred, gt = pred.permute(0, 1, 4, 2, 3), gt.permute(0, 3, 1, 2)
    lo, hi = value_range
    if pred.dtype == torch.uint8:
        p, g = pred.float() / 255, gt.float() / 255
    else:
        p, g = (pred - lo) / (hi - lo), (gt - lo) / (hi - lo)
    h, w = g.shape[-2:]
    p = p.reshape(n * s, 3, h, w)
    g = g[:, None].expand(n, s, 3, h, w).reshape(n * s, 3, h, w)
    taps = torch.tensor([torch.exp(torch.tensor(-(x - 5) ** 2 / 4.5)) for x in range(11)], dtype=torch.float32, device=p.device)
    taps = (taps / taps.sum()).unsqueeze(1)
    window = taps.mm(taps.t())[None, None].expand(3, 1, 11, 11).contiguous()
    mu1, mu2 = F.conv2d(p, window, padding=5, groups=3), F.conv2d(g, window, padding=5, groups=3)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(p * p, window, padding=5, groups=3) - mu1_sq
    sigma2_sq = F.conv2d(g * g, window, padding=5, groups=3) - mu2_sq
    sigma12 = F.conv2d(p * g, window, padding=5, groups=3) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + 1e-4) * (2 * sigma12 + 9e-4)) / ((mu1_sq + mu2_sq + 1e-4) * (sigma1_sq + sigma2_sq + 9e-4))
    sq = (p - g) ** 2
    if shave:
        sq = sq[:, :, shave:-shave, shave:-shave]
    if mask is None:
        ssim = ssim_map.mean((1, 2, 3))
        mse = sq.mean((1, 2, 3))
    else:
        wgt = (mask != 255).float()[:, None, None].expand(n, s, 1, h, w).reshape(n * s, 1, h, w)
        ssim = (ssim_map * wgt).sum((1, 2, 3)) / (3 * wgt.sum((1, 2, 3)))
        wp = wgt[:, :, shave:h - shave, shave:w - shave] if shave else wgt
        mse = (sq * wp).sum((1, 2, 3)) / (3 * wp.sum((1, 2, 3)))
    return (-10 * torch.log10(mse)).reshape(n, s), ssim.reshape(n, s)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--shave", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="only the fused call (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda:0")
    n, s, r = a.batch, a.samples, a.size
    gen = torch.Generator().manual_seed(5)
    result = {"device": torch.cuda.get_device_name(0), "batch": n, "samples": s, "size": r, "shave": a.shave, "reps": a.reps, "warmup": a.warmup,
              "cases": []}
    base = torch.rand((n, 3, r, r), generator=gen)
    base = F.avg_pool2d(base, 5, 1, 2) * 0.7 + base * 0.3                                   # some structure, some noise
    comp = (base[:, None] + 0.1 * torch.randn((n, s, 3, r, r), generator=gen)).clamp(0, 1)
    mask = torch.full((n, r, r), 255, dtype=torch.uint8)
    mask[:, r // 4:r // 4 * 3, r // 8:r // 8 * 5] = 0
    for name, hwc in (("uint8 hwc", True), ("float32 chw", False)):
        if hwc:
            gt = (base * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
            pred = (comp * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous().to(dev)
        else:
            gt, pred = base.contiguous().to(dev), comp.contiguous().to(dev)
        for with_mask in (False, True):
            m = mask.to(dev) if with_mask else None
            kw = dict(shave=a.shave, layout="hwc" if hwc else "chw")

            def fused():
                return pkg.metrics.psnr_ssim(pred, gt, m, **kw)

            def formulation():
                return torch_formulation(pred, gt, m, hwc, (0.0, 1.0), a.shave)

            entry = {"data": name, "mask": with_mask}
            if not a.fused_only:
                (pa, sa), (pb, sb) = fused(), formulation()
                entry["max_abs_psnr_difference"] = float((pa - pb.double()).abs().max())
                entry["max_abs_ssim_difference"] = float((sa - sb.double()).abs().max())
                if not (entry["max_abs_psnr_difference"] < 1e-3 and entry["max_abs_ssim_difference"] < 1e-4):
                    raise SystemExit(f"{name} mask={with_mask}: the fused call and the torch formulation disagree: {entry}")
            tf, tt = timed(fused, a.warmup, a.reps, None if a.fused_only else formulation)
            entry["fused"] = stats(tf)
            # what the algorithm has to move: every element of gt and pred once (and the mask), against the time of the fused call
            unique = (gt.numel() * gt.element_size() + pred.numel() * pred.element_size() + (m.numel() if with_mask else 0))
            entry["unique_bytes"] = unique
            entry["fused_unique_gbytes_per_s"] = unique / (entry["fused"]["median_ms"] * 1e-3) / 1e9
            if tt:
                entry["torch"] = stats(tt)
                entry["speedup_median"] = entry["torch"]["median_ms"] / entry["fused"]["median_ms"]
            result["cases"].append(entry)
            print(json.dumps(entry), flush=True)
        del gt, pred
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
