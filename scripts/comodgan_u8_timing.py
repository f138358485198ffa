"""Co-Mod-GAN: the fused uint8 forward (Generator.forward_samples_uint8, include/comodgan_u8_hip.h) against the three-step path it
replaces, pipeline.preprocess -> forward_samples -> pipeline.compose with the repeat of photo and mask that migan_compose_output
(no S argument) asks of the caller, on the same GPU in one process.

    python scripts/comodgan_u8_timing.py [--shapes 16x1 4x4] [--json out.json]

comodgan-512, fp32, const noise, freeze_weights(), synthetic weights and inputs: no files, no network.  Each repetition runs between
torch.cuda.synchronize() calls and the two paths alternate, so that a drift of the machine hits both; the spread printed beside
each median is the inter-quartile range of the repetitions.  Also printed: that the two paths gave the same bytes, the per-launch
times (hipEvent pairs around every launch) of the two uint8 kernels and of the fp32 kernels they replace, the times of the
pack and compose launches the fused call no longer makes, and the bytes of the tensors the caller holds either way.  Needs an
MI355X; there is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--shapes", nargs="+", default=["16x1", "4x4"], help="NxS: photos x completions per photo")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("comodgan_u8_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    cs, cm, pipe = pkg.comodgan_schema, pkg.comodgan, pkg.pipeline
    dev = torch.device("cuda:0")
    r = a.resolution
    cfg = cs.Config(resolution=r, num_ws=cs.default_num_ws(r))
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=r), cm.Synthesis(resolution=r))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 1)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval().freeze_weights()
    result = {"device": torch.cuda.get_device_name(0), "resolution": r, "reps": a.reps, "warmup": a.warmup, "shapes": []}
    for shape in a.shapes:
        n, s = (int(v) for v in shape.split("x"))
        img_np, mask_np = pkg.synth.make_uint8_input(n, r, 3)
        img, mask = torch.from_numpy(img_np).to(dev).contiguous(), torch.from_numpy(mask_np).to(dev).contiguous()
        z = torch.from_numpy(pkg.synth.make_latent(n * s, cfg.z_dim, 3).reshape(n, s, -1)).to(dev)
        kept = {}

        def three_step():
            x = pipe.preprocess(img, mask)
            y = m.forward_samples(x, z, noise_mode="const")
            imgr, maskr = (img, mask) if s == 1 else (img.repeat_interleave(s, 0), mask.repeat_interleave(s, 0))
            out = pipe.compose(y.reshape(n * s, 3, r, r), imgr, maskr)
            kept["three"] = (out, nbytes(x, y, out) + (0 if s == 1 else nbytes(imgr, maskr)))

        def fused():
            out = m.forward_samples_uint8(img, mask, z, noise_mode="const")
            kept["fused"] = (out, nbytes(out))

        with torch.no_grad():
            for _ in range(a.warmup):
                three_step()
                fused()
            t3, t1 = [], []
            for _ in range(a.reps):
                t3.append(timed(three_step))
                t1.append(timed(fused))
            same = torch.equal(kept["three"][0].reshape(-1), kept["fused"][0].reshape(-1))
            # per launch: the fp32-I/O plan and the uint8 plan differ in the first encoder launch and the last launch
            _, ms32 = m.forward_samples(pipe.preprocess(img, mask), z, noise_mode="const", _timed=True)
            info32 = m.launch_info()
            _, ms8 = m.forward_samples_uint8(img, mask, z, noise_mode="const", _timed=True)
            info8 = m.launch_info()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            y = m.forward_samples(pipe.preprocess(img, mask), z, noise_mode="const").reshape(n * s, 3, r, r)
            imgr, maskr = img.repeat_interleave(s, 0), mask.repeat_interleave(s, 0)
            extra = {}
            for name, fn in (("pack", lambda: pipe.preprocess(img, mask)), ("compose", lambda: pipe.compose(y, imgr, maskr)),
                             ("repeat", lambda: (img.repeat_interleave(s, 0), mask.repeat_interleave(s, 0)))):
                fn()
                start.record()
                fn()
                stop.record()
                torch.cuda.synchronize()
                extra[name] = start.elapsed_time(stop)
        launches = []
        for a32, b8, m32, m8 in zip(info32, info8, ms32, ms8):
            if a32["kernel"] != b8["kernel"]:
                launches.append({"layer": a32["layer"], "fp32_kernel": a32["kernel"], "fp32_ms": m32, "u8_kernel": b8["kernel"], "u8_ms": m8})
        row = {"images": n, "samples": s, "same_bytes": same,
               "three_step_ms": statistics.median(t3), "three_step_iqr_ms": iqr(t3), "fused_ms": statistics.median(t1), "fused_iqr_ms": iqr(t1),
               "three_step_all_ms": t3, "fused_all_ms": t1, "launches": launches, "extra_launch_ms": extra,
               "forward_sum_ms": {"fp32": sum(ms32), "u8": sum(ms8)},
               "caller_tensor_bytes": {"three_step": kept["three"][1], "fused": kept["fused"][1]}}
        result["shapes"].append(row)
        print(f"N = {n}, S = {s}: three-step {row['three_step_ms']:.3f} ms (iqr {row['three_step_iqr_ms']:.3f}), fused uint8 "
              f"{row['fused_ms']:.3f} ms (iqr {row['fused_iqr_ms']:.3f}), per forward of {n * s} completions; same bytes: {same}")
        for L in launches:
            print(f"  {L['layer']}: {L['fp32_kernel']} {L['fp32_ms'] * 1e3:.1f} us -> {L['u8_kernel']} {L['u8_ms'] * 1e3:.1f} us")
        print(f"  launches the fused call does not make: pack {extra['pack'] * 1e3:.1f} us, compose {extra['compose'] * 1e3:.1f} us"
              + ("" if s == 1 else f", repeat of photo and mask {extra['repeat'] * 1e3:.1f} us"))
        print(f"  caller-visible tensors beside photo, mask and z: three-step {row['caller_tensor_bytes']['three_step'] / 2**20:.1f} MiB, "
              f"fused {row['caller_tensor_bytes']['fused'] / 2**20:.1f} MiB")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
