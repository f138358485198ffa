"""Co-Mod-GAN: the callable stages (G.mapping / G.encoder / G.synthesis) against the fused Generator.forward, on one GPU in one process.

    python profiles/comodgan_stages_timing.py [--batch 16] [--json out.json] [--forward-only]

comodgan-512, fp32, const noise, freeze_weights(), synthetic weights and inputs: no files, no network.  Each repetition runs between
torch.cuda.synchronize() calls (host wall clock, so the launch overhead of a call counts); the variants alternate within a repetition,
so that a drift of the machine hits all of them.  --forward-only times the fused forward alone: it runs on a checkout that has no
stages yet, which is how the parent commit's figure in profiles/comodgan_stages.md was taken.  Needs an MI355X; there is no CPU path."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("comodgan_stages_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    dev = torch.device("cuda:0")
    r, n = a.resolution, a.batch
    cfg = cs.Config(resolution=r, num_ws=cs.default_num_ws(r))
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=r), cm.Synthesis(resolution=r))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 1)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval().freeze_weights()
    x = torch.from_numpy(pkg.synth.make_input(n, r, 3)).to(dev)
    z = torch.from_numpy(pkg.synth.make_latent(n, cfg.z_dim, 3)).to(dev)
    keep = {}
    with torch.no_grad():
        variants = {"forward": lambda: keep.__setitem__("y", m(x, z=z, noise_mode="const"))}
        if not a.forward_only:
            variants["mapping"] = lambda: keep.__setitem__("ws", m.mapping(z))
            variants["encoder"] = lambda: keep.__setitem__("enc", m.encoder(x))
            variants["synthesis"] = lambda: keep.__setitem__("ys", m.synthesis(*keep["enc"], keep["ws"], noise_mode="const"))
            variants["synthesis_intermediate_outs"] = lambda: keep.__setitem__(
                "yo", m.synthesis(*keep["enc"], keep["ws"], noise_mode="const", return_intermediate_outs=True))
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn))
    result = {"device": torch.cuda.get_device_name(0), "resolution": r, "batch": n, "reps": a.reps, "warmup": a.warmup,
              "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
    if not a.forward_only:
        med = {k: v["median"] for k, v in result["ms"].items()}
        result["composition_equals_forward"] = bool(torch.equal(keep["ys"], keep["y"]) and torch.equal(keep["yo"][0], keep["y"]))
        result["stages_sum_ms"] = med["mapping"] + med["encoder"] + med["synthesis"]
        result["stages_sum_over_forward"] = result["stages_sum_ms"] / med["forward"]
        result["synthesis_over_forward"] = med["synthesis"] / med["forward"]
        result["intermediate_outs_extra_ms"] = med["synthesis_intermediate_outs"] - med["synthesis"]
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
