"""Co-Mod-GAN: S completions per image from one encoder pass (Generator.forward_samples) against the only way without it,
Generator.forward on the images repeated S times, on the same GPU in one process.

    python scripts/comodgan_samples_timing.py [--shapes 4x4 8x2 2x8] [--json out.json]

comodgan-512, fp32, const noise, freeze_weights(), synthetic weights and inputs: no files, no network.  The repeated forward is the
parent's code unchanged, so timing it here stands in for a run of the parent.  Each repetition runs between
torch.cuda.synchronize() calls and the two paths alternate, so that a drift of the machine hits both.  Beside each measured ratio:
E, the share of the encoder launches in the repeated forward's time (hipEvent pairs around every launch, forward_timed), and the
prediction (E + (1 - E) S) / S made from it.  Needs an MI355X; there is no CPU path."""
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

FLOP_ENCODER_SHARE = 0.49      # 119 of 240.8 GFLOP per image, from the channel table of comodgan-512


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def encoder_launch(layer):
    """what a forward does once per image whatever S is: the encoder and the fc at the head of synthesis.b4"""
    return layer.startswith("encoder.") or layer == "synthesis.b4.fc"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--shapes", nargs="+", default=["4x4", "8x2", "2x8"], help="NxS: images x samples per image")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("comodgan_samples_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    dev = torch.device("cuda:0")
    r = a.resolution
    cfg = cs.Config(resolution=r, num_ws=cs.default_num_ws(r))
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=r), cm.Synthesis(resolution=r))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 1)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval().freeze_weights()
    result = {"device": torch.cuda.get_device_name(0), "resolution": r, "reps": a.reps, "warmup": a.warmup,
              "flop_encoder_share": FLOP_ENCODER_SHARE, "shapes": []}
    with torch.no_grad():
        for shape in a.shapes:
            n, s = (int(v) for v in shape.split("x"))
            x = torch.from_numpy(pkg.synth.make_input(n, r, 3)).to(dev)
            z = torch.from_numpy(pkg.synth.make_latent(n * s, cfg.z_dim, 3)).to(dev)
            xr, z3 = x.repeat_interleave(s, 0), z.reshape(n, s, -1)
            out = {}

            def samples():
                out["s"] = m.forward_samples(x, z3, noise_mode="const")

            def repeated():
                out["r"] = m(xr, z=z, noise_mode="const")

            for _ in range(a.warmup):
                samples()
                repeated()
            torch.cuda.synchronize()
            diff = float((out["s"].reshape(n * s, 3, r, r) - out["r"]).abs().max())
            ts, tr = [], []
            for _ in range(a.reps):
                tr.append(timed(repeated))
                ts.append(timed(samples))
            # per-launch times (everything on one stream, an event pair around every launch)
            _, ms_r = m.forward_timed(xr, z, noise_mode="const")
            info_r = m.launch_info()
            _, ms_s = m.forward_samples(x, z3, noise_mode="const", _timed=True)
            info_s = m.launch_info()
            enc_r = sum(t for t, i in zip(ms_r, info_r) if encoder_launch(i["layer"]))
            enc_s = sum(t for t, i in zip(ms_s, info_s) if encoder_launch(i["layer"]))
            e = enc_r / sum(ms_r)
            by_r = {i["layer"]: t for t, i in zip(ms_r, info_r)}
            # the per-sample launches whose time moved most against the same launch of the repeated forward (same batch N * S there)
            moved = sorted(((t - by_r[i["layer"]], i["layer"], by_r[i["layer"]], t) for t, i in zip(ms_s, info_s)
                            if not encoder_launch(i["layer"]) and i["layer"] in by_r), reverse=True)[:4]
            med_s, med_r = statistics.median(ts), statistics.median(tr)
            result["shapes"].append({
                "images": n, "samples": s, "max_abs_difference": diff,
                "repeated_forward_ms": {"median": med_r, "min": min(tr)}, "forward_samples_ms": {"median": med_s, "min": min(ts)},
                "ratio_median": med_s / med_r, "encoder_share_E": e, "predicted_ratio_from_E": (e + (1 - e) * s) / s,
                "predicted_ratio_from_flops": (FLOP_ENCODER_SHARE + (1 - FLOP_ENCODER_SHARE) * s) / s,
                "launch_sum_ms": {"repeated": sum(ms_r), "samples": sum(ms_s), "repeated_encoder": enc_r, "samples_encoder": enc_s},
                "per_sample_launches_that_moved_most_ms": [{"layer": l, "repeated": b, "samples": t} for _, l, b, t in moved]})
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
