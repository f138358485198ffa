"""MI-GAN: S completions per image from per-row noise (Generator.forward_noise_samples) against the only way without it, Generator.forward
on the images repeated S times, on the same GPU in one process.

    python scripts/migan_noise_samples_timing.py [--n 8] [--samples 4] [--json out.json]

migan-512, fp32, freeze_weights(), synthetic weights and inputs: no files, no network.  The repeated forward is the parent's code unchanged,
so timing it here stands in for a run of the parent.  Each repetition runs between torch.cuda.synchronize() calls and the two paths
alternate, so that a drift of the machine hits both.  Beside the measured times: E, the share in the repeated forward's time of the
launches the samples call runs once per image (the encoder and synthesis.b4: hipEvent pairs around every launch, forward_timed), and the
prediction t_forward * (1 - E * (S - 1) / S) made from it; and, to see where a gap to the prediction comes from, the same per-launch times of
a forward at batch n (the once-per-image launches as the samples call runs them, where the prediction takes 1 / S of their batch n * S
time).  Needs an MI355X; there is no CPU path."""
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


def once_per_image(layer):
    return layer.startswith("encoder.") or layer.startswith("synthesis.b4.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    pkg = importlib.import_module("mi-gan_amd")
    dev = torch.device("cuda", 0)
    res, n, s = a.resolution, a.n, a.samples
    sd = pkg.synth.make_state_dict(res, seed=3)
    m = pkg.Generator(resolution=res)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).eval().freeze_weights()
    x = torch.from_numpy(pkg.synth.make_input(n, res, seed=3)).to(dev)
    xr = x.repeat_interleave(s, dim=0).contiguous()
    noise = torch.randn(n, s, m.noise_floats(), device=dev)
    with torch.no_grad():
        for _ in range(5):
            m(xr)
            m.forward_noise_samples(x, noise)
        _, ms = m.forward_timed(xr)
        info = m.launch_info()
        layers = [row[0] if isinstance(row, (tuple, list)) else row["layer"] for row in info]
        total = sum(ms)
        share = sum(t for name, t in zip(layers, ms) if once_per_image(name)) / total
        # the same launches at batch n: what the once-per-image part of the samples call really costs, where the prediction takes 1 / S of
        # its batch n * S time
        m(x)
        _, ms_n = m.forward_timed(x)
        once_rows = sum(t for name, t in zip(layers, ms) if once_per_image(name))
        once_n = sum(t for name, t in zip(layers, ms_n) if once_per_image(name))
        t_fwd, t_smp = [], []
        for _ in range(a.reps):
            t_fwd.append(timed(lambda: m(xr)))
            t_smp.append(timed(lambda: m.forward_noise_samples(x, noise)))
    fwd, smp = statistics.median(t_fwd), statistics.median(t_smp)
    out = dict(model=f"migan-{res}", n=n, samples=s, rows=n * s, forward_ms=round(fwd, 3), forward_ms_min=round(min(t_fwd), 3),
               samples_ms=round(smp, 3), samples_ms_min=round(min(t_smp), 3), once_per_image_share=round(share, 4),
               predicted_ms=round(fwd * (1.0 - share * (s - 1) / s), 3), sum_launch_ms=round(total, 3),
               once_per_image_ms_at_rows=round(once_rows, 3), once_per_image_ms_at_n=round(once_n, 3),
               per_row_ms_at_rows=round(total - once_rows, 3),
               per_launch=[dict(layer=name, ms=round(t, 4), ms_at_n=round(tn, 4)) for name, t, tn in zip(layers, ms, ms_n)],
               device=torch.cuda.get_device_name(0))
    print(json.dumps({k: v for k, v in out.items() if k != "per_launch"}))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
