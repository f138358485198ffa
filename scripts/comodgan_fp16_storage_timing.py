"""Co-Mod-GAN: what fp16 activation storage (Generator.set_fp16_storage()) buys in the half-precision blocks, on one GPU in one
process: the default mode, and every marking given with --flags once operand-only and once with fp16 storage; workspace bytes
and forward time of each, the storage-on figure against the operand-only figure of the same flags.

    python scripts/comodgan_fp16_storage_timing.py [--batch 16] [--flags 16,16 4,4] [--json out.json]

comodgan-512, const noise, freeze_weights(), synthetic weights and inputs: no files, no network.  One module; the marking and the storage
switch are changed on it between the measurements, and the modes alternate inside every repetition, so that a drift of the machine hits
all of them.  A forward is timed with a hipEvent pair; the per-launch table comes from forward_timed (an event pair around every
launch, everything on one stream).  Needs an MI355X; there is no CPU path."""
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


def parse_flags(s):
    before, after = (None if v in ("None", "none", "-1") else int(v) for v in s.split(","))
    return before, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--flags", nargs="*", default=["16,16", "4,4"], help="use_fp16_before_res,use_fp16_after_res per measured marking")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("comodgan_fp16_storage_timing.py needs an MI355X: there is no CPU path and no number without one")
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
    # a mode: (use_fp16_before_res, use_fp16_after_res, fp16 storage)
    modes = [(None, None, False)] + [parse_flags(f) + (st,) for f in a.flags for st in (False, True)]
    out, times = {}, {md: [] for md in modes}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def select(md):
        m.encoder.use_fp16_before_res, m.synthesis.use_fp16_after_res = md[:2]
        m.set_fp16_storage(md[2])

    def run(md):
        select(md)
        out[md] = m(x, z=z, noise_mode="const")

    with torch.no_grad():
        for _ in range(a.warmup):
            for md in modes:
                run(md)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for md in modes:
                select(md)
                torch.cuda.synchronize()
                start.record()
                out[md] = m(x, z=z, noise_mode="const")
                stop.record()
                stop.synchronize()
                times[md].append(start.elapsed_time(stop))
        result = {"device": torch.cuda.get_device_name(0), "resolution": r, "batch": n, "reps": a.reps, "warmup": a.warmup, "modes": []}
        base = statistics.median(times[modes[0]])
        for md in modes:
            select(md)
            _, ms = m.forward_timed(x, z, noise_mode="const")
            info = m.launch_info()
            med = statistics.median(times[md])
            ops = statistics.median(times[md[:2] + (False,)])
            result["modes"].append({
                "use_fp16_before_res": md[0], "use_fp16_after_res": md[1], "fp16_storage": md[2],
                "workspace_bytes": m._handle.workspace_bytes(n), "ratio_to_operand_only": med / ops, "forward_ms": {"median": med, "min": min(times[md])},
                "ratio_to_default": med / base, "max_abs_difference_to_default": float((out[md] - out[modes[0]]).abs().max()),
                "max_abs_output": float(out[md].abs().max()), "launch_sum_ms": sum(ms),
                "conv_ms": sum(t for t, i in zip(ms, info) if "cm_conv" in i["kernel"]),
                "streaming_ms": sum(t for t, i in zip(ms, info) if any(k in i["kernel"] for k in ("cm_fir", "cm_fromrgb", "cm_torgb"))),
                "launches": [{"layer": i["layer"], "kernel": i["kernel"], "ms": t, "mfma_flops": i["mfma_flops"]} for t, i in zip(ms, info)]})
    line = json.dumps(result)
    print(json.dumps({k: ([{kk: vv for kk, vv in md.items() if kk != "launches"} for md in v] if k == "modes" else v) for k, v in result.items()}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
