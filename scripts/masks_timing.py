"""Random hole masks on the device: mi-gan_amd/masks.py::random_masks (-> migan_masks_draw on the host, migan_masks_raster on the
device), milliseconds per mask, split into the host's draws and the device's raster.

    python scripts/masks_timing.py [--json out.json]

Workloads: 32 and 256 masks at R = 256 and 512, hole_range (0, 1) and (0.2, 0.4), seed 0.  Before anything is timed the masks are
compared with the numpy restatement of tests/masks_case.py on a few of the timed shapes.  Three figures per workload:
  total   wall time of random_masks, the device idle before and after (what a caller waits)
  draws   wall time of migan_masks_draw alone for the candidates that call drew (host code, one core)
  raster  device events around migan_masks_raster alone on the same plans, already on the device
Each is the median of `reps` runs after a warm-up, from the same generator state every time.  Seeded: no files, no network.
Needs an MI355X; there is no CPU path."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masks_timing.py needs an MI355X: there is no CPU path and no number without one")
    pkg = importlib.import_module("mi-gan_amd")
    from tests import masks_case as mc
    lib = pkg.load_library()
    hb, masks = pkg.hipbind, pkg.masks
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cases": []}
    for r in (256, 512):
        for hole_range in ((0, 1), (0.2, 0.4)):
            for n in (32, 256):
                entry = {"resolution": r, "hole_range": list(hole_range), "masks": n}
                if n == 32:                                                   # equal bytes first
                    rng = np.random.RandomState(0)
                    got = masks.random_masks(3, r, hole_range, rng=rng, device=dev).cpu().numpy()
                    ref = np.random.RandomState(0)
                    want, _, _ = mc.random_masks(3, r, hole_range, ref)
                    if not np.array_equal(got, want) or not mc.same_state(rng.get_state(), ref.get_state()):
                        raise SystemExit(f"R {r} {hole_range}: the masks differ from the restatement")
                total = []
                for i in range(a.warmup + a.reps):
                    rng = np.random.RandomState(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = masks.random_masks(n, r, hole_range, rng=rng, device=dev)
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        total.append((time.perf_counter() - t0) * 1e3)
                # the candidates that call drew: count them by drawing until the state is the one the call left
                final = rng.get_state()
                probe = hb.MasksRng.from_state(np.random.RandomState(0).get_state())
                coef = min(hole_range[0] + hole_range[1], 1.0)
                cand = 0
                while not mc.same_state(probe.to_state(), final):
                    lib.masks_draw(probe, r, coef, 1)
                    cand += 1
                    if cand > 100000:
                        raise SystemExit("the final state was not reached")
                entry["candidates"] = cand
                buf = np.empty(cand + 1 + cand * hb.MASKS_PLAN_WORDS_MAX, np.int32)
                draws = []
                for i in range(a.warmup + a.reps):
                    state = hb.MasksRng.from_state(np.random.RandomState(0).get_state())
                    t0 = time.perf_counter()
                    used = lib.masks_draw(state, r, coef, cand, buf.ctypes.data, buf.size)
                    if i >= a.warmup:
                        draws.append((time.perf_counter() - t0) * 1e3)
                d_plans = torch.from_numpy(buf[:used]).to(dev)
                d_out = torch.empty((cand, r, r), dtype=torch.uint8, device=dev)
                d_holes = torch.empty((cand, (r + hb.MASKS_BAND - 1) // hb.MASKS_BAND), dtype=torch.int32, device=dev)
                raster = []
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    lib.masks_raster(d_plans.data_ptr(), used, cand, r, d_out.data_ptr(), d_holes.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        raster.append(e0.elapsed_time(e1))
                for key, ms in (("total", total), ("draws", draws), ("raster", raster)):
                    entry[key + "_ms"] = statistics.median(ms)
                    entry[key + "_ms_min_max"] = [min(ms), max(ms)]
                    entry[key + "_ms_per_mask"] = statistics.median(ms) / n
                entry["plan_bytes"] = int(used) * 4
                result["cases"].append(entry)
                print(json.dumps(entry), flush=True)
                del d_plans, d_out, d_holes, out
                torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
