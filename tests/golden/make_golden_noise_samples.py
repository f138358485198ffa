#!/usr/bin/env python3
"""Golden for Generator.forward_noise_samples: the reference's TRAINING generator with noise_mode='random' and the draw recorded.

    lib/model_zoo/migan.py:130-138   every synthesis SeparableConv2d with use_noise adds torch.randn([N,1,H,W]) * noise_strength
    Generator.forward(x, noise_mode='random') (:546)

The generator of tests/golden/training_r64.npz (same seeded tensors: the recipe stored there) runs on x.repeat_interleave(S), n = 2 images,
S = 2 completions each, under a wrapper around torch.randn that records every draw.  Row i * S + s of the recorded draws, layer by layer in
call order, is that row's noise blob (include/migan_noise_samples_hip.h: synthesis.b8.conv1, b8.conv2, b16.conv1, ...).  Stored: x, the blobs
[n, S, F], y [n * S, 3, 64, 64], and the same generator's noise_mode='const' output on the repeated x.

Guard (asserted here and by the test): the random-noise output differs from the const-noise output by more than 10 x the bound the test
holds the kernels to (1e-4 * max(1, |y|max) and 1e-3, the bound of tests/test_gpu_round2.py for this model pair), so a forward that ignored
the blobs would fail.

Build container only (imports the reference):   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noise_samples.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MIGAN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
for name in ("cv2", "torchvision", "torchvision.transforms"):
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)

pkg = importlib.import_module("mi-gan_amd")
import lib.model_zoo.migan as train_mod                     # noqa: E402  (training-time model)

N_IMAGES, SAMPLES, DRAW_SEED = 2, 2, 1234


def bound(y_absmax: float) -> float:
    return min(1e-4 * max(1.0, y_absmax), 1e-3)


def main():
    g = np.load(os.path.join(HERE, "training_r64.npz"))
    res, seed = int(g["resolution"]), int(g["seed"])
    kw = dict(resolution=res, ch_base=32768, ch_max=512, depthwise=True, reparametrize=True, num_reparam_tensors=9)
    G = train_mod.Generator(train_mod.Encoder(ic_n=4, **kw), train_mod.Synthesis(rgb_n=3, **kw)).eval()
    new = dict(G.state_dict())
    for key, shp in zip([str(k) for k in g["keys"]], [str(s) for s in g["shapes"]]):
        shape = tuple(int(v) for v in shp.split(",")) if shp else ()
        leaf = key.rsplit(".", 1)[1]
        scale = 0.5 if leaf == "bias" else (0.3 if leaf == "noise_strength" else 1.0)
        new[key] = torch.from_numpy((pkg.synth.normal(shape or (1,), seed, "train/" + key) * scale).astype(np.float32)).reshape(shape)
    G.load_state_dict(new, strict=True)
    x = pkg.synth.make_input(N_IMAGES, res, seed=seed)
    xr = torch.from_numpy(x.copy()).repeat_interleave(SAMPLES, dim=0)
    draws = []
    real_randn = torch.randn

    def logging_randn(*args, **kwargs):
        t = real_randn(*args, **kwargs)
        draws.append(t.detach().clone())
        return t

    torch.manual_seed(DRAW_SEED)
    torch.randn = logging_randn
    try:
        with torch.no_grad():
            y = G(xr, noise_mode="random")
    finally:
        torch.randn = real_randn
    with torch.no_grad():
        y_const = G(xr, noise_mode="const")
    rows = N_IMAGES * SAMPLES
    want_shapes, r = [], 8
    while r <= res:
        want_shapes += [(rows, 1, r, r), (rows, 1, r, r)]
        r *= 2
    assert [tuple(d.shape) for d in draws] == want_shapes, [tuple(d.shape) for d in draws]
    blobs = torch.cat([d.reshape(rows, -1) for d in draws], dim=1).reshape(N_IMAGES, SAMPLES, -1).numpy().astype(np.float32)
    y, y_const = y.numpy().astype(np.float32), y_const.numpy().astype(np.float32)
    absmax = float(np.abs(y).max())
    gap = float(np.abs(y - y_const).max())
    print("noise_samples_r64: y", y.shape, "absmax", absmax, "blob floats", blobs.shape[-1], "random vs const", gap, "bound", bound(absmax))
    assert gap > 10.0 * bound(absmax), (gap, bound(absmax))
    assert float(np.abs(y[0] - y[1]).max()) > 10.0 * bound(absmax)          # two draws of one image differ as well
    np.savez_compressed(os.path.join(HERE, "noise_samples_r64.npz"), resolution=res, seed=seed, n=N_IMAGES, samples=SAMPLES, x=x, noise=blobs, y=y,
                        y_const=y_const, y_absmax=absmax)


if __name__ == "__main__":
    main()
