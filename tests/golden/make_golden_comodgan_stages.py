#!/usr/bin/env python3
"""Golden vector that pins the staged Co-Mod-GAN calls to the REFERENCE generator called with return_intermediate_outs=True.

Run in the build container only (imports the reference checkout, absent on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_comodgan_stages.py

Output (committed):
    tests/golden/cmstages_r16.npz    lib.model_zoo.comodgan.Generator at R = 16 (ch_base 1024, ch_max 64), batch 2, noise_mode='const',
                                     truncation_psi 0.7 with truncation_cutoff 3: ws, the image, res_to_rgb[res] and res_img[res]

Weights, inputs and z come from mi-gan_amd/synth.py (seeded), so the fixture holds outputs only.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_comodgan as mg  # noqa: E402  (puts the repository and the reference on sys.path)

cs, synth = mg.cs, mg.synth
R, CB, CM, N, SEED, PSI, CUTOFF = 16, 1024, 64, 2, 51, 0.7, 3


def main():
    cfg = cs.Config(resolution=R, ch_base=CB, ch_max=CM, num_ws=cs.default_num_ws(R))
    sd = synth.make_comodgan_state_dict(cfg, SEED)
    g = mg.build(cfg)
    g.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    x, z = synth.make_input(N, R, SEED), synth.make_latent(N, cfg.z_dim, SEED)
    with torch.no_grad():
        ws = g.mapping(torch.from_numpy(z), None, truncation_psi=PSI, truncation_cutoff=CUTOFF)
        y, outs = g(torch.from_numpy(x), z=torch.from_numpy(z), truncation_psi=PSI, truncation_cutoff=CUTOFF, noise_mode="const",
                    return_intermediate_outs=True)
    out = {"y": y.numpy().astype(np.float32), "ws": ws.numpy().astype(np.float32),
           "cfg": np.asarray([R, CB, CM, N, SEED], dtype=np.int64), "psi": np.asarray(PSI), "cutoff": np.asarray(CUTOFF)}
    for key in ("res_to_rgb", "res_img"):
        for res, t in outs[key].items():
            out[f"{key}:{res}"] = t.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, f"cmstages_r{R}.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
