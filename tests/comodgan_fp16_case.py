"""Shared by the GPU tests of Co-Mod-GAN's half-precision blocks (test_gpu_comodgan_fp16*.py): the golden cases of
tests/golden/make_golden_comodgan_fp16.py, the module built with a case's flags, and the two checks every test makes."""
import os

import numpy as np
import torch

F16 = "cm_conv_f16_kernel"


def load_case(pkg, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, f"cmfp16_{tag}.npz"))
    r, cb, cmx, n, seed = (int(v) for v in g["cfg"])
    flags = tuple(None if int(v) < 0 else int(v) for v in g["flags"])
    cs = pkg.comodgan_schema
    cfg = cs.Config(resolution=r, ch_base=cb, ch_max=cmx, num_ws=cs.default_num_ws(r))
    return g, cfg, seed, n, flags


def build(pkg, cfg, seed, dev, flags):
    cm = pkg.comodgan
    kw = dict(resolution=cfg.resolution, ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(use_fp16_before_res=flags[0], **kw), cm.Synthesis(use_fp16_after_res=flags[1], **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def inputs(pkg, cfg, n, seed, dev):
    return (torch.from_numpy(pkg.synth.make_input(n, cfg.resolution, seed)).to(dev),
            torch.from_numpy(pkg.synth.make_latent(n, cfg.z_dim, seed)).to(dev))


def marked(layer, flags):
    """is `layer` a 3x3 convolution launch of a block the reference marks half precision (comodgan.py:148,384)?"""
    net, block = layer.split(".")[:2]
    if block == "b4" or ".conv" not in layer or layer.endswith((".fir", ".wprep", ".split")):
        return False
    f = flags[0] if net == "encoder" else flags[1]
    return f is not None and int(block[1:]) > f


def check_names(info, flags):
    assert any("cm_conv" in i["kernel"] for i in info)
    for i in info:
        assert (F16 in i["kernel"]) == marked(i["layer"], flags), (i["layer"], i["kernel"])


def envelope(tag, y, g):
    e = float(np.abs(g["y16"] - g["y32"]).max())
    err = float(np.abs(y - g["y32"]).max())
    print(f"{tag}: E = max|y16 - y32| = {e:.5f}, max|y - y32| = {err:.5f}, ratio {err / e:.3f}")
    assert np.isfinite(y).all()
    assert err <= 2 * e, (tag, err, e)
