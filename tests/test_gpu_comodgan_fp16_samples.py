"""forward_samples (several completions per image from one encoder pass) with half-precision blocks, on a real MI355X."""
import numpy as np
import pytest
import torch

from tests.comodgan_fp16_case import F16, build, check_names, inputs, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("tag", ["r32_c128", "r64_c64"])
def test_forward_samples_in_half_precision_mode(pkg, dev, golden_dir, tag):
    """S = 1 is the plain forward bit for bit.  S = 2 agrees with the forward on the repeated input within E of the case: the encoder
    runs at another batch and the styles are normalised over another batch, which the demodulation cancels up to rounding."""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, tag)
    e = float(np.abs(g["y16"] - g["y32"]).max())
    m = build(pkg, cfg, seed, dev, flags)
    x, z = inputs(pkg, cfg, n, seed, dev)
    z2 = torch.from_numpy(pkg.synth.make_latent(2 * n, cfg.z_dim, seed + 70)).to(dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
        y1 = m.forward_samples(x, z[:, None], noise_mode="const")
        y2 = m.forward_samples(x, z2.reshape(n, 2, -1), noise_mode="const")
        info2 = m.launch_info()
        yr = m(x.repeat_interleave(2, 0), z=z2, noise_mode="const")
    assert torch.equal(y1[:, 0], y)
    check_names(info2, flags)
    assert any(F16 in i["kernel"] for i in info2)
    err = float((y2.reshape(2 * n, 3, cfg.resolution, cfg.resolution) - yr).abs().max())
    print(f"{tag}: forward_samples S=2 vs repeated forward {err:.6f} (E = {e:.5f})")
    assert bool(torch.isfinite(y2).all()) and err <= e
    assert float((y2[:, 0] - y2[:, 1]).abs().max()) > 1e-2       # the samples really differ
