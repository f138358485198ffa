"""comodgan.Generator.forward_samples on a real MI355X: S completions per image from one encoder pass, against its definition
(the plain forward on the input repeated S times) and against the CPU oracle on that repeated input."""
import numpy as np
import pytest
import torch

from oracle import comodgan_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _cfg(pkg, r, cb=32768, cm=512):
    cs = pkg.comodgan_schema
    return cs.Config(resolution=r, ch_base=cb, ch_max=cm, num_ws=cs.default_num_ws(r))


def _build(pkg, cfg, seed, dev):
    cm = pkg.comodgan
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=cfg.resolution, **kw), cm.Synthesis(resolution=cfg.resolution, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval(), sd


@pytest.fixture(scope="module")
def r64(pkg, dev):
    """R = 64, N = 3, S = 2: several tiles per image, the skip read crosses tile and image boundaries, batch 6 from an odd N"""
    cfg = _cfg(pkg, 64, 4096, 64)
    m, sd = _build(pkg, cfg, 41, dev)
    x = pkg.synth.make_input(3, 64, 41)
    z = pkg.synth.make_latent(6, cfg.z_dim, 41).reshape(3, 2, cfg.z_dim)
    return cfg, m, sd, x, z, torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)


def test_r64_matches_the_repeated_forward_and_the_oracle(pkg, dev, r64):
    cfg, m, sd, x, z, xt, zt = r64
    with torch.no_grad():
        y = m.forward_samples(xt, zt, noise_mode="const")
        y_rep = m(xt.repeat_interleave(2, 0), z=zt.reshape(6, -1), noise_mode="const")
    assert y.shape == (3, 2, 3, 64, 64)
    want = orc.generator(np.repeat(x, 2, axis=0), z.reshape(6, -1), sd, 64, cfg.num_ws)
    scale = float(np.abs(want).max())
    d_rep = float((y.reshape(6, 3, 64, 64) - y_rep).abs().max())
    err = float(np.abs(y.cpu().numpy().reshape(6, 3, 64, 64) - want).max())
    print(f"forward_samples vs repeated forward: {d_rep:.3e} (bit-equal: {torch.equal(y.reshape(6, 3, 64, 64), y_rep)}); "
          f"vs oracle: {err:.3e}; max|y| {scale:.3f}")
    # the bound the project states for the same image in different batches ("Co-Mod-GAN batch coupling")
    assert d_rep <= 1e-4 * max(1.0, scale)
    assert err <= TOL
    assert m._lib.backend() == "hip:gfx950"


def test_properties(pkg, dev, r64):
    cfg, m, sd, x, z, xt, zt = r64
    x0 = xt.clone()
    with torch.no_grad():
        y1 = m.forward_samples(xt, zt, noise_mode="const")
        y2 = m.forward_samples(xt, zt, noise_mode="const")
        one = m.forward_samples(xt, zt[:, :1], samples=1, noise_mode="const")
        plain = m(xt, z=zt[:, 0], noise_mode="const")
        drawn = m.forward_samples(xt, samples=3, noise_mode="const")
    assert torch.equal(xt, x0)                                     # the input is not modified
    assert torch.equal(y1, y2)                                     # run-to-run determinism
    assert one.shape == (3, 1, 3, 64, 64) and torch.equal(one[:, 0], plain)
    assert float((y1[:, 0] - y1[:, 1]).abs().amax(dim=(1, 2, 3)).min()) > 1e-2     # different z, different completions
    assert drawn.shape == (3, 3, 3, 64, 64) and bool(torch.isfinite(drawn).all())
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert float((drawn[:, a] - drawn[:, b]).abs().amax(dim=(1, 2, 3)).min()) > 1e-2


def test_r512_two_samples_vs_oracle(pkg, dev):
    """The standard configuration (512 channels up to 64^2, the 64-channel 512^2 skip read), N = 1, S = 2: the only full-size case."""
    cfg = _cfg(pkg, 512)
    m, sd = _build(pkg, cfg, 12, dev)
    x = pkg.synth.make_input(1, 512, 12)
    z = pkg.synth.make_latent(2, cfg.z_dim, 12)
    with torch.no_grad():
        y = m.forward_samples(torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev).reshape(1, 2, -1), noise_mode="const")
    assert y.shape == (1, 2, 3, 512, 512)
    assert "migan::cm_fir_samples_kernel" in {i["kernel"] for i in m.launch_info()}
    want = orc.generator(np.repeat(x, 2, axis=0), z, sd, 512, cfg.num_ws)
    err = float(np.abs(y[0].cpu().numpy() - want).max())
    print(f"512: vs oracle {err:.3e}; max|y| {float(np.abs(want).max()):.3f}")
    assert err <= TOL


def test_module_errors(pkg, dev):
    cfg = _cfg(pkg, 16, 1024, 64)
    m, _ = _build(pkg, cfg, 1, dev)
    x = torch.zeros(2, 4, 16, 16, device=dev)
    with pytest.raises(RuntimeError, match=r"\[2, S, 512\]"):
        m.forward_samples(x, torch.zeros(2, 512, device=dev))                      # a 2-D z
    with pytest.raises(ValueError, match="contradicts"):
        m.forward_samples(x, torch.zeros(2, 3, 512, device=dev), samples=2)
    with pytest.raises(ValueError, match="samples"):
        m.forward_samples(x)                                                       # z=None without samples
    with pytest.raises(ValueError, match="samples"):
        m.forward_samples(x, samples=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_samples(torch.zeros(2, 4, 16, 16), torch.zeros(2, 3, 512))       # CPU tensor
    with pytest.raises(RuntimeError):
        m.forward_samples(x, torch.zeros(3, 2, 512, device=dev))                   # z for another batch
    with pytest.raises(ValueError):
        m.forward_samples(x, samples=2, truncation_cutoff=-2)
