"""comodgan.Generator.forward_uint8 / forward_samples_uint8 on a real MI355X (include/comodgan_u8_hip.h): photo and mask bytes in,
composited bytes out, against their definition -- pipeline.preprocess -> forward_samples -> pipeline.compose, byte for byte -- and
once against the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import comodgan_oracle as orc
from oracle import migan_prepost as pp
from tests.comodgan_u8_case import CASES, config, make_u8

pytestmark = pytest.mark.gpu
# the emulator's cases, and R = 64, N = 3, S = 2: several workgroups per image in both kernels, batch 6 from an odd N
GPU_CASES = dict(CASES, r64=(config(64, 4096, 64), 3, 2, {}, None))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _build(pkg, cfg, seed, dev, fp16=None):
    cm = pkg.comodgan
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    before, after, storage = fp16 or (None, None, False)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=cfg.resolution, use_fp16_before_res=before, **kw),
                     cm.Synthesis(resolution=cfg.resolution, use_fp16_after_res=after, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    m.set_fp16_storage(storage)
    return m, sd


def _three_step(pkg, m, img, mask, z, **opts):
    """[N,S,R,R,3]: the path a caller had to write, with the repeat migan_compose_output needs (it has no S argument)"""
    n, s = z.shape[0], z.shape[1]
    y = m.forward_samples(pkg.pipeline.preprocess(img, mask), z, **opts)
    out = pkg.pipeline.compose(y.reshape(n * s, *y.shape[2:]), img.repeat_interleave(s, 0), mask.repeat_interleave(s, 0))
    return out.reshape(n, s, *out.shape[1:])


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_bytes_of_the_three_step_path(pkg, dev, name):
    cfg, n, s, opts, fp16 = GPU_CASES[name]
    seed = 70 + list(GPU_CASES).index(name)
    r = cfg.resolution
    m, sd = _build(pkg, cfg, seed, dev, fp16)
    img_np, mask_np = make_u8(n, r, seed)
    z_np = pkg.synth.make_latent(n * s, cfg.z_dim, seed).reshape(n, s, cfg.z_dim)
    img, mask, z = torch.from_numpy(img_np).to(dev), torch.from_numpy(mask_np).to(dev), torch.from_numpy(z_np).to(dev)
    img0, mask0 = img.clone(), mask.clone()
    with torch.no_grad():
        want = _three_step(pkg, m, img, mask, z, noise_mode="const", **opts)
        out = m.forward_samples_uint8(img, mask, z, noise_mode="const", **opts)
        kernels = {i["kernel"] for i in m.launch_info()}
        again = m.forward_samples_uint8(img, mask, z, noise_mode="const", **opts)
        first = m.forward_uint8(img, mask, z[:, 0], noise_mode="const", **opts)
        one = m.forward_samples_uint8(img, mask, z[:, :1], noise_mode="const", **opts)
    assert out.shape == (n, s, r, r, 3) and out.dtype == torch.uint8
    diff = (out != want)
    print(f"{name}: {int(diff.sum())} of {diff.numel()} bytes differ from the three-step path")
    assert torch.equal(out, want)
    assert torch.equal(out, again)                                   # run to run
    assert first.shape == (n, r, r, 3) and torch.equal(first, one[:, 0])
    assert torch.equal(img, img0) and torch.equal(mask, mask0)       # the inputs are only read
    known = (mask == 255)[:, None].expand(n, s, r, r)
    assert torch.equal(out[known], img[:, None].expand(n, s, r, r, 3)[known])
    half = str(fp16 is not None).lower()
    lpp = {64: 4, 128: 8}.get(cfg.channels(r), 16)
    assert {f"migan::cm_fromrgb_u8_kernel<{half}>", f"migan::cm_torgb_u8_kernel<{lpp}, {half}>"} <= kernels
    assert m._lib.backend() == "hip:gfx950"
    if name != "lpp4":
        return
    # once, against the CPU oracle: TOL = 1e-3 on y is 1e-3 * 127.5 < 1 byte step before truncation, so a byte moves by at most one
    xr = np.repeat(pp.preprocess(img_np, mask_np), s, axis=0)
    ref = pp.compose(orc.generator(xr, z_np.reshape(n * s, -1), sd, r, cfg.num_ws), np.repeat(img_np, s, axis=0), np.repeat(mask_np, s, axis=0))
    got = out.cpu().numpy().reshape(n * s, r, r, 3)
    step = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    print("bytes off the oracle by one step:", int((step == 1).sum()), "of", step.size, "worst", int(step.max()))
    assert step.max() <= 1
    hole = mask_np != 255
    assert (got.reshape(n, s, r, r, 3)[0, 0][hole[0]] != got.reshape(n, s, r, r, 3)[0, 1][hole[0]]).any()      # samples differ


def test_random_noise(pkg, dev):
    cfg, n, s, _, _ = GPU_CASES["lpp4"]
    m, _ = _build(pkg, cfg, 80, dev)
    img_np, mask_np = make_u8(n, 16, 80)
    img, mask = torch.from_numpy(img_np).to(dev), torch.from_numpy(mask_np).to(dev)
    z = torch.from_numpy(pkg.synth.make_latent(n * s, cfg.z_dim, 80).reshape(n, s, -1)).to(dev)
    with torch.no_grad():
        a = m.forward_samples_uint8(img, mask, z)                    # noise_mode "random" is the default, as in forward
        b = m.forward_samples_uint8(img, mask, z)
        drawn = m.forward_samples_uint8(img, mask, samples=2)
        plain = m.forward_uint8(img, mask)
    assert a.shape == (n, s, 16, 16, 3) and a.dtype == torch.uint8 and drawn.shape == (n, 2, 16, 16, 3) and plain.shape == (n, 16, 16, 3)
    known = (mask == 255)
    for out in (a, b, drawn):
        k = known[:, None].expand(n, out.shape[1], 16, 16)
        assert torch.equal(out[k], img[:, None].expand(n, out.shape[1], 16, 16, 3)[k])
    assert torch.equal(plain[known], img[known])
    assert not torch.equal(a, b)                                     # another draw of the noise


def test_module_errors(pkg, dev):
    cfg = config(16, 1024, 64)
    m, _ = _build(pkg, cfg, 1, dev)
    img = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    mask = torch.full((2, 16, 16), 255, dtype=torch.uint8, device=dev)
    z = torch.zeros(2, 3, 512, device=dev)
    for call in (m.forward_uint8, lambda *a, **k: m.forward_samples_uint8(*a, samples=2, **k)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(img.cpu(), mask.cpu())
        with pytest.raises(RuntimeError, match="must be uint8"):
            call(img.float(), mask)
        with pytest.raises(RuntimeError, match="must be uint8"):
            call(img, mask.float())
        with pytest.raises(RuntimeError, match=r"expected image \[N,16,16,3\]"):
            call(img.permute(0, 3, 1, 2), mask)
        with pytest.raises(RuntimeError, match=r"expected image \[N,16,16,3\]"):
            call(img, mask[:1])
        with pytest.raises(RuntimeError, match="empty batch"):
            call(img[:0], mask[:0])
        with pytest.raises(ValueError, match="truncation_cutoff"):
            call(img, mask, truncation_cutoff=-2)
    with pytest.raises(RuntimeError, match=r"\[2, 512\]"):
        m.forward_uint8(img, mask, z)                                              # a 3-D z
    with pytest.raises(RuntimeError, match=r"\[2, S, 512\]"):
        m.forward_samples_uint8(img, mask, z[:, 0])                                # a 2-D z
    with pytest.raises(ValueError, match="contradicts"):
        m.forward_samples_uint8(img, mask, z, samples=2)
    with pytest.raises(ValueError, match="samples"):
        m.forward_samples_uint8(img, mask)                                         # z=None without samples
    with pytest.raises(ValueError, match="samples"):
        m.forward_samples_uint8(img, mask, samples=0)
    with pytest.raises(RuntimeError):
        m.forward_samples_uint8(img, mask, torch.zeros(3, 2, 512, device=dev))     # z for another batch
