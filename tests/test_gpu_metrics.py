"""PSNR / SSIM of completions against the photo on the MI355X: the cases of tests/metrics_case.py (those of tests/test_emu_metrics.py)
through migan_metrics_batch with ctypes on device buffers, then the Python front (mi-gan_amd/metrics.py) behind a small Co-Mod-GAN's
forward_samples_uint8 and behind MIGAN_Pipeline.forward_samples.  SSIM within 4 rulers of the float64 yardstick, the MSE exactly
(uint8) or within the bound of a reordered fp64 sum (float32)."""
import numpy as np
import pytest
import torch

from tests import metrics_case as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def mem():
    return mc.CudaMem(DEV)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case(lib, mem, name):
    mse, ssim = mc.run_case(lib, mem, name)
    if mc.CASES[name].get("nohole"):
        assert np.isnan(mse[1]).all() and np.isnan(ssim[1]).all()
        assert np.isfinite(mse[[0, 2]]).all() and np.isfinite(ssim[[0, 2]]).all()


@pytest.mark.parametrize("name", ["small_u8_hwc_s3_mask", "small_f32_chw_s3"])
def test_sample_alone_is_bit_equal(lib, mem, name):
    mc.run_samples_alone(lib, mem, name)


@pytest.mark.parametrize("dtype,layout", [(mc.U8, mc.HWC), (mc.F32, mc.CHW)])
def test_identity(lib, mem, dtype, layout):
    mc.run_identity(lib, mem, dtype, layout)


def test_two_launches(lib, mem):
    mc.run_two_launches(lib, mem)


def test_argument_errors(lib, mem):
    mc.run_arg_errors(lib, mem)


def test_exports_in_the_built_libraries(pkg, lib):
    import os
    assert lib.backend() == "hip:gfx950"
    for path in (pkg.library_path(), os.path.join(os.path.dirname(pkg.library_path()), "libmigan_hip_nanclamp.so")):
        loaded = pkg.hipbind.MiganLib(path)
        for name in pkg.hipbind.exports("migan_metrics_hip.h"):
            assert hasattr(loaded.lib, name), f"{path} does not export {name}"


# ---- the Python front ----------------------------------------------------------------------------------------------------------
def _comodgan(pkg):
    """the smoke() configuration"""
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    cfg = cs.Config(resolution=32, ch_base=4096, ch_max=128, num_ws=cs.default_num_ws(32))
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=32, **kw), cm.Synthesis(resolution=32, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 2)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval(), cfg


def _against_yardsticks(psnr, ssim, gts, preds, masks, what):
    """psnr, ssim [N, S] (host) against expected() on the downloaded bytes, CHW"""
    for i, (g, p) in enumerate(zip(gts, preds)):
        e = mc.expected(g, p, None if masks is None else masks[i])
        for s in range(p.shape[0]):
            assert -10.0 * np.log10(e["mse"][s]) == pytest.approx(psnr[i, s], rel=0, abs=1e-12), f"{what} photo {i} sample {s}"   # (log10 of the exact mse)
            dist = abs(ssim[i, s] - e["ssim"][s])
            print(f"{what} photo {i} sample {s}: psnr {psnr[i, s]:.4f} ssim {ssim[i, s]:.6f} ruler {e['ruler'][s]:.2e} distance {dist:.2e}")
            assert dist <= mc.RULERS * e["ruler"][s], f"{what} photo {i} sample {s}: {dist:.3e} vs ruler {e['ruler'][s]:.3e}"


def test_front_comodgan_samples_uint8(pkg):
    m, cfg = _comodgan(pkg)
    rng = np.random.default_rng(81)
    img = np.stack([mc.image("smooth", 32, 32, 1, mc.U8), mc.image("noise", 32, 32, 2, mc.U8)]).transpose(0, 2, 3, 1).copy()      # [2, 32, 32, 3]
    mask = np.full((2, 32, 32), 255, dtype=np.uint8)
    mask[0, 8:24, 10:30] = 0
    mask[1, 3:17, 5:12] = rng.integers(0, 255, (14, 7), dtype=np.uint8)
    d_img, d_mask = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    z = torch.from_numpy(pkg.synth.make_latent(6, cfg.z_dim, 81).reshape(2, 3, cfg.z_dim)).to(DEV)
    with torch.no_grad():
        out = m.forward_samples_uint8(d_img, d_mask, z, noise_mode="const")
    assert tuple(out.shape) == (2, 3, 32, 32, 3) and out.dtype == torch.uint8
    gts = list(img.transpose(0, 3, 1, 2))
    preds = list(out.cpu().numpy().transpose(0, 1, 4, 2, 3))
    for with_mask in (False, True):
        psnr, ssim = pkg.metrics.psnr_ssim(out, d_img, d_mask if with_mask else None)
        assert tuple(psnr.shape) == tuple(ssim.shape) == (2, 3) and psnr.dtype == ssim.dtype == torch.float64 and psnr.device == out.device
        _against_yardsticks(psnr.cpu().numpy(), ssim.cpu().numpy(), gts, preds, list(mask) if with_mask else None, f"comodgan mask={with_mask}")
    assert torch.equal(pkg.metrics.psnr(out, d_img), pkg.metrics.psnr_ssim(out, d_img)[0])
    assert torch.equal(pkg.metrics.ssim(out, d_img, d_mask), pkg.metrics.psnr_ssim(out, d_img, d_mask)[1])


def test_front_pipeline_list_form(pkg):
    m, cfg = _comodgan(pkg)
    pipe = pkg.pipeline.MIGAN_Pipeline(m, 32, padding=8, device=DEV)
    sizes = [(90, 120), (70, 51), (33, 97)]
    holes = [(slice(30, 61), slice(40, 75)), (slice(50, 70), slice(31, 51)), (slice(5, 20), slice(10, 30))]
    images = [mc.image("smooth" if i % 2 else "noise", h, w, 30 + i, mc.U8) for i, (h, w) in enumerate(sizes)]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for mk, hole in zip(masks, holes):
        mk[hole] = 0
    d_img = [torch.from_numpy(a)[None].to(DEV) for a in images]
    d_mask = [torch.from_numpy(mk)[None, None].to(DEV) for mk in masks]
    z = torch.from_numpy(pkg.synth.make_latent(6, cfg.z_dim, 82).reshape(3, 2, cfg.z_dim)).to(DEV)
    outs = pipe.forward_samples(d_img, d_mask, z, noise_mode="const")
    assert [tuple(o.shape) for o in outs] == [(2, 3) + s for s in sizes]
    psnr, ssim = pkg.metrics.psnr_ssim(outs, d_img, d_mask)
    assert tuple(psnr.shape) == tuple(ssim.shape) == (3, 2)
    _against_yardsticks(psnr.cpu().numpy(), ssim.cpu().numpy(), images, [o.cpu().numpy() for o in outs], masks, "pipeline")
    for a, d in zip(images, d_img):
        assert np.array_equal(d[0].cpu().numpy(), a)


def test_front_shapes_identity_and_errors(pkg):
    mt = pkg.metrics
    g = torch.from_numpy(np.stack([mc.image("smooth", 20, 24, 1, mc.F32), mc.image("noise", 20, 24, 2, mc.F32)])).to(DEV)      # [2, 3, 20, 24]
    p = (g * 0.9 + 0.05).contiguous()
    psnr, ssim = mt.psnr_ssim(p, g, shave=2)
    assert tuple(psnr.shape) == tuple(ssim.shape) == (2,)
    e = [mc.expected(a, b[None], shave=2) for a, b in zip(g.cpu().numpy(), p.cpu().numpy())]
    for i in range(2):
        assert abs(float(ssim[i]) - e[i]["ssim"][0]) <= mc.RULERS * e[i]["ruler"][0]
        assert abs(float(psnr[i]) + 10.0 * np.log10(e[i]["mse"][0])) <= 1e-9
    # an identical pair: +inf, as numpy gives in the reference; uint8 hwc by default
    gu = torch.from_numpy(mc.image("noise", 20, 24, 3, mc.U8).transpose(1, 2, 0).copy())[None].to(DEV)
    psnr, ssim = mt.psnr_ssim(gu.clone(), gu)
    assert float(psnr[0]) == float("inf") and float(ssim[0]) == 1.0
    # hwc given for float32, masks in both shapes, (-1, 1)
    gh = (g.permute(0, 2, 3, 1) * 2 - 1).contiguous()
    ph = (p.permute(0, 2, 3, 1) * 2 - 1).contiguous()
    mask = torch.full((2, 20, 24), 255, dtype=torch.uint8, device=DEV)
    mask[:, 4:15, 6:20] = 0
    a = mt.psnr_ssim(ph, gh, mask, layout="hwc", value_range=(-1.0, 1.0))
    b = mt.psnr_ssim(ph, gh, mask[:, None], layout="hwc", value_range=(-1.0, 1.0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()
    with pytest.raises(RuntimeError, match="no CPU path"):
        mt.psnr_ssim(p.cpu(), g.cpu())
    with pytest.raises(RuntimeError, match="one dtype"):
        mt.psnr_ssim(gu.expand(2, -1, -1, -1).permute(0, 3, 1, 2).contiguous(), g)
    with pytest.raises(RuntimeError, match="contiguous"):
        mt.psnr_ssim(p.transpose(2, 3), g)
    with pytest.raises(RuntimeError, match="of size"):
        mt.psnr_ssim(p, g, mask[:, :19].contiguous())
    with pytest.raises(RuntimeError, match="shave"):
        mt.psnr_ssim(p, g, shave=-1)
    with pytest.raises(RuntimeError, match="shave"):
        mt.psnr_ssim(p, g, shave=10)
    with pytest.raises(RuntimeError, match="expected pred"):
        mt.psnr_ssim(p[:, :, :19].contiguous(), g)
    with pytest.raises(RuntimeError, match="layout"):
        mt.psnr_ssim(p, g, layout="nhwc")
    with pytest.raises(ValueError):
        mt.psnr_ssim(p, g, value_range=(1.0, 1.0))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="same device"):
            mt.psnr_ssim(p.to("cuda:1"), g)
