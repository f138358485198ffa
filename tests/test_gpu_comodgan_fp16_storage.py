"""fp16 activation storage in Co-Mod-GAN's half-precision blocks on a real MI355X: Generator.set_fp16_storage() ->
comodgan_set_fp16_storage -> the typed twins of the convolution, FIR, FromRGB and ToRGB kernels (include/comodgan_fp16_storage_hip.h).

The yardstick is the reference itself (tests/golden/cmfp16_*.npz): E = max|y16 - y32| is how far the reference's own half-precision
path, which also stores fp16, moves its output; ours must stay within 2 E of the reference's fp32 output in every case and every
forced kernel form.  Every rounding this mode adds is one the reference's path makes too, so a ratio above 2 is a defect.
Measured ratios: profiles/comodgan_fp16_storage.md."""
import numpy as np
import pytest
import torch

from tests.comodgan_fp16_case import build, envelope, inputs, load_case
from tests.comodgan_fp16_storage_case import blocks, check_storage_names

pytestmark = pytest.mark.gpu
TAGS = ["r32_c128", "r64_c64", "r64_c64_syn", "r64_std"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("tag", TAGS)
def test_envelope_names_workspace_and_switching(pkg, dev, golden_dir, tag):
    """Every golden: within 2 E of the reference's fp32 output and finite; every launch of the plan carries the name the tensor rule
    gives it; the workspace shrinks by at least the marked skip tensors; storage on -> off reproduces the operand-only bits computed
    before, on one module and one handle; two runs with storage on are bit-identical; the input is not modified."""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, tag)
    m = build(pkg, cfg, seed, dev, flags)
    x, z = inputs(pkg, cfg, n, seed, dev)
    x0 = x.clone()
    with torch.no_grad():
        y_ops = m(x, z=z, noise_mode="const")
        info_ops = m.launch_info()
        handle = m._handle
        ws_ops = handle.workspace_bytes(n)
        assert m.set_fp16_storage() is m
        y = m(x, z=z, noise_mode="const")
        info = m.launch_info()
        assert handle.get_fp16_storage() is True
        ws_st = handle.workspace_bytes(n)
        y_again = m(x, z=z, noise_mode="const")
        m.set_fp16_storage(False)
        y_back = m(x, z=z, noise_mode="const")
        assert m.launch_info() == info_ops
    assert m._handle is handle and torch.equal(x, x0)
    envelope(tag + " storage", y.cpu().numpy(), g)
    check_storage_names(info, info_ops, cfg, flags)
    enc, _ = blocks(cfg, flags)
    assert ws_ops - ws_st >= sum(n * r * r * min(cfg.ch_base // r, cfg.ch_max) * 2 for r in enc)
    assert ws_st < ws_ops
    assert not torch.equal(y, y_ops)
    assert torch.equal(y_again, y) and torch.equal(y_back, y_ops)
    assert m._lib.backend() == "hip:gfx950"


def test_nothing_moves_without_marked_blocks(pkg, dev, golden_dir):
    """storage on with no block marked: the launch list, the workspace size and the bits of the default mode"""
    g, cfg, seed, n, _ = load_case(pkg, golden_dir, "r32_c128")
    m = build(pkg, cfg, seed, dev, (None, None))
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y32 = m(x, z=z, noise_mode="const")
        info32, ws32 = m.launch_info(), m._handle.workspace_bytes(n)
        m.set_fp16_storage()
        y = m(x, z=z, noise_mode="const")
    assert m._handle.get_fp16_storage() is True
    assert m.launch_info() == info32 and m._handle.workspace_bytes(n) == ws32
    assert torch.equal(y, y32)
    for name in pkg.hipbind.exports("comodgan_fp16_storage_hip.h"):
        assert hasattr(m._lib.lib, name)


@pytest.mark.parametrize("tag,env,names", [
    # 16 x 16 pixels x 256 channels per workgroup (the host picks these tiles for large launches only)
    ("r64_std", {"COMODGAN_MTI": "4"}, ["migan::cm_conv_h_kernel<256, 32, 11, true, 4, false, true>", "migan::cm_conv_h_kernel<256, 16, 18, true, 4, false, true>",
                                        "migan::cm_conv_h_kernel<256, 16, 18, true, 4, false, false>"]),
    # one launch per transposed-convolution phase: the generic single-phase tap list, on 64 and on 128 columns
    ("r64_c64", {"COMODGAN_UP4": "0"}, ["migan::cm_conv_h_kernel<64, 32, 6, false, 2, false, true>"]),
    ("r32_c128", {"COMODGAN_UP4": "0"}, ["migan::cm_conv_h_kernel<128, 32, 6, false, 2, false, true>"]),
    # the four-phase launch on 128 columns, and the tap list on 256
    ("r32_c128", {"COMODGAN_UP4_NT": "128"}, ["migan::cm_conv_h_kernel<128, 32, 6, true, 2, true, true>"]),
    ("r64_std", {"COMODGAN_MTI": "4", "COMODGAN_UP4": "0"}, ["migan::cm_conv_h_kernel<256, 32, 11, false, 4, false, true>"]),
])
def test_every_form(pkg, dev, golden_dir, monkeypatch, tag, env, names):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, tag)
    m = build(pkg, cfg, seed, dev, flags).set_fp16_storage()
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
    envelope(f"{tag} {env} storage", y.cpu().numpy(), g)
    info = m.launch_info()
    assert set(names) <= {i["kernel"] for i in info}, {i["kernel"] for i in info}


def test_skip_type_follows_the_encoder_block(pkg, dev, golden_dir):
    """flags (8, 16) on r32_c128: encoder b16 is marked, synthesis b16 is not -- its FIR-up reads an fp16 skip tensor into an fp32
    block.  The flags mark a subset of the blocks the golden's (8, 8) marks, hence a subset of its roundings: the same 2 E bound."""
    g, cfg, seed, n, _ = load_case(pkg, golden_dir, "r32_c128")
    m = build(pkg, cfg, seed, dev, (8, 16))
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        m(x, z=z, noise_mode="const")
        info_ops = m.launch_info()
        y = m.set_fp16_storage()(x, z=z, noise_mode="const")
    info = m.launch_info()
    envelope("r32_c128 flags (8, 16) storage", y.cpu().numpy(), g)
    check_storage_names(info, info_ops, cfg, (8, 16))
    k = {i["layer"]: i["kernel"] for i in info}
    assert k["synthesis.b16.conv0.fir"] == "migan::cm_fir_h_kernel<1, false, false, true>"
    assert k["synthesis.b32.conv0.fir"] == "migan::cm_fir_h_kernel<1, false, true, true>"


def test_forward_samples_and_forward_timed(pkg, dev, golden_dir):
    """r32_c128, S = 3, storage on: row i S + s equals the plain forward on the repeated input within 1e-4 |y|max (the bound of the
    samples tests); S = 1 is the plain forward bit for bit; the typed samples-FIR kernel is launched; forward_timed honours the switch"""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, "r32_c128")
    m = build(pkg, cfg, seed, dev, flags).set_fp16_storage()
    x, z = inputs(pkg, cfg, n, seed, dev)
    s = 3
    zs = torch.from_numpy(pkg.synth.make_latent(s * n, cfg.z_dim, seed + 70)).to(dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
        y1 = m.forward_samples(x, z[:, None], noise_mode="const")
        ys = m.forward_samples(x, zs.reshape(n, s, -1), noise_mode="const")
        info_s = m.launch_info()
        yr = m(x.repeat_interleave(s, 0), z=zs, noise_mode="const")
        yt, ms = m.forward_timed(x, z)
        info_t = m.launch_info()
    assert torch.equal(y1[:, 0], y) and torch.equal(yt, y)
    assert len(ms) == len(info_t) and any("cm_conv_h_kernel" in i["kernel"] for i in info_t)
    fir_up = [i["kernel"] for i in info_s if i["layer"].startswith("synthesis") and i["layer"].endswith(".fir")]
    assert fir_up and all("cm_fir_samples" in k for k in fir_up) and any("cm_fir_samples_h_kernel" in k for k in fir_up)
    err, top = float((ys.reshape(s * n, 3, cfg.resolution, cfg.resolution) - yr).abs().max()), float(yr.abs().max())
    print(f"forward_samples S=3, storage on, vs repeated forward: {err:.3e} (|y|max = {top:.3f})")
    assert bool(torch.isfinite(ys).all()) and err <= 1e-4 * top
    assert float((ys[:, 0] - ys[:, 1]).abs().max()) > 1e-2       # the samples really differ
