"""Half-precision blocks of Co-Mod-GAN on a real MI355X: comodgan.Encoder(use_fp16_before_res=) / Synthesis(use_fp16_after_res=)
-> comodgan_set_fp16_blocks -> the single-plane form of the 3x3 convolution kernel (cm_conv_f16_kernel).

The yardstick is the reference itself (tests/golden/cmfp16_*.npz, make_golden_comodgan_fp16.py): E = max|y16 - y32| is how far
the reference's own half-precision path moves its output.  Ours rounds the convolution operands only (fp32 accumulation and
storage), so it should sit below E; the tests grant 2 E, the margin the project gives a 16-bit mode, against the reference's
fp32 output.  Measured ratios: profiles/comodgan_fp16.md."""
import numpy as np
import pytest
import torch

from tests.comodgan_fp16_case import F16, build, check_names, envelope, inputs, load_case

pytestmark = pytest.mark.gpu
TAGS = ["r32_c128", "r64_c64", "r64_c64_syn", "r64_std"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("tag", TAGS)
def test_envelope_names_and_switching(pkg, dev, golden_dir, tag):
    """Every golden: within 2 E of the reference's fp32 output and finite; the convolutions of marked blocks, and only those, run the
    single-plane kernel; the result differs from the same module's default-mode result; switching the marking on one module (one
    handle) plans again and reproduces the earlier bits; run-to-run results are bit-identical; the input is not modified."""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, tag)
    m = build(pkg, cfg, seed, dev, flags)
    x, z = inputs(pkg, cfg, n, seed, dev)
    x0 = x.clone()
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
        info = m.launch_info()
        handle = m._handle
        assert handle.fp16_blocks() == flags
        y_again = m(x, z=z, noise_mode="const")
        m.encoder.use_fp16_before_res, m.synthesis.use_fp16_after_res = None, None
        y32 = m(x, z=z, noise_mode="const")
        info32 = m.launch_info()
        m.encoder.use_fp16_before_res, m.synthesis.use_fp16_after_res = flags
        y_back = m(x, z=z, noise_mode="const")
    assert m._handle is handle and torch.equal(x, x0)
    envelope(tag, y.cpu().numpy(), g)
    check_names(info, flags)
    assert any(F16 in i["kernel"] for i in info)
    assert not any(F16 in i["kernel"] for i in info32)
    assert float(np.abs(y32.cpu().numpy() - g["y32"]).max()) <= 1e-3           # the default mode is the fp32 result
    assert not torch.equal(y, y32)
    assert torch.equal(y_again, y) and torch.equal(y_back, y)
    # the two modes make the same launches and report the same figures (mfma_flops is the single-pass count in both)
    strip = lambda launches: [{k: (v.replace("_f16", "") if k == "kernel" else v) for k, v in i.items()} for i in launches]
    assert strip(info) == strip(info32)
    kernels = {i["kernel"] for i in info}
    want = {"r32_c128": {"migan::cm_conv_f16_kernel<128, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<128, 16, 9, true, 2, false>",
                         "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>"},
            "r64_c64": {"migan::cm_conv_f16_kernel<64, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<64, 16, 9, true, 2, false>",
                        "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>"},
            "r64_c64_syn": {"migan::cm_conv_f16_kernel<64, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>"},
            "r64_std": {"migan::cm_conv_f16_kernel<128, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<128, 16, 9, true, 2, false>"}}[tag]
    assert want <= kernels, kernels


def test_default_mode_names_no_single_plane_kernel_and_the_exports_exist(pkg, dev, golden_dir):
    g, cfg, seed, n, _ = load_case(pkg, golden_dir, "r32_c128")
    m = build(pkg, cfg, seed, dev, (None, None))
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
    assert float(np.abs(y.cpu().numpy() - g["y32"]).max()) <= 1e-3
    assert not any(F16 in i["kernel"] for i in m.launch_info())
    assert m._handle.fp16_blocks() == (None, None)
    for name in ("comodgan_set_fp16_blocks", "comodgan_get_fp16_blocks"):
        assert name in pkg.hipbind.exports("comodgan_fp16_hip.h") and hasattr(m._lib.lib, name)
    with pytest.raises(ValueError):
        m._handle.set_fp16_blocks(-2, 4)
    assert m._lib.backend() == "hip:gfx950"


@pytest.mark.parametrize("tag,env,names", [
    # 16 x 16 pixels x 256 channels per workgroup (the host picks these tiles for large launches only)
    ("r64_std", {"COMODGAN_MTI": "4"}, ["migan::cm_conv_f16_kernel<256, 32, 11, true, 4, false>", "migan::cm_conv_f16_kernel<256, 16, 18, true, 4, false>"]),
    # one launch per transposed-convolution phase: the generic single-phase tap list, on 64 and on 128 columns
    ("r64_c64", {"COMODGAN_UP4": "0"}, ["migan::cm_conv_f16_kernel<64, 32, 6, false, 2, false>"]),
    ("r32_c128", {"COMODGAN_UP4": "0"}, ["migan::cm_conv_f16_kernel<128, 32, 6, false, 2, false>"]),
    # the four-phase launch on 128 columns, and the tap list on 256
    ("r32_c128", {"COMODGAN_UP4_NT": "128"}, ["migan::cm_conv_f16_kernel<128, 32, 6, true, 2, true>"]),
    ("r64_std", {"COMODGAN_MTI": "4", "COMODGAN_UP4": "0"}, ["migan::cm_conv_f16_kernel<256, 32, 11, false, 4, false>"]),
])
def test_every_form(pkg, dev, golden_dir, monkeypatch, tag, env, names):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, tag)
    m = build(pkg, cfg, seed, dev, flags)
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
    envelope(f"{tag} {env}", y.cpu().numpy(), g)
    info = m.launch_info()
    check_names(info, flags)
    assert set(names) <= {i["kernel"] for i in info}, {i["kernel"] for i in info}


def test_freeze_weights_gives_the_same_bits(pkg, dev, golden_dir):
    """the prepared weight planes serve both forms: frozen, a forward in either mode reuses them"""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, "r32_c128")
    m = build(pkg, cfg, seed, dev, flags)
    x, z = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y = m(x, z=z, noise_mode="const")
        m.freeze_weights()
        y1 = m(x, z=z, noise_mode="const")             # prepares once more ...
        y2 = m(x, z=z, noise_mode="const")             # ... and reuses
        m.encoder.use_fp16_before_res = None
        y3 = m(x, z=z, noise_mode="const")             # another marking, the same planes
        m.freeze_weights(False)
        y4 = m(x, z=z, noise_mode="const")
    assert torch.equal(y1, y) and torch.equal(y2, y)
    assert torch.equal(y3, y4) and not torch.equal(y3, y)
