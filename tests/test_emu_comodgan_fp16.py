"""CPU execution (fiber SIMT emulator, tests/emu) of the half-precision blocks of Co-Mod-GAN (include/comodgan_fp16_hip.h): the
single-plane form of the 3x3 convolution kernel behind the reference's use_fp16_before_res / use_fp16_after_res.  No GPU involved.

The yardstick is the reference itself (tests/golden/cmfp16_*.npz, make_golden_comodgan_fp16.py): E = max|y16 - y32| is how far
the reference's own half-precision path moves its output; ours must stay within 2 E of the reference's fp32 output (it rounds
the convolution operands only, so it should sit below E; 2 x is the margin the project grants a 16-bit mode)."""
import importlib
import os

import numpy as np
import pytest

from tests.emu_util import aligned, emu_lib

pkg = importlib.import_module("mi-gan_amd")
cs = importlib.import_module("mi-gan_amd.comodgan_schema")
hb = pkg.hipbind
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F16 = "cm_conv_f16_kernel"


def case(tag):
    g = np.load(os.path.join(GOLD, f"cmfp16_{tag}.npz"))
    r, cb, cm, n, seed = (int(v) for v in g["cfg"])
    flags = tuple(None if int(v) < 0 else int(v) for v in g["flags"])
    cfg = cs.Config(resolution=r, ch_base=cb, ch_max=cm, num_ws=cs.default_num_ws(r))
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    return g, cfg, sd, pkg.synth.make_input(n, r, seed), pkg.synth.make_latent(n, cfg.z_dim, seed), flags


def make_handle(cfg, sd):
    h = hb.CoModGANHandle(emu_lib(), cfg.resolution, cfg.num_ws, cfg.ch_base, cfg.ch_max, cfg.z_dim, cfg.w_dim, cfg.w0_dim, cfg.map_layers)
    keep = {k: aligned(v) for k, v in sd.items()}
    for name, shape, _ in h.weights():
        h.set_weight(name, keep[name].ctypes.data, shape)
    h.commit()
    return h, keep


def workspace(nbytes):
    ws = np.zeros(nbytes // 4 + 64, dtype=np.float32)
    return ws[(256 - ws.ctypes.data % 256) % 256 // 4:]


def forward(h, cfg, x, z, samples=None):
    """x [N,4,R,R]; z [N, z_dim], or [N*S, z_dim] with samples=S -> y, launch list"""
    n, s = x.shape[0], samples or 1
    nbytes = h.workspace_bytes(n) if samples is None else h.workspace_bytes_samples(n, s)
    wsv = workspace(nbytes)
    xa, za = aligned(x), aligned(z)
    y = aligned(np.zeros((n * s, 3, cfg.resolution, cfg.resolution), np.float32))
    if samples is None:
        h.forward(xa.ctypes.data, za.ctypes.data, y.ctypes.data, n, wsv.ctypes.data, nbytes)
    else:
        h.forward_samples(xa.ctypes.data, za.ctypes.data, y.ctypes.data, n, s, wsv.ctypes.data, nbytes)
    assert np.array_equal(xa, x)                       # the input is not modified
    return y.copy(), h.launches()


def marked(layer, cfg, flags):
    """is `layer` a 3x3 convolution launch of a block the reference marks half precision (comodgan.py:148,384)?"""
    net, block = layer.split(".")[:2]
    if block == "b4" or ".conv" not in layer or layer.endswith((".fir", ".wprep", ".split")):
        return False
    f = flags[0] if net == "encoder" else flags[1]
    return f is not None and int(block[1:]) > f


def check_names(info, cfg, flags):
    convs = [i for i in info if "cm_conv" in i["kernel"]]
    assert convs
    for i in info:
        assert (F16 in i["kernel"]) == marked(i["layer"], cfg, flags), (i["layer"], i["kernel"])
    assert any(F16 in i["kernel"] for i in convs) == any(marked(i["layer"], cfg, flags) for i in convs)


@pytest.fixture(scope="module")
def r32():
    """the r32_c128 case run once in half-precision mode and once in the default mode on one handle; shared, never modified"""
    g, cfg, sd, x, z, flags = case("r32_c128")
    h, keep = make_handle(cfg, sd)
    y32, info32 = forward(h, cfg, x, z)
    h.set_fp16_blocks(*flags)
    y16, info16 = forward(h, cfg, x, z)
    h.close()
    for a in (y32, y16):
        a.setflags(write=False)
    return dict(g=g, cfg=cfg, sd=sd, x=x, z=z, flags=flags, y32=y32, y16=y16, info32=info32, info16=info16)


def envelope(tag, y, g):
    e = float(np.abs(g["y16"] - g["y32"]).max())
    err = float(np.abs(y - g["y32"]).max())
    print(f"{tag}: E = max|y16 - y32| = {e:.5f}, max|y - y32| = {err:.5f}, ratio {err / e:.3f}")
    assert np.isfinite(y).all()
    assert err <= 2 * e, (tag, err, e)


def test_exports_and_c_abi():
    h = hb.CoModGANHandle(emu_lib(), 16, 6, 1024, 64)
    assert h.fp16_blocks() == (None, None)
    h.set_fp16_blocks(8, None)
    assert h.fp16_blocks() == (8, None)
    h.set_fp16_blocks(0, 4)
    assert h.fp16_blocks() == (0, 4)
    for bad in ((-2, 4), (4, -2), (-100, -1)):
        with pytest.raises(ValueError):
            h.set_fp16_blocks(*bad)
    assert h.fp16_blocks() == (0, 4)                   # a refused call changes nothing
    h.set_fp16_blocks(None, None)
    assert h.fp16_blocks() == (None, None)
    h.close()


def test_default_mode_names_no_single_plane_kernel(r32):
    assert not any(F16 in i["kernel"] for i in r32["info32"])
    check_names(r32["info32"], r32["cfg"], (None, None))


def test_r32_envelope_names_and_the_switch_does_something(r32):
    """128-column tiles: plain nine-tap, strided (16-channel chunks) and the four-phase launch on 64 columns"""
    envelope("r32_c128", r32["y16"], r32["g"])
    assert not np.array_equal(r32["y16"], r32["y32"])
    assert np.abs(r32["y32"] - r32["g"]["y32"]).max() <= 1e-3              # the default mode is the fp32 result
    check_names(r32["info16"], r32["cfg"], r32["flags"])
    kernels = {i["kernel"] for i in r32["info16"]}
    assert {"migan::cm_conv_f16_kernel<128, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<128, 16, 9, true, 2, false>",
            "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>"} <= kernels, kernels
    # the two modes report the same launches and the same figures (mfma_flops is the single-pass count in both)
    strip = lambda info: [{k: (v.replace("_f16", "") if k == "kernel" else v) for k, v in i.items()} for i in info]
    assert strip(r32["info16"]) == strip(r32["info32"])


@pytest.mark.parametrize("tag", ["r64_c64", "r64_c64_syn"])
def test_r64_envelope_64_column_tiles(tag):
    """64-column tiles, several tiles per image: plain, strided (a weight tile of 128 pieces: half the workgroup stages it) and
    four-phase; flags (16, 16) leave b16 / b8 unmarked, (None, 4) marks every synthesis block and no encoder block"""
    g, cfg, sd, x, z, flags = case(tag)
    h, _ = make_handle(cfg, sd)
    h.set_fp16_blocks(*flags)
    y, info = forward(h, cfg, x, z)
    h.close()
    envelope(tag, y, g)
    check_names(info, cfg, flags)
    kernels = {i["kernel"] for i in info}
    assert "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>" in kernels
    if flags[0] is not None:
        assert {"migan::cm_conv_f16_kernel<64, 32, 6, true, 2, false>", "migan::cm_conv_f16_kernel<64, 16, 9, true, 2, false>"} <= kernels


def test_single_phase_tap_lists(monkeypatch):
    """COMODGAN_UP4=0: one launch per transposed-convolution phase, the generic tap list, on 64 and on 128 columns"""
    monkeypatch.setenv("COMODGAN_UP4", "0")
    for tag, name in (("r64_c64", "migan::cm_conv_f16_kernel<64, 32, 6, false, 2, false>"),
                      ("r32_c128", "migan::cm_conv_f16_kernel<128, 32, 6, false, 2, false>")):
        g, cfg, sd, x, z, flags = case(tag)
        h, _ = make_handle(cfg, sd)
        h.set_fp16_blocks(*flags)
        y, info = forward(h, cfg, x, z)
        h.close()
        envelope(tag + " UP4=0", y, g)
        check_names(info, cfg, flags)
        assert name in {i["kernel"] for i in info}
        assert not any(", true>" in i["kernel"] for i in info if "cm_conv" in i["kernel"])


def test_four_phase_launch_on_128_columns(monkeypatch, r32):
    monkeypatch.setenv("COMODGAN_UP4_NT", "128")
    h, _ = make_handle(r32["cfg"], r32["sd"])
    h.set_fp16_blocks(*r32["flags"])
    y, info = forward(h, r32["cfg"], r32["x"], r32["z"])
    h.close()
    envelope("r32_c128 UP4_NT=128", y, r32["g"])
    assert "migan::cm_conv_f16_kernel<128, 32, 6, true, 2, true>" in {i["kernel"] for i in info}


def test_256_column_tiles(monkeypatch):
    """cm_conv_f16_kernel<256, ..., 4>: 16 x 16 pixels x 256 channels per workgroup, all three tap-list forms, every block marked"""
    monkeypatch.setenv("COMODGAN_MTI", "4")
    monkeypatch.setenv("COMODGAN_UP4", "0")
    g, cfg, sd, x, z, flags = case("r16_c256")
    h, _ = make_handle(cfg, sd)
    h.set_fp16_blocks(*flags)
    y, info = forward(h, cfg, x, z)
    h.close()
    envelope("r16_c256 MTI=4 UP4=0", y, g)
    check_names(info, cfg, flags)
    assert {"migan::cm_conv_f16_kernel<256, 32, 11, true, 4, false>", "migan::cm_conv_f16_kernel<256, 16, 18, true, 4, false>",
            "migan::cm_conv_f16_kernel<256, 32, 11, false, 4, false>"} <= {i["kernel"] for i in info}


def test_switching_the_flags_plans_again_and_reproduces(r32):
    """one handle: half precision -> default -> half precision, with the prepared weight planes kept (they serve both forms);
    run-to-run results are bit-identical"""
    cfg, x, z = r32["cfg"], r32["x"], r32["z"]
    h, _ = make_handle(cfg, r32["sd"])
    h.assume_static_weights(True)
    n = x.shape[0]
    nbytes = h.workspace_bytes(n)
    wsv = workspace(nbytes)
    xa, za = aligned(x), aligned(z)

    def fwd():
        assert h.workspace_bytes(n) == nbytes          # the marking does not change the workspace
        y = aligned(np.zeros((n, 3, cfg.resolution, cfg.resolution), np.float32))
        h.forward(xa.ctypes.data, za.ctypes.data, y.ctypes.data, n, wsv.ctypes.data, nbytes)
        return y.copy()

    h.set_fp16_blocks(*r32["flags"])
    a = fwd()
    assert any(F16 in i["kernel"] for i in h.launches())
    b = fwd()
    h.set_fp16_blocks(None, None)
    assert not any(F16 in i["kernel"] for i in h.launches())       # the query plans again by itself
    c = fwd()
    h.set_fp16_blocks(*r32["flags"])
    d = fwd()
    h.close()
    np.testing.assert_array_equal(a, r32["y16"])       # static weights (prepared once) give the bits of a preparing forward
    np.testing.assert_array_equal(b, a)
    np.testing.assert_array_equal(c, r32["y32"])
    np.testing.assert_array_equal(d, a)


def test_forward_samples_in_half_precision_mode(r32):
    """S = 1 is the plain forward bit for bit; S = 2 agrees with the forward on the repeated input within E (the encoder runs at
    another batch; the styles are normalised over another batch, which the demodulation cancels up to rounding)"""
    cfg, x, z, g = r32["cfg"], r32["x"], r32["z"], r32["g"]
    e = float(np.abs(g["y16"] - g["y32"]).max())
    h, _ = make_handle(cfg, r32["sd"])
    h.set_fp16_blocks(*r32["flags"])
    y1, info1 = forward(h, cfg, x, z, samples=1)
    np.testing.assert_array_equal(y1, r32["y16"])
    x1 = x[:1]
    z2 = pkg.synth.make_latent(2, cfg.z_dim, 77)
    y2, info2 = forward(h, cfg, x1, z2, samples=2)
    check_names(info2, cfg, r32["flags"])
    yr, _ = forward(h, cfg, np.repeat(x1, 2, axis=0), z2)
    h.close()
    err = float(np.abs(y2 - yr).max())
    print(f"forward_samples S=2 vs repeated forward: {err:.6f} (E = {e:.5f})")
    assert err <= e
    assert np.abs(y2[0] - y2[1]).max() > 1e-2          # the samples really differ


def test_module_constructors_take_the_reference_arguments():
    """Encoder(use_fp16_before_res=) / Synthesis(use_fp16_after_res=) are explicit, validated and kept as attributes; the state_dict
    does not depend on them; other unknown keywords are still swallowed"""
    cm = pkg.comodgan
    kw = dict(resolution=16, ch_base=1024, ch_max=64)
    e, s = cm.Encoder(use_fp16_before_res=8, mbstd_group_size=0, **kw), cm.Synthesis(use_fp16_after_res=np.int64(4), resample_filter=[1, 3, 3, 1], **kw)
    assert e.use_fp16_before_res == 8 and s.use_fp16_after_res == 4
    e0, s0 = cm.Encoder(**kw), cm.Synthesis(**kw)
    assert e0.use_fp16_before_res is None and s0.use_fp16_after_res is None
    assert list(e.state_dict()) == list(e0.state_dict()) and list(s.state_dict()) == list(s0.state_dict())
    for bad in ("8", 8.0, True, -1, [8]):
        with pytest.raises(ValueError, match="use_fp16_before_res"):
            cm.Encoder(use_fp16_before_res=bad, **kw)
        with pytest.raises(ValueError, match="use_fp16_after_res"):
            cm.Synthesis(use_fp16_after_res=bad, **kw)
