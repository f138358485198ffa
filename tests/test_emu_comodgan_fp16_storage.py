"""CPU execution (fiber SIMT emulator, tests/emu) of fp16 activation storage in Co-Mod-GAN's half-precision blocks
(include/comodgan_fp16_storage_hip.h): the typed twins of the convolution, FIR, FromRGB and ToRGB kernels.  No GPU involved.

The yardstick is the reference itself (tests/golden/cmfp16_*.npz): E = max|y16 - y32| is how far the reference's own half-precision
path, which also stores fp16, moves its output; ours must stay within 2 E of the reference's fp32 output in every case and every
forced kernel form (the bound of tests/comodgan_fp16_case.py::envelope; operand-only mode sits at 0.52-0.57 E).  Every rounding
this mode adds is one the reference's path makes too, so a ratio above 2 is a defect.  Measured ratios: profiles/comodgan_fp16_storage.md."""
import importlib

import numpy as np
import pytest

from tests.comodgan_fp16_storage_case import blocks, check_storage_names
from tests.emu_util import aligned, emu_lib
from tests.test_emu_comodgan_fp16 import case, envelope, forward, make_handle, workspace

pkg = importlib.import_module("mi-gan_amd")
hb = pkg.hipbind


def run_case(tag, storage=True):
    g, cfg, sd, x, z, flags = case(tag)
    h, _ = make_handle(cfg, sd)
    h.set_fp16_blocks(*flags)
    _ = h.workspace_bytes(x.shape[0])
    info_ops = h.launches()
    h.set_fp16_storage(storage)
    y, info = forward(h, cfg, x, z)
    h.close()
    return g, cfg, flags, y, info, info_ops


@pytest.fixture(scope="module")
def r32():
    """r32_c128 (batch 2, flags 8/8) on one handle: default mode, operand-only, storage on; shared, never modified"""
    g, cfg, sd, x, z, flags = case("r32_c128")
    h, keep = make_handle(cfg, sd)
    n = x.shape[0]
    y32, info32 = forward(h, cfg, x, z)
    ws32 = h.workspace_bytes(n)
    h.set_fp16_blocks(*flags)
    yop, info_ops = forward(h, cfg, x, z)
    ws_ops = h.workspace_bytes(n)
    h.set_fp16_storage(True)
    assert h.get_fp16_storage() is True
    yst, info_st = forward(h, cfg, x, z)
    ws_st = h.workspace_bytes(n)
    h.close()
    for a in (y32, yop, yst):
        a.setflags(write=False)
    return dict(g=g, cfg=cfg, sd=sd, x=x, z=z, flags=flags, y32=y32, yop=yop, yst=yst, info32=info32, info_ops=info_ops, info_st=info_st,
                ws32=ws32, ws_ops=ws_ops, ws_st=ws_st)


def test_exports_and_c_abi():
    h = hb.CoModGANHandle(emu_lib(), 16, 6, 1024, 64)
    assert h.get_fp16_storage() is False               # off by default
    h.set_fp16_storage()
    assert h.get_fp16_storage() is True
    h.set_fp16_storage(False)
    assert h.get_fp16_storage() is False
    with pytest.raises(pkg.hipbind.MiganError):        # the dtype query is a debug query
        h.debug_tensor_dtype(1, "mapping")
    h.close()


def test_r32_envelope_names_and_workspace(r32):
    """128-column tiles, four-phase on 64: accuracy, every launch name, and the workspace shrinks by at least the marked skip tensors"""
    envelope("r32_c128 storage", r32["yst"], r32["g"])
    assert not np.array_equal(r32["yst"], r32["yop"])
    seen = check_storage_names(r32["info_st"], r32["info_ops"], r32["cfg"], r32["flags"])
    assert seen == {"cm_conv_h_kernel", "cm_fir_h_kernel", "cm_fromrgb_h_kernel", "cm_torgb_h_kernel"}, seen
    kernels = {i["kernel"] for i in r32["info_st"]}
    assert {"migan::cm_conv_h_kernel<128, 32, 6, true, 2, false, true>", "migan::cm_conv_h_kernel<128, 16, 9, true, 2, false, true>",
            "migan::cm_conv_h_kernel<128, 16, 9, true, 2, false, false>", "migan::cm_conv_h_kernel<64, 32, 6, true, 2, true, true>",
            "migan::cm_conv_f16_kernel<64, 32, 6, true, 2, true>"} <= kernels, kernels
    cfg, n = r32["cfg"], r32["x"].shape[0]
    enc, _ = blocks(cfg, r32["flags"])
    ch = lambda r: min(cfg.ch_base // r, cfg.ch_max)
    assert r32["ws_ops"] == r32["ws32"]
    assert r32["ws32"] - r32["ws_st"] >= sum(n * r * r * ch(r) * 2 for r in enc) > 0
    # same launches, same arithmetic; fewer bytes wherever a typed kernel runs
    for a, b in zip(r32["info_st"], r32["info_ops"]):
        assert (a["flops"], a["mfma_flops"]) == (b["flops"], b["mfma_flops"])
        assert a["bytes"] < b["bytes"] if a["kernel"] != b["kernel"] else a["bytes"] == b["bytes"], (a, b)


@pytest.mark.parametrize("tag", ["r64_c64", "r64_c64_syn"])
def test_r64_envelope_64_column_tiles(tag):
    """64-column tiles, several tiles per image; _syn marks no encoder block: every skip tensor is fp32 against fp16 outputs"""
    g, cfg, flags, y, info, info_ops = run_case(tag)
    envelope(tag + " storage", y, g)
    check_storage_names(info, info_ops, cfg, flags)
    kernels = {i["kernel"] for i in info}
    assert "migan::cm_conv_h_kernel<64, 32, 6, true, 2, true, true>" in kernels
    if flags[0] is None:
        assert not any("fromrgb_h" in k or "cm_fir_h_kernel<0" in k for k in kernels)
        assert {"migan::cm_fir_h_kernel<1, false, true, false>", "migan::cm_fir_h_kernel<1, true, true, false>"} <= kernels, kernels
    else:
        assert {"migan::cm_conv_h_kernel<64, 32, 6, true, 2, false, true>", "migan::cm_conv_h_kernel<64, 16, 9, true, 2, false, false>",
                "migan::cm_fir_h_kernel<1, false, true, true>", "migan::cm_fir_h_kernel<1, true, true, true>"} <= kernels, kernels


def test_single_phase_tap_lists(monkeypatch):
    """COMODGAN_UP4=0: one launch per transposed-convolution phase, the generic tap list, on 64 and on 128 columns"""
    monkeypatch.setenv("COMODGAN_UP4", "0")
    for tag, name in (("r64_c64", "migan::cm_conv_h_kernel<64, 32, 6, false, 2, false, true>"),
                      ("r32_c128", "migan::cm_conv_h_kernel<128, 32, 6, false, 2, false, true>")):
        g, cfg, flags, y, info, info_ops = run_case(tag)
        envelope(tag + " storage UP4=0", y, g)
        check_storage_names(info, info_ops, cfg, flags)
        assert name in {i["kernel"] for i in info}


def test_four_phase_launch_on_128_columns(monkeypatch):
    monkeypatch.setenv("COMODGAN_UP4_NT", "128")
    g, cfg, flags, y, info, info_ops = run_case("r32_c128")
    envelope("r32_c128 storage UP4_NT=128", y, g)
    check_storage_names(info, info_ops, cfg, flags)
    assert "migan::cm_conv_h_kernel<128, 32, 6, true, 2, true, true>" in {i["kernel"] for i in info}


def test_256_column_tiles(monkeypatch):
    """16 x 16 pixels x 256 channels per workgroup, all three tap-list forms, every block marked"""
    monkeypatch.setenv("COMODGAN_MTI", "4")
    monkeypatch.setenv("COMODGAN_UP4", "0")
    g, cfg, flags, y, info, info_ops = run_case("r16_c256")
    envelope("r16_c256 storage MTI=4 UP4=0", y, g)
    check_storage_names(info, info_ops, cfg, flags)
    assert {"migan::cm_conv_h_kernel<256, 32, 11, true, 4, false, true>", "migan::cm_conv_h_kernel<256, 16, 18, true, 4, false, false>",
            "migan::cm_conv_h_kernel<256, 32, 11, false, 4, false, true>"} <= {i["kernel"] for i in info}


def test_skip_type_follows_the_encoder_block(r32):
    """flags (8, 16): encoder b16 is marked, synthesis b16 is not -- its FIR-up reads an fp16 skip tensor into an fp32 block (the one
    launch of an unmarked block that must change, since a marked block owns one of its operands).  The flags mark a subset of the
    blocks the golden's (8, 8) marks, so the result makes a subset of its roundings: the same 2 E bound holds."""
    cfg, x, z = r32["cfg"], r32["x"], r32["z"]
    h, _ = make_handle(cfg, r32["sd"])
    h.set_fp16_blocks(8, 16)
    _ = h.workspace_bytes(x.shape[0])
    info_ops = h.launches()
    h.set_fp16_storage(True)
    y, info = forward(h, cfg, x, z)
    h.close()
    envelope("r32_c128 flags (8, 16) storage", y, r32["g"])
    check_storage_names(info, info_ops, cfg, (8, 16))
    k = {i["layer"]: i["kernel"] for i in info}
    assert k["synthesis.b16.conv0.fir"] == "migan::cm_fir_h_kernel<1, false, false, true>"
    assert k["synthesis.b32.conv0.fir"] == "migan::cm_fir_h_kernel<1, false, true, true>"
    assert "cm_torgb_kernel" in k["synthesis.b16.torgb"] and "cm_torgb_h_kernel" in k["synthesis.b32.torgb"]


def test_debug_tensor_dtypes(r32):
    """a debug plan reports fp16 for exactly the tensors of the rule in include/comodgan_fp16_storage_hip.h, and the reader returns
    float32 arrays that agree with the operand-only mode's tensors to fp16 precision"""
    cfg, x, z, flags = r32["cfg"], r32["x"], r32["z"], r32["flags"]
    n = x.shape[0]
    enc, syn = blocks(cfg, flags)
    first = min(syn)
    h, _ = make_handle(cfg, r32["sd"])
    h.set_fp16_blocks(*flags)
    h.set_debug(True)
    F32, H16 = hb.COMODGAN_DTYPE_F32, hb.COMODGAN_DTYPE_F16
    want = {"mapping": F32, "encoder.b4.conv": F32, "encoder.b4.fc": F32, "synthesis.b4.fc": F32, "synthesis.b4.conv": F32,
            "synthesis.b4.img": F32, f"encoder.b{cfg.resolution}.fromrgb": H16 if cfg.resolution in enc else F32}
    for r in (8, 16, 32):
        e, s = r in enc, r in syn
        want[f"encoder.b{r}.conv0"] = H16 if e else F32
        want[f"encoder.b{r}.conv1.fir"] = H16 if e else F32
        want[f"encoder.b{r}.conv1"] = H16 if e and (r // 2) in enc else F32
        want[f"synthesis.b{r}.conv0.raw"] = H16 if s and r != first else F32
        want[f"synthesis.b{r}.conv0"] = H16 if s else F32
        want[f"synthesis.b{r}.conv1"] = H16 if s else F32
        if r != cfg.resolution:
            want[f"synthesis.b{r}.img"] = F32
    assert sorted(set(want.values())) == [F32, H16]
    for name in want:
        assert h.debug_tensor_dtype(n, name) == F32, name          # storage off: everything is fp32

    def run():
        nbytes = h.workspace_bytes(n)
        wsv = workspace(nbytes)
        xa, za = aligned(x), aligned(z)
        y = aligned(np.zeros((n, 3, cfg.resolution, cfg.resolution), np.float32))
        h.forward(xa.ctypes.data, za.ctypes.data, y.ctypes.data, n, wsv.ctypes.data, nbytes)
        raw = wsv.view(np.uint8)[:nbytes]
        return y.copy(), {name: h.read_debug_tensor(raw, n, name) for name in want}

    y_ops, t_ops = run()
    h.set_fp16_storage(True)
    for name, dt in want.items():
        assert h.debug_tensor_dtype(n, name) == dt, name
    with pytest.raises(ValueError):
        h.debug_tensor_dtype(n, "no.such.layer")
    y_st, t_st = run()
    h.close()
    np.testing.assert_array_equal(y_ops, r32["yop"])               # a debug plan computes the same bits
    np.testing.assert_array_equal(y_st, r32["yst"])
    for name in ("encoder.b32.fromrgb", "encoder.b32.conv0", "encoder.b32.conv1", "synthesis.b16.conv0", "synthesis.b32.conv1"):
        a, b = t_st[name], t_ops[name]
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all()
        assert np.array_equal(a, a.astype(np.float16).astype(np.float32))          # what was stored is fp16
    # FromRGB is the first rounding: exactly the operand-only tensor rounded to nearest even
    np.testing.assert_array_equal(t_st["encoder.b32.fromrgb"], t_ops["encoder.b32.fromrgb"].astype(np.float16).astype(np.float32))


def test_nothing_moves_without_marked_blocks_and_the_switch_reproduces(r32):
    """storage on with no block marked is the default mode (launches, workspace, bits); on -> off gives the operand-only bits again,
    with the prepared weight planes kept; two runs with storage on are bit-identical"""
    cfg, x, z = r32["cfg"], r32["x"], r32["z"]
    n = x.shape[0]
    h, _ = make_handle(cfg, r32["sd"])
    h.assume_static_weights(True)
    nbytes = h.workspace_bytes(n)
    wsv = workspace(nbytes)                             # one workspace, sized for the default mode, serves every mode
    xa, za = aligned(x), aligned(z)

    def fwd():
        assert h.workspace_bytes(n) <= nbytes
        y = aligned(np.zeros((n, 3, cfg.resolution, cfg.resolution), np.float32))
        h.forward(xa.ctypes.data, za.ctypes.data, y.ctypes.data, n, wsv.ctypes.data, nbytes)
        return y.copy()

    h.set_fp16_storage(True)
    assert h.workspace_bytes(n) == r32["ws32"] and h.launches() == r32["info32"]
    np.testing.assert_array_equal(fwd(), r32["y32"])
    h.set_fp16_blocks(*r32["flags"])
    assert h.workspace_bytes(n) == r32["ws_st"] and h.launches() == r32["info_st"]
    a = fwd()
    b = fwd()
    h.set_fp16_storage(False)
    assert h.workspace_bytes(n) == r32["ws_ops"] and h.launches() == r32["info_ops"]      # the query plans again by itself
    c = fwd()
    h.set_fp16_storage(True)
    d = fwd()
    h.close()
    np.testing.assert_array_equal(a, r32["yst"])
    np.testing.assert_array_equal(b, a)
    np.testing.assert_array_equal(c, r32["yop"])
    np.testing.assert_array_equal(d, a)


def test_forward_samples_with_storage_on(r32):
    """S = 3: row i S + s equals the plain forward on the repeated input within the 1e-4 |y|max of the samples tests; samples = 1 is
    the plain forward bit for bit; the typed samples-FIR kernel is the one launched"""
    cfg, x, z = r32["cfg"], r32["x"], r32["z"]
    n, s = x.shape[0], 3
    h, _ = make_handle(cfg, r32["sd"])
    h.set_fp16_blocks(*r32["flags"])
    _ = h.workspace_bytes_samples(n, s)
    info_ops = h.launches()
    h.set_fp16_storage(True)
    y1, _ = forward(h, cfg, x, z, samples=1)
    np.testing.assert_array_equal(y1, r32["yst"])
    zs = pkg.synth.make_latent(n * s, cfg.z_dim, 77)
    ys, info = forward(h, cfg, x, zs, samples=s)
    yr, _ = forward(h, cfg, np.repeat(x, s, axis=0), zs)
    h.close()
    seen = check_storage_names(info, info_ops, cfg, r32["flags"])
    assert "cm_fir_samples_h_kernel" in seen and "cm_fir_h_kernel" in seen          # (the encoder's FIR-down is per image)
    fir_up = [i["kernel"] for i in info if i["layer"].startswith("synthesis") and i["layer"].endswith(".fir")]
    assert fir_up and all("cm_fir_samples" in k for k in fir_up)
    err, top = float(np.abs(ys - yr).max()), float(np.abs(yr).max())
    print(f"forward_samples S=3, storage on, vs repeated forward: {err:.3e} (|y|max = {top:.3f})")
    assert err <= 1e-4 * top
    assert np.abs(ys[0] - ys[1]).max() > 1e-2          # the samples really differ
