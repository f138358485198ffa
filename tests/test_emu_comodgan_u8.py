"""CPU execution (fiber SIMT emulator, tests/emu) of the uint8 Co-Mod-GAN forward of include/comodgan_u8_hip.h: photo and mask bytes
in, composited bytes out, the pre- and post-processing inside the first and the last kernel.  Its definition is the three-step
path migan_pack_input -> comodgan_forward[_samples] -> migan_compose_output, byte for byte.  No GPU involved."""
import importlib
import os

import numpy as np
import pytest

from oracle import comodgan_oracle as orc
from oracle import migan_prepost as pp
from tests.comodgan_u8_case import CASES, make_u8, noise_floats, pkg
from tests.emu_util import aligned, emu_lib
from tests.test_emu_comodgan_samples import make_handle, small, workspace

hb = pkg.hipbind


def prepare(cfg, seed, fp16=None, cutoff=None):
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    h, keep = make_handle(cfg, sd)
    if fp16 is not None:
        h.set_fp16_blocks(fp16[0], fp16[1])
        h.set_fp16_storage(fp16[2])
    if cutoff is not None:
        h.set_truncation_cutoff(cutoff)
    return h, keep, sd


def three_step(lib, h, cfg, img, mask, za, n, s, wsv, nbytes, **opts):
    """migan_pack_input -> forward (S = 1) / forward_samples -> migan_compose_output on rows repeated S times -> [N * S,R,R,3], y"""
    r = cfg.resolution
    x = aligned(np.zeros((n, 4, r, r), np.float32))
    lib.pack_input(img.ctypes.data, mask.ctypes.data, x.ctypes.data, n, r)
    y = aligned(np.zeros((n * s, 3, r, r), np.float32))
    if s == 1:
        h.forward(x.ctypes.data, za.ctypes.data, y.ctypes.data, n, wsv.ctypes.data, nbytes, **opts)
    else:
        h.forward_samples(x.ctypes.data, za.ctypes.data, y.ctypes.data, n, s, wsv.ctypes.data, nbytes, **opts)
    imgr, maskr = np.ascontiguousarray(np.repeat(img, s, axis=0)), np.ascontiguousarray(np.repeat(mask, s, axis=0))
    want = np.full((n * s, r, r, 3), 99, np.uint8)
    lib.compose_output(y.ctypes.data, imgr.ctypes.data, maskr.ctypes.data, want.ctypes.data, n * s, r)
    return want, y


def fused(h, cfg, img, mask, za, n, s, wsv, nbytes, **opts):
    out = np.full((n * s, cfg.resolution, cfg.resolution, 3), 77, np.uint8)
    h.forward_u8(img.ctypes.data, mask.ctypes.data, za.ctypes.data, out.ctypes.data, n, s, wsv.ctypes.data, nbytes, **opts)
    return out


def abi_opts(opts):
    return {k: v for k, v in opts.items() if k != "truncation_cutoff"}


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_of_the_three_step_path(name):
    cfg, n, s, opts, fp16 = CASES[name]
    seed = 50 + list(CASES).index(name)
    lib = emu_lib()
    h, keep, sd = prepare(cfg, seed, fp16, opts.get("truncation_cutoff"))
    r = cfg.resolution
    img, mask = make_u8(n, r, seed)
    img0, mask0 = img.copy(), mask.copy()
    z = pkg.synth.make_latent(n * s, cfg.z_dim, seed)
    za = aligned(z)
    nbytes = h.workspace_bytes_samples(n, s)
    wsv = workspace(nbytes)
    want, y = three_step(lib, h, cfg, img, mask, za, n, s, wsv, nbytes, **abi_opts(opts))
    info32 = h.launches()
    out = fused(h, cfg, img, mask, za, n, s, wsv, nbytes, **abi_opts(opts))
    info8 = h.launches()
    assert h.workspace_bytes_samples(n, s) == nbytes                 # the workspace that served the fp32 path served the uint8 call
    h.close()
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(img, img0)                         # the inputs are only read
    np.testing.assert_array_equal(mask, mask0)
    known = np.repeat(mask == 255, s, axis=0)
    assert (out[known] == np.repeat(img, s, axis=0)[known]).all()
    # the two kernels of the case's form, and nothing else changed in the plan
    lpp = {64: 4, 128: 8}.get(cfg.channels(r), 16)
    half = fp16 is not None
    top, last = f"encoder.b{r}.fromrgb", f"synthesis.b{r}.torgb"
    changed = {a["layer"]: (a, b) for a, b in zip(info32, info8) if a != b}
    assert len(info32) == len(info8) and set(changed) == {top, last}
    a, b = changed[top]
    assert b["kernel"] == f"migan::cm_fromrgb_u8_kernel<{str(half).lower()}>"
    assert b["flops"] == a["flops"] and a["bytes"] - b["bytes"] == (16 - 4) * r * r          # 4 fp32 planes -> 3 + 1 bytes per pixel
    a, b = changed[last]
    assert b["kernel"] == f"migan::cm_torgb_u8_kernel<{lpp}, {str(half).lower()}>"
    assert b["flops"] == a["flops"] and a["bytes"] - b["bytes"] == s * (12 - (3 + 1 + 3)) * r * r  # 3 fp32 out -> 3 + 1 bytes in, 3 out
    if name != "lpp4":
        return
    # against the oracle: TOL = 1e-3 on y is 1e-3 * 127.5 < 1 byte step before truncation, so a byte moves by at most one
    xr = np.repeat(pp.preprocess(img, mask), s, axis=0)
    ref = pp.compose(orc.generator(xr, z, sd, r, cfg.num_ws), np.repeat(img, s, axis=0), np.repeat(mask, s, axis=0))
    step = np.abs(out.astype(np.int16) - ref.astype(np.int16))
    print("bytes off the oracle by one step:", int((step == 1).sum()), "of", step.size, "worst", int(step.max()))
    assert step.max() <= 1
    assert (out[known] == ref[known]).all()
    # not a copy: samples of one photo differ in its holes, and so do the photos
    o = out.reshape(n, s, r, r, 3)
    hole = mask != 255
    assert (o[0, 0][hole[0]] != o[0, 1][hole[0]]).any() and (o[1, 0][hole[1]] != o[1, 2][hole[1]]).any()
    both = hole[0] & hole[1]
    assert both.any() and (o[0, 0][both] != o[1, 0][both]).any()


def test_explicit_random_noise_reaches_the_uint8_forward():
    """noise_mode random with the caller's blob, laid out per sample as for comodgan_forward_samples"""
    cfg = small(16)
    n, s = 2, 2
    lib = emu_lib()
    h, keep, sd = prepare(cfg, 58)
    img, mask = make_u8(n, 16, 58)
    za = aligned(pkg.synth.make_latent(n * s, cfg.z_dim, 58))
    noise = aligned(pkg.synth.normal((n * s * noise_floats(16),), 7, "drawn-noise").astype(np.float32))
    assert noise_floats(16) == h.noise_floats()
    nbytes = h.workspace_bytes_samples(n, s)
    wsv = workspace(nbytes)
    opts = dict(noise_mode="random", noise_ptr=noise.ctypes.data)
    want, _ = three_step(lib, h, cfg, img, mask, za, n, s, wsv, nbytes, **opts)
    out = fused(h, cfg, img, mask, za, n, s, wsv, nbytes, **opts)
    const = fused(h, cfg, img, mask, za, n, s, wsv, nbytes)
    h.close()
    np.testing.assert_array_equal(out, want)
    assert (out != const).any()                                      # the blob was read


@pytest.mark.parametrize("static", [False, True])
def test_fp32_and_uint8_forwards_alternate_on_one_workspace(static):
    """the layout does not depend on the I/O mode: each call reproduces its own earlier result bit for bit, and with static
    weights asserted the planes the first call prepared serve all four"""
    cfg = small(16)
    n, s = 2, 2
    lib = emu_lib()
    h, keep, sd = prepare(cfg, 59)
    img, mask = make_u8(n, 16, 59)
    za = aligned(pkg.synth.make_latent(n * s, cfg.z_dim, 59))
    nbytes = h.workspace_bytes_samples(n, s)
    wsv = workspace(nbytes)
    if static:
        h.assume_static_weights(True)
    out_a = fused(h, cfg, img, mask, za, n, s, wsv, nbytes)
    want_a, y_a = three_step(lib, h, cfg, img, mask, za, n, s, wsv, nbytes)
    y_a = y_a.copy()
    out_b = fused(h, cfg, img, mask, za, n, s, wsv, nbytes)
    want_b, y_b = three_step(lib, h, cfg, img, mask, za, n, s, wsv, nbytes)
    preparations = h.weight_preparations()
    h.close()
    np.testing.assert_array_equal(out_a, out_b)
    np.testing.assert_array_equal(y_a, y_b)
    np.testing.assert_array_equal(out_a, want_a)
    np.testing.assert_array_equal(out_b, want_b)
    assert preparations == (1 if static else 4)


def test_c_abi_errors():
    cfg = small(16)
    n, s = 2, 2
    h, keep, sd = prepare(cfg, 60)
    img, mask = make_u8(n, 16, 60)
    za = aligned(pkg.synth.make_latent(n * s, cfg.z_dim, 60))
    nbytes = h.workspace_bytes_samples(n, s)
    small_bytes = h.workspace_bytes_samples(n, 1)
    assert small_bytes < nbytes
    wsv = workspace(nbytes)
    out = np.zeros((n * s, 16, 16, 3), np.uint8)
    args = [img.ctypes.data, mask.ctypes.data, za.ctypes.data, out.ctypes.data]
    with pytest.raises(ValueError, match="samples"):
        h.forward_u8(*args, n, 0, wsv.ctypes.data, nbytes)
    with pytest.raises(ValueError, match="samples"):
        h.forward_u8(*args, 1 << 20, 1 << 12, wsv.ctypes.data, nbytes)            # batch * samples = 2^32
    for k in range(4):
        bad = list(args)
        bad[k] = 0
        with pytest.raises(ValueError, match="null tensor"):
            h.forward_u8(*bad, n, s, wsv.ctypes.data, nbytes)
    with pytest.raises(ValueError, match="empty batch"):
        h.forward_u8(*args, 0, s, wsv.ctypes.data, nbytes)
    with pytest.raises(ValueError, match="workspace too small"):
        h.forward_u8(*args, n, s, wsv.ctypes.data, small_bytes)
    with pytest.raises(ValueError, match="workspace"):
        h.forward_u8(*args, n, s, 0, nbytes)
    with pytest.raises(ValueError, match="workspace"):
        h.forward_u8(*args, n, s, wsv.ctypes.data + 4, nbytes)                   # 256-byte alignment
    with pytest.raises(ValueError, match="noise"):
        h.forward_u8(*args, n, s, wsv.ctypes.data, nbytes, noise_mode="random")  # random without the blob
    with pytest.raises(ValueError, match="launch_ms"):
        h.lib.check(h.lib.lib.comodgan_forward_u8_timed(h._h, *args, n, s, 1.0, 1, None, wsv.ctypes.data, nbytes, None, None, 0))
    assert (out == 0).all()                                                       # no refused call wrote anything
    ms = h.forward_u8(*args, n, s, wsv.ctypes.data, nbytes, timed=True)
    assert len(ms) == len(h.launches()) and "migan::cm_fromrgb_u8_kernel<false>" in {i["kernel"] for i in h.launches()}
    h.close()
    # before commit
    raw = hb.CoModGANHandle(emu_lib(), cfg.resolution, cfg.num_ws, cfg.ch_base, cfg.ch_max, cfg.z_dim, cfg.w_dim, cfg.w0_dim, cfg.map_layers)
    with pytest.raises(hb.MiganError, match="before comodgan_commit"):
        raw.forward_u8(*args, n, s, wsv.ctypes.data, nbytes)
    raw.close()


def test_exports_and_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = importlib.import_module("mi-gan_amd.build")
    assert os.path.join(root, "include", "comodgan_u8_hip.h") in build.sources()  # a change of the header rebuilds the library
