"""CPU execution (fiber SIMT emulator, tests/emu) of the staged Co-Mod-GAN calls of include/comodgan_stages_hip.h: comodgan_mapping,
comodgan_encode and comodgan_synthesize with the stage tensors (ws, w0, the per-resolution features) in caller memory.  Composed they
make the launches of the fused forward on the same operands, so they must give its bits; with per-layer rows of ws the CPU oracle's
synthesis is the reference.  No GPU involved."""
import importlib

import numpy as np
import pytest
import torch

from oracle import comodgan_oracle as orc
from tests.emu_util import aligned, emu_lib

pkg = importlib.import_module("mi-gan_amd")
cs = importlib.import_module("mi-gan_amd.comodgan_schema")
hb = pkg.hipbind
TOL = 1e-3


def cfg16():
    return cs.Config(resolution=16, ch_base=1024, ch_max=64, num_ws=cs.default_num_ws(16))


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


def resolutions(cfg):
    return [1 << k for k in range(2, cfg.resolution.bit_length())]


def channels(cfg, res):
    return min(cfg.ch_base // res, cfg.ch_max)


def encode(h, cfg, x, wsv, nbytes):
    """-> w0 [N, w0_dim], feats {res: NHWC array}"""
    n = x.shape[0]
    xa = aligned(x)
    w0 = aligned(np.zeros((n, cfg.w0_dim), np.float32))
    feats = {res: aligned(np.zeros((n, res, res, channels(cfg, res)), np.float32)) for res in resolutions(cfg)}
    h.encode(xa.ctypes.data, w0.ctypes.data, [feats[r].ctypes.data for r in resolutions(cfg)], n, wsv.ctypes.data, nbytes)
    return w0, feats


def synthesize(h, cfg, w0, feats, rows, samples, wsv, nbytes, noise_mode="const", outs=False):
    n, b = w0.shape[0], w0.shape[0] * samples
    rows = aligned(rows)
    y = aligned(np.zeros((b, 3, cfg.resolution, cfg.resolution), np.float32))
    rgb = img = None
    if outs:
        rgb = {r: aligned(np.zeros((b, 3, r, r), np.float32)) for r in resolutions(cfg) if r > 4}
        img = {r: aligned(np.zeros((b, 3, r, r), np.float32)) for r in resolutions(cfg) if r < cfg.resolution}
    h.synthesize(w0.ctypes.data, [feats[r].ctypes.data for r in resolutions(cfg)], rows.ctypes.data, y.ctypes.data, n, samples, wsv.ctypes.data,
                 nbytes, noise_mode, None, None if rgb is None else [rgb[r].ctypes.data if r in rgb else 0 for r in resolutions(cfg)],
                 None if img is None else [img[r].ctypes.data if r in img else 0 for r in resolutions(cfg)])
    return y, rgb, img


def test_r16_composition_gives_the_bits_of_the_fused_forward():
    """mapping(psi 0.7, cutoff 3) -> encode -> synthesize against comodgan_forward with the same options on one handle and one
    workspace: the same kernels on the same operands, bit for bit; each stage reports its own launches; the fused plan is unchanged."""
    cfg = cfg16()
    n = 2
    sd = pkg.synth.make_comodgan_state_dict(cfg, 41)
    x, z = pkg.synth.make_input(n, 16, 41), pkg.synth.make_latent(n, cfg.z_dim, 41)
    h, keep = make_handle(cfg, sd)
    h.set_truncation_cutoff(3)
    nbytes = h.stages_workspace_bytes(n, 1)
    assert nbytes >= h.workspace_bytes(n)
    wsv = workspace(nbytes)
    xa, za = aligned(x), aligned(z)
    y_fused = aligned(np.zeros((n, 3, 16, 16), np.float32))
    h.forward(xa.ctypes.data, za.ctypes.data, y_fused.ctypes.data, n, wsv.ctypes.data, nbytes, truncation_psi=0.7)
    info_fused = h.launches()
    rows = aligned(np.zeros((n, cfg.num_ws, cfg.w_dim), np.float32))
    h.mapping(za.ctypes.data, rows.ctypes.data, n, wsv.ctypes.data, nbytes, truncation_psi=0.7, truncation_cutoff=3)
    info_map = h.launches()
    w0, feats = encode(h, cfg, x, wsv, nbytes)
    info_enc = h.launches()
    y, _, _ = synthesize(h, cfg, w0, feats, rows, 1, wsv, nbytes)
    info_syn = h.launches()
    h.workspace_bytes(n)
    assert h.launches() == info_fused
    h.close()
    np.testing.assert_array_equal(y, y_fused)
    # rows below the cutoff are truncated copies of one w, the others raw copies of another
    assert np.array_equal(rows[:, 0], rows[:, 2]) and np.array_equal(rows[:, 3], rows[:, cfg.num_ws - 1])
    assert np.abs(rows[:, 2] - rows[:, 3]).max() > 1e-3
    want_rows = orc.mapping(torch.from_numpy(z), {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cfg.num_ws, cfg.map_layers, 0.7, 3).numpy()
    assert np.abs(rows - want_rows).max() <= 2e-5 * max(1.0, np.abs(want_rows).max())
    want = orc.generator(x, z, sd, 16, cfg.num_ws, truncation_psi=0.7, truncation_cutoff=3)
    assert np.abs(y - want).max() <= TOL
    # the launch lists: every fused launch belongs to exactly one stage, under the same kernel, except the affine launch (rows form);
    # the mapping stage adds the expansion to ws and prepares no weights
    fused = {i["layer"]: i for i in info_fused}
    layers = lambda info: [i["layer"] for i in info]
    assert layers(info_map) == [f"mapping.fc{i}" for i in range(cfg.map_layers)] + ["mapping.ws"]
    assert info_map[-1]["kernel"] == "migan::cm_ws_rows_kernel"
    prep = [l for l in layers(info_fused) if l.endswith((".wprep", ".split"))]
    assert layers(info_enc)[:len(prep)] == prep and layers(info_syn)[:len(prep)] == prep
    enc = [l for l in layers(info_enc) if l not in prep]
    syn = [l for l in layers(info_syn) if l not in prep]
    assert enc and all(l.startswith("encoder.") for l in enc) and all(l.startswith("synthesis.") for l in syn)
    assert sorted(layers(info_map)[:-1] + enc + syn + prep) == sorted(layers(info_fused))
    for i in info_enc + info_syn + info_map[:-1]:
        if i["layer"] == "synthesis.affine":
            assert i["kernel"] == "migan::cm_dense_multi_rows_kernel" and i["flops"] == fused[i["layer"]]["flops"]
        else:
            assert i == fused[i["layer"]], i["layer"]


def test_distinct_rows_and_intermediate_outputs_against_the_oracle():
    """Every row of ws different, N = 2 images x S = 2 samples: the oracle's synthesis on the oracle's encoder output is the reference;
    had every layer read row 0 the answer would be off by far more than the tolerance.  The optional outputs: res_img against the
    oracle's running images, res_to_rgb against their un-added part, and the image itself unchanged by asking for them."""
    cfg = cfg16()
    n, s = 2, 2
    sd = pkg.synth.make_comodgan_state_dict(cfg, 42)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    x = pkg.synth.make_input(n, 16, 42)
    rows = pkg.synth.normal((n * s, cfg.num_ws, cfg.w_dim), 42, "ws-rows").astype(np.float32)
    h, keep = make_handle(cfg, sd)
    nbytes = h.stages_workspace_bytes(n, s)
    wsv = workspace(nbytes)
    w0, feats = encode(h, cfg, x, wsv, nbytes)
    y, _, _ = synthesize(h, cfg, w0, feats, rows, s, wsv, nbytes)
    y2, rgb, img = synthesize(h, cfg, w0, feats, rows, s, wsv, nbytes, outs=True)
    kernels = {i["layer"]: i["kernel"] for i in h.launches()}
    h.close()
    with torch.no_grad():
        g, ofeats = orc.encoder(torch.from_numpy(x), tsd, 16)
        for r in resolutions(cfg):
            assert np.abs(np.transpose(feats[r], (0, 3, 1, 2)) - ofeats[r].numpy()).max() <= 2e-4 * max(1.0, float(ofeats[r].abs().max())), r
        assert np.abs(w0 - g.numpy()).max() <= 2e-4 * max(1.0, float(g.abs().max()))
        gr = g.repeat_interleave(s, 0)
        fr = {r: f.repeat_interleave(s, 0) for r, f in ofeats.items()}
        taps = {}
        want = orc.synthesis(gr, fr, torch.from_numpy(rows), tsd, 16, taps=taps).numpy()
        row0 = orc.synthesis(gr, fr, torch.from_numpy(rows[:, :1]).repeat(1, cfg.num_ws, 1), tsd, 16).numpy()
        up = {r: orc.upsample2d(taps[f"synthesis.b{r // 2}.img"], orc.fir(torch.float32)).numpy() for r in (8, 16)}
    assert np.abs(row0 - want).max() > 10 * TOL             # the rows matter for this seed
    err = np.abs(y - want).max()
    print("distinct rows, output max abs err", err)
    assert err <= TOL
    np.testing.assert_array_equal(y2, y)
    assert kernels["synthesis.b8.torgb"] == "migan::cm_torgb_parts_kernel<4>" and kernels["synthesis.b4.torgb"] == "migan::cm_torgb_kernel<4>"
    assert sorted(rgb) == [8, 16] and sorted(img) == [4, 8]
    for r in (4, 8):
        assert np.abs(img[r] - taps[f"synthesis.b{r}.img"].numpy()).max() <= TOL, r
    for r in (8, 16):
        part = taps[f"synthesis.b{r}.img"].numpy() - up[r]
        assert np.abs(rgb[r] - part).max() <= TOL, r
        assert np.abs(part).max() > 10 * TOL


def test_static_weights_span_encode_synthesize_and_forward():
    """comodgan_assume_static_weights on one workspace: comodgan_encode prepares the weight planes, comodgan_synthesize and
    comodgan_forward find them (an in-place change of a 3x3 weight after the encode is not seen: that is the contract); the
    mapping stage in between leaves them alone."""
    cfg = cfg16()
    n = 1
    sd = pkg.synth.make_comodgan_state_dict(cfg, 43)
    x, z = pkg.synth.make_input(n, 16, 43), pkg.synth.make_latent(n, cfg.z_dim, 43)
    h, keep = make_handle(cfg, sd)
    nbytes = h.stages_workspace_bytes(n, 1)
    wsv = workspace(nbytes)
    xa, za = aligned(x), aligned(z)
    want = orc.generator(x, z, sd, 16, cfg.num_ws)              # (before the in-place write below: keep may alias sd)
    h.assume_static_weights(True)
    assert h.weight_preparations() == 0
    w0, feats = encode(h, cfg, x, wsv, nbytes)
    assert h.weight_preparations() == 1
    keep["encoder.b16.conv0.weight"] *= 1.5                 # in place, same address: read again only by a call that prepares
    rows = aligned(np.zeros((n, cfg.num_ws, cfg.w_dim), np.float32))
    h.mapping(za.ctypes.data, rows.ctypes.data, n, wsv.ctypes.data, nbytes)
    y, _, _ = synthesize(h, cfg, w0, feats, rows, 1, wsv, nbytes)
    yf = aligned(np.zeros((n, 3, 16, 16), np.float32))
    h.forward(xa.ctypes.data, za.ctypes.data, yf.ctypes.data, n, wsv.ctypes.data, nbytes)
    assert h.weight_preparations() == 1
    np.testing.assert_array_equal(y, yf)
    assert np.abs(y - want).max() <= TOL                       # the weights as they were when prepared
    h.assume_static_weights(False)
    w0b, _ = encode(h, cfg, x, wsv, nbytes)
    assert h.weight_preparations() == 2 and np.abs(w0b - w0).max() > 1e-3
    h.close()


def test_c_abi_errors():
    cfg = cfg16()
    sd = pkg.synth.make_comodgan_state_dict(cfg, 44)
    h, keep = make_handle(cfg, sd)
    nbytes = h.stages_workspace_bytes(2, 3)
    assert nbytes >= h.workspace_bytes_samples(2, 3) and nbytes >= h.stages_workspace_bytes(2, 1)
    wsv = workspace(nbytes)
    w0, feats = encode(h, cfg, pkg.synth.make_input(2, 16, 44), wsv, nbytes)
    rows = aligned(np.zeros((6, cfg.num_ws, cfg.w_dim), np.float32))
    with pytest.raises(ValueError, match="workspace too small"):
        synthesize(h, cfg, w0, feats, rows, 3, wsv, 4096)
    with pytest.raises(ValueError, match="samples"):
        synthesize(h, cfg, w0, feats, rows, 0, wsv, nbytes)
    with pytest.raises(ValueError, match="feats"):
        h.encode(w0.ctypes.data, w0.ctypes.data, [feats[4].ctypes.data], 2, wsv.ctypes.data, nbytes)
    with pytest.raises(ValueError, match="feature tensor"):
        h.encode(w0.ctypes.data, w0.ctypes.data, [feats[4].ctypes.data, 0, feats[16].ctypes.data], 2, wsv.ctypes.data, nbytes)
    with pytest.raises(ValueError, match="truncation_cutoff"):
        h.mapping(w0.ctypes.data, rows.ctypes.data, 2, wsv.ctypes.data, nbytes, truncation_cutoff=-3)
    h.close()
