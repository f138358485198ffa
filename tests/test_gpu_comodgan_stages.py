"""The callable stages of the Co-Mod-GAN drop-in on a real MI355X: G.mapping / G.encoder / G.synthesis (nn.Module ->
include/comodgan_stages_hip.h -> HIP kernels) with the reference's signatures and the stage tensors in torch memory.

Composed at equal batch the stages make the launches of the fused forward on the same operands (the affine launch reads the same
values through rows of ws), so the composition must give the fused forward's bits.  With per-layer rows and for the intermediate
outputs the CPU oracle is the reference, at the tolerance of tests/test_gpu_comodgan.py."""
import os

import numpy as np
import pytest
import torch

from oracle import comodgan_oracle as orc
from tests.comodgan_fp16_case import build as build_fp16
from tests.comodgan_fp16_case import envelope, inputs, load_case

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _cfg(pkg, r, cb, cm):
    cs = pkg.comodgan_schema
    return cs.Config(resolution=r, ch_base=cb, ch_max=cm, num_ws=cs.default_num_ws(r))


def _build(pkg, cfg, seed, dev):
    cm = pkg.comodgan
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=cfg.resolution, **kw), cm.Synthesis(resolution=cfg.resolution, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval(), sd


def _resolutions(r):
    return [1 << k for k in range(2, r.bit_length())]


@pytest.fixture(scope="module")
def r16(pkg, dev):
    """R = 16 (the shape test_module_errors_on_gpu builds), N = 3: the module, its weights, inputs, and the oracle's encoder output"""
    cfg = _cfg(pkg, 16, 1024, 64)
    m, sd = _build(pkg, cfg, 61, dev)
    x, z = pkg.synth.make_input(3, 16, 61), pkg.synth.make_latent(3, cfg.z_dim, 61)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    with torch.no_grad():
        g, feats = orc.encoder(torch.from_numpy(x), tsd, 16)
    return dict(cfg=cfg, m=m, sd=sd, tsd=tsd, x=x, z=z, xt=torch.from_numpy(x).to(dev), zt=torch.from_numpy(z).to(dev), g=g, feats=feats)


@pytest.mark.parametrize("mode", ["const", "none"])
def test_r16_composition_equals_the_fused_forward(r16, mode):
    m, xt, zt = r16["m"], r16["xt"], r16["zt"]
    with torch.no_grad():
        y = m(xt, zt, truncation_psi=0.7, truncation_cutoff=3, noise_mode=mode)
        ws = m.mapping(zt, truncation_psi=0.7, truncation_cutoff=3)
        x, feats = m.encoder(xt)
        ys = m.synthesis(x, feats, ws, noise_mode=mode)
    assert ws.shape == (3, r16["cfg"].num_ws, 512) and ws.dtype == torch.float32
    assert x.shape == (3, 1024) and list(feats) == [16, 8, 4]
    for res, f in feats.items():
        assert f.shape == (3, 64, res, res) and f.dtype == torch.float32 and f.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(ys, y)                              # the same kernels on the same operands
    assert torch.equal(ws[:, 0], ws[:, 2]) and torch.equal(ws[:, 3], ws[:, 5]) and not torch.equal(ws[:, 2], ws[:, 3])
    assert m._lib.backend() == "hip:gfx950"


def test_composition_at_every_torgb_width(pkg, dev):
    """R = 32 with ch_base 2048, ch_max 256: 256 channels at res 4 / 8, 128 at 16, 64 at 32 -- the ToRGB launches of 16, 8 and 4 lanes
    per pixel -- with and without the intermediate outputs (the _parts symbols of all three widths)."""
    cfg = _cfg(pkg, 32, 2048, 256)
    m, sd = _build(pkg, cfg, 62, dev)
    xt = torch.from_numpy(pkg.synth.make_input(3, 32, 62)).to(dev)
    zt = torch.from_numpy(pkg.synth.make_latent(3, cfg.z_dim, 62)).to(dev)
    with torch.no_grad():
        y = m(xt, zt, truncation_psi=0.7, truncation_cutoff=3, noise_mode="const")
        fused = {i["layer"]: i["kernel"] for i in m.launch_info()}
        ws = m.mapping(zt, truncation_psi=0.7, truncation_cutoff=3)
        x, feats = m.encoder(xt)
        ys = m.synthesis(x, feats, ws, noise_mode="const")
        plain = {i["layer"]: i["kernel"] for i in m.launch_info()}
        yo, outs = m.synthesis(x, feats, ws, noise_mode="const", return_intermediate_outs=True)
        parts = {i["layer"]: i["kernel"] for i in m.launch_info()}
    assert {fused[f"synthesis.b{r}.torgb"] for r in (4, 8, 16, 32)} == {f"migan::cm_torgb_kernel<{l}>" for l in (4, 8, 16)}
    assert all(plain[f"synthesis.b{r}.torgb"] == fused[f"synthesis.b{r}.torgb"] for r in (4, 8, 16, 32))
    assert [parts[f"synthesis.b{r}.torgb"] for r in (4, 8, 16, 32)] == ["migan::cm_torgb_kernel<16>", "migan::cm_torgb_parts_kernel<16>",
                                                                       "migan::cm_torgb_parts_kernel<8>", "migan::cm_torgb_parts_kernel<4>"]
    assert torch.equal(ys, y) and torch.equal(yo, y)
    for res in (8, 16, 32):                                # the device's own upsample-then-add: fp32 sums of the two stored parts
        assert float(outs["res_to_rgb"][res].abs().max()) > 1e-2
        up = outs["res_img"][res] - outs["res_to_rgb"][res]
        want = orc.upsample2d(outs["res_img"][res // 2].cpu(), orc.fir(torch.float32))
        assert float((up.cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max())), res


def _oracle_synthesis(r16, rows, s=1, taps=None):
    with torch.no_grad():
        g = r16["g"].repeat_interleave(s, 0)
        feats = {r: f.repeat_interleave(s, 0) for r, f in r16["feats"].items()}
        return orc.synthesis(g, feats, rows, r16["tsd"], 16, taps=taps).numpy()


@pytest.mark.parametrize("kind", ["random", "mix"])
def test_per_layer_rows_matter(pkg, r16, dev, kind):
    """Every row of ws distinct: random rows; a style mix of two mapped latents crossing at row 2, inside block b8 (rows 1, 2, 3)."""
    m, cfg = r16["m"], r16["cfg"]
    with torch.no_grad():
        x, feats = m.encoder(r16["xt"])
        if kind == "random":
            rows = torch.from_numpy(pkg.synth.normal((3, cfg.num_ws, cfg.w_dim), 63, "ws-rows").astype(np.float32))
        else:
            za = torch.from_numpy(pkg.synth.make_latent(3, cfg.z_dim, 64)).to(dev)
            wa, wb = m.mapping(r16["zt"]).cpu(), m.mapping(za).cpu()
            scale = 1.0 + 0.05 * torch.arange(cfg.num_ws, dtype=torch.float32)[None, :, None]      # all rows distinct
            rows = torch.cat([wa[:, :2], wb[:, 2:]], 1) * scale
        y = m.synthesis(x, feats, rows.to(dev), noise_mode="const").cpu().numpy()
    want = _oracle_synthesis(r16, rows)
    row0 = _oracle_synthesis(r16, rows[:, :1].repeat(1, cfg.num_ws, 1))
    assert float(np.abs(row0 - want).max()) > TOL          # a walk that read row 0 everywhere would fail below
    err = float(np.abs(y - want).max())
    print(f"{kind} rows: max abs err {err:.3e}, row-0 answer off by {float(np.abs(row0 - want).max()):.3e}")
    assert err <= TOL


def test_intermediate_outputs(pkg, r16, dev):
    m, cfg = r16["m"], r16["cfg"]
    rows = torch.from_numpy(pkg.synth.normal((3, cfg.num_ws, cfg.w_dim), 65, "ws-rows").astype(np.float32))
    with torch.no_grad():
        x, feats = m.encoder(r16["xt"])
        y = m.synthesis(x, feats, rows.to(dev), noise_mode="const")
        yo, outs = m.synthesis(x, feats, rows.to(dev), noise_mode="const", return_intermediate_outs=True)
    taps = {}
    want = _oracle_synthesis(r16, rows, taps=taps)
    assert sorted(outs) == ["res_img", "res_to_rgb"] and sorted(outs["res_img"]) == [4, 8, 16] and sorted(outs["res_to_rgb"]) == [4, 8, 16]
    assert outs["res_to_rgb"][4] is outs["res_img"][4]
    seen = set()
    for key in ("res_to_rgb", "res_img"):
        for res, t in outs[key].items():
            assert t.shape == (3, 3, res, res) and t.dtype == torch.float32 and t.is_contiguous(), (key, res)
            seen.add(t.data_ptr())
    assert len(seen) == 5                                  # one tensor at res 4, res_img[R] is img, everything else distinct
    assert torch.equal(outs["res_img"][16], yo) and torch.equal(yo, y)
    assert float(np.abs(yo.cpu().numpy() - want).max()) <= TOL
    f = orc.fir(torch.float32)
    for res in (4, 8, 16):
        tap = taps[f"synthesis.b{res}.img"]
        assert float((outs["res_img"][res].cpu() - tap).abs().max()) <= TOL, res
        if res > 4:
            part = tap - orc.upsample2d(taps[f"synthesis.b{res // 2}.img"], f)
            assert float(part.abs().max()) > 10 * TOL
            assert float((outs["res_to_rgb"][res].cpu() - part).abs().max()) <= TOL, res


def test_reference_golden_intermediate_outputs(pkg, dev, golden_dir):
    """tests/golden/cmstages_r16.npz: the reference Generator called with return_intermediate_outs=True (make_golden_comodgan_stages.py)"""
    g = np.load(os.path.join(golden_dir, "cmstages_r16.npz"))
    r, cb, cmx, n, seed = (int(v) for v in g["cfg"])
    cfg = _cfg(pkg, r, cb, cmx)
    m, _ = _build(pkg, cfg, seed, dev)
    xt = torch.from_numpy(pkg.synth.make_input(n, r, seed)).to(dev)
    zt = torch.from_numpy(pkg.synth.make_latent(n, cfg.z_dim, seed)).to(dev)
    with torch.no_grad():
        ws = m.mapping(zt, None, truncation_psi=float(g["psi"]), truncation_cutoff=int(g["cutoff"]))
        y, outs = m.synthesis(*m.encoder(xt), ws, noise_mode="const", return_intermediate_outs=True)
    assert float(np.abs(ws.cpu().numpy() - g["ws"]).max()) <= TOL
    assert float(np.abs(y.cpu().numpy() - g["y"]).max()) <= TOL
    for key in ("res_to_rgb", "res_img"):
        for res in _resolutions(r):
            err = float(np.abs(outs[key][res].cpu().numpy() - g[f"{key}:{res}"]).max())
            assert np.isfinite(err) and err <= TOL, (key, res, err)


def test_complete_later(pkg, r16, dev):
    """N = 2 images, S = 3 samples: synthesis on six rows of ws against the features of two images is forward_samples; the features are
    the caller's tensors, so an unrelated forward in between changes nothing."""
    m, cfg = r16["m"], r16["cfg"]
    xt = r16["xt"][:2]
    z = torch.from_numpy(pkg.synth.make_latent(6, cfg.z_dim, 66)).to(dev)
    x2 = torch.from_numpy(pkg.synth.make_input(3, 16, 67)).to(dev)
    with torch.no_grad():
        want = m.forward_samples(xt, z.reshape(2, 3, -1), noise_mode="const")
        x, feats = m.encoder(xt)
        ws6 = m.mapping(z)
        y = m.synthesis(x, feats, ws6, noise_mode="const")
        m(x2, noise_mode="random")
        y_later = m.synthesis(x, feats, ws6, noise_mode="const")
    want = want.reshape(6, 3, 16, 16)
    err, top = float((y - want).abs().max()), float(want.abs().max())
    print(f"complete later vs forward_samples: max abs diff {err:.3e} (|y|max {top:.3f}), bit-equal {torch.equal(y, want)}")
    assert torch.equal(y, want)                            # the launches coincide: same kernels, same batch, same operands
    assert torch.equal(y_later, y)
    assert float((y[0] - y[1]).abs().max()) > 1e-2 and float((y[0] - y[3]).abs().max()) > 1e-2


def test_fp16_storage_features(pkg, dev, golden_dir):
    """R = 64, blocks above 16 marked on both sides, fp16 storage: the features of the marked blocks are float16 channels_last, the
    composition gives the fused forward's bits, and features handed back as fp32 NCHW are converted (exactly) before the call."""
    g, cfg, seed, n, flags = load_case(pkg, golden_dir, "r64_c64")
    assert flags == (16, 16)
    m = build_fp16(pkg, cfg, seed, dev, flags).set_fp16_storage()
    xt, zt = inputs(pkg, cfg, n, seed, dev)
    with torch.no_grad():
        y = m(xt, z=zt, noise_mode="const")
        x, feats = m.encoder(xt)
        ws = m.mapping(zt)
        ys = m.synthesis(x, feats, ws, noise_mode="const")
        wide = {r: f.float().contiguous() for r, f in feats.items()}
        yw = m.synthesis(x, wide, ws, noise_mode="const")
    for res, f in feats.items():
        assert f.dtype == (torch.float16 if res > 16 else torch.float32), res
        assert f.is_contiguous(memory_format=torch.channels_last) and f.shape == (n, 64, res, res)
    assert torch.equal(ys, y)
    envelope("r64_c64 stages, storage on", ys.cpu().numpy(), g)
    envelope("r64_c64 stages, features through fp32 NCHW", yw.cpu().numpy(), g)
    assert torch.equal(yw, ys)                             # fp16 -> fp32 -> fp16 is exact


def test_errors(pkg, r16, dev):
    m, cfg, cm = r16["m"], r16["cfg"], pkg.comodgan
    with torch.no_grad():
        x, feats = m.encoder(r16["xt"])
        ws = m.mapping(r16["zt"])
    with pytest.raises(ValueError, match="resolution 8"):
        m.synthesis(x, {k: v for k, v in feats.items() if k != 8}, ws)
    with pytest.raises(ValueError, match="4 rows for 3"):
        m.synthesis(x, feats, torch.cat([ws, ws[:1]]))
    with pytest.raises(RuntimeError, match="feats\\[8\\]"):
        m.synthesis(x, {**feats, 8: feats[16]}, ws)
    with pytest.raises(RuntimeError):
        m.synthesis(x, feats, ws[:, :3])
    for call in (lambda: m.mapping(torch.zeros(1, 512)), lambda: m.encoder(torch.zeros(1, 4, 16, 16)),
                 lambda: m.synthesis(x.cpu(), feats, ws)):
        with pytest.raises(RuntimeError):                  # CPU tensor
            call()
    with pytest.raises(ValueError):
        m.mapping(r16["zt"], truncation_cutoff=-2)
    for stage, args in ((cm.Mapping(num_ws=cfg.num_ws), (r16["zt"],)), (cm.Encoder(resolution=16, ch_base=1024, ch_max=64), (r16["xt"],)),
                        (cm.Synthesis(resolution=16, ch_base=1024, ch_max=64), (x, feats, ws))):
        with pytest.raises(NotImplementedError):           # a stage outside a Generator holds parameters only
            stage.to(dev)(*args)
    with pytest.raises(NotImplementedError, match="G.synthesis"):
        m(r16["xt"], return_intermediate_outs=True)


def test_freeze_weights_spans_the_stage_calls(pkg, dev):
    """encoder, synthesis, forward on one frozen model: each call's launch list starts with the weight preparation (it is part of the
    plan), the library ran it once -- an in-place write after the first call is not seen, as freeze_weights() documents."""
    cfg = _cfg(pkg, 16, 1024, 64)
    m, sd = _build(pkg, cfg, 68, dev)
    xt = torch.from_numpy(pkg.synth.make_input(2, 16, 68)).to(dev)
    zt = torch.from_numpy(pkg.synth.make_latent(2, cfg.z_dim, 68)).to(dev)
    with torch.no_grad():
        want = m(xt, zt, noise_mode="const")
        m.freeze_weights()
        before = m._handle.weight_preparations()
        x, feats = m.encoder(xt)
        lists = [m.launch_info()]
        assert m._handle.weight_preparations() == before + 1
        m.encoder.b16.conv0.weight.data.mul_(1.5)
        ws = m.mapping(zt)
        ys = m.synthesis(x, feats, ws, noise_mode="const")
        lists.append(m.launch_info())
        y = m(xt, zt, noise_mode="const")
        lists.append(m.launch_info())
        assert m._handle.weight_preparations() == before + 1
        m.freeze_weights(False)
        x2, _ = m.encoder(xt)
        assert m._handle.weight_preparations() == before + 2
    prep = [[i["layer"] for i in info if i["layer"].endswith((".wprep", ".split"))] for info in lists]
    assert prep[0] and prep[0] == prep[1] == prep[2]
    assert torch.equal(ys, want) and torch.equal(y, want)
    assert float((x2 - x).abs().max()) > 1e-3
