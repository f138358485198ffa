"""Several completions per photo on the MI355X, written out of place: migan_pipeline_batch_post_samples through ctypes on device
buffers, and MIGAN_Pipeline.forward_samples around a Co-Mod-GAN (S completions from one encoder pass) and around the MI-GAN
generator (one completion).  The yardstick of every byte comparison is the existing in-place path on device copies
(pipeline_batch_post / forward_batch), fed the same generator output."""
import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests.pipeline_batch_case import five_items

pytestmark = pytest.mark.gpu
RES, PADDING = 64, 8


def _device_items(images, masks, dev):
    d_img = [torch.from_numpy(a)[None].to(dev) for a in images]
    d_mask = [torch.from_numpy(m)[None, None].to(dev) for m in masks]
    return d_img, d_mask


def _items(d_img, d_mask):
    return [(a.data_ptr(), m.data_ptr(), a.shape[-2], a.shape[-1], m.shape[-2], m.shape[-1]) for a, m in zip(d_img, d_mask)]


def _pre(lib, d_img, d_mask, dev, stream):
    """pipeline_batch_pre -> items, scratch, bbox [n, 4], x [n, 4, R, R]"""
    items = _items(d_img, d_mask)
    scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=dev)
    bbox = torch.empty((len(items), 4), dtype=torch.int32, device=dev)
    x = torch.empty((len(items), 4, RES, RES), dtype=torch.float32, device=dev)
    lib.pipeline_batch_pre(items, RES, PADDING, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), stream)
    return items, scratch, bbox, x


def _post_on_copies(lib, d_img, d_mask, scratch, bbox, y, samples, gauss, stream):
    """-> want[i][s]: the existing pipeline_batch_post on a device copy of every image, once per sample (y rows s, S + s, ...)"""
    want = [[None] * samples for _ in d_img]
    for s in range(samples):
        copies = [a.clone() for a in d_img]
        ys = y[s::samples].contiguous()
        lib.pipeline_batch_post(_items(copies, d_mask), RES, ys.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), gauss25=gauss, stream=stream)
        for i, c in enumerate(copies):
            want[i][s] = c[0]
    return want


def _migan_pipeline(pkg, dev):
    sd = pkg.synth.make_state_dict(RES, seed=1, regime="export")
    m = pkg.Generator(resolution=RES)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, RES, padding=PADDING, device=dev)


def _comodgan_pipeline(pkg, dev):
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    cfg = cs.Config(resolution=RES, ch_base=4096, ch_max=64, num_ws=cs.default_num_ws(RES))
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=RES, **kw), cm.Synthesis(resolution=RES, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 41)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, RES, padding=PADDING, device=dev), cfg


def test_c_abi_on_device_buffers(pkg):
    """the five items and a 300 x 200 image with a 20 x 20 hole (most of its tiles only copy), S = 3"""
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(51)
    samples = 3
    images, masks = five_items(rng)
    images.append(rng.integers(0, 256, (3, 300, 200), dtype=np.uint8))
    masks.append(np.full((300, 200), 255, dtype=np.uint8))
    masks[5][140:160, 90:110] = 0
    d_img, d_mask = _device_items(images, masks, dev)
    y = torch.from_numpy((rng.standard_normal((6 * samples, 3, RES, RES)) * 0.6).astype(np.float32)).to(dev)
    items, scratch, bbox, _ = _pre(lib, d_img, d_mask, dev, stream)
    outs = [torch.full((samples, 3) + tuple(a.shape[-2:]), 0xA5, dtype=torch.uint8, device=dev) for a in d_img]
    lib.pipeline_batch_post_samples(items, samples, RES, y.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), [o.data_ptr() for o in outs],
                                    stream=stream)
    want = _post_on_copies(lib, d_img, d_mask, scratch, bbox, y, samples, None, stream)
    boxes = bbox.cpu().tolist()
    assert boxes == [list(po.masked_bbox(m, RES, PADDING)) for m in masks]
    assert boxes[5][1] - boxes[5][0] == 64 and boxes[5][3] - boxes[5][2] == 64       # 64 x 64 of 300 x 200: most tiles only copy
    for i in range(6):
        assert torch.equal(d_img[i].cpu(), torch.from_numpy(images[i])[None]), f"source image {i} was written"
        for s in range(samples):
            assert torch.equal(outs[i][s], want[i][s]), f"item {i}, sample {s}"
    assert not torch.equal(outs[5][0], outs[5][1])


def test_comodgan_through_the_module(pkg):
    """three images of different sizes, S = 2: forward_samples == pipeline_batch_pre -> model.forward_samples -> the in-place post on
    copies (that forward is run-to-run identical: tests/test_gpu_comodgan_samples.py::test_properties)"""
    dev = torch.device("cuda:0")
    pipe, cfg = _comodgan_pipeline(pkg, dev)
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(52)
    samples = 2
    sizes = [(96, 80), (70, 131), (97, 83)]
    holes = [(slice(30, 50), slice(20, 45)), (slice(50, 70), slice(100, 131)), (slice(20, 71), slice(25, 55))]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m, hole in zip(masks, holes):
        m[hole] = 0
    d_img, d_mask = _device_items(images, masks, dev)
    z = torch.from_numpy(pkg.synth.make_latent(3 * samples, cfg.z_dim, 52).reshape(3, samples, cfg.z_dim)).to(dev)
    items, scratch, bbox, x = _pre(lib, d_img, d_mask, dev, stream)
    with torch.no_grad():
        y = pipe.model.forward_samples(x, z, noise_mode="const").reshape(3 * samples, 3, RES, RES).contiguous()
    want = _post_on_copies(lib, d_img, d_mask, scratch, bbox, y, samples, pipe._gauss, stream)
    outs, boxes = pipe.forward_samples(d_img, d_mask, z, noise_mode="const", return_bbox=True)
    assert torch.equal(boxes, bbox)
    assert lib.backend() == "hip:gfx950"
    for i in range(3):
        assert outs[i].shape == (samples, 3) + sizes[i] and outs[i].dtype == torch.uint8
        assert torch.equal(d_img[i].cpu(), torch.from_numpy(images[i])[None]) and torch.equal(d_mask[i].cpu(), torch.from_numpy(masks[i])[None, None])
        for s in range(samples):
            assert torch.equal(outs[i][s], want[i][s]), f"item {i}, sample {s}"
        x0, x1, y0, y1 = boxes[i].tolist()
        a, b = outs[i][0].clone(), outs[i][1].clone()
        assert not torch.equal(a[(slice(None),) + holes[i]], b[(slice(None),) + holes[i]])     # different z: different completions
        a[:, y0:y1, x0:x1] = 0
        b[:, y0:y1, x0:x1] = 0
        assert torch.equal(a, b)                                          # and the same image outside the box
    # z drawn by the call: S from `samples`, chunks of max_rows // S images
    drawn = pipe.forward_samples(d_img, d_mask, samples=2, max_rows=2, noise_mode="const")
    assert [tuple(o.shape) for o in drawn] == [(2, 3) + s for s in sizes]


@pytest.mark.parametrize("max_rows", [2, 32])
def test_migan_gives_what_forward_batch_gives(pkg, max_rows):
    """a model without forward_samples: one completion, forward_batch's chunks (max_rows=2: 2 + 2 + a lone chunk padded to batch 2)"""
    dev = torch.device("cuda:0")
    pipe = _migan_pipeline(pkg, dev)
    images, masks = five_items(np.random.default_rng(21))
    d_img, d_mask = _device_items(images, masks, dev)
    want, want_boxes = pipe.forward_batch([a.clone() for a in d_img], d_mask, max_batch=max_rows, return_bbox=True)
    outs, boxes = pipe.forward_samples(d_img, d_mask, max_rows=max_rows, return_bbox=True)
    assert torch.equal(boxes, want_boxes)
    for i in range(5):
        assert outs[i].shape == (1,) + tuple(want[i].shape[1:])
        assert torch.equal(outs[i][0], want[i][0]), f"item {i}"
        assert torch.equal(d_img[i].cpu(), torch.from_numpy(images[i])[None]), f"source image {i} was written"
        assert i == 2 or not torch.equal(outs[i][0], d_img[i][0])         # (only the all-255 item may stay as it is)


def test_python_errors(pkg):
    dev = torch.device("cuda:0")
    pipe = _migan_pipeline(pkg, dev)
    img, mask = torch.zeros((1, 3, 64, 64), dtype=torch.uint8), torch.zeros((1, 1, 64, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="no forward_samples"):
        pipe.forward_samples([img.to(dev)], [mask.to(dev)], torch.zeros(1, 2, 512, device=dev))     # z for a model that takes none
    with pytest.raises(ValueError, match="no forward_samples"):
        pipe.forward_samples([img.to(dev)], [mask.to(dev)], samples=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_samples([img], [mask])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_samples([img.to(dev)], [mask])
    cpipe, cfg = _comodgan_pipeline(pkg, dev)
    with pytest.raises(ValueError, match="max_rows"):
        cpipe.forward_samples([img.to(dev)], [mask.to(dev)], torch.zeros(1, 3, cfg.z_dim, device=dev), max_rows=2)   # S > max_rows
    with pytest.raises(ValueError, match=r"\[1, S, z_dim\]"):
        cpipe.forward_samples([img.to(dev)], [mask.to(dev)], torch.zeros(2, 3, cfg.z_dim, device=dev))             # z of the wrong N
    with pytest.raises(ValueError, match="samples"):
        cpipe.forward_samples([img.to(dev)], [mask.to(dev)])                                                        # neither z nor samples
