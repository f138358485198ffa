"""The completions of every photo as box-sized patches on the MI355X: migan_pipeline_batch_post_patches through ctypes on device
buffers against migan_pipeline_batch_post_samples on the device, and MIGAN_Pipeline.forward_patches around a small Co-Mod-GAN and
around the MI-GAN generator against forward_samples.  Every comparison is byte for byte."""
import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests.pipeline_patches_case import (BAD_BOXES, FILL, GUARD, TILE_H, TILE_W, case_clipped, case_five, case_smallest, case_three,
                                         case_two_launches, patch_bytes, random_y)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class OnDevice:
    """a case uploaded and through pipeline_batch_pre: items, scratch, bbox [n, 4] (device), y [n * S, 3, R, R] seeded random"""

    def __init__(self, lib, case, rng):
        self.lib, self.case = lib, case
        self.res, self.samples = case["res"], case["samples"]
        self.stream = int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        self.images = [torch.from_numpy(a)[None].to(DEV) for a in case["images"]]
        self.masks = [torch.from_numpy(m)[None, None].to(DEV) for m in case["masks"]]
        self.items = [(a.data_ptr(), m.data_ptr(), a.shape[-2], a.shape[-1], m.shape[-2], m.shape[-1]) for a, m in zip(self.images, self.masks)]
        n = len(self.items)
        self.scratch = torch.empty(lib.pipeline_batch_scratch_bytes(self.items), dtype=torch.uint8, device=DEV)
        self.bbox = torch.empty((n, 4), dtype=torch.int32, device=DEV)
        self.x = torch.empty((n, 4, self.res, self.res), dtype=torch.float32, device=DEV)
        lib.pipeline_batch_pre(self.items, self.res, case["padding"], self.x.data_ptr(), self.bbox.data_ptr(), self.scratch.data_ptr(), self.stream)
        self.y = torch.from_numpy(random_y(rng, n, self.samples, self.res)).to(DEV)

    def boxes(self):
        return self.bbox.cpu().tolist()

    def yardstick(self, gauss=None):
        """pipeline_batch_post_samples -> [S, 3, H_i, W_i] per item"""
        outs = [torch.full((self.samples, 3) + tuple(a.shape[-2:]), FILL, dtype=torch.uint8, device=DEV) for a in self.images]
        self.lib.pipeline_batch_post_samples(self.items, self.samples, self.res, self.y.data_ptr(), self.bbox.data_ptr(), self.scratch.data_ptr(),
                                             [o.data_ptr() for o in outs], gauss25=gauss, stream=self.stream)
        return outs

    def patches(self, sizes, capacities=None, gauss=None):
        """pipeline_batch_post_patches -> flat destinations of sizes[i] + GUARD bytes, FILL before the call"""
        bufs = [torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=DEV) for n in sizes]
        self.lib.pipeline_batch_post_patches(self.items, self.samples, self.res, self.y.data_ptr(), self.bbox.data_ptr(), self.scratch.data_ptr(),
                                             [b.data_ptr() for b in bufs], sizes if capacities is None else capacities, gauss25=gauss,
                                             stream=self.stream)
        return bufs

    def assert_patch(self, buf, whole, box, what):
        x0, x1, y0, y1 = box
        n = patch_bytes(box, self.samples)
        want = whole[:, :, y0:y1, x0:x1].contiguous()
        assert np.array_equal(buf[:n].view(want.shape).cpu().numpy(), want.cpu().numpy()), what
        assert bool((buf[n:] == FILL).all()), f"{what}: bytes behind the patch were written"

    def assert_inputs_untouched(self, boxes, x):
        for i, (a, m) in enumerate(zip(self.images, self.masks)):
            assert np.array_equal(a[0].cpu().numpy(), self.case["images"][i]), f"image {i} was written"
            assert np.array_equal(m[0, 0].cpu().numpy(), self.case["masks"][i]), f"mask {i} was written"
        assert self.boxes() == boxes and torch.equal(self.x, x)


@pytest.mark.parametrize("make", [case_five, case_smallest, case_two_launches, case_clipped], ids=lambda f: f.__name__[5:])
def test_operator_against_the_samples_form(pkg, make):
    lib = pkg.load_library()
    rng = np.random.default_rng(71)
    d = OnDevice(lib, make(rng), rng)
    boxes, x = d.boxes(), d.x.clone()
    assert boxes == [list(po.masked_bbox(m, d.res, d.case["padding"])) for m in d.case["masks"]]
    if make is case_five:                              # a crop off the tile grid in both directions, several tiles each way
        cw, ch = boxes[4][1] - boxes[4][0], boxes[4][3] - boxes[4][2]
        assert cw % TILE_W != 0 and ch % TILE_H != 0 and cw > TILE_W and ch > TILE_H
    if make is case_clipped:
        assert boxes == [[0, 34, 0, 27], [0, 25, 16, 45]]
    for gauss in (None, po.gaussian_kernel().flatten().tolist()) if make is case_five else (None,):
        want = d.yardstick(gauss)
        bufs = d.patches([patch_bytes(b, d.samples) for b in boxes], gauss=gauss)
        for i, box in enumerate(boxes):
            d.assert_patch(bufs[i], want[i], box, f"item {i}")
    d.assert_inputs_untouched(boxes, x)


def test_operator_skips_a_box_that_does_not_fit(pkg):
    lib = pkg.load_library()
    rng = np.random.default_rng(72)
    d = OnDevice(lib, case_three(rng), rng)
    for i, row in BAD_BOXES.items():
        d.bbox[i] = torch.tensor(row, dtype=torch.int32)
    boxes, x = d.boxes(), d.x.clone()
    sizes = [d.samples * a.numel() for a in d.images[:2]] + [patch_bytes(boxes[2], d.samples)]
    bufs = d.patches(sizes)
    want = d.yardstick()
    assert bool((bufs[0] == FILL).all()) and bool((bufs[1] == FILL).all())
    d.assert_patch(bufs[2], want[2], boxes[2], "item 2")
    d.assert_inputs_untouched(boxes, x)


def test_operator_skips_an_item_whose_capacity_is_one_byte_short(pkg):
    lib = pkg.load_library()
    rng = np.random.default_rng(73)
    d = OnDevice(lib, case_three(rng), rng)
    boxes, x = d.boxes(), d.x.clone()
    sizes = [patch_bytes(b, d.samples) for b in boxes]
    bufs = d.patches(sizes, capacities=[sizes[0], sizes[1] - 1, sizes[2]])
    want = d.yardstick()
    assert bool((bufs[1] == FILL).all())
    for i in (0, 2):
        d.assert_patch(bufs[i], want[i], boxes[i], f"item {i}")
    d.assert_inputs_untouched(boxes, x)


def _comodgan_pipeline(pkg):
    """the smoke() configuration"""
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    cfg = cs.Config(resolution=32, ch_base=4096, ch_max=128, num_ws=cs.default_num_ws(32))
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=32, **kw), cm.Synthesis(resolution=32, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 2)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, 32, padding=8, device=DEV), cfg


def _migan_pipeline(pkg):
    sd = pkg.synth.make_state_dict(64, seed=1, regime="export")
    m = pkg.Generator(resolution=64)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, 64, padding=8, device=DEV)


def _three_photos(rng):
    sizes = [(90, 120), (70, 51), (33, 97)]
    holes = [(slice(30, 61), slice(40, 75)), (slice(50, 70), slice(31, 51)), (slice(5, 20), slice(10, 30))]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m, hole in zip(masks, holes):
        m[hole] = 0
    return images, masks


def _check_against_forward_samples(images, masks, d_img, d_mask, patches, boxes, wholes, whole_boxes, samples):
    assert boxes.dtype == torch.int32 and boxes.device.type == "cpu" and tuple(boxes.shape) == (len(images), 4)
    assert torch.equal(boxes, whole_boxes.cpu())
    for i, (x0, x1, y0, y1) in enumerate(boxes.tolist()):
        assert patches[i].dtype == torch.uint8 and patches[i].is_cuda and tuple(patches[i].shape) == (samples, 3, y1 - y0, x1 - x0)
        assert torch.equal(patches[i], wholes[i][:, :, y0:y1, x0:x1]), f"image {i}"
        assert np.array_equal(d_img[i][0].cpu().numpy(), images[i]), f"image {i} was written"
        assert np.array_equal(d_mask[i][0, 0].cpu().numpy(), masks[i]), f"mask {i} was written"


def test_forward_patches_comodgan(pkg):
    """N = 3 photos of different sizes, S = 3, two chunks (max_rows = 6: two photos, then one)"""
    pipe, cfg = _comodgan_pipeline(pkg)
    rng = np.random.default_rng(74)
    images, masks = _three_photos(rng)
    d_img = [torch.from_numpy(a)[None].to(DEV) for a in images]
    d_mask = [torch.from_numpy(m)[None, None].to(DEV) for m in masks]
    z = torch.from_numpy(pkg.synth.make_latent(9, cfg.z_dim, 74).reshape(3, 3, cfg.z_dim)).to(DEV)
    for max_rows in (32, 6):
        wholes, whole_boxes = pipe.forward_samples(d_img, d_mask, z, max_rows=max_rows, return_bbox=True, noise_mode="const")
        patches, boxes = pipe.forward_patches(d_img, d_mask, z, max_rows=max_rows, noise_mode="const")
        _check_against_forward_samples(images, masks, d_img, d_mask, patches, boxes, wholes, whole_boxes, 3)
        assert boxes.tolist() == [list(po.masked_bbox(m, 32, 8)) for m in masks]
        assert not torch.equal(patches[0][0], patches[0][1])              # different z: different completions
    assert pkg.load_library().backend() == "hip:gfx950"


def test_forward_patches_migan(pkg):
    """a model without forward_samples: one completion; N = 3 at max_rows = 2 leaves a lone last chunk, which runs padded to batch 2"""
    pipe = _migan_pipeline(pkg)
    rng = np.random.default_rng(75)
    images, masks = _three_photos(rng)
    d_img = [torch.from_numpy(a)[None].to(DEV) for a in images]
    d_mask = [torch.from_numpy(m)[None, None].to(DEV) for m in masks]
    wholes, whole_boxes = pipe.forward_samples(d_img, d_mask, max_rows=2, return_bbox=True)
    patches, boxes = pipe.forward_patches(d_img, d_mask, max_rows=2)
    _check_against_forward_samples(images, masks, d_img, d_mask, patches, boxes, wholes, whole_boxes, 1)
    x0, x1, y0, y1 = boxes[2].tolist()
    assert not torch.equal(patches[2][0], d_img[2][0][:, y0:y1, x0:x1])   # the lone chunk's photo was completed


def test_forward_patches_errors(pkg):
    pipe = _migan_pipeline(pkg)
    img = torch.zeros((1, 3, 64, 64), dtype=torch.uint8, device=DEV)
    mask = torch.zeros((1, 1, 64, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="no forward_samples"):
        pipe.forward_patches([img], [mask], torch.zeros(1, 2, 512, device=DEV))           # z for a model that takes none
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_patches([img.cpu()], [mask.cpu()])
    cpipe, cfg = _comodgan_pipeline(pkg)
    with pytest.raises(ValueError, match="max_rows"):
        cpipe.forward_patches([img], [mask], torch.zeros(1, 3, cfg.z_dim, device=DEV), max_rows=2)    # S > max_rows
