"""MIGAN_Pipeline.forward_batch on the MI355X: N images of different sizes around one generator forward, the boxes kept on the
device (migan_pipeline_batch_pre / _post).  Per image it must give what MIGAN_Pipeline.forward gives: the post-processing byte for
byte (same y), the whole pipeline within the caps tests/test_gpu_pipeline.py states for the single-image path (a batched generator
forward has the same measured error against the reference as the batch-1 forward, README: 6.9e-5 against 5.7e-5)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests.pipeline_batch_case import five_items

pytestmark = pytest.mark.gpu
CASES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "pipeline_*.npz")))


def _pipeline(pkg, res, seed, padding, dev):
    sd = pkg.synth.make_state_dict(res, seed=seed, regime="export")
    m = pkg.Generator(resolution=res)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, res, padding=padding, device=dev)


def _five(dev):
    images, masks = five_items(np.random.default_rng(21))
    return images, masks, [torch.from_numpy(a)[None].to(dev) for a in images], [torch.from_numpy(m)[None, None].to(dev) for m in masks]


def test_postprocessing_is_exact_on_the_gpu(pkg):
    """x from pipeline_batch_pre, y = model(x), then the EXISTING pipeline_post per image on a copy: forward_batch gives those bytes"""
    dev = torch.device("cuda:0")
    res, padding = 64, 8
    pipe = _pipeline(pkg, res, 1, padding, dev)
    images, masks, d_img, d_mask = _five(dev)
    want_boxes = [po.masked_bbox(m, res, padding) for m in masks]
    lib = pkg.load_library()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    items = [(a.data_ptr(), m.data_ptr(), a.shape[2], a.shape[3], m.shape[2], m.shape[3]) for a, m in zip(d_img, d_mask)]
    scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=dev)
    bbox = torch.empty((5, 4), dtype=torch.int32, device=dev)
    x = torch.empty((5, 4, res, res), dtype=torch.float32, device=dev)
    lib.pipeline_batch_pre(items, res, padding, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), stream)
    with torch.no_grad():
        y = pipe.model(x).contiguous()
    assert bbox.cpu().tolist() == [list(b) for b in want_boxes]
    want = []
    for i in range(5):
        c = d_img[i].clone()
        h, w = c.shape[2:]
        s1 = torch.empty(lib.pipeline_scratch_bytes(h, w), dtype=torch.uint8, device=dev)
        lib.pipeline_post(c.data_ptr(), d_mask[i].data_ptr(), h, w, want_boxes[i], res, y[i:i + 1].contiguous().data_ptr(), s1.data_ptr(),
                          gauss25=pipe._gauss, stream=stream)
        want.append(c)
    out, boxes = pipe.forward_batch(d_img, d_mask, return_bbox=True)
    assert boxes.dtype == torch.int32 and boxes.is_cuda and boxes.cpu().tolist() == [list(b) for b in want_boxes]
    for i in range(5):
        assert torch.equal(out[i], want[i]), f"item {i}"
        assert i == 2 or not torch.equal(out[i].cpu(), torch.from_numpy(images[i])[None])      # (only the all-255 item may stay as it is)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[9:-4] for p in CASES])
def test_goldens_within_the_caps_of_the_single_image_path(pkg, path):
    g = np.load(path)
    res, seed, padding = int(g["resolution"]), int(g["seed"]), int(g["padding"])
    dev = torch.device("cuda:0")
    pipe = _pipeline(pkg, res, seed, padding, dev)
    rng = np.random.default_rng(31)
    other = torch.from_numpy(rng.integers(0, 256, (3, 200, 150), dtype=np.uint8)).to(dev)            # (3, H, W) form
    other_mask = torch.full((200, 150), 255, dtype=torch.uint8, device=dev)                           # (h, w) form
    other_mask[60:140, 30:100] = 0
    images = [torch.from_numpy(np.array(g["image"], copy=True))[None].to(dev), other, torch.from_numpy(np.array(g["image"], copy=True))[None].to(dev)]
    masks = [torch.from_numpy(np.array(g["mask"], copy=True))[None].to(dev), other_mask, torch.from_numpy(np.array(g["mask"], copy=True))[None].to(dev)]
    out, boxes = pipe.forward_batch(images, masks, return_bbox=True)
    assert boxes[0].cpu().tolist() == [int(v) for v in g["bbox"]] == boxes[2].cpu().tolist()
    assert torch.equal(out[0], out[2])                                  # batch invariance
    got = out[0][0].cpu().numpy()
    diff = np.abs(got.astype(np.int32) - g["result"].astype(np.int32))
    print(f"{os.path.basename(path)}: max diff {diff.max()}, {(diff > 0).mean():.4%} of the result bytes one step off")
    assert diff.max() <= 1, f"max diff {diff.max()}"
    assert (diff > 0).mean() <= 0.02, f"{(diff > 0).mean():.3%} of the result bytes are one step off"
    x0, x1, y0, y1 = [int(v) for v in g["bbox"]]
    m = torch.from_numpy(g["mask"][0, y0:y1, x0:x1].astype(np.float32))[None, None]
    far = (torch.nn.functional.max_pool2d(255 - m, 7, stride=1, padding=3) == 0)[0, 0].numpy()
    np.testing.assert_array_equal(got[:, y0:y1, x0:x1][:, far], g["image"][:, y0:y1, x0:x1][:, far])
    outside = np.ones(g["mask"].shape[1:], dtype=bool)
    outside[y0:y1, x0:x1] = False
    np.testing.assert_array_equal(got[:, outside], g["image"][:, outside])


def test_in_place_same_objects_and_close_to_forward(pkg):
    dev = torch.device("cuda:0")
    pipe = _pipeline(pkg, 64, 1, 8, dev)
    images, _, d_img, d_mask = _five(dev)
    single = [pipe(a.clone(), m) for a, m in zip(d_img, d_mask)]
    ptrs = [a.data_ptr() for a in d_img]
    out = pipe.forward_batch(d_img, d_mask)
    assert isinstance(out, list) and [a.data_ptr() for a in out] == ptrs and all(a is b for a, b in zip(out, d_img))
    for i in range(5):
        # the batch-1 generator of forward differs from the batched one by fp32 rounding only: at most one uint8 step
        d = (out[i].to(torch.int32) - single[i].to(torch.int32)).abs()
        assert int(d.max()) <= 1, f"item {i}: {int(d.max())}"
    # a list of ONE image runs the generator at batch 1, like forward: the same bytes
    one = pipe.forward_batch([torch.from_numpy(images[0])[None].to(dev)], [d_mask[0]])
    assert torch.equal(one[0], single[0])


def test_max_batch_does_not_change_the_result(pkg):
    dev = torch.device("cuda:0")
    pipe = _pipeline(pkg, 64, 1, 8, dev)
    _, _, a_img, d_mask = _five(dev)
    b_img = [a.clone() for a in a_img]
    a, abox = pipe.forward_batch(a_img, d_mask, max_batch=2, return_bbox=True)         # 2 + 2 + 1
    b, bbox = pipe.forward_batch(b_img, d_mask, max_batch=32, return_bbox=True)
    assert torch.equal(abox, bbox)
    for i in range(5):
        assert torch.equal(a[i], b[i]), f"item {i}"


def test_forward_batch_rejects_cpu_tensors(pkg):
    dev = torch.device("cuda:0")
    pipe = _pipeline(pkg, 64, 1, 8, dev)
    img, mask = torch.zeros((1, 3, 64, 64), dtype=torch.uint8), torch.zeros((1, 1, 64, 64), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_batch([img], [mask])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_batch([img.to(dev)], [mask])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_batch([img], [mask.to(dev)])
    with pytest.raises(RuntimeError, match="must be uint8"):
        pipe.forward_batch([img.to(dev).float()], [mask.to(dev)])
    with pytest.raises(RuntimeError, match="expected a contiguous image"):
        pipe.forward_batch([img.to(dev)[0, 0]], [mask.to(dev)])
