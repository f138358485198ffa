"""Crops at native size on the MI355X: migan_pipeline_native_pre / _post through ctypes on device buffers (the checks of
tests/pipeline_native_case.py, as tests/test_emu_pipeline_native.py runs them on the emulator), and MIGAN_Pipeline.forward_native
around a small MI-GAN generator: replayed call by call from what return_rows lists -- x by pipeline_native_pre, the generator's
forward_any_size on exactly those calls, the oracle's post-processing -- and held to forward_regions' bytes where the two must agree.
Every comparison is byte for byte."""
import numpy as np
import pytest
import torch

from oracle import migan_pipeline_oracle as po
from tests import pipeline_native_case as nc
from tests import pipeline_regions_case as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = nc.RES


def _bufs():
    return nc.Buffers(to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV), ptr=lambda t: t.data_ptr(),
                      to_np=lambda t: t.cpu().numpy(), stream=int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


@pytest.mark.parametrize("name", sorted(nc.CHECKS))
def test_kernels(pkg, name):
    lib = pkg.load_library()
    nc.CHECKS[name](lib, _bufs())
    assert lib.backend() == "hip:gfx950"


@pytest.fixture(scope="module")
def pipe(pkg):
    sd = pkg.synth.make_state_dict(R, seed=1, regime="export")
    m = pkg.Generator(resolution=R)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, R, padding=nc.PADDING, device=DEV)


def _upload(photos):
    return ([torch.from_numpy(img.copy())[None].to(DEV) for img, _ in photos], [torch.from_numpy(m.copy())[None, None].to(DEV) for _, m in photos])


def _window(pipe, mask):
    """the reference's box of all hole pixels, and what the window rule makes of it"""
    box = tuple(int(v) for v in po.masked_bbox(mask, R, nc.PADDING))
    return box, pipe.native_window(box, *mask.shape)


def _replay(pkg, pipe, photos, calls, labels=None):
    """the photos after the listed calls, each replayed on its own: x from the ORIGINAL photos by pipeline_native_pre, forward_any_size
    of that x, the oracle's post-processing of the crop with the part of y over it"""
    lib, bufs = pkg.load_library(), _bufs()
    labels = [None] * len(photos) if labels is None else labels
    scenes = [nc.Scene(bufs, img, m, lab) for (img, m), lab in zip(photos, labels)]
    out = [np.array(img, copy=True) for img, _ in photos]
    for hc, wc, rows in calls:
        x = nc.run_pre(lib, bufs, scenes, rows, hc, wc)
        y = pipe.model.forward_any_size(torch.from_numpy(x).to(DEV)).cpu().numpy()
        for r, (i, label, box) in enumerate(rows):
            nc.oracle_post(photos[i][0], photos[i][1], labels[i], [(label, box)], y[r:r + 1], out=out[i])
    return out


def test_forward_native_replay(pkg, pipe):
    """two photos of different sizes, two different non-square windows: two calls in ascending window order, replayed; a second run
    gives the same bytes"""
    photos = [nc.photo(41, 96, 203, [(30, 60, 40, 150)]), nc.photo(42, 157, 80, [(30, 120, 20, 50)])]
    wins = [_window(pipe, m)[1] for _, m in photos]
    assert [hw for _, hw in wins] == [(96, 128), (112, 80)]
    imgs, masks = _upload(photos)
    got, calls = pipe.forward_native(imgs, masks, return_rows=True)
    assert calls == [(96, 128, [(0, 0, wins[0][0])]), (112, 80, [(1, 0, wins[1][0])])]
    for g, want, (img, _) in zip(got, _replay(pkg, pipe, photos, calls), photos):
        np.testing.assert_array_equal(g[0].cpu().numpy(), want)
        assert (want != img).any()
    again, _ = _upload(photos)
    pipe.forward_native(again, masks)
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_forward_native_windows_of_one_size_share_a_call(pkg, pipe):
    photos = [nc.photo(43, 157, 203, [(50, 120, 60, 130)]), nc.photo(44, 140, 150, [(30, 95, 40, 110)])]
    wins = [_window(pipe, m)[1] for _, m in photos]
    assert [hw for _, hw in wins] == [(96, 96), (96, 96)]
    imgs, masks = _upload(photos)
    got, calls = pipe.forward_native(imgs, masks, return_rows=True)
    assert calls == [(96, 96, [(0, 0, wins[0][0]), (1, 0, wins[1][0])])]
    for g, want in zip(got, _replay(pkg, pipe, photos, calls)):
        np.testing.assert_array_equal(g[0].cpu().numpy(), want)
    # max_batch = 2: max(1, 2 * 64 * 64 // (96 * 96)) = 1 row per call
    _, calls = pipe.forward_native(*_upload(photos), max_batch=2, return_rows=True)
    assert [(h, w, len(rows)) for h, w, rows in calls] == [(96, 96, 1), (96, 96, 1)]


def test_forward_native_r_by_r_windows_are_forward_regions(pkg, pipe):
    """three photos with small holes: every window is R x R and inside its photo; chunks of two, the lone last one at batch 2"""
    photos = [nc.photo(45, 100, 120, [(40, 60, 50, 70)]), nc.photo(46, 157, 203, [(5, 25, 170, 200)]), nc.photo(47, 90, 90, [(60, 85, 10, 30)])]
    for _, m in photos:
        box, (win, hw) = _window(pipe, m)
        assert hw == (R, R) and win == box
    imgs, masks = _upload(photos)
    want, _ = _upload(photos)
    pipe.forward_regions(want, masks, max_batch=2)
    got, calls = pipe.forward_native(imgs, masks, max_batch=2, return_rows=True)
    assert [(h, w, [i for i, _, _ in rows]) for h, w, rows in calls] == [(R, R, [0, 1]), (R, R, [2])]
    for g, w, (img, _) in zip(got, want, photos):
        assert torch.equal(g, w)
        assert not torch.equal(g[0].cpu(), torch.from_numpy(img))                   # something was completed


def test_forward_native_small_max_side_falls_back(pkg, pipe):
    photos = [nc.photo(43, 157, 203, [(50, 120, 60, 130)])]
    box, (_, hw) = _window(pipe, photos[0][1])
    assert hw == (96, 96)
    imgs, masks = _upload(photos)
    want, _ = _upload(photos)
    pipe.forward_regions(want, masks)
    got, calls = pipe.forward_native(imgs, masks, max_side=R, return_rows=True)
    assert calls == [(R, R, [(0, 0, box)])]
    assert torch.equal(got[0], want[0]) and not torch.equal(got[0][0].cpu(), torch.from_numpy(photos[0][0]))
    # a fallback row between two R x R windows shares their calls, in row order
    three = [nc.photo(45, 100, 120, [(40, 60, 50, 70)]), photos[0], nc.photo(47, 90, 90, [(60, 85, 10, 30)])]
    imgs, masks = _upload(three)
    want, _ = _upload(three)
    pipe.forward_regions(want, masks)
    got, calls = pipe.forward_native(imgs, masks, max_side=R, return_rows=True)
    assert [(h, w, [i for i, _, _ in rows]) for h, w, rows in calls] == [(R, R, [0, 1, 2])] and calls[0][2][1] == (1, 0, box)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_forward_native_photo_smaller_than_the_window(pkg, pipe):
    photos = [nc.photo(48, 40, 50, [(10, 30, 20, 45)])]
    assert _window(pipe, photos[0][1]) == ((0, 50, 0, 40), ((0, 50, 0, 40), (48, 64)))
    imgs, masks = _upload(photos)
    got, calls = pipe.forward_native(imgs, masks, return_rows=True)
    assert calls == [(48, 64, [(0, 0, (0, 50, 0, 40))])]
    want = _replay(pkg, pipe, photos, calls)[0]
    np.testing.assert_array_equal(got[0][0].cpu().numpy(), want)
    assert (want != photos[0][0]).any()


def test_forward_native_regions(pkg, pipe):
    """one row per region.  three_blobs: three R x R windows, forward_regions' bytes.  Two large blobs: two 80 x 80 windows in one
    call, replayed with the oracle's label map; pixels with label 0 are untouched"""
    case = rc.CASES["three_blobs"]()
    found = case["found"][0]
    photos = [(case["images"][0], case["full"][0])]
    imgs, masks = _upload(photos)
    want, _ = _upload(photos)
    pipe.forward_regions(want, masks, gap=case["gap"])
    got, calls = pipe.forward_native(imgs, masks, gap=case["gap"], return_rows=True)
    assert calls == [(R, R, [(0, r + 1, b) for r, b in enumerate(found["boxes"])])]
    assert torch.equal(got[0], want[0])
    out = got[0][0].cpu().numpy()
    np.testing.assert_array_equal(out[:, found["labels"] == 0], case["images"][0][:, found["labels"] == 0])
    assert (out != case["images"][0]).any()

    photos = [nc.photo(49, 200, 260, [(20, 80, 20, 80), (120, 180, 170, 230)])]
    found = rc.oracle_find(photos[0][1], 2, 8)
    assert found["K"] == 2 and found["split"]
    wins = [pipe.native_window(b, 200, 260) for b in found["boxes"]]
    assert [hw for _, hw in wins] == [(80, 80), (80, 80)]
    imgs, masks = _upload(photos)
    got, calls = pipe.forward_native(imgs, masks, gap=2, return_rows=True)
    assert calls == [(80, 80, [(0, 1, wins[0][0]), (0, 2, wins[1][0])])]
    out = got[0][0].cpu().numpy()
    np.testing.assert_array_equal(out, _replay(pkg, pipe, photos, calls, labels=[found["labels"]])[0])
    np.testing.assert_array_equal(out[:, found["labels"] == 0], photos[0][0][:, found["labels"] == 0])
    for k in (1, 2):
        assert (out[:, found["labels"] == k] != photos[0][0][:, found["labels"] == k]).any()
    # max_regions = 1: one box per photo
    _, calls = pipe.forward_native(*_upload(photos), gap=2, max_regions=1, return_rows=True)
    assert len(calls) == 1 and [label for _, label, _ in calls[0][2]] == [0]


def test_forward_native_checks_its_arguments(pkg, pipe):
    photos = [nc.photo(43, 157, 203, [(50, 120, 60, 130)])]
    imgs, masks = _upload(photos)
    for bad in (dict(gap=1), dict(gap=65), dict(max_regions=0), dict(max_side=R - 1), dict(max_side=4097)):
        with pytest.raises(ValueError):
            pipe.forward_native(imgs, masks, **bad)
    with pytest.raises(RuntimeError):
        pipe.forward_native(imgs, masks + masks)
    with pytest.raises(RuntimeError):
        pipe.forward_native([], [])
    with pytest.raises(RuntimeError):
        pipe.forward_native([imgs[0].cpu()], masks)
    with pytest.raises(RuntimeError):
        pipe.forward_native(imgs, [masks[0].cpu()])
    with pytest.raises(RuntimeError):
        pipe.forward_native(imgs, masks, max_batch=0)
    with pytest.raises(RuntimeError):
        pipe.forward_native([imgs[0].float()], masks)

    class Plain(torch.nn.Module):                                                   # a model without forward_any_size
        def forward(self, x):
            return x[:, 1:]

    other = pkg.pipeline.MIGAN_Pipeline(Plain(), R, padding=nc.PADDING, device=DEV)
    with pytest.raises(RuntimeError, match="forward_any_size"):
        other.forward_native(imgs, masks)
    assert torch.equal(imgs[0][0].cpu(), torch.from_numpy(photos[0][0]))            # nothing was touched by any of them
    assert pipe.forward_native(imgs, masks, max_side=R)[0] is imgs[0] and pipe.forward_native(imgs, masks, max_side=4096)[0] is imgs[0]
