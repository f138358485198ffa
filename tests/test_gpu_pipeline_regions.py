"""One crop per hole region on the MI355X: migan_pipeline_regions_find / _pre / _post through ctypes on device buffers against the
scipy / pipeline oracle of tests/pipeline_regions_case.py (the cases of tests/test_emu_pipeline_regions.py), and
MIGAN_Pipeline.forward_regions around a small MI-GAN generator.  Every comparison is byte for byte: label map, counts, boxes, x and
image bytes."""
import numpy as np
import pytest
import torch

from tests import pipeline_regions_case as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bufs():
    return rc.Buffers(to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV), ptr=lambda t: t.data_ptr(),
                      to_np=lambda t: t.cpu().numpy(), stream=int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


def _pipeline(pkg):
    sd = pkg.synth.make_state_dict(64, seed=1, regime="export")
    m = pkg.Generator(resolution=64)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, rc.RES, padding=rc.PADDING, device=DEV)


def _upload(case):
    return ([torch.from_numpy(a.copy())[None].to(DEV) for a in case["images"]],
            [torch.from_numpy(m.copy())[None, None].to(DEV) for m in case["masks"]])


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_case_against_the_oracle(pkg, name):
    lib = pkg.load_library()
    rc.run_case(lib, _bufs(), rc.CASES[name]())
    assert lib.backend() == "hip:gfx950"


def test_fallback_rows_give_the_batch_pipelines_bytes(pkg):
    """rule6: the rows that are not split hold migan_pipeline_batch_post's bytes for the same y row"""
    lib, bufs = pkg.load_library(), _bufs()
    case = rc.CASES["rule6"]()
    out = rc.run_case(lib, bufs, case)
    assert list(out["count"]) == [9, 1, 0, 2] and all(label == 0 for _, label, _ in out["flat"])
    keep = [0, 1, 3]
    images = [bufs.to_dev(case["images"][i]) for i in keep]
    masks = [bufs.to_dev(case["masks"][i]) for i in keep]
    items = [(a.data_ptr(), m.data_ptr(), a.shape[1], a.shape[2], m.shape[0], m.shape[1]) for a, m in zip(images, masks)]
    scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=DEV)
    bbox = torch.empty((3, 4), dtype=torch.int32, device=DEV)
    x = torch.empty((3, 4, rc.RES, rc.RES), dtype=torch.float32, device=DEV)
    y = bufs.to_dev(out["y"])
    lib.pipeline_batch_pre(items, rc.RES, rc.PADDING, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), bufs.stream)
    lib.pipeline_batch_post(items, rc.RES, y.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), gauss25=rc.GAUSS, stream=bufs.stream)
    np.testing.assert_array_equal(x.cpu().numpy(), out["x"])
    for j, i in enumerate(keep):
        np.testing.assert_array_equal(images[j].cpu().numpy(), out["images"][i])


def test_more_items_than_one_launch_of_find_carries(pkg):
    """17 items, kRegionsFindMax = 16: one call gives the bytes of 17 calls with one item each"""
    rc.check_find_splits_like_single_calls(pkg.load_library(), _bufs())


def test_twice_the_same(pkg):
    lib = pkg.load_library()
    case = rc.CASES["serpentine"]()
    a, b = rc.run_case(lib, _bufs(), case), rc.run_case(lib, _bufs(), case)
    np.testing.assert_array_equal(a["labels"][0], b["labels"][0])
    np.testing.assert_array_equal(a["boxes"], b["boxes"])
    np.testing.assert_array_equal(a["images"][0], b["images"][0])


def test_forward_regions_unsplit_images_are_forward_batch(pkg):
    """images that are not split (nine regions with max_regions = 8; one region; no hole; two regions inside an R x R box) get
    forward_batch's bytes, in a list and alone"""
    pipe = _pipeline(pkg)
    case = rc.CASES["rule6"]()
    imgs, masks = _upload(case)
    want, _ = _upload(case)
    pipe.forward_batch(want, masks)
    got, used, labels = pipe.forward_regions(imgs, masks, gap=3, return_regions=True)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert not torch.equal(got[1], torch.from_numpy(case["images"][1])[None].to(DEV))            # something was completed
    assert [u.shape[0] for u in used] == [1, 1, 0, 1]
    assert [u.tolist() for u in used] == [[list(f["single"])] if f["hole"] else [] for f in case["found"]]
    one_a, _ = _upload(case)
    one_b, _ = _upload(case)
    assert torch.equal(pipe.forward_regions(one_a[1:2], masks[1:2])[0], pipe.forward_batch(one_b[1:2], masks[1:2])[0])


def test_forward_regions_three_blobs(pkg):
    """three regions -> three rows: the generator run separately on the rows' x, that y through the oracle's post-processing, the
    same bytes; max_batch = 2 (an image's rows straddle chunks, the lone last chunk runs at batch 2) gives them too"""
    pipe, lib, bufs = _pipeline(pkg), pkg.load_library(), _bufs()
    case = rc.CASES["three_blobs"]()
    found = case["found"][0]
    imgs, masks = _upload(case)
    got, used, labels = pipe.forward_regions(imgs, masks, gap=case["gap"], return_regions=True)
    assert used[0].tolist() == [list(b) for b in found["boxes"]]
    np.testing.assert_array_equal(labels[0].cpu().numpy(), found["labels"])
    orig = bufs.to_dev(case["images"][0])
    rows = [(orig.data_ptr(), masks[0].data_ptr(), labels[0].data_ptr(), 157, 203, r + 1, b) for r, b in enumerate(found["boxes"])]
    x = torch.empty((3, 4, rc.RES, rc.RES), dtype=torch.float32, device=DEV)
    lib.pipeline_regions_pre(rows, rc.RES, x.data_ptr(), bufs.stream)
    y = pipe.model(x).contiguous().cpu().numpy()
    want = rc.oracle_post(case["images"][0], case["full"][0], found["labels"], rc.rows_of(found), y)
    np.testing.assert_array_equal(got[0][0].cpu().numpy(), want)
    again, _ = _upload(case)
    pipe.forward_regions(again, masks, gap=case["gap"], max_batch=2)
    assert torch.equal(again[0], got[0])
    twice, _ = _upload(case)
    pipe.forward_regions(twice, masks, gap=case["gap"])
    assert torch.equal(twice[0], got[0])


def test_forward_regions_rows_straddle_chunks(pkg):
    """many_rows: 40 rows in chunks of 32, the second image's rows in both; chunks of 7 give the same bytes"""
    pipe = _pipeline(pkg)
    case = rc.CASES["many_rows"]()
    imgs, masks = _upload(case)
    _, used, labels = pipe.forward_regions(imgs, masks, gap=2, max_regions=32, return_regions=True)
    assert [u.shape[0] for u in used] == [20, 20]
    other, _ = _upload(case)
    pipe.forward_regions(other, masks, gap=2, max_regions=32, max_batch=7)
    for i in range(2):
        assert torch.equal(other[i], imgs[i])
        lab = labels[i].cpu().numpy()
        np.testing.assert_array_equal(lab, case["found"][i]["labels"])
        got = imgs[i][0].cpu().numpy()
        np.testing.assert_array_equal(got[:, lab == 0], case["images"][i][:, lab == 0])
        assert (got[:, case["full"][i] == 0] != case["images"][i][:, case["full"][i] == 0]).any()


def test_forward_regions_checks_its_arguments(pkg):
    pipe = _pipeline(pkg)
    case = rc.CASES["three_blobs"]()
    imgs, masks = _upload(case)
    with pytest.raises(ValueError):
        pipe.forward_regions(imgs, masks, gap=1)
    with pytest.raises(ValueError):
        pipe.forward_regions(imgs, masks, gap=65)
    with pytest.raises(ValueError):
        pipe.forward_regions(imgs, masks, max_regions=0)
    with pytest.raises(RuntimeError):
        pipe.forward_regions(imgs, masks + masks)
    with pytest.raises(RuntimeError):
        pipe.forward_regions([], [])
    with pytest.raises(RuntimeError):
        pipe.forward_regions([imgs[0].cpu()], masks)
    with pytest.raises(RuntimeError):
        pipe.forward_regions(imgs, [masks[0].cpu()])
    with pytest.raises(RuntimeError):
        pipe.forward_regions(imgs, masks, max_batch=0)
    with pytest.raises(RuntimeError):
        pipe.forward_regions([imgs[0].float()], masks)
    assert torch.equal(imgs[0], torch.from_numpy(case["images"][0])[None].to(DEV))
    assert pipe.forward_regions(imgs, masks)[0] is imgs[0]                        # gap=None: max(2, padding // 4) = 2
