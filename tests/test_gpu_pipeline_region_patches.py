"""S completions per hole region as patches on the MI355X: migan_pipeline_regions_post_patches / _paste through ctypes on device
buffers against the oracle of tests/pipeline_region_patches_case.py (the cases of tests/test_emu_pipeline_region_patches.py), and
MIGAN_Pipeline.forward_region_patches / paste_patches around a small MI-GAN generator and a small Co-Mod-GAN.  Every comparison is
byte for byte."""
import numpy as np
import pytest
import torch

from tests import pipeline_region_patches_case as pc
from tests import pipeline_regions_case as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bufs():
    return pc.Buffers(to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV), ptr=lambda t: t.data_ptr(),
                      to_np=lambda t: t.cpu().numpy(), stream=int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


def _upload(images, masks):
    return ([torch.from_numpy(a.copy())[None].to(DEV) for a in images], [torch.from_numpy(m.copy())[None, None].to(DEV) for m in masks])


def _migan_pipeline(pkg):
    sd = pkg.synth.make_state_dict(64, seed=1, regime="export")
    m = pkg.Generator(resolution=64)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, rc.RES, padding=rc.PADDING, device=DEV)


def _comodgan_pipeline(pkg):
    """the smoke() configuration"""
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    cfg = cs.Config(resolution=32, ch_base=4096, ch_max=128, num_ws=cs.default_num_ws(32))
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=32, **kw), cm.Synthesis(resolution=32, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 2)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return pkg.pipeline.MIGAN_Pipeline(m, 32, padding=8, device=DEV), cfg


# ---- the operators on device buffers ---------------------------------------------------------------------------------------------------
# many_rows (40 rows) runs at S = 2, every other case at S = 3, as under the emulator
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_against_the_oracle(pkg, name):
    lib = pkg.load_library()
    out = pc.check_case(lib, _bufs(), name, 2 if name == "many_rows" else 3)
    if name == "many_rows":
        assert len(out["prep"].flat) == 40
    assert lib.backend() == "hip:gfx950"


@pytest.mark.parametrize("name", ["three_blobs", "borders", "rule6"])
def test_one_sample(pkg, name):
    pc.check_case(pkg.load_library(), _bufs(), name, 1)


def test_twice_the_same_and_every_byte_written(pkg):
    """two calls, into destinations of different fills: the same bytes inside the capacity, neither guard touched"""
    lib, bufs = pkg.load_library(), _bufs()
    y, _ = pc.reference("overlapping_crops", 3)
    prep = pc.Prepared(lib, bufs, pc.CASES["overlapping_crops"]())
    y_dev = bufs.to_dev(y)
    a, b = pc.post_patches(prep, y_dev, 3, fill=pc.FILL), pc.post_patches(prep, y_dev, 3, fill=0x5A)
    for r, (_, _, box) in enumerate(prep.flat):
        n = pc.patch_bytes(box, 3)
        assert torch.equal(a[r][:n], b[r][:n]), f"row {r}"
        assert bool((a[r][n:] == pc.FILL).all()) and bool((b[r][n:] == 0x5A).all())


def test_a_tile_without_a_pixel_of_its_label_is_still_written(pkg):
    r, (ty0, tx0) = pc.empty_tile("overlapping_crops")
    out = pc.check_case(pkg.load_library(), _bufs(), "overlapping_crops", 3)
    i, _, (x0, x1, y0, y1) = out["prep"].flat[r]
    photo = out["prep"].case["images"][i][:, y0:y1, x0:x1]
    for s in range(3):
        np.testing.assert_array_equal(out["patches"][r][s][:, ty0:ty0 + pc.TILE_H, tx0:tx0 + pc.TILE_W],
                                      photo[:, ty0:ty0 + pc.TILE_H, tx0:tx0 + pc.TILE_W])
    sel = out["prep"].labels[0][y0:y1, x0:x1] == 2                   # and patch 1 holds the photo where region 2 lies
    assert r == 0 and sel.any()
    np.testing.assert_array_equal(out["patches"][0][1][:, sel], photo[:, sel])


def test_label_0_rows_give_the_batch_patches_bytes(pkg):
    """rule6: the rows that are not split hold migan_pipeline_batch_post_patches' bytes for the same y"""
    lib, bufs = pkg.load_library(), _bufs()
    out = pc.check_case(lib, bufs, "rule6", 3)
    case, prep = out["prep"].case, out["prep"]
    keep = [i for i, _, _ in prep.flat]
    assert keep == [0, 1, 3] and all(label == 0 for _, label, _ in prep.flat)
    images = [bufs.to_dev(case["images"][i]) for i in keep]
    masks = [bufs.to_dev(case["masks"][i]) for i in keep]
    items = [(a.data_ptr(), m.data_ptr(), a.shape[1], a.shape[2], m.shape[0], m.shape[1]) for a, m in zip(images, masks)]
    scratch = torch.empty(lib.pipeline_batch_scratch_bytes(items), dtype=torch.uint8, device=DEV)
    bbox = torch.empty((3, 4), dtype=torch.int32, device=DEV)
    x = torch.empty((3, 4, rc.RES, rc.RES), dtype=torch.float32, device=DEV)
    lib.pipeline_batch_pre(items, rc.RES, rc.PADDING, x.data_ptr(), bbox.data_ptr(), scratch.data_ptr(), bufs.stream)
    sizes = [pc.patch_bytes(box, 3) for _, _, box in prep.flat]
    outs = [torch.full((n,), pc.FILL, dtype=torch.uint8, device=DEV) for n in sizes]
    lib.pipeline_batch_post_patches(items, 3, rc.RES, out["y_dev"].data_ptr(), bbox.data_ptr(), scratch.data_ptr(), [o.data_ptr() for o in outs],
                                    sizes, gauss25=pc.GAUSS, stream=bufs.stream)
    assert [tuple(b) for b in bbox.cpu().tolist()] == [box for _, _, box in prep.flat]
    for r, (_, _, box) in enumerate(prep.flat):
        np.testing.assert_array_equal(pc.patch_view(outs[r].cpu().numpy(), box, 3), out["patches"][r], err_msg=f"row {r}")


@pytest.mark.parametrize("name", ["overlapping_crops", "three_blobs", "borders"])
def test_paste_a_different_sample_per_region(pkg, name):
    lib, bufs = pkg.load_library(), _bufs()
    out = pc.check_case(lib, bufs, name, 3)
    prep, case = out["prep"], out["prep"].case
    choice = pc.mixed_choice(prep.flat, 3)
    assert len(set(choice)) >= 2
    want = pc.oracle_paste(case, prep.flat, out["y"], 3, choice)
    before = [o.clone() for o in out["outs"]]
    for order in ("forward", "reversed", "two calls"):
        images = [bufs.to_dev(a) for a in case["images"]]
        table = pc.paste_rows(prep, out["outs"], 3, choice, images)
        if order == "two calls":
            lib.pipeline_regions_paste(table[1:], bufs.stream)
            lib.pipeline_regions_paste(table[:1], bufs.stream)
        else:
            lib.pipeline_regions_paste(table if order == "forward" else table[::-1], bufs.stream)
        for got, w in zip(images, want):
            np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=f"{name}, {order}")
    for o, b in zip(out["outs"], before):
        assert torch.equal(o, b)
    prep.assert_inputs_untouched()
    # an unlisted region keeps the photo's bytes
    part = [choice[0]] + [None] * (len(choice) - 1)
    images = [bufs.to_dev(a) for a in case["images"]]
    lib.pipeline_regions_paste(pc.paste_rows(prep, out["outs"], 3, part, images), bufs.stream)
    got = images[0].cpu().numpy()
    np.testing.assert_array_equal(got, pc.oracle_paste(case, prep.flat, out["y"], 3, part)[0])
    np.testing.assert_array_equal(got[:, prep.labels[0] != 1], case["images"][0][:, prep.labels[0] != 1])


def test_pasting_the_one_sample_is_the_in_place_post(pkg):
    """S = 1, choice 0: what migan_pipeline_regions_post leaves for the same y; the 40 rows of many_rows cross a launch of 32"""
    lib, bufs = pkg.load_library(), _bufs()
    out = pc.check_case(lib, bufs, "many_rows", 1)
    prep, case = out["prep"], out["prep"].case
    pasted = [bufs.to_dev(a) for a in case["images"]]
    lib.pipeline_regions_paste(pc.paste_rows(prep, out["outs"], 1, [0] * len(prep.flat), pasted), bufs.stream)
    posted = [bufs.to_dev(a) for a in case["images"]]
    lib.pipeline_regions_post([prep.row(r, posted[prep.flat[r][0]]) for r in range(len(prep.flat))], case["res"], out["y_dev"].data_ptr(),
                              pc.GAUSS, bufs.stream)
    for a, b in zip(pasted, posted):
        assert torch.equal(a, b)
    assert not torch.equal(pasted[0], bufs.to_dev(case["images"][0]))


def test_operator_argument_errors(pkg):
    """every EINVAL of the header returns with nothing written"""
    lib, bufs = pkg.load_library(), _bufs()
    case = pc.CASES["three_blobs"]()
    prep = pc.Prepared(lib, bufs, case)
    h, w = case["images"][0].shape[1:]
    good, box = prep.table[0], prep.flat[0][2]
    y = torch.zeros((2, 3, rc.RES, rc.RES), dtype=torch.float32, device=DEV)
    n = pc.patch_bytes(box, 2)
    out = torch.full((n + pc.GUARD,), pc.FILL, dtype=torch.uint8, device=DEV)

    def post(rows=(good,), samples=2, outs=(out.data_ptr(),), caps=(n,)):
        lib.pipeline_regions_post_patches(list(rows), samples, rc.RES, y.data_ptr(), None if outs is None else list(outs),
                                          None if caps is None else list(caps), pc.GAUSS, bufs.stream)

    for bad in (dict(samples=0), dict(outs=(0,)), dict(outs=None), dict(caps=None), dict(caps=(n - 1,)),
                dict(rows=(good[:6] + ((0, w + 1, 0, 64),),)), dict(rows=(good[:6] + ((5, 7, 0, 64),),)), dict(rows=(good[:5] + (65, box),)),
                dict(rows=(good[:2] + (0,) + good[3:],))):
        with pytest.raises(ValueError):
            post(**bad)
    assert bool((out == pc.FILL).all())
    post()
    assert not bool((out[:n] == pc.FILL).all()) and bool((out[n:] == pc.FILL).all())
    img = bufs.to_dev(case["images"][0])
    pgood = (img.data_ptr(), prep.labels_dev[0].data_ptr(), out.data_ptr(), h, w, 1, box)
    for bad in (pgood[:2] + (0,) + pgood[3:], pgood[:1] + (0,) + pgood[2:], pgood[:5] + (65, box), pgood[:6] + ((0, w + 1, 0, 64),)):
        with pytest.raises(ValueError):
            lib.pipeline_regions_paste([pgood, bad], bufs.stream)
    np.testing.assert_array_equal(img.cpu().numpy(), case["images"][0])
    prep.assert_inputs_untouched()


# ---- MIGAN_Pipeline.forward_region_patches / paste_patches around the MI-GAN generator ----------------------------------------------------
@pytest.mark.parametrize("name, batch, kw", [("three_blobs", 2, dict(gap=3)), ("many_rows", 32, dict(gap=2, max_regions=32)),
                                             ("rule6", 32, dict(gap=3))])
def test_migan_paste_of_choice_0_is_forward_regions(pkg, name, batch, kw):
    """one completion per region, pasted back: forward_regions' bytes, boxes and label maps; three_blobs at B = 2 has a lone last
    chunk (batch 2), many_rows at B = 32 has rows of the second photo in both chunks, rule6 has unsplit photos and one without a hole"""
    pipe = _migan_pipeline(pkg)
    case = pc.CASES[name]()
    photos, masks = _upload(case["images"], case["masks"])
    copies, _ = _upload(case["images"], case["masks"])
    want, _ = _upload(case["images"], case["masks"])
    patches, boxes, labels = pipe.forward_region_patches(photos, masks, max_rows=batch, **kw)
    _, used, want_labels = pipe.forward_regions(want, masks, max_batch=batch, return_regions=True, **kw)
    got = pipe.paste_patches(copies, patches, boxes, labels, 0)
    assert got[0] is copies[0]
    for i, found in enumerate(case["found"]):
        assert torch.equal(copies[i], want[i]), f"image {i}"
        assert boxes[i].dtype == torch.int32 and boxes[i].device.type == "cpu" and torch.equal(boxes[i], used[i])
        assert boxes[i].tolist() == [list(b) for _, b in rc.rows_of(found)]
        if found["K"] <= case["max_regions"]:
            assert torch.equal(labels[i], want_labels[i])
        assert len(patches[i]) == boxes[i].shape[0]
        for p, (x0, x1, y0, y1) in zip(patches[i], boxes[i].tolist()):
            assert p.dtype == torch.uint8 and p.is_cuda and tuple(p.shape) == (1, 3, y1 - y0, x1 - x0)
        assert np.array_equal(photos[i][0].cpu().numpy(), case["images"][i]), f"photo {i} was written"
        assert np.array_equal(masks[i][0, 0].cpu().numpy(), case["masks"][i]), f"mask {i} was written"
    assert not torch.equal(copies[0], photos[0])                     # something was completed
    if name == "rule6":
        assert patches[2] == [] and tuple(boxes[2].shape) == (0, 4)


# ---- around a small Co-Mod-GAN -------------------------------------------------------------------------------------------------------------
def _three_photos(rng):
    """one region each: no photo is split"""
    sizes = [(90, 120), (70, 51), (33, 97)]
    holes = [(slice(30, 61), slice(40, 75)), (slice(50, 70), slice(31, 51)), (slice(5, 20), slice(10, 30))]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m, hole in zip(masks, holes):
        m[hole] = 0
    for m in masks:
        found = rc.oracle_find(m, 2, 8, res=32, padding=8)
        assert found["K"] == 1 and not found["split"]
    return images, masks


def _split_photos(rng):
    """three_blobs' mask at the Co-Mod-GAN's resolution (R = 32, padding 8, gap 2): three regions, split; and a photo with one region"""
    blobs = rc.CASES["three_blobs"]()["masks"][0]
    one = np.full((70, 51), 255, dtype=np.uint8)
    one[50:70, 31:51] = 0
    masks = [blobs, one]
    found = [rc.oracle_find(m, 2, 8, res=32, padding=8) for m in masks]
    assert [f["K"] for f in found] == [3, 1] and [f["split"] for f in found] == [True, False]
    images = [rng.integers(0, 256, (3,) + m.shape, dtype=np.uint8) for m in masks]
    return images, masks, found


def test_comodgan_unsplit_photos_are_forward_patches(pkg):
    """no photo is split: patches[i][0] and boxes[i][0] are forward_patches' for the same z and max_rows (two chunks at max_rows = 6)"""
    pipe, cfg = _comodgan_pipeline(pkg)
    rng = np.random.default_rng(81)
    images, masks = _three_photos(rng)
    d_img, d_mask = _upload(images, masks)
    z = torch.from_numpy(pkg.synth.make_latent(9, cfg.z_dim, 81).reshape(3, 3, cfg.z_dim)).to(DEV)
    for max_rows in (32, 6):
        want, want_boxes = pipe.forward_patches(d_img, d_mask, z, max_rows=max_rows, noise_mode="const")
        patches, boxes, labels = pipe.forward_region_patches(d_img, d_mask, z, max_rows=max_rows, noise_mode="const")
        for i in range(3):
            assert len(patches[i]) == 1 and tuple(boxes[i].shape) == (1, 4)
            assert torch.equal(boxes[i][0], want_boxes[i])
            assert torch.equal(patches[i][0], want[i]), f"image {i}, max_rows {max_rows}"
            assert tuple(labels[i].shape) == images[i].shape[1:] and labels[i].dtype == torch.uint8
            assert np.array_equal(d_img[i][0].cpu().numpy(), images[i]), f"image {i} was written"
        assert not torch.equal(patches[0][0][0], patches[0][0][1])   # different z: different completions
    assert pkg.load_library().backend() == "hip:gfx950"


def test_comodgan_split_photo_equals_its_stages_and_pastes_a_mixed_choice(pkg):
    """a split photo (three rows) and an unsplit one, S = 2, one chunk: the method equals find -> rows -> pre -> forward_samples(x,
    z[image of row]) -> post_patches called by hand; paste_patches with a mixed choice equals migan_pipeline_regions_post fed the
    chosen y rows"""
    pipe, cfg = _comodgan_pipeline(pkg)
    lib = pkg.load_library()
    rng = np.random.default_rng(82)
    images, masks, found = _split_photos(rng)
    d_img, d_mask = _upload(images, masks)
    S, R = 2, 32
    z = torch.from_numpy(pkg.synth.make_latent(2 * S, cfg.z_dim, 82).reshape(2, S, cfg.z_dim)).to(DEV)
    patches, boxes, labels = pipe.forward_region_patches(d_img, d_mask, z, gap=2, noise_mode="const")
    want_rows = [rc.rows_of(f) for f in found]
    assert [b.tolist() for b in boxes] == [[list(box) for _, box in rows] for rows in want_rows]
    assert [len(p) for p in patches] == [3, 1]
    np.testing.assert_array_equal(labels[0].cpu().numpy(), found[0]["labels"])
    # the stages by hand
    stream = int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    flat = [(i, label, box) for i, rows in enumerate(want_rows) for label, box in rows]
    table = [(d_img[i].data_ptr(), d_mask[i].data_ptr(), labels[i].data_ptr(), images[i].shape[1], images[i].shape[2], label, box)
             for i, label, box in flat]
    x = torch.empty((len(flat), 4, R, R), dtype=torch.float32, device=DEV)
    lib.pipeline_regions_pre(table, R, x.data_ptr(), stream)
    y = pipe.model.forward_samples(x, z[[i for i, _, _ in flat]], noise_mode="const").reshape(len(flat) * S, 3, R, R).contiguous()
    sizes = [pc.patch_bytes(box, S) for _, _, box in flat]
    outs = [torch.full((n + pc.GUARD,), pc.FILL, dtype=torch.uint8, device=DEV) for n in sizes]
    lib.pipeline_regions_post_patches(table, S, R, y.data_ptr(), [o.data_ptr() for o in outs], sizes, pipe._gauss, stream)
    got = [p for mine in patches for p in mine]
    for r, (o, n) in enumerate(zip(outs, sizes)):
        assert torch.equal(got[r].flatten(), o[:n]), f"row {r}"
        assert bool((o[n:] == pc.FILL).all())
    assert not torch.equal(got[0][0], got[0][1])
    # the definition of a patch byte, on the generator's own y (which saturates, so blends land next to integers): patch (r, s) is
    # the crop of what migan_pipeline_regions_post leaves in a copy of the photo for row r alone with y row r * S + s
    for r, (i, label, (x0, x1, y0, y1)) in enumerate(flat):
        for s in range(S):
            alone = d_img[i].clone()
            lib.pipeline_regions_post([(alone.data_ptr(),) + table[r][1:]], R, y[r * S + s:r * S + s + 1].data_ptr(), pipe._gauss, stream)
            assert torch.equal(got[r][s], alone[0][:, y0:y1, x0:x1]), f"row {r} sample {s}"
    # paste: a different sample per region of photo 0, region 2 left alone; photo 1 by one int
    choice = [[1, None, 0], 1]
    copies, _ = _upload(images, masks)
    assert pipe.paste_patches(copies, patches, boxes, labels, choice)[1] is copies[1]
    posted, _ = _upload(images, masks)
    picks = [(0, 1), (2, 0), (3, 1)]                                 # (row of `flat`, sample)
    rows = [(posted[flat[r][0]].data_ptr(),) + table[r][1:] for r, _ in picks]
    ys = torch.stack([y[r * S + s] for r, s in picks]).contiguous()
    lib.pipeline_regions_post(rows, R, ys.data_ptr(), pipe._gauss, stream)
    for i in range(2):
        assert torch.equal(copies[i], posted[i]), f"image {i}"
        assert np.array_equal(d_img[i][0].cpu().numpy(), images[i]), f"photo {i} was written"
    lab = found[0]["labels"]
    got0 = copies[0][0].cpu().numpy()
    keep = (lab != 1) & (lab != 3)
    np.testing.assert_array_equal(got0[:, keep], images[0][:, keep])
    assert (got0[:, lab == 1] != images[0][:, lab == 1]).any() and (got0[:, lab == 3] != images[0][:, lab == 3]).any()
    # samples=S draws z as forward_samples does: the same generator state, the same patches
    torch.manual_seed(5)
    drawn, _, _ = pipe.forward_region_patches(d_img, d_mask, samples=S, gap=2, noise_mode="const")
    torch.manual_seed(5)
    z5 = torch.randn([2, S, cfg.z_dim]).to(DEV)
    given, _, _ = pipe.forward_region_patches(d_img, d_mask, z5, gap=2, noise_mode="const")
    assert all(torch.equal(a, b) for ma, mb in zip(drawn, given) for a, b in zip(ma, mb))


def test_argument_errors_of_both_methods(pkg):
    pipe = _migan_pipeline(pkg)
    case = pc.CASES["three_blobs"]()
    imgs, masks = _upload(case["images"], case["masks"])
    with pytest.raises(ValueError, match="no forward_samples"):
        pipe.forward_region_patches(imgs, masks, torch.zeros(1, 2, 512, device=DEV))
    with pytest.raises(ValueError, match="no forward_samples"):
        pipe.forward_region_patches(imgs, masks, samples=2)
    with pytest.raises(ValueError, match="gap"):
        pipe.forward_region_patches(imgs, masks, gap=1)
    with pytest.raises(ValueError, match="max_regions"):
        pipe.forward_region_patches(imgs, masks, max_regions=65)
    with pytest.raises(RuntimeError, match="max_rows"):
        pipe.forward_region_patches(imgs, masks, max_rows=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.forward_region_patches([imgs[0].cpu()], [masks[0].cpu()])
    with pytest.raises(RuntimeError):
        pipe.forward_region_patches(imgs, masks + masks)
    cpipe, cfg = _comodgan_pipeline(pkg)
    with pytest.raises(ValueError, match="max_rows"):
        cpipe.forward_region_patches(imgs, masks, torch.zeros(1, 3, cfg.z_dim, device=DEV), max_rows=2)         # S > max_rows
    with pytest.raises(ValueError):
        cpipe.forward_region_patches(imgs, masks)                                                               # neither z nor samples
    with pytest.raises(ValueError):
        cpipe.forward_region_patches(imgs, masks, torch.zeros(2, 3, cfg.z_dim, device=DEV))                     # z for two photos

    patches, boxes, labels = pipe.forward_region_patches(imgs, masks, gap=3)
    assert len(patches[0]) == 3
    copies, _ = _upload(case["images"], case["masks"])
    for bad in (1, [[0, 0]], [[0, 0, 1]], [[0, -2, 0]], [0, 0]):                                                 # S = 1: choice 1 does not exist
        with pytest.raises(ValueError):
            pipe.paste_patches(copies, patches, boxes, labels, bad)
    with pytest.raises(ValueError):
        pipe.paste_patches(copies, [patches[0][:2]], boxes, labels, 0)                                          # a patch is missing
    with pytest.raises(ValueError):
        pipe.paste_patches(copies, [[patches[0][0][:, :, 1:].contiguous()] + patches[0][1:]], boxes, labels, 0)   # a patch of another shape
    with pytest.raises(ValueError):
        pipe.paste_patches(copies, patches, boxes, [], 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.paste_patches([copies[0].cpu()], patches, boxes, labels, 0)
    assert np.array_equal(copies[0][0].cpu().numpy(), case["images"][0])                                        # nothing was pasted
    assert pipe.paste_patches(copies, patches, boxes, labels, [[None, -1, None]])[0] is copies[0]
    assert np.array_equal(copies[0][0].cpu().numpy(), case["images"][0])
    pipe.paste_patches(copies, patches, boxes, labels, [[None, 0, None]])
    lab = case["found"][0]["labels"]
    got = copies[0][0].cpu().numpy()
    assert (got[:, lab == 2] != case["images"][0][:, lab == 2]).any()
    np.testing.assert_array_equal(got[:, lab != 2], case["images"][0][:, lab != 2])
