"""Photo loading on the MI355X: the cases of tests/photo_case.py (those of tests/test_emu_photo.py) through migan_photo_resize_batch
with ctypes on device buffers, then the Python front (mi-gan_amd/photo.py) and what it feeds: forward_uint8 of both generators.  Only
the goldens are read (tests/golden/photo_*.npz: Pillow's and the reference functions' bytes); every comparison is equality of bytes."""
import os

import numpy as np
import pytest
import torch

from tests import photo_case as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def mem():
    return pc.CudaMem(DEV)


@pytest.mark.parametrize("name", sorted(pc.BICUBIC_CASES))
def test_bicubic(lib, mem, name):
    pc.run_bicubic_case(lib, mem, name)


def test_bicubic_from_odd_addresses(lib, mem):
    for name in ("down_37x53_to_16x16", "narrow_7x5_to_16x16", "near1_129x127_to_128x128"):
        pc.run_bicubic_case(lib, mem, name, odd=True)


def test_bicubic_span_longer_than_the_stage(lib, mem):
    src = pc.photo(100, 3000, 7)
    got = pc.call(lib, mem, [src], [(2, 100)], pc.BICUBIC)[0]
    assert np.array_equal(got, pc.pil_bicubic(src, (2, 100)))


@pytest.mark.parametrize("name", sorted(pc.NEAREST_CASES))
def test_nearest(lib, mem, name):
    pc.run_nearest_case(lib, mem, name)


def test_nearest_flags(lib, mem):
    pc.run_flags(lib, mem)


def test_batches(lib, mem):
    pc.run_batches(lib, mem)


def test_argument_errors(lib, mem):
    pc.run_arg_errors(lib, mem)


def test_exports_in_the_built_libraries(pkg, lib):
    assert lib.backend() == "hip:gfx950"
    for path in (pkg.library_path(), os.path.join(os.path.dirname(pkg.library_path()), "libmigan_hip_nanclamp.so")):
        loaded = pkg.hipbind.MiganLib(path)
        for name in pkg.hipbind.exports("migan_photo_hip.h"):
            assert hasattr(loaded.lib, name), f"{path} does not export {name}"


# ---- the Python front ----------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.array(a))                          # (a writable copy: the goldens are read-only)


def _device(arrays):
    return [_t(a).to(DEV) for a in arrays]


def test_front_resizes(pkg):
    ph = pkg.photo
    g = pc.golden("batch")
    srcs = _device([g[f"b5.src{i}"] for i in range(5)])
    outs = ph.resize_bicubic(srcs, list(pc.BATCH5_SIZES))
    assert isinstance(outs, list) and all(torch.equal(o.cpu(), _t(g[f"b5.out{i}"])) for i, o in enumerate(outs))
    one = ph.resize_bicubic(srcs, (24, 24))                        # one size for all: a stacked tensor
    assert tuple(one.shape) == (5, 24, 24, 3) and torch.equal(one[2].cpu(), _t(g["b5.out2"])) and torch.equal(one[4], srcs[4])
    n = pc.golden("nearest")
    flag_src = _device([n["flags.src"]])
    for invert in (False, True):
        for threshold in (False, True):
            flags = (pc.INVERT if invert else 0) | (pc.THRESHOLD if threshold else 0)
            got = ph.resize_nearest(flag_src, (7, 17), invert=invert, threshold=threshold)
            want = n[f"flags.{flags}.7x17"] if flags else pc.pil_nearest(n["flags.src"], (7, 17))
            assert tuple(got.shape) == (1, 17, 7) and torch.equal(got[0].cpu(), _t(want))
    name = "up_16x16_to_37x53"
    got = ph.resize_nearest(_device([n[f"{name}.src"]]), [(53, 37)])
    assert torch.equal(got[0].cpu(), _t(n[f"{name}.out"]))


@pytest.mark.parametrize("r", pc.FLOW_RESOLUTIONS)
def test_front_flows(pkg, r):
    ph = pkg.photo
    images, masks = pc.flow_sources()
    d_img, d_mask = _device(images), _device(masks)
    img, mask = ph.load_eval(d_img, d_mask, r)
    want = pc.flow_golden("eval", r)
    assert img.dtype == mask.dtype == torch.uint8 and tuple(img.shape) == (5, r, r, 3) and tuple(mask.shape) == (5, r, r)
    assert torch.equal(img.cpu(), _t(want[0])) and torch.equal(mask.cpu(), _t(want[1]))
    for invert in (False, True):
        img, mask = ph.load_demo(d_img, d_mask, r, invert_mask=invert)
        want = pc.flow_golden("demo", r, invert)
        assert torch.equal(img.cpu(), _t(want[0])) and torch.equal(mask.cpu(), _t(want[1])), f"invert {invert}"
    for a, d in zip(images + masks, d_img + d_mask):               # the inputs are only read
        assert np.array_equal(d.cpu().numpy(), a)


def test_end_to_end_migan(pkg):
    """Generator(16): forward_uint8 of what load_eval made of the photos is forward_uint8 of the golden arrays, bit for bit"""
    m = pkg.Generator(resolution=16)
    sd = pkg.synth.make_state_dict(16, seed=13)
    m.load_state_dict({k: _t(v.copy()) for k, v in sd.items()})
    m = m.to(DEV).eval()
    images, masks = pc.flow_sources()
    want_img, want_mask = (_t(a).to(DEV) for a in pc.flow_golden("eval", 16))
    with torch.no_grad():
        got = m.forward_uint8(*pkg.photo.load_eval(_device(images), _device(masks), 16))
        want = m.forward_uint8(want_img, want_mask)
    assert torch.equal(got, want) and bool((got[want_mask == 255] == want_img[want_mask == 255]).all())


def test_end_to_end_comodgan(pkg):
    cs, cm = pkg.comodgan_schema, pkg.comodgan
    cfg = cs.Config(resolution=16, ch_base=1024, ch_max=64, num_ws=cs.default_num_ws(16))          # (the smallest golden size of the u8 tests)
    kw = dict(ch_base=cfg.ch_base, ch_max=cfg.ch_max)
    m = cm.Generator(cm.Mapping(num_ws=cfg.num_ws), cm.Encoder(resolution=16, **kw), cm.Synthesis(resolution=16, **kw))
    sd = pkg.synth.make_comodgan_state_dict(cfg, 51)
    m.load_state_dict({k: _t(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    images, masks = pc.flow_sources()
    want_img, want_mask = (_t(a).to(DEV) for a in pc.flow_golden("demo", 16, True))
    z = _t(pkg.synth.make_latent(10, cfg.z_dim, 51).reshape(5, 2, cfg.z_dim)).to(DEV)
    with torch.no_grad():
        got = m.forward_samples_uint8(*pkg.photo.load_demo(_device(images), _device(masks), 16, invert_mask=True), z, noise_mode="const")
        want = m.forward_samples_uint8(want_img, want_mask, z, noise_mode="const")
    assert tuple(got.shape) == (5, 2, 16, 16, 3) and torch.equal(got, want)


def test_front_errors(pkg):
    ph = pkg.photo
    img = torch.zeros((20, 24, 3), dtype=torch.uint8, device=DEV)
    msk = torch.zeros((20, 24), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="aspect"):
        ph.resize_bicubic([torch.zeros((33, 1, 3), dtype=torch.uint8, device=DEV)], (16, 16))
    with pytest.raises(ValueError, match="destination sides"):
        ph.resize_nearest([msk], (4097, 16))
    with pytest.raises(ValueError, match="destination sides"):
        ph.resize_bicubic([img], (0, 16))
    with pytest.raises(ValueError, match="side of 0"):
        ph.load_demo([torch.zeros((2, 40, 3), dtype=torch.uint8, device=DEV)], [msk], 16)
    with pytest.raises(ValueError, match="size must be"):
        ph.resize_bicubic([img, img], [(16, 16)])
    with pytest.raises(ValueError, match="resolution"):
        ph.load_eval([img], [msk], 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ph.load_eval([img.cpu()], [msk.cpu()], 16)
    with pytest.raises(RuntimeError, match="uint8"):
        ph.resize_bicubic([img.float()], (16, 16))
    with pytest.raises(RuntimeError, match="contiguous"):
        ph.resize_nearest([msk.t()], (16, 16))
    with pytest.raises(RuntimeError, match=r"\(H, W, 3\)"):
        ph.resize_bicubic([msk], (16, 16))
    with pytest.raises(RuntimeError, match="one length"):
        ph.load_eval([img, img], [msk], 16)
    with pytest.raises(RuntimeError, match="non-empty list"):
        ph.resize_bicubic([], (16, 16))
