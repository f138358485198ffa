"""Photo loading (include/migan_photo_hip.h) on the CPU emulator: the kernels of mi-gan_amd/csrc/migan_photo.hpp and the host code
behind migan_photo_resize_batch, on host memory, against the bytes Pillow and the reference's own functions gave
(tests/golden/photo_*.npz).  Every comparison is equality of bytes.  The same cases run on the device in tests/test_gpu_photo.py."""
import os
import re

import numpy as np
import pytest

from tests import photo_case as pc
from tests.emu_util import ROOT, aligned, emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.mark.parametrize("name", sorted(pc.BICUBIC_CASES))
def test_bicubic(lib, mem, name):
    pc.run_bicubic_case(lib, mem, name)


def test_bicubic_from_odd_addresses(lib, mem):
    """neither the sources nor the destinations are aligned: the staging reads whole dwords only inside the image"""
    for name in ("down_37x53_to_16x16", "narrow_7x5_to_16x16", "near1_129x127_to_128x128"):
        pc.run_bicubic_case(lib, mem, name, odd=True)


def test_bicubic_one_channel(lib, mem):
    src = pc.golden("bicubic")["down_37x53_to_16x16.src"]
    for c in range(3):
        plane = np.ascontiguousarray(src[:, :, c])
        got = pc.call(lib, mem, [plane], [(16, 16)], pc.BICUBIC)[0]
        assert np.array_equal(got, pc.golden("bicubic")["down_37x53_to_16x16.out"][:, :, c])


def test_bicubic_span_longer_than_the_stage(lib, mem):
    """3000 -> 2 columns: one output's taps cover more source bytes than one staged piece holds, so the pieces are walked"""
    src = pc.photo(100, 3000, 7)
    assert 3 * 4 * 1500 > pc.ROW_BYTES
    got = pc.call(lib, mem, [src], [(2, 100)], pc.BICUBIC)[0]
    assert np.array_equal(got, pc.pil_bicubic(src, (2, 100)))


@pytest.mark.parametrize("name", sorted(pc.NEAREST_CASES))
def test_nearest(lib, mem, name):
    pc.run_nearest_case(lib, mem, name)


def test_nearest_flags(lib, mem):
    pc.run_flags(lib, mem)


def test_batches(lib, mem):
    pc.run_batches(lib, mem)


@pytest.mark.parametrize("r", pc.FLOW_RESOLUTIONS)
def test_flows(lib, mem, r):
    images, masks = pc.flow_sources()
    img, mask = pc.flow_through_abi(lib, mem, "eval", images, masks, r)
    want = pc.flow_golden("eval", r)
    assert np.array_equal(img, want[0]) and np.array_equal(mask, want[1])
    for invert in (False, True):
        img, mask = pc.flow_through_abi(lib, mem, "demo", images, masks, r, invert)
        want = pc.flow_golden("demo", r, invert)
        assert np.array_equal(img, want[0]) and np.array_equal(mask, want[1]), f"demo r {r} invert {invert}"


def test_end_to_end_migan(pkg, lib, mem):
    """Generator(16): forward_u8 of what the loader made of the photos is forward_u8 of the golden arrays, bit for bit"""
    from tests.test_emu_round2 import _bind
    images, masks = pc.flow_sources()
    img, mask = pc.flow_through_abi(lib, mem, "eval", images, masks, 16)
    h, _, keep = _bind(pkg, lib, 16, 13)
    n = len(images)
    need = h.workspace_bytes(n)
    outs = []
    for a, b in ((img, mask), pc.flow_golden("eval", 16)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        out = np.full((n, 16, 16, 3), 77, np.uint8)
        ws = np.zeros(need // 4 + 64, np.float32)
        h.forward_u8(a.ctypes.data, b.ctypes.data, out.ctypes.data, n, ws.ctypes.data, need)
        outs.append(out)
    h.close()
    assert np.array_equal(outs[0], outs[1]) and not (outs[0] == 77).all()
    known = pc.flow_golden("eval", 16)[1] == 255
    assert (outs[0][known] == pc.flow_golden("eval", 16)[0][known]).all()


def test_end_to_end_comodgan(pkg, lib, mem):
    from tests.test_emu_comodgan_samples import small, workspace
    from tests.test_emu_comodgan_u8 import fused, prepare
    cfg = small(16)
    images, masks = pc.flow_sources()
    img, mask = pc.flow_through_abi(lib, mem, "eval", images, masks, 16)
    h, keep, _ = prepare(cfg, 51)
    n, s = len(images), 2
    za = aligned(pkg.synth.make_latent(n * s, cfg.z_dim, 51))
    nbytes = h.workspace_bytes_samples(n, s)
    wsv = workspace(nbytes)
    got = fused(h, cfg, np.ascontiguousarray(img), np.ascontiguousarray(mask), za, n, s, wsv, nbytes, noise_mode="const")
    want = fused(h, cfg, np.ascontiguousarray(pc.flow_golden("eval", 16)[0]), np.ascontiguousarray(pc.flow_golden("eval", 16)[1]), za, n, s, wsv, nbytes,
                 noise_mode="const")
    h.close()
    assert np.array_equal(got, want) and not (got == 77).all()


def test_argument_errors(lib, mem):
    pc.run_arg_errors(lib, mem)


def test_python_front_refuses_before_the_device(pkg):
    """what mi-gan_amd/photo.py decides on the host: demo.py's sizes in the script's own expressions, a side of 0, the domain"""
    ph = pkg.photo
    assert ph.fit_size(100, 75, 16) == (16, 12) and ph.fit_size(75, 100, 16) == (12, 16) and ph.fit_size(12, 9, 16) == (12, 9)
    for w, h, r in ((100, 75, 16), (4000, 3000, 512), (450, 600, 512), (49, 7, 32), (107, 30, 16)):
        assert ph.fit_size(w, h, r) == pc.fit_size(w, h, r)
    # int(w * (R / w)) can be R - 1, and the result follows it
    odd = [(w, r) for r in (16, 32, 256, 512) for w in range(r + 1, 4 * r) if int(w * (r / w)) != r]
    assert odd and all(ph.fit_size(w, 1 + w // 2, r)[0] == r - 1 for w, r in odd)
    assert ph.demo_plan((100, 75), (450, 600), 16) == ((16, 12), (384, 512), (12, 16))
    with pytest.raises(ValueError, match="side of 0"):
        ph.fit_size(40, 2, 16)
    with pytest.raises(ValueError, match="side of 0"):
        ph.demo_plan((20, 20), (2, 40), 16)
    with pytest.raises(ValueError, match="aspect"):
        ph.check_sizes((33, 1), (16, 16))
    with pytest.raises(ValueError, match="source sides"):
        ph.check_sizes((16385, 16384), (16, 16))
    with pytest.raises(ValueError, match="destination sides"):
        ph.check_sizes((20, 20), (4097, 16))
    ph.check_sizes((16384, 16384), (4096, 4096))
    ph.check_sizes((32, 1), (1, 1))
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        ph.resize_bicubic([torch.zeros((4, 4, 3), dtype=torch.uint8)], (2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ph.load_demo([torch.zeros((4, 4, 3), dtype=torch.uint8)], [torch.zeros((4, 4), dtype=torch.uint8)], 16)


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "mi-gan_amd", "csrc", "migan_photo.hpp")).read()
    assert re.search(r"kPhItemsMax = (\d+)", text).group(1) == str(pc.ITEMS_PER_LAUNCH)
    assert re.search(r"kPhTW = (\d+), kPhTR = (\d+)", text).groups() == (str(pc.TILE_W), str(pc.TILE_R))
    assert re.search(r"kPhRowBytes = (\d+)", text).group(1) == str(pc.ROW_BYTES)
    assert re.search(r"kPhSrcMax = (\d+), kPhDstMax = (\d+), kPhAspectMax = (\d+)", text).groups() == (str(pc.SRC_MAX), str(pc.DST_MAX), str(pc.ASPECT_MAX))
    assert re.search(r"kPhPrecisionBits = (\d+)", text).group(1) == str(pc.PRECISION_BITS)
    # the table kernel's arithmetic runs with contraction off, and nothing in the unit is an atomic
    assert text.count("#pragma clang fp contract(off)") >= 3 and "atomic" not in text.replace("No atomics", "")


def test_exports(pkg):
    """the header against the binding: tests/test_abi_headers.py; here the case module against the binding"""
    hb = pkg.hipbind
    assert (pc.NEAREST, pc.BICUBIC, pc.INVERT, pc.THRESHOLD) == (hb.PHOTO_NEAREST, hb.PHOTO_BICUBIC, hb.PHOTO_INVERT, hb.PHOTO_THRESHOLD)
    assert pkg.photo.SRC_MAX == pc.SRC_MAX and pkg.photo.DST_MAX == pc.DST_MAX and pkg.photo.ASPECT_MAX == pc.ASPECT_MAX
    assert "photo" in pkg.__all__
