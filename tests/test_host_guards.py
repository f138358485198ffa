"""Host-side guards of the C ABI, through the CPU emulator build of the same host code: the 32-bit per-image
offsets of the kernels bound the arbitrary-size forward, a plan that fails to build is never cached, the sub-batch hand-over
event is always recorded, the 'default' GEMM name resolves per storage format."""
import importlib

import numpy as np
import pytest

from tests.emu_util import aligned, emu_lib
from tests.knobs import knobs


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("mi-gan_amd")


def _bind(pkg, lib, res, seed, dtype="f32"):
    h = pkg.hipbind.MiganHandle(lib, res, dtype=dtype)
    sd = pkg.synth.make_state_dict(res, seed=seed, regime="export")
    keep = {k: aligned(v.reshape(1) if v.ndim == 0 else v) for k, v in sd.items()}
    for name, shape, _ in h.weights():
        h.set_weight(name, keep[name].ctypes.data, shape)
    h.commit()
    return h, sd, keep


def test_oversize_forward_hw_is_refused_by_the_offset_width_not_a_pixel_cap(pkg, lib):
    """channels_at(64) = 512: 4096 x 4096 pixels would be 2^33 elements per tensor; the kernels' 32-bit byte offsets end at 2^30
    fp32 elements.  Generator(512) (64 channels at full size) fits a larger image than Generator(64)."""
    h64 = pkg.hipbind.MiganHandle(lib, 64)
    with pytest.raises(ValueError, match="too large"):
        h64.workspace_bytes_hw(1, 4096, 4096)
    with pytest.raises(ValueError, match="too large"):
        h64.workspace_bytes_hw(1, 2048, 1024)                      # 2^21 pixels x 512 channels = 2^30 elements: one past the end
    assert h64.workspace_bytes_hw(1, 1024, 1008) > 0               # just below
    h512 = pkg.hipbind.MiganHandle(lib, 512)
    assert h512.workspace_bytes_hw(1, 2048, 4096) > 0              # 2^23 pixels x 64 channels = 2^29 elements
    with pytest.raises(ValueError, match="too large"):
        h512.workspace_bytes_hw(1, 4096, 4096)


# the extent limit (kMaxImageElems in migan_host.hpp): h * w * channels <= 2^30 - 1024 for every per-image tensor
LIMIT = 2 ** 30 - 1024
OPERATOR_EDGES = [
    # name, layer, (h, w) one step beyond the limit, the step before it (one row less)
    ("64to64", dict(cin=64, cout=64), (4096, 4096), (4095, 4096)),
    ("64to256", dict(cin=64, cout=256), (2048, 2048), (2047, 2048)),
    ("64to64_up", dict(cin=64, cout=64, up=2), (2048, 2048), (2047, 2048)),             # the output is the larger tensor
    ("64to128_down", dict(cin=64, cout=128, down=2), (4096, 4096), (4094, 4096)),       # the input is
    ("narrow", dict(cin=32, cout=32), (8192, 4096), (8191, 4096)),
    ("sliver", dict(cin=64, cout=64), (4095, 4097), (4095, 4096)),                      # 2^32 - 256 bytes: the padding marker in range
]


@pytest.mark.parametrize("name,layer,beyond,inside", OPERATOR_EDGES, ids=[e[0] for e in OPERATOR_EDGES])
def test_operator_refuses_one_step_beyond_the_extent_limit(pkg, lib, name, layer, beyond, inside):
    """migan_sepconv_forward applies the plan's limit, on the tiled and on the narrow branch, before any launch: small buffers suffice,
    and they keep their fill.  (The size just inside cannot run on the emulator; tests/test_gpu_large_extents.py runs it on the GPU.)"""
    cin, cout = layer["cin"], layer["cout"]
    f = lambda h, w: (h // 2, w // 2) if layer.get("down") == 2 else ((2 * h, 2 * w) if layer.get("up") == 2 else (h, w))
    top = lambda h, w: max(h * w * cin, f(h, w)[0] * f(h, w)[1] * cout)
    assert top(*inside) <= LIMIT < top(*beyond)
    fill = lambda n: aligned(np.full(n, 7.5, np.float32))
    x, y, skip, scratch, img = fill(4096), fill(4096), fill(4096), fill(4096), fill(4096)
    w1, b1, w2 = fill(cin * 9), fill(cin), fill(cin * cout)
    nc, ns, wsp = fill(4096), fill(1), fill(2 * cin * cout + 64)
    for samples in ((None,) if name == "narrow" or layer.get("down") else (None, 1)):
        with pytest.raises(ValueError, match="too large"):
            lib.sepconv_forward(samples=samples, x=x.ctypes.data, y=y.ctypes.data, skip=skip.ctypes.data, conv1_weight=w1.ctypes.data,
                                conv1_bias=b1.ctypes.data, conv2_weight=w2.ctypes.data, noise_const=nc.ctypes.data,
                                noise_strength=ns.ctypes.data, batch=1, cin=cin, cout=cout, res_in=beyond[0], width_in=beyond[1],
                                down=layer.get("down", 1), up=layer.get("up", 1), scratch=scratch.ctypes.data, scratch_bytes=1 << 40,
                                wsplit=wsp.ctypes.data, wsplit_bytes=wsp.nbytes, dtype=0)
    for a in (x, y, skip, scratch, img, w1, b1, w2, nc, ns, wsp):
        assert (a == 7.5).all(), "a refused call wrote a buffer"


def test_the_size_just_inside_the_extent_limit_plans(pkg, lib):
    """the plan and the operator share the function: Generator(512) has 64 channels at full size, 4096 x 3968 is the largest multiple of
    128 below 2^24 - 16 pixels"""
    h512 = pkg.hipbind.MiganHandle(lib, 512)
    assert 4096 * 3968 * 64 <= LIMIT < 4096 * 4096 * 64
    assert h512.workspace_bytes_hw(1, 4096, 3968) > 0
    assert h512.workspace_bytes_hw(1, 3968, 4096) > 0


def test_a_failed_plan_is_not_cached(pkg, lib):
    """sizes that are refused leave nothing behind: asking again fails the same way, and a valid size still plans and runs"""
    res = 8
    h, sd, keep = _bind(pkg, lib, res, seed=4)
    for _ in range(2):
        with pytest.raises(ValueError):
            h.workspace_bytes_hw(1, 7, 8)                          # not a multiple of resolution / 4
    for k in range(20):                                            # more distinct sizes than the plan cache keeps
        assert h.workspace_bytes_hw(1, 8 + 2 * (k % 5), 8 + 2 * (k // 5)) > 0
    x = pkg.synth.make_input(1, res, seed=9)
    xa, y = aligned(x), aligned(np.full((1, 3, res, res), np.nan, np.float32))
    need = h.workspace_bytes_hw(1, res, res)
    ws = np.zeros(need // 4 + 64, np.float32)
    h.forward_hw(xa.ctypes.data, y.ctypes.data, 1, res, res, ws.ctypes.data, need)
    assert np.isfinite(y).all()


@pytest.mark.parametrize("pct", [0, 100])
def test_sub_batch_stagger_is_clamped_to_an_existing_launch(pkg, lib, pct):
    """stagger_pct = 100 used to index one past the last launch: the event the next sub-batch waits on was never recorded"""
    res = 8
    with knobs(lib, stagger_pct=pct):
        h, sd, keep = _bind(pkg, lib, res, seed=6)
        x = pkg.synth.make_input(16, res, seed=6)
        outs = []
        for streams in (1, 2):
            h.set_streams(streams)
            xa, y = aligned(x), aligned(np.full((16, 3, res, res), np.nan, np.float32))
            need = h.workspace_bytes(16)
            ws = np.zeros(need // 4 + 64, np.float32)
            h.forward(xa.ctypes.data, y.ctypes.data, 16, ws.ctypes.data, need)
            outs.append(y.copy())
        np.testing.assert_array_equal(outs[0], outs[1])


def test_default_gemm_name_resolves_per_storage_format(pkg, lib):
    h = pkg.hipbind.MiganHandle(lib, 8)
    h.set_gemm("f32")
    h.set_gemm("default")
    assert h.gemm() == lib.gemm_variant()
    hb = pkg.hipbind.MiganHandle(lib, 8, dtype="bf16")
    hb.set_gemm("f16x2")
    hb.set_gemm("default")
    assert hb.gemm() == "f16"
