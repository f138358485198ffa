"""Every launch of an MI-GAN plan on a real MI355X against the oracle on the device's own input tap (tests/migan_layers_case.py; the
R = 16 cases run through the emulator in tests/test_emu_migan_layers.py).  Run with -s for the per-unit table; measured figures and the
wall time of each case: profiles/migan_layers.md."""
import pytest
import torch

from tests.migan_layers_case import GPU_16BIT, GPU_16BIT_KNOBS, GPU_CASES, GPU_F32, is_small, run_case, run_window_case
from tests.sepconv_case import CudaMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg.load_library()
    assert lib.backend() == "hip:gfx950"
    return lib


RAN = {}          # case -> the kernel symbols its forward launched
REPORT = {}       # case -> rows and wall time (a script that writes profiles/migan_layers.md reads it)


def _run(pkg, lib, dev, name):
    if name not in RAN:
        REPORT[name] = {}
        RAN[name] = run_case(lib, pkg, CudaMem(dev), tag=name, report=REPORT[name], **GPU_CASES[name])
    return RAN[name]


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_every_launch_in_isolation(pkg, lib, dev, name):
    _run(pkg, lib, dev, name)
    print(f"{name}: {REPORT[name]['seconds']:.2f} s, of which bind + forward + read-back {REPORT[name]['device_seconds']:.2f} s")


def test_generator_at_the_extent_limit(pkg, lib, dev):
    """Generator(512) through migan_forward_hw at 4096 x 3968, the largest multiples of 128 whose full-resolution tensors (64 channels)
    stay within the extent limit of the kernels, 2^30 - 1024 elements (4096 x 4096 is refused): every unit in plan context, on row
    windows read back from the device (the debug workspace is some 30 GiB)"""
    import torch
    assert 4096 * 3968 * 64 <= 2 ** 30 - 1024 < 4096 * 4096 * 64
    rep = {}
    run_window_case(lib, pkg, dev, res=512, hw=(4096, 3968), seed=251, tag="r512_4096x3968", report=rep)
    torch.cuda.empty_cache()
    print(f"r512_4096x3968: {rep['seconds']:.2f} s, debug workspace {rep['workspace_bytes']} bytes")


def _union(pkg, lib, dev, names):
    return set().union(*(_run(pkg, lib, dev, n) for n in names))


def test_fp32_cases_run_all_eleven_small_tiles(pkg, lib, dev):
    """the 11 MIGAN_GEOMETRIES_SMALL kernels of slice (f16x2, fp32), by name"""
    ran = _union(pkg, lib, dev, GPU_F32)
    want = {
        "migan::sepconv_kernel<0, 32, 128, 32, false, 3, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<3, 32, 128, 32, false, 1, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<2, 64, 128, 32, false, 4, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<0, 32, 128, 64, false, 5, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<3, 32, 128, 64, false, 2, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<2, 64, 128, 64, false, 7, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<2, 32, 128, 32, false, 2, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<2, 32, 128, 64, false, 4, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<0, 32, 32, 64, false, 5, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<3, 32, 32, 64, false, 2, 2, false, false, 2, false, 0>",
        "migan::sepconv_kernel<2, 32, 32, 64, false, 4, 2, false, false, 2, false, 0>",
    }
    assert want <= ran, sorted(want - ran)


@pytest.mark.parametrize("stv", [1, 2])
def test_16bit_cases_run_all_eleven_small_tiles(pkg, lib, dev, stv):
    """the 11 of slice (f16, bf16) and the 11 of slice (f16, fp16).  The default-knob cases reach six of each (K-split and KC-64 32-row
    tiles); the KC-32 tiles and the 64-row FIR-up tiles need the knob variants of GPU_16BIT_KNOBS"""
    ran = _union(pkg, lib, dev, list(GPU_16BIT) + list(GPU_16BIT_KNOBS))
    want = {
        f"migan::sepconv_kernel<0, 32, 128, 32, false, 3, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<3, 32, 128, 32, false, 1, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<2, 64, 128, 32, false, 4, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<0, 32, 128, 64, false, 5, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<3, 32, 128, 64, false, 2, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<2, 64, 128, 64, false, 7, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<2, 32, 128, 32, false, 2, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<2, 32, 128, 64, false, 4, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<0, 32, 32, 64, false, 5, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<3, 32, 32, 64, false, 2, 2, false, false, 3, false, {stv}>",
        f"migan::sepconv_kernel<2, 32, 32, 64, false, 4, 2, false, false, 3, false, {stv}>",
    }
    assert want <= ran, sorted(want - ran)


def test_control_cases_run_no_small_tile(pkg, lib, dev):
    """small = 0, and the f16x2 slice of 16-bit storage, which has no small tiles: the regular multi-image tiles at the same sizes"""
    for name in ("r32_b1_small0", "r32_b1_bf16_f16x2"):
        ran = _run(pkg, lib, dev, name)
        assert ran and not [s for s in ran if is_small(s)], (name, sorted(ran))


def test_64x64_falls_through_the_ksplit_tile(pkg, lib, dev):
    """R = 64, batch 1: the 32 x 32 K-split tile would need 2048 workgroups at 64 x 64 (over small_max_wgs), so the two 64 x 64 layers that
    take small tiles run the next one, the 32-row KC-64 tile; the layers below still run the K-split tiles"""
    _run(pkg, lib, dev, "r64_b1")
    by_layer = {}
    for row in REPORT["r64_b1"]["rows"]:
        by_layer[row["unit"]] = row["kernels"]
    assert by_layer["synthesis.b64.conv1"] == ["migan::sepconv_kernel<2, 32, 128, 64, false, 4, 2, false, false, 2, false, 0>"]
    assert by_layer["synthesis.b64.conv2"] == ["migan::sepconv_kernel<0, 32, 128, 64, false, 5, 2, false, false, 2, false, 0>"]
    assert by_layer["synthesis.b32.conv1"] == ["migan::sepconv_kernel<2, 32, 32, 64, false, 4, 2, false, false, 2, false, 0>"]
    assert by_layer["synthesis.b32.conv2"] == ["migan::sepconv_kernel<0, 32, 32, 64, false, 5, 2, false, false, 2, false, 0>"]
