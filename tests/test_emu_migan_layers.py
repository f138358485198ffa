"""CPU execution (fiber SIMT emulator, tests/emu) of the MI-GAN layer-isolating check (tests/migan_layers_case.py): every launch of a
debug plan against the oracle on the device's own input tap.  No GPU involved.  Run with -s for the per-unit table; measured figures:
profiles/migan_layers.md.

The emulator executes Generator(16): 4 x 4, 8 x 8 and 16 x 16 layers of 512 channels, which is where the small-launch tiles run.  What the
larger GPU cases launch is a pure host decision, so their symbol coverage is checked here as well, on dry runs (tests/launch_stream.py)."""
import re

import pytest

from tests import launch_stream as ls
from tests.emu_util import emu_lib
from tests.knobs import knobs
from tests.migan_layers_case import EMU_CASES, GPU_16BIT, GPU_16BIT_KNOBS, GPU_CASES, GPU_F32, SMALL_TILES, is_small, run_case, small_symbols
from tests.sepconv_case import HostMem


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


RAN = {}


@pytest.mark.parametrize("name", sorted(EMU_CASES))
def test_every_launch_in_isolation(pkg, lib, name):
    RAN[name] = run_case(lib, pkg, HostMem(), tag=name, **EMU_CASES[name])


def test_emulator_cases_run_small_tiles(pkg, lib):
    """the cases above ran K-split, 32-row and 64-row FIR-up small tiles of two slices, not only regular ones"""
    for name in sorted(EMU_CASES):
        if name not in RAN:
            RAN[name] = run_case(lib, pkg, HostMem(), tag=name, **EMU_CASES[name])
    f32 = RAN["r16_b1"] | RAN["r16_b2"] | RAN["r16_b1_kc32_up64"]
    for sym in ("migan::sepconv_kernel<0, 32, 32, 64, false, 5, 2, false, false, 2, false, 0>",
                "migan::sepconv_kernel<3, 32, 32, 64, false, 2, 2, false, false, 2, false, 0>",
                "migan::sepconv_kernel<2, 32, 32, 64, false, 4, 2, false, false, 2, false, 0>",
                "migan::sepconv_kernel<0, 32, 128, 32, false, 3, 2, false, false, 2, false, 0>",
                "migan::sepconv_kernel<3, 32, 128, 32, false, 1, 2, false, false, 2, false, 0>",
                "migan::sepconv_kernel<2, 64, 128, 32, false, 4, 2, false, false, 2, false, 0>"):
        assert sym in f32, (sym, sorted(f32))
    assert RAN["r16_b1_bf16"] & small_symbols(3, 1), sorted(RAN["r16_b1_bf16"])
    assert RAN["r16_12x20_b1"] == set()          # (launch_info does not report a forward at another size)


def _symbol(logged):
    """the emulator logs a kernel's signature: "void migan::k<...>(migan::Args)" -> "migan::k<...>", the name launch_info gives"""
    return re.sub(r"\(migan::\w+\)$", "", logged[5:] if logged.startswith("void ") else logged)


def _dry_symbols(lib, case):
    """symbols a forward of `case` launches, from a dry run of the same plan (debug plan, one stream, the case's knobs)"""
    with knobs(lib, **case.get("knobs", {})):
        h = ls.generator(lib, ls.Weights(), case["res"], storage=case.get("storage", "f32"), gemm=case.get("gemm"), streams=1, debug=True)
        with ls.dry_run(lib):
            if "hw" in case:
                out = ls.step(lib, h, "hw", case["batch"], hw=case["hw"])
                layers = []
                names = {_symbol(row[0]) for row in out["launches"]}
            else:
                out = ls.step(lib, h, "forward", case["batch"])
                names = {i["kernel"] for i in out["after"]}
                layers = [(i["layer"], i["kernel"]) for i in out["after"]]
                assert {_symbol(row[0]) for row in out["launches"]} - names <= {"migan::split_weights_kernel", "migan::weight_absmax_kernel"}
        h.close()
    return names, layers


def test_gpu_cases_cover_every_small_tile_symbol(pkg, lib):
    """What tests/test_gpu_migan_layers.py asserts about the symbols of its cases, on dry runs of the same plans: the 22 + 11 small-launch
    kernels are all reached, the control case reaches none, the R = 64 case falls through the K-split tile at 64 x 64."""
    got, got_layers = {}, {}
    for name, case in GPU_CASES.items():
        got[name], got_layers[name] = _dry_symbols(lib, case)
    f32 = set().union(*(got[n] for n in GPU_F32))
    assert small_symbols(2, 0) <= f32, sorted(small_symbols(2, 0) - f32)
    b16 = set().union(*(got[n] for n in list(GPU_16BIT) + list(GPU_16BIT_KNOBS)))
    assert small_symbols(3, 1) <= b16, sorted(small_symbols(3, 1) - b16)
    assert small_symbols(3, 2) <= b16, sorted(small_symbols(3, 2) - b16)
    assert not [s for s in got["r32_b1_small0"] if is_small(s)]
    assert not [s for s in got["r32_b1_bf16_f16x2"] if is_small(s)]
    # 64 x 64 at batch 1: 512 K-split tiles would be 2048 workgroups, over small_max_wgs, so the next small tile runs
    at64 = {k for l, k in got_layers["r64_b1"] if l in ("synthesis.b64.conv1", "synthesis.b64.conv2")}
    assert at64 == {"migan::sepconv_kernel<2, 32, 128, 64, false, 4, 2, false, false, 2, false, 0>",
                    "migan::sepconv_kernel<0, 32, 128, 64, false, 5, 2, false, false, 2, false, 0>"}, at64
    # the ragged FIR-up small tiles at H x W (3 x 5, 6 x 10, 12 x 20 inputs), which launch_info cannot show after forward_hw
    for name in ("r64_48x80_b1", "r64_48x80_b2"):
        assert got[name] & small_symbols(2, 0, [t for t in SMALL_TILES if t.startswith("2, ")]), sorted(got[name])


def test_debug_tensor_hw_describes_the_plan_at_h_by_w(pkg, lib):
    """migan_debug_tensor_hw: host code only.  At H = W = R the answer of migan_debug_tensor; at another size the layer's own shape, offsets
    inside the workspace of that size, in launch order and not overlapping; the refusals of migan_debug_tensor and migan_forward_hw."""
    h = ls.generator(lib, ls.Weights(), 16, streams=1, debug=True)
    names = ["encoder.b16.conv1", "encoder.b16.conv2", "encoder.b4.conv2", "synthesis.b4.img", "synthesis.b8.conv1", "synthesis.b16.conv2"]
    for batch in (1, 3):
        for name in names:
            assert h.debug_tensor_hw(batch, 16, 16, name) == h.debug_tensor(batch, name)
    assert h.debug_tensor_hw(2, 12, 20, "encoder.b16.conv1")[1] == (2, 12, 20, 512)
    assert h.debug_tensor_hw(2, 12, 20, "encoder.b16.conv2")[1] == (2, 6, 10, 512)
    assert h.debug_tensor_hw(2, 12, 20, "synthesis.b8.img")[1] == (2, 3, 6, 10)
    need = h.workspace_bytes_hw(2, 12, 20)
    spans = []
    for name in ("encoder.b16.conv2", "encoder.b8.conv2", "encoder.b4.conv2", "synthesis.b4.conv1", "synthesis.b4.conv2", "synthesis.b4.img",
                 "synthesis.b8.conv1", "synthesis.b8.conv2", "synthesis.b8.img", "synthesis.b16.conv1", "synthesis.b16.conv2"):
        off, shape = h.debug_tensor_hw(2, 12, 20, name)
        spans.append((off, off + 4 * shape[0] * shape[1] * shape[2] * shape[3]))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= need, (spans, need)
    with pytest.raises(ValueError, match="no such debug tensor"):
        h.debug_tensor_hw(1, 12, 20, "synthesis.b16.img")          # (the last image is y)
    with pytest.raises(ValueError, match="multiples of resolution / 4"):
        h.debug_tensor_hw(1, 12, 18, "encoder.b16.conv1")
    with pytest.raises(ValueError, match="empty batch"):
        h.debug_tensor_hw(0, 12, 20, "encoder.b16.conv1")
    h.set_debug(False)
    with pytest.raises(pkg.hipbind.MiganError, match="migan_set_debug"):
        h.debug_tensor_hw(1, 12, 20, "encoder.b16.conv1")
    h.close()
