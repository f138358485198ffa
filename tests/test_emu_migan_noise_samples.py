"""MI-GAN: S completions per image from per-row noise (tests/migan_noise_samples_case.py) on the CPU emulator of the product's kernel
source: the host plan, the per-row addressing of the small-tile and multi-image forms, the row copies and the guards."""
import numpy as np
import pytest

from tests.emu_util import emu_lib
from tests.last_store_case import FILL
from tests.migan_noise_samples_case import (SamplesBound, check_const_noise_gives_forward_bits, check_host_guards, check_rows_are_independent,
                                            check_single_image_runs_the_k_split_rows_form, const_blob, run_rows_sepconv_case)
from tests.sepconv_case import HostMem


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def test_const_noise_gives_forward_bits_and_rows_are_independent(pkg, lib):
    """Generator(16), n = 2, S = 2: the 8 x 8 layers run two rows per tile (a tile spans two images' samples), the 16 x 16 ones the small tiles"""
    g, x, _ = check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (16, 16), 2, 2)
    check_rows_are_independent(pkg, g, x, 2)


def test_odd_sample_count_and_two_streams(pkg, lib):
    """S = 3 (a multi-image tile then straddles an image boundary at an odd row); 16 rows on two streams: sub-batches of 2 + 2 images"""
    check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (16, 16), 3, 3)
    check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (16, 16), 4, 4, streams=2)


@pytest.mark.parametrize("n,s", [(2, 8), (3, 6)])
def test_a_sub_batch_of_one_image_keeps_the_forms_of_the_batch(pkg, lib, n, s):
    """the library's default of two streams splits 16 and 18 rows into 1 + 1 and 2 + 1 images: the one-image sub-batch must not run the
    single-image (K-split) forms, which a forward of these n images runs for none of them"""
    check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (16, 16), n, s)


def test_single_image_several_samples(pkg, lib):
    """n = 1, S = 3: every form is the single image's, as in its forward, and the K-split per-row form runs with three rows"""
    check_single_image_runs_the_k_split_rows_form(pkg, lib, HostMem(), 16, 3)


def test_non_square_input(pkg, lib):
    g, x, _ = check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (8, 12), 2, 2)
    check_rows_are_independent(pkg, g, x, 2)


def test_bf16_storage(pkg, lib):
    check_const_noise_gives_forward_bits(pkg, lib, HostMem(), 16, (16, 16), 2, 2, dtype="bf16")


# the small-resolution forms of sepconv_kernel one by one: several rows per tile (4 x 4 -> 8 x 8 FIR-up: two images per tile; 8 x 8 plain:
# two images per tile), ragged tiles, the main 8 x 16 tile; with and without the skip tensor, which is per IMAGE
@pytest.mark.parametrize("case", [
    dict(cin=64, cout=128, h=4, up=2, skip=True, n=2, s=2),
    dict(cin=64, cout=128, h=4, up=2, skip=True, n=1, s=3),
    dict(cin=64, cout=128, h=8, skip=False, n=2, s=2),
    dict(cin=64, cout=128, h=8, skip=True, n=3, s=1),
    dict(cin=32, cout=64, h=8, w=16, up=2, skip=True, n=2, s=2),
    dict(cin=32, cout=64, h=6, w=10, skip=True, n=2, s=2),
    dict(cin=32, cout=64, h=8, w=16, torgb=True, with_prev=True, n=2, s=2),
    dict(cin=64, cout=128, h=8, noise=False, skip=True, n=2, s=2),
])
def test_each_small_form_alone(pkg, lib, case):
    run_rows_sepconv_case(lib, pkg, HostMem(), gemm=2, symbol="migan::sepconv_rows_kernel<", **case)


# the other families at their smallest shapes (the MI355X runs more of them: tests/test_gpu_migan_noise_samples.py): the 128 x 256 tile plain
# and FIR-up, and -- with their tile thresholds at 1 and 8 persistent workgroups, so that a workgroup's walk crosses rows and images -- the
# pipelined plain / ToRGB / FIR-up forms and the 256 x 256 persistent tile
@pytest.mark.parametrize("symbol,case", [
    ("migan::sepconv_wide_rows_kernel<", dict(cin=64, cout=256, h=8, w=16, skip=True)),
    ("migan::sepconv_wide_rows_kernel<", dict(cin=64, cout=256, h=8, w=16, up=2, skip=True)),
    ("migan::sepconv_pipe_rows_kernel<", dict(cin=64, cout=64, h=16, w=32, n=3, s=2)),
    ("migan::sepconv_pipe_rows_kernel<", dict(cin=64, cout=64, h=8, w=16, torgb=True, with_prev=True, n=3, s=2)),
    ("migan::sepconv_pipe_rows_kernel<", dict(cin=128, cout=64, h=8, w=16, up=2, skip=True, n=3, s=2)),
    ("migan::sepconv_wide2_rows_kernel<", dict(cin=64, cout=256, h=16, w=16, n=3, s=3)),
])
def test_each_other_family_alone(pkg, lib, symbol, case):
    from tests.knobs import knobs
    with knobs(lib, pipe_min_tiles=1, w2_min_tiles=1, pipe_grid=8):
        run_rows_sepconv_case(lib, pkg, HostMem(), gemm=2, symbol=symbol, **case)


def test_operator_entry_refuses_what_no_samples_forward_contains(pkg, lib):
    mem = HostMem()
    buf = np.zeros(64 * 64 * 64, np.float32)
    base = dict(x=mem.ptr(buf), y=mem.ptr(buf), conv1_weight=mem.ptr(buf), conv1_bias=mem.ptr(buf), conv2_weight=mem.ptr(buf), cin=64, cout=64,
                res_in=8, batch=4)
    for samples, change in [(0, {}), (-1, {}), (3, {}), (2, dict(down=2)), (2, dict(fromrgb_weight=mem.ptr(buf), fromrgb_bias=mem.ptr(buf))),
                            (2, dict(cin=16, cout=16))]:
        with pytest.raises(ValueError):                      # MIGAN_EINVAL
            lib.sepconv_forward(samples=samples, **dict(base, **change))
    assert not buf.any()


def test_host_guards(pkg, lib):
    check_host_guards(pkg, lib, HostMem())


def test_resolutions_above_512_are_unsupported_before_any_launch(pkg, lib):
    """narrow layers (fewer than 64 channels) have no per-row form: MIGAN_EUNSUPPORTED, nothing written"""
    g = SamplesBound(pkg, lib, HostMem(), 1024, seed=43)          # committed, with weights: nothing but the narrow layers stands in the way
    hh = ww = 256
    f = g.h.noise_floats_hw(hh, ww)
    assert f == sum(2 * (256 * r // 1024) ** 2 for r in (8, 16, 32, 64, 128, 256, 512, 1024))
    x = (pkg.synth.normal((1, 4, hh, ww), 43, "x1024") * 0.7).astype(np.float32)
    with pytest.raises(NotImplementedError, match="above 512"):     # MIGAN_EUNSUPPORTED
        g.forward_samples_hw(x, np.zeros((1, 2, f), np.float32))
    assert np.isnan(g.last_y).all(), "the refused call wrote y"
    assert (g.last_ws == FILL).all(), "the refused call wrote the workspace"


def test_python_blob_layout_matches_the_library(pkg, lib):
    """Generator.noise_floats / const_noise (pure torch, any device) spell the blob the C entry measures"""
    import torch
    m = pkg.Generator(resolution=32)
    sd = pkg.synth.make_state_dict(32, seed=7)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    h = pkg.hipbind.MiganHandle(lib, 32)
    for hw in (None, (8, 24), (40, 32)):
        hh, ww = hw or (32, 32)
        assert m.noise_floats(hw) == h.noise_floats_hw(hh, ww)
        np.testing.assert_array_equal(m.const_noise(hw).numpy(), const_blob(sd, 32, hw))
    with pytest.raises(RuntimeError):
        m.noise_floats((33, 32))
    assert not hasattr(m, "forward_samples")
    s = pkg.migan_inference.NoiseSampler(m)
    assert s.z_dim == m.noise_floats() and s.resolution == 32 and callable(s.forward_samples)
