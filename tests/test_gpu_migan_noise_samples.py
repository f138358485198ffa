"""MI-GAN: S completions per image from per-row noise (tests/migan_noise_samples_case.py) on a real MI355X: every kernel family's per-row
form inside the generator and alone, the reference golden, the host guards, the module API and MIGAN_Pipeline around NoiseSampler."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests.knobs import knobs
from tests.migan_noise_samples_case import (check_const_noise_gives_forward_bits, check_host_guards, check_rows_are_independent,
                                            check_single_image_runs_the_k_split_rows_form, run_rows_sepconv_case)
from tests.sepconv_case import CudaMem
from tests.test_convert import training_case

pytestmark = pytest.mark.gpu
ROWS = {"sep": "migan::sepconv_rows_kernel<", "wide": "migan::sepconv_wide_rows_kernel<", "pipe": "migan::sepconv_pipe_rows_kernel<",
        "wide2": "migan::sepconv_wide2_rows_kernel<"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# 1 + 2.  Generator(512) at 128 x 128, its smallest input, reaches the pipelined, wide and small-tile families (tests/last_store_case.py);
# 128 x 256 gives a non-square tile grid; Generator(64) runs the multi-image and small tiles; S = 1: rows = images.
@pytest.mark.parametrize("res,hw,n,s,dtype", [
    (512, (128, 128), 2, 3, "f32"), (512, (128, 256), 2, 3, "f32"), (512, (128, 128), 2, 3, "bf16"),
    (64, (64, 64), 3, 2, "f32"), (64, (64, 64), 3, 2, "bf16"), (64, (64, 64), 2, 1, "f32"), (64, (64, 64), 3, 2, "f16"),
])
def test_const_noise_gives_forward_bits_and_rows_are_independent(pkg, lib, dev, res, hw, n, s, dtype):
    g, x, _ = check_const_noise_gives_forward_bits(pkg, lib, CudaMem(dev), res, hw, n, s, dtype=dtype)
    if s >= 2:
        check_rows_are_independent(pkg, g, x, s)


def test_pipelined_and_wide2_forms_inside_the_generator(pkg, lib, dev):
    """with the thresholds of the persistent families at 1 tile, the 128 x 128 forward of Generator(512) runs them (pipe_min_tiles: the
    pipelined plain / ToRGB / FIR-up forms; w2_min_tiles: the 256-column persistent tile) in the plain forward and in the samples forward"""
    with knobs(lib, pipe_min_tiles=1, w2_min_tiles=1):
        g, x, _ = check_const_noise_gives_forward_bits(pkg, lib, CudaMem(dev), 512, (128, 128), 2, 2, seed=33)
        assert lib.last_kernel().startswith("migan::sepconv_pipe_kernel<"), lib.last_kernel()
        check_rows_are_independent(pkg, g, x, 2)


def test_sub_batches_on_two_streams_split_between_images(pkg, lib, dev):
    check_const_noise_gives_forward_bits(pkg, lib, CudaMem(dev), 64, (64, 64), 5, 4, streams=2)       # 20 rows: images 3 + 2


# the library's default of two streams: 16 and 18 rows split into 1 + 1 and 2 + 1 images, and a one-image sub-batch must keep the forms of
# the batch; 17 images x 2: the forward runs 8 + 9 images, the samples call its once-per-image launches for all 17 and its rows as 9 + 8
@pytest.mark.parametrize("res,hw,n,s", [(64, (64, 64), 2, 8), (64, (64, 64), 3, 6), (512, (128, 128), 2, 8), (64, (64, 64), 17, 2)])
def test_a_sub_batch_of_one_image_keeps_the_forms_of_the_batch(pkg, lib, dev, res, hw, n, s):
    check_const_noise_gives_forward_bits(pkg, lib, CudaMem(dev), res, hw, n, s)


@pytest.mark.parametrize("res,dtype", [(64, "f32"), (64, "bf16"), (128, "f32")])
def test_single_image_several_samples_run_the_k_split_rows_form(pkg, lib, dev, res, dtype):
    """n = 1, S = 3, the pipeline's ordinary last chunk: the single image's forms, the 32 x 32 K-split tile among them, with three rows"""
    check_single_image_runs_the_k_split_rows_form(pkg, lib, CudaMem(dev), res, 3, dtype=dtype)


# 3.  the reference's training generator, noise_mode='random', the draw recorded (tests/golden/make_golden_noise_samples.py)
def test_reference_training_generator_with_the_recorded_draw(pkg, dev, golden_dir):
    conv = importlib.import_module("mi-gan_amd.convert")
    g = np.load(os.path.join(golden_dir, "noise_samples_r64.npz"))
    _, res, _, train = training_case(pkg, golden_dir, "r64")
    n, s = int(g["n"]), int(g["samples"])
    bound = min(1e-4 * max(1.0, float(g["y_absmax"])), 1e-3)                 # tests/test_gpu_round2.py, this model pair
    gap = float(np.abs(g["y"] - g["y_const"]).max())
    assert gap > 10.0 * bound, (gap, bound)                                   # a forward that ignored the blobs could not pass
    m = pkg.Generator(resolution=res)
    m.load_state_dict(conv.convert_training_state_dict(train, res), strict=True)
    m = m.to(dev).eval()
    x, noise = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["noise"]).to(dev)
    assert tuple(noise.shape) == (n, s, m.noise_floats())
    with torch.no_grad():
        y = m.forward_noise_samples(x, noise)
        y1 = m(x)
    assert tuple(y.shape) == (n, s, 3, res, res)
    err = float(np.abs(y.reshape(n * s, 3, res, res).cpu().numpy() - g["y"]).max())
    print(f"noise samples vs the training generator: max abs err {err:.3e}, bound {bound:.3e}, random vs const {gap:.3e}")
    assert err <= 1e-4 * max(1.0, float(g["y_absmax"])), err
    assert err <= 1e-3
    # the module's own blob gives the module's forward; a drawn blob gives S different completions
    with torch.no_grad():
        yc = m.forward_noise_samples(x, m.const_noise()[None, None].expand(n, s, -1).contiguous())
        yr = m.forward_noise_samples(x, samples=3)
    for k in range(s):
        assert torch.equal(yc[:, k], y1)
    assert tuple(yr.shape) == (n, 3, 3, res, res) and not torch.equal(yr[:, 0], yr[:, 1])
    with pytest.raises(RuntimeError):
        m.forward_noise_samples(x, noise[:, :, :-1].contiguous())
    with pytest.raises(RuntimeError):
        m.forward_noise_samples(x)


# 4.  each family alone, through migan_sepconv_forward_samples, against the oracle row by row.  Shapes: the smallest at which each form exists
# (tests/sepconv_matrix.py, tests/test_gpu_round2.py); batch 4 = 2 images x 2 samples
@pytest.mark.parametrize("family,case", [
    ("sep", dict(cin=64, cout=128, h=4, up=2, skip=True)),                           # two rows per tile, FIR-up
    ("sep", dict(cin=64, cout=128, h=8, skip=True)),                                 # two rows per tile, plain
    ("sep", dict(cin=64, cout=128, h=8, skip=True, n=1, s=3)),                       # ... a tile that straddles nothing but is ragged in the batch
    ("sep", dict(cin=64, cout=128, h=16, up=2, skip=True)),                          # main tile, FIR-up
    ("sep", dict(cin=64, cout=128, h=16, w=32)),                                     # main tile, plain, no skip
    ("sep", dict(cin=32, cout=64, h=6, w=10, skip=True)),                            # ragged run-time tile
    ("sep", dict(cin=64, cout=64, h=16, torgb=True, with_prev=True)),                # fused ToRGB, previous image per row
    ("sep", dict(cin=64, cout=128, h=16, noise=False, skip=True)),                   # skip without noise
    ("sep", dict(cin=64, cout=128, h=16, up=2, skip=True, storage="bf16")),
    ("sep", dict(cin=64, cout=128, h=16, skip=True, storage="f16")),
    ("wide", dict(cin=64, cout=256, h=16, skip=True)),                               # 128 x 256 tile, plain
    ("wide", dict(cin=64, cout=256, h=16, up=2, skip=True)),                         # ... FIR-up (wide_up)
    ("wide", dict(cin=64, cout=256, h=16, up=2)),
    ("wide", dict(cin=64, cout=256, h=16, storage="bf16", skip=True)),
])
def test_each_family_alone(pkg, lib, dev, family, case):
    kw = dict(case)
    gemm = 2 if kw.get("storage", "f32") == "f32" else -1
    run_rows_sepconv_case(lib, pkg, CudaMem(dev), gemm=gemm, symbol=ROWS[family], **kw)


@pytest.mark.parametrize("family,case", [
    ("pipe", dict(cin=64, cout=64, h=32)),                                           # pipelined plain
    ("pipe", dict(cin=64, cout=64, h=32, torgb=True, with_prev=True)),               # ... + fused ToRGB
    ("pipe", dict(cin=128, cout=128, h=32)),                                         # ... 128-column tiles
    ("pipe", dict(cin=128, cout=64, h=16, w=32, up=2, skip=True)),                   # pipelined FIR-up, skip per image
    ("pipe", dict(cin=128, cout=64, h=16, up=2)),
    ("wide2", dict(cin=64, cout=256, h=32)),                                         # 256 x 256 persistent tile
    ("wide2", dict(cin=128, cout=512, h=16, w=32)),
])
def test_each_persistent_family_alone(pkg, lib, dev, family, case):
    """the persistent families take a launch from 256 tiles on; with the thresholds at 1 these small layers run them: several tiles per
    workgroup at pipe_grid = 8, so that the tile walk crosses rows and images"""
    with knobs(lib, pipe_min_tiles=1, w2_min_tiles=1, pipe_grid=8):
        run_rows_sepconv_case(lib, pkg, CudaMem(dev), gemm=2, symbol=ROWS[family], **case)


# 5.  host guards; the symbols in both libraries
def test_host_guards(pkg, lib, dev):
    check_host_guards(pkg, lib, CudaMem(dev), res=64)


def test_both_libraries_export_the_entries(pkg):
    build = importlib.import_module("mi-gan_amd.build")
    for path in (build.OUT, build.NAN_CLAMP_OUT):
        L = pkg.hipbind.MiganLib(path)                   # (refuses a library that lacks one of hipbind's export lists)
        for name in pkg.hipbind.exports("migan_noise_samples_hip.h"):
            assert hasattr(L.lib, name), (path, name)


# 6.  MIGAN_Pipeline around NoiseSampler: forward_samples == pre -> model.forward_samples -> the batch post, by hand
def test_pipeline_serves_samples_with_the_noise_sampler(pkg, lib, dev):
    from tests.test_gpu_pipeline_samples import PADDING, RES, _device_items, _post_on_copies, _pre
    sd = pkg.synth.make_state_dict(RES, seed=1, regime="export")
    m = pkg.Generator(resolution=RES)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    assert not hasattr(m, "forward_samples")
    sampler = pkg.migan_inference.NoiseSampler(m)
    pipe = pkg.pipeline.MIGAN_Pipeline(sampler, RES, padding=PADDING, device=dev)
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(53)
    samples = 2
    sizes = [(96, 80), (70, 131), (97, 83)]
    holes = [(slice(30, 50), slice(20, 45)), (slice(50, 70), slice(100, 131)), (slice(20, 71), slice(25, 55))]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(sz, 255, dtype=np.uint8) for sz in sizes]
    for mk, hole in zip(masks, holes):
        mk[hole] = 0
    d_img, d_mask = _device_items(images, masks, dev)
    z = torch.randn(3, samples, sampler.z_dim, generator=torch.Generator().manual_seed(53)).to(dev)
    items, scratch, bbox, x = _pre(lib, d_img, d_mask, dev, stream)
    with torch.no_grad():
        y = pipe.model.forward_samples(x, z).reshape(3 * samples, 3, RES, RES).contiguous()
    want = _post_on_copies(lib, d_img, d_mask, scratch, bbox, y, samples, pipe._gauss, stream)
    outs, boxes = pipe.forward_samples(d_img, d_mask, z, return_bbox=True)
    assert torch.equal(boxes, bbox)
    for i in range(3):
        assert outs[i].shape == (samples, 3) + sizes[i] and outs[i].dtype == torch.uint8
        assert torch.equal(d_img[i].cpu(), torch.from_numpy(images[i])[None]), f"photo {i} was written"
        for k in range(samples):
            assert torch.equal(outs[i][k], want[i][k]), f"item {i}, sample {k}"
        # (different blobs: different completions.  Checked on the generator's rows: with synthetic weights most pixels of y saturate the
        # uint8 range, so two completions may well agree in every byte of a small hole)
        assert not torch.equal(y[i * samples], y[i * samples + 1])
    patches, pboxes = pipe.forward_patches(d_img, d_mask, z)
    for i in range(3):
        x0, x1, y0, y1 = pboxes[i].tolist()
        assert torch.equal(patches[i], outs[i][:, :, y0:y1, x0:x1])
    drawn = pipe.forward_samples(d_img, d_mask, samples=2, max_rows=4)           # z drawn by the pipeline (on the CPU: fine at 64)
    assert [tuple(o.shape) for o in drawn] == [(2, 3) + sz for sz in sizes]
