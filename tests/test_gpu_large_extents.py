"""Every kernel family behind migan_sepconv_forward once at the edge of its stated range: per-image tensors of (just under) 2^30 - 1024
elements, the extent limit of migan_host.hpp, and whole batches above 2^32 bytes.  The error a kernel can make here is a function of the
byte offset, not of the workload: 32-bit lane offsets, int element indices, signed casts on buffer offsets above 2^31, the scalar window
offset of the pipelined kernels, and the out-of-range marker that fetches padding pixels.  tests/large_extent_case.py keeps the tensors on
the device and judges row windows with the float64 oracle; see there for the windows, the bounds and the band-consistency pass.
profiles/large_extents.md records what each case measured."""
import pytest
import torch

from tests import sepconv_matrix as mx
from tests.knobs import knobs
from tests.large_extent_case import run_batch_case, run_large_case

pytestmark = pytest.mark.gpu

LIMIT = 2 ** 30 - 1024            # kMaxImageElems


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def largest_hw(w_near, cin, cout, down=1, up=1, hm=1, wm=1, odd=False):
    """the input size (h a multiple of hm, w a multiple of wm within 256 columns below w_near; h odd where asked) with the most pixels
    whose widest tensor stays within the limit"""
    per_pixel = max(cin, cout // 4 if down == 2 else (cout * 4 if up == 2 else cout))        # elements per INPUT pixel of the widest tensor
    best = None
    for w in ([w_near] if wm == 1 else range(w_near // wm * wm, w_near - 256, -wm)):
        h = (LIMIT // per_pixel) // w // hm * hm
        h -= 1 if odd and h % 2 == 0 else 0
        if best is None or h * w > best[0] * best[1]:
            best = (h, w)
    assert best[0] * best[1] * per_pixel <= LIMIT
    return best


F = lambda **kw: dict(dict(skip=False, noise=False, torgb=False, with_prev=False, fromrgb=False), **kw)
PIPE64 = lambda f: mx.expected(mx.ROW["pipe64"], f, "f32")[1]
PIPE128 = lambda f: mx.expected(mx.ROW["pipe128"], f, "f32")[1]
RAGGED = dict(odd=True)                      # W = 4090 (or half of it) with odd H: a ragged right and bottom edge
EVEN = dict(hm=2)
T8x16, T16x16, T8x32, T32x32, T32x64 = dict(hm=8, wm=16), dict(hm=16, wm=16), dict(hm=8, wm=32), dict(hm=32, wm=32), dict(hm=32, wm=64)
T16x32 = dict(hm=16, wm=32)                  # down=2: whole 8 x 16 tiles of the output

# (id, layer, width to start from, size rule, flags, storage, kernel, knobs).  The families that take whole tiles only (the plain and down=2
# pipelined kernels, the 256-column tiles) get the whole-tile size with the most pixels; the others W = 4096 and the ragged W = 4090.
CASES = [
    # ---- pipelined
    ("pipe64-noise", dict(cin=64, cout=64), 4096, T8x16, F(noise=True), "f32", PIPE64(F(noise=True)), {}),
    ("pipe64-torgb-prev", dict(cin=64, cout=64), 4096, T8x16, F(torgb=True, with_prev=True), "f32", PIPE64(F(torgb=True, with_prev=True)), {}),
    ("pipe64-fromrgb", dict(cin=64, cout=64), 4096, T8x16, F(fromrgb=True), "f32", PIPE64(F(fromrgb=True)), {}),
    ("pipe128", dict(cin=128, cout=128), 4096, T8x16, F(), "f32", PIPE128(F()), {}),
    ("pipe128-torgb", dict(cin=128, cout=128), 4096, T8x16, F(torgb=True), "f32", PIPE128(F(torgb=True)), {}),
    ("pipe-up", dict(cin=128, cout=64, up=2), 2048, {}, F(noise=True, skip=True), "f32", mx.pipe(2, 64, 128, False, False, 2, 4), {}),
    ("pipe-up-ragged", dict(cin=128, cout=64, up=2), 2045, RAGGED, F(noise=True, skip=True), "f32", mx.pipe(2, 64, 128, False, False, 2, 4), {}),
    ("pipedown", dict(cin=64, cout=128, down=2), 4096, T8x32, F(), "f32", mx.PIPEDOWN, {}),
    ("pipedown256", dict(cin=128, cout=256, down=2), 4096, T8x32, F(), "f32", mx.PIPEDOWN256, {}),
    # ---- the one-tile kernel
    # (whole tiles: the MAING instantiation, whose epilogue has no bounds checks; ragged: the run-time tile)
    ("tile-skip", dict(cin=64, cout=64), 4096, T8x16, F(skip=True), "f32", mx.tile(0, 64, False, 6, 3, True, False, 0), {}),
    ("tile-skip-ragged", dict(cin=64, cout=64), 4090, RAGGED, F(skip=True), "f32", mx.tile(0, 64, False, 9, 2, False, False, 0), {}),
    ("tile-up", dict(cin=64, cout=128, up=2), 2048, {}, F(noise=True), "f32", mx.tile(2, 128, False, 6, 2, True, False, 0), {}),
    ("tile-up-ragged", dict(cin=64, cout=128, up=2), 2045, RAGGED, F(noise=True), "f32", mx.tile(2, 128, False, 6, 2, True, False, 0), {}),
    ("dwfir-pw", dict(cin=64, cout=64, down=2), 4096, T16x32, F(skip=True), "f32", mx.tile(3, 64, False, 4, 2, True, False, 0), {}),
    ("dwfir-pw-ragged", dict(cin=64, cout=64, down=2), 4090, EVEN, F(skip=True), "f32", mx.tile(3, 64, False, 4, 2, False, False, 0), {}),
    ("persist-pw", dict(cin=128, cout=256, down=2), 4096, T32x64, F(skip=True), "f32", mx.tile(3, 128, False, 4, 2, True, False, 0, persist=True), {}),
    # ---- 256-column tiles
    ("wide-skip", dict(cin=64, cout=256), 2048, T8x16, F(skip=True), "f32", mx.wide(False, 0), {}),
    ("wide-up", dict(cin=64, cout=256, up=2), 1024, {}, F(noise=True), "f32", mx.WIDE_UP, {}),
    ("wide-up-ragged", dict(cin=64, cout=256, up=2), 1022, RAGGED, F(noise=True), "f32", mx.WIDE_UP, {}),
    ("wide2", dict(cin=64, cout=256), 2048, T16x16, F(noise=True), "f32", mx.WIDE2, {}),
    ("wide2-512", dict(cin=512, cout=512), 2048, T16x16, F(), "f32", mx.WIDE2, {}),
    ("wide2-pw", dict(cin=64, cout=256, down=2), 4096, T32x32, F(), "f32", mx.WIDE2_PW, {}),
    ("torgb-unfused", dict(cin=64, cout=192), 2048, T8x16, F(torgb=True, with_prev=True), "f32", mx.tile(0, 64, False, 6, 3, True, False, 0), {}),
    # ---- fewer than 64 channels
    ("narrow-plain", dict(cin=32, cout=32), 4096, {}, F(noise=True), "f32", "migan::narrow_sepconv_kernel<0, false>", {}),
    ("narrow-down", dict(cin=16, cout=32, down=2), 4090, EVEN, F(), "f32", "migan::narrow_sepconv_kernel<1, false>", {}),
    ("narrow-up", dict(cin=64, cout=32, up=2), 2045, RAGGED, F(skip=True), "f32", "migan::narrow_sepconv_kernel<2, false>", {}),
    # ---- 16-bit storage: the element limit binds, at 2^31 bytes
    ("bf16-plain", dict(cin=64, cout=64), 4096, T8x16, F(noise=True), "bf16", mx.tile(0, 64, False, 6, 3, True, False, 1), {}),
    ("bf16-plain-ragged", dict(cin=64, cout=64), 4090, RAGGED, F(noise=True), "bf16", mx.tile(0, 64, False, 9, 2, False, False, 1), {}),
    ("f16-up", dict(cin=64, cout=128, up=2), 2045, RAGGED, F(skip=True), "f16", mx.tile(2, 128, False, 6, 2, True, False, 2), {}),
    ("bf16-wide", dict(cin=64, cout=256), 2048, T8x16, F(skip=True), "bf16", mx.wide(False, 1), {}),
]

REPORT = []


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for r in REPORT:
        print("| " + " | ".join(str(v) for v in r) + " |")


@pytest.mark.parametrize("name,layer,w_near,rule,flags,storage,kernel,kn", CASES, ids=[c[0] for c in CASES])
def test_large_extent(lib, pkg, dev, name, layer, w_near, rule, flags, storage, kernel, kn):
    h, w = largest_hw(w_near, layer["cin"], layer["cout"], layer.get("down", 1), layer.get("up", 1), **rule)
    with knobs(lib, **kn):
        r = run_large_case(lib, pkg, dev, h=h, w=w, storage=storage, kernel=kernel, **layer, **flags)
    REPORT.append((name, f"{h}x{w}", r["kernel"], r["image_bytes"], r["image_bytes"], f"{r['window']:.3f}", f"{r['band']:.3f}", f"{r['seconds']:.1f}"))
    print(REPORT[-1])


def test_per_row_form_with_the_last_row_above_4gib(lib, pkg, dev):
    """migan_sepconv_forward_samples, pipelined FIR-up rows at n = 1, S = 3 and the largest ragged size: a row of y is 4102 x 4090 x 64
    floats, 9216 bytes short of 2^32, so byte 2^32 of the batch falls in the first output row of row 1 and row 2 lies wholly above it
    (from byte 2^33 - 18432 on).  Its noise plane is the third of the blob: a plane is at most 2^24 - 16 pixels here, 64 MiB, and cannot
    itself lie above 2^32 bytes.  The bands run the per-row kernel too (S = 1, the row's own plane)."""
    layer = dict(cin=128, cout=64, up=2)
    h, w = largest_hw(2045, **layer, **RAGGED)
    assert 0 < (1 << 32) - 2 * h * 2 * w * 64 * 4 < 2 * w * 64 * 4
    r = run_large_case(lib, pkg, dev, h=h, w=w, rows=3, kernel_prefix="migan::sepconv_pipe_rows_kernel<2, 64, 128,", noise=True, skip=True, **layer)
    REPORT.append(("pipe-up-rows", f"3x{h}x{w}", r["kernel"], r["image_bytes"], 3 * r["image_bytes"], f"{r['window']:.3f}", f"{r['band']:.3f}", f"{r['seconds']:.1f}"))
    print(REPORT[-1])


# ---- whole batch above 2^32 bytes, small images: 64-bit image base plus 32-bit lane offset
BATCH_CASES = [
    ("batch-pipe64", dict(cin=64, cout=64), 512, 512, 72, F(noise=True), PIPE64(F(noise=True))),
    ("batch-tile-skip", dict(cin=64, cout=64), 512, 512, 72, F(skip=True), mx.tile(0, 64, False, 6, 3, True, False, 0)),
    ("batch-wide", dict(cin=64, cout=256), 256, 256, 72, F(skip=True), mx.wide(False, 0)),
    ("batch-two-images-per-tile", dict(cin=64, cout=128), 8, 8, 131075, F(skip=True), mx.tile(0, 128, False, 9, 2, False, False, 0)),
]


@pytest.mark.parametrize("name,layer,h,w,batch,flags,kernel", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_above_4gib(lib, pkg, dev, name, layer, h, w, batch, flags, kernel):
    r = run_batch_case(lib, pkg, dev, h=h, w=w, batch=batch, kernel=kernel, **layer, **flags)
    assert r["batch_bytes"] > 1 << 32
    REPORT.append((name, f"{batch}x{h}x{w}", r["kernel"], r["image_bytes"], r["batch_bytes"], f"{r['window']:.3f}", f"{r['band']:.3f}", f"{r['seconds']:.1f}"))
    print(REPORT[-1])


def test_the_sliver_is_refused(lib, pkg, dev):
    """4095 x 4097 x 64 fp32 is 2^32 - 256 bytes: below 2^32, so the earlier guard (elements < 2^30, bytes < 2^32) accepted it, but within
    4096 bytes of it.  The kernels fetch padding pixels at lane offset 0xfffff000 = 2^32 - 4096 and rely on the buffer descriptor's range
    check to return zeros; in an image of this size that offset is a real pixel (row 4094, column 4082), so every border tile would
    convolve it into its zero padding.  No kernel can run this size correctly: the limit is 2^30 - 1024 elements and the call is REFUSED,
    before any launch (y keeps its fill)."""
    h, w, c = 4095, 4097, 64
    assert LIMIT * 4 < h * w * c * 4 < 1 << 32
    small = torch.full((4096,), 7.5, device=dev)
    with pytest.raises(ValueError, match="too large"):
        lib.sepconv_forward(x=small.data_ptr(), y=small.data_ptr(), conv1_weight=small.data_ptr(), conv1_bias=small.data_ptr(),
                            conv2_weight=small.data_ptr(), batch=1, cin=c, cout=c, res_in=h, width_in=w, dtype=0)
    torch.cuda.synchronize()
    assert bool((small == 7.5).all())
