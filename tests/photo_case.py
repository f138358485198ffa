"""Shared cases and the numpy restatement of the photo-loading tests (include/migan_photo_hip.h): tests/test_photo_oracle.py ties the
restatement to Pillow's own bytes (tests/golden/photo_*.npz, tests/golden/make_golden_photo.py, and live Pillow where installed),
tests/test_emu_photo.py and tests/test_gpu_photo.py run the cases through the C ABI, on the emulator (host memory) and on the device.
Every comparison is equality of bytes.  Test infrastructure only.

The restatement is Pillow's arithmetic for uint8 images (src/libImaging/Resample.c, Geometry.c), in numpy float64 one operation at a
time (numpy never fuses a multiply-add) and Python ints:
  BICUBIC  precompute_coeffs + normalize_coeffs_8bpc per axis, horizontal pass into a uint8 image, then vertical
  NEAREST  ImagingScaleAffine's repeated addition of the step
"""
import math
import os

import numpy as np

from tests.metrics_case import CudaMem, HostMem      # noqa: F401  (memory the library reads and writes: host arrays / device buffers)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEAREST, BICUBIC = 0, 1                    # MIGAN_PHOTO_NEAREST / _BICUBIC
INVERT, THRESHOLD = 1, 2                   # MIGAN_PHOTO_INVERT / _THRESHOLD
ITEMS_PER_LAUNCH = 32                      # kPhItemsMax of mi-gan_amd/csrc/migan_photo.hpp
TILE_W, TILE_R, ROW_BYTES = 64, 4, 4096    # kPhTW, kPhTR, kPhRowBytes
SRC_MAX, DST_MAX, ASPECT_MAX = 16384, 4096, 32
PRECISION_BITS = 22
GUARD, FILL = 16, 0xA5                     # bytes behind every destination, and what destinations hold before a call
EINVAL = 1


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_TABLES = {}


def coeffs(in_size, out_size):
    """(ksize, xmin [out], n [out], K [out, ksize] int64) of one axis; Python floats are IEEE doubles, one rounding per operation"""
    key = (in_size, out_size)
    if key in _TABLES:
        return _TABLES[key]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmins, ns, kk = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * 4194304.0) if k < 0 else int(0.5 + k * 4194304.0)
        xmins[xx], ns[xx] = xmin, n
    _TABLES[key] = (ksize, xmins, ns, kk)
    return _TABLES[key]


def worst_partial_sum(in_size, out_size):
    """the largest magnitude any left-to-right partial sum of the int32 accumulator can reach with bytes in 0 .. 255"""
    _, _, ns, kk = coeffs(in_size, out_size)
    worst = 0
    for xx in range(out_size):
        pos = neg = 1 << (PRECISION_BITS - 1)
        for k in kk[xx, :ns[xx]]:
            pos += 255 * max(int(k), 0)
            neg += 255 * min(int(k), 0)
            worst = max(worst, pos, -neg)
    return worst


def _resample_rows(img, out_size):
    """[A, inS, C] uint8 -> [A, outS, C] along axis 1"""
    _, xmins, ns, kk = coeffs(img.shape[1], out_size)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        x0, n = int(xmins[xx]), int(ns[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + n], kk[xx, :n], axes=([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)          # (numpy's >> on int64 is arithmetic)
    return out


def pil_bicubic(img, size):
    """Image.resize((w, h), Image.BICUBIC) of uint8 [H, W, 3] or [H, W]"""
    w, h = size
    a = img if img.ndim == 3 else img[:, :, None]
    if a.shape[1] != w:
        a = _resample_rows(a, w)
    if a.shape[0] != h:
        a = np.ascontiguousarray(_resample_rows(np.ascontiguousarray(a.transpose(1, 0, 2)), h).transpose(1, 0, 2))
    a = np.ascontiguousarray(a)
    return a.copy() if img.ndim == 3 else a[:, :, 0].copy()


def nearest_index(in_size, out_size):
    a0 = in_size / out_size
    xo = a0 * 0.5
    idx = np.empty(out_size, np.int64)
    for x in range(out_size):
        idx[x] = int(xo)
        xo += a0
    return idx


def closed_form_index(in_size, out_size):
    """floor((x + 0.5) * inS / outS): NOT Pillow's rule (the cases below count where it differs)"""
    return np.array([int(math.floor((x + 0.5) * in_size / out_size)) for x in range(out_size)], np.int64)


def pil_nearest(mask, size, flags=0):
    """Image.resize((w, h), Image.NEAREST) of uint8 [H, W] (or [H, W, 3]), then demo.py:42-44's inversion / threshold"""
    w, h = size
    out = mask[nearest_index(mask.shape[0], h)][:, nearest_index(mask.shape[1], w)].copy()
    if flags & INVERT:
        out = 255 - out
    if flags & THRESHOLD:
        out[out < 255] = 0
    return out


def fit_size(w, h, max_size):
    """demo.py:48-53"""
    if w > max_size or h > max_size:
        resize_ratio = max_size / w if w > h else max_size / h
        w, h = int(w * resize_ratio), int(h * resize_ratio)
    return w, h


def eval_flow(img, mask, r):
    """evaluate_fid_lpips.py:142-149"""
    if img.shape[1] != r or img.shape[0] != r:
        img = pil_bicubic(img, (r, r))
    return img, pil_nearest(mask, (r, r))


def demo_flow(img, mask, r, invert):
    """demo.py:125-130 with resize, read_mask (one-channel mask) and the two resizes of preprocess"""
    img = pil_bicubic(img, fit_size(img.shape[1], img.shape[0], r))
    mask = pil_nearest(mask, fit_size(mask.shape[1], mask.shape[0], 512), (INVERT if invert else 0) | THRESHOLD)
    mask = pil_nearest(mask, fit_size(mask.shape[1], mask.shape[0], r))
    return pil_bicubic(img, (r, r)), pil_nearest(mask, (r, r))


# ---- images ----------------------------------------------------------------------------------------------------------------------
def photo(h, w, seed, channels=3):
    """uint8 [H, W, 3]: a smooth pattern with noise on top and saturated patches (both clamps of an overshooting filter fire)"""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    c = np.arange(channels, dtype=np.float64)[None, None, :]
    v = 0.5 + 0.45 * np.sin(0.21 * yy[..., None] + 0.9 * c + 0.37 * seed) * np.cos(0.17 * xx[..., None] - 0.5 * c)
    v = v + 0.25 * (rng.random((h, w, channels)) - 0.5)
    out = np.rint(np.clip(v, 0.0, 1.0) * 255.0).astype(np.uint8)
    out[(yy.astype(np.int64) // 3 + xx.astype(np.int64) // 5) % 7 == 0] = 255 if seed % 2 else 0
    return out if channels == 3 else np.ascontiguousarray(out[:, :, 0])


def checkerboard(h, w):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2).copy()


def mask_image(h, w, seed):
    """uint8 [H, W]: known (255) with rectangular holes (0) and a band of every other value (compresses well at 600 x 450)"""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    m = np.full((h, w), 255, np.uint8)
    m[h // 5:h // 5 + max(1, h // 3), w // 4:w // 4 + max(1, w // 2)] = 0
    band = (yy >= h - max(1, h // 4)) & ((xx + seed) % 3 != 0)
    m[band] = ((xx * 7 + yy * 3 + seed) % 256).astype(np.uint8)[band]
    m[(yy + 2 * xx + seed) % 11 == 0] = 254
    return m


def flag_mask():
    """values 0, 1, 128, 254 and 255"""
    return np.array([0, 1, 128, 254, 255], np.uint8)[(np.arange(12)[:, None] * 3 + np.arange(10)[None, :]) % 5].copy()


# name -> ([H, W], [h, w])
BICUBIC_CASES = {
    "down_37x53_to_16x16": ((37, 53), (16, 16)),           # both passes, non-integer ratios, bounds clipped at both edges
    "up_16x16_to_37x53": ((16, 16), (37, 53)),             # upscale: fs clamps to 1
    "narrow_7x5_to_16x16": ((7, 5), (16, 16)),             # source narrower than the support
    "hskip_64x64_to_64x31": ((64, 64), (64, 31)),          # vertical pass skipped
    "copy_64x31": ((64, 31), (64, 31)),
    "near1_129x127_to_128x128": ((129, 127), (128, 128)),  # scale just off 1
    "taps257_1023x40_to_16x16": ((1023, 40), (16, 16)),    # 257 taps, more than a workgroup; aspect 25.6
    "checker_40x40_to_64x64": ((40, 40), (64, 64)),        # overshoot: both clamps fire
    "checker_40x40_to_24x24": ((40, 40), (24, 24)),
}
NEAREST_CASES = {
    "up_16x16_to_37x53": ((16, 16), (37, 53), 37),         # (output positions where the closed form picks another pixel: one column)
    "hskip_64x64_to_64x31": ((64, 64), (64, 31), 64),
    "down_520x390_to_16x16": ((520, 390), (16, 16), None),
}
FLOW_PHOTOS = ((100, 75), (48, 64), (80, 80), (16, 16), (12, 9))            # [H, W]
FLOW_MASKS = ((600, 450), (64, 48), (33, 90), (20, 20), (40, 25))           # other sizes than their photo, one above read_mask's 512
FLOW_RESOLUTIONS = (16, 32)


def bicubic_source(name):
    (h, w), _ = BICUBIC_CASES[name]
    return checkerboard(h, w) if name.startswith("checker") else photo(h, w, sorted(BICUBIC_CASES).index(name))


def nearest_source(name):
    (h, w) = NEAREST_CASES[name][0]
    return mask_image(h, w, sorted(NEAREST_CASES).index(name))


def batch5_sources():
    return [photo(h, w, 40 + i) for i, (h, w) in enumerate(((37, 53), (16, 16), (9, 70), (64, 31), (24, 24)))]


BATCH5_SIZES = ((16, 16), (37, 53), (24, 24), (31, 64), (24, 24))           # (w, h); the last is a copy


def batch33_sources():
    return [photo(18 + i % 5, 17 + (3 * i) % 7, 60 + i) for i in range(ITEMS_PER_LAUNCH + 1)]


def batch33_sizes():
    return [(12 + i % 9, 11 + (5 * i) % 8) for i in range(ITEMS_PER_LAUNCH + 1)]


def flow_inputs():
    photos = [photo(h, w, 80 + i) for i, (h, w) in enumerate(FLOW_PHOTOS)]
    masks = [mask_image(h, w, i) for i, (h, w) in enumerate(FLOW_MASKS)]
    return photos, masks


_GOLDEN = {}


def golden(name):
    if name not in _GOLDEN:
        with np.load(os.path.join(GOLDEN, f"photo_{name}.npz")) as z:
            _GOLDEN[name] = {k: z[k] for k in z.files}
        for v in _GOLDEN[name].values():
            v.setflags(write=False)
    return _GOLDEN[name]


# ---- through the C ABI ------------------------------------------------------------------------------------------------------------
def call(lib, mem, sources, sizes, filt, flags=0, odd=False):
    """migan_photo_resize_batch on `sources` (uint8 [H, W, 3] or [H, W]) to `sizes` (w, h) -> the list of results; asserts that nothing
    behind a destination was written and that the sources still hold their bytes"""
    channels = 3 if sources[0].ndim == 3 else 1
    ins = [mem.put(s, odd) for s in sources]
    outs = [mem.put(np.full(h * w * channels + GUARD, FILL, np.uint8), odd) for w, h in sizes]
    table = [(mem.ptr(i), mem.ptr(o), s.shape[0], s.shape[1], h, w) for i, o, s, (w, h) in zip(ins, outs, sources, sizes)]
    scratch = mem.put(np.zeros(max(16, lib.photo_scratch_bytes(table, channels, filt)), np.uint8))
    lib.photo_resize_batch(table, channels, filt, flags, mem.ptr(scratch), mem.stream)
    mem.sync()
    got = []
    for i, (o, s, (w, h)) in enumerate(zip(outs, sources, sizes)):
        raw = mem.get(o)
        assert (raw[h * w * channels:] == FILL).all(), f"item {i}: bytes behind the destination were written"
        got.append(raw[:h * w * channels].reshape((h, w, 3) if channels == 3 else (h, w)).copy())
        assert np.array_equal(mem.get(ins[i]), np.ascontiguousarray(s).reshape(-1)), f"item {i}: the source was written"
    return got


def differing(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, f"{a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    return int((a != b).sum())


def run_bicubic_case(lib, mem, name, odd=False):
    _, (h, w) = BICUBIC_CASES[name]
    g = golden("bicubic")
    src = g[f"{name}.src"]
    got = call(lib, mem, [src], [(w, h)], BICUBIC, odd=odd)[0]
    assert differing(got, g[f"{name}.out"]) == 0, f"{name}: {differing(got, g[f'{name}.out'])} bytes differ from Pillow's"
    if name == "checker_40x40_to_64x64":
        want = g[f"{name}.out"]
        assert (want == 0).any() and (want == 255).any()             # both clamps fired (tests/test_photo_oracle.py: the sums leave 0 .. 255)
    return got


def run_nearest_case(lib, mem, name):
    _, (h, w), _ = NEAREST_CASES[name]
    g = golden("nearest")
    got = call(lib, mem, [g[f"{name}.src"]], [(w, h)], NEAREST)[0]
    assert differing(got, g[f"{name}.out"]) == 0, name
    return got


def run_flags(lib, mem):
    g = golden("nearest")
    src = g["flags.src"]
    assert set(np.unique(src)) == {0, 1, 128, 254, 255}
    for flags in (INVERT, THRESHOLD, INVERT | THRESHOLD):
        for size in ((10, 12), (7, 17)):                               # the copy applies the flags as well
            got = call(lib, mem, [src], [size], NEAREST, flags)[0]
            assert differing(got, g[f"flags.{flags}.{size[0]}x{size[1]}"]) == 0, (flags, size)
    # the same on three channels
    rgb = np.repeat(src[:, :, None], 3, axis=2).copy()
    got = call(lib, mem, [rgb], [(7, 17)], NEAREST, INVERT | THRESHOLD)[0]
    assert differing(got, np.repeat(g["flags.3.7x17"][:, :, None], 3, axis=2)) == 0


def run_batches(lib, mem):
    g = golden("batch")
    for name, sizes in (("b5", BATCH5_SIZES), ("b33", batch33_sizes())):
        n = len(sizes)
        srcs = [g[f"{name}.src{i}"] for i in range(n)]
        got = call(lib, mem, srcs, sizes, BICUBIC, odd=(name == "b5"))
        for i in range(n):
            assert differing(got[i], g[f"{name}.out{i}"]) == 0, f"{name} item {i}"
        # independent of the batch's composition: an item alone gives the bytes it has in the batch
        for i in ((0, 2, 4) if name == "b5" else (0, 31, 32)):
            alone = call(lib, mem, [srcs[i]], [sizes[i]], BICUBIC)[0]
            assert np.array_equal(alone, got[i]), f"{name} item {i} alone differs"
    masks = [g[f"m33.src{i}"] for i in range(ITEMS_PER_LAUNCH + 1)]
    got = call(lib, mem, masks, batch33_sizes(), NEAREST, THRESHOLD)
    for i in range(len(masks)):
        assert differing(got[i], g[f"m33.out{i}"]) == 0, f"m33 item {i}"


def flow_through_abi(lib, mem, flow, images, masks, r, invert=False):
    """load_eval / load_demo of mi-gan_amd/photo.py restated hop by hop on the C ABI (the emulator runs on host memory, the Python front
    only on the device): the same hop sizes, from the package's own demo_plan"""
    import importlib
    ph = importlib.import_module("mi-gan_amd").photo
    n = len(images)
    if flow == "eval":
        return (np.stack(call(lib, mem, images, [(r, r)] * n, BICUBIC)), np.stack(call(lib, mem, masks, [(r, r)] * n, NEAREST)))
    plans = [ph.demo_plan((i.shape[1], i.shape[0]), (m.shape[1], m.shape[0]), r) for i, m in zip(images, masks)]
    fitted = call(lib, mem, images, [p[0] for p in plans], BICUBIC)
    img = call(lib, mem, fitted, [(r, r)] * n, BICUBIC)
    m1 = call(lib, mem, masks, [p[1] for p in plans], NEAREST, (INVERT if invert else 0) | THRESHOLD)
    m2 = call(lib, mem, m1, [p[2] for p in plans], NEAREST)
    return np.stack(img), np.stack(call(lib, mem, m2, [(r, r)] * n, NEAREST))


def flow_golden(flow, r, invert=False):
    g = golden("flows")
    key = f"{flow}.r{r}" + (".inv" if invert else "")
    return g[f"{key}.img"], g[f"{key}.mask"]


def flow_sources():
    g = golden("flows")
    n = len(FLOW_PHOTOS)
    return [g[f"photo{i}"] for i in range(n)], [g[f"mask{i}"] for i in range(n)]


def run_arg_errors(lib, mem):
    """every MIGAN_EINVAL of include/migan_photo_hip.h, each with nothing launched (the destination keeps its fill), then the good call"""
    import ctypes as C
    import importlib
    hb = importlib.import_module("mi-gan_amd").hipbind
    src = photo(20, 24, 5)
    d_src = mem.put(src)
    d_dst = mem.put(np.full(16 * 16 * 3 + GUARD, FILL, np.uint8))
    good_item = (mem.ptr(d_src), mem.ptr(d_dst), 20, 24, 16, 16)
    scratch = mem.put(np.zeros(lib.photo_scratch_bytes([good_item], 3, BICUBIC), np.uint8))
    good = dict(items=[good_item], n=1, channels=3, filter=BICUBIC, flags=0, scratch=mem.ptr(scratch))

    def raw(**kw):
        a = dict(good, **kw)
        return lib.lib.migan_photo_resize_batch(hb.photo_items(a["items"]), a["n"], a["channels"], a["filter"], a["flags"], C.c_void_p(a["scratch"]),
                                                C.c_void_p(mem.stream))

    def item(**kw):
        d = dict(zip(("src", "dst", "sh", "sw", "dh", "dw"), good_item), **kw)
        return [(d["src"], d["dst"], d["sh"], d["sw"], d["dh"], d["dw"])]

    bad = {
        "null items": dict(items=None), "null src": dict(items=item(src=None)), "null dst": dict(items=item(dst=None)),
        "null scratch": dict(scratch=None), "n 0": dict(n=0), "n -1": dict(n=-1),
        "channels 2": dict(channels=2), "channels 4": dict(channels=4), "channels 0": dict(channels=0),
        "filter 2": dict(filter=2), "filter -1": dict(filter=-1),
        "flags with bicubic": dict(flags=INVERT), "threshold with bicubic": dict(flags=THRESHOLD), "flags 4": dict(filter=NEAREST, flags=4),
        "flags -1": dict(filter=NEAREST, flags=-1),
        "src H 0": dict(items=item(sh=0)), "src W 0": dict(items=item(sw=0)), "src H -2": dict(items=item(sh=-2)),
        "src W 16385": dict(items=item(sh=16384, sw=16385)), "src H 16385": dict(items=item(sh=16385, sw=16384)),
        "dst H 0": dict(items=item(dh=0)), "dst W 0": dict(items=item(dw=0)), "dst W 4097": dict(items=item(dw=4097)),
        "dst H 4097": dict(items=item(dh=4097)),
        "aspect 33 : 1": dict(items=item(sh=33, sw=1)), "aspect 1 : 33": dict(items=item(sh=10, sw=331)),
    }
    for what, kw in bad.items():
        rc = raw(**kw)
        assert rc == EINVAL, f"{what}: return code {rc}"
        assert (lib.lib.migan_last_error() or b"").decode(), f"{what}: no error text"
        mem.sync()
        assert (mem.get(d_dst) == FILL).all(), f"{what}: something was launched"
    # the size query refuses the same items
    n = C.c_size_t(7)
    for what, args in {"null items": (None, 1, 3, BICUBIC, C.byref(n)), "null bytes": (hb.photo_items([good_item]), 1, 3, BICUBIC, None),
                       "n 0": (hb.photo_items([good_item]), 0, 3, BICUBIC, C.byref(n)), "channels 2": (hb.photo_items([good_item]), 1, 2, BICUBIC, C.byref(n)),
                       "filter 3": (hb.photo_items([good_item]), 1, 3, 3, C.byref(n)), "aspect": (hb.photo_items(item(sh=330, sw=10)), 1, 3, BICUBIC, C.byref(n)),
                       "dst 4097": (hb.photo_items(item(dw=4097)), 1, 3, NEAREST, C.byref(n))}.items():
        assert lib.lib.migan_photo_scratch_bytes(*args) == EINVAL, what
    # the limits themselves are inside the domain (sizes only: nothing is launched by the query)
    for it in (item(sh=16384, sw=16384, dh=4096, dw=4096), item(sh=32, sw=1), item(sh=1, sw=32, dh=1, dw=1)):
        assert lib.lib.migan_photo_scratch_bytes(hb.photo_items(it), 1, 3, BICUBIC, C.byref(n)) == 0 and n.value > 0
    assert raw() == 0
    mem.sync()
    got = mem.get(d_dst)
    assert np.array_equal(got[:16 * 16 * 3].reshape(16, 16, 3), pil_bicubic(src, (16, 16))) and (got[16 * 16 * 3:] == FILL).all()
