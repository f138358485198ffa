"""Shared cases and yardsticks of the PSNR / SSIM tests (include/migan_metrics_hip.h): tests/test_metrics_oracle.py ties the
yardsticks to the reference's own compute_ssim, tests/test_emu_metrics.py and tests/test_gpu_metrics.py run the cases through the C
ABI, on the emulator (host memory) and on the device.  Test infrastructure only.

Yardsticks, both torch-CPU:
  float64   the definition in include/migan_metrics_hip.h evaluated in float64 (taps: the reference's float32 values, the 2-D window
            their exact outer product)
  float32   the reference's formulation (eva_ssim.py:15-41: the 2-D float32 window through F.conv2d, float32 throughout)
The ruler of an image pair is the mean over the averaging region of |float32 map - float64 map|: what the reference's own arithmetic
is off by on that very pair.  The kernels' SSIM must lie within RULERS x ruler of the float64 value.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

TILE_W, TILE_H = 32, 32          # kMetTW, kMetTH of mi-gan_amd/csrc/migan_metrics.hpp
HALO = 5
ITEMS_PER_LAUNCH = 32            # kMetItemsMax
U8, F32 = 0, 1                   # MIGAN_METRICS_U8 / _F32
CHW, HWC = 0, 1                  # MIGAN_METRICS_CHW / _HWC
RULERS = 4.0
GUARD, FILL = 4, -7.25           # elements behind the last output row, and what the outputs hold before a call
EINVAL = 1


def taps32():
    """gaussian(11, 1.5), eva_ssim.py:11-13"""
    g = torch.tensor([np.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def normalise(a, value_range=(0.0, 1.0), dtype=torch.float32):
    """[..., H, W] uint8 -> v / 255; float32 -> (v - lo) / (hi - lo) with lo, hi and hi - lo float32 numbers; evaluated in `dtype`"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype == np.uint8:
        return t.to(dtype) / 255
    lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
    return (t.to(dtype) - float(lo)) / float(np.float32(hi - lo))


def ssim_map32(g, p):
    """eva_ssim.py:15-36 on float32 [N, 3, H, W]"""
    w1 = taps32().unsqueeze(1)
    window = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(3, 1, 11, 11).contiguous()
    return _ssim_map(g, p, window)


def ssim_map64(g, p):
    """the definition in float64 on float64 [N, 3, H, W]"""
    w1 = taps32().double()
    window = torch.outer(w1, w1)[None, None].expand(3, 1, 11, 11).contiguous()
    return _ssim_map(g, p, window)


def _ssim_map(img1, img2, window):
    mu1 = F.conv2d(img1, window, padding=5, groups=3)
    mu2 = F.conv2d(img2, window, padding=5, groups=3)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=5, groups=3) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=5, groups=3) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=5, groups=3) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def regions(h, w, mask, shave):
    """(P of the MSE, the SSIM averaging region) as bool [H, W]"""
    hole = np.ones((h, w), dtype=bool) if mask is None else mask != 255
    box = np.zeros((h, w), dtype=bool)
    box[shave:h - shave, shave:w - shave] = True
    return hole & box, hole


def expected(gt, pred, mask=None, shave=0, value_range=(0.0, 1.0)):
    """gt [3, H, W], pred [S, 3, H, W] (uint8 or float32), mask [H, W] uint8 or None -> per sample: mse (the exact expression the kernel
    is held to), count = 3 |P|, ssim (float64 yardstick), ssim32 (float32 yardstick), ruler"""
    s, _, h, w = pred.shape
    p_reg, s_reg = regions(h, w, mask, shave)
    count = 3 * int(p_reg.sum())
    out = dict(mse=np.full(s, np.nan), ssim=np.full(s, np.nan), ssim32=np.full(s, np.nan), ruler=np.full(s, np.nan), count=count)
    g32, p32 = normalise(gt[None], value_range), normalise(pred, value_range)
    g64, p64 = normalise(gt[None], value_range, torch.float64), normalise(pred, value_range, torch.float64)
    m32 = ssim_map32(g32.expand_as(p32).contiguous(), p32).double().numpy()
    m64 = ssim_map64(g64.expand_as(p64).contiguous(), p64).numpy()
    for i in range(s):
        if count:
            if gt.dtype == np.uint8:
                d = pred[i].astype(np.int64) - gt.astype(np.int64)
                out["mse"][i] = int((d * d)[:, p_reg].sum()) / (count * 65025.0)
            else:
                d = (p32[i] - g32[0]).numpy()                      # the fp32 differences ...
                out["mse"][i] = float((d.astype(np.float64) ** 2)[:, p_reg].sum()) / count      # ... squared and summed in fp64
        if s_reg.any():
            out["ssim"][i] = m64[i][:, s_reg].mean()
            out["ssim32"][i] = m32[i][:, s_reg].mean()
            out["ruler"][i] = np.abs(m32[i] - m64[i])[:, s_reg].mean()
    return out


# ---- images ---------------------------------------------------------------------------------------------------------------
def _unit(kind, h, w, seed):
    """float64 [3, H, W] in [0, 1]: white noise, or a smooth pattern"""
    if kind == "noise":
        return np.random.default_rng(seed).random((3, h, w))
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    c = np.arange(3, dtype=np.float64)[:, None, None]
    return 0.5 + 0.45 * np.sin(0.13 * yy[None] + 0.7 * c + 0.37 * seed) * np.cos(0.09 * xx[None] - 0.4 * c + 0.11 * seed)


def image(kind, h, w, seed, dtype, value_range=(0.0, 1.0)):
    v = _unit(kind, h, w, seed)
    if dtype == U8:
        return np.rint(v * 255.0).astype(np.uint8)
    lo, hi = value_range
    return (lo + v * (hi - lo)).astype(np.float32)


def hole_rect(h, w):
    """(y0, y1, x0, x1) of the rectangle in which the completions differ from the photo: across the first tile border where the image
    has one in that direction, otherwise the middle of the image"""
    def span(n, tile):
        if n > tile:
            return tile - 6, min(n, tile + 7)
        return n // 4, max(n // 4 + 1, n - n // 4)
    return span(h, TILE_H) + span(w, TILE_W)


def assert_straddles(rect, h, w):
    """a hole inside one tile would hide a halo defect from the hole-only mean"""
    y0, y1, x0, x1 = rect
    assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w
    if h > TILE_H:
        assert y0 // TILE_H != (y1 - 1) // TILE_H, "the hole does not cross a horizontal tile border"
    if w > TILE_W:
        assert x0 // TILE_W != (x1 - 1) // TILE_W, "the hole does not cross a vertical tile border"


def make_item(kind, h, w, samples, dtype, seed, with_mask=True, value_range=(0.0, 1.0), hole=True):
    """(gt [3, H, W], pred [S, 3, H, W], mask [H, W] or None): the completions differ from the photo, and from each other, inside
    hole_rect; hole=False: a mask without a hole pixel (completions still differ)"""
    other = "smooth" if kind == "noise" else "noise"
    gt = image(kind, h, w, seed, dtype, value_range)
    rect = hole_rect(h, w)
    assert_straddles(rect, h, w)
    y0, y1, x0, x1 = rect
    pred = np.stack([gt] * samples)
    for s in range(samples):
        fill = image(other if s % 2 == 0 else kind, h, w, 100 + 7 * seed + s, dtype, value_range)
        pred[s][:, y0:y1, x0:x1] = fill[:, y0:y1, x0:x1]
    mask = None
    if with_mask:
        mask = np.full((h, w), 255, dtype=np.uint8)
        if hole:
            mask[y0:y1, x0:x1] = (np.arange((y1 - y0) * (x1 - x0)).reshape(y1 - y0, x1 - x0) % 5).astype(np.uint8)      # "not 255" is the hole, not "0"
    return gt, pred, mask


SMALL_SIZES = ((5, 7), (11, 11), (2 * TILE_H + 3, 3 * TILE_W + 1), (33, 41))
SHAVE_SIZES = ((2 * TILE_H + 3, 3 * TILE_W + 1), (33, 41))       # (shave 8 needs more than 16 rows and columns)

# name -> dict(sizes, dtype, layout, samples, shave, mask, value_range, odd, nohole): every size once with a noise photo and once with
# a smooth one; nohole appends one item whose mask has no hole pixel (NaN in both outputs)
CASES = {
    "small_u8_hwc_s3_mask": dict(sizes=SMALL_SIZES, dtype=U8, layout=HWC, samples=3, mask=True),
    "small_u8_chw_s1": dict(sizes=SMALL_SIZES, dtype=U8, layout=CHW, samples=1, mask=False),
    "small_f32_chw_s3": dict(sizes=SMALL_SIZES, dtype=F32, layout=CHW, samples=3, mask=False),
    "small_f32_hwc_s1_mask": dict(sizes=SMALL_SIZES, dtype=F32, layout=HWC, samples=1, mask=True),
    "u8_chw_shave8_mask_nohole": dict(sizes=SHAVE_SIZES, dtype=U8, layout=CHW, samples=3, shave=8, mask=True, nohole=True),
    "u8_hwc_shave8": dict(sizes=SHAVE_SIZES, dtype=U8, layout=HWC, samples=1, shave=8, mask=False),
    "f32_hwc_range_shave8_mask_nohole": dict(sizes=SHAVE_SIZES, dtype=F32, layout=HWC, samples=3, shave=8, mask=True, nohole=True,
                                             value_range=(-1.0, 1.0)),
    "f32_chw_range": dict(sizes=SMALL_SIZES, dtype=F32, layout=CHW, samples=1, mask=False, value_range=(-1.0, 1.0)),
    "u8_chw_odd_mask": dict(sizes=((33, 41), (5, 7)), dtype=U8, layout=CHW, samples=3, mask=True, odd=True),
    "u8_hwc_odd": dict(sizes=((33, 41), (5, 7)), dtype=U8, layout=HWC, samples=1, mask=False, odd=True, shave=2),
}
_ITEMS, _EXPECTED = {}, {}


def case_items(name):
    """the items of a case (built once) and what is expected of each (computed once, shared by the emulator and the GPU tests)"""
    if name not in _ITEMS:
        c = CASES[name]
        vr = c.get("value_range", (0.0, 1.0))
        items = [make_item(kind, h, w, c["samples"], c["dtype"], 3 * i + j, c["mask"], vr)
                 for i, (h, w) in enumerate(c["sizes"]) for j, kind in enumerate(("noise", "smooth"))]
        if c.get("nohole"):
            h, w = c["sizes"][-1]
            items.insert(1, make_item("noise", h, w, c["samples"], c["dtype"], 50, True, vr, hole=False))
        _ITEMS[name] = items
        _EXPECTED[name] = [expected(g, p, m, c.get("shave", 0), vr) for g, p, m in items]
        for a in items:
            for b in a:
                if b is not None:
                    b.setflags(write=False)
    return _ITEMS[name], _EXPECTED[name]


# ---- memory the library reads and writes: host arrays for the emulator, device buffers on the GPU ------------------------------
class HostMem:
    """the emulator runs on host memory"""

    def put(self, a, odd=False):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.empty(raw.size + 64, dtype=np.uint8)
        off = (-buf.ctypes.data) % 16 + (1 if odd else 0)
        view = buf[off:off + raw.size]
        view[...] = raw
        return view

    def ptr(self, view):
        return view.ctypes.data

    def get(self, view):
        return np.array(view, copy=True)

    def sync(self):
        pass

    stream = 0


class CudaMem:
    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.stream = int(torch.cuda.current_stream(self.device).cuda_stream)

    def put(self, a, odd=False):
        raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
        buf = torch.empty(raw.numel() + 64, dtype=torch.uint8, device=self.device)
        off = (-buf.data_ptr()) % 16 + (1 if odd else 0)
        view = buf[off:off + raw.numel()]
        view.copy_(raw)
        return view

    def ptr(self, view):
        return view.data_ptr()

    def get(self, view):
        return view.cpu().numpy()

    def sync(self):
        torch.cuda.synchronize(self.device)


def _laid_out(a, layout):
    """[..., 3, H, W] -> the bytes of that tensor in `layout`"""
    return np.ascontiguousarray(np.moveaxis(a, -3, -1)) if layout == HWC else np.ascontiguousarray(a)


def call(lib, mem, items, samples, dtype, layout, shave=0, value_range=(0.0, 1.0), odd=False):
    """migan_metrics_batch on `items` = [(gt [3, H, W], pred [S, 3, H, W], mask or None), ...] -> (mse [n, S], ssim [n, S]); asserts
    that nothing behind the last row was written and that the inputs still hold their bytes"""
    n = len(items)
    up, table = [], []
    for gt, pred, mask in items:
        assert pred.shape == (samples,) + gt.shape
        bufs = [mem.put(_laid_out(gt, layout), odd), mem.put(_laid_out(pred, layout), odd), None if mask is None else mem.put(mask, odd)]
        if odd:
            assert all(mem.ptr(b) % 2 == 1 for b in bufs if b is not None)
        up.append(bufs)
        table.append((mem.ptr(bufs[0]), mem.ptr(bufs[1]), None if mask is None else mem.ptr(bufs[2]), gt.shape[1], gt.shape[2]))
    before = [[None if b is None else mem.get(b) for b in bufs] for bufs in up]
    scratch = mem.put(np.zeros(lib.metrics_scratch_bytes(table, samples), dtype=np.uint8))
    outs = [mem.put(np.full(n * samples + GUARD, FILL, dtype=np.float64)) for _ in range(2)]
    lib.metrics_batch(table, samples, dtype, layout, shave, value_range[0], value_range[1], mem.ptr(scratch), mem.ptr(outs[0]),
                      mem.ptr(outs[1]), mem.stream)
    mem.sync()
    got = [mem.get(o).view(np.float64) for o in outs]
    for g in got:
        assert (g[n * samples:] == FILL).all(), "elements behind the last row were written"
    for bufs, olds in zip(up, before):
        for b, old in zip(bufs, olds):
            assert b is None or np.array_equal(mem.get(b), old), "an input was written"
    return got[0][:n * samples].reshape(n, samples).copy(), got[1][:n * samples].reshape(n, samples).copy()


FIGURES = []       # (case, item, sample, ruler, |ssim - float64|, mse relative error): printed by the tests, recorded in profiles/metrics.md


def check(name, mse, ssim, items, exp, dtype):
    """the outputs of one call against what is expected of each item"""
    try:
        _check(name, mse, ssim, items, exp, dtype)
    finally:
        rows = [f for f in FIGURES if f[0] == name]
        del FIGURES[:]
        if rows:
            print(f"{name}: {len(rows)} rows, rulers {min(r[3] for r in rows):.2e} .. {max(r[3] for r in rows):.2e}, |ssim - float64| at most "
                  f"{max(r[4] for r in rows):.2e} = {max(r[4] / r[3] for r in rows):.3f} rulers, mse relative error at most "
                  f"{np.nanmax([r[5] for r in rows]):.2e}")


def _check(name, mse, ssim, items, exp, dtype):
    for i, ((gt, pred, mask), e) in enumerate(zip(items, exp)):
        for s in range(pred.shape[0]):
            what = f"{name} item {i} ({gt.shape[1]}x{gt.shape[2]}) sample {s}"
            if np.isnan(e["ssim"][s]):
                assert np.isnan(ssim[i, s]) and np.isnan(mse[i, s]), f"{what}: an empty region must give NaN, got {mse[i, s]}, {ssim[i, s]}"
                continue
            dist, ruler = abs(ssim[i, s] - e["ssim"][s]), e["ruler"][s]
            rel = 0.0 if mse[i, s] == e["mse"][s] else abs(mse[i, s] - e["mse"][s]) / e["mse"][s]
            FIGURES.append((name, i, s, ruler, dist, rel))
            if e["count"] == 0:                 # (the hole lies in the shaved border: P is empty, the SSIM region is not)
                assert np.isnan(mse[i, s]), f"{what}: an empty P must give NaN, got {mse[i, s]}"
            elif dtype == U8:
                assert mse[i, s] == e["mse"][s], f"{what}: mse {mse[i, s]!r} is not sse / (count * 65025.0) = {e['mse'][s]!r}"
            else:
                # a sum of `count` non-negative fp64 terms, reordered: every partial sum is off by at most half an ulp of the total
                assert rel <= e["count"] * 2.0 ** -52, f"{what}: mse {mse[i, s]!r} vs {e['mse'][s]!r}, relative error {rel:.3e}"
            assert dist <= RULERS * ruler, f"{what}: ssim {ssim[i, s]!r} vs {e['ssim'][s]!r}: {dist:.3e} is {dist / ruler:.2f} rulers of {ruler:.3e}"


def run_case(lib, mem, name):
    c = CASES[name]
    items, exp = case_items(name)
    mse, ssim = call(lib, mem, items, c["samples"], c["dtype"], c["layout"], c.get("shave", 0), c.get("value_range", (0.0, 1.0)), c.get("odd", False))
    check(name, mse, ssim, items, exp, c["dtype"])
    return mse, ssim


def run_samples_alone(lib, mem, name):
    """sample s of an S = 3 call is bit-equal to the S = 1 call on that completion alone"""
    c = CASES[name]
    assert c["samples"] == 3
    items, _ = case_items(name)
    args = (c["dtype"], c["layout"], c.get("shave", 0), c.get("value_range", (0.0, 1.0)), c.get("odd", False))
    mse, ssim = call(lib, mem, items, 3, *args)
    for s in range(3):
        m1, s1 = call(lib, mem, [(g, p[s:s + 1], m) for g, p, m in items], 1, *args)
        assert np.array_equal(m1[:, 0].view(np.uint64), mse[:, s].view(np.uint64)), f"{name}: mse of sample {s} alone differs"
        assert np.array_equal(s1[:, 0].view(np.uint64), ssim[:, s].view(np.uint64)), f"{name}: ssim of sample {s} alone differs"


def run_identity(lib, mem, dtype, layout):
    """pred identical to gt: mse is exactly 0, ssim within the ruler of 1"""
    items = []
    for i, (h, w) in enumerate(SMALL_SIZES):
        gt = image("noise" if i % 2 else "smooth", h, w, 20 + i, dtype)
        items.append((gt, np.stack([gt, gt]), None))
    mse, ssim = call(lib, mem, items, 2, dtype, layout)
    for i, (gt, pred, _) in enumerate(items):
        e = expected(gt, pred)
        for s in range(2):
            print(f"identity {gt.shape[1]}x{gt.shape[2]}: ruler {e['ruler'][s]:.3e} |ssim - 1| {abs(ssim[i, s] - 1.0):.3e} mse {mse[i, s]!r}")
            assert mse[i, s] == 0.0 and not np.signbit(mse[i, s])
            assert abs(e["ssim"][s] - 1.0) <= 1e-12
            assert abs(ssim[i, s] - 1.0) <= RULERS * e["ruler"][s]
    return mse, ssim


def two_launch_items(dtype=U8):
    """33 tiny items of different sizes: two launches"""
    items = []
    for i in range(ITEMS_PER_LAUNCH + 1):
        h, w = 3 + i % 7, 4 + (5 * i) % 11 + (30 if i == 32 else 0)
        items.append(make_item("noise" if i % 2 else "smooth", h, w, 2, dtype, i, with_mask=(i % 3 == 0)))
    assert len({(g.shape[1], g.shape[2]) for g, _, _ in items}) > 16
    return items


def run_two_launches(lib, mem):
    items = two_launch_items()
    a = call(lib, mem, items, 2, U8, CHW)                  # (guards and inputs: call() looks at them)
    b = call(lib, mem, items, 2, U8, CHW)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "two calls on the same inputs differ"
    exp = [expected(g, p, m) for g, p, m in items]
    check("two_launches", a[0], a[1], items, exp, U8)


def run_arg_errors(lib, mem):
    """every MIGAN_EINVAL of include/migan_metrics_hip.h, each with nothing launched (the outputs keep their fill), then the good call"""
    import importlib
    hb = importlib.import_module("mi-gan_amd").hipbind
    gt, pred, mask = make_item("noise", 20, 24, 1, U8, 1)
    bufs = [mem.put(gt), mem.put(pred), mem.put(mask)]
    good_item = (mem.ptr(bufs[0]), mem.ptr(bufs[1]), mem.ptr(bufs[2]), 20, 24)
    scratch = mem.put(np.zeros(lib.metrics_scratch_bytes([good_item], 1), dtype=np.uint8))
    outs = [mem.put(np.full(1 + GUARD, FILL, dtype=np.float64)) for _ in range(2)]
    good = dict(items=[good_item], n=1, samples=1, dtype=U8, layout=CHW, shave=0, lo=0.0, hi=1.0, scratch=mem.ptr(scratch),
                mse=mem.ptr(outs[0]), ssim=mem.ptr(outs[1]))

    def raw(**kw):
        a = dict(good, **kw)
        return lib.lib.migan_metrics_batch(hb.metrics_items(a["items"]), a["n"], a["samples"], a["dtype"], a["layout"], a["shave"],
                                           C.c_float(a["lo"]), C.c_float(a["hi"]), C.c_void_p(a["scratch"]), C.c_void_p(a["mse"]),
                                           C.c_void_p(a["ssim"]), C.c_void_p(mem.stream))

    def item(**kw):
        d = dict(zip(("gt", "pred", "mask", "H", "W"), good_item), **kw)
        return [(d["gt"], d["pred"], d["mask"], d["H"], d["W"])]

    bad = {
        "null items": dict(items=None), "null gt": dict(items=item(gt=None)), "null pred": dict(items=item(pred=None)),
        "null scratch": dict(scratch=None), "null out_mse": dict(mse=None), "null out_ssim": dict(ssim=None),
        "samples 0": dict(samples=0), "n 0": dict(n=0), "n -1": dict(n=-1), "H 0": dict(items=item(H=0)), "W 0": dict(items=item(W=0)),
        "H -3": dict(items=item(H=-3)), "shave -1": dict(shave=-1), "shave eats H": dict(shave=10), "shave eats W": dict(items=item(H=40), shave=12),
        "hi == lo": dict(lo=0.5, hi=0.5), "nan lo": dict(lo=float("nan")), "inf hi": dict(hi=float("inf")), "-inf lo": dict(lo=float("-inf")),
        "dtype 2": dict(dtype=2), "dtype -1": dict(dtype=-1), "layout 2": dict(layout=2), "layout -1": dict(layout=-1),
    }
    for what, kw in bad.items():
        rc = raw(**kw)
        assert rc == EINVAL, f"{what}: return code {rc}"
        assert (lib.lib.migan_last_error() or b"").decode(), f"{what}: no error text"
        mem.sync()
        for o in outs:
            assert (mem.get(o).view(np.float64) == FILL).all(), f"{what}: something was launched"
    # the size query: 0 and an error text
    for what, args in {"null items": (None, 1, 1), "n 0": (hb.metrics_items([good_item]), 0, 1), "samples 0": (hb.metrics_items([good_item]), 1, 0),
                       "H 0": (hb.metrics_items(item(H=0)), 1, 1)}.items():
        assert lib.lib.migan_metrics_scratch_bytes(*args) == 0, what
    assert raw() == 0
    mem.sync()
    e = expected(gt, pred, mask)
    got = [mem.get(o).view(np.float64) for o in outs]
    assert got[0][0] == e["mse"][0] and abs(got[1][0] - e["ssim"][0]) <= RULERS * e["ruler"][0]
    assert (got[0][1:] == FILL).all() and (got[1][1:] == FILL).all()
