"""Random hole masks (include/migan_masks_hip.h): a numpy restatement of the reference's RandomMask (scripts/generate_masks.py:16-93) --
the order of its draws from numpy's legacy generator, and Pillow's rasterisation of wide lines and ellipses -- plus the cases the CPU
and the device tests share.  Written from the rules, not from the reference's text; tests/test_masks_oracle.py holds it against the
goldens the reference's own functions gave (tests/golden/masks_*.npz) and against ImageDraw itself.  Test infrastructure only.

A plan is what the host code hands the kernel for one candidate, int32 words:
  [n_rect, n_quad, n_disc, flips]  flips bit 0: np.flip(mask, 0) of the brush layer (rows), bit 1: np.flip(mask, 1) (columns)
  n_rect x (x0, y0, x1, y1)        half-open, clipped to the image
  n_quad x (x[4], y[4], dx[4])     the corners of Pillow's wide-line quadrilateral in its order; dx[k]: fp32 bits of the slope of the edge
                                   corner k -> corner k + 1 (0 for a horizontal edge).  A zero-length segment: four equal corners
  n_disc x (cx, cy, d)             the ellipse in the box (c - d / 2, c + d / 2), d = 2 * (width // 2)
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_RECTS, MAX_STROKES, MAX_POINTS = 13, 19, 18
MAX_QUADS, MAX_DISCS = MAX_STROKES * (MAX_POINTS - 1), MAX_STROKES * MAX_POINTS
PLAN_WORDS_MAX = 4 + 4 * MAX_RECTS + 12 * MAX_QUADS + 3 * MAX_DISCS
BAND = 32                                                          # rows of one workgroup (kMkBand)
R_MIN, R_MAX = 16, 1024
DIAMETERS = tuple(range(12, 48, 2))
# (seed, R, hole_range, masks): the goldens of tests/golden/make_golden_masks.py
GOLDENS = ((0, 32, (0, 1), 64), (0, 37, (0, 1), 64), (0, 64, (0, 1), 64), (0, 64, (0.2, 0.4), 16), (0, 32, (0.4, 0.6), 16),
           (0, 512, (0, 1), 4), (0, 1024, (0, 1), 2))
SMALL = tuple(g for g in GOLDENS if g[1] <= 64)


def golden_name(seed, r, hole_range):
    return f"masks_s{seed}_r{r}_{hole_range[0]}_{hole_range[1]}.npz"


_CACHE = {}


def golden(seed, r, hole_range):
    """-> (masks uint8 [n, r, r] of 0 / 255, state after the run as RandomState.get_state() gives it, candidates drawn)"""
    key = golden_name(seed, r, hole_range)
    if key not in _CACHE:
        g = np.load(os.path.join(GOLDEN, key))
        n = int(g["n"])
        bits = np.unpackbits(g["bits"])[:n * r * r].reshape(n, r, r)
        masks = (bits * 255).astype(np.uint8)
        masks.setflags(write=False)
        state = ("MT19937", g["key"].astype(np.uint32), int(g["pos"]), int(g["has_gauss"]), float(g["gauss"]))
        _CACHE[key] = (masks, state, int(g["candidates"]))
    return _CACHE[key]


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3]) and (
        np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes())


def coef_of(hole_range):
    """the reference's `coef`; hole_range None (no rejection) draws like [0, 1]"""
    return 1.0 if hole_range is None else min(hole_range[0] + hole_range[1], 1.0)


# ---- rounding as Pillow's ROUND_UP / ROUND_DOWN ---------------------------------------------------------------------------------
def ru(f):
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def rd(f):
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def _round32(v, up):
    """ROUND_UP / ROUND_DOWN of a float32 array: `f + 0.5F` is a float32 sum where f >= 0, a double one on |f| where f < 0"""
    v = v.astype(np.float32)
    half = np.float32(0.5)
    pos = np.floor(v + half) if up else np.ceil(v - half)
    a = np.abs(v).astype(np.float64)
    neg = -(np.floor(a + 0.5) if up else np.ceil(a - 0.5))
    return np.where(v >= 0, pos.astype(np.float64), neg).astype(np.int64)


def quad_of_segment(x0, y0, x1, y1, width):
    """ImagingDrawWideLine: the 12 plan words of one segment"""
    dx, dy = x1 - x0, y1 - y0
    if dx == 0 and dy == 0:
        xs, ys = [x0] * 4, [y0] * 4
    else:
        big = float(np.hypot(np.float64(dx), np.float64(dy)))      # (libm's hypot, the one Pillow calls; math.hypot is Python's own)
        small = (width - 1) / 2.0
        ratio_max, ratio_min = ru(small) / big, rd(small) / big
        dxmin, dxmax = rd(ratio_min * dy), rd(ratio_max * dy)
        dymin, dymax = ru(ratio_min * dx), ru(ratio_max * dx)
        xs = [x0 - dxmin, x1 - dxmin, x1 + dxmax, x0 + dxmax]
        ys = [y0 + dymax, y1 + dymax, y1 - dymin, y0 - dymin]
    slopes = []
    for k in range(4):
        ax, ay, bx, by = xs[k], ys[k], xs[(k + 1) % 4], ys[(k + 1) % 4]
        slopes.append(np.float32(0) if ay == by else np.float32(bx - ax) / np.float32(by - ay))
    return xs + ys + [int(v) for v in np.array(slopes, np.float32).view(np.int32)]


# ---- the draws of one candidate, in the reference's order ------------------------------------------------------------------------
def draw_plan(rng, s, coef):
    """one candidate of RandomMask(s) from `rng` (np.random.RandomState, or the np.random module) -> int32 plan"""
    rects, quads, discs = [], [], []
    for tries, max_size in ((int(10 * coef), s // 2), (int(5 * coef), s)):
        for _ in range(rng.randint(tries)):
            w, h = rng.randint(max_size), rng.randint(max_size)
            ww, hh = w // 2, h // 2
            x, y = rng.randint(-ww, s - w + ww), rng.randint(-hh, s - h + hh)
            rects += [max(x, 0), max(y, 0), min(x + w, s), min(y + h, s)]
    average_radius = math.sqrt(s * s + s * s) / 8
    mean_angle, angle_range = 2 * math.pi / 5, 2 * math.pi / 15
    for _ in range(rng.randint(int(20 * coef))):
        num_vertex = rng.randint(4, 18)
        angle_min = mean_angle - rng.uniform(0, angle_range)
        angle_max = mean_angle + rng.uniform(0, angle_range)
        angles = [(2 * math.pi - rng.uniform(angle_min, angle_max)) if i % 2 == 0 else rng.uniform(angle_min, angle_max) for i in range(num_vertex)]
        vertex = [(int(rng.randint(0, s)), int(rng.randint(0, s)))]
        for i in range(num_vertex):
            r = min(max(rng.normal(loc=average_radius, scale=average_radius // 2), 0), 2 * average_radius)
            new_x = min(max(vertex[-1][0] + r * math.cos(angles[i]), 0), s)
            new_y = min(max(vertex[-1][1] + r * math.sin(angles[i]), 0), s)
            vertex.append((int(new_x), int(new_y)))
        width = int(rng.uniform(12, 48))
        for a, b in zip(vertex[:-1], vertex[1:]):
            quads += quad_of_segment(a[0], a[1], b[0], b[1], width)
        for v in vertex:
            discs += [v[0], v[1], 2 * (width // 2)]
        rng.random_sample()                                        # the two discarded mask.transpose() draws, per stroke
        rng.random_sample()
    f0 = rng.random_sample() > 0.5
    f1 = rng.random_sample() > 0.5
    return np.array([len(rects) // 4, len(quads) // 12, len(discs) // 3, int(f0) | 2 * int(f1)] + rects + quads + discs, np.int32)


def split_plan(plan):
    nr, nq, nd, flips = (int(v) for v in plan[:4])
    a, b, c = 4, 4 + 4 * nr, 4 + 4 * nr + 12 * nq
    return plan[a:b].reshape(nr, 4), plan[b:c].reshape(nq, 12), plan[c:c + 3 * nd].reshape(nd, 3), flips


def make_plan(rects=(), quads=(), discs=(), flips=0):
    rects, quads, discs = [list(r) for r in rects], [list(q) for q in quads], [list(d) for d in discs]
    flat = [v for group in (rects, quads, discs) for item in group for v in item]
    return np.array([len(rects), len(quads), len(discs), flips] + flat, np.int32)


# ---- the raster ------------------------------------------------------------------------------------------------------------------
def disc_half_widths(d):
    """Pillow's quarter walk of the ellipse a = b = d: half-width X / 2 of the rows c +- k, k = 0 .. d / 2"""
    a = b = d
    def delta(x, y):
        return abs(a * a * y * y + b * b * x * x - a * a * b * b)
    cx, cy = a, b % 2
    half = {cy // 2: cx // 2}
    while (cx, cy) != (a % 2, b):
        nx, ny = cx, cy + 2
        nd = delta(nx, ny)
        if nx > 1:
            t = delta(cx - 2, cy + 2)
            if nd > t:
                nx, ny, nd = cx - 2, cy + 2, t
            t = delta(cx - 2, cy)
            if nd > t:
                nx, ny = cx - 2, cy
        cx, cy = nx, ny
        half.setdefault(cy // 2, cx // 2)                          # the first cx reached on a row
    return [half[k] for k in range(d // 2 + 1)]


def _quad_spans(quads, s):
    """polygon_generic over every quad at once -> (rows, first column, last column) of the spans, unclipped columns"""
    q = quads.astype(np.int64)
    X, Y = q[:, 0:4], q[:, 4:8]
    dx = quads[:, 8:12].astype(np.int32).view(np.float32)
    X1, Y1 = np.roll(X, -1, axis=1), np.roll(Y, -1, axis=1)
    exmin, exmax, eymin, eymax = np.minimum(X, X1), np.maximum(X, X1), np.minimum(Y, Y1), np.maximum(Y, Y1)
    horiz = Y == Y1
    ys, xa, xb = [eymin[horiz]], [exmin[horiz]], [exmax[horiz]]   # a horizontal edge is its own span
    qymax = np.minimum(Y.max(axis=1), s)[:, None, None]
    y = np.arange(s, dtype=np.int64)[None, :, None]
    active = ~horiz[:, None, :] & (y >= eymin[:, None, :]) & (y <= eymax[:, None, :])
    x = (y - Y[:, None, :]).astype(np.float32) * dx[:, None, :] + X[:, None, :].astype(np.float32)      # one fp32 product, one fp32 sum
    dup = active & (y == eymax[:, None, :]) & (y < qymax)
    inf = np.float32(np.inf)
    v = np.sort(np.concatenate([np.where(active, x, inf), np.where(dup, x, inf)], axis=2), axis=2)
    j = active.sum(axis=2) + dup.sum(axis=2)
    x_pos = np.zeros(j.shape, np.int64)
    rows = np.broadcast_to(y[:, :, 0], j.shape)
    for p in range(4):
        valid = 2 * p + 1 < j
        first, second = np.where(valid, v[:, :, 2 * p], 0), np.where(valid, v[:, :, 2 * p + 1], 0)
        x_end = _round32(second, up=False)
        ok = valid & ~(x_end < x_pos)
        x_start = np.maximum(_round32(first, up=True), x_pos)
        ok &= ~(x_end < x_start)
        ys.append(rows[ok]); xa.append(x_start[ok]); xb.append(x_end[ok])
        x_pos = np.where(ok, x_end + 1, x_pos)
    return np.concatenate(ys), np.concatenate(xa), np.concatenate(xb)


def _disc_spans(discs):
    ys, xa, xb = [], [], []
    for cx, cy, d in discs.astype(np.int64):
        hw = np.array(disc_half_widths(int(d)), np.int64) if d > 0 else np.zeros(1, np.int64)
        k = np.arange(-(d // 2), d // 2 + 1)
        ys.append(cy + k); xa.append(cx - hw[np.abs(k)]); xb.append(cx + hw[np.abs(k)])
    return np.concatenate(ys), np.concatenate(xa), np.concatenate(xb)


def _fill(s, ys, xa, xb):
    keep = (ys >= 0) & (ys < s) & (xb >= 0) & (xa < s)
    ys, xa, xb = ys[keep], np.maximum(xa[keep], 0), np.minimum(xb[keep], s - 1)
    keep = xa <= xb
    diff = np.zeros((s, s + 1), np.int32)
    np.add.at(diff, (ys[keep], xa[keep]), 1)
    np.add.at(diff, (ys[keep], xb[keep] + 1), -1)
    return np.cumsum(diff, axis=1)[:, :s] > 0


def raster(plan, s):
    """the mask of a plan: uint8 [s, s], 255 known, 0 hole"""
    rects, quads, discs, flips = split_plan(plan)
    brush = np.zeros((s, s), bool)
    if len(quads):
        brush |= _fill(s, *_quad_spans(quads, s))
    if len(discs):
        brush |= _fill(s, *_disc_spans(discs))
    if flips & 1:
        brush = brush[::-1]
    if flips & 2:
        brush = brush[:, ::-1]
    hole = brush.copy()
    for x0, y0, x1, y1 in rects:
        hole[y0:y1, x0:x1] = True
    return np.where(hole, 0, 255).astype(np.uint8)


def hole_ratio(mask):
    known = int(np.count_nonzero(mask))
    return 1.0 - known / float(mask.shape[0] * mask.shape[1])


def accepted(ratio, hole_range):
    return hole_range is None or not (ratio <= hole_range[0] or ratio >= hole_range[1])


def random_masks(n, s, hole_range, rng):
    """the restatement end to end -> (masks [n, s, s], candidates drawn, plans of the candidates)"""
    coef = coef_of(hole_range)
    out, plans = [], []
    while len(out) < n:
        plans.append(draw_plan(rng, s, coef))
        m = raster(plans[-1], s)
        if accepted(hole_ratio(m), hole_range):
            out.append(m)
    return np.stack(out), len(plans), plans


# ---- hand-made plans: what no seed reaches quickly -------------------------------------------------------------------------------
def capacity_plan(s, seed=5):
    """every table full: 13 rectangles, 323 quads, 342 discs, all widths"""
    r = np.random.RandomState(seed)
    rects = []
    for _ in range(MAX_RECTS):
        x0, y0 = int(r.randint(0, s)), int(r.randint(0, s))
        rects.append((x0, y0, min(s, x0 + int(r.randint(0, 6))), min(s, y0 + int(r.randint(0, 6)))))
    quads, discs = [], []
    for i in range(MAX_QUADS):
        a, b = r.randint(0, s + 1, 2), r.randint(0, s + 1, 2)
        quads.append(quad_of_segment(int(a[0]), int(a[1]), int(b[0]), int(b[1]), 12 + i % 36))
    for i in range(MAX_DISCS):
        c = r.randint(0, s + 1, 2)
        discs.append((int(c[0]), int(c[1]), DIAMETERS[i % len(DIAMETERS)]))
    return make_plan(rects, quads, discs, 0)


def edge_plans(s):
    """(name, plan): segments along x = s and y = s, a zero-length one inside and one on the border, every flip combination of an
    asymmetric figure, every diameter, a rectangle that covers all and an empty plan"""
    out = [("empty", make_plan()), ("all", make_plan(rects=[(0, 0, s, s)])), ("empty_rect", make_plan(rects=[(3, 3, 3, 9), (s, 0, s, s)]))]
    out.append(("along_x_eq_s", make_plan(quads=[quad_of_segment(s, 2, s, s - 3, 13)], discs=[(s, 2, 12)])))
    out.append(("along_y_eq_s", make_plan(quads=[quad_of_segment(1, s, s - 2, s, 14)], discs=[(s - 2, s, 14)])))
    out.append(("corner_s_s", make_plan(quads=[quad_of_segment(s, s, s - 9, s - 4, 47)], discs=[(s, s, 46)])))
    out.append(("zero_length", make_plan(quads=[quad_of_segment(5, 7, 5, 7, 20), quad_of_segment(s, 3, s, 3, 20), quad_of_segment(0, 0, 0, 0, 12)])))
    for flips in range(4):
        out.append((f"flips{flips}", make_plan(rects=[(1, 2, 4, 5)], quads=[quad_of_segment(3, 4, s - 6, s // 2, 12)], discs=[(s // 3, s - 5, 16)],
                                                flips=flips)))
    out.append(("diameters", make_plan(discs=[((7 * i) % s, (11 * i + 3) % s, d) for i, d in enumerate(DIAMETERS)])))
    out.append(("steep_and_flat", make_plan(quads=[quad_of_segment(2, 1, 3, s - 1, 25), quad_of_segment(0, s // 2, s, s // 2 + 1, 31),
                                                     quad_of_segment(s - 1, 0, 0, s - 1, 12), quad_of_segment(4, 4, 4, s - 4, 12),
                                                     quad_of_segment(s - 3, 9, 3, 9, 47)])))
    return out


def pack_plans(plans):
    """plans of one launch as the C ABI takes them: (int32 words, int64 offsets [k + 1])"""
    off = np.zeros(len(plans) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in plans])
    return np.ascontiguousarray(np.concatenate(plans), np.int32), off


# ---- the C ABI on host memory (CPU emulator) or device memory --------------------------------------------------------------------
class HostBackend:
    """mi-gan_amd/masks.py's backend over numpy arrays: the emulator library rasterises into host memory"""

    def __init__(self, lib):
        self.lib = lib
        self.launches = 0

    def empty(self, k, r):
        return np.full((k, r, r), 77, np.uint8)

    def raster(self, words, count, r, buf):
        assert buf.flags.c_contiguous and buf.shape[0] >= count
        words = np.ascontiguousarray(words, np.int32)
        holes = np.full((count, (r + BAND - 1) // BAND), -7, np.int32)
        self.lib.masks_raster(words.ctypes.data, words.size, count, r, buf.ctypes.data, holes.ctypes.data, 0)
        self.launches += 1
        return holes

    def holes(self, handle):
        return handle.astype(np.int64).sum(axis=1)

    def take(self, buf, idx, out, pos):
        out[pos:pos + len(idx)] = buf[list(idx)]


def emu_random_masks(pkg, lib, n, r, hole_range, rng, **kw):
    """random_masks through the emulator: mi-gan_amd/masks.py's own acceptance loop, host memory in place of the device's"""
    out = kw.pop("out", None)
    pkg.masks.check_arguments(n, r, hole_range)                  # (random_masks refuses before it allocates, too)
    if out is None:
        out = np.full((n, r, r), 99, np.uint8)
    backend = HostBackend(lib)
    ratios = pkg.masks.generate(backend, lib, n, r, hole_range, rng, out, **kw)
    return out, ratios, backend


def raster_plans(lib, mem, plans, r, odd=False):
    """one migan_masks_raster over hand-made plans -> (masks [k, r, r], hole pixels [k]); `mem`: HostMem or CudaMem"""
    words, off = pack_plans(plans)
    k = len(plans)
    buf = np.concatenate([(off + k + 1).astype(np.int32), words])
    nb = (r + BAND - 1) // BAND
    got, holes = mem.run(lib, buf, k, r, nb, odd)
    return got, holes.astype(np.int64).sum(axis=1)


class HostMem:
    def run(self, lib, buf, k, r, nb, odd):
        raw = np.full(k * r * r + 16, 55, np.uint8)
        shift = (1 if odd else 0) + (-raw.ctypes.data) % 16
        out = raw[shift:shift + k * r * r]
        holes = np.full((k, nb), -7, np.int32)
        lib.masks_raster(buf.ctypes.data, buf.size, k, r, out.ctypes.data, holes.ctypes.data, 0)
        assert (raw[:shift] == 55).all() and (raw[shift + k * r * r:] == 55).all()
        return out.reshape(k, r, r).copy(), holes


class CudaMem:
    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def run(self, lib, buf, k, r, nb, odd):
        torch = self.torch
        d_buf = torch.from_numpy(buf).to(self.device)
        raw = torch.full((k * r * r + 32,), 55, dtype=torch.uint8, device=self.device)
        shift = 17 if odd else 16
        out = raw[shift:shift + k * r * r]
        holes = torch.full((k, nb), -7, dtype=torch.int32, device=self.device)
        lib.masks_raster(d_buf.data_ptr(), buf.size, k, r, out.data_ptr(), holes.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((raw[:shift] == 55).all()) and bool((raw[shift + k * r * r:] == 55).all())
        return out.reshape(k, r, r).cpu().numpy(), holes.cpu().numpy()


def run_edge_plans(lib, mem, r):
    names, plans = zip(*edge_plans(r))
    for odd in (False, True):
        got, holes = raster_plans(lib, mem, list(plans), r, odd)
        for i, (name, plan) in enumerate(zip(names, plans)):
            want = raster(plan, r)
            assert np.array_equal(got[i], want), f"r {r} {name} odd {odd}: {int((got[i] != want).sum())} bytes differ"
            assert holes[i] == int((want == 0).sum()), f"r {r} {name}: hole count"


def run_capacity_plan(lib, mem, r):
    plan = capacity_plan(r)
    assert len(plan) == PLAN_WORDS_MAX
    got, holes = raster_plans(lib, mem, [plan, make_plan(), plan], r)
    want = raster(plan, r)
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and (got[1] == 255).all()
    assert holes[0] == holes[2] == int((want == 0).sum()) and holes[1] == 0


def run_refused_plans(lib, mem, r):
    """plans beyond the capacities or the buffer get a negative count; their neighbours are untouched by that"""
    good = make_plan(rects=[(1, 1, 5, 6)])
    too_many = make_plan(rects=[(0, 0, 1, 1)] * (MAX_RECTS + 1))
    bad_flips = make_plan(flips=4)
    got, holes = raster_plans(lib, mem, [good, too_many, bad_flips, good], r)
    assert holes[0] == holes[3] == 20 and holes[1] < 0 and holes[2] < 0
    assert np.array_equal(got[0], raster(good, r)) and np.array_equal(got[3], got[0])
    # a plan whose counts point past the end of the buffer
    words, off = pack_plans([good, good])
    buf = np.concatenate([(off + 3).astype(np.int32), words])
    buf[int(buf[1]) + 1] = MAX_QUADS                               # the last plan now claims 323 quads it does not have
    nb = (r + BAND - 1) // BAND
    got, holes = mem.run(lib, buf, 2, r, nb, False)
    assert holes[0].sum() == 20 and holes[1].sum() < 0


def run_arg_errors(lib, mem_ptr=12345 * 16):
    import pytest
    p = mem_ptr
    for kw in (dict(plans_ptr=0), dict(out_ptr=0), dict(holes_ptr=0), dict(resolution=15), dict(resolution=1025), dict(count=0),
               dict(count=65537), dict(words=3), dict(words=1 << 31), dict(plans_ptr=p + 2)):
        a = dict(plans_ptr=p, words=100, count=4, resolution=32, out_ptr=p, holes_ptr=p)
        a.update(kw)
        with pytest.raises(ValueError):
            lib.masks_raster(a["plans_ptr"], a["words"], a["count"], a["resolution"], a["out_ptr"], a["holes_ptr"], 0)
