// Random hole masks on the device (include/migan_masks_hip.h): one gfx950 kernel rasterises the plans the host drew
// (migan_masks_host.hpp) exactly as Pillow's ImageDraw rasterises the reference's strokes, composes them with the rectangles and
// counts the hole pixels.  Compiled for the product and (tests/emu, through migan_host.hpp) for the CPU emulator; needs only the
// MIGAN_* macros of migan_rt_hip.h / hip_emu.h.
//
// What Pillow computes (src/libImaging/Draw.c) and this kernel restates, for an image of s x s:
//   wide line    polygon_generic over the four edges of the quadrilateral.  A horizontal edge is the span [xmin, xmax] on its row.  On
//                every row y of [max(ymin, 0), min(ymax, s)] each other edge with ymin_e <= y <= ymax_e contributes
//                x = (float)(y - y0) * dx + (float)x0 -- ONE fp32 product and ONE fp32 sum (a fused multiply-add gives other pixels) --
//                and contributes it twice when y == ymax_e and y < ymax.  The <= 8 values are sorted and taken in pairs with a running
//                x_pos = 0: x_end = ROUND_DOWN(second), skipped when x_end < x_pos; x_start = max(ROUND_UP(first), x_pos), skipped when
//                x_end < x_start; the span [x_start, x_end] is filled and x_pos = x_end + 1.
//                ROUND_UP(f) = f >= 0 ? floor(f + 0.5F) : -floor(fabs(f) + 0.5F), ROUND_DOWN(f) = f >= 0 ? ceil(f - 0.5F) : -ceil(fabs(f) - 0.5F):
//                a float sum where f >= 0, a double one on |f| where f < 0.
//   ellipse      the quarter walk with a = b = d from (d, 0) to (0, d): a step goes to (cx, cy + 2) unless cx > 1 and
//                |a^2 y^2 + b^2 x^2 - a^2 b^2| (int64) is strictly smaller at (cx - 2, cy + 2), and then at (cx - 2, cy); the first cx
//                reached on a cy is the half-width of the rows c +- cy / 2.  Only the 18 even diameters 12 .. 46 occur: every workgroup
//                builds their table in LDS, one thread per diameter.
//   composition  a brush pixel (x, y) lands at (f1 ? s - 1 - x : x, f0 ? s - 1 - y : y); a pixel is a hole (0) where a rectangle or a
//                landed brush pixel covers it, known (255) elsewhere.
//
// masks_raster_kernel: a workgroup of 256 threads owns a band of kMkBand rows of one candidate as a bit image in LDS (s <= 1024: 32
// words per row).  Threads take (primitive, row) pairs -- consecutive threads consecutive rows of one primitive, so the lanes of a wave
// read the same plan words and touch different LDS rows -- and OR the spans in with LDS integer atomics; then every output byte is
// written once, 16 at a time where s % 16 == 0, and the band's hole pixels are counted with popcounts and one LDS integer add per
// thread.  Integers only behind the fp32 row formula: two runs give the same bytes and counts.  The plan words are checked against
// the capacities and the buffer before anything is read through them; a candidate whose plan fails gets a negative count.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef MIGAN_ATOMIC_OR_U32
// the CPU emulator: the lanes of a workgroup share one OS thread, workgroups run on several
#define MIGAN_ATOMIC_ADD_I32(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define MIGAN_ATOMIC_OR_U32(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#endif

namespace migan {

constexpr int kMkThreads = 256;
constexpr int kMkBand = 32;                                    // rows of one workgroup
constexpr int kMkResMin = 16, kMkResMax = 1024;
constexpr int kMkRowWords = kMkResMax / 32;
// capacities that follow from the reference's text: randint(10) + randint(5) rectangles, randint(20) strokes of randint(4, 18) + 1 points
constexpr int kMkRects = 13, kMkStrokes = 19, kMkPoints = 18;
constexpr int kMkQuads = kMkStrokes * (kMkPoints - 1), kMkDiscs = kMkStrokes * kMkPoints;
constexpr int kMkPlanWordsMax = 4 + 4 * kMkRects + 12 * kMkQuads + 3 * kMkDiscs;
constexpr int kMkDiamMin = 12, kMkDiams = 18, kMkHalfRows = 24;      // diameters 12, 14 .. 46; rows 0 .. d / 2 of a quarter
constexpr int kMkCountMax = 65536;                             // candidates of one launch
// LDS, in words: the bit image | the half-width tables | the band's hole count
constexpr int kMkLdsImg = 0, kMkLdsDisc = kMkBand * kMkRowWords, kMkLdsHoles = kMkLdsDisc + kMkDiams * kMkHalfRows;
constexpr int kMkLdsBytes = (kMkLdsHoles + 4) * 4;
static_assert(kMkDiamMin + 2 * (kMkDiams - 1) <= 2 * (kMkHalfRows - 1), "a quarter of the largest diameter fits its table row");

struct MkArgs {
  const int* plans;                  // [count + 1] word offsets, then the plans (migan_masks_draw's layout)
  unsigned char* out;                // [count][R][R]
  int* holes;                        // [count][bands]: hole pixels of the band; negative: the plan was refused
  unsigned words;                    // words behind `plans`
  int count, R;
  int wide;                          // 16-byte stores (R % 16 == 0 and `out` aligned)
};

MIGAN_HOST_DEVICE MIGAN_INLINE int mk_bands(int R) { return (R + kMkBand - 1) / kMkBand; }

void (*masks_form())(const MkArgs);  // the kernel for the host (it lives in migan_masks.hip: every symbol the library had keeps its code)

#ifndef MIGAN_MASKS_ELSEWHERE
typedef unsigned mk_u4 __attribute__((ext_vector_type(4)));

MIGAN_DEVICE MIGAN_INLINE float mk_bound(float f) { return f < -1.0e6f ? -1.0e6f : (f > 1.0e6f ? 1.0e6f : f); }      // (no coordinate comes near)
MIGAN_DEVICE MIGAN_INLINE int mk_round_up(float f) {
#pragma clang fp contract(off)
  f = mk_bound(f);
  return f >= 0.0f ? (int)__builtin_floorf(f + 0.5f) : -(int)__builtin_floor(__builtin_fabs((double)f) + 0.5);
}
MIGAN_DEVICE MIGAN_INLINE int mk_round_down(float f) {
#pragma clang fp contract(off)
  f = mk_bound(f);
  return f >= 0.0f ? (int)__builtin_ceilf(f - 0.5f) : -(int)__builtin_ceil(__builtin_fabs((double)f) - 0.5);
}

// |a^2 y^2 + b^2 x^2 - a^2 b^2| with a = b = d
MIGAN_DEVICE MIGAN_INLINE long long mk_delta(long long d, long long x, long long y) {
  const long long v = d * d * y * y + d * d * x * x - d * d * d * d;
  return v < 0 ? -v : v;
}
// hw[k] = half-width of the rows c +- k of the ellipse of diameter d, k = 0 .. d / 2
MIGAN_DEVICE MIGAN_INLINE void mk_disc_table(int* hw, int d) {
  int cx = d, cy = 0;
  hw[0] = d >> 1;
  for (int step = 0; step < 4 * d + 8 && !(cx == 0 && cy == d); ++step) {      // (every step lowers cx or raises cy: d steps at the most)
    int nx = cx, ny = cy + 2;
    long long nd = mk_delta(d, nx, ny);
    if (nx > 1) {
      long long t = mk_delta(d, cx - 2, cy + 2);
      if (nd > t) { nx = cx - 2; ny = cy + 2; nd = t; }
      t = mk_delta(d, cx - 2, cy);
      if (nd > t) { nx = cx - 2; ny = cy; }
    }
    if (ny != cy && ny <= d) hw[ny >> 1] = nx >> 1;      // the first cx reached on a new row
    cx = nx; cy = ny;
  }
}

// OR the span [xs, xe] of a source row into the landed row `row` (f1: the columns are mirrored)
MIGAN_DEVICE MIGAN_INLINE void mk_span(unsigned* row, int xs, int xe, int R, bool f1) {
  if (xs < 0) xs = 0;
  if (xe > R - 1) xe = R - 1;
  if (xs > xe) return;
  if (f1) { const int t = xs; xs = R - 1 - xe; xe = R - 1 - t; }
  const int w0 = xs >> 5, w1 = xe >> 5;
  for (int w = w0; w <= w1; ++w) {
    unsigned m = 0xffffffffu;
    if (w == w0) m &= 0xffffffffu << (xs & 31);
    if (w == w1) m &= 0xffffffffu >> (31 - (xe & 31));
    MIGAN_ATOMIC_OR_U32(row + w, m);
  }
}

#define MK_CSWAP(a, b) do { const float lo_ = v[a] < v[b] ? v[a] : v[b], hi_ = v[a] < v[b] ? v[b] : v[a]; v[a] = lo_; v[b] = hi_; } while (0)

// polygon_generic on row y of one quadrilateral q = (x[4], y[4], dx[4])
MIGAN_DEVICE MIGAN_INLINE void mk_quad_row(const int* q, int y, unsigned* row, int R, bool f1) {
#pragma clang fp contract(off)
  int X[4], Y[4];
  float D[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    X[k] = q[k];
    Y[k] = q[4 + k];
    D[k] = __builtin_bit_cast(float, q[8 + k]);
  }
  int ymin = Y[0], ymax = Y[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    ymin = Y[k] < ymin ? Y[k] : ymin;
    ymax = Y[k] > ymax ? Y[k] : ymax;
  }
  if (y < ymin || y > ymax) return;
  if (ymax > R) ymax = R;
  float v[8];
  int j = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3;
    const int x0 = X[k], y0 = Y[k], x1 = X[k1], y1 = Y[k1];
    const int eymin = y0 < y1 ? y0 : y1, eymax = y0 < y1 ? y1 : y0;
    const bool horizontal = y0 == y1;
    if (horizontal && y == y0) mk_span(row, x0 < x1 ? x0 : x1, x0 < x1 ? x1 : x0, R, f1);
    const bool active = !horizontal && y >= eymin && y <= eymax;
    const float prod = (float)(y - y0) * D[k];
    const float x = prod + (float)x0;
    const bool twice = active && y == eymax && y < ymax;
    v[2 * k] = active ? x : __builtin_inff();
    v[2 * k + 1] = twice ? x : __builtin_inff();
    j += (active ? 1 : 0) + (twice ? 1 : 0);
  }
  // Batcher's odd-even merge sort of 8 (the absent values are +inf and end up last)
  MK_CSWAP(0, 1); MK_CSWAP(2, 3); MK_CSWAP(4, 5); MK_CSWAP(6, 7);
  MK_CSWAP(0, 2); MK_CSWAP(1, 3); MK_CSWAP(4, 6); MK_CSWAP(5, 7);
  MK_CSWAP(1, 2); MK_CSWAP(5, 6);
  MK_CSWAP(0, 4); MK_CSWAP(1, 5); MK_CSWAP(2, 6); MK_CSWAP(3, 7);
  MK_CSWAP(2, 4); MK_CSWAP(3, 5);
  MK_CSWAP(1, 2); MK_CSWAP(3, 4); MK_CSWAP(5, 6);
  int x_pos = 0;
#pragma unroll
  for (int i = 1; i < 8; i += 2) {
    if (i >= j) break;
    const int x_end = mk_round_down(v[i]);
    if (x_end < x_pos) continue;
    int x_start = mk_round_up(v[i - 1]);
    if (x_pos > x_start) {
      x_start = x_pos;
      if (x_end < x_start) continue;
    }
    mk_span(row, x_start, x_end, R, f1);
    x_pos = x_end + 1;
  }
}
#undef MK_CSWAP

MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 4) masks_raster_kernel(const MkArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned* img = reinterpret_cast<unsigned*>(smem) + kMkLdsImg;
  int* disc = reinterpret_cast<int*>(smem) + kMkLdsDisc;
  int* holes = reinterpret_cast<int*>(smem) + kMkLdsHoles;
  const int t = (int)threadIdx.x, R = p.R;
  const int nb = mk_bands(R), c = (int)blockIdx.x / nb, band = (int)blockIdx.x % nb;
  const int r0 = band * kMkBand, rows = R - r0 < kMkBand ? R - r0 : kMkBand, W32 = (R + 31) >> 5;
  for (int i = t; i < kMkBand * kMkRowWords; i += kMkThreads) img[i] = 0u;
  if (t < kMkDiams) mk_disc_table(disc + t * kMkHalfRows, kMkDiamMin + 2 * t);
  if (t == 64) holes[0] = 0;
  // the plan, checked before anything is read through it (workgroup-uniform)
  const unsigned off = (unsigned)p.plans[c];
  bool ok = off >= (unsigned)p.count + 1u && off <= p.words && p.words - off >= 4u;
  int nr = 0, nq = 0, nd = 0, flips = 0;
  if (ok) {
    nr = p.plans[off]; nq = p.plans[off + 1]; nd = p.plans[off + 2]; flips = p.plans[off + 3];
    ok = nr >= 0 && nr <= kMkRects && nq >= 0 && nq <= kMkQuads && nd >= 0 && nd <= kMkDiscs && (flips & ~3) == 0;
    ok = ok && p.words - off >= (unsigned)(4 + 4 * nr + 12 * nq + 3 * nd);
  }
  if (!ok) nr = nq = nd = 0;
  const int* rect = p.plans + off + 4;
  const int* quad = rect + 4 * nr;
  const int* dsc = quad + 12 * nq;
  const bool f0 = (flips & 1) != 0, f1 = (flips & 2) != 0;
  __syncthreads();
  const int items = (nr + nq + nd) * kMkBand;
  for (int i = t; i < items; i += kMkThreads) {
    const int prim = i / kMkBand, j = i % kMkBand;
    if (j >= rows) continue;
    unsigned* row = img + j * kMkRowWords;
    const int yo = r0 + j, ys = f0 ? R - 1 - yo : yo;            // the landed row, and the brush row that lands on it
    if (prim < nr) {
      const int* r = rect + 4 * prim;
      if (yo >= r[1] && yo < r[3]) mk_span(row, r[0], r[2] - 1, R, false);
    } else if (prim < nr + nq) {
      mk_quad_row(quad + 12 * (prim - nr), ys, row, R, f1);
    } else {
      const int* d = dsc + 3 * (prim - nr - nq);
      const int di = (d[2] - kMkDiamMin) >> 1;
      int k = ys - d[1];
      k = k < 0 ? -k : k;
      if ((d[2] & 1) == 0 && di >= 0 && di < kMkDiams && k <= (d[2] >> 1)) {
        const int X = disc[di * kMkHalfRows + k];
        mk_span(row, d[0] - X, d[0] + X, R, f1);
      }
    }
  }
  __syncthreads();
  unsigned char* out = p.out + (size_t)c * R * R + (size_t)r0 * R;
  if (p.wide) {
    const int G = R >> 4;
    for (int i = t; i < rows * G; i += kMkThreads) {
      const int j = i / G, g = i % G;
      const unsigned bits = img[j * kMkRowWords + (g >> 1)] >> (16 * (g & 1));
      mk_u4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned m = (bits >> (4 * e)) & 15u;
        const unsigned hole = ((m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21)) * 255u;
        w[e] = ~hole;
      }
      *reinterpret_cast<mk_u4*>(out + (size_t)j * R + 16 * g) = w;
    }
  } else {
    const int G = (R + 3) >> 2;
    for (int i = t; i < rows * G; i += kMkThreads) {
      const int j = i / G, x = 4 * (i % G);
      const unsigned bits = img[j * kMkRowWords + (x >> 5)] >> (x & 31);
      for (int e = 0; e < 4 && x + e < R; ++e) out[(size_t)j * R + x + e] = ((bits >> e) & 1u) ? 0 : 255;
    }
  }
  int local = 0;
  for (int i = t; i < rows * W32; i += kMkThreads) {
    const int w = i % W32;
    unsigned m = img[(i / W32) * kMkRowWords + w];
    if (w == W32 - 1 && (R & 31)) m &= 0xffffffffu >> (32 - (R & 31));      // (mk_span never sets a bit beyond R - 1; kept for the count's sake)
    local += __builtin_popcount(m);
  }
  if (local) MIGAN_ATOMIC_ADD_I32(holes, local);
  __syncthreads();
  if (t == 0) p.holes[blockIdx.x] = ok ? holes[0] : -1 - R * R;
}

void (*masks_form())(const MkArgs) { return masks_raster_kernel; }
#endif  // MIGAN_MASKS_ELSEWHERE

}  // namespace migan
