// Random hole masks, host half (include/migan_masks_hip.h, migan_masks_draw): numpy's legacy generator and the draws of the
// reference's RandomMask (scripts/generate_masks.py:16-93), restated so that a seed gives the reference's masks and leaves the
// generator where the reference leaves it.  No GPU call in this file; the kernel that rasterises the plans is migan_masks.hpp's.
//
// numpy.random.RandomState, as far as RandomMask uses it:
//   genrand        MT19937, 624 words, regenerated when pos reaches 624
//   random_sample  two words a, b: ((a >> 5) * 2^26 + (b >> 6)) / 2^53
//   uniform(l, h)  l + (h - l) * random_sample
//   normal(m, s)   m + s * gauss; gauss is the polar method on pairs of random_sample, the second value of a pair kept for the next
//                  call (has_gauss, gauss: part of the state)
//   randint(l, h)  an int64 range h - 1 - l: nothing is drawn when it is 0; otherwise one word per try, masked with the smallest
//                  2^k - 1 that covers the range, drawn again while it exceeds the range
// Everything that rounds in double goes through the host's libm (log, sqrt, cos, sin, hypot), as numpy, CPython and Pillow do; the
// arithmetic keeps the reference's order of operations and is never contracted.
//
// One candidate, in the reference's order: MultiFill(int(10 coef), s / 2), MultiFill(int(5 coef), s) -- per rectangle w, h, x, y --
// then RandomBrush(int(20 coef), s): per stroke num_vertex, two uniforms for the angle window, num_vertex angles, the start vertex
// (x, y), num_vertex normals for the radii (vertices are int() of doubles clipped to [0, s]: s itself occurs), the width, and two
// random_sample whose mask.transpose() results the reference discards; after all strokes the two np.flip bits, which apply to the
// brush layer only.  Per stroke segment the corners of Pillow's wide-line quadrilateral (Draw.c, ImagingDrawWideLine) and the fp32
// slopes of its four edges (add_edge) are computed here, per vertex the ellipse's centre and diameter 2 (width / 2).
//
// Plan of one candidate, int32 words (what the kernel reads; tests/masks_case.py states the same):
//   [n_rect, n_quad, n_disc, flips] | n_rect x (x0, y0, x1, y1) half-open, clipped | n_quad x (x[4], y[4], dx[4] as fp32 bits) |
//   n_disc x (cx, cy, d).  A zero-length segment (Pillow draws the point) is a quadrilateral of four equal corners.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "migan_masks.hpp"

namespace migan {

constexpr int kMkMtN = 624, kMkMtM = 397;

struct MkRng {                       // = struct migan_masks_rng
  uint32_t key[kMkMtN];
  int pos, has_gauss;
  double gauss;
};

inline void mk_mt_gen(MkRng& s) {
  const uint32_t kUpper = 0x80000000u, kLower = 0x7fffffffu, kMatrixA = 0x9908b0dfu;
  uint32_t y;
  int i = 0;
  for (; i < kMkMtN - kMkMtM; ++i) {
    y = (s.key[i] & kUpper) | (s.key[i + 1] & kLower);
    s.key[i] = s.key[i + kMkMtM] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrixA);
  }
  for (; i < kMkMtN - 1; ++i) {
    y = (s.key[i] & kUpper) | (s.key[i + 1] & kLower);
    s.key[i] = s.key[i + (kMkMtM - kMkMtN)] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrixA);
  }
  y = (s.key[kMkMtN - 1] & kUpper) | (s.key[0] & kLower);
  s.key[kMkMtN - 1] = s.key[kMkMtM - 1] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrixA);
  s.pos = 0;
}
inline uint32_t mk_u32(MkRng& s) {
  if (s.pos >= kMkMtN) mk_mt_gen(s);
  uint32_t y = s.key[s.pos++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
inline double mk_double(MkRng& s) {
#pragma clang fp contract(off)
  const uint32_t a = mk_u32(s) >> 5, b = mk_u32(s) >> 6;
  return (a * 67108864.0 + b) / 9007199254740992.0;
}
inline double mk_uniform(MkRng& s, double lo, double hi) {
#pragma clang fp contract(off)
  const double range = hi - lo;
  return lo + range * mk_double(s);
}
inline double mk_gauss(MkRng& s) {
#pragma clang fp contract(off)
  if (s.has_gauss) {
    const double v = s.gauss;
    s.has_gauss = 0;
    s.gauss = 0.0;
    return v;
  }
  double x1, x2, r2;
  do {
    x1 = 2.0 * mk_double(s) - 1.0;
    x2 = 2.0 * mk_double(s) - 1.0;
    const double a = x1 * x1, b = x2 * x2;
    r2 = a + b;
  } while (r2 >= 1.0 || r2 == 0.0);
  const double f = std::sqrt(-2.0 * std::log(r2) / r2);
  s.gauss = f * x1;
  s.has_gauss = 1;
  return f * x2;
}
inline double mk_normal(MkRng& s, double loc, double scale) {
#pragma clang fp contract(off)
  const double g = scale * mk_gauss(s);
  return loc + g;
}
// randint(low, high): high > low
inline long long mk_randint(MkRng& s, long long low, long long high) {
  const uint64_t range = (uint64_t)(high - 1 - low);
  if (range == 0) return low;
  uint64_t mask = range;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16; mask |= mask >> 32;
  uint32_t v;
  do v = mk_u32(s) & (uint32_t)mask; while (v > range);          // (every range here is far below 2^32)
  return low + (long long)v;
}

// Pillow's ROUND_UP / ROUND_DOWN of a double
inline int mk_round_up_d(double f) { return (int)(f >= 0.0 ? std::floor(f + 0.5) : -std::floor(std::fabs(f) + 0.5)); }
inline int mk_round_down_d(double f) { return (int)(f >= 0.0 ? std::ceil(f - 0.5) : -std::ceil(std::fabs(f) - 0.5)); }

// ImagingDrawWideLine + add_edge: the 12 words of the segment (x0, y0) -> (x1, y1)
inline void mk_quad(int x0, int y0, int x1, int y1, int width, int32_t* q) {
#pragma clang fp contract(off)
  int xs[4], ys[4];
  const int dx = x1 - x0, dy = y1 - y0;
  if (dx == 0 && dy == 0) {
    for (int k = 0; k < 4; ++k) { xs[k] = x0; ys[k] = y0; }
  } else {
    const double big = std::hypot((double)dx, (double)dy);
    const double small = (width - 1) / 2.0;
    const double ratio_max = mk_round_up_d(small) / big, ratio_min = mk_round_down_d(small) / big;
    const int dxmin = mk_round_down_d(ratio_min * dy), dxmax = mk_round_down_d(ratio_max * dy);
    const int dymin = mk_round_up_d(ratio_min * dx), dymax = mk_round_up_d(ratio_max * dx);
    xs[0] = x0 - dxmin; ys[0] = y0 + dymax;
    xs[1] = x1 - dxmin; ys[1] = y1 + dymax;
    xs[2] = x1 + dxmax; ys[2] = y1 - dymin;
    xs[3] = x0 + dxmax; ys[3] = y0 - dymin;
  }
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3;
    const float slope = ys[k] == ys[k1] ? 0.0f : (float)(xs[k1] - xs[k]) / (float)(ys[k1] - ys[k]);
    q[k] = xs[k];
    q[4 + k] = ys[k];
    std::memcpy(&q[8 + k], &slope, 4);
  }
}

inline double mk_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the draws of one candidate of RandomMask(s); `plan`: kMkPlanWordsMax words, or null to advance the generator only.
// Returns the words written (counted for a null plan as well).
inline int mk_draw_candidate(MkRng& g, int s, double coef, int32_t* plan) {
#pragma clang fp contract(off)
  const double kPi = 3.141592653589793;                            // math.pi
  int32_t rects[4 * kMkRects], discs[3 * kMkDiscs];
  int32_t quads_local[12];
  int nr = 0, nq = 0, nd = 0;
  int32_t* quads = plan ? plan + 4 + 4 * kMkRects : nullptr;       // staged behind the widest rectangle table, moved down at the end
  const int tries[2] = {(int)(10 * coef), (int)(5 * coef)};
  const int sizes[2] = {s / 2, s};
  for (int m = 0; m < 2; ++m) {
    const int fills = (int)mk_randint(g, 0, tries[m]);
    for (int i = 0; i < fills; ++i) {
      const int w = (int)mk_randint(g, 0, sizes[m]), h = (int)mk_randint(g, 0, sizes[m]);
      const int ww = w / 2, hh = h / 2;
      const int x = (int)mk_randint(g, -ww, s - w + ww), y = (int)mk_randint(g, -hh, s - h + hh);
      int32_t* r = rects + 4 * nr++;
      r[0] = x > 0 ? x : 0; r[1] = y > 0 ? y : 0;
      r[2] = x + w < s ? x + w : s; r[3] = y + h < s ? y + h : s;
    }
  }
  const double average_radius = std::sqrt((double)(s * s + s * s)) / 8;
  const double radius_scale = std::floor(average_radius / 2);      // average_radius // 2
  const double mean_angle = 2 * kPi / 5, angle_range = 2 * kPi / 15;
  const int strokes = (int)mk_randint(g, 0, (int)(20 * coef));
  for (int st = 0; st < strokes; ++st) {
    const int num_vertex = (int)mk_randint(g, 4, 18);
    const double angle_min = mean_angle - mk_uniform(g, 0, angle_range);
    const double angle_max = mean_angle + mk_uniform(g, 0, angle_range);
    double angles[kMkPoints];
    for (int i = 0; i < num_vertex; ++i) angles[i] = i % 2 == 0 ? 2 * kPi - mk_uniform(g, angle_min, angle_max) : mk_uniform(g, angle_min, angle_max);
    int vx[kMkPoints], vy[kMkPoints];
    vx[0] = (int)mk_randint(g, 0, s);
    vy[0] = (int)mk_randint(g, 0, s);
    for (int i = 0; i < num_vertex; ++i) {
      const double r = mk_clip(mk_normal(g, average_radius, radius_scale), 0, 2 * average_radius);
      const double px = r * std::cos(angles[i]), py = r * std::sin(angles[i]);
      vx[i + 1] = (int)mk_clip(vx[i] + px, 0, s);
      vy[i + 1] = (int)mk_clip(vy[i] + py, 0, s);
    }
    const int width = (int)mk_uniform(g, 12, 48);
    for (int i = 0; i < num_vertex; ++i, ++nq) mk_quad(vx[i], vy[i], vx[i + 1], vy[i + 1], width, quads ? quads + 12 * nq : quads_local);
    for (int i = 0; i <= num_vertex; ++i, ++nd) {
      discs[3 * nd] = vx[i]; discs[3 * nd + 1] = vy[i]; discs[3 * nd + 2] = 2 * (width / 2);
    }
    mk_double(g);                                                  // the two mask.transpose() results are discarded, their draws are not
    mk_double(g);
  }
  const int f0 = mk_double(g) > 0.5;
  const int f1 = mk_double(g) > 0.5;
  const int words = 4 + 4 * nr + 12 * nq + 3 * nd;
  if (plan) {
    plan[0] = nr; plan[1] = nq; plan[2] = nd; plan[3] = f0 | (f1 << 1);
    std::memcpy(plan + 4, rects, sizeof(int32_t) * 4 * nr);
    std::memmove(plan + 4 + 4 * nr, quads, sizeof(int32_t) * 12 * nq);
    std::memcpy(plan + 4 + 4 * nr + 12 * nq, discs, sizeof(int32_t) * 3 * nd);
  }
  return words;
}

}  // namespace migan
