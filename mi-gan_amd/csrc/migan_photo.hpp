// Photo loading on the device (include/migan_photo_hip.h): Pillow's Image.resize for uint8 images, BICUBIC and NEAREST, byte for
// byte, as gfx950 kernels.  Compiled for the product and (tests/emu, through migan_host.hpp) for the CPU emulator; needs only the
// MIGAN_* macros of migan_rt_hip.h / hip_emu.h.
//
// What Pillow computes (src/libImaging/Resample.c, precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc; Geometry.c, ImagingScaleAffine) and these kernels restate:
//   BICUBIC  per axis inS -> outS, in IEEE double and in this order of operations: scale = inS / outS, fs = max(scale, 1),
//            support = 2 fs, ksize = (int)ceil(support) * 2 + 1; per output xx: center = (xx + 0.5) scale,
//            xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), inS), the weights
//            w[x] = filter((x + xmin - center + 0.5) / fs) summed left to right, each divided by the sum and rounded to 22 fractional
//            bits away from zero.  out = clamp((2^21 + sum in[xmin + x] K[x]) >> 22, 0, 255), int32.  Horizontal pass first, into a
//            uint8 image of [sh][dw], then vertical; a pass whose sizes agree is skipped.
//   NEAREST  per axis idx[x] = (int)xo with xo = a0 * 0.5 to begin with and xo += a0 after every x, a0 = inS / outS: the repeated
//            addition IS the specification (the closed form rounds differently in tens of positions of an ordinary mask).
//
// Launches of one chunk of up to kPhItemsMax items of different sizes (host-built prefix of workgroups per item, as the metrics):
//   photo_table_kernel   the coefficient tables of both passes of every item, fp64 with contraction off (a fused multiply-add in
//                        filter or in center changes rounded coefficients), one thread per output index; the NEAREST index tables, one
//                        thread per (item, axis) doing the serial additions.  Layout of a BICUBIC table: int32 [outS][2] = (xmin, n),
//                        then int32 [ksize][outS], tap-major, so that lanes of consecutive outputs read consecutive words.
//   photo_hpass_kernel   a workgroup owns kPhTW output pixels of kPhTR rows.  The source bytes its taps touch are staged in LDS with
//                        whole aligned dwords where they lie inside the image and bounds-checked bytes at its two ends (neither W nor
//                        the row pitch has any alignment); a span longer than the stage is walked in pieces, left to right.  Each
//                        thread accumulates one output pixel's channels in int32 over ITS tap count, read from the table.
//   photo_vpass_kernel   the same sum down a column; a thread owns one output byte, consecutive threads consecutive bytes of a row.
//   photo_gather_kernel  NEAREST through the two index tables, optional inversion (255 - v) and threshold (v < 255 -> 0) in that order;
//                        also the copy of a BICUBIC item whose sizes agree (identity tables).
// No atomics; every output byte has one writer; nothing outside [0, sh) x [0, sw) x [0, C) of a source is read.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef MIGAN_HOST_DEVICE          // (the CPU emulator build is host code throughout)
#define MIGAN_HOST_DEVICE
#endif

namespace migan {

constexpr int kPhItemsMax = 32;
constexpr int kPhThreads = 256;
constexpr int kPhTW = 64, kPhTR = 4;                           // horizontal pass: output pixels x rows of a workgroup
constexpr int kPhRowBytes = 4096;                              // LDS bytes of one staged row piece, its misalignment (<= 3) included
constexpr int kPhLdsBytes = kPhTR * kPhRowBytes;
constexpr int kPhSrcMax = 16384, kPhDstMax = 4096, kPhAspectMax = 32;
constexpr int kPhPrecisionBits = 22;                           // Pillow's PRECISION_BITS = 32 - 8 - 2
static_assert(kPhTW * kPhTR == kPhThreads && kPhRowBytes % 4 == 0, "a thread owns one output pixel of one row");

// ks_h / ks_v: > 0 a BICUBIC pass with that ksize; 0 no pass on that axis; -1 a NEAREST index table
struct PhItem {
  const unsigned char* src;          // [sh][sw][C] of the launch this item is handed to
  unsigned char* dst;
  int sh, sw, dh, dw;
  unsigned tab_h, tab_v;             // first int32 of the item's horizontal / vertical table in PhArgs::tab
  int ks_h, ks_v;
};
struct PhArgs {
  PhItem item[kPhItemsMax];
  int first[kPhItemsMax + 1];        // first[k]: first workgroup of item k in this launch
  int* tab;
  int n, C, flags;                   // flags (gather only): bit 0 invert, bit 1 threshold
};
static_assert(sizeof(PhArgs) <= 2048, "the photo argument must stay well under the 4 KB kernel-argument limit");

MIGAN_HOST_DEVICE MIGAN_INLINE int ph_cdiv(int a, int b) { return (a + b - 1) / b; }
// workgroups of item `it` in the table launch: its horizontal coefficients, its vertical ones, one for NEAREST index tables
MIGAN_HOST_DEVICE MIGAN_INLINE int ph_table_groups_h(const PhItem& it) { return it.ks_h > 0 ? ph_cdiv(it.dw, kPhThreads) : 0; }
MIGAN_HOST_DEVICE MIGAN_INLINE int ph_table_groups_v(const PhItem& it) { return it.ks_v > 0 ? ph_cdiv(it.dh, kPhThreads) : 0; }
MIGAN_HOST_DEVICE MIGAN_INLINE int ph_table_groups(const PhItem& it) {
  return ph_table_groups_h(it) + ph_table_groups_v(it) + ((it.ks_h < 0 || it.ks_v < 0) ? 1 : 0);
}

// The kernels for the host.  They live in a translation unit of their own, migan_photo.hip (as the metrics': every symbol the
// library had keeps its code); the unit that holds the host code sees only this declaration (MIGAN_PHOTO_ELSEWHERE); the CPU test
// harness, a single unit, compiles them here.
struct PhForm {
  void (*table)(const PhArgs);
  void (*hpass[2])(const PhArgs);    // [0] one channel, [1] three
  void (*vpass[2])(const PhArgs);
  void (*gather[2])(const PhArgs);
};
PhForm photo_form();

#ifndef MIGAN_PHOTO_ELSEWHERE
// item of workgroup `bid` (workgroup-uniform; items without a workgroup in this launch are stepped over)
MIGAN_DEVICE MIGAN_INLINE int ph_item_of(const PhArgs& p, int bid) {
  int k = 0;
  while (k + 1 < p.n && bid >= p.first[k + 1]) ++k;
  return k;
}

// Resample.c bicubic_filter, a = -0.5
MIGAN_DEVICE MIGAN_INLINE double ph_bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// the table row of output xx of one axis inS -> outS: (xmin, n) and n rounded coefficients
MIGAN_DEVICE MIGAN_INLINE void ph_coeffs(int* tab, int inS, int outS, int ks, int xx) {
#pragma clang fp contract(off)
  const double scale = (double)inS / (double)outS;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > inS) xmax = inS;
  int n = xmax - xmin;
  if (n > ks) n = ks;                                    // (cannot happen: ksize covers 2 support + 1; keeps every write inside the table)
  if (n < 0) n = 0;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += ph_bicubic((x + xmin - center + 0.5) * ss);
  int* k = tab + 2 * (size_t)outS + xx;
  for (int x = 0; x < n; ++x) {
    double w = ph_bicubic((x + xmin - center + 0.5) * ss);       // (the same operands give the same weight as in the sum)
    if (ww != 0.0) w /= ww;
    k[(size_t)x * outS] = w < 0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
  }
  tab[2 * xx] = xmin;
  tab[2 * xx + 1] = n;
}

// Geometry.c ImagingScaleAffine: the source index of every output of one axis, by repeated addition
MIGAN_DEVICE MIGAN_INLINE void ph_nearest_table(int* idx, int inS, int outS) {
#pragma clang fp contract(off)
  const double a0 = (double)inS / (double)outS;
  double xo = a0 * 0.5;
  for (int x = 0; x < outS; ++x) {
    int i = (int)xo;
    if (i > inS - 1) i = inS - 1;                        // (not reached inside the domain: the sum's error is far below a0 / 2)
    idx[x] = i;
    xo += a0;
  }
}

MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) photo_table_kernel(const PhArgs p) {
  const int t = (int)threadIdx.x;
  const int k = ph_item_of(p, (int)blockIdx.x);
  const PhItem& it = p.item[k];
  const int g = (int)blockIdx.x - p.first[k], gh = ph_table_groups_h(it), gv = ph_table_groups_v(it);
  if (g < gh) {
    const int xx = g * kPhThreads + t;
    if (xx < it.dw) ph_coeffs(p.tab + it.tab_h, it.sw, it.dw, it.ks_h, xx);
  } else if (g < gh + gv) {
    const int yy = (g - gh) * kPhThreads + t;
    if (yy < it.dh) ph_coeffs(p.tab + it.tab_v, it.sh, it.dh, it.ks_v, yy);
  } else {
    if (t == 0 && it.ks_h < 0) ph_nearest_table(p.tab + it.tab_h, it.sw, it.dw);
    if (t == 64 && it.ks_v < 0) ph_nearest_table(p.tab + it.tab_v, it.sh, it.dh);       // (another wave: the two chains run side by side)
  }
}

MIGAN_DEVICE MIGAN_INLINE unsigned char ph_clip8(int acc) {
  const int v = acc >> kPhPrecisionBits;                 // (arithmetic shift, as Pillow's clip8)
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int C>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 4) photo_hpass_kernel(const PhArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned* lw = reinterpret_cast<unsigned*>(smem);
  const unsigned char* lb = reinterpret_cast<const unsigned char*>(smem);
  constexpr int kCap = (kPhRowBytes - 4) / C;            // source pixels of one staged piece
  const int t = (int)threadIdx.x;
  const int k = ph_item_of(p, (int)blockIdx.x);
  const PhItem& it = p.item[k];
  const int tile = (int)blockIdx.x - p.first[k], ntx = ph_cdiv(it.dw, kPhTW);
  const int x0 = tile % ntx * kPhTW, y0 = tile / ntx * kPhTR;
  const int r = t / kPhTW, ox = x0 + t % kPhTW, y = y0 + r;
  const int* bounds = p.tab + it.tab_h;
  const int* coef = bounds + 2 * (size_t)it.dw + ox;     // tap j of output ox: coef[j * dw]
  const int xl = (x0 + kPhTW < it.dw ? x0 + kPhTW : it.dw) - 1;
  const int lo = bounds[2 * x0], hi = bounds[2 * xl] + bounds[2 * xl + 1];      // source pixels [lo, hi) feed this tile (xmin and xmax never decrease)
  const bool live = ox < it.dw && y < it.sh;
  const int xmin = live ? bounds[2 * ox] : 0, n = live ? bounds[2 * ox + 1] : 0;
  const uintptr_t img0 = (uintptr_t)it.src, img1 = img0 + (size_t)it.sh * it.sw * C;      // the image's bytes: [img0, img1)
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << (kPhPrecisionBits - 1);
  for (int p0 = lo; p0 < hi; p0 += kCap) {               // (workgroup-uniform trip count)
    const int p1 = p0 + kCap < hi ? p0 + kCap : hi;
    __syncthreads();                                     // the last piece's readers are done
    for (int rr = 0; rr < kPhTR && y0 + rr < it.sh; ++rr) {
      const uintptr_t a0 = img0 + ((size_t)(y0 + rr) * it.sw + p0) * C;
      const uintptr_t w0 = a0 & ~(uintptr_t)3;           // aligned dwords from here hold the piece
      const int nwords = (int)((a0 - w0 + (size_t)(p1 - p0) * C + 3) / 4);
      for (int w = t; w < nwords; w += kPhThreads) {
        const uintptr_t q = w0 + 4 * (size_t)w;
        unsigned v = 0;
        if (q >= img0 && q + 4 <= img1) {
          v = *reinterpret_cast<const unsigned*>(q);
        } else {
          for (int j = 0; j < 4; ++j)
            if (q + j >= img0 && q + j < img1) v |= (unsigned)*reinterpret_cast<const unsigned char*>(q + j) << (8 * j);
        }
        lw[rr * (kPhRowBytes / 4) + w] = v;
      }
    }
    __syncthreads();
    if (live) {
      const int mis = (int)((img0 + ((size_t)y * it.sw + p0) * C) & 3);
      const unsigned char* row = lb + r * kPhRowBytes + mis;     // byte 0 of source pixel p0 of this thread's row
      const int j0 = p0 - xmin > 0 ? p0 - xmin : 0, j1 = p1 - xmin < n ? p1 - xmin : n;
      for (int j = j0; j < j1; ++j) {
        const int kv = coef[(size_t)j * it.dw];
        const unsigned char* px = row + (xmin + j - p0) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)px[c] * kv;
      }
    }
  }
  if (live) {
    unsigned char* out = it.dst + ((size_t)y * it.dw + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = ph_clip8(acc[c]);
  }
}

// src is [sh][dw][C] (the horizontal pass has run or was not needed); one output byte per thread
template <int C>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 4) photo_vpass_kernel(const PhArgs p) {
  const int k = ph_item_of(p, (int)blockIdx.x);
  const PhItem& it = p.item[k];
  const size_t rowb = (size_t)it.dw * C;
  const size_t e = (size_t)((int)blockIdx.x - p.first[k]) * kPhThreads + threadIdx.x;
  if (e >= (size_t)it.dh * rowb) return;
  const int y = (int)(e / rowb);
  const int* bounds = p.tab + it.tab_v;
  const int* coef = bounds + 2 * (size_t)it.dh + y;
  const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
  const unsigned char* s = it.src + (size_t)ymin * rowb + e % rowb;
  int acc = 1 << (kPhPrecisionBits - 1);
  for (int j = 0; j < n; ++j) acc += (int)s[(size_t)j * rowb] * coef[(size_t)j * it.dh];
  it.dst[e] = ph_clip8(acc);
}

template <int C>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 4) photo_gather_kernel(const PhArgs p) {
  const int k = ph_item_of(p, (int)blockIdx.x);
  const PhItem& it = p.item[k];
  const size_t rowb = (size_t)it.dw * C;
  const size_t e = (size_t)((int)blockIdx.x - p.first[k]) * kPhThreads + threadIdx.x;
  if (e >= (size_t)it.dh * rowb) return;
  const int y = (int)(e / rowb), xc = (int)(e % rowb), x = xc / C, c = xc % C;
  const int iy = p.tab[it.tab_v + y], ix = p.tab[it.tab_h + x];
  int v = it.src[((size_t)iy * it.sw + ix) * C + c];
  if (p.flags & 1) v = 255 - v;
  if ((p.flags & 2) && v < 255) v = 0;
  it.dst[e] = (unsigned char)v;
}

PhForm photo_form() {
  return {photo_table_kernel, {photo_hpass_kernel<1>, photo_hpass_kernel<3>}, {photo_vpass_kernel<1>, photo_vpass_kernel<3>},
          {photo_gather_kernel<1>, photo_gather_kernel<3>}};
}
#endif  // MIGAN_PHOTO_ELSEWHERE

}  // namespace migan
