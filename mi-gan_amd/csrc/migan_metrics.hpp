// PSNR / SSIM of completions against the ground-truth photo (include/migan_metrics_hip.h; reference lib/evaluator/eva_psnr.py:34-56
// and lib/evaluator/eva_ssim.py:11-41, size_average=False) as gfx950 kernels.  Compiled for the product and (tests/emu, through
// migan_host.hpp) for the CPU emulator; needs only the MIGAN_* macros of migan_rt_hip.h / hip_emu.h.
//
// One launch carries up to kMetItemsMax photos of different sizes, each with S completions.  A workgroup owns one kMetTW x kMetTH
// tile of one photo and walks the three channels.  Per channel it stages the photo's tile plus the window's 5-pixel halo in LDS,
// NORMALISED, zero outside the image (the reference's zero padding of the normalised image), and forms the photo's two windowed
// moments (mu1, E[g^2]) once; then it loops over the S completions: stage the completion's tile, form the three moments that depend
// on it (mu2, E[p^2], E[gp]), and add the map values and the squared differences of its four pixels per thread into partials.
// No moment, map or normalised image exists in global memory; a photo element is read once per tile, whatever S.
//
// The 11 x 11 window is the outer product of the 11 taps, so a moment is two 1-D passes in fp32:
//   pass 1 (vertical)    42 columns x 32 rows from the 42 x 42 staged tile; a thread owns 8 rows of one column (18 LDS reads of
//                        consecutive addresses across the lanes), 168 of the 256 threads work
//   pass 2 (horizontal)  32 x 32 from that; a thread owns 4 adjacent pixels of one row (14 LDS reads per moment)
// Per tile, channel and sample: 42 * 32 * 11 * 3 + 32 * 32 * 11 * 3 = 78 144 multiply-adds, against 121 * 5 * 1024 = 619 520 of the
// 2-D formulation.
//
// Addressing is by (row, pixel, channel) strides in elements, so one text serves planar [3][H][W] and interleaved [H][W][3]; the
// element type (uint8 or float32) is the template parameter.  Loads are per element: byte pointers need no alignment, and nothing
// outside [0, H) x [0, W) of a plane is read.
//
// Reduction (deterministic, no floating-point atomics): the workgroup adds its 256 partials in a fixed order in LDS and stores
// one (ssim sum, sse) pair per (tile, sample, channel) and one (|P|, |SSIM region|) pair per tile to scratch; metrics_final_kernel,
// one workgroup per output row, adds those in a fixed order and divides.  uint8 data: the sse is an integer throughout.
#pragma once

#include <cmath>
#include <cstddef>

namespace migan {

constexpr int kMetItemsMax = 32;
constexpr int kMetThreads = 256;
constexpr int kMetTW = 32, kMetTH = 32;                        // output tile
constexpr int kMetR = 5;                                       // halo: the window has 2 * kMetR + 1 = 11 taps
constexpr int kMetSW = kMetTW + 2 * kMetR, kMetSH = kMetTH + 2 * kMetR;       // staged tile, 42 x 42
constexpr int kMetStage = kMetSH * kMetSW;                     // floats of one staged tile
constexpr int kMetV = kMetTH * kMetSW;                         // floats of one moment after pass 1: [kMetTH][kMetSW]
constexpr int kMetLdsFloats = 2 * kMetStage + 3 * kMetV;       // photo tile, completion tile, three moments: 30 240 bytes
constexpr int kMetLdsBytes = kMetLdsFloats * 4;
constexpr int kMetFinalLdsBytes = kMetThreads * 4 * 8;
static_assert(kMetTW * kMetTH == 4 * kMetThreads && kMetTW == 32, "pass 2: a thread owns 4 adjacent pixels, 8 threads per row");
static_assert(kMetSW * (kMetTH / 8) <= kMetThreads, "pass 1: a thread owns 8 rows of one column");
static_assert((2 * kMetStage) % 2 == 0 && 3 * kMetV * 4 >= kMetThreads * 16, "the partial sums (8-byte) reuse the moments' LDS");

// gaussian(11, 1.5) of eva_ssim.py:11-13 as it comes out in float32: float32(exp(-(k - 5)^2 / 4.5)) / their float32 sum
#define MIGAN_MET_TAPS {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, \
                        0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}

struct MetItem {
  const void* gt;                    // one image
  const void* pred;                  // S images, tightly packed, gt's layout and type
  const unsigned char* mask;         // null or [H][W], 255 = known pixel
  int H, W;
};
struct MetArgs {
  MetItem item[kMetItemsMax];
  int first[kMetItemsMax + 1];       // first[k]: first workgroup (= tile slot in scratch) of item k
  void* part;                        // [tiles][S][3] MetPart
  unsigned* cnt;                     // [tiles][2]: pixels of the tile in P, pixels in the SSIM region
  double* out_mse;                   // [n * S] of this launch
  double* out_ssim;
  int n, S, shave, hwc;
  float lo, span;                    // float32 data: (v - lo) / span
};
static_assert(sizeof(MetArgs) <= 2048, "the metrics argument must stay well under the 4 KB kernel-argument limit");

template <bool U8> struct MetAcc { typedef double type; };
template <> struct MetAcc<true> { typedef unsigned long long type; };
template <bool U8>
struct MetPart {
  double ssim;                       // sum of the map over the SSIM region's pixels of one tile, sample and channel
  typename MetAcc<U8>::type sse;     // sum of squared differences over P: of bytes (integer) or of normalised fp32 values (fp64)
};

template <bool U8>
MIGAN_DEVICE MIGAN_INLINE float met_load(const void* base, size_t at, float lo, float span) {
  if (U8) return (float)static_cast<const unsigned char*>(base)[at] / 255.0f;
  return (static_cast<const float*>(base)[at] - lo) / span;
}

// the normalised tile of channel c around (ty0, tx0), halo included, zero outside the image
template <bool U8>
MIGAN_DEVICE MIGAN_INLINE void met_stage(float* dst, const void* img, int H, int W, size_t sr, size_t sp, size_t coff, int ty0, int tx0,
                                         float lo, float span, int t) {
  for (int e = t; e < kMetStage; e += kMetThreads) {
    const int y = ty0 - kMetR + e / kMetSW, x = tx0 - kMetR + e % kMetSW;
    float v = 0.0f;
    if (y >= 0 && y < H && x >= 0 && x < W) v = met_load<U8>(img, (size_t)y * sr + (size_t)x * sp + coff, lo, span);
    dst[e] = v;
  }
}

// One statement of a tap's arithmetic: the first tap is a rounded product, every further one a fused multiply-add, written out.  Left
// to the compiler's contraction, the photo's and the completion's moments come out of differently fused chains, and an identical pair
// -- whose map the reference's formulation gives as exactly 1 -- lands an ulp off in some pixels.
MIGAN_DEVICE MIGAN_INLINE float met_fma(float a, float b, float c) { return fmaf(a, b, c); }

// pass 1.  GT: V[0] = taps * g, V[1] = taps * g^2 down the columns of G.  Otherwise: V[0] = taps * p, V[1] = taps * p^2, V[2] = taps * gp
template <bool GT>
MIGAN_DEVICE MIGAN_INLINE void met_vpass(const float* G, const float* P, float* V, int t) {
#pragma clang fp contract(off)
  if (t >= kMetSW * (kMetTH / 8)) return;
  const float w[11] = MIGAN_MET_TAPS;
  const int x = t % kMetSW, r0 = t / kMetSW * 8;
  float a[18], b[18], c[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const float g = G[(r0 + i) * kMetSW + x];
    if (GT) {
      a[i] = g; b[i] = MIGAN_FMUL_RN(g, g);
    } else {
      const float q = P[(r0 + i) * kMetSW + x];
      a[i] = q; b[i] = MIGAN_FMUL_RN(q, q); c[i] = MIGAN_FMUL_RN(g, q);
    }
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    float s0 = MIGAN_FMUL_RN(w[0], a[o]), s1 = MIGAN_FMUL_RN(w[0], b[o]), s2 = GT ? 0.0f : MIGAN_FMUL_RN(w[0], c[o]);
#pragma unroll
    for (int k = 1; k < 11; ++k) {
      s0 = met_fma(w[k], a[o + k], s0);
      s1 = met_fma(w[k], b[o + k], s1);
      if (!GT) s2 = met_fma(w[k], c[o + k], s2);
    }
    V[(r0 + o) * kMetSW + x] = s0;
    V[kMetV + (r0 + o) * kMetSW + x] = s1;
    if (!GT) V[2 * kMetV + (r0 + o) * kMetSW + x] = s2;
  }
}
// pass 2: the thread's four pixels (row oy, columns ox ... ox + 3 of the tile) of moment plane V
MIGAN_DEVICE MIGAN_INLINE void met_hpass(const float* V, int oy, int ox, float out[4]) {
#pragma clang fp contract(off)
  const float w[11] = MIGAN_MET_TAPS;
  float v[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) v[i] = V[oy * kMetSW + ox + i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s = MIGAN_FMUL_RN(w[0], v[j]);
#pragma unroll
    for (int k = 1; k < 11; ++k) s = met_fma(w[k], v[j + k], s);
    out[j] = s;
  }
}

// eva_ssim.py:25-36 on one pixel's five moments, one rounding per operation as torch does it.  Contraction is off for this body (the
// pragma; __fmul_rn and its kin are plain operators to this compiler and contract like any other): the differences cancel, and
// mu1 * mu2 fused into sigma12 but rounded for the numerator's other factor leaves an identical pair an ulp off 1 in some pixels.
MIGAN_DEVICE MIGAN_INLINE float met_ssim_value(float mu1, float mu2, float e11, float e22, float e12) {
#pragma clang fp contract(off)
  const float C1 = 1e-4f, C2 = 9e-4f;
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
  return ((2.0f * mu1_mu2 + C1) * (2.0f * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2));
}

// sum of one value per thread in a fixed order (thread t < 32 adds t, t + 32, ..., then thread 0 adds those 32); the result is valid in
// thread 0 only.  `buf`: kMetThreads values of LDS nobody else uses between the barriers
template <class T>
MIGAN_DEVICE MIGAN_INLINE T met_block_sum(T* buf, T v, int t) {
  buf[t] = v;
  __syncthreads();
  if (t < 32) {
    T a = buf[t];
    for (int i = 1; i < kMetThreads / 32; ++i) a += buf[t + 32 * i];
    buf[t] = a;
  }
  __syncthreads();
  T a = 0;
  if (t == 0)
    for (int i = 0; i < 32; ++i) a += buf[i];
  return a;
}

template <bool U8>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 4) metrics_tile_kernel(const MetArgs p) {
  typedef typename MetAcc<U8>::type Acc;
  MIGAN_DYN_SMEM(smem);
  float* G = smem;                                       // [kMetSH][kMetSW] normalised photo tile, row ty0 - 5 ..., column tx0 - 5 ...
  float* P = G + kMetStage;                              // the same of the completion
  float* V = P + kMetStage;                              // [3][kMetTH][kMetSW] moments after pass 1; between passes, the partial sums
  const int t = (int)threadIdx.x;
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (workgroup-uniform)
  const MetItem& it = p.item[k];
  const int H = it.H, W = it.W;
  const int tile = (int)blockIdx.x - p.first[k], ntx = (W + kMetTW - 1) / kMetTW;
  const int ty0 = tile / ntx * kMetTH, tx0 = tile % ntx * kMetTW;
  const size_t plane = (size_t)H * W;
  const size_t sr = p.hwc ? 3 * (size_t)W : (size_t)W, sp = p.hwc ? 3 : 1, sc = p.hwc ? 1 : plane;
  MetPart<U8>* part = static_cast<MetPart<U8>*>(p.part) + (size_t)blockIdx.x * p.S * 3;

  // the thread's four pixels: which of them the SSIM mean runs over (inside the image, a hole where a mask is given), which are in P
  const int oy = t / 8, ox = t % 8 * 4, y = ty0 + oy;
  unsigned in_ssim = 0, in_p = 0;
  for (int j = 0; j < 4; ++j) {
    const int x = tx0 + ox + j;
    if (y >= H || x >= W) continue;
    if (it.mask != nullptr && it.mask[(size_t)y * W + x] == 255) continue;
    in_ssim |= 1u << j;
    if (y >= p.shave && y < H - p.shave && x >= p.shave && x < W - p.shave) in_p |= 1u << j;
  }
  unsigned* ri = reinterpret_cast<unsigned*>(V);
  const unsigned mine = (unsigned)__builtin_popcount(in_ssim) | ((unsigned)__builtin_popcount(in_p) << 16);     // (two sums <= 1024 in one word)
  const unsigned both = met_block_sum<unsigned>(ri, mine, t);
  if (t == 0) {
    ri[32] = both;
    p.cnt[2 * (size_t)blockIdx.x] = both >> 16;
    p.cnt[2 * (size_t)blockIdx.x + 1] = both & 0xffffu;
  }
  __syncthreads();
  const bool empty = ri[32] == 0;                        // workgroup-uniform: no pixel of this tile counts (every one is a known pixel)
  if (empty) {
    if (t == 0)
      for (int i = 0; i < p.S * 3; ++i) { part[i].ssim = 0.0; part[i].sse = 0; }
    return;
  }

  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                     // the last readers of G and V are done
    met_stage<U8>(G, it.gt, H, W, sr, sp, c * sc, ty0, tx0, p.lo, p.span, t);
    __syncthreads();
    met_vpass<true>(G, nullptr, V, t);
    __syncthreads();
    float mu1[4], e11[4];
    met_hpass(V, oy, ox, mu1);
    met_hpass(V + kMetV, oy, ox, e11);
    for (int s = 0; s < p.S; ++s) {
      __syncthreads();                                   // the last readers of P and V are done
      met_stage<U8>(P, it.pred, H, W, sr, sp, (size_t)s * 3 * plane + c * sc, ty0, tx0, p.lo, p.span, t);
      __syncthreads();
      met_vpass<false>(G, P, V, t);
      __syncthreads();
      float mu2[4], e22[4], e12[4];
      met_hpass(V, oy, ox, mu2);
      met_hpass(V + kMetV, oy, ox, e22);
      met_hpass(V + 2 * kMetV, oy, ox, e12);
      double ssim = 0.0;
      Acc sse = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (in_ssim >> j & 1u) ssim += (double)met_ssim_value(mu1[j], mu2[j], e11[j], e22[j], e12[j]);
        if (in_p >> j & 1u) {                            // eva_psnr.py:34-54
          const float g = G[(oy + kMetR) * kMetSW + ox + j + kMetR], q = P[(oy + kMetR) * kMetSW + ox + j + kMetR];
          if (U8) {
            // (the byte back from its normalised value: float(b) / 255 * 255 is within 3e-5 of b)
            const int d = (int)rintf(q * 255.0f) - (int)rintf(g * 255.0f);
            sse += (Acc)(d * d);
          } else {
            const float d = q - g;
            sse += (Acc)((double)d * (double)d);
          }
        }
      }
      __syncthreads();                                   // pass 2 has read V: the partial sums go there
      double* rd = reinterpret_cast<double*>(V);
      Acc* ra = reinterpret_cast<Acc*>(V + 2 * kMetThreads);
      const double tile_ssim = met_block_sum<double>(rd, ssim, t);
      const Acc tile_sse = met_block_sum<Acc>(ra, sse, t);
      if (t == 0) {
        part[s * 3 + c].ssim = tile_ssim;
        part[s * 3 + c].sse = tile_sse;
      }
    }
  }
}

// row r of the launch = sample r % S of item r / S: its tiles' partials, added in a fixed order (thread t takes tiles t, t + 256, ...
// and their channels in order, then met_block_sum), and the two divisions.  An empty region gives 0 / 0 = NaN.
template <bool U8>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) metrics_final_kernel(const MetArgs p) {
  typedef typename MetAcc<U8>::type Acc;
  MIGAN_DYN_SMEM(smem);
  const int t = (int)threadIdx.x;
  const int k = (int)blockIdx.x / p.S, s = (int)blockIdx.x % p.S;
  const int t0 = p.first[k], nt = p.first[k + 1] - t0;
  const MetPart<U8>* part = static_cast<const MetPart<U8>*>(p.part);
  double ssim = 0.0;
  Acc sse = 0;
  unsigned long long np = 0, ns = 0;
  for (int tile = t; tile < nt; tile += kMetThreads) {
    const MetPart<U8>* q = part + ((size_t)(t0 + tile) * p.S + s) * 3;
    for (int c = 0; c < 3; ++c) { ssim += q[c].ssim; sse += q[c].sse; }
    np += p.cnt[2 * (size_t)(t0 + tile)];
    ns += p.cnt[2 * (size_t)(t0 + tile) + 1];
  }
  double* rd = reinterpret_cast<double*>(smem);
  Acc* ra = reinterpret_cast<Acc*>(smem + 2 * kMetThreads);
  unsigned long long* rp = reinterpret_cast<unsigned long long*>(smem + 4 * kMetThreads);
  unsigned long long* rs = reinterpret_cast<unsigned long long*>(smem + 6 * kMetThreads);
  ssim = met_block_sum<double>(rd, ssim, t);
  sse = met_block_sum<Acc>(ra, sse, t);
  np = met_block_sum<unsigned long long>(rp, np, t);
  ns = met_block_sum<unsigned long long>(rs, ns, t);
  if (t != 0) return;
  const double count = (double)(3ull * np);              // eva_psnr.py:52-54: the mean over channels and the region's pixels
  p.out_mse[blockIdx.x] = U8 ? (double)sse / (count * 65025.0) : (double)sse / count;
  p.out_ssim[blockIdx.x] = ssim / (double)(3ull * ns);   // eva_ssim.py:41
}

// The kernels by element type, for the host.  Their instantiations live in a translation unit of their own, migan_metrics.hip (as
// comodgan_u8.hip's, comodgan_kernels.hpp: every symbol the library had keeps its code); the unit that holds the host code
// declares them (MIGAN_METRICS_ELSEWHERE); the CPU test harness, a single unit, defines them here.
struct MetForm {
  void (*tile)(const MetArgs);
  void (*final)(const MetArgs);
  const char* tile_name;
  const char* final_name;
};
MetForm metrics_form(bool u8);
#ifndef MIGAN_METRICS_ELSEWHERE
MetForm metrics_form(bool u8) {
  if (u8) return {metrics_tile_kernel<true>, metrics_final_kernel<true>, "migan::metrics_tile_kernel<true>", "migan::metrics_final_kernel<true>"};
  return {metrics_tile_kernel<false>, metrics_final_kernel<false>, "migan::metrics_tile_kernel<false>", "migan::metrics_final_kernel<false>"};
}
#endif  // MIGAN_METRICS_ELSEWHERE

}  // namespace migan
