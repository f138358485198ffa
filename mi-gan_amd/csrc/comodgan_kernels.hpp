// Co-Mod-GAN generator forward: gfx950 (MI355X / CDNA4) device kernels.
//
// Reference being replaced: lib/model_zoo/comodgan.py::Generator.forward (:435-455) = Mapping (stylegan.py:396-439),
// Encoder (comodgan.py:192-204), Synthesis (comodgan.py:395-420); layers stylegan.py: dense :64-99,
// modulated_conv2d :102-195, conv2d_layer :197-244, synthesis_layer :247-309, torgb_layer :312-344;
// resampling torch_utils/ops/conv2d_resample.py and upfirdn2d.py.
//
// Everything that is a dense contraction (the 3x3 convolutions, 99 % of the 240 GFLOP per 512x512 image) runs
// on the matrix cores as an implicit GEMM (cm_conv_kernel); the rest are streaming kernels:
//
//   cm_*_h_kernel       the typed twins of the conv / FIR / FromRGB / ToRGB kernels: _Float16 activation tensors in the blocks a
//                       caller has declared half precision, with comodgan_set_fp16_storage on (fp32 arithmetic on converted values).
//                       A twin is a symbol, not a text: each of these four layers has one body, comodgan_{conv,fir,fromrgb,torgb}_body.inc,
//                       compiled into every symbol of its family with the element types as constants of the enclosing kernel
//   cm_conv_kernel      3x3 convolution, NHWC, M = 8x16 output-grid pixels, N = 64/128 output channels, K = taps x Cin.
//                       A operand: the input halo tile of a 32-channel chunk is staged ONCE in LDS (scaled by the
//                       per-sample style = the "scale activations" form of weight modulation, stylegan.py:171-182,
//                       split into two fp16 planes) and re-read at 1..9 shifted positions, one per filter tap.
//                       B operand: per (tap, chunk) weight tile, pre-split fp16 planes, double-buffered in LDS.
//                       v_mfma_f32_32x32x16_f16 x 3 per fp32 product (error-compensated, fp32 accumulate), same
//                       scheme as the MI-GAN 1x1 GEMM (migan_kernels.hpp, GEMMV 2).
//                       Epilogue: per-(sample, channel) demodulation coefficient, noise, bias, lrelu*sqrt2, clamp, skip.
//                       The tap list is data: plain 3x3 (9 taps, stride 1), stride-2 on the FIR-filtered input
//                       (encoder down path), and the four output phases of the stride-2 transposed convolution
//                       (synthesis up path: 4 + 2 + 2 + 1 taps, no multiplications by inserted zeros) -- one launch per
//                       phase, or all four in one launch with one accumulator set per phase.
//                       Tiles: 8x16 pixels x 64/128 channels (two waves per SIMD) or 16x16 pixels x 256 channels (one
//                       wave per SIMD, 128x128 wave tiles, accumulators in AGPRs), chosen per launch by the host.
//   cm_fir_kernel<0>    upfirdn2d [1,3,3,1] FIR with pad 2 in front of the strided convolution (conv2d_resample down path)
//   cm_fir_kernel<1>    upfirdn2d FIR (gain 4) behind the transposed convolution + noise/bias/activation/skip epilogue
//   cm_fir_samples_kernel, cm_dense_multi_samples_kernel, cm_bcast_kernel   the three places of an S-samples forward
//                       (comodgan_forward_samples) where a per-sample launch reads a per-image operand: sample b -> image b / S.
//                       The first is the FIR body with SAMP set, the second shares cm_affine_job with cm_dense_multi_kernel
//   cm_fromrgb_kernel   1x1 conv 4 -> C with bias and activation, NCHW planes -> NHWC
//   cm_torgb_kernel     modulated 1x1 conv C -> 3 (no demodulation) + bias + 2x FIR upsample of the running image
//   cm_fromrgb_u8_kernel, cm_torgb_u8_kernel   the first and the last launch of a uint8 forward (comodgan_forward_u8): the same two
//                       bodies with migan_pack_input's arithmetic in front and migan_compose_output's behind, photo and mask bytes in,
//                       composited bytes out
//   cm_dense_kernel     fully connected layers (mapping, affine, encoder fc, synthesis fc): weight streaming, fp32 FMA
//   cm_wprep_kernel     per-tensor statistics: max |w| per output channel (fp16 range scale), demodulation sums of w^2
//   cm_style_multi_kernel  styles -> normalised input scales (with the per-sample power-of-two fp16 range scale) and
//                       demodulation coefficients, or (ToRGB) the per-sample modulated 1x1 weights
//   cm_split_conv_kernel  3x3 weights -> two fp16 planes, [plane][tap][Cin/32][Cout][32]
//
// Compiled twice like migan_kernels.hpp: by hipcc for gfx950 and by the host compiler against tests/emu/hip_emu.h.
// MIGAN_TEMPLATE_KERNELS_ONLY (as in migan_kernels.hpp): a unit that only instantiates kernel templates (comodgan_u8.hip) leaves out
// the kernels that are no templates, which belong to migan_hip.hip.
#pragma once

namespace migan {

constexpr int kCmMaxTaps = 9;
constexpr float kCmInBound = 512.0f;        // |conv input| <= 256 (lrelu_agc clamp) + 256 (skip added after the activation)
constexpr float kCmF16Top = 32768.0f;       // scaled A operands stay below 2^15 (fp16 max 65504)

struct CmConvArgs {
  const float* x;               // NHWC [B][H][W][CI]
  float* y;                     // NHWC [B][HO][WO][CO]
  const float* skip;            // NHWC like y, added after the activation, or null
  const unsigned short* wsplit; // fp16 planes [2][9][CI/32][CO][32] behind a 16-byte header (cm_split_conv_kernel)
  const float* sa;              // [B][CI] per-sample input scale (normalised style x 2^e) or null -> a_scale
  const float* coef;            // [B][CO] per-sample output coefficient or null -> cgain
  const float* bias;            // [CO]
  const float* noise;           // [HO][WO] (+ noise_bstride floats per image) or null
  const float* noise_strength;  // scalar
  long long noise_bstride;
  float a_scale, cgain;
  int B, H, W, CI, CO, HO, WO;
  int stride;                   // input pixels per output-grid pixel (1, or 2 for the strided convolution)
  int ntaps;
  int dy[kCmMaxTaps], dx[kCmMaxTaps], wtap[kCmMaxTaps];   // input offset of each tap (relative to grid*stride), weight tap plane
  int dymin, dxmin, IH, IW;     // input tile origin offset and extent for an 8x16 grid tile
  int oy_mul, oy_add, ox_mul, ox_add;   // output pixel of grid pixel (gy, gx)
  int GHn, GWn;                 // grid extent; grid pixels beyond are not stored
  int tiles_x, tiles_y, nchunks;
  int raw;                      // 1: store acc * coef only (transposed-convolution phases; cm_fir_kernel<1> finishes the layer)
  int off_b;                    // LDS carve in bytes: start of the B tile buffers (the result tile aliases everything)
  unsigned long long* prof;     // phase-cycle accumulators (MIGAN_PHASE_PROF builds only), else null
};

// LDS layout of the A (input tile) and B (weight tile) operands: one row per pixel / output channel holding both fp16
// planes of the KC channels back to back plus 16 bytes of padding: pitch = 2 * KC * 2 + 16 bytes (144 for KC = 32, 80 for
// KC = 16).  16 consecutive rows of one 16-byte slot then fall into 16 different bank quads (pitch / 4 mod 64 = 36 resp. 20
// generates all multiples of 4), and -- unlike an XOR swizzle -- the address of a shifted row is the address of the row plus
// a constant, so one filter tap costs two VALU adds of address arithmetic and every other offset is an immediate.
// (Every VALU instruction in the tap loop costs matrix-core time on gfx950: MFMA and VALU issue cycles add up.)
template <int V>
struct IntT { static constexpr int value = V; };

// GEMM row r (0..127 of the workgroup tile; MFMA row = r % 32 of its 32-row tile) -> grid pixel gy * 16 + gx of the
// 8 x 16 tile.  ds_read_b128 is served in lane groups {0-3,12-15,20-27} and {4-11,16-19,28-31} (and the same + 32): with
// the identity map and the 18-pixel tile rows of the plain 3x3 mode, lanes 12,13 and 26,27 of a group read pixels 16
// rows apart = the same banks.  Swapping which pixels of the second tile row the lanes 16-31 take (16-19 -> columns
// 0,1,10,11; 20-27 -> 2..9; 28-31 -> 12..15) gives every group 16 pixels that are distinct modulo 16.
MIGAN_DEVICE MIGAN_INLINE int cm_pixel_of_row(int r) {
  const int k = r & 15;
  int col = k;
  if (r & 16) col = k < 2 ? k : (k < 4 ? k + 8 : (k < 12 ? k - 2 : k));
  return (r & ~15) | col;
}

//   NT  : output channels per workgroup (64 / 128 / 256)
//   KC  : input channels per K chunk (32; 16 for the strided mode, whose 17x33-pixel input tile would otherwise
//         leave room for one workgroup per CU only)
//   NIA : float4 input-tile items per thread per chunk = ceil(tile pixels * KC/4 / 256) (prefetch registers)
//   NINE: the tap list has exactly nine entries and CI / KC is even (plain and strided 3x3): K loop unrolled over two
//         chunks, two weight tiles in flight
//   MTI : 32-row MFMA tiles per wave along M: the workgroup owns MT = 64 * MTI grid pixels ((4 * MTI) x 16).  MTI = 4 (16 x 16
//         pixels): every weight tile fetched from L2 feeds twice the MFMAs -- the weight-tile stream (MT-independent bytes per
//         workgroup and tap) is what saturates the per-CU vector-memory path with 128-pixel tiles
//   Register budget: accumulators MTI * NT/64 * 16; more than 64 of them -> one workgroup per CU, one wave per SIMD (512 registers)
//   UP4 : all four output phases of the stride-2 transposed convolution in one launch (synthesis conv0): the nine taps of the 3x3
//         kernel, each feeding the accumulator set of its phase (tap (ky, kx) -> output parity (ky == 1, kx == 1), input shift
//         (-(ky == 2), -(kx == 2))).  The low-resolution input tile is staged once per chunk for all phases instead of once per
//         phase launch, and the K loop has nine taps per chunk (the unrolled NINE path) instead of 1 / 2 / 2 / 4.
//   F16 : single-plane form (cm_conv_f16_kernel, the blocks a caller has declared half precision: comodgan_set_fp16_blocks).  Both
//         operands are the high fp16 plane only -- the A tile rounded once to fp16 after the same style and range scaling, the B tile
//         plane 0 of cm_split_conv_kernel's output -- so a product is ONE MFMA (fp32 accumulate), an LDS row holds one plane
//         (pitch 2 * KC + 16 bytes: 80 for KC = 32, 48 for KC = 16, both conflict-free by the argument above) and a weight tile
//         is half the bytes from L2.  Tiles, tap lists, prefetch registers (the input tile is loaded as fp32 either way) and
//         accumulators are those of the two-plane form, and so are the launch bounds, which the accumulators decide.
// The kernel's text is comodgan_conv_body.inc, compiled into two kernel templates: F16 is a constant of the enclosing kernel.
template <int NT, int KC, int NIA, bool NINE, int MTI, bool UP4 = false>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, ((MTI * NT * (UP4 ? 4 : 1) > 512) ? 1 : 2)) cm_conv_kernel(const CmConvArgs p) {
  constexpr bool F16 = false, XH = false, YH = false;
#include "comodgan_conv_body.inc"
}
// The single-plane form: symbols of their own, so that the two-plane launches keep their names and their code.
template <int NT, int KC, int NIA, bool NINE, int MTI, bool UP4 = false>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, ((MTI * NT * (UP4 ? 4 : 1) > 512) ? 1 : 2)) cm_conv_f16_kernel(const CmConvArgs p) {
  constexpr bool F16 = true, XH = false, YH = false;
#include "comodgan_conv_body.inc"
}
// The single-plane form on fp16 activation storage (comodgan_set_fp16_storage): p.x holds _Float16, and so do p.y and p.skip
// when YH (the strided conv1 of the last half-precision encoder block hands fp32 to an fp32 block: YH = false).  Symbols of
// their own again.  Why no stored value overflows: include/comodgan_fp16_storage_hip.h.
template <int NT, int KC, int NIA, bool NINE, int MTI, bool UP4, bool YH>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, ((MTI * NT * (UP4 ? 4 : 1) > 512) ? 1 : 2)) cm_conv_h_kernel(const CmConvArgs p) {
  constexpr bool F16 = true, XH = true;
#include "comodgan_conv_body.inc"
}

// ------------------------------------------------------------------------------------------------
// Per-tensor statistics of one 3x3 weight tensor, one workgroup per output channel:
//   amax[co]     = max |w[co]|                       (fp16 range scale of the split GEMM operands)
//   wsq[co][ci]  = sum_k w^2, wn2[co] = 1 / mean_{ci,k} w^2    (demodulation, stylegan.py:138,147; modulated layers only)
struct CmWprepArgs {
  const float* w;      // [CO][CI][3][3]
  float* amax;         // [CO]
  float* wsq;          // [CO][CI] or null
  float* wn2;          // [CO] or null
  int CO, CI;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_wprep_kernel(const CmWprepArgs p) {
  MIGAN_DYN_SMEM(red);
  const int co = (int)blockIdx.x;
  float tot = 0.0f, mx = 0.0f;
  for (int ci = threadIdx.x; ci < p.CI; ci += 256) {
    const float* s = p.w + ((size_t)co * p.CI + ci) * 9;
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      a += s[k] * s[k];
      mx = fmaxf(mx, fabsf(s[k]));
    }
    if (p.wsq) p.wsq[(size_t)co * p.CI + ci] = a;
    tot += a;
  }
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) {
    tot += __shfl_xor(tot, sft);
    mx = fmaxf(mx, __shfl_xor(mx, sft));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = tot;
    red[4 + (threadIdx.x >> 6)] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (p.wn2) p.wn2[co] = (float)(p.CI * 9) / (red[0] + red[1] + red[2] + red[3]);
    p.amax[co] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  }
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// 3x3 weights [CO][CI][3][3] fp32 -> two fp16 planes [plane][tap][CI/32][CO][32] of w * wscale, wscale = the power of
// two that maps max|w| into [2^13, 2^14) (every workgroup derives it from amax[]; workgroup 0 also writes it to the
// 16-byte header in front of plane 0, float [2], where cm_conv_kernel reads it).
struct CmSplitArgs {
  const float* src;
  const float* amax;          // [CO]
  unsigned short* dst;        // plane 0; a 16-byte header precedes it
  int CO, CI;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_split_conv_kernel(const CmSplitArgs p) {
  MIGAN_DYN_SMEM(red);
  float m = 0.0f;
  for (int i = threadIdx.x; i < p.CO; i += 256) m = fmaxf(m, p.amax[i]);
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) m = fmaxf(m, __shfl_xor(m, sft));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127;       // floor(log2(max|w|))
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  const float sw = __builtin_bit_cast(float, (unsigned)(127 + 13 - e) << 23);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float* hdr = reinterpret_cast<float*>(p.dst) - 4;
    hdr[0] = 1.0f / sw; hdr[1] = m; hdr[2] = sw; hdr[3] = 0.0f;
  }
  const size_t plane = (size_t)9 * p.CI * p.CO;
  const size_t n = (size_t)p.CO * p.CI;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int co = (int)(i / p.CI), ci = (int)(i % p.CI);
    const float* s = p.src + i * 9;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
      const float v = s[tp] * sw;
      const unsigned pk = MIGAN_PACK_F16(v, 0.0f);
      const float r = v - MIGAN_F16LO_F32(pk);
      const unsigned pk2 = MIGAN_PACK_F16(r, 0.0f);
      const size_t o = ((size_t)(tp * (p.CI / 32) + (ci >> 5)) * p.CO + co) * 32 + (ci & 31);
      p.dst[o] = (unsigned short)(pk & 0xffffu);
      p.dst[plane + o] = (unsigned short)(pk2 & 0xffffu);
    }
  }
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// ------------------------------------------------------------------------------------------------
// styles [B][CI] (output of the affine dense layer) ->
//   demod = 1 (synthesis_layer): s~ = styles * rsqrt(mean over batch and channels of styles^2)   (stylegan.py:139)
//             sa[b][ci]   = s~ * 2^e_b, e_b the largest power of two keeping |x * sa| < 2^15 for |x| <= kCmInBound
//             coef[b][co] = wn[co] * rsqrt(wn2[co] * sum_ci s~^2 wsq[co][ci] + 1e-8) / 2^e_b           (stylegan.py:138-147,161)
//   demod = 0 (torgb_layer): wm[b][3][ci] = w[c][ci] * styles[b][ci] * wgain                             (stylegan.py:337-338)
// One workgroup per sample.
struct CmStyleArgs {
  const float* styles;  // [B][CI]
  const float* wsq;     // [CO][CI]   (demod)
  const float* wn2;     // [CO]       (demod)
  const float* w;       // [3][CI]    (torgb)
  float* sa;            // [B][CI]    (demod)
  float* coef;          // [B][CO]    (demod)
  float* wm;            // [B][3][CI] (torgb)
  float wgain;
  int B, CI, CO, demod;
};
constexpr int kCmStyleSlice = 16;       // output channels per workgroup (demod); grid = B * ceil(CO / 16)
MIGAN_DEVICE MIGAN_INLINE void cm_style_block(const CmStyleArgs& p, int block) {
  MIGAN_DYN_SMEM(sm);            // [CI] s~^2 of this sample, then 8 floats of reduction scratch
  const int tid = threadIdx.x;
  if (!p.demod) {
    const int b = block;
    const float* st = p.styles + (size_t)b * p.CI;
    for (int i = tid; i < 3 * p.CI; i += 256) {
      const int ci = i % p.CI;
      p.wm[(size_t)b * 3 * p.CI + i] = p.w[i] * (st[ci] * p.wgain);
    }
    return;
  }
  const int nsl = (p.CO + kCmStyleSlice - 1) / kCmStyleSlice;
  const int b = block / nsl, sl = block % nsl;
  const float* st = p.styles + (size_t)b * p.CI;
  float* red = sm + p.CI;
  float ss = 0.0f;
  for (int i = tid; i < p.B * p.CI; i += 256) ss += p.styles[i] * p.styles[i];
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) ss += __shfl_xor(ss, sft);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float g = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)(p.B * p.CI));
  float mx = 0.0f;
  for (int ci = tid; ci < p.CI; ci += 256) {
    const float s = st[ci] * g;
    sm[ci] = s * s;
    mx = fmaxf(mx, fabsf(s));
  }
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sft));
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  // 2^e <= kCmF16Top / (kCmInBound * mx): e = 6 - ceil(log2 mx); exponent arithmetic on the float bits
  int ex = (int)((__builtin_bit_cast(unsigned, mx) >> 23) & 0xffu) - 127;          // floor(log2 mx)
  ex = ex < -60 ? -60 : (ex > 60 ? 60 : ex);
  const int e = 6 - (ex + 1);                                                      // mx < 2^(ex+1)
  const float up = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
  const float dn = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
  if (sl == 0)
    for (int ci = tid; ci < p.CI; ci += 256) p.sa[(size_t)b * p.CI + ci] = st[ci] * g * up;
  // one wave per output channel of the slice: sum_ci s~^2 wsq[co][ci]
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = wave; k < kCmStyleSlice; k += 4) {
    const int co = sl * kCmStyleSlice + k;
    if (co >= p.CO) break;
    const float* wq = p.wsq + (size_t)co * p.CI;
    float a = 0.0f;
    for (int ci = lane; ci < p.CI; ci += 64) a += sm[ci] * wq[ci];
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) a += __shfl_xor(a, sft);
    if (lane == 0) {
      const float n2 = p.wn2[co];
      p.coef[(size_t)b * p.CO + co] = sqrtf(n2) * (1.0f / sqrtf(n2 * a + 1e-8f)) * dn;
    }
  }
}

// Every style computation of the synthesis network in one launch: they depend only on the affine outputs (one launch, above)
// and on the weight statistics, not on activations, so the 23 small launches that used to sit between the convolutions
// (0.4 ms of a 19 ms forward at comodgan-512) become one.
constexpr int kCmMaxStyle = 32;
struct CmStyleMultiArgs {
  CmStyleArgs job[kCmMaxStyle];
  int blk0[kCmMaxStyle + 1];     // first workgroup of each job
  int njobs;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_style_multi_kernel(const CmStyleMultiArgs p) {
  int j = 0;
  while (j + 1 < p.njobs && (int)blockIdx.x >= p.blk0[j + 1]) ++j;
  cm_style_block(p.job[j], (int)blockIdx.x - p.blk0[j]);
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// ------------------------------------------------------------------------------------------------
// dense (stylegan.py:64-99): y[n][o] = act((sum_k x[n][k] W[o][k]) * wgain + b[o] * bgain)
// Optional: per-row input normalisation x * rsqrt(mean(x^2) + 1e-8) (normalize_2nd_moment, stylegan.py:351-352),
// NHWC<->NCHW index permutations of the 4x4 bottleneck (in_c / out_c = channel count, 0 = none), `add` (same layout
// as the output, after the activation: comodgan.py:243), truncation lerp towards w_avg (stylegan.py:432-437),
// row-concatenated input (x2 supplies columns >= K1: torch.cat([w, w0]) of comodgan.py:247).
// One wave per 2 output features, 8 batch rows per pass.
struct CmDenseArgs {
  const float* x;      // [N][K1]
  const float* x2;     // [N][K-K1] or null
  const float* w;      // [O][K]
  const float* b;      // [O]
  const float* add;    // or null
  const float* lerp0;  // w_avg [O] or null
  float* y;            // [N][O]
  float* y_raw;        // with lerp0: also the value before the truncation lerp (the ws rows beyond truncation_cutoff), or null
  float wgain, bgain, psi;
  int N, K, K1, O;
  int act, norm, in_c, out_c;
};
// SAMP (the affine launch of an S-samples forward): x is per sample, x2 per image -- row n of x2 is n / S.
// ROWS (the affine launch of the staged walk): x is one row of a caller's ws [N][num_ws][w_dim] per batch row, xs floats apart.
template <bool SAMP = false, bool ROWS = false>
MIGAN_DEVICE MIGAN_INLINE void cm_dense_block(const CmDenseArgs& p, int block, int S = 1, int xs = 0) {
  constexpr int RP = 8;                      // batch rows per pass over the weights (16 spills)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int o0 = (block * 4 + wave) * 2;
  if (o0 >= p.O) return;
  const int no = (o0 + 1 < p.O) ? 2 : 1;
  const int K2 = p.K - p.K1;
  const float* wr0 = p.w + (size_t)o0 * p.K;
  const float* wr1 = p.w + (size_t)(o0 + (no > 1 ? 1 : 0)) * p.K;
  for (int n0 = 0; n0 < p.N; n0 += RP) {
    float acc[2][RP], nrm[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) { acc[0][r] = 0.0f; acc[1][r] = 0.0f; nrm[r] = 0.0f; }
    if (p.in_c) {
      // The input is the NHWC 4x4 bottleneck [N][16][C] and feature k of the reference's NCHW flatten is c * 16 + pos: a lane
      // owns channel c, reads its 16 weights per output row as four float4 (64 contiguous bytes per lane) and the 16 inputs
      // x[n][pos][c] with consecutive lanes on consecutive channels -- every access coalesced (walking k in weight order
      // would gather the inputs at a 2 KB stride)
      for (int c = lane; c < p.in_c; c += 64) {
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {          // (kept rolled: unrolling all 16 positions x 16 rows spills)
          const f4 a = ld4(wr0 + (size_t)c * 16 + q * 4), bq = ld4(wr1 + (size_t)c * 16 + q * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int pos = q * 4 + e;
#pragma unroll
            for (int r = 0; r < RP; ++r) {
              const int n = n0 + r;
              const float xv = n < p.N ? p.x[(size_t)n * p.K1 + (size_t)pos * p.in_c + c] : 0.0f;
              acc[0][r] += xv * a[e];
              acc[1][r] += xv * bq[e];
              nrm[r] += xv * xv;
            }
          }
        }
      }
    } else {
      for (int k = lane; k < p.K; k += 64) {
        const float w0 = wr0[k];
        const float w1 = no > 1 ? wr1[k] : 0.0f;
#pragma unroll
        for (int r = 0; r < RP; ++r) {
          const int n = n0 + r;
          float xv = 0.0f;
          if (n < p.N) xv = (k < p.K1) ? p.x[(size_t)n * (ROWS ? xs : p.K1) + k] : p.x2[(size_t)(SAMP ? n / S : n) * K2 + (k - p.K1)];
          acc[0][r] += xv * w0;
          acc[1][r] += xv * w1;
          nrm[r] += xv * xv;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RP; ++r) {
#pragma unroll
      for (int sft = 32; sft >= 1; sft >>= 1) {
        acc[0][r] += __shfl_xor(acc[0][r], sft);
        acc[1][r] += __shfl_xor(acc[1][r], sft);
        if (p.norm) nrm[r] += __shfl_xor(nrm[r], sft);
      }
    }
    if (lane < 2 * RP) {
      const int r = lane & (RP - 1), j = lane / RP;
      const int n = n0 + r, o = o0 + j;
      if (n < p.N && j < no) {
        // select without dynamic register indexing
        float a = 0.0f, q = 0.0f;
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
          if (rr == r) { a = j ? acc[1][rr] : acc[0][rr]; q = nrm[rr]; }
        if (p.norm) a = a * (1.0f / sqrtf(q / (float)p.K + 1e-8f));
        float v = a * p.wgain + p.b[o] * p.bgain;
        if (p.act) v = act1(v);
        const int oi = p.out_c ? (o & 15) * p.out_c + (o >> 4) : o;
        if (p.add) v += p.add[(size_t)n * p.O + oi];
        if (p.lerp0) {
          if (p.y_raw) p.y_raw[(size_t)n * p.O + oi] = v;
          const float s = p.lerp0[o];
          v = (p.psi < 0.5f) ? s + p.psi * (v - s) : v - (v - s) * (1.0f - p.psi);     // torch.lerp
        }
        p.y[(size_t)n * p.O + oi] = v;
      }
    }
  }
}

#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_dense_kernel(const CmDenseArgs p) { cm_dense_block(p, (int)blockIdx.x); }
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// All affine layers of the synthesis network in one launch (they depend only on the latent w and the global code w0,
// stylegan.py:282): a table of (weight, bias, output, out_features); same input cat([w, w0]), no activation.
constexpr int kCmMaxAffine = 48;
struct CmDenseMultiArgs {
  const float* w[kCmMaxAffine];
  const float* b[kCmMaxAffine];
  float* y[kCmMaxAffine];
  int O[kCmMaxAffine];
  int blk0[kCmMaxAffine + 1];     // first workgroup of each job
  const float* x;
  const float* x2;
  const float* x_alt;             // truncation_cutoff: the un-truncated w, read by the jobs whose bit is set in alt_mask (stylegan.py:436-437)
  unsigned long long alt_mask;
  float wgain;
  int N, K, K1, njobs;
};
// The job of this workgroup as a dense layer `a`; returns the workgroup's index within the job.  P: const CmDenseMultiArgs or a
// reference to one -- the table by value where it is the kernel's own argument, by reference where it is a member of it, which is
// how each kernel read it before the two shared this function and keeps the code of both as it was.
template <class P>
MIGAN_DEVICE MIGAN_INLINE int cm_affine_job(P p, CmDenseArgs& a, int* job = nullptr) {
  int j = 0;
  while (j + 1 < p.njobs && (int)blockIdx.x >= p.blk0[j + 1]) ++j;
  if (job) *job = j;
  a.x = ((p.alt_mask >> j) & 1ull) ? p.x_alt : p.x; a.x2 = p.x2; a.w = p.w[j]; a.b = p.b[j]; a.y = p.y[j];
  a.wgain = p.wgain; a.bgain = 1.0f; a.psi = 1.0f; a.N = p.N; a.K = p.K; a.K1 = p.K1; a.O = p.O[j];
  return (int)blockIdx.x - p.blk0[j];
}
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_dense_multi_kernel(const CmDenseMultiArgs p) {
  CmDenseArgs a{};
  const int block = cm_affine_job<const CmDenseMultiArgs>(p, a);
  cm_dense_block(a, block);
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY
// The same launch of an S-samples forward (comodgan_forward_samples): N = images x S rows of x / x_alt (the latents, one per
// sample, image-major) against the global code x2 of N / S images.  A symbol of its own, so that the launch above keeps its
// arguments and its code.
struct CmDenseMultiSamplesArgs {
  CmDenseMultiArgs m;
  int S;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_dense_multi_samples_kernel(const CmDenseMultiSamplesArgs q) {
  CmDenseArgs a{};
  const int block = cm_affine_job<const CmDenseMultiArgs&>(q.m, a);
  cm_dense_block<true>(a, block, q.S);
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY
// The same launch of the staged walk (comodgan_synthesize, include/comodgan_stages_hip.h): the latents are the caller's
// ws [N][num_ws][w_dim], N = images x S rows; job j reads row widx[j] of each (comodgan.py:399-405), so the row stride of x is
// num_ws * w_dim and whatever truncation the caller wants is already in the rows: no x_alt, alt_mask = 0.  x2 = w0 of N / S images.
struct CmDenseMultiRowsArgs {
  CmDenseMultiArgs m;              // x: ws
  int widx[kCmMaxAffine];
  int S, num_ws;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_dense_multi_rows_kernel(const CmDenseMultiRowsArgs q) {
  CmDenseArgs a{};
  int j = 0;
  const int block = cm_affine_job<const CmDenseMultiArgs&>(q.m, a, &j);
  a.x += (size_t)q.widx[j] * q.m.K1;
  cm_dense_block<true, true>(a, block, q.S, q.num_ws * q.m.K1);
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// ws of the mapping stage (comodgan_mapping; stylegan.py:429-437): the mapping output w [B][D] repeated to [B][num_ws][D], rows
// below `cutoff` from w (truncated towards w_avg by the last dense launch), the others from w_raw (the value before the lerp).
struct CmWsRowsArgs {
  const float* w;      // [B][D]
  const float* w_raw;  // [B][D]; read only where cutoff < num_ws
  float* ws;           // [B][num_ws][D]
  int B, num_ws, D, cutoff;      // D a multiple of 4
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_ws_rows_kernel(const CmWsRowsArgs p) {
  const int dq = p.D >> 2;
  const size_t total = (size_t)p.B * p.num_ws * dq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int q = (int)(i % dq);
    const size_t br = i / dq;
    const int r = (int)(br % p.num_ws);
    const size_t b = br / p.num_ws;
    const float* src = r < p.cutoff ? p.w : p.w_raw;
    st4(p.ws + br * p.D + q * 4, ld4(src + b * p.D + q * 4));
  }
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// Head of synthesis.b4 of an S-samples forward: x4 = fc(w0) + feat[4] depends on the image only and is computed at batch N;
// this copies it to the [N * S][4][4][C] tensor cm_conv_kernel reads (image-major: rows i * S ... i * S + S - 1 = image i).
// 32 KB per sample at 512 channels.
struct CmBcastArgs {
  const float* x;      // [N][M]
  float* y;            // [N * S][M]
  int N, S, M;         // M: floats per image, a multiple of 4
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_bcast_kernel(const CmBcastArgs p) {
  const int mq = p.M >> 2;
  const size_t total = (size_t)p.N * p.S * mq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int q = (int)(i % mq);
    const int b = (int)(i / mq);
    st4(p.y + (size_t)b * p.M + q * 4, ld4(p.x + (size_t)(b / p.S) * p.M + q * 4));
  }
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

// ------------------------------------------------------------------------------------------------
// conv2d_layer(4 -> C, kernel 1, bias, activation) of the first encoder block (comodgan.py:46-48, stylegan.py:231-244):
// NCHW network input -> NHWC features.  One thread per pixel and channel quad.
struct CmFromRgbArgs {
  const float* x;      // [B][4][R][R]
  const float* w;      // [C][4]
  const float* b;      // [C]
  float* y;            // [B][R][R][C]
  float wgain;
  int B, R, C;
};
// cm_fromrgb_h_kernel writes _Float16 (encoder block b<R> is half precision and fp16 storage is on; p.y is reinterpreted): values
// are bounded by the +-256 clamp, rounded to nearest even, 8 bytes per channel quad.  One text, comodgan_fromrgb_body.inc, and a
// symbol per output type, so that the fp32 launch keeps its name.
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fromrgb_kernel(const CmFromRgbArgs p) {
  constexpr bool YH = false, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
#include "comodgan_fromrgb_body.inc"
}
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fromrgb_h_kernel(const CmFromRgbArgs p) {
  constexpr bool YH = true, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
#include "comodgan_fromrgb_body.inc"
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY
// The FromRGB of a uint8 forward (comodgan_forward_u8, include/comodgan_u8_hip.h): the network input cat([mask - 0.5, img * mask])
// (migan_pack_input, pack_pixel) is formed in registers from the photo [B][R][R][3] and the mask [B][R][R]; f.x is unused, no fp32
// input tensor exists.  Symbols of their own, so that the launches above keep their arguments and their code, and templates: they are
// instantiated by comodgan_u8.hip alone (cm_fromrgb_u8_form below).
struct CmFromRgbU8Args {
  CmFromRgbArgs f;             // x: null
  const unsigned char* img;    // [B][R][R][3]
  const unsigned char* mask;   // [B][R][R], 255 = known pixel
};
template <bool YH>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fromrgb_u8_kernel(const CmFromRgbU8Args q) {
  constexpr bool U8 = true;
  const CmFromRgbArgs& p = q.f;
  const unsigned char *const u8_img = q.img, *const u8_mask = q.mask;
#include "comodgan_fromrgb_body.inc"
}

// ------------------------------------------------------------------------------------------------
// upfirdn2d with the separable [1,3,3,1] filter (taps [1,3,3,1] * fs per axis), up = down = 1, zero padding `pad` on
// every side, NHWC: out[y][x] = sum_{a,b} f[a] f[b] in[y + a - pad][x + b - pad].  Each thread produces a 2 x 4 block of
// output pixels for one channel quad from a 5 x 7 input window (4.4 loads per output instead of 16), one input row at
// a time: horizontal taps into 4 row sums, which feed the two output rows.
//   EPI = 0: FIR in front of the strided convolution (conv2d_resample.py down path: pad = 2, gain 1, fs = 1/8),
//                      [B][H][W][C] -> [B][H+1][W+1][C]
//   EPI = 1: second half of an up=2 synthesis_layer: FIR (gain 4: fs = 1/4, pad 1) over the (2H+1)^2 output
//                      of the transposed convolution (conv2d_resample.py up path), then noise, bias, activation, skip
//                      (stylegan.py:300-309, comodgan.py:331-332); the demodulation coefficient is already applied
//                      (cm_conv_kernel raw mode)
struct CmFirArgs {
  const float* x;              // NHWC [B][H][W][C]
  float* y;                    // NHWC [B][HO][WO][C]
  const float* skip;           // EPI 1: NHWC like y or null
  const float* bias;           // EPI 1: [C]
  const float* noise;          // EPI 1: [HO][WO] (+ noise_bstride per image) or null
  const float* noise_strength;
  long long noise_bstride;
  float fs;
  int B, H, W, C, HO, WO, pad;
};
// How the FIR body addresses one of its activation tensors behind the float* argument.  at(t, el, c4): channel quad c4 of the
// pixel whose first element is el; at(a, el): el elements on; ld / ld_once (a tensor read exactly once) / st (streamed): four
// consecutive channels, `raw4` what a thread keeps until cvt.  Two spellings of the same addresses, the ones the kernels had while
// each had a text of its own: the all-fp32 kernels compute in float* with ld4 / ld4once / st4o; a typed kernel (TYPED: some tensor
// holds _Float16) addresses every tensor in bytes through Io<2> or, for its fp32 tensors, Io<0>.  The compiler schedules the two
// differently, and this is what keeps every symbol's code instruction for instruction (profiles/comodgan_stream_bodies.md).
template <class IO> struct CmBytes {
  typedef typename IO::raw4 raw4;
  static MIGAN_DEVICE MIGAN_INLINE const char* at(const float* t, size_t el, int c4) { return reinterpret_cast<const char*>(t) + (el + c4 * 4) * IO::ESZ; }
  static MIGAN_DEVICE MIGAN_INLINE const char* at(const char* a, size_t el) { return a + el * IO::ESZ; }
  static MIGAN_DEVICE MIGAN_INLINE char* at(float* t, size_t el) { return reinterpret_cast<char*>(t) + el * IO::ESZ; }
  static MIGAN_DEVICE MIGAN_INLINE raw4 ld(const char* a) { return IO::ld(a, 0u); }
  static MIGAN_DEVICE MIGAN_INLINE raw4 ld_once(const char* a) { return IO::ld_once(a, 0u); }
  static MIGAN_DEVICE MIGAN_INLINE f4 cvt(raw4 r) { return IO::cvt(r); }
  static MIGAN_DEVICE MIGAN_INLINE raw4 zero() { return IO::zero(); }
  static MIGAN_DEVICE MIGAN_INLINE void st(char* a, f4 v) { IO::st(a, 0u, v); }
};
template <bool TYPED, bool H> struct CmAct : CmBytes<Io<H ? 2 : 0>> {};
template <> struct CmAct<false, false> {
  typedef f4 raw4;
  static MIGAN_DEVICE MIGAN_INLINE const float* at(const float* t, size_t el, int c4) { return t + el + c4 * 4; }
  static MIGAN_DEVICE MIGAN_INLINE const float* at(const float* t, size_t el) { return t + el; }
  static MIGAN_DEVICE MIGAN_INLINE float* at(float* t, size_t el) { return t + el; }
  static MIGAN_DEVICE MIGAN_INLINE raw4 ld(const float* a) { return ld4(a); }
  static MIGAN_DEVICE MIGAN_INLINE raw4 ld_once(const float* a) { return ld4once(a); }
  static MIGAN_DEVICE MIGAN_INLINE f4 cvt(raw4 r) { return r; }
  static MIGAN_DEVICE MIGAN_INLINE raw4 zero() { return f4{0.f, 0.f, 0.f, 0.f}; }
  static MIGAN_DEVICE MIGAN_INLINE void st(float* a, f4 v) { st4o(a, v); }
};

// The kernels' text is comodgan_fir_body.inc; EPI, SAMP, S and the element types are constants of the enclosing kernel.
template <int EPI>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fir_kernel(const CmFirArgs p) {
  constexpr bool SAMP = false, XH = false, YH = false, SH = false;
  constexpr int S = 1;
#include "comodgan_fir_body.inc"
}
// cm_fir_kernel<1> of an S-samples forward (comodgan_forward_samples): B = N * S, skip: [N].  Symbols of their own (and so are
// the typed twins below), so that cm_fir_kernel<1> keeps its arguments and its code.
struct CmFirSamplesArgs {
  CmFirArgs f;                 // B = N * S; skip: [N]
  int S;
};
#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fir_samples_kernel(const CmFirSamplesArgs q) {
  constexpr int EPI = 1;
  constexpr bool SAMP = true, XH = false, YH = false, SH = false;
  const CmFirArgs& p = q.f;
  const int S = q.S;
#include "comodgan_fir_body.inc"
}
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY
// The typed twins (fp16 activation storage): XH / YH / SH say which of x, y and the skip tensor hold _Float16 (the pointers of
// CmFirArgs are reinterpreted).  The skip tensor is the encoder's and typed by the encoder block's marking, x (the raw
// transposed-convolution output) and y by the synthesis block's, so every combination but fp16 x with fp32 y occurs.  These reach
// the text through a function taking the arguments by reference, as they always have: included straight into the kernel it
// compiles to other (somewhat shorter, unmeasured) code, and the all-fp32 kernels through the function likewise.
template <int EPI, bool SAMP, bool XH, bool YH, bool SH>
MIGAN_DEVICE MIGAN_INLINE void cm_fir_h_body(const CmFirArgs& p, int S) {
#include "comodgan_fir_body.inc"
}
template <int EPI, bool XH, bool YH, bool SH>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fir_h_kernel(const CmFirArgs p) {
  static_assert(XH || YH || SH, "the all-fp32 form is cm_fir_kernel");
  cm_fir_h_body<EPI, false, XH, YH, SH>(p, 1);
}
template <bool XH, bool YH, bool SH>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_fir_samples_h_kernel(const CmFirSamplesArgs q) {
  static_assert(XH || YH || SH, "the all-fp32 form is cm_fir_samples_kernel");
  cm_fir_h_body<1, true, XH, YH, SH>(q.f, q.S);
}

// ------------------------------------------------------------------------------------------------
// torgb_layer (stylegan.py:330-344) with per-sample modulated weights wm [B][3][C] (cm_style_multi_kernel) + bias +
// upsample2d of the running image (comodgan.py:334-343).  16 lanes per pixel, wave-shuffle butterfly.
struct CmRgbArgs {
  const float* x;        // NHWC [B][H][W][C]
  const float* wm;       // [B][3][C]
  const float* bias;     // [3]
  const float* img_prev; // planar [B][3][H/2][W/2] or null
  float* img_out;        // planar [B][3][H][W]
  int B, H, W, C;
};
// LPP lanes per pixel (4 for 64 channels ... 16 for >= 256): each lane reads C / (4 LPP) float4 of the pixel, a butterfly over
// the LPP lanes forms the three sums, lane ch of the group finishes channel ch (bias, upsampled previous image) -- a wave
// writes 64 / LPP consecutive pixels of each plane.
// cm_torgb_h_kernel reads an fp16 feature map (the ToRGB of a half-precision block with fp16 storage on; p.x is reinterpreted):
// 8 bytes per lane and step; the weights, the sums, the running image and the output stay fp32.  One text,
// comodgan_torgb_body.inc, and a symbol family per feature-map type, so that the fp32 launches keep their names.
template <int LPP>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_torgb_kernel(const CmRgbArgs p) {
  constexpr bool XH = false, PARTS = false, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
  unsigned char* const u8_out = nullptr;
  constexpr int u8_S = 1;
  float* const rgb_out = nullptr;
#include "comodgan_torgb_body.inc"
}
template <int LPP>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_torgb_h_kernel(const CmRgbArgs p) {
  constexpr bool XH = true, PARTS = false, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
  unsigned char* const u8_out = nullptr;
  constexpr int u8_S = 1;
  float* const rgb_out = nullptr;
#include "comodgan_torgb_body.inc"
}
// The ToRGB of the staged walk with return_intermediate_outs (comodgan.py:334-343 returns to_rgb_out beside img): the same pass
// also stores the un-added torgb(x) to rgb_out, planar like img_out.  Symbols of their own, so that the launches above keep their
// arguments and their code.
struct CmRgbPartsArgs {
  CmRgbArgs r;
  float* rgb_out;        // planar [B][3][H][W]
};
template <int LPP>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_torgb_parts_kernel(const CmRgbPartsArgs q) {
  constexpr bool XH = false, PARTS = true, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
  unsigned char* const u8_out = nullptr;
  constexpr int u8_S = 1;
  const CmRgbArgs& p = q.r;
  float* const rgb_out = q.rgb_out;
#include "comodgan_torgb_body.inc"
}
template <int LPP>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_torgb_parts_h_kernel(const CmRgbPartsArgs q) {
  constexpr bool XH = true, PARTS = true, U8 = false;
  const unsigned char *const u8_img = nullptr, *const u8_mask = nullptr;
  unsigned char* const u8_out = nullptr;
  constexpr int u8_S = 1;
  const CmRgbArgs& p = q.r;
  float* const rgb_out = q.rgb_out;
#include "comodgan_torgb_body.inc"
}

// The last ToRGB (res == R) of a uint8 forward (comodgan_forward_u8, include/comodgan_u8_hip.h): the same reduction and upsampled
// running image, then migan_compose_output's arithmetic (compose_pixel) instead of the fp32 store -- row b of the B = N * S rows is
// composed over photo b / S and written as HWC bytes; r.img_out is unused, no fp32 output tensor exists.  S is an argument: one
// family serves S = 1 and S > 1.  Symbols of their own again; XH: the feature map holds _Float16.
struct CmRgbU8Args {
  CmRgbArgs r;                 // img_out: null
  const unsigned char* img;    // [B / S][H][W][3]
  const unsigned char* mask;   // [B / S][H][W], 255 = known pixel
  unsigned char* out;          // [B][H][W][3]
  int S;
};
template <int LPP, bool XH>
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) cm_torgb_u8_kernel(const CmRgbU8Args q) {
  constexpr bool PARTS = false, U8 = true;
  const CmRgbArgs& p = q.r;
  float* const rgb_out = nullptr;
  const unsigned char *const u8_img = q.img, *const u8_mask = q.mask;
  unsigned char* const u8_out = q.out;
  const int u8_S = q.S;
#include "comodgan_torgb_body.inc"
}

// The uint8 kernels by form, for the host walk.  Their instantiations live in a translation unit of their own, comodgan_u8.hip:
// compiled into the unit that holds pack_input_kernel, a second user of unit_image() changes that kernel's code (the optimiser's
// result for one function depends on what else the module holds), and every symbol the library had keeps its code.  The unit that
// holds the host walk declares them (MIGAN_CM_U8_ELSEWHERE); the CPU test harness, a single unit, defines them here.
struct CmFromRgbU8Form { void (*fn)(const CmFromRgbU8Args); const char* name; };
struct CmRgbU8Form { void (*fn)(const CmRgbU8Args); const char* name; };
CmFromRgbU8Form cm_fromrgb_u8_form(bool yh);
CmRgbU8Form cm_torgb_u8_form(int lpp, bool xh);       // lpp: 4, 8 or 16
#ifndef MIGAN_CM_U8_ELSEWHERE
CmFromRgbU8Form cm_fromrgb_u8_form(bool yh) {
  if (yh) return {cm_fromrgb_u8_kernel<true>, "migan::cm_fromrgb_u8_kernel<true>"};
  return {cm_fromrgb_u8_kernel<false>, "migan::cm_fromrgb_u8_kernel<false>"};
}
CmRgbU8Form cm_torgb_u8_form(int lpp, bool xh) {
#define CM_TORGB_U8_FORM(LPP, XH) {cm_torgb_u8_kernel<LPP, XH>, "migan::cm_torgb_u8_kernel<" #LPP ", " #XH ">"}
  static const CmRgbU8Form forms[2][3] = {{CM_TORGB_U8_FORM(4, false), CM_TORGB_U8_FORM(8, false), CM_TORGB_U8_FORM(16, false)},
                                          {CM_TORGB_U8_FORM(4, true), CM_TORGB_U8_FORM(8, true), CM_TORGB_U8_FORM(16, true)}};
#undef CM_TORGB_U8_FORM
  return forms[xh][lpp / 8];
}
#endif  // MIGAN_CM_U8_ELSEWHERE

}  // namespace migan
