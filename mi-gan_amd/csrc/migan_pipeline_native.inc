// Crops at native size (include/migan_pipeline_native_hip.h), included by migan_pipeline.hpp inside namespace migan behind
// migan_pipeline_region_patches.inc: the steps either side of the fully convolutional forward (migan_forward_hw), for a table of
// rows whose network window [height][width] has one size.  A row's box is the part of its window that lies inside the photo, at the
// window's top-left corner; the rest of the window is unknown pixels.
//
//   pipe_pre_native_kernel    pipe_pre_rows_kernel without the two resamplings: window pixel (py, px) is box pixel (py, px)
//   pipe_post_native_kernel   pipe_post_rows_kernel with the generator output taken at the same pixel instead of through four taps
//
// Both take PipeRowItem rows by value in the kernel argument, like PipeRowsArgs, with (height, width) in place of R.
struct PipeNativeArgs {
  PipeRowItem item[kPipeRowsMax];
  int first[kPipeRowsMax + 1];
  float* x;                          // pre: network input [n][4][height][width]
  const float* y;                    // post: network output [n][3][height][width]
  int n, height, width;
  int quads;                         // pre: a thread owns four consecutive columns (the host: width % 4 == 0 and x 16-byte aligned)
  float gauss[25];
};
static_assert(sizeof(PipeNativeArgs) <= 2304, "the native rows argument must stay well under the 4 KB kernel-argument limit");

// pipe_pre_pixel's arithmetic for image pixel `at` (its bilinear weights are exactly 1 and 0 at scale 1, the rounded byte is the
// byte): o = {m - 0.5, (c * 2 / 255 - 1) * m ...}
MIGAN_DEVICE MIGAN_INLINE void pipe_native_pixel(const unsigned char* image, const unsigned char* mask, size_t plane, size_t at, float o[4]) {
  const float m = (float)mask[at] / 255.0f;
  o[0] = m - 0.5f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = (float)image[c * plane + at];
    v = MIGAN_FSUB_RN(MIGAN_FMUL_RN(v, 2.0f) / 255.0f, 1.0f);                         // image.float() * 2 / 255 - 1
    o[c + 1] = MIGAN_FMUL_RN(v, m);
  }
}

// A pure streaming kernel: 4 bytes read and 16 written per window pixel, the padding included (no memset in front: every element of
// x is written here, once).  quads: unit u of a row is four consecutive columns of one window row, each plane stored as one 16-byte
// vector (the window rows and planes are multiples of 16 bytes); a wave then writes 1 KiB contiguous per plane.  The box starts at
// any column of the photo, so its bytes are read one by one (consecutive lanes, consecutive words: the same cache lines).  Otherwise
// unit u is one pixel.  cdiv(units, kThreads) tiles per row.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_pre_native_kernel(const PipeNativeArgs p) {
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out as in the other row kernels)
  const PipeRowItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;                   // (the host checked it: never taken)
  const int x_min = it.box[0], y_min = it.box[2], cw = it.box[1] - it.box[0], ch = it.box[3] - it.box[2];
  const size_t plane = (size_t)it.H * it.W, wplane = (size_t)p.height * p.width;
  float* x = p.x + (size_t)k * 4 * wplane;
  const int u = ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x;
  if (p.quads) {                                                     // (uniform over the launch)
    const int qw = p.width >> 2;
    if (u >= p.height * qw) return;
    const int py = u / qw, px = u % qw * 4;
    f4 v[4];
    v[0] = f4{-0.5f, -0.5f, -0.5f, -0.5f};
    v[1] = v[2] = v[3] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (py < ch && px < cw) {                                        // the quad meets the box
      const size_t at = (size_t)(y_min + py) * it.W + x_min + px;
      if (px + 4 <= cw) {                                            // ... and lies inside it: no branch between its 16 loads
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float o[4];
          pipe_native_pixel(it.image, it.mask, plane, at + j, o);
          v[0][j] = o[0]; v[1][j] = o[1]; v[2][j] = o[2]; v[3][j] = o[3];
        }
      } else {                                                       // ... and straddles its right border
        for (int j = 0; px + j < cw; ++j) {
          float o[4];
          pipe_native_pixel(it.image, it.mask, plane, at + j, o);
          v[0][j] = o[0]; v[1][j] = o[1]; v[2][j] = o[2]; v[3][j] = o[3];
        }
      }
    }
    float* dst = x + (size_t)py * p.width + px;
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f4*>(dst + c * wplane) = v[c];
    return;
  }
  if (u >= p.height * p.width) return;
  const int py = u / p.width, px = u % p.width;
  float o[4] = {-0.5f, 0.0f, 0.0f, 0.0f};
  if (py < ch && px < cw) pipe_native_pixel(it.image, it.mask, plane, (size_t)(y_min + py) * it.W + x_min + px, o);
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c * wplane + u] = o[c];
}

// pipe_post_byte for a generator output taken at the pixel itself: its first lines without the four taps and bilinear_mix (whose
// weights would be 1 and 0), its last three as they are
MIGAN_DEVICE MIGAN_INLINE unsigned char pipe_native_byte(float y, float mk, unsigned char image_byte) {
  float o = MIGAN_FMUL_RN(MIGAN_FADD_RN(MIGAN_FMUL_RN(y, 0.5f), 0.5f), 255.0f);       // ((y * 0.5 + 0.5) * 255)
  o = fminf(fmaxf(o, 0.0f), 255.0f);
  const float img = (float)image_byte;
  float v = MIGAN_FADD_RN(MIGAN_FMUL_RN(img, mk), MIGAN_FMUL_RN(o, MIGAN_FSUB_RN(1.0f, mk)));
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (unsigned char)(int)v;
}

// pipe_post_rows_kernel's tile scheme (tiles of the BOX, one pixel per thread, the grid has exactly the box's tiles), label test and
// early exit, the two LDS steps of migan_pipeline_pool_body.inc and the blur in its order; then three loads of y at window pixel
// (py, px) = box pixel (py, px).  Nothing of y outside [0, ch) x [0, cw) is read.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_native_kernel(const PipeNativeArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  int* any = reinterpret_cast<int*>(win + kPostLdsBytes);            // the tile holds a pixel of the row's label
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out as in the other row kernels)
  const PipeRowItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;                   // (the host checked it: never taken)
  const int x_min = it.box[0], y_min = it.box[2], cw = it.box[1] - it.box[0], ch = it.box[3] - it.box[2];
  if (cw > p.width || ch > p.height) return;                         // (the host checked it: y is never read outside the window)
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int ty0 = tile / ntx * kPostTH, tx0 = tile % ntx * kPostTW;
  if (ty0 >= ch) return;                                             // (workgroup-uniform, like the returns above)
  const int t = (int)threadIdx.x;
  const int py = ty0 + t / kPostTW, px = tx0 + t % kPostTW;
  bool mine = py < ch && px < cw;
  if (it.label != 0) {                                               // (workgroup-uniform)
    if (t == 0) *any = 0;
    __syncthreads();
    mine = mine && it.labels[(size_t)(y_min + py) * it.W + x_min + px] == it.label;
    if (mine) *any = 1;                                              // (every writer stores the same value)
    __syncthreads();
    if (*any == 0) return;
  }
#include "migan_pipeline_pool_body.inc"                              // steps 1 and 2
  if (!mine) return;
  double acc = 0.0;
  for (int ky = 0; ky < 5; ++ky) {
    const int yy = pipe_reflect(py + ky - 2, ch) - (ty0 - 2);
    for (int kx = 0; kx < 5; ++kx) {
      const int xx = pipe_reflect(px + kx - 2, cw) - (tx0 - 2);
      acc += (double)p.gauss[ky * 5 + kx] * (double)pool[yy * kPostPW + xx];
    }
  }
  const float mk = (float)acc / 255.0f;
  const size_t plane = (size_t)it.H * it.W, wplane = (size_t)p.height * p.width;
  const size_t at = (size_t)(y_min + py) * it.W + x_min + px;
  const float* y = p.y + (size_t)k * 3 * wplane + (size_t)py * p.width + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) it.image[c * plane + at] = pipe_native_byte(y[c * wplane], mk, it.image[c * plane + at]);
}
