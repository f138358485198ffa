// The reference's DEPLOYED pre/post-processing around the generator forward (second half):
// scripts/create_onnx_pipeline.py::MIGAN_Pipeline (:118-264) -- masked bounding box, crop, bilinear resize to the network
// resolution, generator, bilinear resize back, 3x3 max-pool + 5x5 gaussian feathering of the mask, blend -- as gfx950 kernels.
// All of it is memory-bound elementwise / small-stencil work on one image: one thread per output pixel, coalesced rows.
//
// torch's arithmetic is followed operation by operation where it decides a rounding the test can see:
//   F.interpolate(mode="bilinear", align_corners=False): scale = float(in) / out, src = scale * (dst + 0.5) - 0.5 clamped at 0,
//     i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1, value = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11)
//   F.interpolate(mode="nearest"): src = min(floor(dst * scale), in - 1)
//   torchvision's tensor resize rounds a uint8 image back with torch.round (half to even) -> rintf
// Compiled for the product and (tests/emu) for the CPU emulator.
//
// Two forms: one image per call with the box on the host (PipeArgs; migan_pipeline_bbox / _pre / _post), and a batch of up to
// kPipeBatchMax images of different sizes per launch with the box kept on the device (PipeBatchArgs; migan_pipeline_batch_pre /
// _post): 1-D grids, workgroup -> (item, tile) through the prefix table in the argument, no host synchronisation in between.
// The batch form's post step also exists out of place, for S generator outputs per image: as whole images (PipeSamplesArgs;
// migan_pipeline_batch_post_samples) and as box-sized patches (PipePatchesArgs; migan_pipeline_batch_post_patches).
// A fourth form gives every hole region of an image a box of its own (migan_pipeline_regions.inc; migan_pipeline_regions_*), in
// place, or out of place as S box-sized patches per region with a paste step back (migan_pipeline_region_patches.inc).
// A fifth form runs rows at the photo's own scale, around the fully convolutional forward (migan_pipeline_native.inc).
#pragma once

#ifndef MIGAN_HOST_DEVICE          // (the CPU emulator build is host code throughout)
#define MIGAN_HOST_DEVICE
#endif

namespace migan {

struct PipeArgs {
  unsigned char* image;        // [3][H][W] uint8 (CHW, the reference pipeline's layout); post: read and written in place
  const unsigned char* mask;   // [H][W] uint8, 255 = known pixel
  float* x;                    // pre: network input [4][R][R]
  const float* y;              // post: network output [3][R][R]
  unsigned char* pooled;       // post: 3x3 max-pool of the cropped mask [ch][cw] (scratch)
  int* flags;                  // bbox: [W] column flags then [H] row flags (scratch)
  int H, W, R;
  int x_min, x_max, y_min, y_max;
  float gauss[25];             // GaussianSmoothing(kernel_size=5, sigma=1) weights, row major (:63-85)
};

// get_masked_bbox (:149-229) from the first / last masked column and row (x_min = W, x_max = 0, y_min = H, y_max = 0 when nothing is
// masked: min over [..., w], max over [..., 0]): a dozen integer min/max in the reference's own order.  The ONE statement of it: the
// host calls it in migan_pipeline_bbox, thread 0 of pipe_bbox_batch_kernel on the device.  box = {x_min, x_max, y_min, y_max}
MIGAN_HOST_DEVICE inline void pipe_box(int x_min, int x_max, int y_min, int y_max, int width, int height, int resolution, int padding,
                                       int box[4]) {
  auto lo = [](int a, int b) { return a < b ? a : b; };
  auto hi = [](int a, int b) { return a > b ? a : b; };
  x_min = lo(x_min, x_max); x_max = hi(x_min, x_max);                              // :154-172
  y_min = lo(y_min, y_max); y_max = hi(y_min, y_max);
  const int cnt_x = (x_min + x_max) / 2, cnt_y = (y_min + y_max) / 2;              // :174-175
  int crop = hi(x_max - x_min, y_max - y_min) + 2 * padding;                       // :177-180
  crop = hi(crop, resolution);                                                     // :181-184
  const int off = crop / 2;                                                        // :186
  x_min = hi(cnt_x - off, 0); x_max = lo(cnt_x + off, width);                      // :187-202
  y_min = hi(cnt_y - off, 0); y_max = lo(cnt_y + off, height);
  const int xe = hi(crop - (x_max - x_min), 0), ye = hi(crop - (y_max - y_min), 0);   // :204-211
  x_min = hi(x_min - xe, 0); x_max = lo(x_max + xe, width);                        // :213-229
  y_min = hi(y_min - ye, 0); y_max = lo(y_max + ye, height);
  box[0] = x_min; box[1] = x_max; box[2] = y_min; box[3] = y_max;
}

MIGAN_DEVICE MIGAN_INLINE void bilinear_coord(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.0f) src = 0.0f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l1 = fminf(fmaxf(l1, 0.0f), 1.0f);
  l0 = 1.0f - l1;
}
MIGAN_DEVICE MIGAN_INLINE float bilinear_mix(float p00, float p01, float p10, float p11, float l0x, float l1x, float l0y, float l1y) {
  const float h0 = MIGAN_FADD_RN(MIGAN_FMUL_RN(l0x, p00), MIGAN_FMUL_RN(l1x, p01));
  const float h1 = MIGAN_FADD_RN(MIGAN_FMUL_RN(l0x, p10), MIGAN_FMUL_RN(l1x, p11));
  return MIGAN_FADD_RN(MIGAN_FMUL_RN(l0y, h0), MIGAN_FMUL_RN(l1y, h1));
}

#ifndef MIGAN_TEMPLATE_KERNELS_ONLY
// get_masked_bbox (:132-147): which columns / rows contain a pixel that is not 255 (mean < 255 <=> any pixel < 255 for uint8 data)
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_flags_clear_kernel(const PipeArgs p) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i < p.H + p.W) p.flags[i] = 0;
}
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_flags_kernel(const PipeArgs p) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i >= p.H * p.W) return;
  if (p.mask[i] != 255) {
    p.flags[i % p.W] = 1;                 // (every writer stores the same value)
    p.flags[p.W + i / p.W] = 1;
  }
}

// MIGAN_Pipeline.forward's first line (:256): tvF.resize(mask, image size, NEAREST) = F.interpolate(mode="nearest").
// pixel i of dst [H][W] from src [ih][iw]
MIGAN_DEVICE MIGAN_INLINE void pipe_mask_resize_pixel(const unsigned char* src, int ih, int iw, unsigned char* dst, int H, int W, int i) {
  if (i >= H * W) return;
  const int oy = i / W, ox = i % W;
  int sy = (int)floorf((float)oy * ((float)ih / (float)H)), sx = (int)floorf((float)ox * ((float)iw / (float)W));
  sy = sy < ih - 1 ? sy : ih - 1;
  sx = sx < iw - 1 ? sx : iw - 1;
  dst[i] = src[(size_t)sy * iw + sx];
}

// preprocess (:233-239) of the crop [y_min, y_max) x [x_min, x_max): bilinear resize of the uint8 image (rounded back to uint8 as
// torchvision does), nearest resize of the mask, x = cat([mask / 255 - 0.5, (image * 2 / 255 - 1) * mask / 255]).  Element i of each
// plane of x [4][R][R]
MIGAN_DEVICE MIGAN_INLINE void pipe_pre_pixel(const unsigned char* image, const unsigned char* mask, float* x, int H, int W, int R,
                                              int x_min, int x_max, int y_min, int y_max, int i) {
  if (i >= R * R) return;
  const int oy = i / R, ox = i % R;
  const int ch = y_max - y_min, cw = x_max - x_min;
  const float sy = (float)ch / (float)R, sx = (float)cw / (float)R;
  int y0, y1, x0, x1;
  float l0y, l1y, l0x, l1x;
  bilinear_coord(oy, sy, ch, y0, y1, l0y, l1y);
  bilinear_coord(ox, sx, cw, x0, x1, l0x, l1x);
  int ny = (int)floorf((float)oy * sy), nx = (int)floorf((float)ox * sx);
  ny = ny < ch - 1 ? ny : ch - 1;
  nx = nx < cw - 1 ? nx : cw - 1;
  const float m = (float)mask[(size_t)(y_min + ny) * W + x_min + nx] / 255.0f;
  const size_t plane = (size_t)H * W, oplane = (size_t)R * R;
  x[i] = m - 0.5f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned char* q = image + c * plane;
    const float p00 = (float)q[(size_t)(y_min + y0) * W + x_min + x0], p01 = (float)q[(size_t)(y_min + y0) * W + x_min + x1];
    const float p10 = (float)q[(size_t)(y_min + y1) * W + x_min + x0], p11 = (float)q[(size_t)(y_min + y1) * W + x_min + x1];
    float v = rintf(bilinear_mix(p00, p01, p10, p11, l0x, l1x, l0y, l1y));          // torch.round, then .to(uint8)
    v = (float)(unsigned char)(int)v;
    v = MIGAN_FSUB_RN(MIGAN_FMUL_RN(v, 2.0f) / 255.0f, 1.0f);                        // image.float() * 2 / 255 - 1
    x[(c + 1) * oplane + i] = MIGAN_FMUL_RN(v, m);
  }
}

// F.pad(mode='reflect') (:114) of coordinate v into [0, n)
MIGAN_DEVICE MIGAN_INLINE int pipe_reflect(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

// postprocess (:241-250) + the paste back (:263) of crop pixel (py, px), given acc = the 5x5 gaussian of the max-pooled mask there
// (the 25 products summed in fp64, see pipe_post_kernel): generator output -> [0, 255], bilinear resize to the crop,
// composed = image * mask + output * (1 - mask), clamp, truncate to uint8.  In three parts, so that a kernel that writes several
// generator outputs for one pixel (pipe_post_samples_kernel) states the same arithmetic: what depends on the pixel alone
// (pipe_post_coord), the four taps of one channel of a generator output (pipe_post_taps), the result byte (pipe_post_byte).
struct PipePostCoord {
  float mk;                          // the feathered mask in [0, 1]
  int y0, y1, x0, x1;                // bilinear taps in the generator output
  float l0y, l1y, l0x, l1x;
};
MIGAN_DEVICE MIGAN_INLINE PipePostCoord pipe_post_coord(int R, int cw, int ch, int py, int px, double acc) {
  PipePostCoord k;
  k.mk = (float)acc / 255.0f;
  // generator output resized to the crop
  const float sy = (float)R / (float)ch, sx = (float)R / (float)cw;
  bilinear_coord(py, sy, R, k.y0, k.y1, k.l0y, k.l1y);
  bilinear_coord(px, sx, R, k.x0, k.x1, k.l0x, k.l1x);
  return k;
}
// the four taps of channel plane q [R][R] of a generator output, in bilinear_mix's order
MIGAN_DEVICE MIGAN_INLINE void pipe_post_taps(const float* q, int R, const PipePostCoord& k, float t[4]) {
  t[0] = q[k.y0 * R + k.x0]; t[1] = q[k.y0 * R + k.x1]; t[2] = q[k.y1 * R + k.x0]; t[3] = q[k.y1 * R + k.x1];
}
// taps of one channel + the image's byte there -> the result byte
MIGAN_DEVICE MIGAN_INLINE unsigned char pipe_post_byte(const float t[4], const PipePostCoord& k, unsigned char image_byte) {
  auto to255 = [](float v) {
    float t = MIGAN_FMUL_RN(MIGAN_FADD_RN(MIGAN_FMUL_RN(v, 0.5f), 0.5f), 255.0f);    // ((y * 0.5 + 0.5) * 255)
    return fminf(fmaxf(t, 0.0f), 255.0f);
  };
  const float o = bilinear_mix(to255(t[0]), to255(t[1]), to255(t[2]), to255(t[3]), k.l0x, k.l1x, k.l0y, k.l1y);
  const float img = (float)image_byte;
  float v = MIGAN_FADD_RN(MIGAN_FMUL_RN(img, k.mk), MIGAN_FMUL_RN(o, MIGAN_FSUB_RN(1.0f, k.mk)));
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (unsigned char)(int)v;
}
MIGAN_DEVICE MIGAN_INLINE void pipe_post_pixel(unsigned char* image, const float* y, int H, int W, int R, int x_min, int y_min, int cw,
                                               int ch, int py, int px, double acc) {
  const PipePostCoord k = pipe_post_coord(R, cw, ch, py, px, acc);
  const size_t plane = (size_t)H * W, oplane = (size_t)R * R;
  const size_t at = (size_t)(y_min + py) * W + x_min + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float t[4];
    pipe_post_taps(y + c * oplane, R, k, t);
    image[c * plane + at] = pipe_post_byte(t, k, image[c * plane + at]);
  }
}

// args: mask = source [y_max][x_max] (its height / width ride in y_max / x_max), pooled = destination [H][W]
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_mask_resize_kernel(const PipeArgs p) {
  pipe_mask_resize_pixel(p.mask, p.y_max, p.x_max, p.pooled, p.H, p.W, (int)(blockIdx.x * kThreads + threadIdx.x));
}

MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_pre_kernel(const PipeArgs p) {
  pipe_pre_pixel(p.image, p.mask, p.x, p.H, p.W, p.R, p.x_min, p.x_max, p.y_min, p.y_max, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// F.max_pool2d(mask, 3, stride=1, padding=1) of the cropped mask (:246): neighbours outside the crop do not count
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_maxpool_kernel(const PipeArgs p) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int ch = p.y_max - p.y_min, cw = p.x_max - p.x_min;
  if (i >= ch * cw) return;
  const int py = i / cw, px = i % cw;
  int m = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = py + dy, xx = px + dx;
      if (yy < 0 || yy >= ch || xx < 0 || xx >= cw) continue;
      const int v = p.mask[(size_t)(p.y_min + yy) * p.W + p.x_min + xx];
      m = v > m ? v : m;
    }
  p.pooled[i] = (unsigned char)m;
}

// postprocess (:241-250) + the paste back (:263): feathered mask (gaussian 5x5 on the max-pooled mask, reflect padding), then
// pipe_post_pixel
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_kernel(const PipeArgs p) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int ch = p.y_max - p.y_min, cw = p.x_max - p.x_min;
  if (i >= ch * cw) return;
  const int py = i / cw, px = i % cw;
  // feathered mask.  The 25 products are summed in fp64 and rounded once: the fp32 weights sum to 1 - 3.7e-9, so a flat 255
  // neighbourhood blurs to exactly 255.0f and a known pixel far from the hole is returned unchanged (as ATen's conv2d does on the
  // reference's host); a plain fp32 running sum gives 254.99998 there and the truncation below would darken every known pixel by 1.
  double acc = 0.0;
  for (int ky = 0; ky < 5; ++ky) {
    const int yy = pipe_reflect(py + ky - 2, ch);
    for (int kx = 0; kx < 5; ++kx) {
      const int xx = pipe_reflect(px + kx - 2, cw);
      acc += (double)p.gauss[ky * 5 + kx] * (double)p.pooled[yy * cw + xx];
    }
  }
  pipe_post_pixel(p.image, p.y, p.H, p.W, p.R, p.x_min, p.y_min, cw, ch, py, px, acc);
}

// ---- the batch form: up to kPipeBatchMax images of different sizes per launch, box on the device ---------------------------------------
// The item table travels BY VALUE in the kernel argument (48 bytes per item: about 1.8 KB of the 4 KB a launch may carry), so a
// batch costs no table upload and no allocation.  Grids are 1-D: workgroup b works on item i with first[i] <= b < first[i + 1], as
// tile b - first[i] of it; the host fills `first` per launch (each kernel has its own tile size).  No atomics, no host round trip.
// Every later table of this file and of its .inc files (samples, patches, regions, rows, row patches, paste) has this form, and so
// have the metrics' and the photo resize's.  The host half is stated once for all of them (migan_host.hpp: table_split, which items
// go into which launch, and table_launch, which fills item[], first[] and n); the device half of the tables here is pipe_table_item.
constexpr int kPipeBatchMax = 32;
struct PipeBatchItem {
  unsigned char* image;              // [3][H][W] uint8, post: read and written in place
  const unsigned char* mask_src;     // the caller's mask [mh][mw]
  unsigned char* mask_resized;       // its nearest resize to [H][W] in scratch, or null when (mh, mw) == (H, W)
  int* flags;                        // [W] column flags then [H] row flags (scratch)
  int H, W, mh, mw;
};
struct PipeBatchArgs {
  PipeBatchItem item[kPipeBatchMax];
  int first[kPipeBatchMax + 1];
  float* x;                          // pre: network input [n][4][R][R]
  const float* y;                    // post: network output [n][3][R][R]
  int* bbox;                         // [n][4] = {x_min, x_max, y_min, y_max} per item: written by pipe_bbox_batch_kernel, read by pre / post
  int n, R, padding;
  float gauss[25];
};
static_assert(sizeof(PipeBatchArgs) <= 2048, "the batch argument must stay well under the 4 KB kernel-argument limit");

// the item of workgroup b, for any argument with item[], first[] and n.  Wave-uniform: a handful of scalar compares on the
// argument; an item without a workgroup in this launch is stepped over
template <class Args>
MIGAN_DEVICE MIGAN_INLINE int pipe_table_item(const Args& p, int b) {
  int i = 0;
  while (i + 1 < p.n && b >= p.first[i + 1]) ++i;
  return i;
}
MIGAN_DEVICE MIGAN_INLINE const unsigned char* pipe_batch_mask(const PipeBatchItem& it) {
  return it.mask_resized ? it.mask_resized : it.mask_src;
}

// tiles of kThreads pixels of the items whose mask has another size than their image (the others have no tile)
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_mask_resize_batch_kernel(const PipeBatchArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeBatchItem& it = p.item[k];
  pipe_mask_resize_pixel(it.mask_src, it.mh, it.mw, it.mask_resized, it.H, it.W, ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x);
}

// tiles of kThreads of the H + W flags of each item
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_flags_clear_batch_kernel(const PipeBatchArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeBatchItem& it = p.item[k];
  const int i = ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x;
  if (i < it.H + it.W) it.flags[i] = 0;
}
// tiles of kThreads pixels of each item's mask
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_flags_batch_kernel(const PipeBatchArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeBatchItem& it = p.item[k];
  const int i = ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x;
  if (i >= it.H * it.W) return;
  if (pipe_batch_mask(it)[i] != 255) {
    it.flags[i % it.W] = 1;                // (every writer stores the same value)
    it.flags[it.W + i / it.W] = 1;
  }
}

// get_masked_bbox (:149-229), one workgroup per item: first / last flagged column and row per thread, min / max tree through LDS
// (4 * kThreads ints of dynamic LDS), then thread 0 runs pipe_box and writes the item's row of bbox
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_bbox_batch_kernel(const PipeBatchArgs p) {
  MIGAN_DYN_SMEM(smem);
  int* red = reinterpret_cast<int*>(smem);                     // [x_min | x_max | y_min | y_max][kThreads]
  const PipeBatchItem& it = p.item[blockIdx.x];
  const int t = (int)threadIdx.x;
  int x_min = it.W, x_max = 0, y_min = it.H, y_max = 0;        // :149-152 (min over [..., w], max over [..., 0])
  for (int x = t; x < it.W; x += kThreads)
    if (it.flags[x]) { x_min = x < x_min ? x : x_min; x_max = x > x_max ? x : x_max; }
  for (int y = t; y < it.H; y += kThreads)
    if (it.flags[it.W + y]) { y_min = y < y_min ? y : y_min; y_max = y > y_max ? y : y_max; }
  red[t] = x_min; red[kThreads + t] = x_max; red[2 * kThreads + t] = y_min; red[3 * kThreads + t] = y_max;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      int *a = red + t, *b = red + t + s;
      a[0] = b[0] < a[0] ? b[0] : a[0];
      a[kThreads] = b[kThreads] > a[kThreads] ? b[kThreads] : a[kThreads];
      a[2 * kThreads] = b[2 * kThreads] < a[2 * kThreads] ? b[2 * kThreads] : a[2 * kThreads];
      a[3 * kThreads] = b[3 * kThreads] > a[3 * kThreads] ? b[3 * kThreads] : a[3 * kThreads];
    }
    __syncthreads();
  }
  if (t == 0) {
    int box[4];
    pipe_box(red[0], red[kThreads], red[2 * kThreads], red[3 * kThreads], it.W, it.H, p.R, p.padding, box);
    int* out = p.bbox + 4 * blockIdx.x;
    out[0] = box[0]; out[1] = box[1]; out[2] = box[2]; out[3] = box[3];
  }
}

// a box that pipe_pre_pixel / the post kernel may index with: inside the image and at least 3x3 (reflect padding of the 5x5 blur)
MIGAN_DEVICE MIGAN_INLINE bool pipe_box_valid(const int* box, int H, int W) {
  return box[0] >= 0 && box[1] <= W && box[2] >= 0 && box[3] <= H && box[1] - box[0] >= 3 && box[3] - box[2] >= 3;
}

// cdiv(R * R, kThreads) tiles per item (first[i] = i * that), box read from device memory
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_pre_batch_kernel(const PipeBatchArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeBatchItem& it = p.item[k];
  const int* box = p.bbox + 4 * k;
  if (!pipe_box_valid(box, it.H, it.W)) return;
  pipe_pre_pixel(it.image, pipe_batch_mask(it), p.x + (size_t)k * 4 * p.R * p.R, it.H, it.W, p.R, box[0], box[1], box[2], box[3],
                 ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x);
}

// pipe_maxpool_kernel + pipe_post_kernel in one pass, the pooled mask in LDS instead of scratch.  A workgroup owns a
// kPostTW x kPostTH tile of crop pixels, one per thread (a wave = two rows of 32: coalesced rows in global memory; in LDS each half
// wave reads 32 consecutive bytes = 8 dwords of one row, rows 9 dwords apart -> no bank conflict):
//   1. mask window of the tile + 3 pixels of halo -> LDS, 0 outside the crop (max-pool neighbours outside the crop do not count)
//   2. 3x3 max of it = the pooled mask of the tile + 2 pixels of halo -> LDS.  Entries outside the crop are never read: the blur
//      reflects at the crop border, and a reflected coordinate lies within 2 of the coordinate it came from's tile
//   3. 5x5 blur from LDS (same fp64 sum, same ky, kx order as pipe_post_kernel), then pipe_post_pixel
// The crop is not known on the host: the grid has cdiv(W, TW) * cdiv(H, TH) workgroups per item, at least as many as the crop
// has tiles; tile t is (t / ntx, t % ntx) of the CROP's ntx = cdiv(cw, TW) columns, and the surplus workgroups leave at once.
constexpr int kPostTW = 32, kPostTH = 8;
constexpr int kPostWW = kPostTW + 6, kPostWH = kPostTH + 6, kPostPW = kPostTW + 4, kPostPH = kPostTH + 4;
constexpr int kPostWinBytes = (kPostWW * kPostWH + 15) / 16 * 16;
constexpr int kPostLdsBytes = kPostWinBytes + (kPostPW * kPostPH + 15) / 16 * 16;
static_assert(kPostTW * kPostTH == kThreads, "one thread per tile pixel");
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_batch_kernel(const PipeBatchArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeBatchItem& it = p.item[k];
  const int* box = p.bbox + 4 * k;
  // the box came through device memory: one that does not fit the image is not touched (and nothing of the image is)
  if (!pipe_box_valid(box, it.H, it.W)) return;
  const int x_min = box[0], y_min = box[2], cw = box[1] - box[0], ch = box[3] - box[2];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int ty0 = tile / ntx * kPostTH, tx0 = tile % ntx * kPostTW;
  if (ty0 >= ch) return;                                             // (workgroup-uniform, like the returns above)
  const unsigned char* mask = pipe_batch_mask(it);
  const int t = (int)threadIdx.x;
  for (int e = t; e < kPostWH * kPostWW; e += kThreads) {
    const int cy = ty0 - 3 + e / kPostWW, cx = tx0 - 3 + e % kPostWW;
    win[e] = (cy >= 0 && cy < ch && cx >= 0 && cx < cw) ? mask[(size_t)(y_min + cy) * it.W + x_min + cx] : (unsigned char)0;
  }
  __syncthreads();
  for (int e = t; e < kPostPH * kPostPW; e += kThreads) {
    const unsigned char* w0 = win + e / kPostPW * kPostWW + e % kPostPW;
    int m = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int v = w0[dy * kPostWW + dx];
        m = v > m ? v : m;
      }
    pool[e] = (unsigned char)m;
  }
  __syncthreads();
  const int py = ty0 + t / kPostTW, px = tx0 + t % kPostTW;
  if (py >= ch || px >= cw) return;
  double acc = 0.0;
  for (int ky = 0; ky < 5; ++ky) {
    const int yy = pipe_reflect(py + ky - 2, ch) - (ty0 - 2);
    for (int kx = 0; kx < 5; ++kx) {
      const int xx = pipe_reflect(px + kx - 2, cw) - (tx0 - 2);
      acc += (double)p.gauss[ky * 5 + kx] * (double)pool[yy * kPostPW + xx];
    }
  }
  pipe_post_pixel(it.image, p.y + (size_t)k * 3 * p.R * p.R, it.H, it.W, p.R, x_min, y_min, cw, ch, py, px, acc);
}

// ---- several completions per image, written out of place ---------------------------------------------------------------------------
// pipe_post_batch_kernel for S generator outputs per item (y rows k * S ... k * S + S - 1), into a destination [S][3][H][W] of its
// own: the image is only read.  Inside the box, sample s gets the byte pipe_post_batch_kernel would store for its y row; outside,
// and everywhere when the box does not fit the image, the image's byte.  Every destination byte is written once, by one thread.
//
// The tiles are those of the IMAGE (tile t = (t / ntx, t % ntx) of ntx = cdiv(W, TW) columns), one pixel per thread, so the same
// grid as pipe_post_batch_kernel's has no surplus workgroups: a tile that misses the box copies.  A tile that meets the box runs
// the same three LDS steps around its own origin, (ty0, tx0) in crop coordinates, which may now be negative: window and pooled
// entries outside the crop are filled as before and never read, since a reflected coordinate lies inside the crop and within 2 of
// the pixel it came from.  What depends on the pixel alone -- the 25 fp64 products, the bilinear coordinates and weights, the three
// image bytes -- is computed once, then the samples are looped over.
// The item table is its own (32 bytes per item: no flags, no mask size, the mask pointer already resolved).
constexpr int kPipeSamplesMax = 32;
struct PipeSamplesItem {
  const unsigned char* image;        // [3][H][W] uint8, read only
  const unsigned char* mask;         // [H][W]: the caller's mask, or its nearest resize in scratch
  unsigned char* out;                // [S][3][H][W] uint8
  int H, W;
};
struct PipeSamplesArgs {
  PipeSamplesItem item[kPipeSamplesMax];
  int first[kPipeSamplesMax + 1];
  const float* y;                    // [n * S][3][R][R], row k * S + s = sample s of item k
  const int* bbox;                   // [n][4], as PipeBatchArgs::bbox
  int n, R, S;
  float gauss[25];
};
static_assert(sizeof(PipeSamplesArgs) <= 2048, "the samples argument must stay well under the 4 KB kernel-argument limit");

MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_samples_kernel(const PipeSamplesArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipeSamplesItem& it = p.item[k];
  const int* box = p.bbox + 4 * k;
  // the box came through device memory: one that does not fit the image is an empty crop here, and every tile copies
  const bool valid = pipe_box_valid(box, it.H, it.W);
  const int x_min = valid ? box[0] : 0, y_min = valid ? box[2] : 0, cw = valid ? box[1] - box[0] : 0, ch = valid ? box[3] - box[2] : 0;
  const int tile = (int)blockIdx.x - p.first[k], ntx = (it.W + kPostTW - 1) / kPostTW;
  const int iy0 = tile / ntx * kPostTH, ix0 = tile % ntx * kPostTW;  // the tile's origin in the image ...
  const int ty0 = iy0 - y_min, tx0 = ix0 - x_min;                    // ... and in the crop
  // workgroup-uniform: the tile has a pixel inside the crop
  const bool blend = ty0 < ch && ty0 + kPostTH > 0 && tx0 < cw && tx0 + kPostTW > 0;
  const int t = (int)threadIdx.x;
  if (blend) {                                                       // steps 1 and 2: one text with pipe_post_patches_kernel
#include "migan_pipeline_pool_body.inc"
  }
  const int row = iy0 + t / kPostTW, col = ix0 + t % kPostTW;
  if (row >= it.H || col >= it.W) return;
  const size_t plane = (size_t)it.H * it.W, at = (size_t)row * it.W + col;
  const unsigned char img[3] = {it.image[at], it.image[plane + at], it.image[2 * plane + at]};
  const int py = row - y_min, px = col - x_min;
  if (!blend || py < 0 || py >= ch || px < 0 || px >= cw) {
    for (int s = 0; s < p.S; ++s) {
      unsigned char* o = it.out + (size_t)s * 3 * plane + at;
      o[0] = img[0]; o[plane] = img[1]; o[2 * plane] = img[2];
    }
    return;
  }
  // step 3, pipe_post_coord and the loop over the samples, into plane stride `plane` at offset `at`: one text with pipe_post_patches_kernel
#include "migan_pipeline_samples_body.inc"
}

// ---- several completions per image, as box-sized patches ---------------------------------------------------------------------------
// The same S results per crop pixel as pipe_post_samples_kernel, but only the crop is written: item k's destination is the tightly
// packed [S][3][ch][cw], byte (s, c, py, px) at out + ((s * 3 + c) * ch + py) * cw + px.  Nothing outside the box is read or
// written, so the tiles are again those of the CROP, as in pipe_post_batch_kernel: the grid is sized from the image, tile t is
// (t / ntx, t % ntx) of the crop's ntx = cdiv(cw, TW) columns, and the surplus workgroups leave at once.  The three LDS steps, the
// per-pixel values and the sample loop are pipe_post_samples_kernel's text (the two .inc bodies), around another destination.
// The size of the patches is device data (the box), the size of the destination host data: each item carries its destination's
// capacity, and an item whose S * 3 * ch * cw bytes exceed it is skipped whole, like one whose box does not fit its image -- a wrong
// size on the host leaves a destination unwritten, it does not become a store out of bounds.
constexpr int kPipePatchesMax = 32;
struct PipePatchesItem {
  const unsigned char* image;        // [3][H][W] uint8, read only, and only inside the box
  const unsigned char* mask;         // [H][W]: the caller's mask, or its nearest resize in scratch
  unsigned char* out;                // [S][3][ch][cw] uint8
  unsigned long long capacity;       // bytes `out` can take
  int H, W;
};
struct PipePatchesArgs {
  PipePatchesItem item[kPipePatchesMax];
  int first[kPipePatchesMax + 1];
  const float* y;                    // [n * S][3][R][R], row k * S + s = sample s of item k
  const int* bbox;                   // [n][4], as PipeBatchArgs::bbox
  int n, R, S;
  float gauss[25];
};
static_assert(sizeof(PipePatchesArgs) <= 2048, "the patches argument must stay well under the 4 KB kernel-argument limit");

MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_patches_kernel(const PipePatchesArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipePatchesItem& it = p.item[k];
  const int* box = p.bbox + 4 * k;
  // the box came through device memory: one that does not fit the image has no patch ...
  if (!pipe_box_valid(box, it.H, it.W)) return;
  const int x_min = box[0], y_min = box[2], cw = box[1] - box[0], ch = box[3] - box[2];
  // ... and one whose patches do not fit the destination is not started (ch * cw < 2^30 and S < 2^31: no overflow in 64 bits)
  const size_t plane = (size_t)ch * cw;                              // the destination's channel stride
  if ((unsigned long long)p.S * 3ull * plane > it.capacity) return;
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int ty0 = tile / ntx * kPostTH, tx0 = tile % ntx * kPostTW;
  if (ty0 >= ch) return;                                             // (workgroup-uniform, like the returns above)
  const int t = (int)threadIdx.x;
#include "migan_pipeline_pool_body.inc"                              // steps 1 and 2
  const int py = ty0 + t / kPostTW, px = tx0 + t % kPostTW;
  if (py >= ch || px >= cw) return;
  const size_t iplane = (size_t)it.H * it.W, iat = (size_t)(y_min + py) * it.W + x_min + px;
  const unsigned char img[3] = {it.image[iat], it.image[iplane + iat], it.image[2 * iplane + iat]};
  const size_t at = (size_t)py * cw + px;                            // the pixel in a plane of the destination
#include "migan_pipeline_samples_body.inc"                           // step 3, pipe_post_coord, the loop over the samples
}

// ---- one crop per hole region: labelling, a box per region, pre / post over a row table (include/migan_pipeline_regions_hip.h) -----
#include "migan_pipeline_regions.inc"
// ---- S completions per hole region as patches, and the paste back (include/migan_pipeline_region_patches_hip.h) ----------------------
#include "migan_pipeline_region_patches.inc"
// ---- crops at native size around the fully convolutional forward: no resampling (include/migan_pipeline_native_hip.h) ----------------
#include "migan_pipeline_native.inc"
#endif  // MIGAN_TEMPLATE_KERNELS_ONLY

}  // namespace migan
