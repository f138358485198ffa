// S completions per hole region, as patches, and the way back (include/migan_pipeline_region_patches_hip.h), included by
// migan_pipeline.hpp inside namespace migan behind migan_pipeline_regions.inc:
//
//   pipe_post_rows_patches_kernel   pipe_post_rows_kernel out of place, for S generator outputs per row: row k -> [S][3][ch][cw]
//   pipe_paste_rows_kernel          one sample's patch -> the image, where labels == label
//
// Both take a table of rows by value in the kernel argument, like PipeRowsArgs; the box is host data, so the grids have exactly the
// crop's tiles and the capacity of a destination was checked on the host.
constexpr int kPipeRowPatchesMax = 32;
struct PipeRowPatchesItem {
  const unsigned char* image;        // [3][H][W] uint8, read only, and only inside the box
  const unsigned char* mask;         // [H][W], the full mask at the image's size
  const unsigned char* labels;       // [H][W]; not read when label == 0
  unsigned char* out;                // [S][3][ch][cw] uint8
  int H, W, label;
  int box[4];
};
struct PipeRowPatchesArgs {
  PipeRowPatchesItem item[kPipeRowPatchesMax];
  int first[kPipeRowPatchesMax + 1];
  const float* y;                    // [n * S][3][R][R], row k * S + s = sample s of row k
  int n, R, S;
  float gauss[25];
};
static_assert(sizeof(PipeRowPatchesArgs) <= 2304, "the row patches argument must stay well under the 4 KB kernel-argument limit");

// The tile scheme of pipe_post_rows_kernel (tiles of the CROP, one pixel per thread), the two LDS steps of
// migan_pipeline_pool_body.inc and the per-pixel values and sample loop of migan_pipeline_samples_body.inc -- the shared texts, so
// that the blend contracts as in every other post kernel and the bytes are pipe_post_pixel's -- around the destination geometry of
// pipe_post_patches_kernel: plane = ch * cw, at = py * cw + px.
// Every byte of the destination is written, by one thread: a pixel of the row's label gets the S blended bytes per channel, any other
// pixel of the box the image's byte S times.  So, unlike pipe_post_rows_kernel, a tile without a pixel of its label does not leave:
// it skips the LDS steps (workgroup-uniform: one LDS flag, read behind a barrier) and copies.  Inside a tile that runs them, every
// thread -- outside the crop, or on a pixel of another label -- takes part in every barrier; no thread returns in front of one.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_rows_patches_kernel(const PipeRowPatchesArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  int* any = reinterpret_cast<int*>(win + kPostLdsBytes);            // the tile holds a pixel of the row's label
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipeRowPatchesItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;                   // (the host checked it: never taken)
  const int x_min = it.box[0], y_min = it.box[2], cw = it.box[1] - it.box[0], ch = it.box[3] - it.box[2];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int ty0 = tile / ntx * kPostTH, tx0 = tile % ntx * kPostTW;
  if (ty0 >= ch) return;                                             // (workgroup-uniform, like the return above; the last one)
  const int t = (int)threadIdx.x;
  const int py = ty0 + t / kPostTW, px = tx0 + t % kPostTW;
  const bool inside = py < ch && px < cw;
  bool mine = inside, blend = true;
  if (it.label != 0) {                                               // (workgroup-uniform)
    if (t == 0) *any = 0;
    __syncthreads();
    mine = inside && it.labels[(size_t)(y_min + py) * it.W + x_min + px] == it.label;
    if (mine) *any = 1;                                              // (every writer stores the same value)
    __syncthreads();
    blend = *any != 0;                                               // (workgroup-uniform: the same word, behind the barrier)
  }
  if (blend) {
#include "migan_pipeline_pool_body.inc"                              // steps 1 and 2
  }
  if (!inside) return;
  const size_t iplane = (size_t)it.H * it.W, iat = (size_t)(y_min + py) * it.W + x_min + px;
  const unsigned char img[3] = {it.image[iat], it.image[iplane + iat], it.image[2 * iplane + iat]};
  const size_t plane = (size_t)ch * cw;                              // the destination's channel stride
  const size_t at = (size_t)py * cw + px;                            // the pixel in a plane of the destination
  if (!mine) {
    for (int s = 0; s < p.S; ++s) {
      unsigned char* o = it.out + (size_t)s * 3 * plane + at;
      o[0] = img[0]; o[plane] = img[1]; o[2 * plane] = img[2];
    }
    return;
  }
#include "migan_pipeline_samples_body.inc"                           // step 3, pipe_post_coord, the loop over the samples
}

// ---- the way back: the chosen sample of a region -> the image -------------------------------------------------------------------------
constexpr int kPipePasteMax = 32;
struct PipePasteItem {
  unsigned char* image;              // [3][H][W] uint8, written inside the box where labels == label
  const unsigned char* labels;       // [H][W]; not read when label == 0
  const unsigned char* patch;        // [3][ch][cw] uint8: one sample
  int H, W, label;
  int box[4];
};
struct PipePasteArgs {
  PipePasteItem item[kPipePasteMax];
  int first[kPipePasteMax + 1];
  int n;
};
static_assert(sizeof(PipePasteArgs) <= 2048, "the paste argument must stay well under the 4 KB kernel-argument limit");

// tiles of the crop as above, one pixel per thread: the label test, then three byte copies.  No LDS, no barrier.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_paste_rows_kernel(const PipePasteArgs p) {
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipePasteItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;                   // (the host checked it: never taken)
  const int x_min = it.box[0], y_min = it.box[2], cw = it.box[1] - it.box[0], ch = it.box[3] - it.box[2];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int t = (int)threadIdx.x;
  const int py = tile / ntx * kPostTH + t / kPostTW, px = tile % ntx * kPostTW + t % kPostTW;
  if (py >= ch || px >= cw) return;
  const size_t iplane = (size_t)it.H * it.W, iat = (size_t)(y_min + py) * it.W + x_min + px;
  if (it.label != 0 && it.labels[iat] != it.label) return;
  const size_t plane = (size_t)ch * cw, at = (size_t)py * cw + px;
  it.image[iat] = it.patch[at];
  it.image[iplane + iat] = it.patch[plane + at];
  it.image[2 * iplane + iat] = it.patch[2 * plane + at];
}
