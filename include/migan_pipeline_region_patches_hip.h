/* migan_pipeline_region_patches_hip.h -- C ABI of libmigan_hip.so, deployed pipeline: S completions per hole region, as patches.
 *
 * migan_pipeline_regions_post (migan_pipeline_regions_hip.h) stores ONE completion of every region into the photo.  The calls below
 * are its out-of-place form for S generator outputs per row, and the inverse step that puts a chosen one back:
 *
 *   migan_pipeline_regions_find(...)                      label maps, counts, boxes   (migan_pipeline_regions_hip.h)
 *   ... the caller lists the rows: (image, mask, labels, label, box) ...
 *   migan_pipeline_regions_pre(rows, m, R, x)             network input of every row
 *   generator: x [m][4][R][R] -> y [m * S][3][R][R], row r * S + s = sample s of rows[r]
 *   migan_pipeline_regions_post_patches(rows, m, S, R, y, gauss25, outs, out_bytes)   outs[r] = [S][3][ch_r][cw_r]
 *   ... the user picks a sample per region ...
 *   migan_pipeline_regions_paste(paste_rows, m)           the chosen patch of every listed region -> the photo
 *
 * Definition of a patch byte, for row r with box {x_min, x_max, y_min, y_max}, ch = y_max - y_min, cw = x_max - x_min, label L:
 *   byte (s, c, py, px) of outs[r], at outs[r] + ((s * 3 + c) * ch + py) * cw + px, is
 *     where labels == L   the byte migan_pipeline_regions_post would store at (c, y_min + py, x_min + px) for this row with y row
 *                         r * S + s (the crop's post-processing with the FULL mask),
 *     everywhere else     the image's own byte at (c, y_min + py, x_min + px).
 *   With L = 0 (a single-box row) there is no label test: the whole box takes the blended byte, and the patch holds
 *   migan_pipeline_batch_post_patches' bytes for that box.
 * So every patch is an opaque, self-contained crop and every destination byte is written exactly once.  Nothing outside the box is
 * read; the image, the mask and the label map are never written.
 *
 * Boxes of neighbouring regions may overlap, which is why the way back is not a rectangle copy: _paste writes only the pixels of
 * the row's own label, so pasting region 1's patch leaves region 2 as it is.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).  Nothing here synchronises.
 */
#ifndef MIGAN_PIPELINE_REGION_PATCHES_HIP_H_
#define MIGAN_PIPELINE_REGION_PATCHES_HIP_H_

#include <stddef.h>

#include "migan_pipeline_regions_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows, m, resolution, gauss25: as migan_pipeline_regions_post (rows' image is only READ here).
 * y_nchw    [m * samples][3][R][R] fp32, row r * samples + s = sample s of rows[r]
 * outs      HOST array of m device pointers: outs[r] = uint8 [samples][3][ch_r][cw_r], tightly packed, (ch, cw) from rows[r].box
 * out_bytes HOST array: capacity of outs[r] in bytes
 * Any m >= 1; launches carry 32 rows each.  The box is host data here, so the capacity is checked on the host.  MIGAN_EINVAL with
 * nothing launched: samples < 1, a null outs, out_bytes or outs[r], out_bytes[r] < samples * 3 * ch_r * cw_r, and everything
 * migan_pipeline_regions_pre / _post reject (a null pointer, a resolution that is no power of two >= 8, an image below 3 x 3 or of
 * 2^30 pixels or more, a box that does not lie inside its image or is smaller than 3 x 3, a label outside 0 ... 64, a null
 * labels_u8 with a label above 0).  A destination that overlaps an image, a mask, a label map, y or another destination is
 * UNDEFINED. */
int migan_pipeline_regions_post_patches(const migan_pipeline_region_row* rows, int m, int samples, int resolution,
                                        const void* y_nchw, const float* gauss25, void* const* outs,
                                        const size_t* out_bytes, void* stream);

typedef struct migan_pipeline_region_paste_row {
  void* image_chw_u8;        /* [3][height][width], written inside box where labels == label (label 0: the whole box) */
  const void* labels_u8;     /* [height][width] from migan_pipeline_regions_find; may be null when label is 0 */
  const void* patch_chw_u8;  /* [3][ch][cw]: ONE sample's patch (the caller adds choice * 3 * ch * cw to the row's destination) */
  int height, width, label;
  int box[4];                /* {x_min, x_max, y_min, y_max}, the box the patch was made for */
} migan_pipeline_region_paste_row;

/* A pure copy: image (c, y_min + py, x_min + px) = patch (c, py, px) where labels == label, for every row.  Rows of one image may
 * come in any order and in separate calls: their pixel sets are disjoint.  "Leave this region alone" = do not list its row.  Any
 * m >= 1; launches carry 32 rows each.  MIGAN_EINVAL with nothing launched: a null rows, image or patch pointer, an image below
 * 3 x 3 or of 2^30 pixels or more, a box that does not lie inside its image or is smaller than 3 x 3, a label outside 0 ... 64, a
 * null labels_u8 with a label above 0.  Two rows with the same image and label, a label-0 row next to another row of its image,
 * or an image that overlaps a patch or a label map are UNDEFINED. */
int migan_pipeline_regions_paste(const migan_pipeline_region_paste_row* rows, int m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PIPELINE_REGION_PATCHES_HIP_H_ */
