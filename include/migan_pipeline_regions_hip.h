/* migan_pipeline_regions_hip.h -- C ABI of libmigan_hip.so, deployed pipeline: one crop per hole region.
 *
 * The batch pipeline (migan_hip.h: migan_pipeline_batch_pre / _post) puts ONE box around every hole pixel of a photo.  Two small
 * holes in opposite corners of a large photo then share one crop, squeezed to the network resolution R.  The calls below split the
 * mask into regions on the device (connected-component labelling), give every region a box of its own by the reference's box rule,
 * and let every region write only its own pixels:
 *
 *   migan_pipeline_regions_scratch_bytes(items, n, gap, max_regions) -> scratch
 *   migan_pipeline_regions_find(items, n, R, padding, gap, max_regions, labels, count_dev, boxes_dev, scratch)
 *   ... the caller copies count_dev and boxes_dev to the host and lists the rows: (image, box) pairs ...
 *   migan_pipeline_regions_pre(rows, m, R, x)          network input of every row
 *   generator: x [m][4][R][R] -> y [m][3][R][R]
 *   migan_pipeline_regions_post(rows, m, R, y, gauss25)
 *
 * Definition, for one image [3][H][W] and its mask, nearest-resized to [H][W] first when it has another size:
 *   hole pixel   mask != 255.
 *   D            every pixel within Chebyshev distance `gap` of a hole pixel ((2 gap + 1)^2 box maximum, clipped at the border).
 *   region       an 8-connected component of D.  Label 0 = not in D; regions are numbered 1 ... K in raster order of their smallest
 *                linear index y * W + x (the numbering scipy.ndimage.label(D, structure = ones((3, 3))) gives).  The hole pixels
 *                of region k are the hole pixels with label k; hole pixels of different regions are >= 2 gap + 2 apart.
 *   box k        get_masked_bbox (reference scripts/create_onnx_pipeline.py:149-229) of the column / row extents of region k's hole
 *                pixels, clipped to the image; box 0 is that of ALL hole pixels, i.e. row i of migan_pipeline_batch_pre's bbox_dev.
 *   row          (image, mask, labels, label, box).  _pre gives it the x that migan_pipeline_pre gives that box (the FULL mask:
 *                other regions' hole pixels inside the crop are holes to the network).  _post runs migan_pipeline_batch_post's
 *                arithmetic on the box with the full mask, but reads and writes the image only where labels == label.  With
 *                gap >= 2 the feathered mask at such a pixel depends on the mask within 3 pixels, every other region's hole pixel
 *                is >= gap + 2 away, so the bytes are those a mask holding region k alone would give; no pixel has two writers.
 *                label 0 = a single-box row: no label test, the bytes are migan_pipeline_batch_post's for that box.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).  Nothing here synchronises.
 */
#ifndef MIGAN_PIPELINE_REGIONS_HIP_H_
#define MIGAN_PIPELINE_REGIONS_HIP_H_

#include <stddef.h>

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* items as for migan_pipeline_batch_pre (image_chw_u8 is not touched and may be null).  gap in 2 ... 64, max_regions in 1 ... 64. */
int migan_pipeline_regions_scratch_bytes(const migan_pipeline_item* items, int n, int gap, int max_regions, size_t* bytes);

/* labels     HOST array of n device pointers: labels[i] = uint8 [H_i][W_i], the label map of item i
 * count_dev  DEVICE int32 [n]: K_i, or max_regions + 1 when item i has more regions than max_regions (its label map is then
 *            unspecified, its boxes 1 ... are zero; box 0 is always right)
 * boxes_dev  DEVICE int32 [n][max_regions + 1][4], rows {x_min, x_max, y_min, y_max}: slot 0 the single box, slots 1 ... K_i the
 *            regions, the rest zero
 * scratch    migan_pipeline_regions_scratch_bytes(items, n, gap, max_regions) bytes of device memory
 * Any n >= 1; launches carry 16 items each.  MIGAN_EINVAL with nothing launched: a null pointer (table, entry, mask), gap or
 * max_regions out of range, a resolution that is no power of two >= 8, a negative padding, an image below 3 x 3 or of 2^30 pixels
 * or more.  A label map that overlaps a mask, scratch, count_dev, boxes_dev or another label map is UNDEFINED. */
int migan_pipeline_regions_find(const migan_pipeline_item* items, int n, int resolution, int padding, int gap, int max_regions,
                                void* const* labels, int* count_dev, int* boxes_dev, void* scratch, void* stream);

typedef struct migan_pipeline_region_row {
  void* image_chw_u8;          /* [3][height][width]; _pre reads it, _post reads and writes it where labels == label */
  const void* mask_u8;         /* [height][width], 255 = known pixel: the mask AT THE IMAGE'S SIZE (the caller's, or its nearest
                                  resize by migan_pipeline_mask_resize) */
  const void* labels_u8;       /* [height][width] from migan_pipeline_regions_find; may be null when label is 0 */
  int height, width;
  int label;                   /* 1 ... 64: the region of this row; 0: a single-box row */
  int box[4];                  /* {x_min, x_max, y_min, y_max}: host data, from a copy of boxes_dev */
} migan_pipeline_region_row;

/* x_nchw [m][4][R][R] fp32: row r of x is the network input of rows[r].  Any m >= 1; launches carry 32 rows each.
 * MIGAN_EINVAL with nothing launched: a null pointer, a resolution that is no power of two >= 8, an image below 3 x 3 or of 2^30
 * pixels or more, a box that does not lie inside its image or is smaller than 3 x 3, a label outside 0 ... 64, a null labels_u8
 * with a label above 0. */
int migan_pipeline_regions_pre(const migan_pipeline_region_row* rows, int m, int resolution, void* x_nchw, void* stream);

/* y_nchw [m][3][R][R] fp32, gauss25 as in migan_pipeline_post.  Checks as _pre.  Rows of one image may come in any order and in
 * different calls: their pixel sets are disjoint.  Every _pre that reads an image must be queued before the first _post that
 * writes it.  Two rows with the same image and label, a label-0 row next to another row of its image, or an image that overlaps a
 * mask, a label map or y are UNDEFINED. */
int migan_pipeline_regions_post(const migan_pipeline_region_row* rows, int m, int resolution, const void* y_nchw,
                                const float* gauss25, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PIPELINE_REGIONS_HIP_H_ */
