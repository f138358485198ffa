/* migan_pipeline_native_hip.h -- C ABI of libmigan_hip.so, deployed pipeline: crops at native size, no resampling.
 *
 * The row pipeline (migan_pipeline_regions_hip.h: migan_pipeline_regions_pre / _post) squeezes every box to the network resolution
 * R and blows the generator's output back up to the box (bilinear, both ways).  The fully convolutional forward (migan_hip.h:
 * migan_forward_hw) accepts any height and width that are multiples of R / 4, so a crop can be completed at the photo's own scale.
 * The two calls below are the steps either side of that forward, for rows whose network window has ONE size:
 *
 *   migan_pipeline_native_pre(rows, m, height, width, x)            network input of every row, x [m][4][height][width]
 *   generator: migan_forward_hw(x, y, m, height, width)             y [m][3][height][width]
 *   migan_pipeline_native_post(rows, m, height, width, y, gauss25)
 *
 * The rows are migan_pipeline_region_row (mask_u8 at the image's size, label 0 or a region of labels_u8).  box = {x0, x1, y0, y1}
 * is the part of the window that lies inside the photo, cw = x1 - x0 <= width, ch = y1 - y0 <= height; it sits at the top-left
 * corner of the window.
 *
 * Definition, for row r at window pixel (py, px):
 *   _pre    py < ch and px < cw, m = mask[y0 + py][x0 + px] / 255:  plane 0 = m - 0.5,
 *           plane c + 1 = (image[c][y0 + py][x0 + px] * 2 / 255 - 1) * m  -- migan_pipeline_regions_pre's arithmetic, the same
 *           correctly rounded operations, without the two resamplings.  Everywhere else the pixel is UNKNOWN: (-0.5, 0, 0, 0).
 *           Every element of x[r] is written exactly once.
 *   _post   migan_pipeline_regions_post on the box -- the mask window 0 outside the box, 3 x 3 maximum, 5 x 5 gaussian with reflect
 *           padding at the box's borders, the 25 products summed in fp64 -- with the generator output taken at the same pixel:
 *           o = clamp((y[r][c][py][px] * 0.5 + 0.5) * 255, 0, 255), v = image * mk + o * (1 - mk), clamped, truncated to uint8,
 *           stored in place: everywhere in the box for label 0, only where labels == label otherwise.  Nothing of y outside
 *           [0, ch) x [0, cw) is read.
 * With height = width = R and an R x R box the resamplings of migan_pipeline_regions_pre / _post have weights exactly 1 and 0: both
 * calls then give their bits.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).  Nothing here synchronises.
 */
#ifndef MIGAN_PIPELINE_NATIVE_HIP_H_
#define MIGAN_PIPELINE_NATIVE_HIP_H_

#include "migan_pipeline_regions_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x_nchw [m][4][height][width] fp32.  Any m >= 1; launches carry 32 rows each.  MIGAN_EINVAL with nothing launched: what
 * migan_pipeline_regions_pre refuses in a row (a null pointer, an image below 3 x 3 or of 2^30 pixels or more, a box that does not
 * lie inside its image or is smaller than 3 x 3, a label outside 0 ... 64, a null labels_u8 with a label above 0), a null tensor,
 * height or width below 1 or height * width of 2^28 or more, a box wider or taller than the window. */
int migan_pipeline_native_pre(const migan_pipeline_region_row* rows, int m, int height, int width, void* x_nchw, void* stream);

/* y_nchw [m][3][height][width] fp32, gauss25 as in migan_pipeline_post.  Checks as _pre.  Order and UNDEFINED cases are
 * migan_pipeline_regions_post's: rows of one image may come in any order and in different calls, every _pre that reads an image
 * must be queued before the first _post that writes it; two rows with the same image and label, a label-0 row next to another row
 * of its image, or overlapping buffers are undefined. */
int migan_pipeline_native_post(const migan_pipeline_region_row* rows, int m, int height, int width, const void* y_nchw,
                               const float* gauss25, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PIPELINE_NATIVE_HIP_H_ */
