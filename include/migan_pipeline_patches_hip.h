/* migan_pipeline_patches_hip.h -- C ABI of libmigan_hip.so, deployed pipeline: several completions per photo as box-sized patches.
 *
 * The post step of the batch pipeline (migan_hip.h: migan_pipeline_batch_pre / _post) for a generator that gives S outputs per
 * image, like migan_pipeline_batch_post_samples (migan_pipeline_samples_hip.h), but only the pixels that differ between the
 * completions are written: the crop [y_min, y_max) x [x_min, x_max) of item i, tightly packed.
 *
 *   migan_pipeline_batch_scratch_bytes(items, n) -> scratch
 *   migan_pipeline_batch_pre(items, n, R, padding, x, bbox_dev, scratch)         boxes and network input, once per image
 *   generator: x [n][4][R][R] -> y [n * samples][3][R][R]
 *   migan_pipeline_batch_post_patches(items, n, samples, R, y, bbox_dev, gauss25, scratch, outs, out_bytes)
 *
 * One kernel reads the crop of each image once, builds its feathered mask once and writes `samples` patches.  Nothing outside the
 * box is read or written.
 *
 * Definition: with {x_min, x_max, y_min, y_max} = row i of bbox_dev, cw = x_max - x_min and ch = y_max - y_min, outs[i] is
 * [samples][3][ch][cw] uint8, and its byte (s, c, py, px), at outs[i] + ((s * 3 + c) * ch + py) * cw + px, is the byte
 * migan_pipeline_batch_post_samples writes at (s, c, y_min + py, x_min + px) of its destination for the same arguments.
 *
 * The box is device data, so the size of a patch is not known to this call.  The caller sizes outs[i] from a host copy of
 * bbox_dev (samples * 3 * ch * cw bytes), or from the bound samples * 3 * H_i * W_i, and states the capacity in out_bytes[i]:
 *   capacity rule      an item whose samples * 3 * ch * cw exceeds out_bytes[i] is skipped: outs[i] is left untouched, whole;
 *   invalid-box rule   an item whose row of bbox_dev does not lie inside its image, or is smaller than 3x3, is skipped as well
 *                      (migan_pipeline_batch_post_samples defines plain copies for it; a patch of no box has no size).
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).
 */
#ifndef MIGAN_PIPELINE_PATCHES_HIP_H_
#define MIGAN_PIPELINE_PATCHES_HIP_H_

#include <stddef.h>

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* items: the migan_pipeline_item array that went through migan_pipeline_batch_pre (same scratch, same bbox_dev);
 * image_chw_u8 is only READ here, and only inside the box.  outs: HOST array of n device pointers, out_bytes: HOST array of
 * their capacities in bytes; outs[i] may be null where out_bytes[i] is 0 (the item is then skipped by the capacity rule).
 * y_nchw: [n*samples][3][R][R] fp32, row i*samples + s = sample s of item i (the layout of comodgan_forward_samples).
 * Any n >= 1; launches carry 32 items each.  The items, resolution, bbox_dev and scratch are checked as by
 * migan_pipeline_batch_post_samples; samples < 1, a null outs, a null out_bytes, or a null outs[i] with a non-zero
 * out_bytes[i]: MIGAN_EINVAL.
 * A destination that overlaps an image, a mask, y, scratch, bbox_dev or another destination is UNDEFINED. */
int migan_pipeline_batch_post_patches(const migan_pipeline_item* items, int n, int samples, int resolution,
                                      const void* y_nchw, const int* bbox_dev, const float* gauss25,
                                      void* scratch, void* const* outs, const size_t* out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PIPELINE_PATCHES_HIP_H_ */
