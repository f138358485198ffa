/* migan_pipeline_samples_hip.h -- C ABI of libmigan_hip.so, deployed pipeline: several completions per photo, out of place.
 *
 * The post step of the batch pipeline (migan_hip.h: migan_pipeline_batch_pre / _post) for a generator that gives S outputs per
 * image (comodgan_forward_samples, or S = 1 of any generator), written into destinations of their own:
 *
 *   migan_pipeline_batch_scratch_bytes(items, n) -> scratch
 *   migan_pipeline_batch_pre(items, n, R, padding, x, bbox_dev, scratch)         boxes and network input, once per image
 *   generator: x [n][4][R][R] -> y [n * samples][3][R][R]
 *   migan_pipeline_batch_post_samples(items, n, samples, R, y, bbox_dev, gauss25, scratch, outs)
 *
 * One kernel reads each image once, builds its feathered mask once and writes `samples` finished images.
 *
 * Definition: for every sample s, outs[i][s] holds
 *   inside the box of item i   the byte migan_pipeline_batch_post stores into a copy of the image for y row i * samples + s,
 *   outside the box            the image's byte.
 * Unlike the in-place form, which leaves the image of an item alone when its row of bbox_dev does not lie inside the image or
 * is smaller than 3x3, this call defines its output for such an item: `samples` plain copies of the image.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).
 */
#ifndef MIGAN_PIPELINE_SAMPLES_HIP_H_
#define MIGAN_PIPELINE_SAMPLES_HIP_H_

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* items: the migan_pipeline_item array that went through migan_pipeline_batch_pre (same scratch, same bbox_dev);
 * image_chw_u8 is only READ here.  outs: HOST array of n device pointers, outs[i] = [samples][3][H_i][W_i] uint8.
 * y_nchw: [n*samples][3][R][R] fp32, row i*samples + s = sample s of item i (the layout of comodgan_forward_samples).
 * Any n >= 1; launches carry 32 items each.  The items, resolution, bbox_dev and scratch are checked as by
 * migan_pipeline_batch_post; samples < 1, a null outs or a null outs[i]: MIGAN_EINVAL.
 * A destination that overlaps an image, a mask, y, scratch or another destination is UNDEFINED. */
int migan_pipeline_batch_post_samples(const migan_pipeline_item* items, int n, int samples, int resolution,
                                      const void* y_nchw, const int* bbox_dev, const float* gauss25,
                                      void* scratch, void* const* outs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PIPELINE_SAMPLES_HIP_H_ */
