/* migan_metrics_hip.h -- C ABI of libmigan_hip.so, PSNR / SSIM of completions against the ground-truth photo, on the device.
 *
 * The reference's two evaluators that need no downloaded network (lib/evaluator/eva_psnr.py:34-56, the for_dataset=None and
 * 'div2k' branches; lib/evaluator/eva_ssim.py:11-41 with size_average=False), for `samples` completions per photo in one call:
 * what depends on the photo alone is computed once, nothing but two doubles per (photo, sample) is written.
 *
 * Per photo of H x W, sample s, channel c, with g the photo's and p the completion's NORMALISED value
 *   uint8 data    v / 255
 *   float32 data  (v - lo) / (hi - lo), not clamped
 *
 *   mse   sum over P of (p - g)^2 / (3 |P|); P = the pixels with shave <= y < H - shave and shave <= x < W - shave.
 *         uint8: the squared byte differences are summed in integers, mse = (double)sse / ((double)count * 65025.0);
 *         float32: the difference is formed in fp32, squared and summed in fp64.   psnr = -10 log10(mse) is the caller's.
 *   ssim  window of 11 taps, sigma 1.5 (the reference's float32 taps), zero padding of 5, taps not renormalised at the border;
 *         per channel the map ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = 1e-4, C2 = 9e-4, in
 *         fp32, evaluated separably; its mean over all channels and ALL pixels (never shaved), summed in fp64.
 *
 * With a mask (uint8 [H][W], 255 = known pixel, the convention of migan_compose_output and of the pipeline) both P and the
 * pixels the SSIM map is averaged over keep only the pixels whose mask byte is not 255; the windows still see the whole image.
 * A region that turns out empty gives NaN (0 / 0) in that row; it is not an error, the mask being device data.
 *
 * Deterministic: every workgroup writes partial sums to scratch, a second launch adds them in index order; no floating-point
 * atomics.  Two calls on the same inputs give the same bits.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).
 */
#ifndef MIGAN_METRICS_HIP_H_
#define MIGAN_METRICS_HIP_H_

#include <stddef.h>

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIGAN_METRICS_U8 0   /* element type of gt and pred */
#define MIGAN_METRICS_F32 1
#define MIGAN_METRICS_CHW 0  /* [3][H][W] */
#define MIGAN_METRICS_HWC 1  /* [H][W][3] */

/* gt: one image; pred: `samples` tightly packed images in gt's layout and type; mask: null or [H][W] uint8.  Device memory. */
typedef struct {
  const void* gt;
  const void* pred;
  const unsigned char* mask;
  int H, W;
} migan_metrics_item;

/* Bytes of scratch migan_metrics_batch needs for these items (the pointers are not looked at).  0 with migan_last_error set
 * when items is null, n < 1, samples < 1, or an item has H < 1 or W < 1. */
size_t migan_metrics_scratch_bytes(const migan_metrics_item* items, int n, int samples);

/* out_mse, out_ssim: device arrays [n * samples] of double, row i * samples + s = sample s of item i.  Any n >= 1; launches
 * carry 32 items each.  Byte pointers carry no alignment promise; float32 pointers are 4-byte aligned.  Inputs are only read;
 * nothing outside [0, H) x [0, W) of any plane is read.
 * MIGAN_EINVAL, with nothing launched: a null items, gt, pred, scratch, out_mse or out_ssim; n < 1; samples < 1; H < 1 or W < 1;
 * shave < 0; H - 2 shave < 1 or W - 2 shave < 1 for any item; hi == lo or a non-finite lo / hi; an unknown dtype or layout.
 * (lo, hi) is used by float32 data only. */
int migan_metrics_batch(const migan_metrics_item* items, int n, int samples, int dtype, int layout, int shave,
                        float lo, float hi, void* scratch, double* out_mse, double* out_ssim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_METRICS_HIP_H_ */
