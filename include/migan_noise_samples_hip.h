/* migan_noise_samples_hip.h -- C ABI of libmigan_hip.so, MI-GAN: S completions per image from per-sample noise, one encoder pass.
 *
 * The reference's TRAINING generator (lib/model_zoo/migan.py:130-138, Generator.forward(x, noise_mode='random') :546) adds
 * torch.randn([N,1,H,W]) * noise_strength in every synthesis SeparableConv2d with use_noise: a fresh noise image per batch row.  The
 * exported inference module (migan_inference.py:165-167) froze that to one noise_const [res,res] plane, broadcast over the batch, and
 * so does migan_forward.  The calls below take the draw from the caller instead: one noise blob per output row.
 *
 *   F (migan_noise_floats_hw) = the sum, over the noisy layers in the order they run, of hout * wout:
 *     synthesis.b8.conv1, synthesis.b8.conv2, synthesis.b16.conv1, ... synthesis.b<R>.conv2
 *   a row's blob = those planes, each [hout][wout] fp32, concatenated
 *
 *   x [n][4][H][W], noise [n * samples][F]  ->  y [n * samples][3][H][W]
 *   y row i * samples + s = the reference inference module's forward of x[i] with every noisy layer's noise_const replaced by that
 *   row's plane (= the training generator's noise_mode='random' with the draw given).  noise_strength, the fp32 add before the
 *   activation and the storage rounding are those of migan_forward; with every row's blob = the model's own planes (tiled and
 *   cropped as migan_forward_hw does at H x W) every row i * samples + s holds the bits of migan_forward_hw's row i.
 *
 * The encoder and synthesis.b4 have no noise (migan_inference.py:264-265): they run ONCE per image, at batch n; everything from
 * synthesis.b8.conv1 on runs at batch n * samples through the per-row form of each kernel (migan::SepRowArgs), which reads row b's
 * plane where it lies in the caller's blob and the skip tensor of image b / samples.  The encoder's feature maps are not replicated;
 * only synthesis.b4's 4 x 4 output and image are copied once per row.  No noise plane is tiled, cropped or copied.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).  height, width: migan_forward_hw's rule
 * (positive multiples of resolution / 4); height = width = resolution is the square case.
 * MIGAN_EINVAL, with nothing launched: samples < 1, n < 1, a null tensor, a bad height / width, a workspace that is too small.
 * MIGAN_EUNSUPPORTED, with nothing launched: resolutions above 512 (layers with fewer than 64 channels have no per-row form), and a handle
 * in keep-intermediates mode (migan_set_debug).
 */
#ifndef MIGAN_NOISE_SAMPLES_HIP_H_
#define MIGAN_NOISE_SAMPLES_HIP_H_

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* floats of one row's noise blob for inputs of height x width */
int migan_noise_floats_hw(migan_handle* h, int height, int width, size_t* floats);
/* workspace of migan_forward_samples_hw for n images x samples completions (larger than migan_workspace_bytes_hw(n)) */
int migan_workspace_bytes_samples_hw(migan_handle* h, int n, int samples, int height, int width, size_t* bytes);
/* sub-batches of the n * samples rows run on the handle's streams like migan_forward's (migan_set_streams), split on image boundaries.
 * Kernel forms are picked as migan_forward_hw of the n images picks them (grids are sized for the rows): the single-image forms for
 * n = 1 and for no row otherwise, also where a sub-batch holds one image's rows.  samples is at most 2^20 - 64, n * samples below 2^24.
 * After the call migan_launch_info names the kernels it ran (the per-row forms from synthesis.b8.conv1 on). */
int migan_forward_samples_hw(migan_handle* h, const void* x_nchw, const void* noise, void* y_nchw, int n, int samples,
                             int height, int width, void* workspace, size_t workspace_bytes, void* stream);

/* One SeparableConv2d of that forward on its own (operator-level tests): migan_sepconv_forward on the same descriptor, unchanged in
 * layout, with
 *   d->noise_const  [batch][res_out][width_out]: one plane per row (null: no noise)
 *   d->skip         [batch / samples][res_out][width_out][cout]: row b adds image b / samples (null: no skip)
 * batch must be a multiple of samples >= 1.  A layer no samples forward contains -- down == 2, fromrgb, fewer than 64 channels -- is
 * MIGAN_EINVAL.  migan_last_kernel() then names the per-row symbol (migan::sepconv_rows_kernel<...>, ..._pipe_rows_kernel<...>, ...). */
int migan_sepconv_forward_samples(const migan_sepconv_desc* d, int samples, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_NOISE_SAMPLES_HIP_H_ */
