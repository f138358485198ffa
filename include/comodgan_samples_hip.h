/* comodgan_samples_hip.h -- C ABI of libmigan_hip.so, Co-Mod-GAN: several completions per image from one encoder pass.
 *
 * Co-Mod-GAN is the stochastic model of the pair: the same (image, mask) with S different z gives S different completions.
 * The encoder (comodgan.py:192-204) never sees z, so an S-samples forward runs it once per image, at batch `batch`, and the
 * mapping network, the affine / style layers and the synthesis network once per sample, at batch `batch * samples`.
 *
 * Definition (there is no reference equivalent): with xr = x.repeat_interleave(samples, 0),
 *   forward_samples(x, z)[i * samples + s]  is what  forward(xr, z)[i * samples + s]  gives,
 * for the same truncation_psi, truncation cutoff, noise_mode and -- noise_mode random -- the same noise blob.
 * Output, z and the noise blob are image-major: sample s of image i is row i * samples + s.
 *
 * Same conventions as comodgan_hip.h.  The entry points of that header are the case samples == 1 of these: they make the
 * same launches with the same arguments.
 */
#ifndef COMODGAN_SAMPLES_HIP_H_
#define COMODGAN_SAMPLES_HIP_H_

#include "comodgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* samples < 1, or a batch * samples that does not fit an int: MIGAN_EINVAL (migan_last_error names the argument).
 * The prepared weight planes of comodgan_assume_static_weights sit at the head of the workspace at offsets that depend on
 * neither batch nor samples: forwards with different `samples` on one workspace share them. */
int comodgan_workspace_bytes_samples(const comodgan_handle* h, int batch, int samples, size_t* bytes);

/* x: [batch,4,R,R]; z: [batch*samples, z_dim]; y: [batch*samples,3,R,R];
 * noise (noise_mode random): as for comodgan_forward at batch batch*samples -- for every synthesis layer in forward order a
 * [batch*samples][res][res] block, rows in output order -- or null. */
int comodgan_forward_samples(comodgan_handle* h, const void* x_nchw, const void* z, void* y_nchw, int batch, int samples,
                             float truncation_psi, int noise_mode, const void* noise,
                             void* workspace, size_t workspace_bytes, void* stream);
int comodgan_forward_samples_timed(comodgan_handle* h, const void* x_nchw, const void* z, void* y_nchw, int batch, int samples,
                                   float truncation_psi, int noise_mode, const void* noise,
                                   void* workspace, size_t workspace_bytes, void* stream, float* launch_ms, int n_launch_ms);

/* comodgan_num_launches / comodgan_launch_info describe the plan made last, an S-samples plan included.  Their figures are
 * per INPUT image: an encoder launch (and the weight preparation, and the fc of synthesis.b4, which reads the global code
 * only) is counted once per image; a mapping, affine, style or synthesis launch S times, once per sample of that image.
 * The sum of flops over the launches is the work the plan does for one input image and its S completions.
 *
 * comodgan_debug_tensor for an S-samples plan: encoder tensors ("encoder.*") have leading dimension batch, the tensors of
 * "mapping" and "synthesis.*" batch * samples. */
int comodgan_debug_tensor_samples(const comodgan_handle* h, int batch, int samples, const char* layer, size_t* byte_offset,
                                  int64_t shape[4], int* ndim);

#ifdef __cplusplus
}
#endif
#endif /* COMODGAN_SAMPLES_HIP_H_ */
