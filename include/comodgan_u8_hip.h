/* comodgan_u8_hip.h -- C ABI of libmigan_hip.so, Co-Mod-GAN: uint8 photo and mask in, composited uint8 completions out.
 *
 * What scripts/demo.py does around the generator (:56-66 and :135-140), at network resolution, inside one forward:
 *   x   = cat([mask - 0.5, img * mask])                      migan_pack_input
 *   y   = Generator.forward(x, z, ...)                       comodgan_forward_samples
 *   out = (y * 0.5 + 0.5).clamp(0, 1) * 255 -> uint8, pasted over the known pixels    migan_compose_output
 * The first kernel (FromRGB of the top encoder block) forms x in registers from the bytes, and the last one (ToRGB at
 * res == R) composes its result over the photo and writes bytes: neither x [batch,4,R,R] nor y [batch*samples,3,R,R]
 * exists, and no workspace tenant takes their place.
 *
 * Definition: for img [batch,R,R,3] (HWC), mask [batch,R,R] (255 = known pixel, anything else = hole), z [batch*samples,z_dim],
 *   out[i * samples + s]  ==  compose_output(forward_samples(pack_input(img, mask), z)[i * samples + s], img[i], mask[i])
 * byte for byte, for the same truncation_psi, truncation cutoff, noise_mode, fp16 settings and -- noise_mode random -- the
 * same noise blob: the two kernels evaluate the device functions of migan_pack_input / migan_compose_output on the same
 * values, every launch between them is the fp32-I/O forward's, and the forward is run-to-run deterministic.
 * samples == 1 is the plain forward.  Row i * samples + s of out is composed over photo i: the caller repeats nothing.
 *
 * Fused forward only: comodgan_encode / comodgan_synthesize (comodgan_stages_hip.h) keep their fp32 tensors.
 *
 * Workspace: comodgan_workspace_bytes[_samples](batch, samples) serves this call; the layout does not depend on the I/O
 * mode, so fp32 and uint8 forwards alternate on one workspace and share the planes of comodgan_assume_static_weights.
 *
 * Alignment: img, mask and out are read and written a byte at a time and need none; z and the workspace as for
 * comodgan_forward (4 and 256 bytes).
 * Aliasing: img and mask are only read.  An `out` that overlaps img, mask, z, noise or the workspace is UNDEFINED (a
 * workgroup of the last kernel reads photo bytes that another may already have overwritten).
 *
 * Same conventions as comodgan_hip.h; errors as for comodgan_forward_samples (null tensor, samples < 1, a batch * samples
 * that does not fit an int, noise_mode, workspace: MIGAN_EINVAL; before comodgan_commit: MIGAN_ESTATE).
 */
#ifndef COMODGAN_U8_HIP_H_
#define COMODGAN_U8_HIP_H_

#include "comodgan_samples_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int comodgan_forward_u8(comodgan_handle* h, const void* img_hwc_u8, const void* mask_u8, const void* z, void* out_hwc_u8,
                        int batch, int samples, float truncation_psi, int noise_mode, const void* noise,
                        void* workspace, size_t workspace_bytes, void* stream);

/* After either call comodgan_num_launches / comodgan_launch_info describe the uint8 plan: the fp32-I/O plan of the same
 * (batch, samples, settings) except for its FromRGB entry (migan::cm_fromrgb_u8_kernel<YH>, 3 + 1 bytes in per pixel) and
 * its last ToRGB entry (migan::cm_torgb_u8_kernel<LPP, XH>, 3 + 1 bytes in and 3 bytes out per pixel beside the feature map
 * and the running image).  A sizing query (comodgan_workspace_bytes[_samples]) makes the fp32-I/O plan the one described. */
int comodgan_forward_u8_timed(comodgan_handle* h, const void* img_hwc_u8, const void* mask_u8, const void* z, void* out_hwc_u8,
                              int batch, int samples, float truncation_psi, int noise_mode, const void* noise,
                              void* workspace, size_t workspace_bytes, void* stream, float* launch_ms, int n_launch_ms);

#ifdef __cplusplus
}
#endif
#endif /* COMODGAN_U8_HIP_H_ */
