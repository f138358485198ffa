/* comodgan_stages_hip.h -- C ABI of libmigan_hip.so, Co-Mod-GAN: the three stages of the generator as calls of their own.
 *
 * The reference's Generator.forward (comodgan.py:435-455) is
 *   ws = mapping(z, c, truncation_psi, truncation_cutoff)            stylegan.py:396-439
 *   x, feats = encoder(img)                                           comodgan.py:190-204
 *   img = synthesis(x, feats, ws, noise_mode, return_intermediate_outs)   comodgan.py:395-421
 * and its callers also use the stages alone: encode once and complete later, edit ws (style mixing, interpolation in W,
 * per-layer truncation), read the per-resolution ToRGB outputs (the distillation loss of lib/experiments/loss.py:170-186).
 * comodgan_forward / comodgan_forward_samples stay the fused walk (one workspace holds every stage tensor, the mapping network
 * runs beside the encoder); the calls below make the same launches stage by stage with the stage tensors in CALLER memory.
 *
 * Same conventions as comodgan_hip.h: raw device pointers, nothing allocated, every launch on `stream`, 0 or a MIGAN_E* code.
 *
 * Stage tensors
 *   ws      [rows][num_ws][w_dim] fp32: row r of sample b is what the layers reading ws[:, r] get (comodgan.py:399-405)
 *   w0      [batch][w0_dim] fp32: the encoder's global code (its return value `x`)
 *   feats   one pointer per resolution, index k = log2(res) - 2 for res = 4 ... R: NHWC [batch][res][res][C_res] -- the memory of
 *           a torch channels_last tensor of shape [batch, C_res, res, res].  fp32; _Float16 for the blocks that
 *           comodgan_set_fp16_blocks marks on the encoder side while comodgan_set_fp16_storage is on (never res 4).
 *   to_rgb / res_img   optional outputs of comodgan_synthesize, same index: planar fp32 [rows][3][res][res].
 *
 * One workspace serves the three stages and the fused forward: the prepared weight planes sit at its head at the offsets they
 * have in comodgan_forward, so with comodgan_assume_static_weights the preparation made by any of comodgan_encode /
 * comodgan_synthesize / the fused forwards on a workspace serves the others on the same workspace and stream.
 * comodgan_mapping leaves the head alone.  Past the head every call uses the workspace as scratch: nothing in it survives from one
 * call to the next, which is why the stage tensors are the caller's.
 */
#ifndef COMODGAN_STAGES_HIP_H_
#define COMODGAN_STAGES_HIP_H_

#include "comodgan_samples_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COMODGAN_MAX_RES_LEVELS 8    /* res 4 ... 512 */

/* Bytes that serve comodgan_mapping at batch * samples rows, comodgan_encode at `batch`, comodgan_synthesize at (batch, samples)
 * and comodgan_forward_samples at (batch, samples), with the fp16 settings and the truncation cutoff the handle has now. */
int comodgan_stages_workspace_bytes(const comodgan_handle* h, int batch, int samples, size_t* bytes);

/* Mapping.forward (c_dim = 0).  z: [rows][z_dim]; ws: [rows][num_ws][w_dim].  truncation_psi != 1 pulls rows [0, cutoff) towards
 * w_avg, the others stay raw; truncation_cutoff -1 = None (every row).  The handle's comodgan_set_truncation_cutoff is not read. */
int comodgan_mapping(comodgan_handle* h, const void* z, void* ws, int rows, float truncation_psi, int truncation_cutoff,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Encoder.forward.  x: [batch,4,R,R]; w0 and feats[0 ... log2(R) - 2] are written (feats[k] 16-byte aligned, none null). */
int comodgan_encode(comodgan_handle* h, const void* x_nchw, void* w0, void* const* feats, int batch,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Synthesis.forward on rows = batch * samples rows of ws against the features of `batch` images: row i * samples + s is completed
 * from image i (samples = 1: the reference's call).  y: [rows,3,R,R].  noise: as for comodgan_forward_samples.
 * to_rgb / res_img: null, or arrays of log2(R) - 1 pointers, each null or an output:
 *   res_img[k]  the running image after block b<res> (comodgan.py:416-417); at res = R that is y itself and the entry is ignored
 *   to_rgb[k]   the block's ToRGB output before upsample2d(img) is added (comodgan.py:341-343), written by the launch that writes
 *               the sum; at res = 4 the two are one tensor (comodgan.py:410-411) and the entry is ignored. */
int comodgan_synthesize(comodgan_handle* h, const void* w0, const void* const* feats, const void* ws, void* y_nchw, int batch, int samples,
                        int noise_mode, const void* noise, void* const* to_rgb, void* const* res_img,
                        void* workspace, size_t workspace_bytes, void* stream);

/* comodgan_num_launches / comodgan_launch_info describe the plan made last: after one of the three calls above, that stage's
 * launches (figures per input image, as in comodgan_samples_hip.h).  The lists of comodgan_encode and comodgan_synthesize start
 * with the weight preparation like the fused forward's; whether a call really ran it is counted here: the number of weight
 * preparations this handle has launched since it was created (a call that found valid planes under
 * comodgan_assume_static_weights does not count). */
int comodgan_weight_preparations(const comodgan_handle* h, unsigned long long* n);

#ifdef __cplusplus
}
#endif
#endif /* COMODGAN_STAGES_HIP_H_ */
