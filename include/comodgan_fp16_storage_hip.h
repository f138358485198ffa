/* comodgan_fp16_storage_hip.h -- C ABI of libmigan_hip.so, Co-Mod-GAN: fp16 activation storage in half-precision blocks.
 *
 * comodgan_set_fp16_blocks, declared in comodgan_fp16_hip.h, makes the 3x3 convolutions of the marked blocks single-pass fp16 and leaves
 * every activation in fp32.  The reference stores those activations in fp16 (comodgan.py:37-44,306-313, stylegan.py:174,190,233).
 * This switch, per handle and off by default, does the same: with it on, and only in blocks that are marked, the tensors below are
 * _Float16 in the workspace, which halves their bytes and their traffic.  Without a marked block it changes nothing at all.
 *
 *   FromRGB output                  fp16 iff encoder block b<R> is marked
 *   marked encoder block b<res>     its input, feat[res] (the conv0 output and skip tensor) and the FIR-down output are fp16; the
 *                                   conv1 output is fp16 iff the next block is marked too (the marking is monotone from the top);
 *                                   encoder.b4 and everything behind it is untouched
 *   marked synthesis block b<res>   x0 (the FIR-up output) and x1 (the conv1 output, which ToRGB reads) are fp16.  The raw output
 *                                   of the transposed convolution is fp16 except in the lowest-resolution marked block, whose
 *                                   input comes from an fp32 block: there the convolution launches are those of the operand-only
 *                                   mode, fp32 in and out
 *   skip operand of FIR-up          as the ENCODER block of that resolution is marked, whatever the synthesis block is
 *
 * Everything else stays fp32: the network input, the ToRGB output and the running image, w, w0, styles, coefficients, noise,
 * biases, weights, the mapping network and the dense layers.  All arithmetic is fp32 on converted values (the matrix-core
 * products take the fp16 operands they took before); a stored value is rounded once, to nearest even.
 *
 * No stored value can overflow fp16 (largest finite value 65504):
 *   - a value behind an activation is clamped to +-256 (lrelu_agc), plus at most 256 of skip tensor: |v| <= 512;
 *   - a raw transposed-convolution output is sum_k x_k w_k over at most 9 Cin terms with |x_k| <= 512 and demodulated weights of
 *     unit norm per output channel, so by Cauchy-Schwarz |out| <= 512 sqrt(9 Cin) <= 34753 for Cin <= 512;
 *   - the FIR gain of 4 of the up path is applied after the fp16 load, in fp32, and what is stored behind it is again clamped.
 *
 * The prepared weight planes (comodgan_assume_static_weights) sit at the head of the workspace in both modes: one workspace,
 * sized for the larger mode, serves both.  comodgan_launch_info names the typed kernels (cm_conv_h_kernel, cm_fir_h_kernel,
 * cm_fir_samples_h_kernel, cm_fromrgb_h_kernel, cm_torgb_h_kernel); an FIR-up launch is typed as soon as one of its three
 * tensors is.
 *
 * Same conventions as comodgan_hip.h.
 */
#ifndef COMODGAN_FP16_STORAGE_HIP_H_
#define COMODGAN_FP16_STORAGE_HIP_H_

#include "comodgan_fp16_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element types a workspace tensor can have (the values of MIGAN_DTYPE_F32 / MIGAN_DTYPE_F16) */
#define COMODGAN_DTYPE_F32 0
#define COMODGAN_DTYPE_F16 2

/* on != 0: the blocks marked through comodgan_set_fp16_blocks store their activations in fp16.  Part of what a plan is made for:
 * call it before sizing the workspace; the next query or forward plans again. */
int comodgan_set_fp16_storage(comodgan_handle* h, int on);
int comodgan_get_fp16_storage(const comodgan_handle* h, int* on);

/* Element type of a debug tensor (comodgan_set_debug; the offset and shape come from comodgan_debug_tensor[_samples], which do not
 * say that a tensor is fp16).  Besides the layer outputs, "<encoder block>.fromrgb", "<encoder conv1>.fir" and
 * "<synthesis conv0>.raw" can be asked for; the last two live in one scratch buffer shared by all layers, so their DATA are the
 * last writer's.  Unknown layer: MIGAN_EINVAL. */
int comodgan_debug_tensor_dtype(const comodgan_handle* h, int batch, int samples, const char* layer, int* dtype);

#ifdef __cplusplus
}
#endif
#endif /* COMODGAN_FP16_STORAGE_HIP_H_ */
