/* comodgan_fp16_hip.h -- C ABI of libmigan_hip.so, Co-Mod-GAN: half-precision blocks.
 *
 * The reference's constructors take Encoder(use_fp16_before_res=...) and Synthesis(use_fp16_after_res=...)
 * (comodgan.py:122,355): encoder block b<res> is half precision where res > use_fp16_before_res (:148), synthesis block
 * b<res> where res > use_fp16_after_res (:384); the two b4 blocks never are.  None, the default, marks no block.
 *
 * Here the 3x3 convolutions (conv0, conv1) of a marked block run with fp16 operands in ONE matrix-core pass: activations
 * (after the style and range scaling) and weights are each rounded once to fp16, products are accumulated in fp32.  In an
 * unmarked block every operand is an error-compensated pair of fp16 values and a product takes three passes.
 * Everything else is as without the marking: activations are stored in fp32, FromRGB, ToRGB, the FIR filters, the dense,
 * style and noise computations are fp32, the state_dict, the workspace size and the prepared weight planes
 * (comodgan_assume_static_weights) are the same.  So the result differs from the unmarked one by the operand rounding only,
 * which is less than the reference's own half-precision path rounds (it also stores fp16 activations).
 *
 * Same conventions as comodgan_hip.h.
 */
#ifndef COMODGAN_FP16_HIP_H_
#define COMODGAN_FP16_HIP_H_

#include "comodgan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* encoder_before_res / synthesis_after_res: the reference's two arguments, -1 for None.  Any other negative value:
 * MIGAN_EINVAL.  Part of what a plan is made for, like the truncation cutoff: call it before sizing the workspace; the next
 * query or forward plans again.  comodgan_launch_info names cm_conv_f16_kernel for the convolutions of marked blocks. */
int comodgan_set_fp16_blocks(comodgan_handle* h, int encoder_before_res, int synthesis_after_res);
int comodgan_get_fp16_blocks(const comodgan_handle* h, int* encoder_before_res, int* synthesis_after_res);

#ifdef __cplusplus
}
#endif
#endif /* COMODGAN_FP16_HIP_H_ */
