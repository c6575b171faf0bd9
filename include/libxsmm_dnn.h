/* libxsmm_dnn.h -- the common part of the reference's DNN interface: error codes, data types, tensor formats, datalayouts and
 * tensor handles that link caller memory (reference: include/libxsmm_dnn.h:47-263 and :359-390, include/libxsmm_typedefs.h:
 * 311-346, src/libxsmm_dnn.c:70-189, :330-360, :1000-1570), and the producers of low-precision GEMM inputs: fp32 -> int16
 * quantisation, its inverse and the fp32 <-> bf16 converters (:331-357 and :414-426, src/libxsmm_dnn.c:2394-2907). The layer
 * that uses the tensor handles is the fully-connected one (libxsmm_dnn_fullyconnected.h); the pooling layer and the fused
 * batch-norm layer have headers of their own (libxsmm_dnn_pooling.h, libxsmm_dnn_fusedbatchnorm.h). The convolution layer
 * (:265-329 and :364-412) is declared in libxsmm_dnn_convolution.h, a file of this project's that this header includes. The RNN
 * cell layer is declared in libxsmm_dnn_rnncell.h, as in the reference, and included below (forward pass only: DESIGN.md 8q). The
 * common part lies in libxsmm_dnn_tensor.h, another file of this project's that this header includes (the reference keeps both
 * in libxsmm_dnn.h itself); the quantisation and conversion functions are declared below. Line numbers refer to the
 * reference's include/libxsmm_dnn.h unless a file is named.
 *
 * Where operands may live: memory the GPU reaches (device, pinned, managed) is processed in place on the calling thread's
 * stream (libxsmm_amd_set_stream); host-visible memory (pinned, managed) is complete on return; pageable host memory is
 * staged through device scratch and complete on return. `in` and `out` overlapping is not supported. Inside
 * libxsmm_amd_defer_begin/end the calls are not recorded: they seal the open burst and run in call order. */
#ifndef LIBXSMM_DNN_H
#define LIBXSMM_DNN_H

#include "libxsmm.h"

#include "libxsmm_dnn_tensor.h" /* error codes, data types, formats, datalayouts and tensor handles */
#include "libxsmm_dnn_convolution.h" /* the convolution layer */

typedef union libxsmm_intfloat { unsigned int ui; float f; } libxsmm_intfloat; /* :334-337 */

/* F32 masking defines (:340-346; the spelling is the reference's) */
#define LIBXSNN_DNN_MASK_SIGN_F32      0x80000000
#define LIBXSMM_DNN_MASK_EXP_F32       0x7f800000
#define LIBXSMM_DNN_MASK_MANT_F32      0x007fffff
#define LIBXSMM_DNN_MASK_ABS_F32       0x7fffffff
#define LIBXSMM_DNN_MASK_FULL_F32      0xffffffff
#define LIBXSMM_DNN_MANT_SZ_F32        23
#define LIBXSMM_DNN_SZ_F32             32

/* DFP16 masking defines (:349-350) */
#define LIBXSMM_DNN_MANT_DFP16         15
#define LIXSMMM_DNN_RES_DFP16          libxsmm_sexp2_i8i(-(LIBXSMM_DNN_MANT_DFP16))

/* Quantization Rounding Defines (:353-357) */
#define LIBXSMM_DNN_QUANT_NO_ROUND       80000
#define LIBXSMM_DNN_QUANT_BIAS_ROUND     80001
#define LIBXSMM_DNN_QUANT_STOCH_ROUND    80002
#define LIBXSMM_DNN_QUANT_NEAREST_ROUND  80003
#define LIBXSMM_DNN_QUANT_FPHW_ROUND     80004

/** fp32 -> int16 with one power-of-two scale per tensor (:416-418). max = the largest fabsf over the whole tensor.
 *  FPHW_ROUND: frexpf(max, &e), maxexp = e - (15 - add_shift), out = (short)roundf(in * 2^-maxexp) -- halves away from zero,
 *  the scalar branch of the reference; the narrowing is float -> int32 -> low 16 bits -- and *scf = (unsigned char)(-maxexp).
 *  The other modes work on the bits (libxsmm_internal_quantize_scalar_no_scf): with max_exp the exponent field of max, an
 *  element's mantissa with its leading bit is shifted right by rhs = 9 + (max_exp - exponent) + add_shift (as unsigned
 *  char, at most 24), negated in two's complement if the input is negative and the shifted value is not zero, and only then
 *  incremented by the rounding rule -- so negative values round toward +Inf, and one whose mantissa is shifted out entirely
 *  can become +1; the low 16 bits are the result and *scf = (unsigned char)(14 - add_shift - (max_exp - 127)).
 *  STOCH_ROUND uses the reference's formula with p in [0, 1] from a counter-based generator instead of rand()
 *  (libxsmm_amd_dnn_quantize_set_seed in libxsmm_amd.h). dequantise: value = out * 2^-scf. Non-finite inputs are outside
 *  the contract: the result is unspecified then, but the call completes.
 *  _act: in [N][C/cblk_f32][H][W][cblk_f32] -> out [N][C/(cblk_i16*lp_blk)][H][W][cblk_i16][lp_blk];
 *  _fil: in [K/kblk_f32][C/cblk_f32][R][S][cblk_f32][kblk_f32] -> out [K/kblk_i16][C/(cblk_i16*lp_blk)][R][S][cblk_i16][kblk_i16][lp_blk].
 *  Checked before any device is asked for, with nothing written and one message per entry point at verbosity != 0: a NULL
 *  operand, an unknown round_mode, C not a multiple of cblk_f32 or of cblk_i16*lp_blk, K not a multiple of kblk_f32 or of
 *  kblk_i16, an odd lp_blk (fil) -- the reference asserts these. length <= 0 or an empty tensor does nothing and leaves
 *  *scf alone.
 *  `scf` is a host byte here, as in the reference: each of these calls therefore waits for the stream once and reads one
 *  byte back. The forms libxsmm_amd_dnn_quantize*_async (libxsmm_amd.h) leave the byte in memory the GPU reaches and do
 *  not wait. libxsmm_dnn_quantize_act with plain input (cblk_f32 == 1) runs a kernel that turns tiles through LDS;
 *  the environment variable LIBXSMM_AMD_QUANT_TILED=0 forces the generic kernel (same bits). */
LIBXSMM_API void libxsmm_dnn_quantize(float* in_buffer, short* out_buffer, int length, unsigned char add_shift, unsigned char* scf, int round_mode);
LIBXSMM_API void libxsmm_dnn_quantize_act(float* in_buffer, short* out_buffer, unsigned int N, unsigned int C, unsigned int H, unsigned int W,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode);
LIBXSMM_API void libxsmm_dnn_quantize_fil(float* in_buffer, short* out_buffer, unsigned int K, unsigned int C, unsigned int R, unsigned int S,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int kblk_f32, unsigned int kblk_i16, unsigned int lp_blk, unsigned char add_shift,
  unsigned char* scf, int round_mode);
/** out = (float)in * libxsmm_sexp2_i8((signed char)(-(int)scf)), one rounding (:419). */
LIBXSMM_API void libxsmm_dnn_dequantize(short* in_buffer, float* out_buffer, int length, unsigned char scf);

/** fp32 <-> bf16 (:423-426): truncation, round to nearest with ties away from zero, round to nearest with ties to even, and
 *  the widening (bits << 16). NaN and Inf are not rounded, only shifted: a NaN whose payload lies in the low 16 bits
 *  becomes Inf, as in the reference. */
LIBXSMM_API void libxsmm_truncate_convert_f32_bf16(const float* in, libxsmm_bfloat16* out, unsigned int length);
LIBXSMM_API void libxsmm_rnaz_convert_fp32_bfp16(const float* in, libxsmm_bfloat16* out, unsigned int len);
LIBXSMM_API void libxsmm_rne_convert_fp32_bfp16(const float* in, libxsmm_bfloat16* out, unsigned int len);
LIBXSMM_API void libxsmm_convert_bf16_f32(const libxsmm_bfloat16* in, float* out, unsigned int length);

#include "libxsmm_dnn_rnncell.h" /* the RNN cell layer (its header includes this one first, as the reference's does) */

#endif /* LIBXSMM_DNN_H */
