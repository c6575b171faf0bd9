/* libxsmm_dnn_fusedbatchnorm.h -- the fused batch-norm layer of the reference's DNN interface on the GPU (reference:
 * include/libxsmm_dnn_fusedbatchnorm.h:37-51, include/libxsmm_typedefs.h:373-410, src/libxsmm_dnn_fusedbatchnorm.c,
 * src/libxsmm_dnn_fusedbatchnorm_{forward,backward}.c and src/template/libxsmm_dnn_fusedbatchnorm_st_{fwd,bwd}_custom_generic.tpl.c).
 * Line numbers below refer to the reference's header unless a file is named.
 *
 * Arithmetic: bit for bit what the reference's generic templates return (the reference run with LIBXSMM_TARGET=hsw). Tensors are
 * blocked, [N][C/16][rows][columns][16]; an item is one (image, channel block) plane. nhw = (float)(N*H*W), recp_nhw = 1.0f/nhw;
 * the output plane is (H/u) x (W/v). Every multiply and every add is its own rounding (nothing is fused), in fp32.
 *   FWD, OPS_BN       per item and channel lane sum += x and sumsq += x*x from +0.0f over EVERY pixel of the unpadded input,
 *                     hi ascending, then wi ascending (the stride plays no part); per channel the per-image sums are added from
 *                     +0.0f with img ascending; mean = recp_nhw*sum, var = recp_nhw*sumsq - mean*mean,
 *                     rstd = (float)(1.0/sqrt((double)var + (double)1e-7f)) -- add, sqrt and divide in double precision. mean,
 *                     rstd and var are written to the EXPECTVAL, RCPSTDDEV and VARIANCE tensors.
 *   FWD, OPS_BNSCALE  no statistics: the bound EXPECTVAL and RCPSTDDEV are read.
 *   FWD, both         on the strided pixels only (hi += u, wi += v, ho++, wo++): o = gamma*(x-mean)*rstd + beta, left to right;
 *                     ELTWISE: o += add[hi][wi]; RELU: o = (o < 0.0f) ? 0.0f : o (a NaN and a -0.0 pass unchanged).
 *   BWD, OPS_BN       first walk over the strided pixels: RELU: dout = (out == 0) ? 0 : dout, written back into the doutput
 *                     tensor (a -0.0 output counts as zero); ELTWISE: dinput_add[hi][wi] = dout; per item and lane
 *                     dgamma_img += (x-mean)*dout*rstd and dbeta_img += dout from +0.0f; then per channel the per-image values
 *                     are added from +0.0f with img ascending into GRADIENT_CHANNEL_GAMMA and _BETA.
 *   BWD, OPS_BNSCALE  none of the first walk happens, its RELU and ELTWISE side effects included (they sit inside the reference's
 *                     OPS_BN branch); the bound dgamma and dbeta are read as they are.
 *   BWD, both         on the strided pixels: din = gamma*rstd*recp_nhw*(nhw*dout - (dbeta + (x-mean)*dgamma*rstd)), left to right.
 *                     Input pixels the stride skips are not written.
 *   BF16              widened by a shift, computed in fp32, stored by truncation (the upper 16 bits). Statistics are fp32.
 * Physical padding is never written, and that of a tensor that is read is never read.
 *
 * Handles. libxsmm_dnn_create_fusedbatchnorm follows src/libxsmm_dnn_fusedbatchnorm.c:45-89 and never touches a device:
 * datatypes in/out F32/F32 or BF16/BF16, anything else _ERR_UNSUPPORTED_DATATYPE and NULL. The channel blocks are those of
 * libxsmm_dnn_get_feature_map_blocks(C, C), quirks included (C < 16: a block of C in F32; a C that is no multiple of 16 silently
 * loses the remainder). Layouts (:108-314 there): activations have five dimensions in F32 (16, W, H, C/16, N) and six in BF16
 * (2, 8, W, H, C/16, N), the output side with H/u and W/v plus pad_*_out; format NHWC has four; the seven channel tensor types
 * (REGULAR / GRADIENT / plain CHANNEL_BETA and _GAMMA, CHANNEL_EXPECTVAL, _RCPSTDDEV, _VARIANCE) are (16, C/16) of
 * desc.datatype_stats with tensor_type CHANNEL_SCALAR (NHWC: one dimension C); a datatype_stats other than F32 gives
 * _ERR_UNSUPPORTED_DATATYPE, an unknown tensor type _ERR_UNKNOWN_TENSOR_TYPE, other formats _ERR_INVALID_FORMAT_GENERAL.
 * Scratch: 4*2*C*N + 64 bytes, aligned to 64 by bind_scratch; NULL gives _ERR_SCRATCH_NOT_ALLOCED.
 *
 * execute_st checks, in this order: NULL handle (_ERR_INVALID_HANDLE); kind other than FWD / BWD (_ERR_INVALID_KIND);
 * buffer_format other than exactly _LIBXSMM (_ERR_INVALID_FORMAT_FUSEDBN); bound tensors (_ERR_DATA_NOT_BOUND) -- FWD: regular
 * input and output, beta, gamma, EXPECTVAL, RCPSTDDEV and VARIANCE (with BNSCALE too), with ELTWISE the regular input_add; BWD:
 * regular input, gamma, gradient input and output, gradient beta and gamma, EXPECTVAL, RCPSTDDEV, with ELTWISE the gradient
 * input_add, with RELU the regular output; fuse_order other than BN_ELTWISE_RELU (_ERR_FUSEBN_UNSUPPORTED_ORDER); fuse_ops not
 * one of the eight combinations (_ERR_FUSEBN_UNSUPPORTED_FUSION). Then what is this engine's own:
 *   1. The caller's scratch is never read or written and execute_st does not ask for it (the reference answers
 *      _ERR_DATA_NOT_BOUND for OPS_BN without one); it may be host memory. The per-image partial sums live in device memory the
 *      handle owns, allocated at the first execute_st and freed by destroy.
 *   2. tid - start_thread < 0 returns _ERR_GENERAL (the reference indexes out of bounds). A logical thread >= desc.threads or
 *      one with an empty share returns _SUCCESS and launches nothing.
 *   3. _ERR_GENERAL answers: a handle whose channel block is not 16 (C < 16); non-positive N, H, W, u or v; negative padding;
 *      H % u != 0 or W % v != 0 (the reference then walks one output row or column past its H/u, W/v and writes outside the
 *      tensor); a plane of 2^27 pixels or more; a device tensor that is not 16-byte aligned.
 *   4. Threads: no barrier and no co-operation between calls (the reference's execute_st contains barriers: all desc.threads
 *      callers must be inside it together). The call of logical thread ltid = tid - start_thread owns the items
 *      [ltid*chunk, min((ltid+1)*chunk, N*C/16)), chunk = ceil(N*(C/16) / desc.threads), the reference's split. It computes, for
 *      the channel blocks its items touch, the COMPLETE statistics over all N images (in BWD the complete dgamma / dbeta
 *      reduction with its in-place side effects on doutput and dinput_add), in its own region of the partials buffer, and then
 *      applies the normalisation to its own items. Any subset of the threads, in any order and on any streams, therefore
 *      yields the bits of threads = 1; concurrent calls store identical bits to the shared channel tensors. threads = 1 is the
 *      whole pass and the fast way: threads > 1 repeats the statistics work of a channel block in every call that touches it.
 *   5. Memory: as for the fully-connected and pooling layers -- tensors the GPU reaches are processed in place and the call
 *      does not wait; a host-visible tensor makes the call complete on return; pageable host memory is staged, and a staged
 *      tensor a pass writes travels back: output and the three statistics tensors in FWD; dinput, dgamma, dbeta, doutput (with
 *      RELU) and dinput_add in BWD.
 * One call is at most three kernel launches (partial sums, finish, apply) on the calling thread's stream; BNSCALE is one. */
#ifndef LIBXSMM_DNN_FUSEDBATCHNORM_H
#define LIBXSMM_DNN_FUSEDBATCHNORM_H

#include "libxsmm_dnn.h"

/** Opaque handle (the reference's include/libxsmm_dnn.h:51). */
typedef struct libxsmm_dnn_fusedbatchnorm libxsmm_dnn_fusedbatchnorm;

typedef enum libxsmm_dnn_fusedbatchnorm_fuse_order { /* include/libxsmm_typedefs.h:373-376 */
  /* the fuse order is: 1. BN, 2. element-wise 3. RELU */
  LIBXSMM_DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU = 0
} libxsmm_dnn_fusedbatchnorm_fuse_order;

typedef enum libxsmm_dnn_fusedbatchnorm_fuse_op { /* include/libxsmm_typedefs.h:378-390 */
  LIBXSMM_DNN_FUSEDBN_OPS_BN = 1,
  LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE = 2,
  LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE = 4,
  LIBXSMM_DNN_FUSEDBN_OPS_RELU = 8,
  LIBXSMM_DNN_FUSEDBN_OPS_BN_ELTWISE = LIBXSMM_DNN_FUSEDBN_OPS_BN | LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE,
  LIBXSMM_DNN_FUSEDBN_OPS_BN_RELU = LIBXSMM_DNN_FUSEDBN_OPS_BN | LIBXSMM_DNN_FUSEDBN_OPS_RELU,
  LIBXSMM_DNN_FUSEDBN_OPS_BN_ELTWISE_RELU = LIBXSMM_DNN_FUSEDBN_OPS_BN | LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE | LIBXSMM_DNN_FUSEDBN_OPS_RELU,
  LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_ELTWISE = LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE | LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE,
  LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_RELU = LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE | LIBXSMM_DNN_FUSEDBN_OPS_RELU,
  LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_ELTWISE_RELU = LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE | LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE | LIBXSMM_DNN_FUSEDBN_OPS_RELU
} libxsmm_dnn_fusedbatchnorm_fuse_op;

typedef struct libxsmm_dnn_fusedbatchnorm_desc { /* include/libxsmm_typedefs.h:392-410 */
  int N;                                     /* number of images in mini-batch */
  int C;                                     /* number of feature maps */
  int H;                                     /* height of the input image */
  int W;                                     /* width of the input image */
  int u;                                     /* vertical stride */
  int v;                                     /* horizontal stride */
  int pad_h_in;                              /* physical padding of the input buffer, rows */
  int pad_w_in;                              /* physical padding of the input buffer, columns */
  int pad_h_out;                             /* physical padding of the output buffer, rows */
  int pad_w_out;                             /* physical padding of the output buffer, columns */
  int threads;                               /* number of logical threads the passes are split into */
  libxsmm_dnn_datatype datatype_in;          /* datatype of all input related buffers */
  libxsmm_dnn_datatype datatype_out;         /* datatype of all output related buffers */
  libxsmm_dnn_datatype datatype_stats;       /* datatype of all statistics related buffers */
  libxsmm_dnn_tensor_format buffer_format;   /* format of the activation buffers */
  libxsmm_dnn_fusedbatchnorm_fuse_order fuse_order; /* the order of the fused operations */
  libxsmm_dnn_fusedbatchnorm_fuse_op fuse_ops;      /* the fused operations */
} libxsmm_dnn_fusedbatchnorm_desc;

/* :37-38 */
LIBXSMM_API libxsmm_dnn_fusedbatchnorm* libxsmm_dnn_create_fusedbatchnorm(libxsmm_dnn_fusedbatchnorm_desc fusedbatchnorm_desc, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_fusedbatchnorm(const libxsmm_dnn_fusedbatchnorm* handle);

/* :40 -- type: LIBXSMM_DNN_{REGULAR,GRADIENT}_{INPUT,INPUT_ADD,OUTPUT}, the general _INPUT / _OUTPUT, or one of the channel types */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(const libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);

/* :42-44 */
LIBXSMM_API size_t libxsmm_dnn_fusedbatchnorm_get_scratch_size(const libxsmm_dnn_fusedbatchnorm* handle, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_scratch(libxsmm_dnn_fusedbatchnorm* handle, const void* scratch);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_scratch(libxsmm_dnn_fusedbatchnorm* handle);

/* :46-48 -- thirteen bindable types: regular and gradient input, output and input_add; regular and gradient channel beta and
 * gamma; CHANNEL_EXPECTVAL, _RCPSTDDEV and _VARIANCE. The tensor type is checked first (_ERR_UNKNOWN_TENSOR_TYPE), then NULL
 * arguments (_ERR_INVALID_HANDLE_TENSOR for bind); a tensor whose layout differs from the handle's is not bound:
 * _ERR_MISMATCH_TENSOR */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_fusedbatchnorm_get_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type);

/* :50-51 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_execute_st(libxsmm_dnn_fusedbatchnorm* handle, libxsmm_dnn_compute_kind kind,
  /*unsigned*/int start_thread, /*unsigned*/int tid);

#endif /* LIBXSMM_DNN_FUSEDBATCHNORM_H */
