/* libxsmm_dnn_fullyconnected.h -- the fully-connected layer of the reference's DNN interface on the GPU (reference:
 * include/libxsmm_dnn_fullyconnected.h:37-74, src/libxsmm_dnn_fullyconnected.c, src/libxsmm_dnn_fullyconnected_{forward,
 * backward,weight_update}.c and their templates). Line numbers below refer to the reference's header unless a file is named.
 *
 * Arithmetic (w filter, x input, y output, d. gradients). Every output element is one fp32 fused multiply-add chain over the
 * whole reduction dimension in ascending order, started from +0.0; the destination is never read:
 *   FWD  y[n][k]  = chain over c of w[k][c] * x[n][c]
 *   BWD  dx[n][c] = chain over k of w[k][c] * dy[n][k]
 *   UPD  dw[k][c] = chain over n of dy[n][k] * x[n][c]
 * That is what the reference's SMM and batch-reduce SMM kernels compute per block (beta = 0), so block sizes, thread counts
 * and the storage format do not enter the bits. With datatype_in = BF16 and datatype_out = F32 the 16-bit operands (x, w) are
 * widened exactly (bits << 16) on their way into the kernel, y and dy are fp32, and dx and dw are bf16: the fp32 chain
 * rounded once to nearest even by the rule of libxsmm_rne_convert_fp32_bfp16 (NaN and Inf are only shifted).
 *
 * Handles. libxsmm_dnn_create_fullyconnected follows src/libxsmm_dnn_fullyconnected.c:46-136 and never touches a device:
 *   datatypes in/out: F32/F32, BF16/F32, BF16/BF16; anything else: _ERR_UNSUPPORTED_DATATYPE and NULL. A BF16/BF16 handle is
 *   created as in the reference, but it has no activation layouts and every execute_st on it returns _ERR_UNSUPPORTED_DATATYPE.
 *   buffer_format = _NCPACKED and filter_format = _CKPACKED: blocks bn, bc, bk from the desc; a block that does not divide its
 *   dimension becomes the whole dimension and the status is _WARN_FC_SUBOPTIMAL_{N,C,K}_BLOCKING (the last one that applies).
 *   input [N/bn][C/bc][bn][bc], output [N/bn][K/bk][bn][bk], filter [K/bk][C/bc][bc][bk]; executed for F32/F32 only.
 *   otherwise (buffer_format = filter_format = _LIBXSMM is what execute_st accepts): C % 16 == 0 and K % 16 == 0 gives blocks of
 *   16 and 16; C % 16 == 0 and K == 1000 gives 16 and 10; anything else _ERR_CREATE_HANDLE and NULL.
 *   activations [N][C/16][16], filter [K/ofmb][C/16][16][ofmb]; layouts as create_tensor_datalayout builds them (:155-492 of the .c).
 * execute_st returns _ERR_DATA_NOT_BOUND if a tensor of the pass is not bound, _ERR_FUSEBN_UNSUPPORTED_FUSION for fuse_ops other
 * than NONE, _ERR_INVALID_FORMAT_FC for another pair of formats (NHWC / RSCK among them: the reference's nhwc path is "not
 * implemented" and never reached), _ERR_INVALID_KIND for a kind other than FWD / BWD / UPD, _ERR_INVALID_HANDLE for NULL, and
 * _ERR_GENERAL if no device is usable or a launch fails.
 *
 * Threads. execute_st(handle, kind, start_thread, tid) computes the share of logical thread ltid = tid - start_thread by the
 * reference's split: chunksize = ceil(work / desc.threads), blocks [ltid * chunksize, min((ltid + 1) * chunksize, work)), where
 * work counts blocks of the output -- format LIBXSMM: K/ofmb (FWD), C/ifmb (BWD), (K/ofmb) * (C/ifmb) (UPD, filter blocks in
 * memory order); format NCPACKED: (N/bn) * (K/bk) (FWD), (N/bn) * (C/bc) (BWD), both in memory order of the output, and
 * (K/bk) * (C/bc) (UPD). Each call is ONE kernel launch on the calling thread's stream (libxsmm_amd_set_stream). There is no
 * barrier and nothing is shared between shares: the calls of different threads may run concurrently (on tensors the GPU
 * reaches), and the bits do not depend on desc.threads. ltid >= desc.threads, or a share without blocks, does nothing and
 * returns _SUCCESS; a negative ltid (the reference would index out of bounds) does nothing and returns _ERR_GENERAL.
 * desc.threads = 1 is the whole pass in one launch: the fast way.
 *
 * Memory. Tensors the GPU reaches (device, pinned, managed) are processed in place and the call does not wait; a host-visible
 * tensor (pinned, managed) makes the call complete on return; a tensor in pageable host memory is staged through device
 * scratch (its image travels to the device, the destination's image travels back whole) and the call is complete on return --
 * so shares of one pass that write a pageable destination must not run concurrently. Inside libxsmm_amd_defer_begin/end
 * the calls are not recorded: they seal the open burst and run in call order.
 *
 * Scratch. get_scratch_size returns the reference's formula (:122-127 of the .c, plus 64), bind_scratch and release_scratch
 * keep its statuses (NULL: _ERR_SCRATCH_NOT_ALLOCED), so an unchanged caller allocates and binds what it always did. The
 * engine never reads or writes the scratch: nothing is transposed or widened through memory (kernels/fc.hip addresses the
 * blocked operands where they lie). BWD and UPD still return _ERR_DATA_NOT_BOUND while no scratch is bound, as the reference
 * does; FWD does not ask for it.
 *
 * LIBXSMM_AMD_FC_TILE=64 or 128 forces the work-group tile (same bits); otherwise the largest tile that still gives every
 * compute unit a work-group is taken. */
#ifndef LIBXSMM_DNN_FULLYCONNECTED_H
#define LIBXSMM_DNN_FULLYCONNECTED_H

#include "libxsmm_dnn.h"

/** Opaque handle (:38). */
typedef struct libxsmm_dnn_fullyconnected libxsmm_dnn_fullyconnected;

typedef enum libxsmm_dnn_fullyconnected_fuse_op { /* :40-43 */
  LIBXSMM_DNN_FULLYCONNECTED_FUSE_NONE = 0
} libxsmm_dnn_fullyconnected_fuse_op;

typedef struct libxsmm_dnn_fullyconnected_desc { /* :45-58 */
  int N;                                        /* number of images in mini-batch */
  int C;                                        /* number of input feature maps */
  int K;                                        /* number of output feature maps */
  int bn;
  int bk;
  int bc;
  int threads;                                  /* number of logical threads the passes are split into */
  libxsmm_dnn_datatype datatype_in;             /* datatype of all input related buffers */
  libxsmm_dnn_datatype datatype_out;            /* datatype of all output related buffers */
  libxsmm_dnn_tensor_format buffer_format;      /* format of the activation buffers */
  libxsmm_dnn_tensor_format filter_format;      /* format of the filter buffers */
  libxsmm_dnn_fullyconnected_fuse_op fuse_ops;  /* fused operations */
} libxsmm_dnn_fullyconnected_desc;

/* :60-61 */
LIBXSMM_API libxsmm_dnn_fullyconnected* libxsmm_dnn_create_fullyconnected(libxsmm_dnn_fullyconnected_desc fullyconnected_desc, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_fullyconnected(const libxsmm_dnn_fullyconnected* handle);

/* :63 -- type: LIBXSMM_DNN_{REGULAR,GRADIENT}_{INPUT,OUTPUT,FILTER} or the general _INPUT / _OUTPUT / _FILTER */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_fullyconnected_create_tensor_datalayout(const libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);

/* :65-67 */
LIBXSMM_API size_t libxsmm_dnn_fullyconnected_get_scratch_size(const libxsmm_dnn_fullyconnected* handle, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_bind_scratch(libxsmm_dnn_fullyconnected* handle, const void* scratch);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_release_scratch(libxsmm_dnn_fullyconnected* handle);

/* :69-71 -- a tensor whose layout differs from the handle's (libxsmm_dnn_compare_tensor_datalayout) is not bound: _ERR_MISMATCH_TENSOR */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_bind_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_fullyconnected_get_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_release_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor_type type);

/* :73-74 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_execute_st(libxsmm_dnn_fullyconnected* handle, libxsmm_dnn_compute_kind kind,
  /*unsigned*/int start_thread, /*unsigned*/int tid);

#endif /* LIBXSMM_DNN_FULLYCONNECTED_H */
