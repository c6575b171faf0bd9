/* libxsmm_dnn_tensor.h -- the common part of the reference's DNN interface: error codes, data types, tensor formats,
 * datalayouts and tensor handles that link caller memory (reference: include/libxsmm_dnn.h:47-263 and :359-390,
 * include/libxsmm_typedefs.h:311-346, src/libxsmm_dnn.c:70-189, :330-360, :1000-1570). The reference declares all of this in
 * libxsmm_dnn.h; here libxsmm_dnn.h includes this file, so a caller includes what it always did. Line numbers refer to the
 * reference's include/libxsmm_dnn.h unless a file is named. Where tensor data may live: see libxsmm_dnn.h. */
#ifndef LIBXSMM_DNN_TENSOR_H
#define LIBXSMM_DNN_TENSOR_H

#include "libxsmm.h"

/** Opaque tensor handle (:49) and the status type (:52). */
typedef struct libxsmm_dnn_tensor libxsmm_dnn_tensor;
typedef unsigned int libxsmm_dnn_err_t;

/* error and warning codes (:55-101) */
#define LIBXSMM_DNN_SUCCESS                             0
#define LIBXSMM_DNN_WARN_FALLBACK                   90000
#define LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_N_BLOCKING  90001
#define LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_C_BLOCKING  90002
#define LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_K_BLOCKING  90003
#define LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_N_BLOCKING   90004
#define LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_C_BLOCKING   90005
#define LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_K_BLOCKING   90006
#define LIBXSMM_DNN_ERR_GENERAL                    100000
#define LIBXSMM_DNN_ERR_CREATE_HANDLE              100001
#define LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE       100002
#define LIBXSMM_DNN_ERR_INVALID_BLOCKING           100003
#define LIBXSMM_DNN_ERR_INVALID_HANDLE             100004
#define LIBXSMM_DNN_ERR_DATA_NOT_BOUND             100005
#define LIBXSMM_DNN_ERR_CREATE_TENSOR              100006
#define LIBXSMM_DNN_ERR_INVALID_TENSOR             100007
#define LIBXSMM_DNN_ERR_MISMATCH_TENSOR            100008
#define LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR      100009
#define LIBXSMM_DNN_ERR_INVALID_KIND               100010
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_NCHW        100011
#define LIBXSMM_DNN_ERR_UNSUPPORTED_DST_FORMAT     100012
#define LIBXSMM_DNN_ERR_UNSUPPORTED_SRC_FORMAT     100013
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_CONVOLVE    100014
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_KCRS        100015
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL     100016
#define LIBXSMM_DNN_ERR_CREATE_LAYOUT              100017
#define LIBXSMM_DNN_ERR_INVALID_LAYOUT             100018
#define LIBXSMM_DNN_ERR_UNSUPPORTED_ARCH           100019
#define LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED        100020
#define LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE        100021
#define LIBXSMM_DNN_ERR_INVALID_ALGO               100022
#define LIBXSMM_DNN_ERR_INVALID_PADDING            100023
#define LIBXSMM_DNN_ERR_UNKNOWN_BIAS_TYPE          100024
#define LIBXSMM_DNN_ERR_MISMATCH_BIAS              100025
#define LIBXSMM_DNN_ERR_INVALID_HANDLE_BIAS        100026
#define LIBXSMM_DNN_ERR_TIME_STEPS_TOO_SMALL       100027
#define LIBXSMM_DNN_ERR_CREATE_LAYOUT_ARRAYS       100028
#define LIBXSMM_DNN_ERR_NOT_IMPLEMENTED            100029
#define LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_ORDER   100030
#define LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_FUSION  100031
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_FUSEDBN     100032
#define LIBXSMM_DNN_ERR_UNSUPPORTED_POOLING        100033
#define LIBXSMM_DNN_ERR_INVALID_FORMAT_FC          100034
#define LIBXSMM_DNN_ERR_INVALID_RNN_TYPE           100035
#define LIBXSMM_DNN_ERR_RNN_INVALID_SEQ_LEN        100036

/* include/libxsmm_typedefs.h:311-327 */
typedef enum libxsmm_dnn_tensor_format {
  LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM  = 1,   /* blocked */
  LIBXSMM_DNN_TENSOR_FORMAT_NHWC     = 2,
  LIBXSMM_DNN_TENSOR_FORMAT_NCHW     = 4,
  LIBXSMM_DNN_TENSOR_FORMAT_RSCK     = 8,
  LIBXSMM_DNN_TENSOR_FORMAT_KCRS     = 16,
  LIBXSMM_DNN_TENSOR_FORMAT_CK       = 32,
  LIBXSMM_DNN_TENSOR_FORMAT_CKPACKED = 64,
  LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED = 128,
  LIBXSMM_DNN_TENSOR_FORMAT_NC       = 256
} libxsmm_dnn_tensor_format;

/* include/libxsmm_typedefs.h:329-336 */
typedef enum libxsmm_dnn_internal_format {
  LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1 = 1,  /* NC_bHWc */
  LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_2 = 2,  /* C_bN_bHWnc */
  LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_3 = 3   /* HWN_bC_bnc */
} libxsmm_dnn_internal_format;

/* include/libxsmm_typedefs.h:339-346 */
typedef enum libxsmm_dnn_datatype {
  LIBXSMM_DNN_DATATYPE_F64  = LIBXSMM_DATATYPE_F64,
  LIBXSMM_DNN_DATATYPE_F32  = LIBXSMM_DATATYPE_F32,
  LIBXSMM_DNN_DATATYPE_BF16 = LIBXSMM_DATATYPE_BF16,
  LIBXSMM_DNN_DATATYPE_I32  = LIBXSMM_DATATYPE_I32,
  LIBXSMM_DNN_DATATYPE_I16  = LIBXSMM_DATATYPE_I16,
  LIBXSMM_DNN_DATATYPE_I8   = LIBXSMM_DATATYPE_I8
} libxsmm_dnn_datatype;

/* :104-115 */
typedef enum libxsmm_dnn_compute_kind {
  LIBXSMM_DNN_COMPUTE_KIND_FWD, LIBXSMM_DNN_COMPUTE_KIND_BWD, LIBXSMM_DNN_COMPUTE_KIND_UPD, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD,
  LIBXSMM_DNN_COMPUTE_KIND_ALL
} libxsmm_dnn_compute_kind;

/* :118-137 */
typedef enum libxsmm_dnn_tensor_dimtype {
  LIBXSMM_DNN_TENSOR_DIMTYPE_N, LIBXSMM_DNN_TENSOR_DIMTYPE_H, LIBXSMM_DNN_TENSOR_DIMTYPE_W, LIBXSMM_DNN_TENSOR_DIMTYPE_C,
  LIBXSMM_DNN_TENSOR_DIMTYPE_K, LIBXSMM_DNN_TENSOR_DIMTYPE_R, LIBXSMM_DNN_TENSOR_DIMTYPE_S, LIBXSMM_DNN_TENSOR_DIMTYPE_T,
  LIBXSMM_DNN_TENSOR_DIMTYPE_X
} libxsmm_dnn_tensor_dimtype;

/* :140-251 (the order fixes the values) */
typedef enum libxsmm_dnn_tensor_type {
  LIBXSMM_DNN_REGULAR_INPUT, LIBXSMM_DNN_REGULAR_INPUT_ADD, LIBXSMM_DNN_REGULAR_INPUT_TRANS, LIBXSMM_DNN_GRADIENT_INPUT,
  LIBXSMM_DNN_GRADIENT_INPUT_ADD, LIBXSMM_DNN_REGULAR_OUTPUT, LIBXSMM_DNN_GRADIENT_OUTPUT, LIBXSMM_DNN_INPUT, LIBXSMM_DNN_OUTPUT,
  LIBXSMM_DNN_ACTIVATION, LIBXSMM_DNN_REGULAR_FILTER, LIBXSMM_DNN_REGULAR_FILTER_TRANS, LIBXSMM_DNN_GRADIENT_FILTER, LIBXSMM_DNN_FILTER,
  LIBXSMM_DNN_REGULAR_CHANNEL_BIAS, LIBXSMM_DNN_GRADIENT_CHANNEL_BIAS, LIBXSMM_DNN_CHANNEL_BIAS, LIBXSMM_DNN_REGULAR_CHANNEL_BETA,
  LIBXSMM_DNN_GRADIENT_CHANNEL_BETA, LIBXSMM_DNN_CHANNEL_BETA, LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA, LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA,
  LIBXSMM_DNN_CHANNEL_GAMMA, LIBXSMM_DNN_CHANNEL_EXPECTVAL, LIBXSMM_DNN_CHANNEL_RCPSTDDEV, LIBXSMM_DNN_CHANNEL_VARIANCE,
  LIBXSMM_DNN_CHANNEL_SCALAR, LIBXSMM_DNN_BATCH_STATS, LIBXSMM_DNN_MAX_STATS_FWD, LIBXSMM_DNN_MAX_STATS_BWD, LIBXSMM_DNN_MAX_STATS_UPD,
  LIBXSMM_DNN_POOLING_MASK, LIBXSMM_DNN_TENSOR,
  LIBXSMM_DNN_RNN_REGULAR_INPUT, LIBXSMM_DNN_RNN_REGULAR_CS_PREV, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_REGULAR_WEIGHT,
  LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT, LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT_TRANS,
  LIBXSMM_DNN_RNN_REGULAR_BIAS, LIBXSMM_DNN_RNN_REGULAR_CS, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE, LIBXSMM_DNN_RNN_GRADIENT_INPUT,
  LIBXSMM_DNN_RNN_GRADIENT_CS_PREV, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_GRADIENT_WEIGHT,
  LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT, LIBXSMM_DNN_RNN_GRADIENT_BIAS, LIBXSMM_DNN_RNN_GRADIENT_CS, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE,
  LIBXSMM_DNN_RNN_INTERNAL_I, LIBXSMM_DNN_RNN_INTERNAL_F, LIBXSMM_DNN_RNN_INTERNAL_O, LIBXSMM_DNN_RNN_INTERNAL_CI, LIBXSMM_DNN_RNN_INTERNAL_CO
} libxsmm_dnn_tensor_type;

/** Layout descriptor (:255-263): dimension 0 is the fastest. The arrays belong to the layout (libxsmm_dnn_destroy_tensor_datalayout). */
typedef struct libxsmm_dnn_tensor_datalayout {
  libxsmm_dnn_tensor_dimtype* dim_type;
  unsigned int* dim_size;
  unsigned int num_dims;
  libxsmm_dnn_tensor_format format;
  libxsmm_dnn_internal_format custom_format;
  libxsmm_dnn_datatype datatype;
  libxsmm_dnn_tensor_type tensor_type;
} libxsmm_dnn_tensor_datalayout;

/** Error string and element size (:360-361). */
LIBXSMM_API const char* libxsmm_dnn_get_error(libxsmm_dnn_err_t code);
LIBXSMM_API size_t libxsmm_dnn_typesize(libxsmm_dnn_datatype datatype);

/** Layouts (:370-374). compare returns 0 for equal layouts (tensor_type is not compared), 1 otherwise, 100 for a NULL argument.
 *  The sizes are unsigned int products, as in the reference. None of these touches a device. */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_duplicate_tensor_datalayout(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_tensor_datalayout(libxsmm_dnn_tensor_datalayout* layout);
LIBXSMM_API unsigned int libxsmm_dnn_compare_tensor_datalayout(const libxsmm_dnn_tensor_datalayout* layout_a, const libxsmm_dnn_tensor_datalayout* layout_b, libxsmm_dnn_err_t* status);
LIBXSMM_API unsigned int libxsmm_dnn_get_tensor_size(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status);
LIBXSMM_API unsigned int libxsmm_dnn_get_tensor_elements(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status);

/** Tensors (:377-384): a tensor links memory of the caller's, of any kind (see above), and owns a copy of the layout. None of
 *  these touches a device. libxsmm_dnn_get_tensor_datalayout returns a copy that the caller destroys (it is not part of the
 *  reference's header at the version this interface follows). */
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_link_tensor(const libxsmm_dnn_tensor_datalayout* layout, const void* data, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_link_qtensor(const libxsmm_dnn_tensor_datalayout* layout, const void* data, const unsigned char exp, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_set_tensor_data_ptr(libxsmm_dnn_tensor* tensor, const void* data);
LIBXSMM_API void* libxsmm_dnn_get_tensor_data_ptr(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_get_tensor_datalayout(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status);
LIBXSMM_API unsigned char libxsmm_dnn_get_qtensor_scf(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_set_qtensor_scf(libxsmm_dnn_tensor* tensor, const unsigned char scf);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_tensor(const libxsmm_dnn_tensor* tensor);

/** Zero, copy-in from and copy-out to a plain format (:384-390). Served: blocked (_FORMAT_LIBXSMM) tensors of fp32 or bf16 --
 *  activations (tensor_type input / output kinds, custom format 1) from / to LIBXSMM_DNN_TENSOR_FORMAT_NCHW, filters (custom
 *  format 1) from / to _KCRS, and the thirteen channel tensor types (bias, beta, gamma, expectval, rcpstddev, variance, scalar)
 *  from / to _NCHW (the reference's rule for them): the same order on both sides. Checked in this order, with the reference's
 *  statuses: another tensor type _ERR_INVALID_TENSOR, another plain format _ERR_UNSUPPORTED_SRC_FORMAT (in) / _DST_FORMAT
 *  (out), a tensor that is not blocked _ERR_UNSUPPORTED_DST_FORMAT (in) / _SRC_FORMAT (out), another data type (the integer
 *  types: no layer here creates such layouts) _ERR_UNSUPPORTED_DATATYPE; then custom format 2 _ERR_NOT_IMPLEMENTED, a wrong
 *  number of dimensions _ERR_INVALID_LAYOUT, NULL data _ERR_INVALID_TENSOR. An empty tensor is a success and nothing is
 *  launched. Operands that overlap are undefined, as in the reference.
 *  Where both the tensor and the plain buffer are memory the CPU addresses (pageable, pinned, managed), or there is no device,
 *  the copy is a host loop (the calling thread's stream is waited for first if the GPU may still be writing an operand) and
 *  nothing is launched. Where at least one of them is plain device memory, the permutation is one kernel on the calling thread's
 *  stream (libxsmm_amd_set_stream): an operand in pageable memory is staged through library scratch, pinned or managed memory is
 *  read or written in place, nothing waits before the launch (stream order carries the dependence on earlier work), and the
 *  call waits at its end: it is complete on return. libxsmm_amd_dnn_copyin_tensor_async / _copyout_tensor_async
 *  (libxsmm_amd.h) are the forms without that wait. Inside libxsmm_amd_defer_begin/end the calls are not recorded: they seal
 *  the open burst and run in call order. */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_zero_tensor(const libxsmm_dnn_tensor* tensor);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_copyin_tensor(const libxsmm_dnn_tensor* tensor, const void* data, const libxsmm_dnn_tensor_format in_format);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_copyout_tensor(const libxsmm_dnn_tensor* tensor, void* data, const libxsmm_dnn_tensor_format out_format);

#endif /* LIBXSMM_DNN_TENSOR_H */
