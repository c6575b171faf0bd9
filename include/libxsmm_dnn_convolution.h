/* libxsmm_dnn_convolution.h -- the convolution layer of the reference's DNN interface on the GPU (reference:
 * include/libxsmm_dnn.h:265-329 and :364-412, include/libxsmm_typedefs.h:348-371, src/libxsmm_dnn.c, src/libxsmm_dnn_handle.c:61-150,
 * libxsmm_dnn_setup_generic in src/libxsmm_dnn_setup.c:369-465, src/libxsmm_dnn_convolution_{forward,backward,weight_update}.c and
 * src/template/libxsmm_dnn_convolve_st_{fwd,bwd,upd}_custom_custom_generic.tpl.c). The reference declares all of this in
 * libxsmm_dnn.h; here libxsmm_dnn.h includes this file, so a caller includes what it always did. Line numbers refer to the
 * reference's include/libxsmm_dnn.h unless a file is named. DESIGN.md 8n.
 *
 * Arithmetic: bit for bit what the reference's generic path returns (the reference run with LIBXSMM_TARGET=hsw: its generic
 * templates over AVX2 SMM kernels; the AVX-512 kernel streams are not the contract). Only F32 / F32 computes there, and here.
 *   Blocks   ifmblock = C if C < 16, else the largest power of two up to 16 that divides C; ofmblock likewise for K.
 *   Layouts  activations [N][blocks][rows + 2 pad][columns + 2 pad][block] (five dimensions), filter
 *            [K/ofmblock][C/ifmblock][R][S][ifmblock][ofmblock] (six), REGULAR_FILTER_TRANS
 *            [C/ifmblock][K/ofmblock][R][S][ofmblock][ifmblock] (six), channel bias [K/ofmblock][ofmblock] (two).
 *            ofh = (H + 2 pad_h - R)/u + 1, ifhp = H + 2 pad_h_in, ofhp = ofh + 2 pad_h_out; columns likewise.
 *   FWD      every output element is one chain acc = fmaf(w, x, acc) over ifm1, kj, ki, ifm2, all ascending. It starts from the
 *            bias with _FUSE_BIAS, otherwise from +0.0 with _OPTION_OVERWRITE, otherwise from the value the output holds.
 *            Physical padding (pad_h == pad_h_in and pad_w == pad_w_in): the rim of the input buffer is read as it is. Logical
 *            padding (pad_*_in == 0): the rim terms are products with +0.0 and they are computed (a filter Inf next to the border
 *            gives NaN). Then o = (o < 0) ? 0 : o if fuse_ops & _FUSE_RELU (6: _FUSE_RELU_BWD alone switches it on too); NaN and
 *            -0.0 pass. Output padding is never written.
 *   BWD      every dinput element is one chain over the terms the reference visits: ofm1 ascending, oj ascending (kj descending),
 *            ki ascending, ofm2 ascending; a position whose oj or oi lies outside the output adds no term. It starts from +0.0
 *            with _OPTION_OVERWRITE (an element no term reaches is then +0.0), otherwise from the present value. Physical padding:
 *            the rim of dinput is set to +0.0. Logical padding: only the H x W interior is written. Every fuse bit is ignored.
 *            With _OPTION_BWD_NO_FILTER_TRANSPOSE the filter is read from REGULAR_FILTER_TRANS (libxsmm_dnn_trans_reg_filter).
 *   UPD      if u == v == 1, or R == S == 1 with physical (or no) padding: every dfilter element is one chain over img, oj, oi
 *            ascending, from +0.0 with _OPTION_OVERWRITE, else from the present value; the input of term (oj, oi) is
 *            x[(oj + kj) u][(oi + ki) v] if oj + kj < ifhp/u and oi + ki < ifwp/v, else +0.0 (the reference's transposed copy;
 *            with logical padding the zero rim). Otherwise: per image a chain from +0.0 over oj, oi, then one rounded add of it
 *            into dfilter, images ascending.
 *
 * Kept from the reference: the order of create's checks (_ERR_INVALID_FORMAT_NCHW, _ERR_INVALID_FORMAT_KCRS -- tested on
 * buffer_format, as there --, _ERR_INVALID_ALGO), the layouts, _ERR_UNKNOWN_TENSOR_TYPE, the scratch sizes per kind,
 * _ERR_SCRATCH_NOT_ALLOCED, _ERR_MISMATCH_TENSOR, _ERR_DATA_NOT_BOUND per pass (BWD asks for a scratch bound with kind BWD or
 * ALL, UPD for one bound with UPD or ALL; FWD does not ask for the bias), _ERR_INVALID_KIND, _ERR_INVALID_HANDLE.
 *
 * This engine's own:
 *   - The caller's scratch is never read or written; it may be host memory.
 *   - create answers NULL with _ERR_UNSUPPORTED_DATATYPE for anything but F32 / F32; with _ERR_INVALID_FORMAT_CONVOLVE for a
 *     buffer_format other than _LIBXSMM or a filter_format other than _LIBXSMM (the reference runs NHWC / RSCK); with
 *     _ERR_INVALID_PADDING unless (pad_h_in, pad_w_in) is (pad_h, pad_w) or (0, 0) (the reference then reads the input without
 *     its offset); with _ERR_FUSEBN_UNSUPPORTED_FUSION for fuse bits other than _FUSE_BIAS, _FUSE_RELU_FWD, _FUSE_RELU_BWD or a
 *     non-NULL pre_bn / post_bn (the reference's generic path ignores them); with _ERR_GENERAL for a non-positive N, C, H, W, K,
 *     R, S, u, v or threads, a negative padding, ofh or ofw below 1, or a tensor of 2^31 elements or more. All of these come
 *     before any device is asked for.
 *   - The environment variable LIBXSMM_DNN_INTERNAL_FORMAT is not read: the format is custom format 1 always.
 *   - The layouts of _BATCH_STATS and _MAX_STATS_* do not exist: _ERR_UNKNOWN_TENSOR_TYPE (nothing here would use them).
 *   - tid - start_thread < 0 returns _ERR_GENERAL; a logical thread >= desc.threads, or one whose share is empty, returns
 *     _SUCCESS without a launch. FWD with _FUSE_BIAS and no bias bound, and BWD with _OPTION_BWD_NO_FILTER_TRANSPOSE and no
 *     REGULAR_FILTER_TRANS bound, return _ERR_DATA_NOT_BOUND (the reference dereferences NULL).
 *
 * Threads. Work is N * K/ofmblock items (FWD), N * C/ifmblock (BWD), C/ifmblock * K/ofmblock (UPD), split as in the other layers:
 * logical thread ltid computes [ltid * chunk, min((ltid + 1) * chunk, work)), chunk = ceil(work / desc.threads). No chain crosses a
 * share and there is no barrier: any subset of the threads, in any order and on any streams, gives the bits of threads = 1, which
 * is the fast way. libxsmm_dnn_execute runs all logical threads in turn on the calling thread's stream.
 *
 * Memory: as for the fully-connected layer (libxsmm_dnn_fullyconnected.h) -- tensors the GPU reaches are processed in place and
 * the call does not wait; a host-visible tensor makes the call complete on return; pageable host memory is staged. */
#ifndef LIBXSMM_DNN_CONVOLUTION_H
#define LIBXSMM_DNN_CONVOLUTION_H

#include "libxsmm_dnn_tensor.h"

/** Opaque handle (:48). */
typedef struct libxsmm_dnn_layer libxsmm_dnn_layer;

typedef enum libxsmm_dnn_conv_fuse_op { /* :265-287 */
  LIBXSMM_DNN_CONV_FUSE_NONE = 0,
  LIBXSMM_DNN_CONV_FUSE_BIAS = 1,
  LIBXSMM_DNN_CONV_FUSE_RELU_FWD = 2,
  LIBXSMM_DNN_CONV_FUSE_RELU_BWD = 4,
  LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD = 8,
  LIBXSMM_DNN_CONV_FUSE_MAX_STATS = 16,
  LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_BWD = 32,
  LIBXSMM_DNN_CONV_FUSE_ELTWISE_BWD = 64,
  LIBXSMM_DNN_CONV_FUSE_BATCHNORM_STATS = 128,
  LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD_RELU_BWD = LIBXSMM_DNN_CONV_FUSE_RELU_BWD | LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD,
  LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD_RELU_BWD_AND_MAX = LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD_RELU_BWD | LIBXSMM_DNN_CONV_FUSE_MAX_STATS,
  LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD_AND_MAX = LIBXSMM_DNN_CONV_FUSE_BATCH_STATS_FWD | LIBXSMM_DNN_CONV_FUSE_MAX_STATS,
  LIBXSMM_DNN_CONV_FUSE_RELU_BWD_AND_MAX = LIBXSMM_DNN_CONV_FUSE_RELU_BWD | LIBXSMM_DNN_CONV_FUSE_MAX_STATS,
  LIBXSMM_DNN_CONV_FUSE_RELU = LIBXSMM_DNN_CONV_FUSE_RELU_FWD | LIBXSMM_DNN_CONV_FUSE_RELU_BWD,
  LIBXSMM_DNN_CONV_FUSE_BIAS_RELU = LIBXSMM_DNN_CONV_FUSE_BIAS | LIBXSMM_DNN_CONV_FUSE_RELU
} libxsmm_dnn_conv_fuse_op;

typedef enum libxsmm_dnn_conv_algo { /* :290-295 */
  LIBXSMM_DNN_CONV_ALGO_AUTO,
  LIBXSMM_DNN_CONV_ALGO_DIRECT
} libxsmm_dnn_conv_algo;

typedef enum libxsmm_dnn_conv_option { /* include/libxsmm_typedefs.h:348-371 */
  LIBXSMM_DNN_CONV_OPTION_NONE = 0,
  LIBXSMM_DNN_CONV_OPTION_OVERWRITE = 1,
  LIBXSMM_DNN_CONV_OPTION_ACTIVATION_UNSIGNED = 2,
  LIBXSMM_DNN_CONV_OPTION_UPD_NO_FILTER_REDUCE = 4,
  LIBXSMM_DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE = 8,
  LIBXSMM_DNN_CONV_OPTION_UPD_NO_INPUT_TRANSPOSE = 16,
  LIBXSMM_DNN_CONV_OPTION_F32_BF16_CVT_RNE = 32,
  LIBXSMM_DNN_CONV_OPTION_F32_BF16_CVT_RNE_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_OVERWRITE | LIBXSMM_DNN_CONV_OPTION_F32_BF16_CVT_RNE,
  LIBXSMM_DNN_CONV_OPTION_ACTIVATION_UNSIGNED_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_ACTIVATION_UNSIGNED | LIBXSMM_DNN_CONV_OPTION_OVERWRITE,
  LIBXSMM_DNN_CONV_OPTION_UPD_NO_FILTER_REDUCE_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_UPD_NO_FILTER_REDUCE | LIBXSMM_DNN_CONV_OPTION_OVERWRITE,
  LIBXSMM_DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_OVERWRITE | LIBXSMM_DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE,
  LIBXSMM_DNN_CONV_OPTION_UPD_NO_INPUT_TRANSPOSE_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_OVERWRITE | LIBXSMM_DNN_CONV_OPTION_UPD_NO_INPUT_TRANSPOSE,
  LIBXSMM_DNN_CONV_OPTION_NO_TRANSPOSES_OVERWRITE = LIBXSMM_DNN_CONV_OPTION_OVERWRITE | LIBXSMM_DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE | LIBXSMM_DNN_CONV_OPTION_UPD_NO_INPUT_TRANSPOSE
} libxsmm_dnn_conv_option;

typedef struct libxsmm_dnn_conv_desc { /* :298-329 */
  int N;                                    /* number of images in mini-batch */
  int C;                                    /* number of input feature maps */
  int H;                                    /* height of input image */
  int W;                                    /* width of input image */
  int K;                                    /* number of output feature maps */
  int R;                                    /* height of filter kernel */
  int S;                                    /* width of filter kernel */
  int u;                                    /* vertical stride */
  int v;                                    /* horizontal stride */
  int pad_h;                                /* logical padding of the input, rows */
  int pad_w;                                /* logical padding of the input, columns */
  int pad_h_in;                             /* physical padding of the input buffer, rows: pad_h or 0 */
  int pad_w_in;                             /* physical padding of the input buffer, columns: pad_w or 0 */
  int pad_h_out;                            /* physical padding of the output buffer, rows */
  int pad_w_out;                            /* physical padding of the output buffer, columns */
  int threads;                              /* number of logical threads the passes are split into */
  libxsmm_dnn_datatype datatype_in;         /* datatype of all input related buffers */
  libxsmm_dnn_datatype datatype_out;        /* datatype of all output related buffers */
  libxsmm_dnn_tensor_format buffer_format;  /* format of the activation buffers */
  libxsmm_dnn_tensor_format filter_format;  /* format of the filter buffers */
  libxsmm_dnn_conv_algo algo;               /* convolution algorithm */
  libxsmm_dnn_conv_option options;          /* additional options */
  libxsmm_dnn_conv_fuse_op fuse_ops;        /* operations fused into the convolution */
  struct libxsmm_dnn_fusedbatchnorm* pre_bn;  /* must be NULL */
  struct libxsmm_dnn_fusedbatchnorm* post_bn; /* must be NULL */
} libxsmm_dnn_conv_desc;

/* :365-366 */
LIBXSMM_API libxsmm_dnn_layer* libxsmm_dnn_create_conv_layer(libxsmm_dnn_conv_desc conv_desc, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_conv_layer(const libxsmm_dnn_layer* handle);

/* :369 -- type: LIBXSMM_DNN_{REGULAR,GRADIENT}_{INPUT,OUTPUT,FILTER,CHANNEL_BIAS}, the general _INPUT / _OUTPUT / _FILTER /
 * _CHANNEL_BIAS, or LIBXSMM_DNN_REGULAR_FILTER_TRANS */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_create_tensor_datalayout(const libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);

/* :391 -- REGULAR_FILTER_TRANS[ifm1][ofm1][R-1-kj][S-1-ki][ofm2][ifm2] = REGULAR_FILTER[ofm1][ifm1][kj][ki][ifm2][ofm2], on the
 * device; either of them unbound: _ERR_INVALID_TENSOR */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_trans_reg_filter(const libxsmm_dnn_layer* handle);

/* :394-396 -- kind FWD, BWD, UPD or ALL (else _ERR_INVALID_KIND); the sizes are the reference's */
LIBXSMM_API size_t libxsmm_dnn_get_scratch_size(const libxsmm_dnn_layer* handle, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_bind_scratch(libxsmm_dnn_layer* handle, const libxsmm_dnn_compute_kind kind, const void* scratch);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_release_scratch(libxsmm_dnn_layer* handle, const libxsmm_dnn_compute_kind kind);

/* :399-401 -- the tensor type is checked first (_ERR_UNKNOWN_TENSOR_TYPE), then NULL arguments (_ERR_INVALID_HANDLE_TENSOR for
 * bind and release, _ERR_INVALID_HANDLE for get); a tensor whose layout differs from the handle's is not bound: _ERR_MISMATCH_TENSOR.
 * (The reference declares libxsmm_dnn_get_tensor and defines it nowhere in its library; here it returns what is bound.) */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_bind_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_get_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_release_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type);

/* :404-406 */
LIBXSMM_API void libxsmm_dnn_execute(libxsmm_dnn_layer* handle, libxsmm_dnn_compute_kind kind);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_execute_st(libxsmm_dnn_layer* handle, libxsmm_dnn_compute_kind kind,
  /*unsigned*/int start_thread, /*unsigned*/int tid);

/* :409-412 -- transpose_filter: type REGULAR_FILTER (else _ERR_UNKNOWN_TENSOR_TYPE), a bound filter (_ERR_DATA_NOT_BOUND), a
 * scratch bound with BWD or ALL (_ERR_SCRATCH_NOT_ALLOCED), and then _ERR_MISMATCH_TENSOR: it transposes RSCK filters only.
 * reduce_wu_filters: type GRADIENT_FILTER, a bound gradient filter, and nothing to do (no thread-private filters exist).
 * get_codegen_success: _WARN_FALLBACK for FWD, BWD and UPD, as in the reference's generic path. get_parallel_tasks: the work
 * items of a pass (see Threads). A NULL handle is _ERR_INVALID_HANDLE in all four. */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_transpose_filter(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_reduce_wu_filters(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_get_codegen_success(libxsmm_dnn_layer* handle, libxsmm_dnn_compute_kind kind);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_get_parallel_tasks(libxsmm_dnn_layer* handle, libxsmm_dnn_compute_kind kind, unsigned int* num_tasks);

#endif /* LIBXSMM_DNN_CONVOLUTION_H */
