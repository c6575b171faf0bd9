/* libxsmm_dnn_pooling.h -- the pooling layer of the reference's DNN interface on the GPU (reference:
 * include/libxsmm_dnn_pooling.h:37-82, src/libxsmm_dnn_pooling.c, src/libxsmm_dnn_pooling_{forward,backward}.c and
 * src/template/libxsmm_dnn_pooling_st_{fwd,bwd}_custom_generic.tpl.c). Line numbers below refer to the reference's header unless
 * a file is named.
 *
 * Arithmetic: bit for bit what the reference's generic templates return (the reference run with LIBXSMM_TARGET=hsw; its AVX-512
 * templates fuse the multiply-add of the average BWD and compare differently). Tensors are blocked, [N][C/16][rows][columns][16];
 * an item is one (image, channel block) plane.
 *   FWD MAX  every output starts at -FLT_MAX; its window is walked kh ascending, then kw ascending; positions outside
 *            [0,H) x [0,W) are skipped; a strict > replaces the value. So the first maximum wins ties and a NaN never wins. An
 *            output none of whose inputs exceeds -FLT_MAX is stored as -FLT_MAX and its mask element is NOT written. The mask
 *            value is (hi+kh)*W*16 + (wi+kw)*16 + lane: relative to the unpadded plane of the item.
 *   FWD AVG  an fp32 sum from +0.0f in the same order (skipped positions add nothing), then one multiply by
 *            1.0f / ((float)R * (float)S): the divisor is R*S at the borders too.
 *   BWD MAX  every input element sums, from +0.0f, the dout of the outputs whose mask names it, ho ascending then wo ascending.
 *   BWD AVG  every input element sums dout * recp over the outputs whose window covers it, in the same order; the multiply and
 *            the add are two roundings (not fused), as in the reference's build.
 *            Input elements no window covers are written as +0.0 in both.
 *   BF16     widened by a shift, computed in fp32, stored by truncation (the upper 16 bits).
 * Physical padding (pad_*_out of the FWD output, pad_*_in of the BWD dinput) is never written, and pad_*_in of the input and
 * pad_*_out of doutput are never read.
 *
 * Handles. libxsmm_dnn_create_pooling follows src/libxsmm_dnn_pooling.c:44-95 and never touches a device: datatypes in/out F32/F32
 * or BF16/BF16, anything else _ERR_UNSUPPORTED_DATATYPE and NULL. The channel blocks are those of
 * libxsmm_dnn_get_feature_map_blocks(C, C) (src/libxsmm_dnn_setup.c:197-252), quirks included: F32 with C < 16 has an input block
 * of C, an output block of 16 and therefore NO output blocks (its output and mask layouts have zero elements), and a C that is
 * no multiple of 16 silently loses the remainder. ofh = (H + 2*pad_h - R)/u + 1, ofw likewise. Layouts are those of
 * create_tensor_datalayout there (:114-291): format LIBXSMM has five dimensions in F32 (16, W, H, C/16, N) and six in BF16
 * (2, 8, W, H, C/16, N); format NHWC has four, reports datatype_in for every tensor and answers _ERR_UNKNOWN_TENSOR_TYPE for the
 * mask; other formats _ERR_INVALID_FORMAT_GENERAL. The mask has five dimensions (16, ofw, ofh, C/16, N) of desc.datatype_mask
 * and no physical padding -- in BF16 too, where the reference reports six dimensions and leaves the size of the sixth
 * uninitialised.
 *
 * execute_st checks, in this order: NULL handle (_ERR_INVALID_HANDLE); kind other than FWD / BWD (_ERR_INVALID_KIND);
 * buffer_format other than exactly _LIBXSMM (_ERR_INVALID_FORMAT_FUSEDBN, the code the reference returns here); tensors (FWD:
 * regular input and output, BWD: gradient input and output, both: the mask if the type is MAX; _ERR_DATA_NOT_BOUND);
 * pooling type other than MAX / AVG (_ERR_UNSUPPORTED_POOLING). Then what is this engine's own:
 *   - The scratch is never read or written and execute_st does not ask for it (the reference would dereference NULL).
 *     get_scratch_size, bind_scratch and release_scratch keep the reference's formula and statuses.
 *   - tid - start_thread < 0 returns _ERR_GENERAL (the reference indexes out of bounds), as the fully-connected layer does.
 *   - MAX with datatype_mask != I32 returns _ERR_UNSUPPORTED_DATATYPE: the reference writes 32-bit indices whatever the layout
 *     says and so runs past the end of a smaller tensor.
 *   - A handle whose channel block is not 16 on both sides (C < 16), a desc with a non-positive extent, window or stride or
 *     a negative padding, a plane of 2^27 pixels or more, and a device tensor that is not 16-byte aligned return _ERR_GENERAL
 *     (for C < 16 the reference writes C-wide pixels into an output layout of zero elements).
 *   - BWD MAX trusts only mask values FWD could have written: an index inside the output's own window and in the element's
 *     own channel lane. Anything else, the elements FWD never wrote included, contributes nothing; the reference would use it
 *     as an index.
 *
 * Threads. Work is N * (C/16) items. execute_st(handle, kind, start_thread, tid) computes the items of logical thread
 * ltid = tid - start_thread: [ltid * chunk, min((ltid + 1) * chunk, work)) with chunk = ceil(work / desc.threads). One call is ONE
 * kernel launch over that range on the calling thread's stream (libxsmm_amd_set_stream); an empty range launches nothing and
 * returns _SUCCESS. No barrier, nothing shared: any subset of the threads, in any order and on any streams, gives the bits of
 * threads = 1, which is the fast way.
 *
 * Memory: as for the fully-connected layer (libxsmm_dnn_fullyconnected.h) -- tensors the GPU reaches are processed in place
 * and the call does not wait; a host-visible tensor makes the call complete on return; pageable host memory is staged. */
#ifndef LIBXSMM_DNN_POOLING_H
#define LIBXSMM_DNN_POOLING_H

#include "libxsmm_dnn.h"

/** Opaque handle (:38). */
typedef struct libxsmm_dnn_pooling libxsmm_dnn_pooling;

typedef enum libxsmm_dnn_pooling_type { /* :40-43 */
  LIBXSMM_DNN_POOLING_MAX = 1,
  LIBXSMM_DNN_POOLING_AVG = 2
} libxsmm_dnn_pooling_type;

typedef struct libxsmm_dnn_pooling_desc { /* :45-66 */
  int N;                                     /* number of images in mini-batch */
  int C;                                     /* number of feature maps */
  int H;                                     /* height of the input image */
  int W;                                     /* width of the input image */
  int R;                                     /* window height */
  int S;                                     /* window width */
  int u;                                     /* vertical stride */
  int v;                                     /* horizontal stride */
  int pad_h;                                 /* logical padding of the input, rows */
  int pad_w;                                 /* logical padding of the input, columns */
  int pad_h_in;                              /* physical padding of the input buffer, rows */
  int pad_w_in;                              /* physical padding of the input buffer, columns */
  int pad_h_out;                             /* physical padding of the output buffer, rows */
  int pad_w_out;                             /* physical padding of the output buffer, columns */
  int threads;                               /* number of logical threads the passes are split into */
  libxsmm_dnn_datatype datatype_in;          /* datatype of all input related buffers */
  libxsmm_dnn_datatype datatype_out;         /* datatype of all output related buffers */
  libxsmm_dnn_datatype datatype_mask;        /* datatype of the mask */
  libxsmm_dnn_tensor_format buffer_format;   /* format of the activation buffers */
  libxsmm_dnn_pooling_type pooling_type;     /* max or average */
} libxsmm_dnn_pooling_desc;

/* :68-69 */
LIBXSMM_API libxsmm_dnn_pooling* libxsmm_dnn_create_pooling(libxsmm_dnn_pooling_desc pooling_desc, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_pooling(const libxsmm_dnn_pooling* handle);

/* :71 -- type: LIBXSMM_DNN_{REGULAR,GRADIENT}_{INPUT,OUTPUT}, the general _INPUT / _OUTPUT, or LIBXSMM_DNN_POOLING_MASK */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_pooling_create_tensor_datalayout(const libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);

/* :73-75 */
LIBXSMM_API size_t libxsmm_dnn_pooling_get_scratch_size(const libxsmm_dnn_pooling* handle, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_scratch(libxsmm_dnn_pooling* handle, const void* scratch);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_scratch(libxsmm_dnn_pooling* handle);

/* :77-79 -- the tensor type is checked first (_ERR_UNKNOWN_TENSOR_TYPE), then NULL arguments (_ERR_INVALID_HANDLE_TENSOR for
 * bind); a tensor whose layout differs from the handle's is not bound: _ERR_MISMATCH_TENSOR */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_pooling_get_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type);

/* :81-82 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_execute_st(libxsmm_dnn_pooling* handle, libxsmm_dnn_compute_kind kind,
  /*unsigned*/int start_thread, /*unsigned*/int tid);

#endif /* LIBXSMM_DNN_POOLING_H */
