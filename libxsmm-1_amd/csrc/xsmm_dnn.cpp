// xsmm_dnn.cpp -- the tensor-handle layer of the DNN interface (include/libxsmm_dnn.h): error strings, datalayouts, tensors
// that link caller memory, and copy-in / copy-out / zero.
//
// Reference: src/libxsmm_dnn.c:70-189 (errors, type sizes), :330-360 (link), :1000-1203 (layouts and tensors), :1206-1570
// (copies, with src/template/libxsmm_dnn_tensor_{buffer_copy_{in,out}_nchw,filter_copy_{in,out}_kcrs}.tpl.c). Handles are
// plain host structures and no function here but those that touch tensor data asks for a device. Copy-in and copy-out are host
// loops over the tensor where the CPU addresses both operands (pageable, pinned, managed memory; the calling thread's stream is
// waited for first if the GPU may still be writing them) and one launch of kernels/dnn_copy.hip on the calling thread's stream
// where an operand is plain device memory; the reference forms are complete on return either way, the
// libxsmm_amd_*_async forms do not wait.
#include "xsmm_dnn_internal.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

using namespace xsmm;

LIBXSMM_API const char* libxsmm_dnn_get_error(libxsmm_dnn_err_t code)
{ // src/libxsmm_dnn.c:70-155
  switch (code) {
    case LIBXSMM_DNN_SUCCESS: return "LIBXSMM DNN Success!";
    case LIBXSMM_DNN_WARN_FALLBACK: return "LIBXSMM DNN Warning: Falling back to naive code as target is currently not supported by LIBXSMM!";
    case LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_N_BLOCKING: return "LIBXSMM DNN Warning: RNN cell suboptimal minibatch blocking!";
    case LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_C_BLOCKING: return "LIBXSMM DNN Warning: RNN cell suboptimal input feature blocking!";
    case LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_K_BLOCKING: return "LIBXSMM DNN Warning: RNN cell suboptimal output feature blocking!";
    case LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_N_BLOCKING: return "LIBXSMM DNN Warning: FC layer suboptimal minibatch blocking!";
    case LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_C_BLOCKING: return "LIBXSMM DNN Warning: FC layer suboptimal input feature blocking!";
    case LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_K_BLOCKING: return "LIBXSMM DNN Warning: FC layer suboptimal output feature blocking!";
    case LIBXSMM_DNN_ERR_GENERAL: return "LIBXSMM DNN Error: General error occurred!";
    case LIBXSMM_DNN_ERR_CREATE_HANDLE: return "LIBXSMM DNN Error: Handle creation failed!";
    case LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE: return "LIBXSMM DNN Error: Requested datatype is not available!";
    case LIBXSMM_DNN_ERR_INVALID_BLOCKING: return "LIBXSMM DNN Error: Requested Input/Output buffer size cannot be blocked!";
    case LIBXSMM_DNN_ERR_INVALID_HANDLE: return "LIBXSMM DNN Error: An invalid handle was provided!";
    case LIBXSMM_DNN_ERR_DATA_NOT_BOUND: return "LIBXSMM DNN Error: Not all required sources and destinations have been bound to convolution!";
    case LIBXSMM_DNN_ERR_CREATE_TENSOR: return "LIBXSMM DNN Error: Tensor creation failed!";
    case LIBXSMM_DNN_ERR_INVALID_TENSOR: return "LIBXSMM DNN Error: Invalid tensor was specified!";
    case LIBXSMM_DNN_ERR_MISMATCH_TENSOR: return "LIBXSMM DNN Error: Tensor doesn't match handle it should be bind to!";
    case LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR: return "LIBXSMM DNN Error: Invalid handle or tensor!";
    case LIBXSMM_DNN_ERR_INVALID_KIND: return "LIBXSMM DNN Error: Invalid convolution kind!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_NCHW: return "LIBXSMM DNN Error: NCHW format is currently not natively supported by LIBXSMM!";
    case LIBXSMM_DNN_ERR_UNSUPPORTED_DST_FORMAT: return "LIBXSMM DNN Error: Unsupported destination format when copying data!";
    case LIBXSMM_DNN_ERR_UNSUPPORTED_SRC_FORMAT: return "LIBXSMM DNN Error: Unsupported source format when copying data!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_CONVOLVE: return "LIBXSMM DNN Error: Unsupported format when requesting a convolution!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_KCRS: return "LIBXSMM DNN Error: KCRS format is currently not natively supported by LIBXSMM!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL: return "LIBXSMM DNN Error: Invalid format was specified!";
    case LIBXSMM_DNN_ERR_CREATE_LAYOUT: return "LIBXSMM DNN Error: Layout creation failed!";
    case LIBXSMM_DNN_ERR_INVALID_LAYOUT: return "LIBXSMM DNN Error: Invalid layout was specified!";
    case LIBXSMM_DNN_ERR_UNSUPPORTED_ARCH: return "LIBXSMM DNN Error: Unsupported architecture!";
    case LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED: return "LIBXSMM DNN Error: scratch binding failed as scratch was not allocated!";
    case LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE: return "LIBXSMM DNN Error: an unknown tensor type was provided!";
    case LIBXSMM_DNN_ERR_INVALID_ALGO: return "LIBXSMM DNN Error: Invalid algorithm was specified!";
    case LIBXSMM_DNN_ERR_INVALID_PADDING: return "LIBXSMM DNN Error: Invalid padding was specified!";
    case LIBXSMM_DNN_ERR_TIME_STEPS_TOO_SMALL: return "LIBXSMM DNN Error: time steps should be >= 2 for RNN/LSTM!";
    case LIBXSMM_DNN_ERR_CREATE_LAYOUT_ARRAYS: return "LIBXSMM DNN Error: failed to create internal layout arrays!";
    case LIBXSMM_DNN_ERR_NOT_IMPLEMENTED: return "LIBXSMM DNN Error: the requested functionality is right now not implemented!";
    case LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_ORDER: return "LIBXSMM DNN Error: the requested order of fusion in batch norm is right now not implemented!";
    case LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_FUSION: return "LIBXSMM DNN Error: the requested fusion in batch norm is right now not implemented!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_FUSEDBN: return "LIBXSMM DNN Error: Unsupported format when requesting a fused batch norm!";
    case LIBXSMM_DNN_ERR_UNSUPPORTED_POOLING: return "LIBXSMM DNN Error: Unsupported pooling operations was requested!";
    case LIBXSMM_DNN_ERR_INVALID_FORMAT_FC: return "LIBXSMM DNN Error: Unsupported format when requesting a fullyconnected layer!";
    case LIBXSMM_DNN_ERR_RNN_INVALID_SEQ_LEN: return "LIBXSMM DNN Error: max sequence length is shorter than sequence length we attempt to set!";
    default: return "LIBXSMM DNN Error: Unknown error or warning occurred!";
  }
}

LIBXSMM_API size_t libxsmm_dnn_typesize(libxsmm_dnn_datatype datatype)
{ // src/libxsmm_dnn.c:158-169
  switch (datatype) {
    case LIBXSMM_DNN_DATATYPE_F32: return 4;
    case LIBXSMM_DNN_DATATYPE_I32: return 4;
    case LIBXSMM_DNN_DATATYPE_BF16: return 2;
    case LIBXSMM_DNN_DATATYPE_I16: return 2;
    case LIBXSMM_DNN_DATATYPE_I8: return 1;
    default: return 1;
  }
}

LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_link_tensor(const libxsmm_dnn_tensor_datalayout* layout, const void* data, libxsmm_dnn_err_t* status)
{
  return libxsmm_dnn_link_qtensor(layout, data, 0, status);
}

LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_link_qtensor(const libxsmm_dnn_tensor_datalayout* layout, const void* data, const unsigned char scf, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:336-360
  libxsmm_dnn_tensor* tensor = static_cast<libxsmm_dnn_tensor*>(malloc(sizeof(libxsmm_dnn_tensor)));
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != layout && nullptr != tensor && nullptr != data) {
    memset(tensor, 0, sizeof(*tensor));
    tensor->layout = libxsmm_dnn_duplicate_tensor_datalayout(layout, status);
    tensor->data = const_cast<void*>(data);
    tensor->scf = scf;
    if (LIBXSMM_DNN_SUCCESS != *status && nullptr != tensor->layout) libxsmm_dnn_destroy_tensor_datalayout(tensor->layout);
  }
  else *status = LIBXSMM_DNN_ERR_CREATE_TENSOR;
  if (LIBXSMM_DNN_SUCCESS != *status) { free(tensor); tensor = nullptr; }
  return tensor;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_duplicate_tensor_datalayout(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1000-1035
  libxsmm_dnn_tensor_datalayout* dst = nullptr;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != layout && 0 != layout->num_dims) {
    dst = static_cast<libxsmm_dnn_tensor_datalayout*>(malloc(sizeof(*dst)));
    if (nullptr != dst) {
      memset(dst, 0, sizeof(*dst));
      dst->dim_type = static_cast<libxsmm_dnn_tensor_dimtype*>(malloc(layout->num_dims * sizeof(libxsmm_dnn_tensor_dimtype)));
      dst->dim_size = static_cast<unsigned int*>(malloc(layout->num_dims * sizeof(unsigned int)));
      dst->num_dims = layout->num_dims;
      dst->format = layout->format;
      dst->custom_format = layout->custom_format;
      dst->datatype = layout->datatype;
      dst->tensor_type = layout->tensor_type;
      if (nullptr != dst->dim_type && nullptr != dst->dim_size) {
        for (unsigned int dim = 0; dim < layout->num_dims; ++dim) { dst->dim_type[dim] = layout->dim_type[dim]; dst->dim_size[dim] = layout->dim_size[dim]; }
      }
      else *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT;
    }
    else *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT;
  }
  else *status = LIBXSMM_DNN_ERR_INVALID_LAYOUT;
  return dst;
}

LIBXSMM_API unsigned int libxsmm_dnn_compare_tensor_datalayout(const libxsmm_dnn_tensor_datalayout* a, const libxsmm_dnn_tensor_datalayout* b, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1038-1062 (tensor_type is not compared)
  unsigned int result = 0;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != a && nullptr != b) {
    if (a->num_dims != b->num_dims || a->format != b->format || a->custom_format != b->custom_format || a->datatype != b->datatype) result = 1;
    if (0 == result) {
      for (unsigned int dim = 0; dim < a->num_dims; ++dim) {
        if (a->dim_type[dim] != b->dim_type[dim] || a->dim_size[dim] != b->dim_size[dim]) result = 1;
      }
    }
  }
  else { *status = LIBXSMM_DNN_ERR_INVALID_LAYOUT; result = 100; }
  return result;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_tensor_datalayout(libxsmm_dnn_tensor_datalayout* layout)
{ // src/libxsmm_dnn.c:1065-1078
  if (nullptr == layout) return LIBXSMM_DNN_ERR_INVALID_LAYOUT;
  free(layout->dim_type);
  free(layout->dim_size);
  free(layout);
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API unsigned int libxsmm_dnn_get_tensor_size(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1081-1097 (an unsigned int product, as there)
  unsigned int size = 0;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != layout) {
    size = (unsigned int)libxsmm_dnn_typesize(layout->datatype);
    for (unsigned int dim = 0; dim < layout->num_dims; ++dim) size *= layout->dim_size[dim];
  }
  else *status = LIBXSMM_DNN_ERR_INVALID_LAYOUT;
  return size;
}

LIBXSMM_API unsigned int libxsmm_dnn_get_tensor_elements(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1100-1115
  unsigned int elements = 1;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != layout) {
    for (unsigned int dim = 0; dim < layout->num_dims; ++dim) elements *= layout->dim_size[dim];
  }
  else { *status = LIBXSMM_DNN_ERR_INVALID_LAYOUT; elements = 0; }
  return elements;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_set_tensor_data_ptr(libxsmm_dnn_tensor* tensor, const void* data)
{ // src/libxsmm_dnn.c:1118-1137
  if (nullptr == tensor || nullptr == data) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  if (nullptr == tensor->layout || 0 == tensor->layout->num_dims) return LIBXSMM_DNN_ERR_INVALID_LAYOUT;
  tensor->data = const_cast<void*>(data);
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API void* libxsmm_dnn_get_tensor_data_ptr(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1140-1152
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != tensor) return tensor->data;
  *status = LIBXSMM_DNN_ERR_INVALID_TENSOR;
  return nullptr;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_get_tensor_datalayout(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c: a copy the caller destroys
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != tensor) return libxsmm_dnn_duplicate_tensor_datalayout(tensor->layout, status);
  *status = LIBXSMM_DNN_ERR_INVALID_TENSOR;
  return nullptr;
}

LIBXSMM_API unsigned char libxsmm_dnn_get_qtensor_scf(const libxsmm_dnn_tensor* tensor, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:1155-1167
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != tensor) return tensor->scf;
  *status = LIBXSMM_DNN_ERR_INVALID_TENSOR;
  return 0;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_set_qtensor_scf(libxsmm_dnn_tensor* tensor, const unsigned char scf)
{ // src/libxsmm_dnn.c:1170-1182
  if (nullptr == tensor) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  tensor->scf = scf;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_tensor(const libxsmm_dnn_tensor* tensor)
{ // src/libxsmm_dnn.c:1185-1203 (destroying NULL is no error)
  if (nullptr != tensor) {
    if (nullptr != tensor->layout) libxsmm_dnn_destroy_tensor_datalayout(tensor->layout);
    free(const_cast<libxsmm_dnn_tensor*>(tensor));
  }
  return LIBXSMM_DNN_SUCCESS;
}

namespace {

// ---- tensor data the CPU can work on ---------------------------------------------------------------------------------------
// The tensor's bytes as the host sees them: the tensor itself where the CPU addresses it (after the stream has finished with
// it), a staged image otherwise (plain device memory). commit() sends a changed image back.
struct HostView {
  char* ptr = nullptr;
  std::vector<char> image;
  void* device = nullptr;
  size_t bytes = 0;
  bool open(void* data, size_t nbytes, bool read)
  {
    bytes = nbytes;
    const int kind = device_ready() ? pointer_kind(data) : 0;
    if (0 != kind && 0 != stream_sync()) return false; // (what the stream may still be writing; also seals an open burst)
    if (0 == kind || 0 != (kind & 2)) { ptr = static_cast<char*>(data); return true; }
    device = data;
    image.resize(nbytes);
    ptr = image.data();
    return !read || 0 == d2h(ptr, data, nbytes);
  }
  bool commit()
  {
    if (nullptr == device) return true;
    return 0 == h2d(device, ptr, bytes) && 0 == stream_sync();
  }
};

bool is_activation(libxsmm_dnn_tensor_type t)
{
  return LIBXSMM_DNN_REGULAR_INPUT == t || LIBXSMM_DNN_GRADIENT_INPUT == t || LIBXSMM_DNN_REGULAR_OUTPUT == t || LIBXSMM_DNN_GRADIENT_OUTPUT == t
      || LIBXSMM_DNN_INPUT == t || LIBXSMM_DNN_OUTPUT == t || LIBXSMM_DNN_ACTIVATION == t;
}
bool is_filter(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_FILTER == t || LIBXSMM_DNN_GRADIENT_FILTER == t || LIBXSMM_DNN_FILTER == t; }

// blocked <-> plain, element size ts. Activations (template/libxsmm_dnn_tensor_buffer_copy_{in,out}_nchw.tpl.c, custom format 1):
// blocked [N][fmb][H][W][bfm][lpb], plain [N][C][H][W] with C = fmb * bfm * lpb; 16-bit layouts carry lpb as their first dimension.
bool activation_dims(const libxsmm_dnn_tensor_datalayout& l, unsigned int d[6] /* N fmb H W bfm lpb */)
{
  const bool lowp = (LIBXSMM_DNN_DATATYPE_BF16 == l.datatype);
  if (l.num_dims != (lowp ? 6u : 5u)) return false;
  const unsigned int* s = l.dim_size;
  if (lowp) { d[5] = s[0]; d[4] = s[1]; d[3] = s[2]; d[2] = s[3]; d[1] = s[4]; d[0] = s[5]; }
  else { d[5] = 1; d[4] = s[0]; d[3] = s[1]; d[2] = s[2]; d[1] = s[3]; d[0] = s[4]; }
  return true;
}

void copy_activation(char* blocked, char* plain, const unsigned int d[6], size_t ts, bool in)
{
  const size_t N = d[0], fmb = d[1], H = d[2], W = d[3], bfm = d[4], lpb = d[5], Cc = fmb * bfm * lpb;
  for (size_t i1 = 0; i1 < N; ++i1) for (size_t i2 = 0; i2 < fmb; ++i2) for (size_t i3 = 0; i3 < H; ++i3) for (size_t i4 = 0; i4 < W; ++i4)
    for (size_t i5 = 0; i5 < bfm; ++i5) for (size_t i6 = 0; i6 < lpb; ++i6) {
      char* const b = blocked + (((((i1 * fmb + i2) * H + i3) * W + i4) * bfm + i5) * lpb + i6) * ts;
      char* const p = plain + (((i1 * Cc + (i2 * bfm * lpb + i5 * lpb + i6)) * H + i3) * W + i4) * ts;
      if (in) memcpy(b, p, ts); else memcpy(p, b, ts);
    }
}

// Filters (template/libxsmm_dnn_tensor_filter_copy_{in,out}_kcrs.tpl.c, custom format 1): blocked [ofmb][ifmb][R][S][bifm][bofm][lpb],
// plain [K][C][R][S]; a layout of 7 dimensions carries lpb first, one of 6 has lpb = 1.
bool filter_dims(const libxsmm_dnn_tensor_datalayout& l, unsigned int d[7] /* ofmb ifmb R S bifm bofm lpb */)
{
  const unsigned int* s = l.dim_size;
  if (7 == l.num_dims) { d[6] = s[0]; d[5] = s[1]; d[4] = s[2]; d[3] = s[3]; d[2] = s[4]; d[1] = s[5]; d[0] = s[6]; return true; }
  if (6 == l.num_dims) { d[6] = 1; d[5] = s[0]; d[4] = s[1]; d[3] = s[2]; d[2] = s[3]; d[1] = s[4]; d[0] = s[5]; return true; }
  return false;
}

void copy_filter(char* blocked, char* plain, const unsigned int d[7], size_t ts, bool in)
{
  const size_t ofmb = d[0], ifmb = d[1], R = d[2], S = d[3], bifm = d[4], bofm = d[5], lpb = d[6], Cc = ifmb * bifm * lpb;
  for (size_t i1 = 0; i1 < ofmb; ++i1) for (size_t i2 = 0; i2 < ifmb; ++i2) for (size_t i3 = 0; i3 < R; ++i3) for (size_t i4 = 0; i4 < S; ++i4)
    for (size_t i5 = 0; i5 < bifm; ++i5) for (size_t i6 = 0; i6 < bofm; ++i6) for (size_t i7 = 0; i7 < lpb; ++i7) {
      char* const b = blocked + ((((((i1 * ifmb + i2) * R + i3) * S + i4) * bifm + i5) * bofm + i6) * lpb + i7) * ts;
      char* const p = plain + ((((i1 * bofm + i6) * Cc + (i2 * bifm * lpb + i5 * lpb + i7)) * R + i3) * S + i4) * ts;
      if (in) memcpy(b, p, ts); else memcpy(p, b, ts);
    }
}

bool is_channel(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_CHANNEL_BIAS <= t && t <= LIBXSMM_DNN_CHANNEL_SCALAR; } // the 13 of :1300-1312

// What a copy between a layout and a plain format moves, or the status the reference gives instead (:1206-1362, :1407-1570: the
// tensor type, the plain format, the tensor's format, the data type; then what is not provided here). Channel tensors (bias,
// beta, gamma, statistics; template/libxsmm_dnn_tensor_bias_copy_{in,out}_nchw.tpl.c) have the same order on both sides:
// fmb * bfm * lpb elements, the plain format is NCHW (the reference's rule).
struct CopyShape { int form; unsigned int d[7]; size_t ts; };

libxsmm_dnn_err_t copy_shape(const libxsmm_dnn_tensor_datalayout& l, libxsmm_dnn_tensor_format format, bool in, CopyShape* c)
{
  const libxsmm_dnn_err_t bad_plain = in ? LIBXSMM_DNN_ERR_UNSUPPORTED_SRC_FORMAT : LIBXSMM_DNN_ERR_UNSUPPORTED_DST_FORMAT;
  const libxsmm_dnn_err_t bad_tensor = in ? LIBXSMM_DNN_ERR_UNSUPPORTED_DST_FORMAT : LIBXSMM_DNN_ERR_UNSUPPORTED_SRC_FORMAT;
  const bool act = is_activation(l.tensor_type), fil = is_filter(l.tensor_type), chan = is_channel(l.tensor_type);
  if (!act && !fil && !chan) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  if (format != (fil ? LIBXSMM_DNN_TENSOR_FORMAT_KCRS : LIBXSMM_DNN_TENSOR_FORMAT_NCHW)) return bad_plain;
  if (0 == (l.format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) return bad_tensor;
  if (LIBXSMM_DNN_DATATYPE_F32 != l.datatype && LIBXSMM_DNN_DATATYPE_BF16 != l.datatype) return LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
  for (unsigned int& x : c->d) x = 0;
  c->ts = libxsmm_dnn_typesize(l.datatype);
  if (chan) {
    if (l.num_dims != (LIBXSMM_DNN_DATATYPE_BF16 == l.datatype ? 3u : 2u)) return LIBXSMM_DNN_ERR_INVALID_LAYOUT;
    c->form = DNN_COPY_FLAT; c->d[0] = 1;
    for (unsigned int dim = 0; dim < l.num_dims; ++dim) c->d[0] *= l.dim_size[dim];
    return LIBXSMM_DNN_SUCCESS;
  }
  if (LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1 != l.custom_format) return LIBXSMM_DNN_ERR_NOT_IMPLEMENTED;
  c->form = act ? DNN_COPY_ACT : DNN_COPY_FIL;
  return (act ? activation_dims(l, c->d) : filter_dims(l, c->d)) ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_INVALID_LAYOUT;
}

// The geometry of a shape. dnn_copy_geom searches the LDS pitch, which costs the host tens of microseconds -- as much as the launch
// of a small tensor takes -- and a network repeats a handful of shapes: the last eight are kept per thread.
const DnnCopyGeom& geom_of(const CopyShape& c)
{
  struct Entry { CopyShape shape; DnnCopyGeom geom; bool used; };
  static thread_local Entry cache[8] = {};
  static thread_local unsigned int next = 0;
  for (const Entry& e : cache) {
    if (e.used && e.shape.form == c.form && e.shape.ts == c.ts && 0 == memcmp(e.shape.d, c.d, sizeof(c.d))) return e.geom;
  }
  Entry& e = cache[next++ % 8];
  e.shape = c; e.geom = dnn_copy_geom(c.form, c.d, (int)c.ts); e.used = true;
  return e.geom;
}

// The copy on the GPU: at least one operand is plain device memory (or the form is the one that does not wait). An operand in
// pageable memory travels through scratch slot 0 -- only one can, the other is device memory. Nothing waits before the launch:
// the stream orders the copy behind what was queued before. wait: complete on return.
libxsmm_dnn_err_t copy_on_device(const CopyShape& c, void* tensor_data, int kind_tensor, void* plain, int kind_plain, size_t bytes, bool in, bool wait)
{
  void* const stream = device().stream; // (launches what is open on the thread inside libxsmm_amd_defer_begin/end: call order)
  const DnnCopyGeom& g = geom_of(c);
  void* const src = in ? plain : tensor_data;
  void* const dst = in ? tensor_data : plain;
  void* dsrc = src; void* ddst = dst;
  if (0 == ((in ? kind_plain : kind_tensor) & 1)) {
    dsrc = scratch(0, bytes);
    if (nullptr == dsrc || 0 != h2d(dsrc, src, bytes)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  else if (0 == ((in ? kind_tensor : kind_plain) & 1)) { // (every element is written: nothing travels to the device first)
    ddst = scratch(0, bytes);
    if (nullptr == ddst) return LIBXSMM_DNN_ERR_GENERAL;
  }
  const char* name = "dnn_copy";
  const int e = launch_dnn_copy(g, in ? ddst : dsrc, in ? dsrc : ddst, in, stream, &name);
  if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  if (ddst != dst && 0 != d2h(dst, ddst, bytes)) return LIBXSMM_DNN_ERR_GENERAL;
  return (!wait || 0 == stream_sync()) ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}

// in: plain -> tensor; otherwise tensor -> plain. async: libxsmm_amd_dnn_copy{in,out}_tensor_async.
libxsmm_dnn_err_t copy_tensor(const libxsmm_dnn_tensor* tensor, void* plain, libxsmm_dnn_tensor_format format, bool in, bool async)
{
  if (nullptr == tensor || nullptr == tensor->layout) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  const libxsmm_dnn_tensor_datalayout& l = *tensor->layout;
  CopyShape c;
  const libxsmm_dnn_err_t status = copy_shape(l, format, in, &c);
  if (LIBXSMM_DNN_SUCCESS != status) return status;
  if (nullptr == plain || nullptr == tensor->data) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  size_t bytes = c.ts;
  for (unsigned int dim = 0; dim < l.num_dims; ++dim) bytes *= l.dim_size[dim];
  if (0 == bytes) return status;
  const int kt = device_ready() ? pointer_kind(tensor->data) : 0, kp = device_ready() ? pointer_kind(plain) : 0;
  if (async) { // both operands where the GPU reaches them, nothing staged, no wait
    if (0 == (kt & 1) || 0 == (kp & 1)) return LIBXSMM_DNN_ERR_GENERAL;
    return copy_on_device(c, tensor->data, kt, plain, kp, bytes, in, false);
  }
  if (1 == kt || 1 == kp) return copy_on_device(c, tensor->data, kt, plain, kp, bytes, in, true); // (plain device memory: the CPU cannot address it)
  HostView tv, pv;
  if (!tv.open(tensor->data, bytes, !in) || !pv.open(plain, bytes, in)) return LIBXSMM_DNN_ERR_GENERAL;
  if (DNN_COPY_FLAT == c.form) { if (in) memcpy(tv.ptr, pv.ptr, bytes); else memcpy(pv.ptr, tv.ptr, bytes); }
  else if (DNN_COPY_ACT == c.form) copy_activation(tv.ptr, pv.ptr, c.d, c.ts, in);
  else copy_filter(tv.ptr, pv.ptr, c.d, c.ts, in);
  if (!(in ? tv.commit() : pv.commit())) return LIBXSMM_DNN_ERR_GENERAL;
  return status;
}

} // namespace

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_copyin_tensor(const libxsmm_dnn_tensor* tensor, const void* data, const libxsmm_dnn_tensor_format in_format)
{
  return copy_tensor(tensor, const_cast<void*>(data), in_format, true, false);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_copyout_tensor(const libxsmm_dnn_tensor* tensor, void* data, const libxsmm_dnn_tensor_format out_format)
{
  return copy_tensor(tensor, data, out_format, false, false);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copyin_tensor_async(const libxsmm_dnn_tensor* tensor, const void* data, libxsmm_dnn_tensor_format in_format)
{
  return copy_tensor(tensor, const_cast<void*>(data), in_format, true, true);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copyout_tensor_async(const libxsmm_dnn_tensor* tensor, void* data, libxsmm_dnn_tensor_format out_format)
{
  return copy_tensor(tensor, data, out_format, false, true);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copy_plan(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_tensor_format plain_format, int in, long long plan[8])
{
  if (nullptr == layout || nullptr == plan) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  CopyShape c;
  const libxsmm_dnn_err_t status = copy_shape(*layout, plain_format, 0 != in, &c);
  if (LIBXSMM_DNN_SUCCESS != status) return status;
  const DnnCopyGeom& g = geom_of(c); // (what copy_on_device hands to the launcher)
  plan[0] = g.form; plan[1] = g.ts; plan[2] = g.blocks; plan[3] = g.J; plan[4] = g.L; plan[5] = 0 != g.lds ? g.jn : 0;
  plan[6] = g.items; plan[7] = g.grid;
  return status;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_zero_tensor(const libxsmm_dnn_tensor* tensor)
{ // src/libxsmm_dnn.c:1365-1404
  if (nullptr == tensor || nullptr == tensor->layout) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  libxsmm_dnn_err_t status = LIBXSMM_DNN_SUCCESS;
  const size_t n = libxsmm_dnn_get_tensor_elements(tensor->layout, &status);
  switch (tensor->layout->datatype) {
    case LIBXSMM_DNN_DATATYPE_F32: case LIBXSMM_DNN_DATATYPE_BF16: case LIBXSMM_DNN_DATATYPE_I32: case LIBXSMM_DNN_DATATYPE_I16: case LIBXSMM_DNN_DATATYPE_I8: break;
    default: return LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
  }
  const size_t bytes = n * libxsmm_dnn_typesize(tensor->layout->datatype);
  if (0 == bytes || nullptr == tensor->data) return status;
  const int kind = device_ready() ? pointer_kind(tensor->data) : 0;
  if (0 == kind) { memset(tensor->data, 0, bytes); return status; }
  // memory the GPU reaches: zeroed on the calling thread's stream (behind what was queued before), complete on return
  if (hipSuccess != hipMemsetAsync(tensor->data, 0, bytes, (hipStream_t)device().stream)) { (void)hipGetLastError(); return LIBXSMM_DNN_ERR_GENERAL; }
  return 0 == stream_sync() ? status : LIBXSMM_DNN_ERR_GENERAL;
}
