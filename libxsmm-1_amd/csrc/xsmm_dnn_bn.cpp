// xsmm_dnn_bn.cpp -- the fused batch-norm layer (include/libxsmm_dnn_fusedbatchnorm.h): handle, layouts, scratch and tensor
// binding as in the reference, and libxsmm_dnn_fusedbatchnorm_execute_st as at most three launches of kernels/bn.hip per call.
//
// Reference: src/libxsmm_dnn_fusedbatchnorm.c (handle rules :45-89, layouts :108-314, scratch :316-365, binding :369-536, execute
// :539-575), src/libxsmm_dnn_fusedbatchnorm_{forward,backward}.c (what must be bound: forward.c:137-154, backward.c:136-160; the
// fuse order and the eight fuse combinations) and src/template/libxsmm_dnn_fusedbatchnorm_st_{fwd,bwd}_custom_generic.tpl.c (the
// split of a pass over logical threads, :52-68). There the threads of a pass meet at barriers around a reduction through the
// caller's scratch; here every call is complete in itself. Everything up to execute_st is host-only.
#include "xsmm_dnn_internal.hpp"
#include "../../include/libxsmm_dnn_fusedbatchnorm.h"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>

using namespace xsmm;

struct libxsmm_dnn_fusedbatchnorm { // the fields of src/libxsmm_main.h's libxsmm_dnn_fusedbatchnorm that have a meaning here
  libxsmm_dnn_fusedbatchnorm_desc desc;
  libxsmm_dnn_tensor* reg_input; libxsmm_dnn_tensor* reg_output; libxsmm_dnn_tensor* grad_input; libxsmm_dnn_tensor* grad_output;
  libxsmm_dnn_tensor* reg_add; libxsmm_dnn_tensor* grad_add;
  libxsmm_dnn_tensor* reg_beta; libxsmm_dnn_tensor* reg_gamma; libxsmm_dnn_tensor* grad_beta; libxsmm_dnn_tensor* grad_gamma;
  libxsmm_dnn_tensor* expvalue; libxsmm_dnn_tensor* rcpstddev; libxsmm_dnn_tensor* variance;
  int ifmblock, ifmblock_hp, ofmblock, ofmblock_lp, blocksifm, blocksofm, fm_lp_block;
  size_t scratch_size;
  void* scratch;
  float* partials; // device memory of this handle: per logical thread 2 * 16 * blocks * N floats; allocated by the first execute_st
};

namespace {

std::mutex partials_lock; // the first execute_st of a handle may come from several threads at once

bool dt_pair(const libxsmm_dnn_fusedbatchnorm_desc& d, libxsmm_dnn_datatype in, libxsmm_dnn_datatype out) { return d.datatype_in == in && d.datatype_out == out; }
bool is_input(libxsmm_dnn_tensor_type t)
{
  return LIBXSMM_DNN_REGULAR_INPUT == t || LIBXSMM_DNN_GRADIENT_INPUT == t || LIBXSMM_DNN_INPUT == t || LIBXSMM_DNN_REGULAR_INPUT_ADD == t
      || LIBXSMM_DNN_GRADIENT_INPUT_ADD == t;
}
bool is_output(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_OUTPUT == t || LIBXSMM_DNN_GRADIENT_OUTPUT == t || LIBXSMM_DNN_OUTPUT == t; }
bool is_channel(libxsmm_dnn_tensor_type t)
{
  return LIBXSMM_DNN_REGULAR_CHANNEL_BETA == t || LIBXSMM_DNN_GRADIENT_CHANNEL_BETA == t || LIBXSMM_DNN_CHANNEL_BETA == t
      || LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA == t || LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA == t || LIBXSMM_DNN_CHANNEL_GAMMA == t
      || LIBXSMM_DNN_CHANNEL_EXPECTVAL == t || LIBXSMM_DNN_CHANNEL_RCPSTDDEV == t || LIBXSMM_DNN_CHANNEL_VARIANCE == t;
}

libxsmm_dnn_tensor** slot_of(libxsmm_dnn_fusedbatchnorm* h, libxsmm_dnn_tensor_type t) // nullptr: not one of the thirteen bindable types
{
  switch (t) {
    case LIBXSMM_DNN_REGULAR_INPUT: return &h->reg_input;
    case LIBXSMM_DNN_GRADIENT_INPUT: return &h->grad_input;
    case LIBXSMM_DNN_REGULAR_OUTPUT: return &h->reg_output;
    case LIBXSMM_DNN_GRADIENT_OUTPUT: return &h->grad_output;
    case LIBXSMM_DNN_REGULAR_INPUT_ADD: return &h->reg_add;
    case LIBXSMM_DNN_GRADIENT_INPUT_ADD: return &h->grad_add;
    case LIBXSMM_DNN_REGULAR_CHANNEL_BETA: return &h->reg_beta;
    case LIBXSMM_DNN_GRADIENT_CHANNEL_BETA: return &h->grad_beta;
    case LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA: return &h->reg_gamma;
    case LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA: return &h->grad_gamma;
    case LIBXSMM_DNN_CHANNEL_EXPECTVAL: return &h->expvalue;
    case LIBXSMM_DNN_CHANNEL_RCPSTDDEV: return &h->rcpstddev;
    case LIBXSMM_DNN_CHANNEL_VARIANCE: return &h->variance;
    default: return nullptr;
  }
}
bool bindable(libxsmm_dnn_tensor_type t) { libxsmm_dnn_fusedbatchnorm none; return nullptr != slot_of(&none, t); }

// a layout of n dimensions; false: out of memory
bool layout_dims(libxsmm_dnn_tensor_datalayout* l, unsigned int n, const libxsmm_dnn_tensor_dimtype* types, const unsigned int* sizes)
{
  l->dim_type = static_cast<libxsmm_dnn_tensor_dimtype*>(malloc(n * sizeof(libxsmm_dnn_tensor_dimtype)));
  l->dim_size = static_cast<unsigned int*>(malloc(n * sizeof(unsigned int)));
  if (nullptr == l->dim_type || nullptr == l->dim_size) { free(l->dim_type); free(l->dim_size); l->dim_type = nullptr; l->dim_size = nullptr; return false; }
  l->num_dims = n;
  for (unsigned int i = 0; i < n; ++i) { l->dim_type[i] = types[i]; l->dim_size[i] = sizes[i]; }
  return true;
}

// The tensors of a pass where the kernels can reach them. Those in pageable host memory share one block of device scratch
// (slot 6 of the calling thread), carved up in the order in which they are asked for.
struct Operand {
  void* dev; void* host; size_t bytes; size_t offset; bool upload;
};
struct Staging {
  Operand op[12]; int n = 0; size_t total = 0; bool wait = false;
  Operand* add(const libxsmm_dnn_tensor* t, bool upload)
  {
    Operand* const o = &op[n++];
    libxsmm_dnn_err_t st;
    o->bytes = (size_t)libxsmm_dnn_get_tensor_elements(t->layout, &st) * libxsmm_dnn_typesize(t->layout->datatype);
    const int kind = pointer_kind(t->data);
    o->dev = t->data; o->host = nullptr; o->offset = 0; o->upload = upload;
    if (0 != (kind & 2)) wait = true;
    if (0 == (kind & 1)) { o->host = t->data; o->dev = nullptr; o->offset = total; total += (o->bytes + 255) & ~(size_t)255; wait = true; }
    return o;
  }
  bool place() // false: no memory, or a copy failed
  {
    if (0 == total) return true;
    char* const base = static_cast<char*>(scratch(6, total));
    if (nullptr == base) return false;
    for (int i = 0; i < n; ++i) {
      if (nullptr == op[i].host) continue;
      op[i].dev = base + op[i].offset;
      if (op[i].upload && 0 != h2d(op[i].dev, op[i].host, op[i].bytes)) return false;
    }
    return true;
  }
};
bool back(const Operand* o) { return nullptr == o || nullptr == o->host || 0 == d2h(o->host, o->dev, o->bytes); }
bool aligned16(const Operand* o) { return nullptr == o || 0 == reinterpret_cast<uintptr_t>(o->dev) % 16; }

} // namespace

LIBXSMM_API libxsmm_dnn_fusedbatchnorm* libxsmm_dnn_create_fusedbatchnorm(libxsmm_dnn_fusedbatchnorm_desc desc, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn_fusedbatchnorm.c:45-89
  const bool f32 = dt_pair(desc, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32), lowp = dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16);
  if (!f32 && !lowp) { *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE; return nullptr; }
  libxsmm_dnn_fusedbatchnorm* const h = static_cast<libxsmm_dnn_fusedbatchnorm*>(malloc(sizeof(libxsmm_dnn_fusedbatchnorm)));
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_CREATE_HANDLE; return nullptr; }
  *status = LIBXSMM_DNN_SUCCESS;
  memset(h, 0, sizeof(*h));
  h->desc = desc;
  // libxsmm_dnn_get_feature_map_blocks(C, C) (src/libxsmm_dnn_setup.c:197-252): the output block is 16 whatever C is
  if (f32) { h->ifmblock = desc.C >= 16 ? 16 : desc.C; h->fm_lp_block = 1; }
  else {
    h->ifmblock = desc.C >= 16 ? 8 : desc.C / 2; h->fm_lp_block = 2;
    if (3 == desc.C) { h->ifmblock = 3; h->fm_lp_block = 1; }
  }
  h->ofmblock = 16;
  h->ifmblock_hp = h->ifmblock * h->fm_lp_block;
  h->ofmblock_lp = h->ofmblock / h->fm_lp_block;
  // (a block of zero divides nothing: the reference would trap; here there are no blocks)
  const int iblock = f32 ? h->ifmblock : h->ifmblock_hp;
  h->blocksifm = 0 < iblock ? desc.C / iblock : 0;
  h->blocksofm = desc.C / h->ofmblock;
  h->scratch_size = sizeof(float) * 2 * (size_t)desc.C * (size_t)desc.N; // :80
  return h;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_fusedbatchnorm(const libxsmm_dnn_fusedbatchnorm* handle)
{ // :92-105
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  dev_free(handle->partials); // (waits for what may still use it)
  free(const_cast<libxsmm_dnn_fusedbatchnorm*>(handle));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(const libxsmm_dnn_fusedbatchnorm* h, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :108-314
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dH = LIBXSMM_DNN_TENSOR_DIMTYPE_H, dW = LIBXSMM_DNN_TENSOR_DIMTYPE_W, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* l = static_cast<libxsmm_dnn_tensor_datalayout*>(malloc(sizeof(*l)));
  if (nullptr == l) { *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT; return nullptr; }
  memset(l, 0, sizeof(*l));
  const libxsmm_dnn_fusedbatchnorm_desc& d = h->desc;
  l->format = d.buffer_format;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  const bool f32 = dt_pair(d, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32);
  const unsigned int N = (unsigned int)d.N;
  const unsigned int ifwp = (unsigned int)(d.W + 2 * d.pad_w_in), ifhp = (unsigned int)(d.H + 2 * d.pad_h_in);
  // (a stride of zero divides nothing: the reference would trap; here the output has its padding only)
  const unsigned int ofwp = (unsigned int)((0 != d.v ? d.W / d.v : 0) + 2 * d.pad_w_out), ofhp = (unsigned int)((0 != d.u ? d.H / d.u : 0) + 2 * d.pad_h_out);
  bool ok = true; // false: the arrays could not be allocated
  if (is_input(type) || is_output(type)) {
    if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
      if (f32) {
        const D t[5] = { dC, dW, dH, dC, dN };
        const unsigned int in[5] = { (unsigned int)h->ifmblock, ifwp, ifhp, (unsigned int)h->blocksifm, N };
        const unsigned int out[5] = { (unsigned int)h->ofmblock, ofwp, ofhp, (unsigned int)h->blocksofm, N };
        l->datatype = LIBXSMM_DNN_DATATYPE_F32;
        ok = layout_dims(l, 5, t, is_input(type) ? in : out);
      }
      else {
        const D t[6] = { dC, dC, dW, dH, dC, dN };
        const unsigned int in[6] = { (unsigned int)h->fm_lp_block, (unsigned int)h->ifmblock, ifwp, ifhp, (unsigned int)h->blocksifm, N };
        const unsigned int out[6] = { (unsigned int)h->fm_lp_block, (unsigned int)h->ofmblock_lp, ofwp, ofhp, (unsigned int)h->blocksofm, N };
        l->datatype = LIBXSMM_DNN_DATATYPE_BF16;
        ok = layout_dims(l, 6, t, is_input(type) ? in : out);
      }
    }
    else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NHWC)) {
      const D t[4] = { dC, dW, dH, dN };
      const unsigned int in[4] = { (unsigned int)d.C, ifwp, ifhp, N }, out[4] = { (unsigned int)d.C, ofwp, ofhp, N };
      l->datatype = d.datatype_in;
      ok = layout_dims(l, 4, t, is_input(type) ? in : out);
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else if (is_channel(type)) {
    l->tensor_type = LIBXSMM_DNN_CHANNEL_SCALAR;
    if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
      if (LIBXSMM_DNN_DATATYPE_F32 == d.datatype_stats) {
        const D t[2] = { dC, dC };
        const unsigned int s[2] = { (unsigned int)(h->ifmblock * h->fm_lp_block), (unsigned int)h->blocksifm };
        l->datatype = d.datatype_stats;
        ok = layout_dims(l, 2, t, s);
      }
      else *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
    }
    else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NHWC)) {
      if (LIBXSMM_DNN_DATATYPE_F32 == d.datatype_stats) {
        const D t[1] = { dC };
        const unsigned int s[1] = { (unsigned int)d.C };
        l->datatype = d.datatype_stats;
        ok = layout_dims(l, 1, t, s);
      }
      else *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (!ok) *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT_ARRAYS;
  if (LIBXSMM_DNN_SUCCESS != *status) { free(l->dim_type); free(l->dim_size); free(l); return nullptr; }
  return l;
}

LIBXSMM_API size_t libxsmm_dnn_fusedbatchnorm_get_scratch_size(const libxsmm_dnn_fusedbatchnorm* handle, libxsmm_dnn_err_t* status)
{ // :316-327 (64 bytes more for a caller that does not align)
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != handle) return handle->scratch_size + 64;
  *status = LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return 0;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_scratch(libxsmm_dnn_fusedbatchnorm* handle, const void* scratch)
{ // :330-353 (the pointer is kept, aligned as there, and never dereferenced)
  const uintptr_t address = reinterpret_cast<uintptr_t>(scratch);
  if (nullptr == scratch) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  handle->scratch = reinterpret_cast<void*>(0 == address % 64 ? address : address + (64 - address % 64));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_scratch(libxsmm_dnn_fusedbatchnorm* handle)
{ // :356-365
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  handle->scratch = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{ // :369-428
  libxsmm_dnn_err_t status = LIBXSMM_DNN_SUCCESS;
  if (!bindable(type)) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == handle || nullptr == tensor) return LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR;
  libxsmm_dnn_tensor_datalayout* const want = libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, type, &status);
  if (0 == libxsmm_dnn_compare_tensor_datalayout(want, tensor->layout, &status)) *slot_of(handle, type) = const_cast<libxsmm_dnn_tensor*>(tensor);
  else status = LIBXSMM_DNN_ERR_MISMATCH_TENSOR;
  if (nullptr != want) libxsmm_dnn_destroy_tensor_datalayout(want);
  return status;
}

LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_fusedbatchnorm_get_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :431-483
  *status = LIBXSMM_DNN_SUCCESS;
  if (!bindable(type)) { *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE; return nullptr; }
  if (nullptr == handle) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  return *slot_of(handle, type);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type)
{ // :486-536
  if (!bindable(type)) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  *slot_of(handle, type) = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_execute_st(libxsmm_dnn_fusedbatchnorm* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{ // :539-575 and the drivers of the two passes (src/libxsmm_dnn_fusedbatchnorm_forward.c:132-233, _backward.c:131-239)
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind && LIBXSMM_DNN_COMPUTE_KIND_BWD != kind) return LIBXSMM_DNN_ERR_INVALID_KIND;
  const libxsmm_dnn_fusedbatchnorm_desc& d = h->desc;
  if (LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM != d.buffer_format) return LIBXSMM_DNN_ERR_INVALID_FORMAT_FUSEDBN;
  const bool bwd = LIBXSMM_DNN_COMPUTE_KIND_BWD == kind;
  const int ops = (int)d.fuse_ops;
  const bool stats = 0 != (ops & LIBXSMM_DNN_FUSEDBN_OPS_BN), eltwise = 0 != (ops & LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE), relu = 0 != (ops & LIBXSMM_DNN_FUSEDBN_OPS_RELU);
  if (!bwd) {
    if (nullptr == h->reg_input || nullptr == h->reg_output || nullptr == h->reg_beta || nullptr == h->reg_gamma || nullptr == h->expvalue
      || nullptr == h->rcpstddev || nullptr == h->variance || (eltwise && nullptr == h->reg_add))
    {
      return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
    }
  }
  else if (nullptr == h->reg_input || nullptr == h->reg_gamma || nullptr == h->grad_input || nullptr == h->grad_output || nullptr == h->grad_beta
    || nullptr == h->grad_gamma || nullptr == h->expvalue || nullptr == h->rcpstddev || (eltwise && nullptr == h->grad_add) || (relu && nullptr == h->reg_output))
  {
    return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  }
  if (LIBXSMM_DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU != d.fuse_order) return LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_ORDER;
  // exactly one of BN and BNSCALE, with or without ELTWISE and RELU
  if (0 != (ops & ~15) || (1 != (ops & 3) && 2 != (ops & 3))) return LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_FUSION;
  // from here on: this engine's own (the scratch is not asked for: the partial sums live in memory of the handle)
  const int ltid = tid - start_thread;
  if (ltid < 0 || d.threads < 1) return LIBXSMM_DNN_ERR_GENERAL;
  // the kernels address pixels of 16 channels, with 32-bit indices inside a plane
  if (16 != h->ifmblock_hp || h->blocksifm != h->blocksofm) return LIBXSMM_DNN_ERR_GENERAL;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.u < 1 || d.v < 1 || d.pad_h_in < 0 || d.pad_w_in < 0 || d.pad_h_out < 0 || d.pad_w_out < 0
    || 0 != d.H % d.u || 0 != d.W % d.v || (long long)d.H * d.W >= (1LL << 27))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }

  // the share of ltid (the templates' chunksize, thr_begin, thr_end)
  const long long blocks = h->blocksifm, work = (long long)d.N * blocks;
  const long long chunk = (0 == work % d.threads) ? (work / d.threads) : (work / d.threads + 1);
  const long long b0 = (ltid * chunk < work) ? ltid * chunk : work;
  const long long b1 = ((ltid + 1LL) * chunk < work) ? (ltid + 1LL) * chunk : work;
  if (ltid >= d.threads || b0 >= b1) return LIBXSMM_DNN_SUCCESS;
  if (work > 0x7fffffffLL / 32) return LIBXSMM_DNN_ERR_GENERAL;

  if (!device_ready()) { fail_no_device("libxsmm_dnn_fusedbatchnorm_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  const size_t region = (size_t)work * 32; // floats of one logical thread's partial sums
  if (stats && nullptr == h->partials) {
    std::lock_guard<std::mutex> guard(partials_lock);
    if (nullptr == h->partials) h->partials = static_cast<float*>(dev_alloc(region * sizeof(float) * (size_t)d.threads));
    if (nullptr == h->partials) return LIBXSMM_DNN_ERR_GENERAL;
  }
  // (a staged destination starts from the caller's bytes: only the share's interior is written, and the whole image travels back)
  Staging s;
  Operand* const ox = s.add(h->reg_input, true);
  Operand* const ogamma = s.add(h->reg_gamma, true);
  Operand* const omean = s.add(h->expvalue, true);
  Operand* const orstd = s.add(h->rcpstddev, true);
  Operand *obeta = nullptr, *ovar = nullptr, *oout = nullptr, *oadd = nullptr, *odout = nullptr, *odin = nullptr, *odgamma = nullptr, *odbeta = nullptr;
  if (!bwd) {
    obeta = s.add(h->reg_beta, true); ovar = s.add(h->variance, true); oout = s.add(h->reg_output, true);
    if (eltwise) oadd = s.add(h->reg_add, true);
  }
  else {
    odout = s.add(h->grad_output, true); odin = s.add(h->grad_input, true);
    odgamma = s.add(h->grad_gamma, true); odbeta = s.add(h->grad_beta, true);
    if (eltwise) oadd = s.add(h->grad_add, true);
    if (relu) oout = s.add(h->reg_output, true);
  }
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  if (!aligned16(ox) || !aligned16(oout) || !aligned16(oadd) || !aligned16(odout) || !aligned16(odin) || !aligned16(ogamma) || !aligned16(obeta)
    || !aligned16(omean) || !aligned16(orstd) || !aligned16(ovar) || !aligned16(odgamma) || !aligned16(odbeta))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }
  BnArgs g; memset(&g, 0, sizeof(g));
  g.in = ox->dev; g.add = nullptr != oadd ? oadd->dev : nullptr; g.out = nullptr != oout ? oout->dev : nullptr;
  g.dout = nullptr != odout ? odout->dev : nullptr; g.din = nullptr != odin ? odin->dev : nullptr;
  g.gamma = static_cast<float*>(ogamma->dev); g.beta = nullptr != obeta ? static_cast<float*>(obeta->dev) : nullptr;
  g.mean = static_cast<float*>(omean->dev); g.rstd = static_cast<float*>(orstd->dev); g.var = nullptr != ovar ? static_cast<float*>(ovar->dev) : nullptr;
  g.dgamma = nullptr != odgamma ? static_cast<float*>(odgamma->dev) : nullptr; g.dbeta = nullptr != odbeta ? static_cast<float*>(odbeta->dev) : nullptr;
  g.part = stats ? h->partials + region * (size_t)ltid : nullptr;
  g.N = d.N; g.H = d.H; g.W = d.W; g.u = d.u; g.v = d.v; g.blocks = (int)blocks;
  g.iph = d.pad_h_in; g.ipw = d.pad_w_in; g.oph = d.pad_h_out; g.opw = d.pad_w_out;
  g.ofh = d.H / d.u; g.ofw = d.W / d.v; g.w0 = (int)b0; g.w1 = (int)b1;
  // the channel blocks of the items [b0, b1): all of them once the share is as long as an image, else a run that may wrap
  g.fm0 = (b1 - b0 >= blocks) ? 0 : (int)(b0 % blocks);
  g.nfm = (b1 - b0 >= blocks) ? (int)blocks : (int)(b1 - b0);
  g.nhw = (float)(d.N * d.H * d.W); g.recp_nhw = 1.0f / g.nhw;
  g.bwd = bwd ? 1 : 0; g.bf16 = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16) ? 1 : 0;
  g.stats = stats ? 1 : 0; g.eltwise = eltwise ? 1 : 0; g.relu = relu ? 1 : 0;
  for (int step = stats ? 0 : 2; step < 3; ++step) {
    const char* name = "";
    const int e = 0 == step ? launch_bn_partial(g, stream, &name) : (1 == step ? launch_bn_finish(g, stream, &name) : launch_bn_apply(g, stream, &name));
    note_launch(name);
    if (0 != e) {
      fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
      return LIBXSMM_DNN_ERR_GENERAL;
    }
  }
  // what the pass wrote travels back if it was staged
  bool ok = true;
  if (!bwd) {
    ok = back(oout);
    if (stats) ok = ok && back(omean) && back(orstd) && back(ovar);
  }
  else {
    ok = back(odin);
    if (stats) ok = ok && back(odgamma) && back(odbeta) && (!relu || back(odout)) && (!eltwise || back(oadd));
  }
  if (!ok) return LIBXSMM_DNN_ERR_GENERAL;
  if (s.wait) return 0 == stream_sync() ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
  return LIBXSMM_DNN_SUCCESS;
}
