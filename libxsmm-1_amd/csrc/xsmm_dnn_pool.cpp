// xsmm_dnn_pool.cpp -- the pooling layer (include/libxsmm_dnn_pooling.h): handle, layouts, scratch and tensor binding as in the
// reference, and libxsmm_dnn_pooling_execute_st as one launch of kernels/pool.hip per call.
//
// Reference: src/libxsmm_dnn_pooling.c (handle rules :44-95, layouts :114-291, scratch :293-343, binding :346-453, execute
// :456-492), src/libxsmm_dnn_pooling_{forward,backward}.c (what must be bound: :112-117 of each; the pooling types) and
// src/template/libxsmm_dnn_pooling_st_{fwd,bwd}_custom_generic.tpl.c (the split of a pass over logical threads, :52-60). There a
// pass is a loop over (image, channel block) items through a per-thread copy in scratch; here an item range is one kernel
// launch that addresses the blocked tensors where they lie. Everything up to execute_st is host-only.
#include "xsmm_dnn_internal.hpp"
#include "../../include/libxsmm_dnn_pooling.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

struct libxsmm_dnn_pooling { // the fields of src/libxsmm_main.h's libxsmm_dnn_pooling that have a meaning here
  libxsmm_dnn_pooling_desc desc;
  libxsmm_dnn_tensor* reg_input; libxsmm_dnn_tensor* reg_output;
  libxsmm_dnn_tensor* grad_input; libxsmm_dnn_tensor* grad_output;
  libxsmm_dnn_tensor* mask;
  int ifmblock, ifmblock_hp, ofmblock, ofmblock_lp, blocksifm, blocksofm, fm_lp_block;
  int ofh, ofw;
  size_t scratch_size;
  void* scratch;
};

namespace {

bool dt_pair(const libxsmm_dnn_pooling_desc& d, libxsmm_dnn_datatype in, libxsmm_dnn_datatype out) { return d.datatype_in == in && d.datatype_out == out; }
bool is_input(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_INPUT == t || LIBXSMM_DNN_GRADIENT_INPUT == t || LIBXSMM_DNN_INPUT == t; }
bool is_output(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_OUTPUT == t || LIBXSMM_DNN_GRADIENT_OUTPUT == t || LIBXSMM_DNN_OUTPUT == t; }
bool bindable(libxsmm_dnn_tensor_type t)
{
  return LIBXSMM_DNN_REGULAR_INPUT == t || LIBXSMM_DNN_GRADIENT_INPUT == t || LIBXSMM_DNN_REGULAR_OUTPUT == t || LIBXSMM_DNN_GRADIENT_OUTPUT == t
      || LIBXSMM_DNN_POOLING_MASK == t;
}

libxsmm_dnn_tensor** slot_of(libxsmm_dnn_pooling* h, libxsmm_dnn_tensor_type t)
{
  switch (t) {
    case LIBXSMM_DNN_REGULAR_INPUT: return &h->reg_input;
    case LIBXSMM_DNN_GRADIENT_INPUT: return &h->grad_input;
    case LIBXSMM_DNN_REGULAR_OUTPUT: return &h->reg_output;
    case LIBXSMM_DNN_GRADIENT_OUTPUT: return &h->grad_output;
    default: return &h->mask;
  }
}

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

// One tensor where the kernel can reach it (as in xsmm_dnn_fc.cpp).
struct Operand {
  void* dev; void* host; size_t bytes; bool wait;
};
bool operand_in(Operand* o, const libxsmm_dnn_tensor* t, int slot, bool upload)
{
  libxsmm_dnn_err_t st;
  o->bytes = (size_t)libxsmm_dnn_get_tensor_elements(t->layout, &st) * libxsmm_dnn_typesize(t->layout->datatype);
  const int kind = pointer_kind(t->data);
  o->dev = t->data; o->host = nullptr; o->wait = (0 != (kind & 2));
  if (0 == (kind & 1)) {
    o->dev = scratch(slot, o->bytes);
    if (nullptr == o->dev || (upload && 0 != h2d(o->dev, t->data, o->bytes))) return false;
    o->host = t->data; o->wait = true;
  }
  return true;
}

} // namespace

LIBXSMM_API libxsmm_dnn_pooling* libxsmm_dnn_create_pooling(libxsmm_dnn_pooling_desc desc, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn_pooling.c:44-95
  const bool f32 = dt_pair(desc, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32), lowp = dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16);
  if (!f32 && !lowp) { *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE; return nullptr; }
  libxsmm_dnn_pooling* const h = static_cast<libxsmm_dnn_pooling*>(malloc(sizeof(libxsmm_dnn_pooling)));
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
  h->ofh = 0 != desc.u ? (desc.H + 2 * desc.pad_h - desc.R) / desc.u + 1 : 0;
  h->ofw = 0 != desc.v ? (desc.W + 2 * desc.pad_w - desc.S) / desc.v + 1 : 0;
  const size_t ph = (size_t)(desc.pad_h_in > desc.pad_h_out ? desc.pad_h_in : desc.pad_h_out), pw = (size_t)(desc.pad_w_in > desc.pad_w_out ? desc.pad_w_in : desc.pad_w_out);
  h->scratch_size = sizeof(float) * ((size_t)desc.H + ph * 2) * ((size_t)desc.W + pw * 2) * (size_t)(h->ofmblock > h->ifmblock ? h->ofmblock : h->ifmblock)
                  * (size_t)desc.threads; // :83-86
  return h;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_pooling(const libxsmm_dnn_pooling* handle)
{ // :98-111
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  free(const_cast<libxsmm_dnn_pooling*>(handle));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_pooling_create_tensor_datalayout(const libxsmm_dnn_pooling* h, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :114-291
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dH = LIBXSMM_DNN_TENSOR_DIMTYPE_H, dW = LIBXSMM_DNN_TENSOR_DIMTYPE_W, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* l = static_cast<libxsmm_dnn_tensor_datalayout*>(malloc(sizeof(*l)));
  if (nullptr == l) { *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT; return nullptr; }
  memset(l, 0, sizeof(*l));
  const libxsmm_dnn_pooling_desc& d = h->desc;
  l->format = d.buffer_format;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  const bool f32 = dt_pair(d, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32), mask = LIBXSMM_DNN_POOLING_MASK == type;
  const unsigned int N = (unsigned int)d.N;
  const unsigned int ifwp = (unsigned int)(d.W + 2 * d.pad_w_in), ifhp = (unsigned int)(d.H + 2 * d.pad_h_in);
  const unsigned int ofwp = (unsigned int)(h->ofw + 2 * d.pad_w_out), ofhp = (unsigned int)(h->ofh + 2 * d.pad_h_out);
  bool ok = true; // false: the arrays could not be allocated
  if (!is_input(type) && !is_output(type) && !mask) *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
    if (mask) { // five dimensions over (ofw, ofh), no physical padding; in BF16 too (the reference's sixth size there is uninitialised)
      const D t[5] = { dC, dW, dH, dC, dN };
      const unsigned int s[5] = { (unsigned int)h->ofmblock, (unsigned int)h->ofw, (unsigned int)h->ofh, (unsigned int)h->blocksofm, N };
      l->datatype = d.datatype_mask;
      ok = layout_dims(l, 5, t, s);
    }
    else if (f32) {
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
    // (the reference overwrites the mask's datatype with datatype_in and then has no sizes for a mask: both kept)
    if (mask) *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
    else {
      const D t[4] = { dC, dW, dH, dN };
      const unsigned int in[4] = { (unsigned int)d.C, ifwp, ifhp, N }, out[4] = { (unsigned int)d.C, ofwp, ofhp, N };
      l->datatype = d.datatype_in;
      ok = layout_dims(l, 4, t, is_input(type) ? in : out);
    }
  }
  else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  if (!ok) *status = LIBXSMM_DNN_ERR_CREATE_LAYOUT_ARRAYS;
  if (LIBXSMM_DNN_SUCCESS != *status) { free(l->dim_type); free(l->dim_size); free(l); return nullptr; }
  return l;
}

LIBXSMM_API size_t libxsmm_dnn_pooling_get_scratch_size(const libxsmm_dnn_pooling* handle, libxsmm_dnn_err_t* status)
{ // :293-304 (64 bytes more for a caller that does not align)
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr != handle) return handle->scratch_size + 64;
  *status = LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return 0;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_scratch(libxsmm_dnn_pooling* handle, const void* scratch)
{ // :307-330 (the pointer is kept, aligned as there, and never dereferenced)
  const uintptr_t address = reinterpret_cast<uintptr_t>(scratch);
  if (nullptr == scratch) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  handle->scratch = reinterpret_cast<void*>(0 == address % 64 ? address : address + (64 - address % 64));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_scratch(libxsmm_dnn_pooling* handle)
{ // :333-343
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  handle->scratch = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{ // :346-385
  libxsmm_dnn_err_t status = LIBXSMM_DNN_SUCCESS;
  if (!bindable(type)) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == handle || nullptr == tensor) return LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR;
  libxsmm_dnn_tensor_datalayout* const want = libxsmm_dnn_pooling_create_tensor_datalayout(handle, type, &status);
  if (0 == libxsmm_dnn_compare_tensor_datalayout(want, tensor->layout, &status)) *slot_of(handle, type) = const_cast<libxsmm_dnn_tensor*>(tensor);
  else status = LIBXSMM_DNN_ERR_MISMATCH_TENSOR;
  if (nullptr != want) libxsmm_dnn_destroy_tensor_datalayout(want);
  return status;
}

LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_pooling_get_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :388-420
  *status = LIBXSMM_DNN_SUCCESS;
  if (!bindable(type)) { *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE; return nullptr; }
  if (nullptr == handle) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  return *slot_of(handle, type);
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type)
{ // :423-453
  if (!bindable(type)) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  *slot_of(handle, type) = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_execute_st(libxsmm_dnn_pooling* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{ // :456-492 and the drivers of the two passes (src/libxsmm_dnn_pooling_{forward,backward}.c:108-172)
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind && LIBXSMM_DNN_COMPUTE_KIND_BWD != kind) return LIBXSMM_DNN_ERR_INVALID_KIND;
  const libxsmm_dnn_pooling_desc& d = h->desc;
  if (LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM != d.buffer_format) return LIBXSMM_DNN_ERR_INVALID_FORMAT_FUSEDBN; // (the reference's code for it)
  const bool bwd = LIBXSMM_DNN_COMPUTE_KIND_BWD == kind, is_max = LIBXSMM_DNN_POOLING_MAX == d.pooling_type;
  // the input-side tensor (read by FWD, written by BWD) and the output-side one (written by FWD, read by BWD)
  const libxsmm_dnn_tensor* const ti = bwd ? h->grad_input : h->reg_input;
  const libxsmm_dnn_tensor* const to = bwd ? h->grad_output : h->reg_output;
  if (nullptr == ti || nullptr == to || (nullptr == h->mask && is_max)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (!is_max && LIBXSMM_DNN_POOLING_AVG != d.pooling_type) return LIBXSMM_DNN_ERR_UNSUPPORTED_POOLING;
  // from here on: this engine's own (the scratch is not asked for: nothing is staged through memory)
  const int ltid = tid - start_thread;
  if (ltid < 0 || d.threads < 1) return LIBXSMM_DNN_ERR_GENERAL;
  if (is_max && LIBXSMM_DNN_DATATYPE_I32 != d.datatype_mask) return LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
  // the kernels address pixels of 16 channels on both sides, with 32-bit indices inside a plane
  if (16 != h->ifmblock_hp || h->blocksifm != h->blocksofm) return LIBXSMM_DNN_ERR_GENERAL;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.R < 1 || d.S < 1 || d.u < 1 || d.v < 1 || d.pad_h < 0 || d.pad_w < 0 || d.pad_h_in < 0 || d.pad_w_in < 0
    || d.pad_h_out < 0 || d.pad_w_out < 0 || h->ofh < 1 || h->ofw < 1 || (long long)d.H * d.W >= (1LL << 27) || (long long)h->ofh * h->ofw >= (1LL << 27))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }

  // the share of ltid (the templates' chunksize, thr_begin, thr_end)
  const long long work = (long long)d.N * h->blocksifm;
  const long long chunk = (0 == work % d.threads) ? (work / d.threads) : (work / d.threads + 1);
  const long long b0 = (ltid * chunk < work) ? ltid * chunk : work;
  const long long b1 = ((ltid + 1LL) * chunk < work) ? (ltid + 1LL) * chunk : work;
  if (b0 >= b1) return LIBXSMM_DNN_SUCCESS;
  if (work > 0x7fffffffLL) return LIBXSMM_DNN_ERR_GENERAL;

  if (!device_ready()) { fail_no_device("libxsmm_dnn_pooling_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  Operand oi, oo, om;
  memset(&om, 0, sizeof(om));
  // (a staged destination starts from the caller's bytes: only the share's interior is written, and the whole image travels back)
  if (!operand_in(&oi, ti, 3, true) || !operand_in(&oo, to, 4, true) || (is_max && !operand_in(&om, h->mask, 5, true))) return LIBXSMM_DNN_ERR_GENERAL;
  if (0 != (reinterpret_cast<uintptr_t>(oi.dev) | reinterpret_cast<uintptr_t>(oo.dev) | reinterpret_cast<uintptr_t>(om.dev)) % 16) return LIBXSMM_DNN_ERR_GENERAL;
  PoolArgs g; memset(&g, 0, sizeof(g));
  g.in = oi.dev; g.out = oo.dev; g.mask = om.dev;
  g.H = d.H; g.W = d.W; g.R = d.R; g.S = d.S; g.u = d.u; g.v = d.v; g.pad_h = d.pad_h; g.pad_w = d.pad_w;
  g.iph = d.pad_h_in; g.ipw = d.pad_w_in; g.oph = d.pad_h_out; g.opw = d.pad_w_out;
  g.ofh = h->ofh; g.ofw = h->ofw; g.w0 = (int)b0; g.w1 = (int)b1;
  g.recp = 1.0f / ((float)d.R * (float)d.S);
  g.bwd = bwd ? 1 : 0; g.is_max = is_max ? 1 : 0; g.bf16 = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16) ? 1 : 0;
  const char* name = "";
  const int e = launch_pool(g, stream, &name);
  note_launch(name);
  if (0 != e) {
    fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
    return LIBXSMM_DNN_ERR_GENERAL;
  }
  // what the pass wrote travels back if it was staged: dinput (BWD), output and mask (FWD)
  bool ok = true;
  if (bwd) { if (nullptr != oi.host) ok = 0 == d2h(oi.host, oi.dev, oi.bytes); }
  else {
    if (nullptr != oo.host) ok = 0 == d2h(oo.host, oo.dev, oo.bytes);
    if (ok && nullptr != om.host) ok = 0 == d2h(om.host, om.dev, om.bytes);
  }
  if (!ok) return LIBXSMM_DNN_ERR_GENERAL;
  if (oi.wait || oo.wait || om.wait) return 0 == stream_sync() ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
  return LIBXSMM_DNN_SUCCESS;
}
