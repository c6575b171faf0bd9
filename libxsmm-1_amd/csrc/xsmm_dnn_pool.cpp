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
  FmBlocks fm;
  int ofh, ofw;
  size_t scratch_size;
  void* scratch;
};

// the tensor a type binds; nullptr: not one of the five bindable types (at global scope: the templates of xsmm_dnn_internal.hpp
// find it by its argument)
static libxsmm_dnn_tensor** slot_of(libxsmm_dnn_pooling* h, libxsmm_dnn_tensor_type t)
{
  switch (t) {
    case LIBXSMM_DNN_REGULAR_INPUT: return &h->reg_input;
    case LIBXSMM_DNN_GRADIENT_INPUT: return &h->grad_input;
    case LIBXSMM_DNN_REGULAR_OUTPUT: return &h->reg_output;
    case LIBXSMM_DNN_GRADIENT_OUTPUT: return &h->grad_output;
    case LIBXSMM_DNN_POOLING_MASK: return &h->mask;
    default: return nullptr;
  }
}

namespace {

bool dt_pair(const libxsmm_dnn_pooling_desc& d, libxsmm_dnn_datatype in, libxsmm_dnn_datatype out) { return d.datatype_in == in && d.datatype_out == out; }

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
  h->fm = feature_map_blocks(desc.C, f32);
  h->ofh = 0 != desc.u ? (desc.H + 2 * desc.pad_h - desc.R) / desc.u + 1 : 0;
  h->ofw = 0 != desc.v ? (desc.W + 2 * desc.pad_w - desc.S) / desc.v + 1 : 0;
  const size_t ph = (size_t)(desc.pad_h_in > desc.pad_h_out ? desc.pad_h_in : desc.pad_h_out), pw = (size_t)(desc.pad_w_in > desc.pad_w_out ? desc.pad_w_in : desc.pad_w_out);
  h->scratch_size = sizeof(float) * ((size_t)desc.H + ph * 2) * ((size_t)desc.W + pw * 2) * (size_t)(h->fm.ofmblock > h->fm.ifmblock ? h->fm.ofmblock : h->fm.ifmblock)
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
  libxsmm_dnn_tensor_datalayout* const l = layout_begin(status);
  if (nullptr == l) return nullptr;
  const libxsmm_dnn_pooling_desc& d = h->desc;
  l->format = d.buffer_format;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  bool ok = true; // false: the arrays could not be allocated
  if (is_input(type) || is_output(type)) {
    ok = activation_layout(l, d.buffer_format, d.datatype_in, d.datatype_out, h->fm, d.N, d.C, is_input(type), (unsigned int)(d.H + 2 * d.pad_h_in),
                           (unsigned int)(d.W + 2 * d.pad_w_in), (unsigned int)(h->ofh + 2 * d.pad_h_out), (unsigned int)(h->ofw + 2 * d.pad_w_out), status);
  }
  else if (LIBXSMM_DNN_POOLING_MASK != type) *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
    // five dimensions over (ofw, ofh), no physical padding; in BF16 too (the reference's sixth size there is uninitialised)
    const D t[5] = { dC, dW, dH, dC, dN };
    const unsigned int s[5] = { (unsigned int)h->fm.ofmblock, (unsigned int)h->ofw, (unsigned int)h->ofh, (unsigned int)h->fm.blocksofm, (unsigned int)d.N };
    l->datatype = d.datatype_mask;
    ok = layout_dims(l, 5, t, s);
  }
  // (NHWC: the reference overwrites the mask's datatype with datatype_in and then has no sizes for a mask: both kept)
  else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NHWC)) *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  return layout_end(l, ok, status);
}

// scratch :293-343 (kept, aligned as there, and never dereferenced) and binding :346-453
LIBXSMM_API size_t libxsmm_dnn_pooling_get_scratch_size(const libxsmm_dnn_pooling* handle, libxsmm_dnn_err_t* status) { return scratch_size_of(handle, status); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_scratch(libxsmm_dnn_pooling* handle, const void* scratch) { return bind_scratch(handle, scratch); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_scratch(libxsmm_dnn_pooling* handle) { return release_scratch(handle); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_bind_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{
  return bind_tensor(handle, tensor, type, libxsmm_dnn_pooling_create_tensor_datalayout);
}
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_pooling_get_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{
  return get_tensor(handle, type, status);
}
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_pooling_release_tensor(libxsmm_dnn_pooling* handle, const libxsmm_dnn_tensor_type type) { return release_tensor(handle, type); }

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
  if (16 != h->fm.ifmblock_hp || h->fm.blocksifm != h->fm.blocksofm) return LIBXSMM_DNN_ERR_GENERAL;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.R < 1 || d.S < 1 || d.u < 1 || d.v < 1 || d.pad_h < 0 || d.pad_w < 0 || d.pad_h_in < 0 || d.pad_w_in < 0
    || d.pad_h_out < 0 || d.pad_w_out < 0 || h->ofh < 1 || h->ofw < 1 || (long long)d.H * d.W >= (1LL << 27) || (long long)h->ofh * h->ofw >= (1LL << 27))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }

  const long long work = (long long)d.N * h->fm.blocksifm;
  long long b0, b1;
  if (!thread_share(work, d.threads, ltid, &b0, &b1)) return LIBXSMM_DNN_SUCCESS;
  if (work > 0x7fffffffLL) return LIBXSMM_DNN_ERR_GENERAL;

  if (!device_ready()) { fail_no_device("libxsmm_dnn_pooling_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  // (a staged destination starts from the caller's bytes: only the share's interior is written, and the whole image travels back)
  Staging s;
  const Operand* const oi = s.add(ti);
  const Operand* const oo = s.add(to);
  const Operand* const om = is_max ? s.add(h->mask) : nullptr;
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  if (!aligned16(oi) || !aligned16(oo) || !aligned16(om)) return LIBXSMM_DNN_ERR_GENERAL;
  PoolArgs g; memset(&g, 0, sizeof(g));
  g.in = oi->dev; g.out = oo->dev; g.mask = dev_of(om);
  g.H = d.H; g.W = d.W; g.R = d.R; g.S = d.S; g.u = d.u; g.v = d.v; g.pad_h = d.pad_h; g.pad_w = d.pad_w;
  g.iph = d.pad_h_in; g.ipw = d.pad_w_in; g.oph = d.pad_h_out; g.opw = d.pad_w_out;
  g.ofh = h->ofh; g.ofw = h->ofw; g.w0 = (int)b0; g.w1 = (int)b1;
  g.recp = 1.0f / ((float)d.R * (float)d.S);
  g.bwd = bwd ? 1 : 0; g.is_max = is_max ? 1 : 0; g.bf16 = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16) ? 1 : 0;
  const char* name = "";
  const int e = launch_pool(g, stream, &name);
  if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  // what the pass wrote travels back if it was staged: dinput (BWD), output and mask (FWD)
  const bool ok = bwd ? s.finish({ oi }) : s.finish({ oo, om });
  return ok ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}
