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
  FmBlocks fm;
  size_t scratch_size;
  void* scratch;
  float* partials; // device memory of this handle: per logical thread 2 * 16 * blocks * N floats; allocated by the first execute_st
};

// the tensor a type binds; nullptr: not one of the thirteen bindable types (at global scope: the templates of
// xsmm_dnn_internal.hpp find it by its argument)
static libxsmm_dnn_tensor** slot_of(libxsmm_dnn_fusedbatchnorm* h, libxsmm_dnn_tensor_type t)
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

namespace {

std::mutex partials_lock; // the first execute_st of a handle may come from several threads at once

bool dt_pair(const libxsmm_dnn_fusedbatchnorm_desc& d, libxsmm_dnn_datatype in, libxsmm_dnn_datatype out) { return d.datatype_in == in && d.datatype_out == out; }
bool is_add(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_INPUT_ADD == t || LIBXSMM_DNN_GRADIENT_INPUT_ADD == t; } // laid out as the input
bool is_channel(libxsmm_dnn_tensor_type t)
{
  return LIBXSMM_DNN_REGULAR_CHANNEL_BETA == t || LIBXSMM_DNN_GRADIENT_CHANNEL_BETA == t || LIBXSMM_DNN_CHANNEL_BETA == t
      || LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA == t || LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA == t || LIBXSMM_DNN_CHANNEL_GAMMA == t
      || LIBXSMM_DNN_CHANNEL_EXPECTVAL == t || LIBXSMM_DNN_CHANNEL_RCPSTDDEV == t || LIBXSMM_DNN_CHANNEL_VARIANCE == t;
}

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
  h->fm = feature_map_blocks(desc.C, f32);
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
  const D dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* const l = layout_begin(status);
  if (nullptr == l) return nullptr;
  const libxsmm_dnn_fusedbatchnorm_desc& d = h->desc;
  l->format = d.buffer_format;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  const bool input = is_input(type) || is_add(type);
  bool ok = true; // false: the arrays could not be allocated
  if (input || is_output(type)) {
    // (a stride of zero divides nothing: the reference would trap; here the output has its padding only)
    ok = activation_layout(l, d.buffer_format, d.datatype_in, d.datatype_out, h->fm, d.N, d.C, input, (unsigned int)(d.H + 2 * d.pad_h_in),
                           (unsigned int)(d.W + 2 * d.pad_w_in), (unsigned int)((0 != d.u ? d.H / d.u : 0) + 2 * d.pad_h_out),
                           (unsigned int)((0 != d.v ? d.W / d.v : 0) + 2 * d.pad_w_out), status);
  }
  else if (is_channel(type)) {
    l->tensor_type = LIBXSMM_DNN_CHANNEL_SCALAR;
    if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
      if (LIBXSMM_DNN_DATATYPE_F32 == d.datatype_stats) {
        const D t[2] = { dC, dC };
        const unsigned int s[2] = { (unsigned int)(h->fm.ifmblock * h->fm.fm_lp_block), (unsigned int)h->fm.blocksifm };
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
  return layout_end(l, ok, status);
}

// scratch :316-365 (kept, aligned as there, and never dereferenced) and binding :369-536
LIBXSMM_API size_t libxsmm_dnn_fusedbatchnorm_get_scratch_size(const libxsmm_dnn_fusedbatchnorm* handle, libxsmm_dnn_err_t* status) { return scratch_size_of(handle, status); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_scratch(libxsmm_dnn_fusedbatchnorm* handle, const void* scratch) { return bind_scratch(handle, scratch); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_scratch(libxsmm_dnn_fusedbatchnorm* handle) { return release_scratch(handle); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_bind_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{
  return bind_tensor(handle, tensor, type, libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout);
}
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_fusedbatchnorm_get_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{
  return get_tensor(handle, type, status);
}
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fusedbatchnorm_release_tensor(libxsmm_dnn_fusedbatchnorm* handle, const libxsmm_dnn_tensor_type type) { return release_tensor(handle, type); }

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
  if (16 != h->fm.ifmblock_hp || h->fm.blocksifm != h->fm.blocksofm) return LIBXSMM_DNN_ERR_GENERAL;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.u < 1 || d.v < 1 || d.pad_h_in < 0 || d.pad_w_in < 0 || d.pad_h_out < 0 || d.pad_w_out < 0
    || 0 != d.H % d.u || 0 != d.W % d.v || (long long)d.H * d.W >= (1LL << 27))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }

  const long long blocks = h->fm.blocksifm, work = (long long)d.N * blocks;
  long long b0, b1;
  if (!thread_share(work, d.threads, ltid, &b0, &b1)) return LIBXSMM_DNN_SUCCESS;
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
  const Operand* const ox = s.add(h->reg_input);
  const Operand* const ogamma = s.add(h->reg_gamma);
  const Operand* const omean = s.add(h->expvalue);
  const Operand* const orstd = s.add(h->rcpstddev);
  const Operand *obeta = nullptr, *ovar = nullptr, *oout = nullptr, *oadd = nullptr, *odout = nullptr, *odin = nullptr, *odgamma = nullptr, *odbeta = nullptr;
  if (!bwd) {
    obeta = s.add(h->reg_beta); ovar = s.add(h->variance); oout = s.add(h->reg_output);
    if (eltwise) oadd = s.add(h->reg_add);
  }
  else {
    odout = s.add(h->grad_output); odin = s.add(h->grad_input);
    odgamma = s.add(h->grad_gamma); odbeta = s.add(h->grad_beta);
    if (eltwise) oadd = s.add(h->grad_add);
    if (relu) oout = s.add(h->reg_output);
  }
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  if (!aligned16(ox) || !aligned16(oout) || !aligned16(oadd) || !aligned16(odout) || !aligned16(odin) || !aligned16(ogamma) || !aligned16(obeta)
    || !aligned16(omean) || !aligned16(orstd) || !aligned16(ovar) || !aligned16(odgamma) || !aligned16(odbeta))
  {
    return LIBXSMM_DNN_ERR_GENERAL;
  }
  BnArgs g; memset(&g, 0, sizeof(g));
  g.in = ox->dev; g.add = dev_of(oadd); g.out = dev_of(oout); g.dout = dev_of(odout); g.din = dev_of(odin);
  g.gamma = static_cast<float*>(ogamma->dev); g.beta = static_cast<float*>(dev_of(obeta));
  g.mean = static_cast<float*>(omean->dev); g.rstd = static_cast<float*>(orstd->dev); g.var = static_cast<float*>(dev_of(ovar));
  g.dgamma = static_cast<float*>(dev_of(odgamma)); g.dbeta = static_cast<float*>(dev_of(odbeta));
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
    if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  // what the pass wrote travels back if it was staged
  bool ok;
  if (!bwd) ok = stats ? s.finish({ oout, omean, orstd, ovar }) : s.finish({ oout });
  else ok = stats ? s.finish({ odin, odgamma, odbeta, relu ? odout : nullptr, eltwise ? oadd : nullptr }) : s.finish({ odin });
  return ok ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}
