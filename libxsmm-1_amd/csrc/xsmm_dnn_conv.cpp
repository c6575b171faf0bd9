// xsmm_dnn_conv.cpp -- the convolution layer (include/libxsmm_dnn_convolution.h): handle, layouts, scratch and tensor binding as
// in the reference's generic path, and libxsmm_dnn_execute_st as one launch of kernels/conv.hip per call (FWD: one per slab of
// 65535 pixel tiles).
//
// Reference: src/libxsmm_dnn.c (create :191-308, layouts :363-997, trans_reg_filter :1571-1604, binding :1607-1717, scratch
// :1720-2097, execute :2100-2235, the helpers :2238-2391), src/libxsmm_dnn_handle.c:61-167 (the scratch sizes of the generic path),
// libxsmm_dnn_setup_generic (src/libxsmm_dnn_setup.c:369-465: the blocks), src/libxsmm_dnn_convolution_{forward,backward,
// weight_update}.c (what must be bound) and src/template/libxsmm_dnn_convolve_st_{fwd,bwd,upd}_custom_custom_generic.tpl.c (the
// split of a pass over logical threads and the arithmetic: DESIGN.md 8n). There a pass is a loop of SMM calls through padded and
// transposed copies in scratch; here the kernels address the blocked tensors where they lie and the scratch is never touched.
// Everything up to execute_st and trans_reg_filter is host-only.
#include "xsmm_dnn_internal.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

struct libxsmm_dnn_layer { // the fields of src/libxsmm_main.h's libxsmm_dnn_layer that have a meaning here
  libxsmm_dnn_conv_desc desc;
  libxsmm_dnn_tensor* reg_input; libxsmm_dnn_tensor* grad_input;
  libxsmm_dnn_tensor* reg_output; libxsmm_dnn_tensor* grad_output;
  libxsmm_dnn_tensor* reg_filter; libxsmm_dnn_tensor* grad_filter; libxsmm_dnn_tensor* reg_filter_tr;
  libxsmm_dnn_tensor* reg_bias; libxsmm_dnn_tensor* grad_bias;
  int ifmblock, ofmblock, blocksifm, blocksofm;
  int ifhp, ifwp, ofh, ofw, ofhp, ofwp;
  size_t scratch1_size, scratch5_size, scratch6_size, scratch7_size; // (scratch2, scratch3 and scratch4 have no bytes in the generic path)
  void* scratch1; void* scratch3;                                     // the two pointers the passes ask for (BWD, UPD)
};

// the tensor a type binds; nullptr: not one of the nine bindable types (at global scope: the templates of xsmm_dnn_internal.hpp
// find it by its argument)
static libxsmm_dnn_tensor** slot_of(libxsmm_dnn_layer* h, libxsmm_dnn_tensor_type t)
{
  switch (t) {
    case LIBXSMM_DNN_REGULAR_INPUT: return &h->reg_input;
    case LIBXSMM_DNN_GRADIENT_INPUT: return &h->grad_input;
    case LIBXSMM_DNN_REGULAR_OUTPUT: return &h->reg_output;
    case LIBXSMM_DNN_GRADIENT_OUTPUT: return &h->grad_output;
    case LIBXSMM_DNN_REGULAR_FILTER: return &h->reg_filter;
    case LIBXSMM_DNN_GRADIENT_FILTER: return &h->grad_filter;
    case LIBXSMM_DNN_REGULAR_FILTER_TRANS: return &h->reg_filter_tr;
    case LIBXSMM_DNN_REGULAR_CHANNEL_BIAS: return &h->reg_bias;
    case LIBXSMM_DNN_GRADIENT_CHANNEL_BIAS: return &h->grad_bias;
    default: return nullptr;
  }
}

namespace {

int block_of(int n)
{ // libxsmm_dnn_setup_generic: n below 16 is its own block, else the largest power of two up to 16 that divides n
  if (n < 16) return n;
  int b = 1;
  for (int t = 1; t <= 16; t *= 2) if (0 == n % t) b = t;
  return b;
}

size_t up64(size_t n) { return (n + 63) & ~(size_t)63; }

bool known_kind(libxsmm_dnn_compute_kind k)
{
  return LIBXSMM_DNN_COMPUTE_KIND_FWD == k || LIBXSMM_DNN_COMPUTE_KIND_BWD == k || LIBXSMM_DNN_COMPUTE_KIND_UPD == k || LIBXSMM_DNN_COMPUTE_KIND_ALL == k;
}

int tile_for(const libxsmm_dnn_layer* h, long long pixels)
{
  // LIBXSMM_AMD_CONV_TILE=64 / 128 forces a tile (read per call: tests and the benchmark compare both). Otherwise the rule of the
  // fully-connected layer: the largest tile that still gives every compute unit a work-group (no measurement stands behind it).
  const char* const e = getenv("LIBXSMM_AMD_CONV_TILE");
  if (nullptr != e) { const int v = atoi(e); if (64 == v || 128 == v) return v; }
  static const int cus = []() {
    int n = 0, dev = 0;
    if (hipSuccess != hipGetDevice(&dev) || hipSuccess != hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)) { (void)hipGetLastError(); n = 0; }
    return 0 < n ? n : 256;
  }();
  const long long big = (((long long)h->desc.K + 127) / 128) * ((pixels + 127) / 128);
  return (h->desc.K > 64 && big >= cus) ? 128 : 64;
}

void fill_args(const libxsmm_dnn_layer* h, ConvArgs* g)
{
  const libxsmm_dnn_conv_desc& d = h->desc;
  memset(g, 0, sizeof(*g));
  g->N = d.N; g->C = d.C; g->K = d.K; g->H = d.H; g->W = d.W; g->R = d.R; g->S = d.S; g->u = d.u; g->v = d.v; g->pad_h = d.pad_h; g->pad_w = d.pad_w;
  g->ifmblock = h->ifmblock; g->ofmblock = h->ofmblock; g->blocksifm = h->blocksifm; g->blocksofm = h->blocksofm;
  g->ifhp = h->ifhp; g->ifwp = h->ifwp; g->ofh = h->ofh; g->ofw = h->ofw; g->ofhp = h->ofhp; g->ofwp = h->ofwp; g->oph = d.pad_h_out; g->opw = d.pad_w_out;
  g->logical = (d.pad_h == d.pad_h_in && d.pad_w == d.pad_w_in) ? 0 : 1;
  g->overwrite = (0 != (d.options & LIBXSMM_DNN_CONV_OPTION_OVERWRITE)) ? 1 : 0;
}

} // namespace

LIBXSMM_API libxsmm_dnn_layer* libxsmm_dnn_create_conv_layer(libxsmm_dnn_conv_desc d, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn.c:191-308
  const auto refuse = [&](libxsmm_dnn_err_t e) { *status = e; return static_cast<libxsmm_dnn_layer*>(nullptr); };
  if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NCHW)) return refuse(LIBXSMM_DNN_ERR_INVALID_FORMAT_NCHW);
  if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_KCRS)) return refuse(LIBXSMM_DNN_ERR_INVALID_FORMAT_KCRS); // (buffer_format, as there)
  if (LIBXSMM_DNN_CONV_ALGO_AUTO != d.algo && LIBXSMM_DNN_CONV_ALGO_DIRECT != d.algo) return refuse(LIBXSMM_DNN_ERR_INVALID_ALGO);
  // from here on: this engine's own (libxsmm_dnn_convolution.h)
  if (LIBXSMM_DNN_DATATYPE_F32 != d.datatype_in || LIBXSMM_DNN_DATATYPE_F32 != d.datatype_out) return refuse(LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE);
  if (LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM != d.buffer_format || LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM != d.filter_format) return refuse(LIBXSMM_DNN_ERR_INVALID_FORMAT_CONVOLVE);
  if (d.N < 1 || d.C < 1 || d.H < 1 || d.W < 1 || d.K < 1 || d.R < 1 || d.S < 1 || d.u < 1 || d.v < 1 || d.threads < 1
    || d.pad_h < 0 || d.pad_w < 0 || d.pad_h_in < 0 || d.pad_w_in < 0 || d.pad_h_out < 0 || d.pad_w_out < 0)
  {
    return refuse(LIBXSMM_DNN_ERR_GENERAL);
  }
  if (!((d.pad_h_in == d.pad_h && d.pad_w_in == d.pad_w) || (0 == d.pad_h_in && 0 == d.pad_w_in))) return refuse(LIBXSMM_DNN_ERR_INVALID_PADDING);
  if (0 != ((int)d.fuse_ops & ~(int)(LIBXSMM_DNN_CONV_FUSE_BIAS | LIBXSMM_DNN_CONV_FUSE_RELU)) || nullptr != d.pre_bn || nullptr != d.post_bn) {
    return refuse(LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_FUSION);
  }
  const long long hp = (long long)d.H + 2LL * d.pad_h, wp = (long long)d.W + 2LL * d.pad_w;
  if (hp < d.R || wp < d.S) return refuse(LIBXSMM_DNN_ERR_GENERAL); // ofh or ofw below 1
  const long long ofh = (hp - d.R) / d.u + 1, ofw = (wp - d.S) / d.v + 1;
  const long long ifhp = (long long)d.H + 2LL * d.pad_h_in, ifwp = (long long)d.W + 2LL * d.pad_w_in, ofhp = ofh + 2LL * d.pad_h_out, ofwp = ofw + 2LL * d.pad_w_out;
  const long long limit = 1LL << 31;
  // (the padded plane the reference works on counts as a tensor: the kernels' row and column arithmetic stays in 32 bits)
  if (ifhp >= limit || ifwp >= limit || ofhp >= limit || ofwp >= limit || hp >= limit || wp >= limit || ifhp * ifwp >= limit || ofhp * ofwp >= limit || hp * wp >= limit
    || (long long)d.N * d.C >= limit || (long long)d.N * d.K >= limit || (long long)d.N * d.C * (ifhp * ifwp) >= limit || (long long)d.N * d.C * (hp * wp) >= limit
    || (long long)d.N * d.K * (ofhp * ofwp) >= limit || (long long)d.R * d.S >= limit || (long long)d.C * d.K >= limit || (long long)d.C * d.K * ((long long)d.R * d.S) >= limit)
  {
    return refuse(LIBXSMM_DNN_ERR_GENERAL);
  }
  libxsmm_dnn_layer* const h = static_cast<libxsmm_dnn_layer*>(malloc(sizeof(libxsmm_dnn_layer)));
  if (nullptr == h) return refuse(LIBXSMM_DNN_ERR_CREATE_HANDLE);
  *status = LIBXSMM_DNN_SUCCESS;
  memset(h, 0, sizeof(*h));
  h->desc = d;
  h->ifmblock = block_of(d.C); h->ofmblock = block_of(d.K);
  h->blocksifm = d.C / h->ifmblock; h->blocksofm = d.K / h->ofmblock;
  h->ifhp = (int)ifhp; h->ifwp = (int)ifwp; h->ofh = (int)ofh; h->ofw = (int)ofw; h->ofhp = (int)ofhp; h->ofwp = (int)ofwp;
  // src/libxsmm_dnn_setup.c:453-454 and src/libxsmm_dnn_handle.c:135-164
  const size_t f = sizeof(float), th = (size_t)d.threads;
  h->scratch1_size = (size_t)d.C * d.K * d.R * d.S * f;
  h->scratch5_size = up64((size_t)hp * wp * h->ifmblock * f) * th;
  const size_t a6 = (size_t)h->ofmblock * ofw * ofh * f, b6 = (size_t)h->ifmblock * d.W * d.H * f;
  h->scratch6_size = up64(a6 > b6 ? a6 : b6) * th;
  const size_t c6 = up64((size_t)ofhp * ofwp * h->ofmblock * f) * th;
  if (h->scratch6_size < c6) h->scratch6_size = c6;
  h->scratch7_size = up64((size_t)d.R * d.S * h->ifmblock * h->ofmblock * f) * th;
  return h;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_conv_layer(const libxsmm_dnn_layer* handle)
{ // :311-327 (a NULL handle is not an error there)
  if (nullptr != handle) free(const_cast<libxsmm_dnn_layer*>(handle));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_create_tensor_datalayout(const libxsmm_dnn_layer* h, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :363-997, the F32 branches of custom format 1
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dH = LIBXSMM_DNN_TENSOR_DIMTYPE_H, dW = LIBXSMM_DNN_TENSOR_DIMTYPE_W, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C,
    dK = LIBXSMM_DNN_TENSOR_DIMTYPE_K, dR = LIBXSMM_DNN_TENSOR_DIMTYPE_R, dS = LIBXSMM_DNN_TENSOR_DIMTYPE_S;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* const l = layout_begin(status);
  if (nullptr == l) return nullptr;
  const libxsmm_dnn_conv_desc& d = h->desc;
  const unsigned int ib = (unsigned int)h->ifmblock, ob = (unsigned int)h->ofmblock, nib = (unsigned int)h->blocksifm, nob = (unsigned int)h->blocksofm;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  l->datatype = LIBXSMM_DNN_DATATYPE_F32;
  bool ok = true; // false: the arrays could not be allocated
  if (is_input(type) || is_output(type)) {
    const D t[5] = { dC, dW, dH, dC, dN };
    const unsigned int in[5] = { ib, (unsigned int)h->ifwp, (unsigned int)h->ifhp, nib, (unsigned int)d.N };
    const unsigned int out[5] = { ob, (unsigned int)h->ofwp, (unsigned int)h->ofhp, nob, (unsigned int)d.N };
    l->format = d.buffer_format; l->tensor_type = LIBXSMM_DNN_ACTIVATION;
    ok = layout_dims(l, 5, t, is_input(type) ? in : out);
  }
  else if (LIBXSMM_DNN_REGULAR_FILTER == type || LIBXSMM_DNN_GRADIENT_FILTER == type || LIBXSMM_DNN_FILTER == type) {
    const D t[6] = { dK, dC, dS, dR, dC, dK };
    const unsigned int s[6] = { ob, ib, (unsigned int)d.S, (unsigned int)d.R, nib, nob };
    l->format = d.filter_format; l->tensor_type = LIBXSMM_DNN_FILTER;
    ok = layout_dims(l, 6, t, s);
  }
  else if (LIBXSMM_DNN_REGULAR_FILTER_TRANS == type) {
    const D t[6] = { dC, dK, dS, dR, dK, dC };
    const unsigned int s[6] = { ib, ob, (unsigned int)d.S, (unsigned int)d.R, nob, nib };
    l->format = d.filter_format; l->tensor_type = LIBXSMM_DNN_REGULAR_FILTER_TRANS;
    ok = layout_dims(l, 6, t, s);
  }
  else if (LIBXSMM_DNN_REGULAR_CHANNEL_BIAS == type || LIBXSMM_DNN_GRADIENT_CHANNEL_BIAS == type || LIBXSMM_DNN_CHANNEL_BIAS == type) {
    const D t[2] = { dC, dC };
    const unsigned int s[2] = { ob, nob };
    l->format = d.buffer_format; l->tensor_type = LIBXSMM_DNN_CHANNEL_SCALAR;
    ok = layout_dims(l, 2, t, s);
  }
  else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  return layout_end(l, ok, status);
}

LIBXSMM_API size_t libxsmm_dnn_get_scratch_size(const libxsmm_dnn_layer* h, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status)
{ // :1720-1808 with use_*_generic != 0, padding_flag == 0, no low precision, no thread-private filters; scratch3 has no bytes
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return 0; }
  const size_t s1 = h->scratch1_size + 64, s3 = 64, s5 = h->scratch5_size + 64, s6 = h->scratch6_size + 64, s7 = h->scratch7_size + 64;
  switch (kind) {
    case LIBXSMM_DNN_COMPUTE_KIND_FWD: return s5 + s6 + s7;
    case LIBXSMM_DNN_COMPUTE_KIND_BWD: return s1 + s5 + s7;
    case LIBXSMM_DNN_COMPUTE_KIND_UPD: return s3 + s5 + s6 + s7;
    case LIBXSMM_DNN_COMPUTE_KIND_ALL: return s1 + s3 + s5 + s6 + s7;
    default: *status = LIBXSMM_DNN_ERR_INVALID_KIND; return 0;
  }
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_bind_scratch(libxsmm_dnn_layer* h, const libxsmm_dnn_compute_kind kind, const void* scratch)
{ // :1811-2052: only which of the pointers a kind sets is kept (they are compared with NULL and never dereferenced)
  if (nullptr == scratch) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (!known_kind(kind)) return LIBXSMM_DNN_ERR_INVALID_KIND;
  void* const p = const_cast<void*>(scratch);
  if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind || LIBXSMM_DNN_COMPUTE_KIND_ALL == kind) h->scratch1 = p;
  if (LIBXSMM_DNN_COMPUTE_KIND_UPD == kind || LIBXSMM_DNN_COMPUTE_KIND_ALL == kind) h->scratch3 = p;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_release_scratch(libxsmm_dnn_layer* h, const libxsmm_dnn_compute_kind kind)
{ // :2055-2097
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (!known_kind(kind)) return LIBXSMM_DNN_ERR_INVALID_KIND;
  if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind || LIBXSMM_DNN_COMPUTE_KIND_ALL == kind) h->scratch1 = nullptr;
  if (LIBXSMM_DNN_COMPUTE_KIND_UPD == kind || LIBXSMM_DNN_COMPUTE_KIND_ALL == kind) h->scratch3 = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

// binding :1607-1717 (get_tensor is declared by the reference's header and defined nowhere in its library: here it follows the other layers)
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_bind_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{
  return bind_tensor(handle, tensor, type, libxsmm_dnn_create_tensor_datalayout);
}
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_get_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{
  return get_tensor(handle, type, status);
}
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_release_tensor(libxsmm_dnn_layer* handle, const libxsmm_dnn_tensor_type type)
{ // (a NULL handle is _ERR_INVALID_HANDLE_TENSOR here, unlike in the other layers)
  libxsmm_dnn_err_t status;
  libxsmm_dnn_tensor** const slot = checked_slot(handle, type, true, LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR, &status);
  if (nullptr != slot) *slot = nullptr;
  return status;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_execute_st(libxsmm_dnn_layer* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{ // :2100-2221 and the drivers of the three passes
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  const bool fwd = LIBXSMM_DNN_COMPUTE_KIND_FWD == kind, bwd = LIBXSMM_DNN_COMPUTE_KIND_BWD == kind, upd = LIBXSMM_DNN_COMPUTE_KIND_UPD == kind;
  if (!fwd && !bwd && !upd) return LIBXSMM_DNN_ERR_INVALID_KIND;
  const libxsmm_dnn_conv_desc& d = h->desc;
  // the activation on the input side, the one on the output side and the filter of the pass
  const libxsmm_dnn_tensor* const ti = bwd ? h->grad_input : h->reg_input;
  const libxsmm_dnn_tensor* const to = fwd ? h->reg_output : h->grad_output;
  const libxsmm_dnn_tensor* tf = upd ? h->grad_filter : h->reg_filter;
  if (nullptr == ti || nullptr == to || nullptr == tf || (bwd && nullptr == h->scratch1) || (upd && nullptr == h->scratch3)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  // from here on: this engine's own
  const bool bias = fwd && 0 != (d.fuse_ops & LIBXSMM_DNN_CONV_FUSE_BIAS);
  const bool trans = bwd && 0 != (d.options & LIBXSMM_DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE);
  if ((bias && nullptr == h->reg_bias) || (trans && nullptr == h->reg_filter_tr)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (trans) tf = h->reg_filter_tr;
  const int ltid = tid - start_thread;
  if (ltid < 0) return LIBXSMM_DNN_ERR_GENERAL;
  const long long work = fwd ? (long long)d.N * h->blocksofm : (bwd ? (long long)d.N * h->blocksifm : (long long)h->blocksifm * h->blocksofm);
  long long b0, b1;
  if (!thread_share(work, d.threads, ltid, &b0, &b1)) return LIBXSMM_DNN_SUCCESS;

  if (!device_ready()) { fail_no_device("libxsmm_dnn_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  // (a staged destination starts from the caller's bytes: only the share is written, and the whole image travels back)
  Staging s;
  const Operand* const oi = s.add(ti);
  const Operand* const oo = s.add(to);
  const Operand* const of = s.add(tf);
  const Operand* const ob = bias ? s.add(h->reg_bias) : nullptr;
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  ConvArgs g;
  fill_args(h, &g);
  g.in = oi->dev; g.out = oo->dev; g.flt = of->dev; g.bias = dev_of(ob);
  g.w0 = (int)b0; g.w1 = (int)b1;
  const char* name = "";
  int e;
  if (fwd) {
    g.bias_on = bias ? 1 : 0; g.relu = (0 != (d.fuse_ops & LIBXSMM_DNN_CONV_FUSE_RELU)) ? 1 : 0;
    g.tile = tile_for(h, (long long)(b1 - 1 - b0 + h->blocksofm) / h->blocksofm * h->ofh * h->ofw);
    e = launch_conv_fwd(g, stream, &name);
  }
  else if (bwd) { g.flt_trans = trans ? 1 : 0; e = launch_conv_bwd(g, stream, &name); }
  else { // upd template :91-92
    const bool physical = (0 == g.logical);
    g.per_image = ((1 == d.R && 1 == d.S && physical) || (1 == d.u && 1 == d.v)) ? 0 : 1;
    e = launch_conv_upd(g, stream, &name);
  }
  if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  const bool ok = fwd ? s.finish({ oo }) : (bwd ? s.finish({ oi }) : s.finish({ of }));
  return ok ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}

LIBXSMM_API void libxsmm_dnn_execute(libxsmm_dnn_layer* handle, libxsmm_dnn_compute_kind kind)
{ // :2224-2235: the logical threads in turn; the shares are launches on one stream
  if (nullptr == handle) return;
  for (int tid = 0; tid < handle->desc.threads; ++tid) {
    if (LIBXSMM_DNN_SUCCESS != libxsmm_dnn_execute_st(handle, kind, 0, tid)) return;
  }
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_trans_reg_filter(const libxsmm_dnn_layer* h)
{ // :1571-1604, on the device
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (nullptr == h->reg_filter || nullptr == h->reg_filter_tr) return LIBXSMM_DNN_ERR_INVALID_TENSOR;
  if (!device_ready()) { fail_no_device("libxsmm_dnn_trans_reg_filter"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream;
  Staging s;
  const Operand* const of = s.add(h->reg_filter);
  const Operand* const ot = s.add(h->reg_filter_tr);
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  ConvArgs g;
  fill_args(h, &g);
  g.flt = of->dev; g.out = ot->dev;
  const char* name = "";
  const int e = launch_conv_trans_filter(g, stream, &name);
  if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  return s.finish({ ot }) ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_transpose_filter(libxsmm_dnn_layer* h, const libxsmm_dnn_tensor_type type)
{ // :2238-2291: it transposes RSCK filters, which create refuses here; the checks before that one are kept
  if (LIBXSMM_DNN_REGULAR_FILTER != type) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (nullptr == h->reg_filter) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (nullptr == h->scratch1) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  return LIBXSMM_DNN_ERR_MISMATCH_TENSOR;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_reduce_wu_filters(libxsmm_dnn_layer* h, const libxsmm_dnn_tensor_type type)
{ // :2294-2329 with upd_use_external_reduce == 0
  if (LIBXSMM_DNN_GRADIENT_FILTER != type) return LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (nullptr == h->grad_filter) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_get_codegen_success(libxsmm_dnn_layer* h, libxsmm_dnn_compute_kind kind)
{ // :2332-2361: the generic path has no generated convolution kernel
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind && LIBXSMM_DNN_COMPUTE_KIND_BWD != kind && LIBXSMM_DNN_COMPUTE_KIND_UPD != kind) return LIBXSMM_DNN_ERR_INVALID_KIND;
  return LIBXSMM_DNN_WARN_FALLBACK;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_get_parallel_tasks(libxsmm_dnn_layer* h, libxsmm_dnn_compute_kind kind, unsigned int* num_tasks)
{ // :2364-2391
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  switch (kind) {
    case LIBXSMM_DNN_COMPUTE_KIND_FWD: *num_tasks = (unsigned int)(h->desc.N * h->blocksofm); return LIBXSMM_DNN_SUCCESS;
    case LIBXSMM_DNN_COMPUTE_KIND_BWD: *num_tasks = (unsigned int)(h->desc.N * h->blocksifm); return LIBXSMM_DNN_SUCCESS;
    case LIBXSMM_DNN_COMPUTE_KIND_UPD: *num_tasks = (unsigned int)(h->blocksifm * h->blocksofm); return LIBXSMM_DNN_SUCCESS;
    default: return LIBXSMM_DNN_ERR_INVALID_KIND;
  }
}
