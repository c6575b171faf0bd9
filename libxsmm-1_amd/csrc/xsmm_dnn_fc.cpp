// xsmm_dnn_fc.cpp -- the fully-connected layer (include/libxsmm_dnn_fullyconnected.h): handle, layouts, scratch and tensor
// binding as in the reference, and libxsmm_dnn_fullyconnected_execute_st as one launch of kernels/fc.hip per call.
//
// Reference: src/libxsmm_dnn_fullyconnected.c (handle rules :46-136, layouts :155-492, scratch :494-544, binding :547-660,
// execute :663-708), src/libxsmm_dnn_fullyconnected_{forward,backward,weight_update}.c (what must be bound, which data types
// run) and src/template/libxsmm_dnn_fullyconnected_st_*_generic.tpl.c (the split of a pass over logical threads). There a
// pass is a loop of SMM / batch-reduce SMM calls per thread with barriers around a transposed copy in scratch; here the
// share of a logical thread is a rectangle of the output (or a range of its blocks inside a bounding rectangle) handed to a
// kernel that addresses the blocked tensors where they lie. Everything up to execute_st is host-only.
#include "xsmm_dnn_internal.hpp"
#include "../../include/libxsmm_dnn_fullyconnected.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

struct libxsmm_dnn_fullyconnected { // the fields of src/libxsmm_main.h:574-597 that have a meaning here
  libxsmm_dnn_fullyconnected_desc desc;
  libxsmm_dnn_tensor* reg_input; libxsmm_dnn_tensor* reg_output;
  libxsmm_dnn_tensor* grad_input; libxsmm_dnn_tensor* grad_output;
  libxsmm_dnn_tensor* reg_filter; libxsmm_dnn_tensor* grad_filter;
  int ifmblock, ifmblock_hp, ofmblock, ofmblock_lp, blocksifm, blocksofm, fm_lp_block;
  int bn, bk, bc;
  size_t scratch_size;
  void* scratch;
};

// the tensor a type binds; nullptr: not one of the six bindable types (at global scope: the templates of xsmm_dnn_internal.hpp
// find it by its argument)
static libxsmm_dnn_tensor** slot_of(libxsmm_dnn_fullyconnected* h, libxsmm_dnn_tensor_type t)
{
  switch (t) {
    case LIBXSMM_DNN_REGULAR_INPUT: return &h->reg_input;
    case LIBXSMM_DNN_GRADIENT_INPUT: return &h->grad_input;
    case LIBXSMM_DNN_REGULAR_OUTPUT: return &h->reg_output;
    case LIBXSMM_DNN_GRADIENT_OUTPUT: return &h->grad_output;
    case LIBXSMM_DNN_REGULAR_FILTER: return &h->reg_filter;
    case LIBXSMM_DNN_GRADIENT_FILTER: return &h->grad_filter;
    default: return nullptr;
  }
}

namespace {

bool dt_pair(const libxsmm_dnn_fullyconnected_desc& d, libxsmm_dnn_datatype in, libxsmm_dnn_datatype out) { return d.datatype_in == in && d.datatype_out == out; }
bool format_packed(const libxsmm_dnn_fullyconnected_desc& d) { return LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED == d.buffer_format && LIBXSMM_DNN_TENSOR_FORMAT_CKPACKED == d.filter_format; }
bool format_custom(const libxsmm_dnn_fullyconnected_desc& d) { return LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM == d.buffer_format && LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM == d.filter_format; }
bool is_filter(libxsmm_dnn_tensor_type t) { return LIBXSMM_DNN_REGULAR_FILTER == t || LIBXSMM_DNN_GRADIENT_FILTER == t || LIBXSMM_DNN_FILTER == t; }

FcDim plain(long long stride) { FcDim d; d.blk = FC_PLAIN; d.outer = 0; d.inner = stride; return d; }
FcDim blocked(int blk, long long outer, long long inner) { FcDim d; d.blk = blk; d.outer = outer; d.inner = inner; return d; }

int tile_for(long long mi, long long mj)
{
  // LIBXSMM_AMD_FC_TILE=64 / 128 forces a tile (read per call: tests and the benchmark compare both). Otherwise the largest
  // tile that still gives every compute unit a work-group, where the problem allows it (no measurement stands behind this
  // rule yet: DESIGN.md 8g).
  const char* const e = getenv("LIBXSMM_AMD_FC_TILE");
  if (nullptr != e) { const int v = atoi(e); if (64 == v || 128 == v) return v; }
  static const int cus = []() {
    int n = 0, dev = 0;
    if (hipSuccess != hipGetDevice(&dev) || hipSuccess != hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)) { (void)hipGetLastError(); n = 0; }
    return 0 < n ? n : 256;
  }();
  const long long big = ((mi + 127) / 128) * ((mj + 127) / 128);
  return big >= cus ? 128 : 64;
}

} // namespace

LIBXSMM_API libxsmm_dnn_fullyconnected* libxsmm_dnn_create_fullyconnected(libxsmm_dnn_fullyconnected_desc desc, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn_fullyconnected.c:46-136
  if (!(dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16) || dt_pair(desc, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32)
     || dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_F32)))
  {
    *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
    return nullptr;
  }
  libxsmm_dnn_fullyconnected* const h = static_cast<libxsmm_dnn_fullyconnected*>(malloc(sizeof(libxsmm_dnn_fullyconnected)));
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_CREATE_HANDLE; return nullptr; }
  *status = LIBXSMM_DNN_SUCCESS;
  memset(h, 0, sizeof(*h));
  h->desc = desc;
  const bool lowp = dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16);
  if (format_packed(desc)) {
    h->bk = desc.bk; h->bn = desc.bn; h->bc = desc.bc;
    // (a block of zero divides nothing: the reference would trap on the modulo; here it falls back like any other misfit)
    if (h->bn <= 0 || 0 != desc.N % h->bn) { h->bn = desc.N; *status = LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_N_BLOCKING; }
    if (h->bc <= 0 || 0 != desc.C % h->bc) { h->bc = desc.C; *status = LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_C_BLOCKING; }
    if (h->bk <= 0 || 0 != desc.K % h->bk) { h->bk = desc.K; *status = LIBXSMM_DNN_WARN_FC_SUBOPTIMAL_K_BLOCKING; }
  }
  else {
    if (0 == desc.C % 16 && 0 == desc.K % 16) { // libxsmm_dnn_get_feature_map_blocks (src/libxsmm_dnn_setup.c:197-252); BF16/F32 asks it for F32/F32
      if (lowp) { h->ifmblock = 8; h->fm_lp_block = 2; }
      else { h->ifmblock = 16; h->fm_lp_block = 1; }
      h->ofmblock = 16;
      h->ifmblock_hp = h->ifmblock * h->fm_lp_block;
      h->ofmblock_lp = h->ofmblock / h->fm_lp_block;
    }
    else if (0 == desc.C % 16 && 1000 == desc.K) { // "a hack for the last FC layer" (:93-99)
      h->ifmblock = 16; h->ifmblock_hp = 16; h->fm_lp_block = 1; h->ofmblock = 10; h->ofmblock_lp = 10;
    }
    else {
      *status = LIBXSMM_DNN_ERR_CREATE_HANDLE;
      free(h);
      return nullptr;
    }
    h->blocksifm = desc.C / (lowp ? h->ifmblock_hp : h->ifmblock);
    h->blocksofm = desc.K / h->ofmblock;
  }
  if (dt_pair(desc, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_F32)) { // :122-127
    h->scratch_size = sizeof(float) * ((size_t)desc.C * (size_t)desc.N + (size_t)desc.C * (size_t)desc.K);
  }
  else {
    const size_t a = ((size_t)desc.C + (size_t)desc.K) * (size_t)desc.N, b = (size_t)desc.C * (size_t)desc.K;
    h->scratch_size = sizeof(float) * (a > b ? a : b);
  }
  return h;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_fullyconnected(const libxsmm_dnn_fullyconnected* handle)
{ // :139-152
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  free(const_cast<libxsmm_dnn_fullyconnected*>(handle));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_fullyconnected_create_tensor_datalayout(const libxsmm_dnn_fullyconnected* h, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :155-492
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dH = LIBXSMM_DNN_TENSOR_DIMTYPE_H, dW = LIBXSMM_DNN_TENSOR_DIMTYPE_W, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C,
          dK = LIBXSMM_DNN_TENSOR_DIMTYPE_K, dR = LIBXSMM_DNN_TENSOR_DIMTYPE_R, dS = LIBXSMM_DNN_TENSOR_DIMTYPE_S;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* const l = layout_begin(status);
  if (nullptr == l) return nullptr;
  l->custom_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM_1;
  const libxsmm_dnn_fullyconnected_desc& d = h->desc;
  const bool f32 = dt_pair(d, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32), mixed = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_F32),
             lowp = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_BF16);
  const unsigned int N = (unsigned int)d.N, Cc = (unsigned int)d.C;
  bool ok = true; // false: the arrays could not be allocated
  if (is_input(type) || is_output(type)) {
    l->format = d.buffer_format;
    if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
      if (f32 || (mixed && is_output(type))) {
        const D t[5] = { dC, dW, dH, dC, dN };
        const unsigned int in[5] = { (unsigned int)h->ifmblock, 1, 1, (unsigned int)h->blocksifm, N }, out[5] = { (unsigned int)h->ofmblock, 1, 1, (unsigned int)h->blocksofm, N };
        l->datatype = f32 ? LIBXSMM_DNN_DATATYPE_F32 : d.datatype_out;
        ok = layout_dims(l, 5, t, is_input(type) ? in : out);
      }
      else if (mixed) {
        const D t[6] = { dC, dC, dW, dH, dC, dN };
        const unsigned int in[6] = { (unsigned int)h->fm_lp_block, (unsigned int)h->ifmblock, 1, 1, (unsigned int)h->blocksifm, N };
        l->datatype = d.datatype_in;
        ok = layout_dims(l, 6, t, in);
      }
      else *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
    }
    else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NHWC)) { // (both sides report C, as the reference does)
      const D t[4] = { dC, dW, dH, dN };
      const unsigned int s[4] = { Cc, 1, 1, N };
      l->datatype = d.datatype_in;
      ok = layout_dims(l, 4, t, s);
    }
    else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED)) {
      if (!f32) *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
      else if (LIBXSMM_DNN_REGULAR_INPUT == type || LIBXSMM_DNN_GRADIENT_INPUT == type) {
        const D t[4] = { dC, dN, dC, dN };
        const unsigned int s[4] = { (unsigned int)h->bc, (unsigned int)h->bn, (unsigned int)(d.C / h->bc), (unsigned int)(d.N / h->bn) };
        l->datatype = LIBXSMM_DNN_DATATYPE_F32;
        ok = layout_dims(l, 4, t, s);
      }
      else if (LIBXSMM_DNN_REGULAR_OUTPUT == type || LIBXSMM_DNN_GRADIENT_OUTPUT == type) {
        const D t[4] = { dK, dN, dK, dN };
        const unsigned int s[4] = { (unsigned int)h->bk, (unsigned int)h->bn, (unsigned int)(d.K / h->bk), (unsigned int)(d.N / h->bn) };
        l->datatype = LIBXSMM_DNN_DATATYPE_F32;
        ok = layout_dims(l, 4, t, s);
      }
      else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else if (is_filter(type)) {
    l->format = d.filter_format;
    l->tensor_type = LIBXSMM_DNN_FILTER;
    if (0 != (d.filter_format & LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM)) {
      if (f32) {
        const D t[6] = { dK, dC, dS, dR, dC, dK };
        const unsigned int s[6] = { (unsigned int)h->ofmblock, (unsigned int)h->ifmblock, 1, 1, (unsigned int)h->blocksifm, (unsigned int)h->blocksofm };
        l->datatype = d.datatype_in;
        ok = layout_dims(l, 6, t, s);
      }
      else if (mixed || lowp) {
        const D t[7] = { dC, dK, dC, dS, dR, dC, dK };
        const unsigned int s[7] = { (unsigned int)h->fm_lp_block, (unsigned int)h->ofmblock, (unsigned int)h->ifmblock, 1, 1, (unsigned int)h->blocksifm, (unsigned int)h->blocksofm };
        l->datatype = LIBXSMM_DNN_DATATYPE_BF16;
        ok = layout_dims(l, 7, t, s);
      }
      else *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
    }
    else if (0 != (d.filter_format & LIBXSMM_DNN_TENSOR_FORMAT_RSCK)) {
      const D t[4] = { dK, dC, dS, dR };
      const unsigned int s[4] = { (unsigned int)(h->ofmblock * h->blocksofm), (unsigned int)(h->ifmblock * h->blocksifm), 1, 1 };
      l->datatype = d.datatype_in;
      ok = layout_dims(l, 4, t, s);
    }
    else if (0 != (d.filter_format & LIBXSMM_DNN_TENSOR_FORMAT_CKPACKED)) {
      if (!f32) *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
      else if (LIBXSMM_DNN_REGULAR_FILTER == type || LIBXSMM_DNN_GRADIENT_FILTER == type) {
        const D t[4] = { dK, dC, dC, dK };
        const unsigned int s[4] = { (unsigned int)h->bk, (unsigned int)h->bc, (unsigned int)(d.C / h->bc), (unsigned int)(d.K / h->bk) };
        l->datatype = LIBXSMM_DNN_DATATYPE_F32;
        ok = layout_dims(l, 4, t, s);
      }
      else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  return layout_end(l, ok, status);
}

// scratch :494-544 (kept, aligned as there, and never dereferenced) and binding :547-660
LIBXSMM_API size_t libxsmm_dnn_fullyconnected_get_scratch_size(const libxsmm_dnn_fullyconnected* handle, libxsmm_dnn_err_t* status) { return scratch_size_of(handle, status); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_bind_scratch(libxsmm_dnn_fullyconnected* handle, const void* scratch) { return bind_scratch(handle, scratch); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_release_scratch(libxsmm_dnn_fullyconnected* handle) { return release_scratch(handle); }
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_bind_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{
  return bind_tensor(handle, tensor, type, libxsmm_dnn_fullyconnected_create_tensor_datalayout);
}
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_fullyconnected_get_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{
  return get_tensor(handle, type, status);
}
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_release_tensor(libxsmm_dnn_fullyconnected* handle, const libxsmm_dnn_tensor_type type) { return release_tensor(handle, type); }

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_fullyconnected_execute_st(libxsmm_dnn_fullyconnected* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{ // :663-708 and the drivers of the three passes
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind && LIBXSMM_DNN_COMPUTE_KIND_BWD != kind && LIBXSMM_DNN_COMPUTE_KIND_UPD != kind) return LIBXSMM_DNN_ERR_INVALID_KIND;
  const libxsmm_dnn_fullyconnected_desc& d = h->desc;
  const bool custom = format_custom(d), packed = format_packed(d);
  if (!custom && !packed) return LIBXSMM_DNN_ERR_INVALID_FORMAT_FC;
  // what the pass reads (tp, tq) and writes (td); BWD and UPD ask for a bound scratch as the reference does (it is not used)
  const libxsmm_dnn_tensor *tp, *tq, *td;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD == kind) { tp = h->reg_filter; tq = h->reg_input; td = h->reg_output; }
  else if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind) { tp = h->reg_filter; tq = h->grad_output; td = h->grad_input; }
  else { tp = h->grad_output; tq = h->reg_input; td = h->grad_filter; }
  if (nullptr == tp || nullptr == tq || nullptr == td || (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind && nullptr == h->scratch)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  const bool f32 = dt_pair(d, LIBXSMM_DNN_DATATYPE_F32, LIBXSMM_DNN_DATATYPE_F32), mixed = dt_pair(d, LIBXSMM_DNN_DATATYPE_BF16, LIBXSMM_DNN_DATATYPE_F32);
  if (!(f32 || (mixed && custom))) return LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE;
  if (LIBXSMM_DNN_FULLYCONNECTED_FUSE_NONE != d.fuse_ops) return LIBXSMM_DNN_ERR_FUSEBN_UNSUPPORTED_FUSION;
  const int ltid = tid - start_thread;
  if (ltid < 0 || d.threads < 1) return LIBXSMM_DNN_ERR_GENERAL;
  if (d.N < 1 || d.C < 1 || d.K < 1) return LIBXSMM_DNN_SUCCESS;

  // the tensors as two-level strided functions of n, c, k
  const long long N = d.N, Cc = d.C, K = d.K;
  const int bc = custom ? h->ifmblock * h->fm_lp_block : h->bc, bk = custom ? h->ofmblock : h->bk, bn = custom ? 1 : h->bn;
  const int nbc = (int)(Cc / bc), nbk = (int)(K / bk), nbn = (int)(N / bn);
  const FcDim w_k = blocked(bk, Cc * bk, 1), w_c = blocked(bc, (long long)bc * bk, bk);           // [K/bk][C/bc][bc][bk]
  const FcDim x_n = custom ? plain(Cc) : blocked(bn, Cc * bn, bc), x_c = custom ? plain(1) : blocked(bc, (long long)bn * bc, 1);  // [N][C] or [N/bn][C/bc][bn][bc]
  const FcDim y_n = custom ? plain(K) : blocked(bn, K * bn, bk), y_k = custom ? plain(1) : blocked(bk, (long long)bn * bk, 1);    // [N][K] or [N/bn][K/bk][bn][bk]

  FcArgs g; memset(&g, 0, sizeof(g));
  long long mi, mj;   // extents of D
  int work;           // blocks of the output the reference hands out
  // the block number of an element of D: (i / sbi) * bmi + (j / sbj) * bmj
  int sbi, bmi, sbj, bmj;
  bool i_major = false; // of two numbered indices, the one whose blocks are counted in whole rows of the other's
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD == kind) { // D(k, n) = chain over c of w(k, c) * x(c, n)
    g.pi = w_k; g.pr = w_c; g.qr = x_c; g.qj = x_n; g.di = y_k; g.dj = y_n; g.R = (int)Cc; mi = K; mj = N;
    g.p_bf16 = g.q_bf16 = mixed ? 1 : 0; g.d_bf16 = 0; g.p_rfast = 0; g.q_rfast = 1;
    sbi = bk; sbj = bn;
    if (custom) { work = nbk; bmi = 1; bmj = 0; } else { work = nbk * nbn; bmi = 1; bmj = nbk; } // mb1 * nBlocksOFm + ofm1
  }
  else if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind) { // D(c, n) = chain over k of w(c, k) * dy(k, n)
    g.pi = w_c; g.pr = w_k; g.qr = y_k; g.qj = y_n; g.di = x_c; g.dj = x_n; g.R = (int)K; mi = Cc; mj = N;
    g.p_bf16 = mixed ? 1 : 0; g.q_bf16 = 0; g.d_bf16 = mixed ? 1 : 0; g.p_rfast = 1; g.q_rfast = 1;
    sbi = bc; sbj = bn;
    if (custom) { work = nbc; bmi = 1; bmj = 0; } else { work = nbc * nbn; bmi = 1; bmj = nbc; } // mb1 * nBlocksIFm + ifm1
  }
  else { // D(k, c) = chain over n of dy(k, n) * x(n, c)
    g.pi = y_k; g.pr = y_n; g.qr = x_n; g.qj = x_c; g.di = w_k; g.dj = w_c; g.R = (int)N; mi = K; mj = Cc;
    g.p_bf16 = 0; g.q_bf16 = mixed ? 1 : 0; g.d_bf16 = mixed ? 1 : 0; g.p_rfast = 0; g.q_rfast = 0;
    sbi = bk; sbj = bc;
    work = nbc * nbk; bmi = nbc; bmj = 1; i_major = true; // ofm1 * nBlocksIFm + ifm1
  }

  long long b0, b1;
  if (!thread_share(work, d.threads, ltid, &b0, &b1)) return LIBXSMM_DNN_SUCCESS;
  g.i0 = 0; g.i1 = (int)mi; g.j0 = 0; g.j1 = (int)mj;
  g.masked = 0; g.sbi = sbi; g.mi = bmi; g.sbj = sbj; g.mj = bmj; g.w0 = (int)b0; g.w1 = (int)b1;
  if (0 != b0 || work != b1) { // the bounding rectangle of the blocks b0 .. b1-1; masked: the range is no rectangle
    if (0 == bmj) { g.i0 = (int)b0 * sbi; g.i1 = (int)b1 * sbi; }
    else {
      const int minor = i_major ? bmi : bmj;
      const int r0 = (int)(b0 / minor), r1 = (int)((b1 - 1) / minor), c0 = (int)(b0 % minor), c1 = (int)((b1 - 1) % minor);
      int lo_major = r0, hi_major = r1 + 1, lo_minor = 0, hi_minor = minor;
      if (r0 == r1) { lo_minor = c0; hi_minor = c1 + 1; }
      else if (0 != c0 || minor - 1 != c1) g.masked = 1;
      const int smajor = i_major ? sbi : sbj, sminor = i_major ? sbj : sbi;
      const int a0 = lo_major * smajor, a1 = hi_major * smajor, m0 = lo_minor * sminor, m1 = hi_minor * sminor;
      if (i_major) { g.i0 = a0; g.i1 = a1; g.j0 = m0; g.j1 = m1; } else { g.j0 = a0; g.j1 = a1; g.i0 = m0; g.i1 = m1; }
    }
  }

  if (!device_ready()) { fail_no_device("libxsmm_dnn_fullyconnected_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  // (a staged destination starts from the caller's bytes: only the share is written, and the whole image travels back)
  Staging s;
  const Operand* const op = s.add(tp);
  const Operand* const oq = s.add(tq);
  const Operand* const od = s.add(td);
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  g.p = op->dev; g.q = oq->dev; g.d = od->dev;
  g.tile = tile_for(g.i1 - g.i0, g.j1 - g.j0);
  const char* name = "";
  const int e = launch_fc(g, stream, &name);
  if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  return s.finish({ od }) ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}
