// xsmm_dnn_rnn.cpp -- the RNN cell layer (include/libxsmm_dnn_rnncell.h): handle, layouts, scratch, internal state and tensor
// binding as in the reference, and the forward pass of libxsmm_dnn_rnncell_execute_st as launches of kernels/rnn.hip, one per step
// (GRU: two) plus, in the split plan, one ahead of them; BWD, UPD and BWDUPD of the simple cells and the LSTM as launches of
// kernels/rnn_bwd.hip (execute_backward).
//
// Reference: src/libxsmm_dnn_rnncell.c (create :48-137, layouts :155-841, scratch :844-1700, internal state :1703-1928, binding
// :1931-2187, sequence length :2190-2217, execute :2220-2258), src/libxsmm_dnn_rnncell_forward.c:218-272 and the templates
// src/template/libxsmm_dnn_rnncell_st_{rnn,lstm,gru}_fwd_nc_ck_generic.tpl.c. There the threads of a call meet at barriers after
// every step and split (N/bn) * (K/bk); here every call is complete in itself and owns rows of the minibatch.
// Everything up to execute_st is host-only, and execute_st's own checks come before any device probe.
#include "xsmm_dnn_internal.hpp"
#include "../../include/libxsmm_dnn_rnncell.h"

#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace xsmm;

struct libxsmm_dnn_rnncell { // the fields of src/libxsmm_main.h's libxsmm_dnn_rnncell that have a meaning here
  libxsmm_dnn_rnncell_desc desc;
  int T, bk, bn, bc;
  float forget_bias;
  libxsmm_dnn_tensor* xt; libxsmm_dnn_tensor* csp; libxsmm_dnn_tensor* hp; libxsmm_dnn_tensor* w; libxsmm_dnn_tensor* r;
  libxsmm_dnn_tensor* wt; libxsmm_dnn_tensor* rt; libxsmm_dnn_tensor* b; libxsmm_dnn_tensor* cst; libxsmm_dnn_tensor* ht;
  libxsmm_dnn_tensor* dxt; libxsmm_dnn_tensor* dcsp; libxsmm_dnn_tensor* dhp; libxsmm_dnn_tensor* dw; libxsmm_dnn_tensor* dr;
  libxsmm_dnn_tensor* db; libxsmm_dnn_tensor* dcs; libxsmm_dnn_tensor* dht;
  libxsmm_dnn_tensor* it; libxsmm_dnn_tensor* ft; libxsmm_dnn_tensor* ot; libxsmm_dnn_tensor* cit; libxsmm_dnn_tensor* cot;
  void* scratch_base; // as bound (never dereferenced)
  void* internal_z;   // aligned to 64
  float* deltas;      // device, [max_T][N][G * K]: the deltas of a backward pass (allocated by the first one, freed by destroy)
};

// the tensor a type binds; nullptr: not one of the 23 RNN types (at global scope: checked_slot finds it by its argument)
static libxsmm_dnn_tensor** slot_of(libxsmm_dnn_rnncell* h, libxsmm_dnn_tensor_type t)
{
  switch (t) {
    case LIBXSMM_DNN_RNN_REGULAR_INPUT: return &h->xt;
    case LIBXSMM_DNN_RNN_REGULAR_CS_PREV: return &h->csp;
    case LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV: return &h->hp;
    case LIBXSMM_DNN_RNN_REGULAR_WEIGHT: return &h->w;
    case LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT: return &h->r;
    case LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS: return &h->wt;
    case LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT_TRANS: return &h->rt;
    case LIBXSMM_DNN_RNN_REGULAR_BIAS: return &h->b;
    case LIBXSMM_DNN_RNN_REGULAR_CS: return &h->cst;
    case LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE: return &h->ht;
    case LIBXSMM_DNN_RNN_GRADIENT_INPUT: return &h->dxt;
    case LIBXSMM_DNN_RNN_GRADIENT_CS_PREV: return &h->dcsp;
    case LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV: return &h->dhp;
    case LIBXSMM_DNN_RNN_GRADIENT_WEIGHT: return &h->dw;
    case LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT: return &h->dr;
    case LIBXSMM_DNN_RNN_GRADIENT_BIAS: return &h->db;
    case LIBXSMM_DNN_RNN_GRADIENT_CS: return &h->dcs;
    case LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE: return &h->dht;
    case LIBXSMM_DNN_RNN_INTERNAL_I: return &h->it;
    case LIBXSMM_DNN_RNN_INTERNAL_F: return &h->ft;
    case LIBXSMM_DNN_RNN_INTERNAL_O: return &h->ot;
    case LIBXSMM_DNN_RNN_INTERNAL_CI: return &h->cit;
    case LIBXSMM_DNN_RNN_INTERNAL_CO: return &h->cot;
    default: return nullptr;
  }
}

namespace {

typedef libxsmm_dnn_tensor_type TT;

bool is_simple(int cell) { return LIBXSMM_DNN_RNNCELL_RNN_RELU == cell || LIBXSMM_DNN_RNNCELL_RNN_SIGMOID == cell || LIBXSMM_DNN_RNNCELL_RNN_TANH == cell; }
int gates_of(int cell) { return LIBXSMM_DNN_RNNCELL_LSTM == cell ? 4 : (LIBXSMM_DNN_RNNCELL_GRU == cell ? 3 : 1); }
bool is_x(TT t) { return LIBXSMM_DNN_RNN_REGULAR_INPUT == t || LIBXSMM_DNN_RNN_GRADIENT_INPUT == t; }
bool is_state(TT t)
{ // the activations with K features
  switch (t) {
    case LIBXSMM_DNN_RNN_REGULAR_CS_PREV: case LIBXSMM_DNN_RNN_GRADIENT_CS_PREV: case LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV:
    case LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV: case LIBXSMM_DNN_RNN_REGULAR_CS: case LIBXSMM_DNN_RNN_GRADIENT_CS:
    case LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE: case LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE: case LIBXSMM_DNN_RNN_INTERNAL_I:
    case LIBXSMM_DNN_RNN_INTERNAL_F: case LIBXSMM_DNN_RNN_INTERNAL_O: case LIBXSMM_DNN_RNN_INTERNAL_CI: case LIBXSMM_DNN_RNN_INTERNAL_CO: return true;
    default: return false;
  }
}
bool is_w(TT t) { return LIBXSMM_DNN_RNN_REGULAR_WEIGHT == t || LIBXSMM_DNN_RNN_GRADIENT_WEIGHT == t; }
bool is_r(TT t) { return LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT == t || LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT == t; }
bool is_bias(TT t) { return LIBXSMM_DNN_RNN_REGULAR_BIAS == t || LIBXSMM_DNN_RNN_GRADIENT_BIAS == t; }

enum KindClass { KIND_FWD, KIND_REST, KIND_UNKNOWN };
KindClass kind_class(libxsmm_dnn_compute_kind k)
{
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD == k) return KIND_FWD;
  if (LIBXSMM_DNN_COMPUTE_KIND_BWD == k || LIBXSMM_DNN_COMPUTE_KIND_UPD == k || LIBXSMM_DNN_COMPUTE_KIND_BWDUPD == k || LIBXSMM_DNN_COMPUTE_KIND_ALL == k) return KIND_REST;
  return KIND_UNKNOWN;
}

// the reference's reduction blocking (lstm template :156-176, gru template :134-154)
int blocking_factor(int C, int K, int cblocks, int kblocks)
{
  int bf = 1;
  if ((C > 1024 && C <= 2048) || (K > 1024 && K <= 2048)) { bf = 8; while (0 != cblocks % bf || 0 != kblocks % bf) --bf; }
  if (C > 2048 || K > 2048) { bf = 16; while (0 != cblocks % bf || 0 != kblocks % bf) --bf; }
  if (2048 == C && 1024 == K) bf = 2;
  return bf;
}

// the chain order of a cell; adjacent pieces of one operand are one segment
int build_segments(int cell, int C, int K, int bc, int bk, RnnSeg* seg)
{
  int n = 0;
  const auto add = [&](int which, int start, int len) {
    if (len <= 0) return;
    if (n > 0 && seg[n - 1].which == which && seg[n - 1].start + seg[n - 1].len == start) { seg[n - 1].len += len; return; }
    seg[n].which = which; seg[n].start = start; seg[n].len = len; ++n;
  };
  if (bc < 1 || bk < 1 || 0 != C % bc || 0 != K % bk) return 0;
  if (is_simple(cell)) { add(0, 0, C); add(1, 0, K); return n; }
  const int cblocks = C / bc, kblocks = K / bk, bf = blocking_factor(C, K, cblocks, kblocks);
  const int wlen = cblocks / bf * bc, rlen = kblocks / bf * bk;
  const bool alternate = LIBXSMM_DNN_RNNCELL_GRU == cell || (2048 == C && 2048 == K);
  if (alternate) for (int cb = 0; cb < bf; ++cb) { add(0, cb * wlen, wlen); add(1, cb * rlen, rlen); }
  else { add(0, 0, bf * wlen); add(1, 0, bf * rlen); }
  return n;
}

} // namespace

LIBXSMM_API int libxsmm_amd_rnn_segments(libxsmm_dnn_rnncell_type cell_type, int C, int K, int bc, int bk, int phase, int* segments, int capacity)
{
  RnnSeg seg[RNN_MAX_SEG];
  (void)phase; // the GRU's f gate walks the same list as its i and c gates
  const int n = build_segments((int)cell_type, C, K, bc, bk, seg);
  for (int i = 0; i < n && i < capacity && nullptr != segments; ++i) { segments[3 * i] = seg[i].which; segments[3 * i + 1] = seg[i].start; segments[3 * i + 2] = seg[i].len; }
  return n;
}

LIBXSMM_API libxsmm_dnn_rnncell* libxsmm_dnn_create_rnncell(libxsmm_dnn_rnncell_desc desc, libxsmm_dnn_err_t* status)
{ // src/libxsmm_dnn_rnncell.c:48-137
  if (desc.datatype_in != desc.datatype_out || (LIBXSMM_DNN_DATATYPE_BF16 != desc.datatype_in && LIBXSMM_DNN_DATATYPE_F32 != desc.datatype_in)) {
    *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE; return nullptr;
  }
  if (LIBXSMM_DNN_DATATYPE_BF16 == desc.datatype_in) { *status = LIBXSMM_DNN_ERR_UNSUPPORTED_DATATYPE; return nullptr; } // (ours: DESIGN.md 9)
  if (desc.max_T < 1) { *status = LIBXSMM_DNN_ERR_TIME_STEPS_TOO_SMALL; return nullptr; }
  libxsmm_dnn_rnncell* const h = static_cast<libxsmm_dnn_rnncell*>(malloc(sizeof(libxsmm_dnn_rnncell)));
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_CREATE_HANDLE; return nullptr; }
  *status = LIBXSMM_DNN_SUCCESS;
  memset(h, 0, sizeof(*h));
  h->desc = desc;
  h->T = desc.max_T;
  h->bk = (0 == desc.bk) ? 64 : desc.bk;
  h->bn = (0 == desc.bn) ? 64 : desc.bn;
  h->bc = (0 == desc.bc) ? 64 : desc.bc;
  // (a negative block divides nothing sensibly: it is treated as one that does not divide; the reference would go on with it)
  if (h->bn < 0 || 0 != desc.N % h->bn) { h->bn = desc.N; *status = LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_N_BLOCKING; }
  if (h->bc < 0 || 0 != desc.C % h->bc) { h->bc = desc.C; *status = LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_C_BLOCKING; }
  if (h->bk < 0 || 0 != desc.K % h->bk) { h->bk = desc.K; *status = LIBXSMM_DNN_WARN_RNN_SUBOPTIMAL_K_BLOCKING; }
  return h;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_rnncell(const libxsmm_dnn_rnncell* handle)
{ // :140-152
  if (nullptr == handle) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (nullptr != handle->deltas) dev_free(handle->deltas); // (only a backward pass on a device ever sets it)
  free(const_cast<libxsmm_dnn_rnncell*>(handle));
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_rnncell_create_tensor_datalayout(const libxsmm_dnn_rnncell* h, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :155-841 (F32 only: create refuses everything else)
  typedef libxsmm_dnn_tensor_dimtype D;
  const D dN = LIBXSMM_DNN_TENSOR_DIMTYPE_N, dC = LIBXSMM_DNN_TENSOR_DIMTYPE_C, dK = LIBXSMM_DNN_TENSOR_DIMTYPE_K, dT = LIBXSMM_DNN_TENSOR_DIMTYPE_T,
          dX = LIBXSMM_DNN_TENSOR_DIMTYPE_X;
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return nullptr; }
  libxsmm_dnn_tensor_datalayout* const l = layout_begin(status);
  if (nullptr == l) return nullptr;
  const libxsmm_dnn_rnncell_desc& d = h->desc;
  const unsigned int N = (unsigned int)d.N, C = (unsigned int)d.C, K = (unsigned int)d.K, T = (unsigned int)d.max_T, G = (unsigned int)gates_of(d.cell_type);
  const unsigned int bn = (unsigned int)h->bn, bc = (unsigned int)h->bc, bk = (unsigned int)h->bk;
  const bool gated = (G > 1);
  bool ok = true; // false: the arrays could not be allocated
  l->datatype = d.datatype_in;
  l->custom_format = (libxsmm_dnn_internal_format)0; // (the reference leaves it zeroed)
  if (is_x(type) || is_state(type)) {
    l->format = d.buffer_format;
    l->tensor_type = LIBXSMM_DNN_ACTIVATION;
    const D df = is_x(type) ? dC : dK;
    const unsigned int f = is_x(type) ? C : K, bf = is_x(type) ? bc : bk;
    if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED)) {
      const D t[5] = { df, dN, df, dN, dT };
      const unsigned int s[5] = { bf, bn, 0 != bf ? f / bf : 0, 0 != bn ? N / bn : 0, T };
      ok = layout_dims(l, 5, t, s);
    }
    else if (0 != (d.buffer_format & LIBXSMM_DNN_TENSOR_FORMAT_NC)) {
      const D t[3] = { df, dN, dT };
      const unsigned int s[3] = { f, N, T };
      ok = layout_dims(l, 3, t, s);
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else if (is_w(type) || is_r(type) || LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS == type || LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT_TRANS == type) {
    const bool trans = !(is_w(type) || is_r(type)), weight = is_w(type) || LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS == type;
    const D dr = weight ? dC : dK;                        // the reduction side: C for w, K for r
    const unsigned int red = weight ? C : K, bred = weight ? bc : bk;
    l->format = d.filter_format;
    l->tensor_type = LIBXSMM_DNN_FILTER;
    if (0 != (d.filter_format & LIBXSMM_DNN_TENSOR_FORMAT_CKPACKED)) {
      const D t[5] = { trans ? dr : dK, trans ? dK : dr, trans ? dK : dr, trans ? dr : dK, dX };
      const unsigned int nred = 0 != bred ? red / bred : 0, nk = 0 != bk ? K / bk : 0;
      const unsigned int s[5] = { trans ? bred : bk, trans ? bk : bred, trans ? nk : nred, trans ? nred : nk, G };
      ok = layout_dims(l, gated ? 5 : 4, t, s);
    }
    else if (0 != (d.filter_format & LIBXSMM_DNN_TENSOR_FORMAT_CK)) {
      const D t[2] = { trans ? dr : dK, trans ? dK : dr };
      const unsigned int s[2] = { trans ? red : G * K, trans ? G * K : red };
      ok = layout_dims(l, 2, t, s);
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else if (is_bias(type)) {
    l->format = d.buffer_format;
    l->tensor_type = LIBXSMM_DNN_CHANNEL_SCALAR;
    if (0 != (d.buffer_format & (LIBXSMM_DNN_TENSOR_FORMAT_NC | LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED))) {
      const D t[1] = { dK };
      const unsigned int s[1] = { G * K };
      ok = layout_dims(l, 1, t, s);
    }
    else *status = LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  }
  else *status = LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE;
  return layout_end(l, ok, status);
}

LIBXSMM_API size_t libxsmm_dnn_rnncell_get_scratch_size(const libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status)
{ // :844-962 with 4-byte elements
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return 0; } // (the reference reads the handle first)
  *status = LIBXSMM_DNN_SUCCESS;
  const size_t C = (size_t)h->desc.C, K = (size_t)h->desc.K, N = (size_t)h->desc.N, T = (size_t)h->desc.max_T, G = (size_t)gates_of(h->desc.cell_type), ts = 4;
  const int cell = (int)h->desc.cell_type;
  const KindClass kc = kind_class(kind);
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) { *status = LIBXSMM_DNN_ERR_INVALID_RNN_TYPE; return 0; }
  if (KIND_UNKNOWN == kc) { *status = LIBXSMM_DNN_ERR_INVALID_KIND; return 0; }
  size_t size = 0;
  if (is_simple(cell)) {
    if (KIND_REST == kc) size = (C * K * ts + 64) + (K * K * ts + 64) + (C * N * ts + 64) + (K * N * ts + 64) + (K * N * ts * T + 64); // wT, rT, xT, hT, deltat
  }
  else {
    size = (C * K * ts * G + G * 64) + (K * K * ts * G + G * 64); // w, r
    if (KIND_REST == kc) size += (C * K * ts * G + G * 64) + (K * K * ts * G + G * 64) + (C * N * ts + 64) + 12 * (K * N * ts + 64); // wT, rT, xT and twelve of K * N
  }
  return size;
}

LIBXSMM_API void* libxsmm_dnn_rnncell_get_scratch_ptr(const libxsmm_dnn_rnncell* h, libxsmm_dnn_err_t* status)
{ // :965-976
  *status = nullptr != h ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return nullptr != h ? h->scratch_base : nullptr;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_scratch(libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind, const void* scratch)
{ // :979-1569: the kind is looked at before the pointer, and FWD of a simple cell needs none
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  const int cell = (int)h->desc.cell_type;
  const KindClass kc = kind_class(kind);
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) return LIBXSMM_DNN_ERR_INVALID_RNN_TYPE;
  if (KIND_UNKNOWN == kc) return LIBXSMM_DNN_ERR_INVALID_KIND;
  if (is_simple(cell) && KIND_FWD == kc) return LIBXSMM_DNN_SUCCESS;
  if (nullptr == scratch) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  h->scratch_base = const_cast<void*>(scratch);
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_scratch(libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind)
{ // :1572-1700 (the pieces are forgotten there; get_scratch_ptr goes on returning the base, as it does here)
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  const int cell = (int)h->desc.cell_type;
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) return LIBXSMM_DNN_ERR_INVALID_RNN_TYPE;
  return KIND_UNKNOWN == kind_class(kind) ? LIBXSMM_DNN_ERR_INVALID_KIND : LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API size_t libxsmm_dnn_rnncell_get_internalstate_size(const libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status)
{ // :1703-1770
  *status = LIBXSMM_DNN_SUCCESS;
  if (nullptr == h) { *status = LIBXSMM_DNN_ERR_INVALID_HANDLE; return 0; }
  const int cell = (int)h->desc.cell_type;
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) { *status = LIBXSMM_DNN_ERR_INVALID_RNN_TYPE; return 0; }
  if (KIND_UNKNOWN == kind_class(kind)) { *status = LIBXSMM_DNN_ERR_INVALID_KIND; return 0; }
  return is_simple(cell) ? (size_t)h->desc.K * (size_t)h->desc.N * sizeof(float) * (size_t)h->desc.max_T + 64 : 0; // z
}

LIBXSMM_API void* libxsmm_dnn_rnncell_get_internalstate_ptr(const libxsmm_dnn_rnncell* h, libxsmm_dnn_err_t* status)
{ // :1773-1784
  *status = nullptr != h ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return nullptr != h ? h->internal_z : nullptr;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_internalstate(libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind, const void* internalstate)
{ // :1787-1864: a simple cell looks at the pointer before the kind
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  const int cell = (int)h->desc.cell_type;
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) return LIBXSMM_DNN_ERR_INVALID_RNN_TYPE;
  if (is_simple(cell) && nullptr == internalstate) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  if (KIND_UNKNOWN == kind_class(kind)) return LIBXSMM_DNN_ERR_INVALID_KIND;
  if (is_simple(cell)) {
    const uintptr_t address = reinterpret_cast<uintptr_t>(internalstate);
    h->internal_z = reinterpret_cast<void*>(0 == address % 64 ? address : address + (64 - address % 64));
  }
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_internalstate(libxsmm_dnn_rnncell* h, const libxsmm_dnn_compute_kind kind)
{ // :1867-1928
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  const int cell = (int)h->desc.cell_type;
  if (!is_simple(cell) && LIBXSMM_DNN_RNNCELL_LSTM != cell && LIBXSMM_DNN_RNNCELL_GRU != cell) return LIBXSMM_DNN_ERR_INVALID_RNN_TYPE;
  if (KIND_UNKNOWN == kind_class(kind)) return LIBXSMM_DNN_ERR_INVALID_KIND;
  if (is_simple(cell)) h->internal_z = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_allocate_forget_bias(libxsmm_dnn_rnncell* h, const float forget_bias)
{ // :1931-1942
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR;
  h->forget_bias = forget_bias;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type)
{ // :1945-2030
  return bind_tensor(handle, tensor, type, libxsmm_dnn_rnncell_create_tensor_datalayout);
}

LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_rnncell_get_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{ // :2033-2107: *status is never written there (the shared get_tensor writes it)
  libxsmm_dnn_err_t unused;
  libxsmm_dnn_tensor** const slot = checked_slot(handle, type, true, LIBXSMM_DNN_ERR_INVALID_HANDLE, &unused);
  (void)status;
  return nullptr != slot ? *slot : nullptr;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor_type type)
{ // :2110-2187: a NULL handle is _ERR_INVALID_HANDLE_TENSOR here (the shared release_tensor answers _ERR_INVALID_HANDLE)
  libxsmm_dnn_err_t status;
  libxsmm_dnn_tensor** const slot = checked_slot(handle, type, true, LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR, &status);
  if (nullptr != slot) *slot = nullptr;
  return status;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_set_sequence_length(libxsmm_dnn_rnncell* h, const libxsmm_blasint T)
{ // :2190-2204
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (h->desc.max_T < T) return LIBXSMM_DNN_ERR_RNN_INVALID_SEQ_LEN;
  h->T = T;
  return LIBXSMM_DNN_SUCCESS;
}

LIBXSMM_API libxsmm_blasint libxsmm_dnn_rnncell_get_sequence_length(libxsmm_dnn_rnncell* h, libxsmm_dnn_err_t* status)
{ // :2207-2217
  *status = nullptr != h ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return nullptr != h ? h->T : 0;
}

namespace {

// The chain order of the backward reductions over the G * K filter columns (lstm bwdupd template :255-270, core template :205-292):
// for every chunk KB of K/BF indices the gates i, c, f, o in turn; BF depends on K alone. Adjacent pieces are one segment.
int build_bwd_segments(int cell, int K, int bk, RnnBwdSeg* seg)
{
  int n = 0;
  const auto add = [&](int start, int len) {
    if (len <= 0) return;
    if (n > 0 && seg[n - 1].start + seg[n - 1].len == start) { seg[n - 1].len += len; return; }
    seg[n].start = start; seg[n].len = len; ++n;
  };
  if (K < 1 || bk < 1 || 0 != K % bk) return 0;
  if (is_simple(cell)) { add(0, K); return n; }
  if (LIBXSMM_DNN_RNNCELL_LSTM != cell) return 0;
  const int kblocks = K / bk;
  int bf = 1;
  if (K > 1024 && K <= 2048) { bf = 8; while (0 != kblocks % bf) --bf; }
  if (K > 2048) { bf = 16; while (0 != kblocks % bf) --bf; }
  const int len = kblocks / bf * bk;
  for (int kb = 0; kb < bf; ++kb) for (int q = 0; q < 4; ++q) add(q * K + kb * len, len);
  return n;
}

std::mutex delta_lock; // (one for all handles: it is held for an allocation, once per handle)

// BWD, UPD and BWDUPD of the simple cells and the LSTM. Launches: one per step (the recurrence), the LSTM's dhp,
// dx of all steps (one per 65535 steps), and dw, dr, db: a function of the sequence length and the kind alone.
libxsmm_dnn_err_t execute_backward(libxsmm_dnn_rnncell* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{
  const bool bwd = (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind || LIBXSMM_DNN_COMPUTE_KIND_BWDUPD == kind);
  const bool upd = (LIBXSMM_DNN_COMPUTE_KIND_UPD == kind || LIBXSMM_DNN_COMPUTE_KIND_BWDUPD == kind);
  if (!bwd && !upd) return LIBXSMM_DNN_ERR_INVALID_KIND;
  const libxsmm_dnn_rnncell_desc& d = h->desc;
  const int cell = (int)d.cell_type;
  const bool simple = is_simple(cell), lstm = LIBXSMM_DNN_RNNCELL_LSTM == cell;
  if (!simple && !lstm) return LIBXSMM_DNN_ERR_INVALID_KIND; // (the GRU's backward is not built)
  if (nullptr == h->dxt && nullptr == h->dcsp && nullptr == h->dhp && nullptr == h->dw && nullptr == h->dr && nullptr == h->db && nullptr == h->dcs && nullptr == h->dht) {
    return LIBXSMM_DNN_ERR_INVALID_KIND; // (no gradient tensor at all: the answer from before these passes existed)
  }
  if (LIBXSMM_DNN_TENSOR_FORMAT_NC != d.buffer_format || LIBXSMM_DNN_TENSOR_FORMAT_CK != d.filter_format) return LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  // what the templates read and write under this kind
  if (nullptr == h->r || nullptr == h->dht) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (simple && nullptr == h->internal_z) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (lstm && (nullptr == h->csp || nullptr == h->cst || nullptr == h->it || nullptr == h->ft || nullptr == h->ot || nullptr == h->cit || nullptr == h->cot
    || nullptr == h->dcs || nullptr == h->dcsp || nullptr == h->dhp)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (bwd && (nullptr == h->w || nullptr == h->dxt)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (upd && (nullptr == h->xt || nullptr == h->hp || nullptr == h->ht || nullptr == h->dw || nullptr == h->dr || nullptr == h->db)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  const int G = gates_of(cell);
  const long long N = d.N, C = d.C, K = d.K, maxT = d.max_T, limit = 1LL << 31;
  if (N < 1 || C < 1 || K < 1 || d.threads < 1) return LIBXSMM_DNN_ERR_GENERAL;
  if (maxT * N * C >= limit || maxT * N * K >= limit || C * G * K >= limit || K * G * K >= limit) return LIBXSMM_DNN_ERR_GENERAL;
  const int ltid = tid - start_thread;
  if (ltid < 0) return LIBXSMM_DNN_ERR_GENERAL;
  const int T = h->T;
  // the recurrence and dx own rows as the forward does; dw, dr and db sum over all rows, and there is no barrier between calls: with
  // UPD or BWDUPD logical thread 0 launches the whole pass and the others have nothing to do
  long long b0 = 0, b1 = N / h->bn;
  if (upd) { if (0 != ltid) return LIBXSMM_DNN_SUCCESS; }
  else if (!thread_share(N / h->bn, d.threads, ltid, &b0, &b1)) return LIBXSMM_DNN_SUCCESS;
  if (T < 1) return LIBXSMM_DNN_SUCCESS;
  const int n0 = (int)(b0 * h->bn), n1 = (int)(b1 * h->bn);
  if (((long long)(n1 - n0) + 63) / 64 > 65535) return LIBXSMM_DNN_ERR_GENERAL; // (more row tiles than a grid has: nothing is written)
  RnnBwdChainArgs g; memset(&g, 0, sizeof(g));
  g.nseg = build_bwd_segments(cell, (int)K, h->bk, g.seg);

  if (!device_ready()) { fail_no_device("libxsmm_dnn_rnncell_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream;
  const long long ld = G * K, nk = N * K, nc = N * C, nld = N * ld;
  float* deltas;
  {
    const std::lock_guard<std::mutex> guard(delta_lock);
    if (nullptr == h->deltas) h->deltas = static_cast<float*>(dev_alloc((size_t)maxT * (size_t)nld * sizeof(float)));
    deltas = h->deltas;
  }
  if (nullptr == deltas) return LIBXSMM_DNN_ERR_GENERAL;
  libxsmm_dnn_tensor_datalayout zl; memset(&zl, 0, sizeof(zl));
  libxsmm_dnn_tensor_dimtype zt[1] = { LIBXSMM_DNN_TENSOR_DIMTYPE_K };
  unsigned int zs[1] = { (unsigned int)(maxT * N * K) };
  zl.dim_type = zt; zl.dim_size = zs; zl.num_dims = 1; zl.datatype = LIBXSMM_DNN_DATATYPE_F32;
  libxsmm_dnn_tensor ztensor; ztensor.layout = &zl; ztensor.data = h->internal_z; ztensor.scf = 0;
  Staging s;
  const Operand* const orr = s.add(h->r); const Operand* const odh = s.add(h->dht);
  const Operand *oz = nullptr, *ow = nullptr, *odx = nullptr, *ox = nullptr, *ohp = nullptr, *oh = nullptr, *odw = nullptr, *odr = nullptr, *odb = nullptr;
  const Operand *ocsp = nullptr, *ocs = nullptr, *oi = nullptr, *of = nullptr, *oo = nullptr, *oci = nullptr, *oco = nullptr, *odcs = nullptr, *odcsp = nullptr, *odhp = nullptr;
  if (simple) oz = s.add(&ztensor);
  if (lstm) {
    ocsp = s.add(h->csp); ocs = s.add(h->cst); oi = s.add(h->it); of = s.add(h->ft); oo = s.add(h->ot); oci = s.add(h->cit); oco = s.add(h->cot);
    odcs = s.add(h->dcs); odcsp = s.add(h->dcsp); odhp = s.add(h->dhp);
  }
  if (bwd) { ow = s.add(h->w); odx = s.add(h->dxt); }
  if (upd) { ox = s.add(h->xt); ohp = s.add(h->hp); oh = s.add(h->ht); odw = s.add(h->dw); odr = s.add(h->dr); odb = s.add(h->db); }
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  const auto f32 = [](const Operand* o) { return static_cast<float*>(dev_of(o)); };
  for (const Operand* o : { orr, odh, oz, ow, odx, ox, ohp, oh, odw, odr, odb, ocsp, ocs, oi, of, oo, oci, oco, odcs, odcsp, odhp }) {
    if (nullptr != o && 0 != reinterpret_cast<uintptr_t>(o->dev) % sizeof(float)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  const auto chain = [&](const RnnBwdChainArgs& a) { const char* name = ""; const int e = launch_rnn_bwd_chain(a, stream, &name); return launched(name, e); };

  g.n0 = n0; g.n1 = n1; g.ld = (int)ld; g.act = cell;
  for (int j = T - 1; j >= 0; --j) { // the recurrence: the deltas of step j from those of step j + 1
    RnnBwdChainArgs a = g;
    a.filt = f32(orr); a.M = (int)K; a.nz = 1;
    a.last = (T - 1 == j) ? 1 : 0;
    if (0 != a.last) a.nseg = 0;
    a.delta = deltas + (long long)(j + 1 < maxT ? j + 1 : j) * nld; // (not read at the last step)
    a.dstep = deltas + (long long)j * nld;
    a.dh = f32(odh) + j * nk;
    if (simple) { a.epi = RNN_BWD_EPI_SIMPLE; a.z = f32(oz) + j * nk; }
    else {
      a.epi = RNN_BWD_EPI_LSTM;
      a.gi = f32(oi) + j * nk; a.gf = f32(of) + j * nk; a.go = f32(oo) + j * nk; a.gci = f32(oci) + j * nk; a.gco = f32(oco) + j * nk;
      a.csprev = (0 == j) ? f32(ocsp) : f32(ocs) + (j - 1) * nk;
      a.dcs = f32(odcs); a.dcsp = f32(odcsp);
    }
    if (!chain(a)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  if (lstm) { // dhp: the chain of step 0, stored without an add
    RnnBwdChainArgs a = g;
    a.epi = RNN_BWD_EPI_STORE; a.filt = f32(orr); a.M = (int)K; a.nz = 1; a.delta = deltas; a.out = f32(odhp);
    if (!chain(a)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  if (bwd) { // dx of all steps: no dependence between them
    for (int s0 = 0; s0 < T; s0 += 65535) {
      RnnBwdChainArgs a = g;
      a.epi = RNN_BWD_EPI_STORE; a.filt = f32(ow); a.M = (int)C;
      a.nz = (T - s0 < 65535) ? (T - s0) : 65535; a.zd = nld; a.zo = nc;
      a.delta = deltas + (long long)s0 * nld; a.out = f32(odx) + s0 * nc;
      if (!chain(a)) return LIBXSMM_DNN_ERR_GENERAL;
    }
  }
  if (upd) {
    const char* name = "";
    RnnBwdWeightArgs a; memset(&a, 0, sizeof(a));
    a.delta = deltas; a.ld = (int)ld; a.N = (int)N; a.T = T;
    a.act = f32(ox); a.M = (int)C; a.out = f32(odw); a.shift = 0;
    int e = launch_rnn_bwd_weight(a, stream, &name);
    if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
    a.act = f32(oh); a.act0 = f32(ohp); a.M = (int)K; a.out = f32(odr); a.shift = 1; // (step 0 multiplies hp, also with one step: 8r)
    e = launch_rnn_bwd_weight(a, stream, &name);
    if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
    e = launch_rnn_bwd_bias(deltas, f32(odb), (int)ld, (int)N, T, stream, &name);
    if (!launched(name, e)) return LIBXSMM_DNN_ERR_GENERAL;
  }
  return s.finish({ odx, odw, odr, odb, odcsp, odhp }) ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}

} // namespace

LIBXSMM_API int libxsmm_amd_rnn_bwd_segments(libxsmm_dnn_rnncell_type cell_type, int K, int bk, int* segments, int capacity)
{
  RnnBwdSeg seg[RNN_BWD_MAX_SEG];
  const int n = build_bwd_segments((int)cell_type, K, bk, seg);
  for (int i = 0; i < n && i < capacity && nullptr != segments; ++i) { segments[2 * i] = seg[i].start; segments[2 * i + 1] = seg[i].len; }
  return n;
}

LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_execute_st(libxsmm_dnn_rnncell* h, libxsmm_dnn_compute_kind kind, int start_thread, int tid)
{ // :2220-2258 and src/libxsmm_dnn_rnncell_forward.c:218-272
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  if (LIBXSMM_DNN_COMPUTE_KIND_FWD != kind) return execute_backward(h, kind, start_thread, tid); // (ALL and the rest: the reference's answer, _ERR_INVALID_KIND)
  const libxsmm_dnn_rnncell_desc& d = h->desc;
  if (LIBXSMM_DNN_TENSOR_FORMAT_NC != d.buffer_format || LIBXSMM_DNN_TENSOR_FORMAT_CK != d.filter_format) return LIBXSMM_DNN_ERR_INVALID_FORMAT_GENERAL;
  const int cell = (int)d.cell_type;
  const bool simple = is_simple(cell), lstm = LIBXSMM_DNN_RNNCELL_LSTM == cell, gru = LIBXSMM_DNN_RNNCELL_GRU == cell;
  if (!simple && !lstm && !gru) return LIBXSMM_DNN_ERR_INVALID_RNN_TYPE;
  // from here on: this engine's own
  if (nullptr == h->xt || nullptr == h->hp || nullptr == h->w || nullptr == h->r || nullptr == h->b || nullptr == h->ht) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (simple && nullptr == h->internal_z) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (lstm && (nullptr == h->csp || nullptr == h->cst || nullptr == h->it || nullptr == h->ft || nullptr == h->ot || nullptr == h->cit || nullptr == h->cot)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  if (gru && (nullptr == h->it || nullptr == h->ft || nullptr == h->ot || nullptr == h->cit)) return LIBXSMM_DNN_ERR_DATA_NOT_BOUND;
  const int G = gates_of(cell);
  const long long N = d.N, C = d.C, K = d.K, maxT = d.max_T, limit = 1LL << 31;
  if (N < 1 || C < 1 || K < 1 || d.threads < 1) return LIBXSMM_DNN_ERR_GENERAL;
  if (maxT * N * C >= limit || maxT * N * K >= limit || C * G * K >= limit || K * G * K >= limit) return LIBXSMM_DNN_ERR_GENERAL;
  const int ltid = tid - start_thread;
  if (ltid < 0) return LIBXSMM_DNN_ERR_GENERAL;
  const int T = h->T;
  long long b0, b1;
  if (!thread_share(N / h->bn, d.threads, ltid, &b0, &b1) || T < 1) return LIBXSMM_DNN_SUCCESS;
  RnnArgs g; memset(&g, 0, sizeof(g));
  g.nseg = build_segments(cell, (int)C, (int)K, h->bc, h->bk, g.seg);
  // the split plan is legal where no piece of w follows a piece of r; it is the default there
  bool split = (g.nseg <= 2);
  { const char* const e = getenv("LIBXSMM_AMD_RNN_PLAN"); if (nullptr != e && 0 == strcmp(e, "whole")) split = false; }
  int first_r = 0; // the first segment of r (the split plan's step launches start there)
  while (first_r < g.nseg && 0 == g.seg[first_r].which) ++first_r;

  if (!device_ready()) { fail_no_device("libxsmm_dnn_rnncell_execute_st"); return LIBXSMM_DNN_ERR_GENERAL; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  // (a staged destination starts from the caller's bytes: only the share's rows are written, and the whole image travels back)
  libxsmm_dnn_tensor_datalayout zl; memset(&zl, 0, sizeof(zl));
  libxsmm_dnn_tensor_dimtype zt[1] = { LIBXSMM_DNN_TENSOR_DIMTYPE_K };
  unsigned int zs[1] = { (unsigned int)(maxT * N * K) };
  zl.dim_type = zt; zl.dim_size = zs; zl.num_dims = 1; zl.datatype = LIBXSMM_DNN_DATATYPE_F32;
  libxsmm_dnn_tensor ztensor; ztensor.layout = &zl; ztensor.data = h->internal_z; ztensor.scf = 0;
  Staging s;
  const Operand* const ox = s.add(h->xt); const Operand* const ohp = s.add(h->hp); const Operand* const ow = s.add(h->w);
  const Operand* const orr = s.add(h->r); const Operand* const ob = s.add(h->b); const Operand* const oh = s.add(h->ht);
  const Operand *oz = nullptr, *ocsp = nullptr, *ocs = nullptr, *oi = nullptr, *of = nullptr, *oo = nullptr, *oci = nullptr, *oco = nullptr;
  if (simple) oz = s.add(&ztensor);
  if (lstm) { ocsp = s.add(h->csp); ocs = s.add(h->cst); oco = s.add(h->cot); }
  if (lstm || gru) { oi = s.add(h->it); of = s.add(h->ft); oo = s.add(h->ot); oci = s.add(h->cit); }
  if (!s.place()) return LIBXSMM_DNN_ERR_GENERAL;
  const auto f32 = [](const Operand* o) { return static_cast<float*>(dev_of(o)); };
  for (const Operand* o : { ox, ohp, ow, orr, ob, oh, oz, ocsp, ocs, oi, of, oo, oci, oco }) {
    if (nullptr != o && 0 != reinterpret_cast<uintptr_t>(o->dev) % sizeof(float)) return LIBXSMM_DNN_ERR_GENERAL;
  }

  g.w = f32(ow); g.r = f32(orr); g.b = f32(ob);
  g.n0 = (int)(b0 * h->bn); g.n1 = (int)(b1 * h->bn); g.K = (int)K; g.C = (int)C; g.ldw = (int)(G * K);
  g.forget_bias = h->forget_bias; g.act = cell;
  const long long nk = N * K, nc = N * C;
  // where the chains of the sets lie between the launches of the split plan: the gate tensors themselves (RNN: z)
  float* const chain[4] = { simple ? f32(oz) : f32(oi), f32(oci), f32(of), f32(oo) }; // in the order of the columns: (z) or i, c, f, o
  const auto run = [&](const RnnArgs& a) { const char* name = ""; const int e = launch_rnn(a, stream, &name); return launched(name, e); };

  if (split) { // bias + w.x of all gates and all steps at once
    for (int t0 = 0; t0 < T; t0 += 65535) {
      RnnArgs a = g;
      a.G = G; a.epi = RNN_EPI_NONE; a.from_bias = 1; a.fgate = lstm ? 2 : -1;
      a.nseg = first_r;
      for (int q = 0; q < G; ++q) { a.gcol[q] = q * (int)K; a.pre[q] = chain[q] + t0 * nk; }
      a.x = f32(ox) + t0 * nc; a.nz = (T - t0 < 65535) ? (T - t0) : 65535; a.zx = nc; a.zo = nk;
      if (!run(a)) return LIBXSMM_DNN_ERR_GENERAL;
    }
  }
  for (int t = 0; t < T; ++t) {
    RnnArgs a = g;
    a.nz = 1; a.from_bias = split ? 0 : 1; a.fgate = -1;
    if (split) { a.nseg = g.nseg - first_r; for (int q = 0; q < a.nseg; ++q) a.seg[q] = g.seg[first_r + q]; }
    a.x = f32(ox) + t * nc;
    a.hprev = (0 == t) ? f32(ohp) : f32(oh) + (t - 1) * nk;
    a.hsrc = a.hprev;
    a.h = f32(oh) + t * nk;
    if (simple) {
      a.G = 1; a.epi = RNN_EPI_RNN; a.gcol[0] = 0; a.pre[0] = chain[0] + t * nk;
      if (!run(a)) return LIBXSMM_DNN_ERR_GENERAL;
    }
    else if (lstm) {
      a.G = 4; a.epi = RNN_EPI_LSTM; a.fgate = 2;
      for (int q = 0; q < 4; ++q) { a.gcol[q] = q * (int)K; a.pre[q] = chain[q] + t * nk; }
      a.csprev = (0 == t) ? f32(ocsp) : f32(ocs) + (t - 1) * nk;
      a.gi = f32(oi) + t * nk; a.gci = f32(oci) + t * nk; a.gf = f32(of) + t * nk; a.go = f32(oo) + t * nk;
      a.cs = f32(ocs) + t * nk; a.gco = f32(oco) + t * nk;
      if (!run(a)) return LIBXSMM_DNN_ERR_GENERAL;
    }
    else { // GRU: i, c and o = h[t-1] * i; then f over w_f.x and r_f.o, and h
      a.gi = f32(oi) + t * nk; a.gci = f32(oci) + t * nk; a.gf = f32(of) + t * nk; a.go = f32(oo) + t * nk;
      RnnArgs p1 = a;
      p1.G = 2; p1.epi = RNN_EPI_GRU1;
      for (int q = 0; q < 2; ++q) { p1.gcol[q] = q * (int)K; p1.pre[q] = chain[q] + t * nk; }
      if (!run(p1)) return LIBXSMM_DNN_ERR_GENERAL;
      RnnArgs p2 = a;
      p2.G = 1; p2.epi = RNN_EPI_GRU2; p2.gcol[0] = 2 * (int)K; p2.pre[0] = chain[2] + t * nk;
      p2.hsrc = a.go;
      if (!run(p2)) return LIBXSMM_DNN_ERR_GENERAL;
    }
  }
  // what the pass wrote travels back if it was staged
  const bool ok = simple ? s.finish({ oh, oz }) : (lstm ? s.finish({ oh, ocs, oi, of, oo, oci, oco }) : s.finish({ oh, oi, of, oo, oci }));
  return ok ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_GENERAL;
}
