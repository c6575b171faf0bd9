// xsmm_dnn_internal.hpp -- what the DNN sources share: the tensor behind the opaque handle of include/libxsmm_dnn.h, the
// arguments of the layers' kernels, and the host plumbing that every layer has (xsmm_dnn_layer.cpp).
#ifndef XSMM_DNN_INTERNAL_HPP
#define XSMM_DNN_INTERNAL_HPP

#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"
#include "../../include/libxsmm_dnn.h"
#include "kernels/dnn_copy_plan.h"

#include <initializer_list>

struct libxsmm_dnn_tensor { // src/libxsmm_main.h:339-343
  libxsmm_dnn_tensor_datalayout* layout;
  void* data;
  unsigned char scf;
};

namespace xsmm {

// pooling layer (xsmm_dnn_pool.cpp, kernels/pool.hip): the items [w0, w1) of blocked activations [item][row][column][16]
struct PoolArgs {
  void* in; void* out; void* mask;        // input / dinput, output / doutput, mask (MAX only): memory the GPU reaches, 16-byte aligned
  int H, W, R, S, u, v, pad_h, pad_w;     // the desc's plane, window, strides and logical padding
  int iph, ipw, oph, opw;                 // physical padding of input and output
  int ofh, ofw;
  int w0, w1;                             // the share: items image * blocks + block
  float recp;                             // 1 / (R * S)
  int bwd, is_max, bf16;
};
int launch_pool(const PoolArgs& args, void* stream, const char** name); // returns hipError_t as int

// fused batch-norm layer (xsmm_dnn_bn.cpp, kernels/bn.hip): blocked activations [item][row][column][16], item = image * blocks + block
struct BnArgs {
  void* in; void* add; void* out; void* dout; void* din; // input, input_add / dinput_add, output, doutput, dinput: 16-byte aligned
  float* gamma; float* beta; float* mean; float* rstd; float* var; float* dgamma; float* dbeta; // [blocks][16]
  float* part;                            // the call's own partial sums: [touched block][image][2][16]
  int N, H, W, u, v, blocks;
  int iph, ipw, oph, opw;                 // physical padding of input and output
  int ofh, ofw;                           // H / u, W / v
  int w0, w1;                             // the share: items image * blocks + block
  int fm0, nfm;                           // the channel blocks the share touches: (fm0 + j) % blocks, j < nfm
  float nhw, recp_nhw;
  int bwd, bf16, stats, eltwise, relu;    // stats: OPS_BN (statistics are computed), else OPS_BNSCALE
};
// the three steps of a pass, in launch order; each returns hipError_t as int
int launch_bn_partial(const BnArgs& args, void* stream, const char** name); // stats only: per (touched block, image) the ordered sums
int launch_bn_finish(const BnArgs& args, void* stream, const char** name);  // stats only: images in order; mean / rstd / var or dgamma / dbeta
int launch_bn_apply(const BnArgs& args, void* stream, const char** name);   // the items [w0, w1)

// convolution layer (xsmm_dnn_conv.cpp, kernels/conv.hip): activations [image][block][row][column][block size], filter
// [ofm1][ifm1][kj][ki][ifm2][ofm2] (trans: [ifm1][ofm1][R-1-kj][S-1-ki][ofm2][ifm2]); every tensor has fewer than 2^31 elements
struct ConvArgs {
  void* in; void* out; void* flt; void* bias; // input / dinput, output / doutput, filter / dfilter, bias (FWD with bias_on)
  int N, C, K, H, W, R, S, u, v, pad_h, pad_w;
  int ifmblock, ofmblock, blocksifm, blocksofm;
  int ifhp, ifwp, ofh, ofw, ofhp, ofwp, oph, opw; // padded extents; physical padding of the output
  int logical;                            // pad_*_in == 0 with a pad_* > 0: the rim is not in memory
  int w0, w1;                             // the share: items img * blocksofm + ofm1 (FWD), img * blocksifm + ifm1 (BWD), ofm1 * blocksifm + ifm1 (UPD)
  int overwrite, bias_on, relu;           // OPTION_OVERWRITE; FWD: FUSE_BIAS, fuse_ops & FUSE_RELU
  int flt_trans;                          // BWD: flt is REGULAR_FILTER_TRANS
  int per_image;                          // UPD: the form with one chain per image and ordered adds
  int tile;                               // FWD: 64 or 128
};
// one pass over the share, or the transposition of the whole filter (in: REGULAR_FILTER, out: REGULAR_FILTER_TRANS in g.flt / g.out);
// each returns hipError_t as int
int launch_conv_fwd(const ConvArgs& args, void* stream, const char** name);
int launch_conv_bwd(const ConvArgs& args, void* stream, const char** name);
int launch_conv_upd(const ConvArgs& args, void* stream, const char** name);
int launch_conv_trans_filter(const ConvArgs& args, void* stream, const char** name);

// RNN cell layer (xsmm_dnn_rnn.cpp, kernels/rnn.hip): one launch computes, for the rows [n0, n1) of the minibatch and all K outputs,
// G accumulator sets (gates) of one step -- or, with nz > 1, of nz steps whose operands lie zx / zo elements apart
constexpr int RNN_MAX_SEG = 34; // two operand pairs times the largest BF, and two to spare
enum RnnEpilogue : int { RNN_EPI_NONE = 0 /* store the chains where they are continued from */, RNN_EPI_RNN, RNN_EPI_LSTM, RNN_EPI_GRU1, RNN_EPI_GRU2 };
struct RnnSeg { int which, start, len; }; // operand pair (0: x / w, 1: hsrc / r), first row of w or r, rows; in chain order
struct RnnArgs {
  const float* x; const float* hsrc;      // [row][C] and [row][K]: the step's input and what r multiplies (h of the step before, hp, or the GRU's o)
  const float* w; const float* r; const float* b; // [C][ldw], [K][ldw], [ldw]
  float* pre[4];                          // per set: where its chain is stored (EPI_NONE) or continued from (!from_bias); RNN: z
  int gcol[4];                            // per set: its first column in w, r and b
  const float* hprev; const float* csprev; // the epilogues' operands of the step before, [row][K]
  float* gi; float* gf; float* go; float* gci; float* gco; float* cs; float* h; // the step's destinations, [row][K]
  int n0, n1, K, C, ldw, G;
  int nz; long long zx, zo;               // steps per launch; their distance in x and in pre
  int from_bias, fgate; float forget_bias; // the chains start from b (set fgate: from b + forget_bias), else from pre
  int epi, act;                           // RnnEpilogue; RNN: the cell type
  int nseg; RnnSeg seg[RNN_MAX_SEG];
};
int launch_rnn(const RnnArgs& args, void* stream, const char** name); // returns hipError_t as int

// RNN cell layer, backward and update (xsmm_dnn_rnn.cpp, kernels/rnn_bwd.hip). The deltas of a pass live in a handle-owned buffer
// [step][row][ld], ld = G * K, the gates side by side in the filters' column order (LSTM: i, c, f, o).
constexpr int RNN_BWD_MAX_SEG = 64; // four gates times the largest BF
enum RnnBwdEpilogue : int { RNN_BWD_EPI_STORE = 0 /* out = the chain */, RNN_BWD_EPI_SIMPLE /* delta = (dh continued by the chain) * act'(z) */,
  RNN_BWD_EPI_LSTM /* dout = the chain + dh; dcsp and the four deltas */ };
struct RnnBwdSeg { int start, len; }; // columns of the filter row and of the delta row, in chain order
// out[row][m] = start continued by, for every segment, the chain over its columns q of filt[m][q] * delta[row][q]
struct RnnBwdChainArgs {
  const float* filt;   // [M][ld]: w (M = C) or r (M = K)
  const float* delta;  // [row][ld], nz steps zd apart: what is reduced (unused with nseg = 0)
  float* out;          // EPI_STORE: [row][M], nz steps zo apart
  int M, ld, n0, n1, nz; long long zd, zo;
  int epi, act, last;  // act: the simple cell's type; last: step T - 1 (dout is dh alone, the LSTM starts from dcs)
  const float* dh; const float* z; // the step's, [row][K]
  float* dstep;        // the step's deltas, [row][ld]
  const float* gi; const float* gf; const float* go; const float* gci; const float* gco; const float* csprev; const float* dcs; // LSTM, [row][K]
  float* dcsp;         // LSTM: the running dcp, [row][K]
  int nseg; RnnBwdSeg seg[RNN_BWD_MAX_SEG];
};
int launch_rnn_bwd_chain(const RnnBwdChainArgs& args, void* stream, const char** name);
// out[m][j] = +0.0 continued by one chain over the steps descending and the rows ascending of act_t[row][m] * delta_t[row][j]
struct RnnBwdWeightArgs {
  const float* act;    // [step][row][M]: x (M = C) or h (M = K)
  const float* act0;   // shift: what step 0 multiplies (hp)
  const float* delta;  // [step][row][ld]
  float* out;          // [M][ld]
  int M, ld, N, T, shift; // shift 1: step t multiplies act[t - 1]
};
int launch_rnn_bwd_weight(const RnnBwdWeightArgs& args, void* stream, const char** name);
int launch_rnn_bwd_bias(const float* delta, float* db, int ld, int N, int T, void* stream, const char** name); // db[j] = +0.0 + delta in the same order

// tensor copy-in / copy-out (xsmm_dnn.cpp, kernels/dnn_copy.hip): one launch moves the whole tensor between its blocked side and its
// plain side (in: plain -> blocked), both memory the GPU reaches, aligned to their element; g comes from dnn_copy_geom
int launch_dnn_copy(const DnnCopyGeom& g, void* blocked, void* plain, bool in, void* stream, const char** name); // returns hipError_t as int

// ---- what the layers share on the host (xsmm_dnn_layer.cpp) ---------------------------------------------------------------
// A layer provides slot_of(handle*, type) at global scope (the tensor pointer a type binds; nullptr for a type it does not
// bind), its create_tensor_datalayout and its execute_st; the rest of its API forwards to the templates below.

// layouts: begin allocates and zeroes (nullptr: *status = ERR_CREATE_LAYOUT); layout_dims gives n dimensions (false: out of
// memory); end turns !ok into ERR_CREATE_LAYOUT_ARRAYS, frees everything on any status but SUCCESS and returns l or nullptr
libxsmm_dnn_tensor_datalayout* layout_begin(libxsmm_dnn_err_t* status);
bool layout_dims(libxsmm_dnn_tensor_datalayout* l, unsigned int n, const libxsmm_dnn_tensor_dimtype* types, const unsigned int* sizes);
libxsmm_dnn_tensor_datalayout* layout_end(libxsmm_dnn_tensor_datalayout* l, bool ok, libxsmm_dnn_err_t* status);

bool is_input(libxsmm_dnn_tensor_type t);   // REGULAR_INPUT, GRADIENT_INPUT, INPUT
bool is_output(libxsmm_dnn_tensor_type t);  // REGULAR_OUTPUT, GRADIENT_OUTPUT, OUTPUT

// the blocking of C feature maps on both sides of a layer without a filter (pooling, batch-norm)
struct FmBlocks { int ifmblock, ifmblock_hp, ofmblock, ofmblock_lp, blocksifm, blocksofm, fm_lp_block; };
FmBlocks feature_map_blocks(int C, bool f32);
// the activation layouts of those layers: LIBXSMM in F32 (5 dimensions) or BF16 (6), NHWC (4), else *status =
// ERR_INVALID_FORMAT_GENERAL; input: the input side's block and extents; false: out of memory
bool activation_layout(libxsmm_dnn_tensor_datalayout* l, libxsmm_dnn_tensor_format format, libxsmm_dnn_datatype datatype_in, libxsmm_dnn_datatype datatype_out,
                       const FmBlocks& b, int N, int C, bool input, unsigned int ifhp, unsigned int ifwp, unsigned int ofhp, unsigned int ofwp, libxsmm_dnn_err_t* status);

// the share [b0, b1) of logical thread ltid of work items (the templates' chunksize, thr_begin, thr_end); false: it is empty
// (ltid >= threads included). threads >= 1, ltid >= 0.
bool thread_share(long long work, int threads, int ltid, long long* b0, long long* b1);

// The tensors of a pass where the kernels can reach them. Those in pageable host memory share one block of device scratch
// (slot 6 of the calling thread), carved up at 256-byte offsets in the order in which they are asked for, and are uploaded.
struct Operand { void* dev; void* host; size_t bytes; size_t offset; }; // host: nullptr unless staged
struct Staging {
  Operand op[24]; int n = 0; size_t total = 0; bool wait = false;
  const Operand* add(const libxsmm_dnn_tensor* t); // (dev is valid after place)
  bool place();                                    // false: no memory, or a copy failed
  // after the launches: the staged ones of the operands the pass wrote (nullptr: skipped) travel back, and the stream is idle on
  // return if anything was staged or is host-visible; false: a copy or the wait failed
  bool finish(std::initializer_list<const Operand*> written);
};
inline void* dev_of(const Operand* o) { return nullptr != o ? o->dev : nullptr; }
inline bool aligned16(const Operand* o) { return 0 == reinterpret_cast<uintptr_t>(dev_of(o)) % 16; }

bool launched(const char* name, int hip_error); // counts the launch; false: it failed (and says so on stderr)

template<typename H> size_t scratch_size_of(const H* h, libxsmm_dnn_err_t* status)
{ // (64 bytes more for a caller that does not align)
  *status = nullptr != h ? LIBXSMM_DNN_SUCCESS : LIBXSMM_DNN_ERR_INVALID_HANDLE;
  return nullptr != h ? h->scratch_size + 64 : 0;
}
template<typename H> libxsmm_dnn_err_t bind_scratch(H* h, const void* p)
{
  const uintptr_t address = reinterpret_cast<uintptr_t>(p);
  if (nullptr == p) return LIBXSMM_DNN_ERR_SCRATCH_NOT_ALLOCED;
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  h->scratch = reinterpret_cast<void*>(0 == address % 64 ? address : address + (64 - address % 64));
  return LIBXSMM_DNN_SUCCESS;
}
template<typename H> libxsmm_dnn_err_t release_scratch(H* h)
{
  if (nullptr == h) return LIBXSMM_DNN_ERR_INVALID_HANDLE;
  h->scratch = nullptr;
  return LIBXSMM_DNN_SUCCESS;
}
// the slot of a type, checked in the reference's order: the type first (on a stand-in where there is no handle), then the handle
// and whatever else must be there (rest)
template<typename H> libxsmm_dnn_tensor** checked_slot(H* h, libxsmm_dnn_tensor_type type, bool rest, libxsmm_dnn_err_t invalid, libxsmm_dnn_err_t* status)
{
  H none;
  const bool known = nullptr != slot_of(nullptr != h ? h : &none, type);
  *status = !known ? LIBXSMM_DNN_ERR_UNKNOWN_TENSOR_TYPE : (nullptr != h && rest ? LIBXSMM_DNN_SUCCESS : invalid);
  return LIBXSMM_DNN_SUCCESS == *status ? slot_of(h, type) : nullptr;
}
template<typename H, typename F> libxsmm_dnn_err_t bind_tensor(H* h, const libxsmm_dnn_tensor* tensor, libxsmm_dnn_tensor_type type, F make_layout)
{
  libxsmm_dnn_err_t status;
  libxsmm_dnn_tensor** const slot = checked_slot(h, type, nullptr != tensor, LIBXSMM_DNN_ERR_INVALID_HANDLE_TENSOR, &status);
  if (nullptr == slot) return status;
  libxsmm_dnn_tensor_datalayout* const want = make_layout(h, type, &status);
  if (0 == libxsmm_dnn_compare_tensor_datalayout(want, tensor->layout, &status)) *slot = const_cast<libxsmm_dnn_tensor*>(tensor);
  else status = LIBXSMM_DNN_ERR_MISMATCH_TENSOR;
  if (nullptr != want) libxsmm_dnn_destroy_tensor_datalayout(want);
  return status;
}
template<typename H> libxsmm_dnn_tensor* get_tensor(H* h, libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status)
{
  libxsmm_dnn_tensor** const slot = checked_slot(h, type, true, LIBXSMM_DNN_ERR_INVALID_HANDLE, status);
  return nullptr != slot ? *slot : nullptr;
}
template<typename H> libxsmm_dnn_err_t release_tensor(H* h, libxsmm_dnn_tensor_type type)
{
  libxsmm_dnn_err_t status;
  libxsmm_dnn_tensor** const slot = checked_slot(h, type, true, LIBXSMM_DNN_ERR_INVALID_HANDLE, &status);
  if (nullptr != slot) *slot = nullptr;
  return status;
}

} // namespace xsmm

#endif
