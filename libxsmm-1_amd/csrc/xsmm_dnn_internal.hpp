// xsmm_dnn_internal.hpp -- what the DNN sources share: the tensor behind the opaque handle of include/libxsmm_dnn.h.
#ifndef XSMM_DNN_INTERNAL_HPP
#define XSMM_DNN_INTERNAL_HPP

#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"
#include "../../include/libxsmm_dnn.h"

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

} // namespace xsmm

#endif
