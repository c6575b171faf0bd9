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

} // namespace xsmm

#endif
