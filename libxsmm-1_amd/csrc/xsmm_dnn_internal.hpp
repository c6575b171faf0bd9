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

#endif
