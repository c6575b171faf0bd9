/* fc_capture.c -- calls the fully-connected layer of the unmodified reference through its public functions only and writes
 * what they return as raw binary, for tools/golden/fc_capture.py to pack into tests/golden/fc.npz. Built against the
 * reference's static libraries (its make writes include/libxsmm.h and lib/libxsmm.a, lib/libxsmmnoblas.a):
 *   gcc -O1 -I<reference>/include fc_capture.c <reference>/lib/libxsmm.a <reference>/lib/libxsmmnoblas.a -lm -lpthread -ldl -lrt -o fc_capture
 * Usage: fc_capture N C K bn bk bc threads dt_in dt_out buffer_format filter_format fuse_ops unbound run x w dy xplain wplain prefix
 *   unbound: bit i set leaves tensor type i of {reg_in, grad_in, reg_out, grad_out, reg_fil, grad_fil} unbound
 *   run: 0 only statuses and layouts, 1 also execute_st for every kind
 *   x, w, dy: files holding the tensors in their own layout and element type; xplain, wplain: the same as plain NCHW / KCRS, or "-"
 * Writes prefix.meta (long long values, see META below) and prefix.{y,dx,dw,cin_x,cin_w,cout_x,cout_w} (raw tensors). */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_fullyconnected.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* META: [0] create status, [1] handle != NULL, [2] scratch size, [3] its status; per tensor type 26 values from [4]: layout status,
 * num_dims, dim_type[8], dim_size[8], datatype, format, custom_format, tensor_type, size in bytes, elements, link status, bind status;
 * [160..164] execute_st status of kinds 0..4; [165..168] status of copyin x, copyin w, copyout x, copyout w. -1: not done. */
#define NMETA 169
static long long meta[NMETA];

static const libxsmm_dnn_tensor_type types[6] = { LIBXSMM_DNN_REGULAR_INPUT, LIBXSMM_DNN_GRADIENT_INPUT, LIBXSMM_DNN_REGULAR_OUTPUT,
  LIBXSMM_DNN_GRADIENT_OUTPUT, LIBXSMM_DNN_REGULAR_FILTER, LIBXSMM_DNN_GRADIENT_FILTER };

static size_t slurp(const char* path, void* dst, size_t bytes)
{
  FILE* f;
  size_t n;
  if (0 == strcmp(path, "-")) return 0;
  f = fopen(path, "rb");
  if (NULL == f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  n = fread(dst, 1, bytes, f);
  fclose(f);
  return n;
}

static void dump(const char* prefix, const char* suffix, const void* p, size_t bytes)
{
  char path[1024];
  FILE* f;
  snprintf(path, sizeof(path), "%s.%s", prefix, suffix);
  f = fopen(path, "wb");
  if (NULL == f || bytes != fwrite(p, 1, bytes, f)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char* argv[])
{
  libxsmm_dnn_fullyconnected_desc desc;
  libxsmm_dnn_fullyconnected* handle;
  libxsmm_dnn_tensor* tensor[6] = { NULL, NULL, NULL, NULL, NULL, NULL };
  void* data[6] = { NULL, NULL, NULL, NULL, NULL, NULL };
  size_t bytes[6] = { 0, 0, 0, 0, 0, 0 };
  libxsmm_dnn_err_t status;
  int unbound, run, i, j, kind;
  const char* prefix;
  void* scratch;
  if (21 != argc) { fprintf(stderr, "see the head of fc_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.K = atoi(argv[3]); desc.bn = atoi(argv[4]); desc.bk = atoi(argv[5]); desc.bc = atoi(argv[6]);
  desc.threads = atoi(argv[7]); desc.datatype_in = (libxsmm_dnn_datatype)atoi(argv[8]); desc.datatype_out = (libxsmm_dnn_datatype)atoi(argv[9]);
  desc.buffer_format = (libxsmm_dnn_tensor_format)atoi(argv[10]); desc.filter_format = (libxsmm_dnn_tensor_format)atoi(argv[11]);
  desc.fuse_ops = (libxsmm_dnn_fullyconnected_fuse_op)atoi(argv[12]);
  unbound = atoi(argv[13]); run = atoi(argv[14]); prefix = argv[20];
  for (i = 0; i < NMETA; ++i) meta[i] = -1;
  libxsmm_init();
  status = 0xdead;
  handle = libxsmm_dnn_create_fullyconnected(desc, &status);
  meta[0] = status; meta[1] = (NULL != handle);
  if (NULL != handle) {
    meta[2] = (long long)libxsmm_dnn_fullyconnected_get_scratch_size(handle, &status); meta[3] = status;
    scratch = libxsmm_aligned_malloc((size_t)meta[2], 64);
    memset(scratch, 0, (size_t)meta[2]);
    for (i = 0; i < 6; ++i) {
      long long* const m = meta + 4 + 26 * i;
      libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_fullyconnected_create_tensor_datalayout(handle, types[i], &status);
      m[0] = status;
      if (NULL == layout) continue;
      m[1] = layout->num_dims;
      for (j = 0; j < (int)layout->num_dims && j < 8; ++j) { m[2 + j] = layout->dim_type[j]; m[10 + j] = layout->dim_size[j]; }
      m[18] = layout->datatype; m[19] = layout->format; m[20] = layout->custom_format; m[21] = layout->tensor_type;
      m[22] = libxsmm_dnn_get_tensor_size(layout, &status); m[23] = libxsmm_dnn_get_tensor_elements(layout, &status);
      bytes[i] = (size_t)m[22];
      data[i] = libxsmm_aligned_malloc(bytes[i] + 64, 64);
      memset(data[i], 0xff, bytes[i] + 64); /* destinations start as NaN */
      tensor[i] = libxsmm_dnn_link_tensor(layout, data[i], &status); m[24] = status;
      libxsmm_dnn_destroy_tensor_datalayout(layout);
      if (NULL != tensor[i] && 0 == (unbound & (1 << i))) m[25] = libxsmm_dnn_fullyconnected_bind_tensor(handle, tensor[i], types[i]);
    }
    if (NULL != data[0]) slurp(argv[15], data[0], bytes[0]);
    if (NULL != data[4]) slurp(argv[16], data[4], bytes[4]);
    if (NULL != data[3]) slurp(argv[17], data[3], bytes[3]);
    libxsmm_dnn_fullyconnected_bind_scratch(handle, scratch);
    if (0 != run) {
      for (kind = 0; kind < 5; ++kind) meta[160 + kind] = libxsmm_dnn_fullyconnected_execute_st(handle, (libxsmm_dnn_compute_kind)kind, 0, 0);
      if (NULL != data[2]) dump(prefix, "y", data[2], bytes[2]);
      if (NULL != data[1]) dump(prefix, "dx", data[1], bytes[1]);
      if (NULL != data[5]) dump(prefix, "dw", data[5], bytes[5]);
    }
    if (0 != strcmp(argv[18], "-") && NULL != tensor[1] && NULL != tensor[5]) { /* copies through the gradient tensors (reg_in, reg_fil keep the inputs) */
      void* const px = malloc(bytes[0] + 64);
      void* const pw = malloc(bytes[4] + 64);
      slurp(argv[18], px, bytes[0]); slurp(argv[19], pw, bytes[4]);
      meta[165] = libxsmm_dnn_copyin_tensor(tensor[1], px, LIBXSMM_DNN_TENSOR_FORMAT_NCHW); dump(prefix, "cin_x", data[1], bytes[1]);
      meta[166] = libxsmm_dnn_copyin_tensor(tensor[5], pw, LIBXSMM_DNN_TENSOR_FORMAT_KCRS); dump(prefix, "cin_w", data[5], bytes[5]);
      memset(px, 0xff, bytes[0]); memset(pw, 0xff, bytes[4]);
      meta[167] = libxsmm_dnn_copyout_tensor(tensor[0], px, LIBXSMM_DNN_TENSOR_FORMAT_NCHW); dump(prefix, "cout_x", px, bytes[0]);
      meta[168] = libxsmm_dnn_copyout_tensor(tensor[4], pw, LIBXSMM_DNN_TENSOR_FORMAT_KCRS); dump(prefix, "cout_w", pw, bytes[4]);
      free(px); free(pw);
    }
    for (i = 0; i < 6; ++i) { libxsmm_dnn_destroy_tensor(tensor[i]); if (NULL != data[i]) libxsmm_free(data[i]); }
    libxsmm_dnn_fullyconnected_release_scratch(handle);
    libxsmm_dnn_destroy_fullyconnected(handle);
    libxsmm_free(scratch);
  }
  dump(prefix, "meta", meta, sizeof(meta));
  return 0;
}
