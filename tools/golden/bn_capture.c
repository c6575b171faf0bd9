/* bn_capture.c -- calls the fused batch-norm layer of the unmodified reference through its public functions only and writes what
 * they return as raw binary, for tools/golden/bn_capture.py to pack into tests/golden/bn.npz. Built against the reference's
 * static libraries (its make writes include/libxsmm.h and lib/libxsmm.a, lib/libxsmmnoblas.a):
 *   gcc -O1 -I<reference>/include bn_capture.c <reference>/lib/libxsmm.a <reference>/lib/libxsmmnoblas.a -lm -lpthread -ldl -lrt -o bn_capture
 * Usage: bn_capture N C H W u v pad_h_in pad_w_in pad_h_out pad_w_out threads dt_in dt_out dt_stats format fuse_order fuse_ops
 *                   unbound run x add dout gamma beta mean rstd dgamma dbeta prefix
 *   unbound: bit i set leaves bindable tensor type i (the order of `types` below) unbound
 *   run: 0 only statuses and layouts, 1 also execute_st for every kind, 2 the same without BWD
 *   x ... dbeta: files holding these tensors in their own layout and element type, or "-"
 * Writes prefix.meta (long long values, see META below) and prefix.{out,mean,rstd,var,din,dadd,dout,dgamma,dbeta} (raw tensors;
 * whatever was not read from a file starts as 0xff bytes). execute_st is called with start_thread = tid = 0 on a handle of
 * threads = 1, with the scratch bound. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_fusedbatchnorm.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* META: [0] create status, [1] handle != NULL, [2] scratch size, [3] its status, [4] bind_scratch(NULL), [5] bind_scratch,
 * [6] release_scratch, [7] bind_tensor with a filter type, [8] bind_tensor(NULL tensor), [9] get_tensor with a filter type;
 * per layout type 26 values from [10]: layout status, num_dims, dim_type[8], dim_size[8], datatype, format, custom_format,
 * tensor_type, size in bytes, elements, link status, bind status; [480..484] execute_st status of kinds 0..4. -1: not done. */
#define NBIND 13
#define NTYPES 18
#define NMETA 486
static long long meta[NMETA];

static const libxsmm_dnn_tensor_type types[NTYPES] = { LIBXSMM_DNN_REGULAR_INPUT, LIBXSMM_DNN_GRADIENT_INPUT, LIBXSMM_DNN_REGULAR_OUTPUT,
  LIBXSMM_DNN_GRADIENT_OUTPUT, LIBXSMM_DNN_REGULAR_INPUT_ADD, LIBXSMM_DNN_GRADIENT_INPUT_ADD, LIBXSMM_DNN_REGULAR_CHANNEL_BETA,
  LIBXSMM_DNN_GRADIENT_CHANNEL_BETA, LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA, LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA, LIBXSMM_DNN_CHANNEL_EXPECTVAL,
  LIBXSMM_DNN_CHANNEL_RCPSTDDEV, LIBXSMM_DNN_CHANNEL_VARIANCE, LIBXSMM_DNN_INPUT, LIBXSMM_DNN_OUTPUT, LIBXSMM_DNN_CHANNEL_BETA,
  LIBXSMM_DNN_CHANNEL_GAMMA, LIBXSMM_DNN_REGULAR_FILTER };
/* the files of the command line, in order, and the tensors written afterwards: indices into `types` */
static const int in_index[9] = { 0, 4, 3, 8, 6, 10, 11, 9, 7 };
static const int out_index[9] = { 2, 10, 11, 12, 1, 5, 3, 9, 7 };
static const char* const out_name[9] = { "out", "mean", "rstd", "var", "din", "dadd", "dout", "dgamma", "dbeta" };

static void slurp(const char* path, void* dst, size_t bytes)
{
  FILE* f;
  if (0 == strcmp(path, "-")) return;
  f = fopen(path, "rb");
  if (NULL == f || bytes != fread(dst, 1, bytes, f)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
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
  libxsmm_dnn_fusedbatchnorm_desc desc;
  libxsmm_dnn_fusedbatchnorm* handle;
  libxsmm_dnn_tensor* tensor[NTYPES];
  void* data[NTYPES];
  size_t bytes[NTYPES];
  libxsmm_dnn_err_t status;
  int unbound, run, i, j, kind;
  const char* prefix;
  void* scratch;
  if (30 != argc) { fprintf(stderr, "see the head of bn_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.H = atoi(argv[3]); desc.W = atoi(argv[4]); desc.u = atoi(argv[5]); desc.v = atoi(argv[6]);
  desc.pad_h_in = atoi(argv[7]); desc.pad_w_in = atoi(argv[8]); desc.pad_h_out = atoi(argv[9]); desc.pad_w_out = atoi(argv[10]);
  desc.threads = atoi(argv[11]); desc.datatype_in = (libxsmm_dnn_datatype)atoi(argv[12]); desc.datatype_out = (libxsmm_dnn_datatype)atoi(argv[13]);
  desc.datatype_stats = (libxsmm_dnn_datatype)atoi(argv[14]); desc.buffer_format = (libxsmm_dnn_tensor_format)atoi(argv[15]);
  desc.fuse_order = (libxsmm_dnn_fusedbatchnorm_fuse_order)atoi(argv[16]); desc.fuse_ops = (libxsmm_dnn_fusedbatchnorm_fuse_op)atoi(argv[17]);
  unbound = atoi(argv[18]); run = atoi(argv[19]); prefix = argv[29];
  for (i = 0; i < NMETA; ++i) meta[i] = -1;
  for (i = 0; i < NTYPES; ++i) { tensor[i] = NULL; data[i] = NULL; bytes[i] = 0; }
  libxsmm_init();
  status = 0xdead;
  handle = libxsmm_dnn_create_fusedbatchnorm(desc, &status);
  meta[0] = status; meta[1] = (NULL != handle);
  if (NULL != handle) {
    meta[2] = (long long)libxsmm_dnn_fusedbatchnorm_get_scratch_size(handle, &status); meta[3] = status;
    scratch = libxsmm_aligned_malloc((size_t)meta[2], 64);
    memset(scratch, 0, (size_t)meta[2]);
    for (i = 0; i < NTYPES; ++i) {
      long long* const m = meta + 10 + 26 * i;
      libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, types[i], &status);
      m[0] = status;
      if (NULL == layout) continue;
      m[1] = layout->num_dims;
      for (j = 0; j < (int)layout->num_dims && j < 8; ++j) { m[2 + j] = layout->dim_type[j]; m[10 + j] = layout->dim_size[j]; }
      m[18] = layout->datatype; m[19] = layout->format; m[20] = layout->custom_format; m[21] = layout->tensor_type;
      m[22] = libxsmm_dnn_get_tensor_size(layout, &status); m[23] = libxsmm_dnn_get_tensor_elements(layout, &status);
      bytes[i] = (size_t)m[22];
      data[i] = libxsmm_aligned_malloc(bytes[i] + 64, 64);
      memset(data[i], 0xff, bytes[i] + 64);
      tensor[i] = libxsmm_dnn_link_tensor(layout, data[i], &status); m[24] = status;
      libxsmm_dnn_destroy_tensor_datalayout(layout);
      if (i < NBIND && NULL != tensor[i] && 0 == (unbound & (1 << i))) m[25] = libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, tensor[i], types[i]);
    }
    if (NULL != tensor[0]) {
      meta[7] = libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, tensor[0], LIBXSMM_DNN_REGULAR_FILTER);
      (void)libxsmm_dnn_fusedbatchnorm_get_tensor(handle, LIBXSMM_DNN_REGULAR_FILTER, &status); meta[9] = status;
    }
    meta[8] = libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, NULL, LIBXSMM_DNN_REGULAR_INPUT);
    for (i = 0; i < 9; ++i) if (NULL != data[in_index[i]]) slurp(argv[20 + i], data[in_index[i]], bytes[in_index[i]]);
    meta[4] = libxsmm_dnn_fusedbatchnorm_bind_scratch(handle, NULL);
    meta[5] = libxsmm_dnn_fusedbatchnorm_bind_scratch(handle, scratch);
    if (0 != run) {
      for (kind = 0; kind < 5; ++kind) {
        if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind && 2 == run) continue;
        meta[480 + kind] = libxsmm_dnn_fusedbatchnorm_execute_st(handle, (libxsmm_dnn_compute_kind)kind, 0, 0);
      }
      for (i = 0; i < 9; ++i) if (NULL != data[out_index[i]]) dump(prefix, out_name[i], data[out_index[i]], bytes[out_index[i]]);
    }
    meta[6] = libxsmm_dnn_fusedbatchnorm_release_scratch(handle);
    for (i = 0; i < NTYPES; ++i) { if (NULL != tensor[i]) libxsmm_dnn_destroy_tensor(tensor[i]); if (NULL != data[i]) libxsmm_free(data[i]); }
    libxsmm_dnn_destroy_fusedbatchnorm(handle);
    libxsmm_free(scratch);
  }
  dump(prefix, "meta", meta, sizeof(meta));
  return 0;
}
