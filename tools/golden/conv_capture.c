/* conv_capture.c -- calls the convolution layer of the unmodified reference through its public functions only and writes what they
 * return as raw binary, for tools/golden/conv_capture.py to pack into tests/golden/conv.npz. Built against the reference's
 * static libraries (its make BLAS=0 FORTRAN=0 STATIC=1 ECFLAGS=-fcommon writes include/libxsmm.h and lib/libxsmm.a,
 * lib/libxsmmnoblas.a):
 *   gcc -O1 -I<reference>/include conv_capture.c <reference>/lib/libxsmm.a <reference>/lib/libxsmmnoblas.a -lm -lpthread -ldl -lrt -o conv_capture
 * Usage: conv_capture N C H W K R S u v pad_h pad_w pad_h_in pad_w_in pad_h_out pad_w_out threads dt_in dt_out buffer_format
 *                     filter_format algo options fuse_ops unbound run scratch x w dout bias out0 din0 dw0 prefix
 *   unbound: bit i set leaves tensor type i of BINDABLE below unbound
 *   run: -1 only create, 0 only statuses and layouts, 1 also trans_reg_filter and execute_st of FWD, BWD and UPD
 *   scratch: 1 binds a scratch with LIBXSMM_DNN_COMPUTE_KIND_ALL before the passes, 0 binds none (FWD is then not run: the
 *            reference's generic FWD does not ask for its scratch and would write through NULL)
 *   x, w, dout, bias: files holding REGULAR_INPUT, REGULAR_FILTER, GRADIENT_OUTPUT and REGULAR_CHANNEL_BIAS in their own layout;
 *   out0, din0, dw0: what REGULAR_OUTPUT, GRADIENT_INPUT and GRADIENT_FILTER hold before the passes; "-": 0xff bytes
 * Writes prefix.meta (long long values, see META below) and prefix.{out,din,dw,wtr} (raw tensors).
 * The scratch is bound with KIND_ALL: under KIND_BWD the reference's generic path lays scratch1 (the transposed filter) and
 * scratch5 (the padded plane) at one address (src/libxsmm_dnn.c:1869-1886). */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* META: [0] create status, [1] handle != NULL, [2..5] scratch size of kinds FWD, BWD, UPD, ALL, [6] status of get_scratch_size
 * for kind BWDUPD, [7] bind_scratch(NULL), [8] bind_scratch(ALL) (-1: scratch == 0), [9] bind_scratch(BWDUPD), [10] release_scratch(ALL),
 * [11] bind_tensor with a pooling type, [12] bind_tensor(NULL tensor), [13] bind_tensor of the input tensor as REGULAR_OUTPUT,
 * [14] release_tensor with a pooling type, [15] execute_st(NULL handle), [16..20] execute_st of kinds 0..4, [21..23]
 * get_codegen_success of FWD, BWD, UPD, [24] of ALL, [25..27] get_parallel_tasks of FWD, BWD, UPD, [28] its status for ALL,
 * [29] transpose_filter(REGULAR_FILTER) after the scratch, [30] transpose_filter(GRADIENT_FILTER), [31]
 * reduce_wu_filters(GRADIENT_FILTER), [32] reduce_wu_filters(REGULAR_FILTER), [33] trans_reg_filter, [34] status of
 * get_scratch_size(NULL handle), [35] status of create_tensor_datalayout(NULL handle), [36] bind_scratch(NULL handle), [37]
 * transpose_filter(REGULAR_FILTER) before any scratch, [38] release_scratch(BWDUPD), [39] release_tensor(REGULAR_INPUT) at the end;
 * per layout type 26 values from [40]: layout status, num_dims, dim_type[8], dim_size[8], datatype, format, custom_format,
 * tensor_type, size in bytes, elements, link status, bind status. -1: not done. */
#define NBIND 9
#define NTYPES 14
#define NMETA (40 + 26 * NTYPES)
static long long meta[NMETA];

/* the first NBIND are BINDABLE */
static const libxsmm_dnn_tensor_type types[NTYPES] = { LIBXSMM_DNN_REGULAR_INPUT, LIBXSMM_DNN_GRADIENT_INPUT, LIBXSMM_DNN_REGULAR_OUTPUT,
  LIBXSMM_DNN_GRADIENT_OUTPUT, LIBXSMM_DNN_REGULAR_FILTER, LIBXSMM_DNN_GRADIENT_FILTER, LIBXSMM_DNN_REGULAR_FILTER_TRANS,
  LIBXSMM_DNN_REGULAR_CHANNEL_BIAS, LIBXSMM_DNN_GRADIENT_CHANNEL_BIAS, LIBXSMM_DNN_INPUT, LIBXSMM_DNN_OUTPUT, LIBXSMM_DNN_FILTER,
  LIBXSMM_DNN_CHANNEL_BIAS, LIBXSMM_DNN_POOLING_MASK };

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
  libxsmm_dnn_conv_desc desc;
  libxsmm_dnn_layer* handle;
  libxsmm_dnn_tensor* tensor[NTYPES];
  void* data[NTYPES];
  size_t bytes[NTYPES];
  libxsmm_dnn_err_t status;
  int unbound, run, with_scratch, i, j, kind;
  unsigned int tasks;
  const char* prefix;
  void* scratch = NULL;
  if (35 != argc) { fprintf(stderr, "see the head of conv_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.H = atoi(argv[3]); desc.W = atoi(argv[4]); desc.K = atoi(argv[5]); desc.R = atoi(argv[6]);
  desc.S = atoi(argv[7]); desc.u = atoi(argv[8]); desc.v = atoi(argv[9]); desc.pad_h = atoi(argv[10]); desc.pad_w = atoi(argv[11]);
  desc.pad_h_in = atoi(argv[12]); desc.pad_w_in = atoi(argv[13]); desc.pad_h_out = atoi(argv[14]); desc.pad_w_out = atoi(argv[15]);
  desc.threads = atoi(argv[16]); desc.datatype_in = (libxsmm_dnn_datatype)atoi(argv[17]); desc.datatype_out = (libxsmm_dnn_datatype)atoi(argv[18]);
  desc.buffer_format = (libxsmm_dnn_tensor_format)atoi(argv[19]); desc.filter_format = (libxsmm_dnn_tensor_format)atoi(argv[20]);
  desc.algo = (libxsmm_dnn_conv_algo)atoi(argv[21]); desc.options = (libxsmm_dnn_conv_option)atoi(argv[22]);
  desc.fuse_ops = (libxsmm_dnn_conv_fuse_op)atoi(argv[23]);
  unbound = atoi(argv[24]); run = atoi(argv[25]); with_scratch = atoi(argv[26]); prefix = argv[34];
  for (i = 0; i < NMETA; ++i) meta[i] = -1;
  for (i = 0; i < NTYPES; ++i) { tensor[i] = NULL; data[i] = NULL; bytes[i] = 0; }
  libxsmm_init();
  status = 0xdead;
  handle = libxsmm_dnn_create_conv_layer(desc, &status);
  meta[0] = status; meta[1] = (NULL != handle);
  (void)libxsmm_dnn_get_scratch_size(NULL, LIBXSMM_DNN_COMPUTE_KIND_ALL, &status); meta[34] = status;
  (void)libxsmm_dnn_create_tensor_datalayout(NULL, LIBXSMM_DNN_REGULAR_INPUT, &status); meta[35] = status;
  meta[36] = libxsmm_dnn_bind_scratch(NULL, LIBXSMM_DNN_COMPUTE_KIND_ALL, &status);
  meta[15] = libxsmm_dnn_execute_st(NULL, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0);
  if (NULL != handle && run < 0) libxsmm_dnn_destroy_conv_layer(handle); /* create only */
  else if (NULL != handle) {
    static const libxsmm_dnn_compute_kind kinds[4] = { LIBXSMM_DNN_COMPUTE_KIND_FWD, LIBXSMM_DNN_COMPUTE_KIND_BWD, LIBXSMM_DNN_COMPUTE_KIND_UPD, LIBXSMM_DNN_COMPUTE_KIND_ALL };
    for (i = 0; i < 4; ++i) meta[2 + i] = (long long)libxsmm_dnn_get_scratch_size(handle, kinds[i], &status);
    (void)libxsmm_dnn_get_scratch_size(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, &status); meta[6] = status;
    for (i = 0; i < NTYPES; ++i) {
      long long* const m = meta + 40 + 26 * i;
      libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_create_tensor_datalayout(handle, types[i], &status);
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
      if (i < NBIND && NULL != tensor[i] && 0 == (unbound & (1 << i))) m[25] = libxsmm_dnn_bind_tensor(handle, tensor[i], types[i]);
    }
    if (NULL != tensor[0]) {
      meta[11] = libxsmm_dnn_bind_tensor(handle, tensor[0], LIBXSMM_DNN_POOLING_MASK);
      if (bytes[0] != bytes[2]) meta[13] = libxsmm_dnn_bind_tensor(handle, tensor[0], LIBXSMM_DNN_REGULAR_OUTPUT);
      if (NULL != tensor[2] && 0 == (unbound & 4)) (void)libxsmm_dnn_bind_tensor(handle, tensor[2], LIBXSMM_DNN_REGULAR_OUTPUT);
    }
    meta[12] = libxsmm_dnn_bind_tensor(handle, NULL, LIBXSMM_DNN_REGULAR_INPUT);
    meta[14] = libxsmm_dnn_release_tensor(handle, LIBXSMM_DNN_POOLING_MASK);
    if (NULL != data[0]) slurp(argv[27], data[0], bytes[0]);
    if (NULL != data[4]) slurp(argv[28], data[4], bytes[4]);
    if (NULL != data[3]) slurp(argv[29], data[3], bytes[3]);
    if (NULL != data[7]) slurp(argv[30], data[7], bytes[7]);
    if (NULL != data[2]) slurp(argv[31], data[2], bytes[2]);
    if (NULL != data[1]) slurp(argv[32], data[1], bytes[1]);
    if (NULL != data[5]) slurp(argv[33], data[5], bytes[5]);
    meta[37] = libxsmm_dnn_transpose_filter(handle, LIBXSMM_DNN_REGULAR_FILTER);
    meta[30] = libxsmm_dnn_transpose_filter(handle, LIBXSMM_DNN_GRADIENT_FILTER);
    meta[7] = libxsmm_dnn_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, NULL);
    if (0 != with_scratch) {
      scratch = libxsmm_aligned_malloc((size_t)meta[5], 64);
      memset(scratch, 0, (size_t)meta[5]);
      meta[9] = libxsmm_dnn_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, scratch);
      meta[8] = libxsmm_dnn_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, scratch);
      meta[29] = libxsmm_dnn_transpose_filter(handle, LIBXSMM_DNN_REGULAR_FILTER);
    }
    meta[31] = libxsmm_dnn_reduce_wu_filters(handle, LIBXSMM_DNN_GRADIENT_FILTER);
    meta[32] = libxsmm_dnn_reduce_wu_filters(handle, LIBXSMM_DNN_REGULAR_FILTER);
    for (i = 0; i < 3; ++i) {
      meta[21 + i] = libxsmm_dnn_get_codegen_success(handle, kinds[i]);
      tasks = 0; status = libxsmm_dnn_get_parallel_tasks(handle, kinds[i], &tasks); meta[25 + i] = (LIBXSMM_DNN_SUCCESS == status ? (long long)tasks : -(long long)status);
    }
    meta[24] = libxsmm_dnn_get_codegen_success(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL);
    meta[28] = libxsmm_dnn_get_parallel_tasks(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, &tasks);
    if (0 != run) {
      meta[33] = libxsmm_dnn_trans_reg_filter(handle);
      for (kind = 0; kind < 5; ++kind) {
        if (LIBXSMM_DNN_COMPUTE_KIND_FWD == kind && 0 == with_scratch && 0 == (unbound & (1 | 4 | 16))) continue;
        meta[16 + kind] = libxsmm_dnn_execute_st(handle, (libxsmm_dnn_compute_kind)kind, 0, 0);
      }
      if (NULL != data[2]) dump(prefix, "out", data[2], bytes[2]);
      if (NULL != data[1]) dump(prefix, "din", data[1], bytes[1]);
      if (NULL != data[5]) dump(prefix, "dw", data[5], bytes[5]);
      if (NULL != data[6]) dump(prefix, "wtr", data[6], bytes[6]);
    }
    meta[38] = libxsmm_dnn_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD);
    meta[10] = libxsmm_dnn_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL);
    meta[39] = libxsmm_dnn_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT);
    for (i = 0; i < NTYPES; ++i) { if (NULL != tensor[i]) libxsmm_dnn_destroy_tensor(tensor[i]); if (NULL != data[i]) libxsmm_free(data[i]); }
    libxsmm_dnn_destroy_conv_layer(handle);
    if (NULL != scratch) libxsmm_free(scratch);
  }
  dump(prefix, "meta", meta, sizeof(meta));
  return 0;
}
