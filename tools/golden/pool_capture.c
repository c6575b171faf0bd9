/* pool_capture.c -- calls the pooling layer of the unmodified reference through its public functions only and writes what they
 * return as raw binary, for tools/golden/pool_capture.py to pack into tests/golden/pool.npz. Built against the reference's
 * static libraries (its make writes include/libxsmm.h and lib/libxsmm.a, lib/libxsmmnoblas.a):
 *   gcc -O1 -I<reference>/include pool_capture.c <reference>/lib/libxsmm.a <reference>/lib/libxsmmnoblas.a -lm -lpthread -ldl -lrt -o pool_capture
 * Usage: pool_capture N C H W R S u v pad_h pad_w pad_h_in pad_w_in pad_h_out pad_w_out threads dt_in dt_out dt_mask format
 *                     pooling_type unbound run x dout prefix
 *   unbound: bit i set leaves tensor type i of {reg_in, grad_in, reg_out, grad_out, mask} unbound
 *   run: 0 only statuses and layouts, 1 also execute_st for every kind
 *   x, dout: files holding REGULAR_INPUT and GRADIENT_OUTPUT in their own layout and element type, or "-"
 * Writes prefix.meta (long long values, see META below) and prefix.{out,mask,din} (raw tensors; destinations start as 0xff
 * bytes, so the mask starts as -1 everywhere). BWD of a max pooling is not run while the bound mask still holds a -1: the
 * reference would use it as an index. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_pooling.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* META: [0] create status, [1] handle != NULL, [2] scratch size, [3] its status, [4] bind_scratch(NULL), [5] bind_scratch,
 * [6] release_scratch, [7] bind_tensor with a filter type, [8] bind_tensor(NULL tensor), [9] get_tensor with a filter type;
 * per layout type 26 values from [10]: layout status, num_dims, dim_type[8], dim_size[8], datatype, format, custom_format,
 * tensor_type, size in bytes, elements, link status, bind status; [220..224] execute_st status of kinds 0..4;
 * [225] BWD was left out because of a -1 in the mask. -1: not done; -2: uninitialised in the reference (see below). */
#define NTYPES 8
#define NMETA 226
static long long meta[NMETA];

static const libxsmm_dnn_tensor_type types[NTYPES] = { LIBXSMM_DNN_REGULAR_INPUT, LIBXSMM_DNN_GRADIENT_INPUT, LIBXSMM_DNN_REGULAR_OUTPUT,
  LIBXSMM_DNN_GRADIENT_OUTPUT, LIBXSMM_DNN_POOLING_MASK, LIBXSMM_DNN_INPUT, LIBXSMM_DNN_OUTPUT, LIBXSMM_DNN_REGULAR_FILTER };

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
  libxsmm_dnn_pooling_desc desc;
  libxsmm_dnn_pooling* handle;
  libxsmm_dnn_tensor* tensor[NTYPES];
  void* data[NTYPES];
  size_t bytes[NTYPES];
  libxsmm_dnn_err_t status;
  int unbound, run, i, j, kind;
  const char* prefix;
  void* scratch;
  if (26 != argc) { fprintf(stderr, "see the head of pool_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.H = atoi(argv[3]); desc.W = atoi(argv[4]); desc.R = atoi(argv[5]); desc.S = atoi(argv[6]);
  desc.u = atoi(argv[7]); desc.v = atoi(argv[8]); desc.pad_h = atoi(argv[9]); desc.pad_w = atoi(argv[10]);
  desc.pad_h_in = atoi(argv[11]); desc.pad_w_in = atoi(argv[12]); desc.pad_h_out = atoi(argv[13]); desc.pad_w_out = atoi(argv[14]);
  desc.threads = atoi(argv[15]); desc.datatype_in = (libxsmm_dnn_datatype)atoi(argv[16]); desc.datatype_out = (libxsmm_dnn_datatype)atoi(argv[17]);
  desc.datatype_mask = (libxsmm_dnn_datatype)atoi(argv[18]); desc.buffer_format = (libxsmm_dnn_tensor_format)atoi(argv[19]);
  desc.pooling_type = (libxsmm_dnn_pooling_type)atoi(argv[20]);
  unbound = atoi(argv[21]); run = atoi(argv[22]); prefix = argv[25];
  for (i = 0; i < NMETA; ++i) meta[i] = -1;
  for (i = 0; i < NTYPES; ++i) { tensor[i] = NULL; data[i] = NULL; bytes[i] = 0; }
  libxsmm_init();
  status = 0xdead;
  handle = libxsmm_dnn_create_pooling(desc, &status);
  meta[0] = status; meta[1] = (NULL != handle);
  if (NULL != handle) {
    meta[2] = (long long)libxsmm_dnn_pooling_get_scratch_size(handle, &status); meta[3] = status;
    scratch = libxsmm_aligned_malloc((size_t)meta[2], 64);
    memset(scratch, 0, (size_t)meta[2]);
    for (i = 0; i < NTYPES; ++i) {
      long long* const m = meta + 10 + 26 * i;
      libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_pooling_create_tensor_datalayout(handle, types[i], &status);
      m[0] = status;
      if (NULL == layout) continue;
      m[1] = layout->num_dims;
      for (j = 0; j < (int)layout->num_dims && j < 8; ++j) { m[2 + j] = layout->dim_type[j]; m[10 + j] = layout->dim_size[j]; }
      m[18] = layout->datatype; m[19] = layout->format; m[20] = layout->custom_format; m[21] = layout->tensor_type;
      m[22] = libxsmm_dnn_get_tensor_size(layout, &status); m[23] = libxsmm_dnn_get_tensor_elements(layout, &status);
      bytes[i] = (size_t)m[22];
      if (LIBXSMM_DNN_POOLING_MASK == types[i] && 6 == layout->num_dims) {
        /* the reference's 16-bit branch reports six dimensions for the mask and sets the sizes of five: the sixth is whatever
         * malloc returned, and so are the sizes derived from it. Recorded as -2; the buffer gets what the five say. */
        bytes[i] = sizeof(int);
        for (j = 0; j < 5; ++j) bytes[i] *= layout->dim_size[j];
        m[15] = m[22] = m[23] = -2;
      }
      data[i] = libxsmm_aligned_malloc(bytes[i] + 64, 64);
      memset(data[i], 0xff, bytes[i] + 64);
      tensor[i] = libxsmm_dnn_link_tensor(layout, data[i], &status); m[24] = status;
      libxsmm_dnn_destroy_tensor_datalayout(layout);
      if (i < 5 && NULL != tensor[i] && 0 == (unbound & (1 << i))) m[25] = libxsmm_dnn_pooling_bind_tensor(handle, tensor[i], types[i]);
    }
    if (NULL != tensor[0]) {
      meta[7] = libxsmm_dnn_pooling_bind_tensor(handle, tensor[0], LIBXSMM_DNN_REGULAR_FILTER);
      (void)libxsmm_dnn_pooling_get_tensor(handle, LIBXSMM_DNN_REGULAR_FILTER, &status); meta[9] = status;
    }
    meta[8] = libxsmm_dnn_pooling_bind_tensor(handle, NULL, LIBXSMM_DNN_REGULAR_INPUT);
    if (NULL != data[0]) slurp(argv[23], data[0], bytes[0]);
    if (NULL != data[3]) slurp(argv[24], data[3], bytes[3]);
    meta[4] = libxsmm_dnn_pooling_bind_scratch(handle, NULL);
    meta[5] = libxsmm_dnn_pooling_bind_scratch(handle, scratch);
    if (0 != run) {
      for (kind = 0; kind < 5; ++kind) {
        if (LIBXSMM_DNN_COMPUTE_KIND_BWD == kind && LIBXSMM_DNN_POOLING_MAX == desc.pooling_type && NULL != data[4] && 0 == (unbound & 16)
          && LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM == desc.buffer_format)
        {
          const int* const mask = (const int*)data[4];
          size_t k;
          meta[225] = 0;
          for (k = 0; k < bytes[4] / sizeof(int); ++k) if (mask[k] < 0) meta[225] = 1;
          if (0 != meta[225]) continue;
        }
        meta[220 + kind] = libxsmm_dnn_pooling_execute_st(handle, (libxsmm_dnn_compute_kind)kind, 0, 0);
      }
      if (NULL != data[2]) dump(prefix, "out", data[2], bytes[2]);
      if (NULL != data[4]) dump(prefix, "mask", data[4], bytes[4]);
      if (NULL != data[1]) dump(prefix, "din", data[1], bytes[1]);
    }
    meta[6] = libxsmm_dnn_pooling_release_scratch(handle);
    for (i = 0; i < NTYPES; ++i) { if (NULL != tensor[i]) libxsmm_dnn_destroy_tensor(tensor[i]); if (NULL != data[i]) libxsmm_free(data[i]); }
    libxsmm_dnn_destroy_pooling(handle);
    libxsmm_free(scratch);
  }
  dump(prefix, "meta", meta, sizeof(meta));
  return 0;
}
