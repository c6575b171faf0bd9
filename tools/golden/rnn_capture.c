/* rnn_capture.c -- calls the RNN cell layer of the unmodified reference through its public functions only and writes what they
 * return as raw binary, for tools/golden/rnn_capture.py to pack into tests/golden/rnn.npz. Built against the reference's static
 * libraries (its make writes include/libxsmm.h and lib/libxsmm.a, lib/libxsmmnoblas.a):
 *   gcc -O1 -I<reference>/include rnn_capture.c <reference>/lib/libxsmm.a <reference>/lib/libxsmmnoblas.a -lm -lpthread -ldl -lrt -o rnn_capture
 * Usage: rnn_capture N C K max_T cell bn bc bk threads dt_in dt_out buffer_format filter_format seq forget_bias run
 *                    x hp csp w r b prefix
 *   seq: the sequence length to set before the pass, or -1 to leave max_T; forget_bias: a float, or "-" not to call
 *   allocate_forget_bias; run: 0 only statuses, sizes and layouts, 1 also execute_st(FWD)
 *   x ... b: files holding these tensors as fp32 in their own layout, or "-"
 * Writes prefix.meta (long long values, see META below) and prefix.{h,cs,i,f,o,ci,co,z} (raw tensors; whatever was not read from a
 * file starts as 0xff bytes). execute_st is called with start_thread = tid = 0 on a handle of threads = 1, with scratch and
 * internal state bound. Only FWD is executed. No function is called with a NULL handle that the reference dereferences. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_rnncell.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* META: [0] create status, [1] handle != NULL; for kind = 0..5 (5 is no kind): [2 + 2 kind] scratch size, [3 + 2 kind] its status,
 * [14 + 2 kind] internal-state size, [15 + 2 kind] its status, [26 + kind] bind_scratch(NULL), [32 + kind] bind_scratch(memory),
 * [38 + kind] release_scratch, [44 + kind] bind_internalstate(NULL), [50 + kind] bind_internalstate(memory), [56 + kind]
 * release_internalstate; [62] bind_tensor(NULL tensor), [63] bind_tensor with LIBXSMM_DNN_REGULAR_INPUT, [64] bind_tensor(NULL
 * handle), [65] release_tensor with LIBXSMM_DNN_REGULAR_INPUT, [66] release_tensor(NULL handle), [67] what get_tensor leaves in a
 * status preset to 57005 for LIBXSMM_DNN_REGULAR_INPUT, [68] the same for a NULL handle, [69] allocate_forget_bias(NULL), [70]
 * set_sequence_length(max_T + 1), [71] get_sequence_length after it, [72] its status, [73] set_sequence_length(seq), [74]
 * get_sequence_length(NULL)'s status, [75] set_sequence_length(NULL), [76] bind_tensor of the input tensor as the hidden state, [77]
 * get_scratch_ptr returns the bound address, [78] get_internalstate_ptr returns the bound address rounded up to 64, [79]
 * destroy(NULL); per layout type 26 values from [80]: layout status, num_dims, dim_type[8], dim_size[8], datatype, format,
 * custom_format, tensor_type, size in bytes, elements, link status, bind status; [704] execute_st(FWD), [705] execute_st(ALL),
 * [706] execute_st(7). -1: not done. */
#define NTYPES 24
#define NMETA 710
static long long meta[NMETA];

/* the 23 RNN types in the order of the enumeration, then one type the layer does not know */
static const libxsmm_dnn_tensor_type types[NTYPES] = { LIBXSMM_DNN_RNN_REGULAR_INPUT, LIBXSMM_DNN_RNN_REGULAR_CS_PREV,
  LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_REGULAR_WEIGHT, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT,
  LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT_TRANS, LIBXSMM_DNN_RNN_REGULAR_BIAS, LIBXSMM_DNN_RNN_REGULAR_CS,
  LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE, LIBXSMM_DNN_RNN_GRADIENT_INPUT, LIBXSMM_DNN_RNN_GRADIENT_CS_PREV,
  LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_GRADIENT_WEIGHT, LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT,
  LIBXSMM_DNN_RNN_GRADIENT_BIAS, LIBXSMM_DNN_RNN_GRADIENT_CS, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE, LIBXSMM_DNN_RNN_INTERNAL_I,
  LIBXSMM_DNN_RNN_INTERNAL_F, LIBXSMM_DNN_RNN_INTERNAL_O, LIBXSMM_DNN_RNN_INTERNAL_CI, LIBXSMM_DNN_RNN_INTERNAL_CO, LIBXSMM_DNN_REGULAR_INPUT };
/* the files of the command line, in order, and the tensors written afterwards: indices into `types` */
static const int in_index[6] = { 0, 2, 1, 3, 4, 7 };
static const int out_index[7] = { 9, 8, 18, 19, 20, 21, 22 };
static const char* const out_name[7] = { "h", "cs", "i", "f", "o", "ci", "co" };

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
  libxsmm_dnn_rnncell_desc desc;
  libxsmm_dnn_rnncell* handle;
  libxsmm_dnn_tensor* tensor[NTYPES];
  void* data[NTYPES];
  size_t bytes[NTYPES];
  libxsmm_dnn_err_t status;
  int seq, run, i, j, kind;
  const char* prefix;
  if (24 != argc) { fprintf(stderr, "see the head of rnn_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.K = atoi(argv[3]); desc.max_T = atoi(argv[4]);
  desc.cell_type = (libxsmm_dnn_rnncell_type)atoi(argv[5]); desc.bn = atoi(argv[6]); desc.bc = atoi(argv[7]); desc.bk = atoi(argv[8]);
  desc.threads = atoi(argv[9]); desc.datatype_in = (libxsmm_dnn_datatype)atoi(argv[10]); desc.datatype_out = (libxsmm_dnn_datatype)atoi(argv[11]);
  desc.buffer_format = (libxsmm_dnn_tensor_format)atoi(argv[12]); desc.filter_format = (libxsmm_dnn_tensor_format)atoi(argv[13]);
  seq = atoi(argv[14]); run = atoi(argv[16]); prefix = argv[23];
  for (i = 0; i < NMETA; ++i) meta[i] = -1;
  for (i = 0; i < NTYPES; ++i) { tensor[i] = NULL; data[i] = NULL; bytes[i] = 0; }
  libxsmm_init();
  status = 0xdead;
  handle = libxsmm_dnn_create_rnncell(desc, &status);
  meta[0] = status; meta[1] = (NULL != handle);
  meta[69] = libxsmm_dnn_rnncell_allocate_forget_bias(NULL, 1.f);
  (void)libxsmm_dnn_rnncell_get_sequence_length(NULL, &status); meta[74] = status;
  meta[75] = libxsmm_dnn_rnncell_set_sequence_length(NULL, 1);
  meta[79] = libxsmm_dnn_destroy_rnncell(NULL);
  if (NULL != handle) {
    size_t scratch_bytes = 64, state_bytes = 64;
    char *scratch, *state;
    for (kind = 0; kind < 6; ++kind) {
      meta[2 + 2 * kind] = (long long)libxsmm_dnn_rnncell_get_scratch_size(handle, (libxsmm_dnn_compute_kind)kind, &status); meta[3 + 2 * kind] = status;
      if ((size_t)meta[2 + 2 * kind] > scratch_bytes) scratch_bytes = (size_t)meta[2 + 2 * kind];
      meta[14 + 2 * kind] = (long long)libxsmm_dnn_rnncell_get_internalstate_size(handle, (libxsmm_dnn_compute_kind)kind, &status); meta[15 + 2 * kind] = status;
      if ((size_t)meta[14 + 2 * kind] > state_bytes) state_bytes = (size_t)meta[14 + 2 * kind];
    }
    scratch = (char*)libxsmm_aligned_malloc(scratch_bytes + 64, 64); memset(scratch, 0, scratch_bytes + 64);
    state = (char*)libxsmm_aligned_malloc(state_bytes + 64, 64); memset(state, 0xff, state_bytes + 64);
    for (i = 0; i < NTYPES; ++i) {
      long long* const m = meta + 80 + 26 * i;
      libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_rnncell_create_tensor_datalayout(handle, types[i], &status);
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
      if (NULL != tensor[i]) m[25] = libxsmm_dnn_rnncell_bind_tensor(handle, tensor[i], types[i]);
    }
    meta[62] = libxsmm_dnn_rnncell_bind_tensor(handle, NULL, LIBXSMM_DNN_RNN_REGULAR_INPUT);
    if (NULL != tensor[0] && NULL != tensor[9]) {
      meta[63] = libxsmm_dnn_rnncell_bind_tensor(handle, tensor[0], LIBXSMM_DNN_REGULAR_INPUT);
      meta[64] = libxsmm_dnn_rnncell_bind_tensor(NULL, tensor[0], LIBXSMM_DNN_RNN_REGULAR_INPUT);
      meta[76] = libxsmm_dnn_rnncell_bind_tensor(handle, tensor[0], LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE);
      (void)libxsmm_dnn_rnncell_bind_tensor(handle, tensor[9], LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE);
    }
    meta[65] = libxsmm_dnn_rnncell_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT);
    meta[66] = libxsmm_dnn_rnncell_release_tensor(NULL, LIBXSMM_DNN_RNN_REGULAR_INPUT);
    status = 0xdead; (void)libxsmm_dnn_rnncell_get_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT, &status); meta[67] = status;
    status = 0xdead; (void)libxsmm_dnn_rnncell_get_tensor(NULL, LIBXSMM_DNN_RNN_REGULAR_INPUT, &status); meta[68] = status;
    for (kind = 0; kind < 6; ++kind) {
      meta[26 + kind] = libxsmm_dnn_rnncell_bind_scratch(handle, (libxsmm_dnn_compute_kind)kind, NULL);
      meta[32 + kind] = libxsmm_dnn_rnncell_bind_scratch(handle, (libxsmm_dnn_compute_kind)kind, scratch + 4);
      if (5 != kind && LIBXSMM_DNN_SUCCESS == meta[32 + kind] && meta[2 + 2 * kind] > 0) {
        meta[77] = ((void*)(scratch + 4) == libxsmm_dnn_rnncell_get_scratch_ptr(handle, &status));
      }
      meta[38 + kind] = libxsmm_dnn_rnncell_release_scratch(handle, (libxsmm_dnn_compute_kind)kind);
      meta[44 + kind] = libxsmm_dnn_rnncell_bind_internalstate(handle, (libxsmm_dnn_compute_kind)kind, NULL);
      meta[50 + kind] = libxsmm_dnn_rnncell_bind_internalstate(handle, (libxsmm_dnn_compute_kind)kind, state + 4);
      if (5 != kind && meta[14 + 2 * kind] > 0) meta[78] = ((void*)(state + 64) == libxsmm_dnn_rnncell_get_internalstate_ptr(handle, &status));
      meta[56 + kind] = libxsmm_dnn_rnncell_release_internalstate(handle, (libxsmm_dnn_compute_kind)kind);
    }
    meta[70] = libxsmm_dnn_rnncell_set_sequence_length(handle, desc.max_T + 1);
    meta[71] = libxsmm_dnn_rnncell_get_sequence_length(handle, &status); meta[72] = status;
    if (0 <= seq) meta[73] = libxsmm_dnn_rnncell_set_sequence_length(handle, seq);
    if (0 != strcmp(argv[15], "-")) (void)libxsmm_dnn_rnncell_allocate_forget_bias(handle, (float)atof(argv[15]));
    for (i = 0; i < 6; ++i) if (NULL != data[in_index[i]]) slurp(argv[17 + i], data[in_index[i]], bytes[in_index[i]]);
    (void)libxsmm_dnn_rnncell_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, scratch);
    (void)libxsmm_dnn_rnncell_bind_internalstate(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, state);
    if (0 != run) {
      meta[704] = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0);
      meta[705] = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, 0, 0);
      meta[706] = libxsmm_dnn_rnncell_execute_st(handle, (libxsmm_dnn_compute_kind)7, 0, 0);
      for (i = 0; i < 7; ++i) if (NULL != data[out_index[i]]) dump(prefix, out_name[i], data[out_index[i]], bytes[out_index[i]]);
      if (meta[14] > 0) dump(prefix, "z", state, (size_t)meta[14] - 64);
    }
    for (i = 0; i < NTYPES; ++i) { if (NULL != tensor[i]) libxsmm_dnn_destroy_tensor(tensor[i]); if (NULL != data[i]) libxsmm_free(data[i]); }
    libxsmm_dnn_destroy_rnncell(handle);
    libxsmm_free(scratch); libxsmm_free(state);
  }
  dump(prefix, "meta", meta, sizeof(meta));
  return 0;
}
