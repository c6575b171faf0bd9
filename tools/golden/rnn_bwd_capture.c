/* rnn_bwd_capture.c -- calls the backward and update passes of the RNN cell layer of the unmodified reference through its public
 * functions only and writes what they return as raw binary, for tools/golden/rnn_bwd_capture.py to pack into
 * tests/golden/rnn_bwd.npz. Built against the reference's static library like rnn_capture.c:
 *   gcc -O1 -I<reference>/include rnn_bwd_capture.c <reference>/lib/libxsmm.a -lm -lpthread -ldl -lrt -o rnn_bwd_capture
 * Usage: rnn_bwd_capture N C K max_T cell bn bc bk seq  x hp csp w r b dh dcs  plant_z plant_o  prefix
 *   seq: the sequence length to set before the passes, or -1 to leave max_T
 *   x ... dcs: files holding these tensors as fp32 in their own layout, or "-" (left as 0xff bytes)
 *   plant_z, plant_o: files that replace the internal state z or the gate tensor o AFTER the forward pass (special values), or "-"
 * The handle has threads = 1; execute_st is called with start_thread = tid = 0, scratch and internal state bound. FWD runs first
 * (it writes h, cs, i, f, o, ci, co and z, which the backward passes read), then BWD (1), UPD (2) and BWDUPD (3), each on gradient
 * destinations refilled with 0xff bytes and a scratch refilled with zero bytes.
 * Writes prefix.meta (long long: [0] create status, [1] FWD status, [2..4] the statuses of the three kinds), prefix.fwd.{h,cs,i,f,
 * o,ci,co,z} (as the backward passes saw them) and prefix.<kind>.{dx,dcsp,dhp,dw,dr,db}. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_rnncell.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NTYPES 23
static const libxsmm_dnn_tensor_type types[NTYPES] = { LIBXSMM_DNN_RNN_REGULAR_INPUT, LIBXSMM_DNN_RNN_REGULAR_CS_PREV,
  LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_REGULAR_WEIGHT, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT,
  LIBXSMM_DNN_RNN_REGULAR_WEIGHT_TRANS, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT_TRANS, LIBXSMM_DNN_RNN_REGULAR_BIAS, LIBXSMM_DNN_RNN_REGULAR_CS,
  LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE, LIBXSMM_DNN_RNN_GRADIENT_INPUT, LIBXSMM_DNN_RNN_GRADIENT_CS_PREV,
  LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV, LIBXSMM_DNN_RNN_GRADIENT_WEIGHT, LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT,
  LIBXSMM_DNN_RNN_GRADIENT_BIAS, LIBXSMM_DNN_RNN_GRADIENT_CS, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE, LIBXSMM_DNN_RNN_INTERNAL_I,
  LIBXSMM_DNN_RNN_INTERNAL_F, LIBXSMM_DNN_RNN_INTERNAL_O, LIBXSMM_DNN_RNN_INTERNAL_CI, LIBXSMM_DNN_RNN_INTERNAL_CO };
/* indices into `types` */
static const int in_index[8] = { 0, 2, 1, 3, 4, 7, 17, 16 };           /* x hp csp w r b dh dcs */
static const int fwd_index[7] = { 9, 8, 18, 19, 20, 21, 22 };          /* h cs i f o ci co */
static const char* const fwd_name[7] = { "h", "cs", "i", "f", "o", "ci", "co" };
static const int grad_index[6] = { 10, 11, 12, 13, 14, 15 };           /* dx dcsp dhp dw dr db */
static const char* const grad_name[6] = { "dx", "dcsp", "dhp", "dw", "dr", "db" };

static void slurp(const char* path, void* dst, size_t bytes)
{
  FILE* f;
  if (0 == strcmp(path, "-")) return;
  f = fopen(path, "rb");
  if (NULL == f || bytes != fread(dst, 1, bytes, f)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
}

static void dump(const char* prefix, const char* mid, const char* suffix, const void* p, size_t bytes)
{
  char path[1024];
  FILE* f;
  snprintf(path, sizeof(path), "%s.%s.%s", prefix, mid, suffix);
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
  size_t bytes[NTYPES], scratch_bytes = 64, state_bytes = 64;
  libxsmm_dnn_err_t status;
  long long meta[5] = { -1, -1, -1, -1, -1 };
  char *scratch, *state;
  const char* prefix;
  int seq, i, kind;
  if (21 != argc) { fprintf(stderr, "see the head of rnn_bwd_capture.c\n"); return 2; }
  memset(&desc, 0, sizeof(desc));
  desc.N = atoi(argv[1]); desc.C = atoi(argv[2]); desc.K = atoi(argv[3]); desc.max_T = atoi(argv[4]);
  desc.cell_type = (libxsmm_dnn_rnncell_type)atoi(argv[5]); desc.bn = atoi(argv[6]); desc.bc = atoi(argv[7]); desc.bk = atoi(argv[8]);
  desc.threads = 1; desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_NC; desc.filter_format = LIBXSMM_DNN_TENSOR_FORMAT_CK;
  seq = atoi(argv[9]); prefix = argv[20];
  libxsmm_init();
  handle = libxsmm_dnn_create_rnncell(desc, &status);
  meta[0] = status;
  if (NULL == handle) { fprintf(stderr, "no handle\n"); return 2; }
  for (kind = 0; kind < 4; ++kind) {
    const size_t a = libxsmm_dnn_rnncell_get_scratch_size(handle, (libxsmm_dnn_compute_kind)kind, &status);
    const size_t b = libxsmm_dnn_rnncell_get_internalstate_size(handle, (libxsmm_dnn_compute_kind)kind, &status);
    if (a > scratch_bytes) scratch_bytes = a;
    if (b > state_bytes) state_bytes = b;
  }
  scratch = (char*)libxsmm_aligned_malloc(scratch_bytes + 64, 64); memset(scratch, 0, scratch_bytes + 64);
  state = (char*)libxsmm_aligned_malloc(state_bytes + 64, 64); memset(state, 0xff, state_bytes + 64);
  for (i = 0; i < NTYPES; ++i) {
    libxsmm_dnn_tensor_datalayout* const layout = libxsmm_dnn_rnncell_create_tensor_datalayout(handle, types[i], &status);
    if (NULL == layout) { fprintf(stderr, "no layout %d\n", i); return 2; }
    bytes[i] = (size_t)libxsmm_dnn_get_tensor_size(layout, &status);
    data[i] = libxsmm_aligned_malloc(bytes[i] + 64, 64);
    memset(data[i], 0xff, bytes[i] + 64);
    tensor[i] = libxsmm_dnn_link_tensor(layout, data[i], &status);
    libxsmm_dnn_destroy_tensor_datalayout(layout);
    if (NULL == tensor[i] || LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_bind_tensor(handle, tensor[i], types[i])) { fprintf(stderr, "no tensor %d\n", i); return 2; }
  }
  if (0 <= seq && LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_set_sequence_length(handle, seq)) return 2;
  for (i = 0; i < 8; ++i) slurp(argv[10 + i], data[in_index[i]], bytes[in_index[i]]);
  (void)libxsmm_dnn_rnncell_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, scratch);
  (void)libxsmm_dnn_rnncell_bind_internalstate(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, state);
  meta[1] = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0);
  if (state_bytes > 64) slurp(argv[18], state, state_bytes - 64);
  slurp(argv[19], data[20], bytes[20]);
  for (i = 0; i < 7; ++i) dump(prefix, "fwd", fwd_name[i], data[fwd_index[i]], bytes[fwd_index[i]]);
  if (state_bytes > 64) dump(prefix, "fwd", "z", state, state_bytes - 64);
  for (kind = 1; kind < 4; ++kind) {
    char mid[8];
    for (i = 0; i < 6; ++i) memset(data[grad_index[i]], 0xff, bytes[grad_index[i]]);
    memset(scratch, 0, scratch_bytes + 64);
    (void)libxsmm_dnn_rnncell_bind_scratch(handle, (libxsmm_dnn_compute_kind)kind, scratch);
    (void)libxsmm_dnn_rnncell_bind_internalstate(handle, (libxsmm_dnn_compute_kind)kind, state);
    meta[1 + kind] = libxsmm_dnn_rnncell_execute_st(handle, (libxsmm_dnn_compute_kind)kind, 0, 0);
    snprintf(mid, sizeof(mid), "%d", kind);
    for (i = 0; i < 6; ++i) dump(prefix, mid, grad_name[i], data[grad_index[i]], bytes[grad_index[i]]);
  }
  for (i = 0; i < NTYPES; ++i) { libxsmm_dnn_destroy_tensor(tensor[i]); libxsmm_free(data[i]); }
  libxsmm_dnn_destroy_rnncell(handle);
  libxsmm_free(scratch); libxsmm_free(state);
  dump(prefix, "meta", "bin", meta, sizeof(meta));
  return 0;
}
