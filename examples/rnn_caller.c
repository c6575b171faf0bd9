/* rnn_caller.c -- a caller of the RNN cell layer written against the reference's interface only (libxsmm_dnn.h and
 * libxsmm_dnn_rnncell.h as the reference declares them): one LSTM and one GRU forward pass over T = 3 steps on host tensors in the
 * plain NC / CK formats, with one element of the last hidden state recomputed by hand in plain loops. Returns 0.
 *   gcc -std=c99 -O1 -I include examples/rnn_caller.c -L <libdir> -lxsmm -lm -o rnn_caller
 * It links against the reference's library the same way. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_rnncell.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NN 4
#define CC 6
#define KK 8
#define TT 3

static float sigmoidf_(float v) { const float e = (float)exp((double)-v); return 1.0f / (1.0f + e); }
static float tanhf_(float v) { return (float)tanh((double)v); }
static float value(unsigned int* state) { *state = *state * 1664525u + 1013904223u; return ((float)(*state >> 8) / 8388608.0f - 1.0f) * 0.5f; }

static libxsmm_dnn_tensor* bind(libxsmm_dnn_rnncell* handle, libxsmm_dnn_tensor_type type, void* data, int* failures)
{
  libxsmm_dnn_err_t status;
  libxsmm_dnn_tensor_datalayout* layout = libxsmm_dnn_rnncell_create_tensor_datalayout(handle, type, &status);
  libxsmm_dnn_tensor* tensor = NULL;
  if (NULL == layout) { ++*failures; return NULL; }
  tensor = libxsmm_dnn_link_tensor(layout, data, &status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  if (NULL == tensor || LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_bind_tensor(handle, tensor, type)) ++*failures;
  return tensor;
}

/* the chain of gate `gate` (its columns start at gate * KK, the leading dimension is G * KK) for row n and output k */
static float chain(const float* w, const float* r, const float* b, int G, int gate, const float* x, const float* h, int n, int k)
{
  float acc = b[gate * KK + k];
  int c;
  for (c = 0; c < CC; ++c) acc = fmaf(w[c * G * KK + gate * KK + k], x[n * CC + c], acc);
  for (c = 0; c < KK; ++c) acc = fmaf(r[c * G * KK + gate * KK + k], h[n * KK + c], acc);
  return acc;
}

static int run(libxsmm_dnn_rnncell_type cell, const char* name)
{
  const int G = (LIBXSMM_DNN_RNNCELL_LSTM == cell) ? 4 : 3;
  static float x[TT * NN * CC], hp[TT * NN * KK], csp[TT * NN * KK], w[CC * 4 * KK], r[KK * 4 * KK], b[4 * KK];
  static float h[TT * NN * KK], cs[TT * NN * KK], gi[TT * NN * KK], gf[TT * NN * KK], go[TT * NN * KK], gci[TT * NN * KK], gco[TT * NN * KK];
  static float href[TT * NN * KK], csref[TT * NN * KK], oref[NN * KK];
  libxsmm_dnn_rnncell_desc desc;
  libxsmm_dnn_rnncell* handle;
  libxsmm_dnn_tensor* tensors[13];
  libxsmm_dnn_err_t status;
  unsigned int seed = 42u + (unsigned int)cell;
  int failures = 0, nt = 0, i, t, n, k;
  size_t scratch_size;
  void* scratch;
  for (i = 0; i < TT * NN * CC; ++i) x[i] = value(&seed);
  for (i = 0; i < TT * NN * KK; ++i) { hp[i] = value(&seed); csp[i] = value(&seed); }
  for (i = 0; i < CC * 4 * KK; ++i) w[i] = value(&seed);
  for (i = 0; i < KK * 4 * KK; ++i) r[i] = value(&seed);
  for (i = 0; i < 4 * KK; ++i) b[i] = value(&seed);
  memset(&desc, 0, sizeof(desc));
  desc.threads = 1; desc.N = NN; desc.C = CC; desc.K = KK; desc.max_T = TT; desc.bn = 2; desc.bc = 3; desc.bk = 4;
  desc.cell_type = cell; desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_NC; desc.filter_format = LIBXSMM_DNN_TENSOR_FORMAT_CK;
  handle = libxsmm_dnn_create_rnncell(desc, &status);
  if (NULL == handle || LIBXSMM_DNN_SUCCESS != status) { printf("rnn_caller: %s create failed (%s)\n", name, libxsmm_dnn_get_error(status)); return 1; }
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_INPUT, x, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV, hp, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_WEIGHT, w, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT, r, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_BIAS, b, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE, h, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_I, gi, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_F, gf, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_O, go, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_CI, gci, &failures);
  if (LIBXSMM_DNN_RNNCELL_LSTM == cell) {
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_CS_PREV, csp, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_CS, cs, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_CO, gco, &failures);
    if (LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_allocate_forget_bias(handle, 1.0f)) ++failures;
  }
  scratch_size = libxsmm_dnn_rnncell_get_scratch_size(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, &status);
  scratch = malloc(scratch_size + 64);
  if (NULL == scratch || LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, scratch)) ++failures;
  if (LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_set_sequence_length(handle, TT) || TT != libxsmm_dnn_rnncell_get_sequence_length(handle, &status)) ++failures;
  if (0 == failures) {
    status = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0);
    if (LIBXSMM_DNN_SUCCESS != status) { printf("rnn_caller: %s execute_st failed (%s)\n", name, libxsmm_dnn_get_error(status)); ++failures; }
  }
  /* by hand: every step in plain loops */
  for (t = 0; t < TT && 0 == failures; ++t) {
    const float* hprev = (0 == t) ? hp : href + (t - 1) * NN * KK;
    const float* xt = x + t * NN * CC;
    for (n = 0; n < NN; ++n) for (k = 0; k < KK; ++k) {
      if (LIBXSMM_DNN_RNNCELL_LSTM == cell) {
        const float iv = sigmoidf_(chain(w, r, b, G, 0, xt, hprev, n, k)), civ = tanhf_(chain(w, r, b, G, 1, xt, hprev, n, k));
        float fpre = b[2 * KK + k] + 1.0f, csv;
        int c;
        for (c = 0; c < CC; ++c) fpre = fmaf(w[c * G * KK + 2 * KK + k], xt[n * CC + c], fpre);
        for (c = 0; c < KK; ++c) fpre = fmaf(r[c * G * KK + 2 * KK + k], hprev[n * KK + c], fpre);
        csv = sigmoidf_(fpre) * ((0 == t) ? csp : csref + (t - 1) * NN * KK)[n * KK + k];
        { volatile float prod = iv * civ; csv = csv + prod; }
        csref[t * NN * KK + n * KK + k] = csv;
        href[t * NN * KK + n * KK + k] = sigmoidf_(chain(w, r, b, G, 3, xt, hprev, n, k)) * tanhf_(csv);
      }
      else oref[n * KK + k] = hprev[n * KK + k] * sigmoidf_(chain(w, r, b, G, 0, xt, hprev, n, k));
    }
    if (LIBXSMM_DNN_RNNCELL_GRU == cell) {
      for (n = 0; n < NN; ++n) for (k = 0; k < KK; ++k) {
        const float cv = sigmoidf_(chain(w, r, b, G, 1, xt, hprev, n, k)), fv = tanhf_(chain(w, r, b, G, 2, xt, oref, n, k));
        volatile float first = (1.0f - cv) * fv, second = cv * hprev[n * KK + k];
        href[t * NN * KK + n * KK + k] = first + second;
      }
    }
  }
  if (0 == failures) {
    const int at = (TT - 1) * NN * KK + 2 * KK + 5; /* the last step, row 2, output 5 */
    int mismatches = 0;
    for (i = 0; i < TT * NN * KK; ++i) if (fabsf(h[i] - href[i]) > 1e-6f) ++mismatches;
    printf("rnn_caller: %s h[%d][2][5] = %.9g, by hand %.9g, %d mismatches\n", name, TT - 1, (double)h[at], (double)href[at], mismatches);
    if (fabsf(h[at] - href[at]) > 1e-6f || 0 != mismatches) ++failures;
  }
  libxsmm_dnn_rnncell_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD);
  for (i = 0; i < nt; ++i) if (NULL != tensors[i]) libxsmm_dnn_destroy_tensor(tensors[i]);
  libxsmm_dnn_destroy_rnncell(handle);
  free(scratch);
  return failures;
}

int main(void)
{
  int failures;
  libxsmm_init();
  failures = run(LIBXSMM_DNN_RNNCELL_LSTM, "lstm") + run(LIBXSMM_DNN_RNNCELL_GRU, "gru");
  libxsmm_finalize();
  return 0 == failures ? 0 : 1;
}
