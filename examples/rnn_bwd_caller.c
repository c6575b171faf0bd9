/* rnn_bwd_caller.c -- a caller of the RNN cell layer's backward and update passes written against the reference's interface only
 * (libxsmm_dnn.h and libxsmm_dnn_rnncell.h as the reference declares them): one LSTM and one tanh cell, FWD and then BWDUPD over
 * T = 3 steps on host tensors in the plain NC / CK formats, with every gradient recomputed by hand in plain loops from what the
 * forward pass stored. Returns 0.
 *   gcc -std=c99 -O1 -I include examples/rnn_bwd_caller.c -L <libdir> -lxsmm -lm -o rnn_bwd_caller
 * It links against the reference's library the same way. */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_rnncell.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NN 4
#define CC 6
#define KK 8
#define TT 3
#define NK (NN * KK)
#define TOL 2e-5f

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

static int differ(const char* name, const char* what, const float* got, const float* want, int count)
{
  int i, bad = 0;
  for (i = 0; i < count; ++i) if (!(fabsf(got[i] - want[i]) <= TOL * (1.0f + fabsf(want[i])))) ++bad;
  printf("rnn_bwd_caller: %s %s[1] = %.9g, by hand %.9g, %d mismatches\n", name, what, (double)got[1], (double)want[1], bad);
  return bad;
}

static int run(libxsmm_dnn_rnncell_type cell, const char* name)
{
  const int lstm = (LIBXSMM_DNN_RNNCELL_LSTM == cell), G = lstm ? 4 : 1, LD = G * KK;
  static float x[TT * NN * CC], hp[TT * NK], csp[TT * NK], w[CC * 4 * KK], r[KK * 4 * KK], b[4 * KK], dh[TT * NK], dcs[TT * NK];
  static float h[TT * NK], cs[TT * NK], gi[TT * NK], gf[TT * NK], go[TT * NK], gci[TT * NK], gco[TT * NK], zmem[TT * NK + 16];
  static float dx[TT * NN * CC], dcsp[TT * NK], dhp[TT * NK], dw[CC * 4 * KK], dr[KK * 4 * KK], db[4 * KK];
  static float delta[TT * NN * 4 * KK], rdx[TT * NN * CC], rdcp[NK], rdhp[NK], rdw[CC * 4 * KK], rdr[KK * 4 * KK], rdb[4 * KK], dout[NK];
  libxsmm_dnn_rnncell_desc desc;
  libxsmm_dnn_rnncell* handle;
  libxsmm_dnn_tensor* tensors[24];
  libxsmm_dnn_err_t status;
  unsigned int seed = 4242u + (unsigned int)cell;
  int failures = 0, nt = 0, i, t, n, k, c, q;
  size_t scratch_size;
  void* scratch;
  float* z = (float*)(((uintptr_t)zmem + 63) & ~(uintptr_t)63);
  for (i = 0; i < TT * NN * CC; ++i) x[i] = value(&seed);
  for (i = 0; i < TT * NK; ++i) { hp[i] = value(&seed); csp[i] = value(&seed); dh[i] = value(&seed); dcs[i] = value(&seed); }
  for (i = 0; i < CC * 4 * KK; ++i) w[i] = value(&seed);
  for (i = 0; i < KK * 4 * KK; ++i) r[i] = value(&seed);
  for (i = 0; i < 4 * KK; ++i) b[i] = value(&seed);
  memset(dx, 0xff, sizeof(dx)); memset(dw, 0xff, sizeof(dw)); memset(dr, 0xff, sizeof(dr)); memset(db, 0xff, sizeof(db));
  memset(dcsp, 0xff, sizeof(dcsp)); memset(dhp, 0xff, sizeof(dhp));
  memset(&desc, 0, sizeof(desc));
  desc.threads = 1; desc.N = NN; desc.C = CC; desc.K = KK; desc.max_T = TT; desc.bn = 2; desc.bc = 3; desc.bk = 4;
  desc.cell_type = cell; desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_NC; desc.filter_format = LIBXSMM_DNN_TENSOR_FORMAT_CK;
  handle = libxsmm_dnn_create_rnncell(desc, &status);
  if (NULL == handle || LIBXSMM_DNN_SUCCESS != status) { printf("rnn_bwd_caller: %s create failed (%s)\n", name, libxsmm_dnn_get_error(status)); return 1; }
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_INPUT, x, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE_PREV, hp, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_WEIGHT, w, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_RECUR_WEIGHT, r, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_BIAS, b, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_HIDDEN_STATE, h, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_INPUT, dx, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_WEIGHT, dw, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_RECUR_WEIGHT, dr, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_BIAS, db, &failures);
  tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE, dh, &failures);
  if (lstm) {
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_CS_PREV, csp, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_REGULAR_CS, cs, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_I, gi, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_F, gf, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_O, go, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_CI, gci, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_INTERNAL_CO, gco, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_CS, dcs, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_CS_PREV, dcsp, &failures);
    tensors[nt++] = bind(handle, LIBXSMM_DNN_RNN_GRADIENT_HIDDEN_STATE_PREV, dhp, &failures);
  }
  else if (LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_bind_internalstate(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, z)) ++failures;
  scratch_size = libxsmm_dnn_rnncell_get_scratch_size(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, &status);
  scratch = malloc(scratch_size + 64);
  if (NULL == scratch || LIBXSMM_DNN_SUCCESS != libxsmm_dnn_rnncell_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, scratch)) ++failures;
  if (NULL != scratch) memset(scratch, 0, scratch_size + 64);
  if (0 == failures) {
    status = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0);
    if (LIBXSMM_DNN_SUCCESS == status) status = libxsmm_dnn_rnncell_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD, 0, 0);
    if (LIBXSMM_DNN_SUCCESS != status) { printf("rnn_bwd_caller: %s execute_st failed (%s)\n", name, libxsmm_dnn_get_error(status)); ++failures; }
  }
  /* by hand, from what the forward pass stored: the deltas [step][row][gate][k] backwards in time, then the gradients */
  memset(rdw, 0, sizeof(rdw)); memset(rdr, 0, sizeof(rdr)); memset(rdb, 0, sizeof(rdb)); memset(rdhp, 0, sizeof(rdhp));
  for (t = TT - 1; t >= 0 && 0 == failures; --t) {
    for (n = 0; n < NN; ++n) for (k = 0; k < KK; ++k) {
      const int at = t * NK + n * KK + k;
      float back = 0.f; /* what the step after hands back through r */
      if (t < TT - 1) for (q = 0; q < LD; ++q) back += r[k * LD + q] * delta[((t + 1) * NN + n) * LD + q];
      if (!lstm) {
        const float th = (float)tanh((double)z[at]);
        delta[(t * NN + n) * LD + k] = (dh[at] + back) * (1.0f - th * th);
      }
      else {
        const float d_out = dh[at] + back, cprev = (0 == t) ? csp[n * KK + k] : cs[at - NK];
        const float d_cp = ((TT - 1 == t) ? dcs[n * KK + k] : rdcp[n * KK + k]) + d_out * go[at] * (1.0f - gco[at] * gco[at]);
        float* const d = delta + (t * NN + n) * LD + k;
        d[0] = d_cp * gci[at] * gi[at] * (1.0f - gi[at]);
        d[KK] = d_cp * gi[at] * (1.0f - gci[at] * gci[at]);
        d[2 * KK] = d_cp * cprev * gf[at] * (1.0f - gf[at]);
        d[3 * KK] = d_out * gco[at] * go[at] * (1.0f - go[at]);
        dout[n * KK + k] = d_cp * gf[at]; /* the running dcp, for the step before */
      }
    }
    if (lstm) memcpy(rdcp, dout, sizeof(rdcp));
    for (n = 0; n < NN; ++n) {
      const float* const d = delta + (t * NN + n) * LD;
      const float* const hprev = (0 == t) ? hp + n * KK : h + (t - 1) * NK + n * KK;
      for (c = 0; c < CC; ++c) {
        float s = 0.f;
        for (q = 0; q < LD; ++q) { s += w[c * LD + q] * d[q]; rdw[c * LD + q] += x[(t * NN + n) * CC + c] * d[q]; }
        rdx[(t * NN + n) * CC + c] = s;
      }
      for (c = 0; c < KK; ++c) for (q = 0; q < LD; ++q) rdr[c * LD + q] += hprev[c] * d[q];
      for (q = 0; q < LD; ++q) rdb[q] += d[q];
      if (lstm && 0 == t) for (k = 0; k < KK; ++k) for (q = 0; q < LD; ++q) rdhp[n * KK + k] += r[k * LD + q] * d[q];
    }
  }
  if (0 == failures) {
    failures += differ(name, "dx", dx, rdx, TT * NN * CC) + differ(name, "dw", dw, rdw, CC * LD) + differ(name, "dr", dr, rdr, KK * LD) + differ(name, "db", db, rdb, LD);
    if (lstm) failures += differ(name, "dcsp", dcsp, rdcp, NK) + differ(name, "dhp", dhp, rdhp, NK);
  }
  libxsmm_dnn_rnncell_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_BWDUPD);
  for (i = 0; i < nt; ++i) if (NULL != tensors[i]) libxsmm_dnn_destroy_tensor(tensors[i]);
  libxsmm_dnn_destroy_rnncell(handle);
  free(scratch);
  return failures;
}

int main(void)
{
  int failures;
  libxsmm_init();
  failures = run(LIBXSMM_DNN_RNNCELL_LSTM, "lstm") + run(LIBXSMM_DNN_RNNCELL_RNN_TANH, "tanh");
  libxsmm_finalize();
  return 0 == failures ? 0 : 1;
}
