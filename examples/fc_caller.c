/* fc_caller.c -- the call sequence of the reference's fully-connected sample (samples/deeplearning/fullyconnecteddriver/
 * layer_example_f32.c), written against the reference API only: create the handle, ask it for the six layouts, link tensors
 * to buffers from libxsmm_aligned_malloc, fill them (copy-in from plain NCHW / KCRS in format 'L', a hand-blocked fill in
 * format 'B'), bind, size and bind the scratch, execute FWD, BWD and UPD for every logical thread, bring the results back to
 * plain (copy-out or by hand), and compare with naive loops through libxsmm_matdiff. The sample fails a run whose
 * Check-norm (normf_rel) exceeds 1 % (CHECK=1); so does this one.
 *   fc_caller [L|B] [N C K] [threads]        default: L 70 48 80 3 */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <libxsmm_dnn_fullyconnected.h>
#include <stdio.h>
#include <stdlib.h>

/* a warning (a status below LIBXSMM_DNN_ERR_GENERAL) is no failure */
#define CHKERR(STATUS) do { const libxsmm_dnn_err_t chkerr_ = (STATUS); if (chkerr_ >= LIBXSMM_DNN_ERR_GENERAL) { \
  fprintf(stderr, "%s (line %d)\n", libxsmm_dnn_get_error(chkerr_), __LINE__); exit(EXIT_FAILURE); } } while (0)

static float* buffer(size_t n) { return (float*)libxsmm_aligned_malloc(n * sizeof(float), 2097152); }

static void fill(float* p, size_t n, unsigned int seed)
{
  size_t i;
  for (i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; p[i] = (float)((seed >> 8) & 0xffff) / 65536.f - 0.5f; }
}

/* plain [N][F] <-> packed [N/bn][F/bf][bn][bf] */
static void pack_act(const float* plain, float* packed, int N, int F, int bn, int bf, int unpack)
{
  int n, f;
  for (n = 0; n < N; ++n) for (f = 0; f < F; ++f) {
    const size_t b = (((size_t)(n / bn) * (F / bf) + f / bf) * bn + n % bn) * bf + f % bf, p = (size_t)n * F + f;
    if (unpack) ((float*)plain)[p] = packed[b]; else packed[b] = plain[p];
  }
}

/* plain [K][C] <-> packed [K/bk][C/bc][bc][bk] */
static void pack_fil(const float* plain, float* packed, int K, int C, int bk, int bc, int unpack)
{
  int k, c;
  for (k = 0; k < K; ++k) for (c = 0; c < C; ++c) {
    const size_t b = (((size_t)(k / bk) * (C / bc) + c / bc) * bc + c % bc) * bk + k % bk, p = (size_t)k * C + c;
    if (unpack) ((float*)plain)[p] = packed[b]; else packed[b] = plain[p];
  }
}

int main(int argc, char* argv[])
{
  const char format = (1 < argc ? argv[1][0] : 'L');
  const int N = (4 < argc ? atoi(argv[2]) : 70), C = (4 < argc ? atoi(argv[3]) : 48), K = (4 < argc ? atoi(argv[4]) : 80);
  const int threads = (5 < argc ? atoi(argv[5]) : 3);
  const int bn = 10, bc = 16, bk = 16; /* format B */
  const size_t nx = (size_t)N * C, ny = (size_t)N * K, nw = (size_t)K * C;
  float *x = buffer(nx), *w = buffer(nw), *dy = buffer(ny);                 /* plain operands */
  float *y_ref = buffer(ny), *dx_ref = buffer(nx), *dw_ref = buffer(nw);     /* naive results */
  float *y_out = buffer(ny), *dx_out = buffer(nx), *dw_out = buffer(nw);     /* the layer's results, plain */
  float *tx = buffer(nx), *ty = buffer(ny), *tdx = buffer(nx), *tdy = buffer(ny), *tw = buffer(nw), *tdw = buffer(nw); /* tensors */
  libxsmm_dnn_fullyconnected_desc desc;
  libxsmm_dnn_fullyconnected* handle;
  libxsmm_dnn_tensor_datalayout* layout;
  libxsmm_dnn_tensor *t_x, *t_y, *t_dx, *t_dy, *t_w, *t_dw;
  libxsmm_dnn_err_t status;
  libxsmm_matdiff_info norms[3], diff;
  void* scratch;
  size_t scratch_size;
  int n, c, k, tid, pass;
  double worst = 0;

  fill(x, nx, 1); fill(w, nw, 2); fill(dy, ny, 3);
  for (n = 0; n < N; ++n) for (k = 0; k < K; ++k) { float s = 0; for (c = 0; c < C; ++c) s += w[(size_t)k * C + c] * x[(size_t)n * C + c]; y_ref[(size_t)n * K + k] = s; }
  for (n = 0; n < N; ++n) for (c = 0; c < C; ++c) { float s = 0; for (k = 0; k < K; ++k) s += w[(size_t)k * C + c] * dy[(size_t)n * K + k]; dx_ref[(size_t)n * C + c] = s; }
  for (k = 0; k < K; ++k) for (c = 0; c < C; ++c) { float s = 0; for (n = 0; n < N; ++n) s += dy[(size_t)n * K + k] * x[(size_t)n * C + c]; dw_ref[(size_t)k * C + c] = s; }

  desc.N = N; desc.C = C; desc.K = K; desc.bn = bn; desc.bk = bk; desc.bc = bc; desc.threads = threads;
  desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = ('L' == format ? LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM : LIBXSMM_DNN_TENSOR_FORMAT_NCPACKED);
  desc.filter_format = ('L' == format ? LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM : LIBXSMM_DNN_TENSOR_FORMAT_CKPACKED);
  desc.fuse_ops = LIBXSMM_DNN_FULLYCONNECTED_FUSE_NONE;
  handle = libxsmm_dnn_create_fullyconnected(desc, &status); CHKERR(status);
  if (NULL == handle || ('B' == format && LIBXSMM_DNN_SUCCESS != status)) { fprintf(stderr, "no handle for these sizes\n"); return EXIT_FAILURE; }

#define LINK(T, TYPE, DATA) \
  layout = libxsmm_dnn_fullyconnected_create_tensor_datalayout(handle, TYPE, &status); CHKERR(status); \
  T = libxsmm_dnn_link_tensor(layout, DATA, &status); CHKERR(status); \
  libxsmm_dnn_destroy_tensor_datalayout(layout)
  LINK(t_x, LIBXSMM_DNN_REGULAR_INPUT, tx); LINK(t_dx, LIBXSMM_DNN_GRADIENT_INPUT, tdx);
  LINK(t_y, LIBXSMM_DNN_REGULAR_OUTPUT, ty); LINK(t_dy, LIBXSMM_DNN_GRADIENT_OUTPUT, tdy);
  LINK(t_w, LIBXSMM_DNN_REGULAR_FILTER, tw); LINK(t_dw, LIBXSMM_DNN_GRADIENT_FILTER, tdw);

  if ('L' == format) {
    CHKERR(libxsmm_dnn_copyin_tensor(t_x, x, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
    CHKERR(libxsmm_dnn_copyin_tensor(t_dy, dy, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
    CHKERR(libxsmm_dnn_copyin_tensor(t_w, w, LIBXSMM_DNN_TENSOR_FORMAT_KCRS));
  }
  else { pack_act(x, tx, N, C, bn, bc, 0); pack_act(dy, tdy, N, K, bn, bk, 0); pack_fil(w, tw, K, C, bk, bc, 0); }
  CHKERR(libxsmm_dnn_zero_tensor(t_y)); CHKERR(libxsmm_dnn_zero_tensor(t_dx)); CHKERR(libxsmm_dnn_zero_tensor(t_dw));

  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_x, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_dx, LIBXSMM_DNN_GRADIENT_INPUT));
  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_y, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_dy, LIBXSMM_DNN_GRADIENT_OUTPUT));
  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_w, LIBXSMM_DNN_REGULAR_FILTER));
  CHKERR(libxsmm_dnn_fullyconnected_bind_tensor(handle, t_dw, LIBXSMM_DNN_GRADIENT_FILTER));
  scratch_size = libxsmm_dnn_fullyconnected_get_scratch_size(handle, &status); CHKERR(status);
  scratch = libxsmm_aligned_malloc(scratch_size, 2097152);
  CHKERR(libxsmm_dnn_fullyconnected_bind_scratch(handle, scratch));

  for (pass = 0; pass < 3; ++pass) { /* the sample's parallel region: every thread executes its share */
    const libxsmm_dnn_compute_kind kind = (0 == pass ? LIBXSMM_DNN_COMPUTE_KIND_FWD : (1 == pass ? LIBXSMM_DNN_COMPUTE_KIND_BWD : LIBXSMM_DNN_COMPUTE_KIND_UPD));
    for (tid = 0; tid < threads; ++tid) CHKERR(libxsmm_dnn_fullyconnected_execute_st(handle, kind, 0, tid));
  }

  if ('L' == format) {
    CHKERR(libxsmm_dnn_copyout_tensor(t_y, y_out, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
    CHKERR(libxsmm_dnn_copyout_tensor(t_dx, dx_out, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
    CHKERR(libxsmm_dnn_copyout_tensor(t_dw, dw_out, LIBXSMM_DNN_TENSOR_FORMAT_KCRS));
  }
  else { pack_act(y_out, ty, N, K, bn, bk, 1); pack_act(dx_out, tdx, N, C, bn, bc, 1); pack_fil(dw_out, tdw, K, C, bk, bc, 1); }

  libxsmm_matdiff_clear(&diff);
  libxsmm_matdiff(&norms[0], LIBXSMM_DATATYPE_F32, (libxsmm_blasint)ny, 1, y_ref, y_out, 0, 0);
  libxsmm_matdiff(&norms[1], LIBXSMM_DATATYPE_F32, (libxsmm_blasint)nx, 1, dx_ref, dx_out, 0, 0);
  libxsmm_matdiff(&norms[2], LIBXSMM_DATATYPE_F32, (libxsmm_blasint)nw, 1, dw_ref, dw_out, 0, 0);
  for (pass = 0; pass < 3; ++pass) {
    printf("fc_caller %c pass %d: L1 reference %.9g, L1 test %.9g, Linf abs.error %.9g, Check-norm %.12f\n", format, pass,
      norms[pass].l1_ref, norms[pass].l1_tst, norms[pass].linf_abs, norms[pass].normf_rel);
    if (norms[pass].normf_rel > worst) worst = norms[pass].normf_rel;
    if (!(0 < norms[pass].l1_tst)) worst = 1; /* nothing was computed */
  }

  CHKERR(libxsmm_dnn_fullyconnected_release_scratch(handle));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_GRADIENT_INPUT));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_GRADIENT_OUTPUT));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_REGULAR_FILTER));
  CHKERR(libxsmm_dnn_fullyconnected_release_tensor(handle, LIBXSMM_DNN_GRADIENT_FILTER));
  CHKERR(libxsmm_dnn_destroy_tensor(t_x)); CHKERR(libxsmm_dnn_destroy_tensor(t_dx)); CHKERR(libxsmm_dnn_destroy_tensor(t_y));
  CHKERR(libxsmm_dnn_destroy_tensor(t_dy)); CHKERR(libxsmm_dnn_destroy_tensor(t_w)); CHKERR(libxsmm_dnn_destroy_tensor(t_dw));
  CHKERR(libxsmm_dnn_destroy_fullyconnected(handle));
  libxsmm_free(scratch);
  libxsmm_free(x); libxsmm_free(w); libxsmm_free(dy); libxsmm_free(y_ref); libxsmm_free(dx_ref); libxsmm_free(dw_ref);
  libxsmm_free(y_out); libxsmm_free(dx_out); libxsmm_free(dw_out);
  libxsmm_free(tx); libxsmm_free(ty); libxsmm_free(tdx); libxsmm_free(tdy); libxsmm_free(tw); libxsmm_free(tdw);
  if (worst > 0.01) { fprintf(stderr, "FAILED with an error of %f%%!\n", 100.0 * worst); return EXIT_FAILURE; }
  printf("fc_caller %c: check norm %.12f below the sample's threshold of 0.01\n", format, worst);
  return EXIT_SUCCESS;
}
