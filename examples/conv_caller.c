/* conv_caller.c -- one convolution layer through the reference's DNN interface only (include/libxsmm_dnn.h as the reference
 * declares it): create, layouts, link and bind the tensors, bind the scratch, then a FWD, BWD, UPD round. The tensors live in
 * plain host memory, so every call is complete on return. The self-check is exact in fp32: all values are small integers, so
 * every sum is exact whatever its order. Returns 0 if everything agrees with naive loops over the blocked tensors. */
#include <libxsmm_dnn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHKERR(call) do { const libxsmm_dnn_err_t chkerr_ = (call); if (LIBXSMM_DNN_SUCCESS != chkerr_) { \
  fprintf(stderr, "conv_caller: %s failed: %s\n", #call, libxsmm_dnn_get_error(chkerr_)); return 1; } } while (0)

enum { N = 2, C = 32, K = 48, H = 9, W = 8, R = 3, S = 3, PAD = 1, B = 16, HP = H + 2 * PAD, WP = W + 2 * PAD };

/* blocked tensors: activations [N][F/16][rows][columns][16], filter [K/16][C/16][R][S][16 c][16 k] */
static size_t act(int n, int f, int rows, int cols, int feats, int y, int x) { return ((((size_t)n * (feats / B) + f / B) * rows + y) * cols + x) * B + f % B; }
static size_t fil(int k, int c, int kj, int ki) { return (((((size_t)(k / B) * (C / B) + c / B) * R + kj) * S + ki) * B + c % B) * B + k % B; }

int main(void)
{
  libxsmm_dnn_conv_desc desc;
  libxsmm_dnn_layer* handle;
  libxsmm_dnn_tensor_datalayout* layout;
  libxsmm_dnn_tensor *t_in, *t_out, *t_w, *t_din, *t_dout, *t_dw;
  libxsmm_dnn_err_t status;
  float *in, *out, *w, *din, *dout, *dw;
  void* scratch;
  size_t n_in, n_out, n_w, i;
  unsigned int tasks = 0;
  int ofh, ofw, n, c, k, y, x, kj, ki, errors = 0;

  memset(&desc, 0, sizeof(desc));
  desc.N = N; desc.C = C; desc.H = H; desc.W = W; desc.K = K; desc.R = R; desc.S = S; desc.u = 1; desc.v = 1;
  desc.pad_h = PAD; desc.pad_w = PAD; desc.pad_h_in = PAD; desc.pad_w_in = PAD; desc.pad_h_out = 0; desc.pad_w_out = 0;
  desc.threads = 1;
  desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM; desc.filter_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM;
  desc.algo = LIBXSMM_DNN_CONV_ALGO_DIRECT; desc.options = LIBXSMM_DNN_CONV_OPTION_OVERWRITE; desc.fuse_ops = LIBXSMM_DNN_CONV_FUSE_NONE;
  handle = libxsmm_dnn_create_conv_layer(desc, &status);
  CHKERR(status);

  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_INPUT, &status); CHKERR(status);
  n_in = libxsmm_dnn_get_tensor_elements(layout, &status);
  if (5 != layout->num_dims || B != layout->dim_size[0] || WP != layout->dim_size[1] || HP != layout->dim_size[2]) { fprintf(stderr, "conv_caller: unexpected input layout\n"); return 1; }
  in = (float*)calloc(n_in, sizeof(float)); din = (float*)malloc(n_in * sizeof(float));
  t_in = libxsmm_dnn_link_tensor(layout, in, &status); CHKERR(status);
  t_din = libxsmm_dnn_link_tensor(layout, din, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_OUTPUT, &status); CHKERR(status);
  n_out = libxsmm_dnn_get_tensor_elements(layout, &status);
  ofw = (int)layout->dim_size[1]; ofh = (int)layout->dim_size[2];
  out = (float*)malloc(n_out * sizeof(float)); dout = (float*)malloc(n_out * sizeof(float));
  t_out = libxsmm_dnn_link_tensor(layout, out, &status); CHKERR(status);
  t_dout = libxsmm_dnn_link_tensor(layout, dout, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_FILTER, &status); CHKERR(status);
  n_w = libxsmm_dnn_get_tensor_elements(layout, &status);
  if (6 != layout->num_dims || (size_t)K * C * R * S != n_w) { fprintf(stderr, "conv_caller: unexpected filter layout\n"); return 1; }
  w = (float*)malloc(n_w * sizeof(float)); dw = (float*)malloc(n_w * sizeof(float));
  t_w = libxsmm_dnn_link_tensor(layout, w, &status); CHKERR(status);
  t_dw = libxsmm_dnn_link_tensor(layout, dw, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  if (H != ofh || W != ofw) { fprintf(stderr, "conv_caller: unexpected output extents\n"); return 1; }

  /* small integers; the physical rim of the input stays zero */
  for (n = 0; n < N; ++n) for (c = 0; c < C; ++c) for (y = 0; y < H; ++y) for (x = 0; x < W; ++x) {
    const unsigned int s = (unsigned int)(((n * C + c) * H + y) * W + x);
    in[act(n, c, HP, WP, C, y + PAD, x + PAD)] = (float)((int)(((s * 2654435761u) >> 7) % 7u) - 3);
  }
  for (i = 0; i < n_w; ++i) { w[i] = (float)((int)((((unsigned int)i * 40503u) >> 3) % 5u) - 2); dw[i] = -1.f; }
  for (i = 0; i < n_out; ++i) { dout[i] = (float)((int)((((unsigned int)i * 2246822519u) >> 9) % 7u) - 3); out[i] = -1.f; }
  for (i = 0; i < n_in; ++i) din[i] = -1.f;

  CHKERR(libxsmm_dnn_bind_tensor(handle, t_in, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_out, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_w, LIBXSMM_DNN_REGULAR_FILTER));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_din, LIBXSMM_DNN_GRADIENT_INPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_dout, LIBXSMM_DNN_GRADIENT_OUTPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_dw, LIBXSMM_DNN_GRADIENT_FILTER));
  scratch = malloc(libxsmm_dnn_get_scratch_size(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, &status)); CHKERR(status);
  CHKERR(libxsmm_dnn_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL, scratch));
  CHKERR(libxsmm_dnn_get_parallel_tasks(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, &tasks));
  if ((unsigned int)(N * (K / B)) != tasks) { fprintf(stderr, "conv_caller: unexpected task count\n"); return 1; }

  CHKERR(libxsmm_dnn_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0));
  CHKERR(libxsmm_dnn_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_BWD, 0, 0));
  CHKERR(libxsmm_dnn_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_UPD, 0, 0));

  /* naive loops */
  for (n = 0; n < N; ++n) for (k = 0; k < K; ++k) for (y = 0; y < ofh; ++y) for (x = 0; x < ofw; ++x) {
    float sum = 0.f;
    for (c = 0; c < C; ++c) for (kj = 0; kj < R; ++kj) for (ki = 0; ki < S; ++ki) sum += in[act(n, c, HP, WP, C, y + kj, x + ki)] * w[fil(k, c, kj, ki)];
    if (out[act(n, k, ofh, ofw, K, y, x)] != sum) ++errors;
  }
  for (n = 0; n < N; ++n) for (c = 0; c < C; ++c) for (y = 0; y < HP; ++y) for (x = 0; x < WP; ++x) {
    float sum = 0.f;
    if (y >= PAD && y < H + PAD && x >= PAD && x < W + PAD) { /* (the rim of dinput is zero) */
      for (k = 0; k < K; ++k) for (kj = 0; kj < R; ++kj) for (ki = 0; ki < S; ++ki) {
        if (y - kj < 0 || y - kj >= ofh || x - ki < 0 || x - ki >= ofw) continue;
        sum += dout[act(n, k, ofh, ofw, K, y - kj, x - ki)] * w[fil(k, c, kj, ki)];
      }
    }
    if (din[act(n, c, HP, WP, C, y, x)] != sum) ++errors;
  }
  for (k = 0; k < K; ++k) for (c = 0; c < C; ++c) for (kj = 0; kj < R; ++kj) for (ki = 0; ki < S; ++ki) {
    float sum = 0.f;
    for (n = 0; n < N; ++n) for (y = 0; y < ofh; ++y) for (x = 0; x < ofw; ++x) sum += dout[act(n, k, ofh, ofw, K, y, x)] * in[act(n, c, HP, WP, C, y + kj, x + ki)];
    if (dw[fil(k, c, kj, ki)] != sum) ++errors;
  }
  printf("conv_caller: N=%d C=%d K=%d %dx%d filter %dx%d pad %d -> %dx%d, %d mismatches\n", N, C, K, H, W, R, S, PAD, ofh, ofw, errors);

  CHKERR(libxsmm_dnn_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_ALL));
  CHKERR(libxsmm_dnn_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_destroy_tensor(t_in)); CHKERR(libxsmm_dnn_destroy_tensor(t_out)); CHKERR(libxsmm_dnn_destroy_tensor(t_w));
  CHKERR(libxsmm_dnn_destroy_tensor(t_din)); CHKERR(libxsmm_dnn_destroy_tensor(t_dout)); CHKERR(libxsmm_dnn_destroy_tensor(t_dw));
  CHKERR(libxsmm_dnn_destroy_conv_layer(handle));
  free(in); free(out); free(w); free(din); free(dout); free(dw); free(scratch);
  return 0 == errors ? 0 : 1;
}
