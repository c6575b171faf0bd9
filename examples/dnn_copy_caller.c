/* dnn_copy_caller.c -- how a framework hands plain tensors to a layer through the reference's DNN interface only
 * (include/libxsmm_dnn.h as the reference declares it): link blocked tensors on a convolution handle, copy-in of the input
 * (NCHW), the filter (KCRS) and the bias (a channel tensor: NCHW is the reference's rule), a FWD pass with the bias fused, and
 * copy-out of the output to NCHW. The input is physically padded, so its plain image has the padded extents with a zero rim.
 * All values are small integers, so every sum is exact whatever its order: the result must equal a plain-C convolution over
 * the plain buffers. The tensors live in host memory here; a caller with device buffers makes the same calls. Returns 0. */
#include <libxsmm_dnn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHKERR(call) do { const libxsmm_dnn_err_t chkerr_ = (call); if (LIBXSMM_DNN_SUCCESS != chkerr_) { \
  fprintf(stderr, "dnn_copy_caller: %s failed: %s\n", #call, libxsmm_dnn_get_error(chkerr_)); return 1; } } while (0)

enum { N = 2, C = 24, K = 40, H = 5, W = 7, R = 3, S = 3, PAD = 1, HP = H + 2 * PAD, WP = W + 2 * PAD };

int main(void)
{
  libxsmm_dnn_conv_desc desc;
  libxsmm_dnn_layer* handle;
  libxsmm_dnn_tensor_datalayout* layout;
  libxsmm_dnn_tensor *t_in, *t_out, *t_w, *t_bias;
  libxsmm_dnn_err_t status;
  float *in, *out, *w, *bias;                   /* blocked, as the layer wants them */
  float *pin, *pout, *pw, *pbias, *back;        /* plain: [N][C][HP][WP], [N][K][H][W], [K][C][R][S], [K] */
  void* scratch;
  size_t n_in, n_out, n_w, n_bias, i;
  int n, c, k, y, x, kj, ki, errors = 0;

  memset(&desc, 0, sizeof(desc));
  desc.N = N; desc.C = C; desc.H = H; desc.W = W; desc.K = K; desc.R = R; desc.S = S; desc.u = 1; desc.v = 1;
  desc.pad_h = PAD; desc.pad_w = PAD; desc.pad_h_in = PAD; desc.pad_w_in = PAD; desc.pad_h_out = 0; desc.pad_w_out = 0;
  desc.threads = 1;
  desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM; desc.filter_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM;
  desc.algo = LIBXSMM_DNN_CONV_ALGO_DIRECT; desc.options = LIBXSMM_DNN_CONV_OPTION_OVERWRITE; desc.fuse_ops = LIBXSMM_DNN_CONV_FUSE_BIAS;
  handle = libxsmm_dnn_create_conv_layer(desc, &status);
  CHKERR(status);

  /* 1. link tensors on the handle */
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_INPUT, &status); CHKERR(status);
  n_in = libxsmm_dnn_get_tensor_elements(layout, &status);
  in = (float*)malloc(n_in * sizeof(float));
  t_in = libxsmm_dnn_link_tensor(layout, in, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_OUTPUT, &status); CHKERR(status);
  n_out = libxsmm_dnn_get_tensor_elements(layout, &status);
  out = (float*)malloc(n_out * sizeof(float));
  t_out = libxsmm_dnn_link_tensor(layout, out, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_FILTER, &status); CHKERR(status);
  n_w = libxsmm_dnn_get_tensor_elements(layout, &status);
  w = (float*)malloc(n_w * sizeof(float));
  t_w = libxsmm_dnn_link_tensor(layout, w, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_CHANNEL_BIAS, &status); CHKERR(status);
  n_bias = libxsmm_dnn_get_tensor_elements(layout, &status);
  bias = (float*)malloc(n_bias * sizeof(float));
  t_bias = libxsmm_dnn_link_tensor(layout, bias, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  if ((size_t)N * C * HP * WP != n_in || (size_t)N * K * H * W != n_out || (size_t)K * C * R * S != n_w || (size_t)K != n_bias) {
    fprintf(stderr, "dnn_copy_caller: unexpected layouts\n"); return 1;
  }

  /* the plain side: small integers; the rim of the input is zero */
  pin = (float*)calloc(n_in, sizeof(float)); pout = (float*)malloc(n_out * sizeof(float)); back = (float*)malloc(n_w * sizeof(float));
  pw = (float*)malloc(n_w * sizeof(float)); pbias = (float*)malloc(n_bias * sizeof(float));
  for (n = 0; n < N; ++n) for (c = 0; c < C; ++c) for (y = 0; y < H; ++y) for (x = 0; x < W; ++x) {
    const unsigned int s = (unsigned int)(((n * C + c) * H + y) * W + x);
    pin[(((size_t)n * C + c) * HP + y + PAD) * WP + x + PAD] = (float)((int)(((s * 2654435761u) >> 7) % 7u) - 3);
  }
  for (i = 0; i < n_w; ++i) pw[i] = (float)((int)((((unsigned int)i * 40503u) >> 3) % 5u) - 2);
  for (i = 0; i < n_bias; ++i) pbias[i] = (float)((int)(i % 9u) - 4);
  for (i = 0; i < n_out; ++i) { out[i] = -1.f; pout[i] = -2.f; }
  for (i = 0; i < n_in; ++i) in[i] = -1.f;
  for (i = 0; i < n_w; ++i) { w[i] = -1.f; back[i] = -2.f; }

  /* 2. copy-in from the plain formats */
  CHKERR(libxsmm_dnn_copyin_tensor(t_in, pin, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
  CHKERR(libxsmm_dnn_copyin_tensor(t_w, pw, LIBXSMM_DNN_TENSOR_FORMAT_KCRS));
  CHKERR(libxsmm_dnn_copyin_tensor(t_bias, pbias, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));

  /* 3. FWD */
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_in, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_out, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_w, LIBXSMM_DNN_REGULAR_FILTER));
  CHKERR(libxsmm_dnn_bind_tensor(handle, t_bias, LIBXSMM_DNN_REGULAR_CHANNEL_BIAS));
  scratch = malloc(libxsmm_dnn_get_scratch_size(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, &status)); CHKERR(status);
  CHKERR(libxsmm_dnn_bind_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, scratch));
  CHKERR(libxsmm_dnn_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0));

  /* 4. copy-out (the filter too: it must come back as it went in) */
  CHKERR(libxsmm_dnn_copyout_tensor(t_out, pout, LIBXSMM_DNN_TENSOR_FORMAT_NCHW));
  CHKERR(libxsmm_dnn_copyout_tensor(t_w, back, LIBXSMM_DNN_TENSOR_FORMAT_KCRS));

  /* 5. a plain convolution over the plain buffers */
  for (n = 0; n < N; ++n) for (k = 0; k < K; ++k) for (y = 0; y < H; ++y) for (x = 0; x < W; ++x) {
    float sum = pbias[k];
    for (c = 0; c < C; ++c) for (kj = 0; kj < R; ++kj) for (ki = 0; ki < S; ++ki) {
      sum += pin[(((size_t)n * C + c) * HP + y + kj) * WP + x + ki] * pw[(((size_t)k * C + c) * R + kj) * S + ki];
    }
    if (pout[(((size_t)n * K + k) * H + y) * W + x] != sum) ++errors;
  }
  for (i = 0; i < n_w; ++i) if (back[i] != pw[i]) ++errors;
  printf("dnn_copy_caller: N=%d C=%d K=%d %dx%d filter %dx%d pad %d, %d mismatches\n", N, C, K, H, W, R, S, PAD, errors);

  CHKERR(libxsmm_dnn_release_scratch(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD));
  CHKERR(libxsmm_dnn_destroy_tensor(t_in)); CHKERR(libxsmm_dnn_destroy_tensor(t_out)); CHKERR(libxsmm_dnn_destroy_tensor(t_w));
  CHKERR(libxsmm_dnn_destroy_tensor(t_bias));
  CHKERR(libxsmm_dnn_destroy_conv_layer(handle));
  free(in); free(out); free(w); free(bias); free(pin); free(pout); free(pw); free(pbias); free(back); free(scratch);
  return 0 == errors ? 0 : 1;
}
