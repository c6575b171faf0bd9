/* pool_caller.c -- one max-pooling layer through the reference's DNN interface only (include/libxsmm_dnn_pooling.h as the
 * reference declares it): create, layouts, link and bind the tensors, bind the scratch, FWD, then BWD. The tensors live in plain
 * host memory, so every call is complete on return. The self-check is exact in fp32: max pooling copies values, and BWD sums
 * gradients that are small integers. Returns 0 if everything agrees with naive loops over the blocked tensors. */
#include <libxsmm_dnn_pooling.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <float.h>

#define CHKERR(call) do { const libxsmm_dnn_err_t chkerr_ = (call); if (LIBXSMM_DNN_SUCCESS != chkerr_) { \
  fprintf(stderr, "pool_caller: %s failed: %s\n", #call, libxsmm_dnn_get_error(chkerr_)); return 1; } } while (0)

int main(void)
{
  const int N = 3, C = 48, H = 13, W = 10, R = 3, S = 3, u = 2, v = 2, pad = 1, cb = 48 / 16;
  libxsmm_dnn_pooling_desc desc;
  libxsmm_dnn_pooling* handle;
  libxsmm_dnn_tensor_datalayout* layout;
  libxsmm_dnn_tensor *t_in, *t_out, *t_din, *t_dout, *t_mask;
  libxsmm_dnn_err_t status;
  float *in, *out, *din, *dout, *ref_out, *ref_din;
  int *mask, *ref_mask;
  void* scratch;
  size_t n_in, n_out, i;
  int ofh, ofw, item, ho, wo, kh, kw, c, errors = 0;

  memset(&desc, 0, sizeof(desc));
  desc.N = N; desc.C = C; desc.H = H; desc.W = W; desc.R = R; desc.S = S; desc.u = u; desc.v = v; desc.pad_h = pad; desc.pad_w = pad;
  desc.threads = 1;
  desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_mask = LIBXSMM_DNN_DATATYPE_I32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM;
  desc.pooling_type = LIBXSMM_DNN_POOLING_MAX;
  handle = libxsmm_dnn_create_pooling(desc, &status);
  CHKERR(status);

  layout = libxsmm_dnn_pooling_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_INPUT, &status); CHKERR(status);
  n_in = libxsmm_dnn_get_tensor_elements(layout, &status);
  in = (float*)malloc(n_in * sizeof(float)); din = (float*)malloc(n_in * sizeof(float)); ref_din = (float*)calloc(n_in, sizeof(float));
  t_in = libxsmm_dnn_link_tensor(layout, in, &status); CHKERR(status);
  t_din = libxsmm_dnn_link_tensor(layout, din, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_pooling_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_OUTPUT, &status); CHKERR(status);
  n_out = libxsmm_dnn_get_tensor_elements(layout, &status);
  ofw = (int)layout->dim_size[1]; ofh = (int)layout->dim_size[2];
  out = (float*)malloc(n_out * sizeof(float)); dout = (float*)malloc(n_out * sizeof(float)); ref_out = (float*)malloc(n_out * sizeof(float));
  t_out = libxsmm_dnn_link_tensor(layout, out, &status); CHKERR(status);
  t_dout = libxsmm_dnn_link_tensor(layout, dout, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_pooling_create_tensor_datalayout(handle, LIBXSMM_DNN_POOLING_MASK, &status); CHKERR(status);
  if (n_out != libxsmm_dnn_get_tensor_elements(layout, &status)) { fprintf(stderr, "pool_caller: unexpected mask layout\n"); return 1; }
  mask = (int*)malloc(n_out * sizeof(int)); ref_mask = (int*)malloc(n_out * sizeof(int));
  t_mask = libxsmm_dnn_link_tensor(layout, mask, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);

  /* values with many ties (first maximum wins) and gradients that are small integers */
  for (i = 0; i < n_in; ++i) { in[i] = (float)((int)((((unsigned int)i * 2654435761u) >> 7) % 23u) - 11); din[i] = -1.f; }
  for (i = 0; i < n_out; ++i) { dout[i] = (float)((int)((((unsigned int)i * 40503u) >> 3) % 7u) - 3); out[i] = -1.f; mask[i] = -1; }

  CHKERR(libxsmm_dnn_pooling_bind_tensor(handle, t_in, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_pooling_bind_tensor(handle, t_out, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_pooling_bind_tensor(handle, t_din, LIBXSMM_DNN_GRADIENT_INPUT));
  CHKERR(libxsmm_dnn_pooling_bind_tensor(handle, t_dout, LIBXSMM_DNN_GRADIENT_OUTPUT));
  CHKERR(libxsmm_dnn_pooling_bind_tensor(handle, t_mask, LIBXSMM_DNN_POOLING_MASK));
  scratch = malloc(libxsmm_dnn_pooling_get_scratch_size(handle, &status)); CHKERR(status);
  CHKERR(libxsmm_dnn_pooling_bind_scratch(handle, scratch));

  CHKERR(libxsmm_dnn_pooling_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0));
  CHKERR(libxsmm_dnn_pooling_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_BWD, 0, 0));

  /* naive loops over the blocked tensors [N][C/16][rows][columns][16] */
  for (item = 0; item < N * cb; ++item) {
    const float* const x = in + (size_t)item * H * W * 16;
    float* const dx = ref_din + (size_t)item * H * W * 16;
    for (ho = 0; ho < ofh; ++ho) for (wo = 0; wo < ofw; ++wo) for (c = 0; c < 16; ++c) {
      const size_t o = (((size_t)item * ofh + ho) * ofw + wo) * 16 + c;
      float best = -FLT_MAX; int at = -1;
      for (kh = 0; kh < R; ++kh) for (kw = 0; kw < S; ++kw) {
        const int hi = ho * u - pad + kh, wi = wo * v - pad + kw;
        if (hi < 0 || hi >= H || wi < 0 || wi >= W) continue;
        if (x[(hi * W + wi) * 16 + c] > best) { best = x[(hi * W + wi) * 16 + c]; at = (hi * W + wi) * 16 + c; }
      }
      ref_out[o] = best; ref_mask[o] = at;
      dx[at] += dout[o];
    }
  }
  for (i = 0; i < n_out; ++i) if (out[i] != ref_out[i] || mask[i] != ref_mask[i]) ++errors;
  for (i = 0; i < n_in; ++i) if (din[i] != ref_din[i]) ++errors;
  printf("pool_caller: N=%d C=%d %dx%d window %dx%d stride %d -> %dx%d, %d mismatches\n", N, C, H, W, R, S, u, ofh, ofw, errors);

  CHKERR(libxsmm_dnn_pooling_release_scratch(handle));
  CHKERR(libxsmm_dnn_pooling_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_destroy_tensor(t_in)); CHKERR(libxsmm_dnn_destroy_tensor(t_out)); CHKERR(libxsmm_dnn_destroy_tensor(t_din));
  CHKERR(libxsmm_dnn_destroy_tensor(t_dout)); CHKERR(libxsmm_dnn_destroy_tensor(t_mask));
  CHKERR(libxsmm_dnn_destroy_pooling(handle));
  free(in); free(out); free(din); free(dout); free(mask); free(ref_out); free(ref_din); free(ref_mask); free(scratch);
  return 0 == errors ? 0 : 1;
}
