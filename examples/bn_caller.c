/* bn_caller.c -- one fused batch-norm layer (BN + RELU) through the reference's DNN interface only
 * (include/libxsmm_dnn_fusedbatchnorm.h as the reference declares it): create, layouts, link and bind the tensors, bind the
 * scratch, FWD, then BWD. The tensors live in plain host memory, so every call is complete on return. The self-check recomputes
 * mean, rstd, the output, dgamma, dbeta and dinput with naive double-precision loops over the blocked tensors and allows a
 * relative error of 1e-4 (the layer sums in fp32). Returns 0 if everything agrees. */
#include <libxsmm_dnn_fusedbatchnorm.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#define CHKERR(call) do { const libxsmm_dnn_err_t chkerr_ = (call); if (LIBXSMM_DNN_SUCCESS != chkerr_) { \
  fprintf(stderr, "bn_caller: %s failed: %s\n", #call, libxsmm_dnn_get_error(chkerr_)); return 1; } } while (0)

static int differs(double got, double want) { return !(fabs(got - want) <= 1e-4 * (fabs(want) + 1.0)); }

int main(void)
{
  const int N = 3, C = 48, H = 6, W = 10, cb = 48 / 16, npix = 6 * 10;
  libxsmm_dnn_fusedbatchnorm_desc desc;
  libxsmm_dnn_fusedbatchnorm* handle;
  libxsmm_dnn_tensor_datalayout* layout;
  libxsmm_dnn_tensor *t_in, *t_out, *t_din, *t_dout, *t_gamma, *t_beta, *t_dgamma, *t_dbeta, *t_mean, *t_rstd, *t_var;
  libxsmm_dnn_err_t status;
  float *in, *out, *din, *dout, *dout0, *chan;
  void* scratch;
  size_t n_act, n_chan, i;
  int img, fm, p, c, errors = 0;

  memset(&desc, 0, sizeof(desc));
  desc.N = N; desc.C = C; desc.H = H; desc.W = W; desc.u = 1; desc.v = 1;
  desc.threads = 1;
  desc.datatype_in = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_out = LIBXSMM_DNN_DATATYPE_F32; desc.datatype_stats = LIBXSMM_DNN_DATATYPE_F32;
  desc.buffer_format = LIBXSMM_DNN_TENSOR_FORMAT_LIBXSMM;
  desc.fuse_order = LIBXSMM_DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU;
  desc.fuse_ops = LIBXSMM_DNN_FUSEDBN_OPS_BN_RELU;
  handle = libxsmm_dnn_create_fusedbatchnorm(desc, &status);
  CHKERR(status);

  /* without padding and stride the four activation tensors share one layout, and the seven channel tensors another */
  layout = libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_INPUT, &status); CHKERR(status);
  n_act = libxsmm_dnn_get_tensor_elements(layout, &status);
  if (n_act != (size_t)N * C * npix) { fprintf(stderr, "bn_caller: unexpected activation layout\n"); return 1; }
  in = (float*)malloc(n_act * sizeof(float)); din = (float*)malloc(n_act * sizeof(float));
  out = (float*)malloc(n_act * sizeof(float)); dout = (float*)malloc(n_act * sizeof(float)); dout0 = (float*)malloc(n_act * sizeof(float));
  t_in = libxsmm_dnn_link_tensor(layout, in, &status); CHKERR(status);
  t_din = libxsmm_dnn_link_tensor(layout, din, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, LIBXSMM_DNN_REGULAR_OUTPUT, &status); CHKERR(status);
  if (n_act != libxsmm_dnn_get_tensor_elements(layout, &status)) { fprintf(stderr, "bn_caller: unexpected output layout\n"); return 1; }
  t_out = libxsmm_dnn_link_tensor(layout, out, &status); CHKERR(status);
  t_dout = libxsmm_dnn_link_tensor(layout, dout, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);
  layout = libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, LIBXSMM_DNN_CHANNEL_EXPECTVAL, &status); CHKERR(status);
  n_chan = libxsmm_dnn_get_tensor_elements(layout, &status);
  if (n_chan != (size_t)C) { fprintf(stderr, "bn_caller: unexpected channel layout\n"); return 1; }
  chan = (float*)malloc(7 * n_chan * sizeof(float)); /* gamma, beta, dgamma, dbeta, mean, rstd, var */
  t_gamma = libxsmm_dnn_link_tensor(layout, chan, &status); CHKERR(status);
  t_beta = libxsmm_dnn_link_tensor(layout, chan + n_chan, &status); CHKERR(status);
  t_dgamma = libxsmm_dnn_link_tensor(layout, chan + 2 * n_chan, &status); CHKERR(status);
  t_dbeta = libxsmm_dnn_link_tensor(layout, chan + 3 * n_chan, &status); CHKERR(status);
  t_mean = libxsmm_dnn_link_tensor(layout, chan + 4 * n_chan, &status); CHKERR(status);
  t_rstd = libxsmm_dnn_link_tensor(layout, chan + 5 * n_chan, &status); CHKERR(status);
  t_var = libxsmm_dnn_link_tensor(layout, chan + 6 * n_chan, &status); CHKERR(status);
  libxsmm_dnn_destroy_tensor_datalayout(layout);

  for (i = 0; i < n_act; ++i) {
    in[i] = (float)((int)((((unsigned int)i * 2654435761u) >> 7) % 201u) - 90) * 0.03125f;
    dout[i] = dout0[i] = (float)((int)((((unsigned int)i * 40503u) >> 3) % 17u) - 8) * 0.125f;
    out[i] = din[i] = -1.f;
  }
  for (i = 0; i < n_chan; ++i) { chan[i] = 0.5f + (float)(i % 5) * 0.25f; chan[n_chan + i] = (float)((int)(i % 7) - 3) * 0.125f; }
  for (i = 2 * n_chan; i < 7 * n_chan; ++i) chan[i] = -1.f;

  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_in, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_out, LIBXSMM_DNN_REGULAR_OUTPUT));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_din, LIBXSMM_DNN_GRADIENT_INPUT));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_dout, LIBXSMM_DNN_GRADIENT_OUTPUT));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_gamma, LIBXSMM_DNN_REGULAR_CHANNEL_GAMMA));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_beta, LIBXSMM_DNN_REGULAR_CHANNEL_BETA));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_dgamma, LIBXSMM_DNN_GRADIENT_CHANNEL_GAMMA));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_dbeta, LIBXSMM_DNN_GRADIENT_CHANNEL_BETA));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_mean, LIBXSMM_DNN_CHANNEL_EXPECTVAL));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_rstd, LIBXSMM_DNN_CHANNEL_RCPSTDDEV));
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t_var, LIBXSMM_DNN_CHANNEL_VARIANCE));
  scratch = malloc(libxsmm_dnn_fusedbatchnorm_get_scratch_size(handle, &status)); CHKERR(status);
  CHKERR(libxsmm_dnn_fusedbatchnorm_bind_scratch(handle, scratch));

  CHKERR(libxsmm_dnn_fusedbatchnorm_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_FWD, 0, 0));
  CHKERR(libxsmm_dnn_fusedbatchnorm_execute_st(handle, LIBXSMM_DNN_COMPUTE_KIND_BWD, 0, 0));

  /* naive loops over the blocked tensors [N][C/16][H*W][16], one channel at a time */
  for (fm = 0; fm < cb; ++fm) for (c = 0; c < 16; ++c) {
    const int ch = fm * 16 + c;
    const double nhw = (double)N * npix, gamma = chan[ch], beta = chan[n_chan + ch];
    double sum = 0, sumsq = 0, mean, var, rstd, dgamma = 0, dbeta = 0;
    for (img = 0; img < N; ++img) for (p = 0; p < npix; ++p) {
      const double x = in[(((size_t)img * cb + fm) * npix + p) * 16 + c];
      sum += x; sumsq += x * x;
    }
    mean = sum / nhw; var = sumsq / nhw - mean * mean; rstd = 1.0 / sqrt(var + 1e-7);
    if (differs(chan[4 * n_chan + ch], mean) || differs(chan[5 * n_chan + ch], rstd) || differs(chan[6 * n_chan + ch], var)) ++errors;
    for (img = 0; img < N; ++img) for (p = 0; p < npix; ++p) {
      const size_t at = (((size_t)img * cb + fm) * npix + p) * 16 + c;
      double o = gamma * (in[at] - mean) * rstd + beta, d;
      if (o < 0) o = 0;
      /* (an output within rounding of zero may be zero on one side only: the check follows what the layer stored) */
      if (differs(out[at], o)) ++errors;
      d = (0 == out[at]) ? 0 : dout0[at];
      if (dout[at] != (float)d) ++errors;  /* BWD with RELU writes the masked gradient back */
      dgamma += (in[at] - mean) * d * rstd; dbeta += d;
    }
    if (differs(chan[2 * n_chan + ch], dgamma) || differs(chan[3 * n_chan + ch], dbeta)) ++errors;
    for (img = 0; img < N; ++img) for (p = 0; p < npix; ++p) {
      const size_t at = (((size_t)img * cb + fm) * npix + p) * 16 + c;
      const double want = gamma * rstd / nhw * (nhw * dout[at] - (dbeta + (in[at] - mean) * dgamma * rstd));
      if (differs(din[at], want)) ++errors;
    }
  }
  printf("bn_caller: N=%d C=%d %dx%d BN+RELU fwd and bwd, %d mismatches\n", N, C, H, W, errors);

  CHKERR(libxsmm_dnn_fusedbatchnorm_release_scratch(handle));
  CHKERR(libxsmm_dnn_fusedbatchnorm_release_tensor(handle, LIBXSMM_DNN_REGULAR_INPUT));
  CHKERR(libxsmm_dnn_destroy_tensor(t_in)); CHKERR(libxsmm_dnn_destroy_tensor(t_out)); CHKERR(libxsmm_dnn_destroy_tensor(t_din));
  CHKERR(libxsmm_dnn_destroy_tensor(t_dout)); CHKERR(libxsmm_dnn_destroy_tensor(t_gamma)); CHKERR(libxsmm_dnn_destroy_tensor(t_beta));
  CHKERR(libxsmm_dnn_destroy_tensor(t_dgamma)); CHKERR(libxsmm_dnn_destroy_tensor(t_dbeta)); CHKERR(libxsmm_dnn_destroy_tensor(t_mean));
  CHKERR(libxsmm_dnn_destroy_tensor(t_rstd)); CHKERR(libxsmm_dnn_destroy_tensor(t_var));
  CHKERR(libxsmm_dnn_destroy_fusedbatchnorm(handle));
  free(in); free(out); free(din); free(dout); free(dout0); free(chan); free(scratch);
  return 0 == errors ? 0 : 1;
}
