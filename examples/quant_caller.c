/* quant_caller.c -- the producers in front of the low-precision GEMM, written against the reference API only
 * (the flow of samples/deeplearning/cnnlayer/layer_example_qi16f32.c:509-525): fp32 A and B are quantised to int16 with
 * libxsmm_dnn_quantize (FPHW rounding, add_shift 2), multiplied with libxsmm_wigemm, and a few quantised values are taken
 * back with libxsmm_dnn_dequantize; everything is checked against plain host loops.
 *   gcc -std=c99 -Wall -I include examples/quant_caller.c -L libxsmm-1_amd/lib -lxsmm -lm */
#include <libxsmm_dnn.h>
#include <libxsmm.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

/* what LIBXSMM_DNN_QUANT_FPHW_ROUND computes: one power-of-two scale for the tensor, halves away from zero */
static unsigned char host_quantize(const float* in, short* out, int n, int add_shift)
{
  float maxabs = 0;
  int i, e = 0;
  for (i = 0; i < n; ++i) if (fabsf(in[i]) > maxabs) maxabs = fabsf(in[i]);
  (void)frexpf(maxabs, &e);
  e -= 15 - add_shift;
  for (i = 0; i < n; ++i) out[i] = (short)roundf(ldexpf(in[i], -e));
  return (unsigned char)(-e);
}

int main(void)
{
  const libxsmm_blasint m = 200, n = 150, k = 75;
  const int ione = 1, izero = 0, ndeq = 16;
  float *a = (float*)malloc(sizeof(float) * m * k), *b = (float*)malloc(sizeof(float) * k * n), deq[16];
  short *qa = (short*)malloc(sizeof(short) * m * k), *qb = (short*)malloc(sizeof(short) * k * n);
  short *ga = (short*)malloc(sizeof(short) * m * k), *gb = (short*)malloc(sizeof(short) * k * n);
  int *c = (int*)malloc(sizeof(int) * m * n), *gold = (int*)malloc(sizeof(int) * m * n);
  unsigned char scf_a = 0, scf_b = 0, gscf_a, gscf_b;
  int i, j, p, result = EXIT_SUCCESS;
  if (NULL == a || NULL == b || NULL == qa || NULL == qb || NULL == ga || NULL == gb || NULL == c || NULL == gold) return EXIT_FAILURE;
  for (i = 0; i < m * k; ++i) a[i] = 0.37f - (float)((i * 7) % 113) / 150.0f;
  for (i = 0; i < k * n; ++i) b[i] = ((float)((i * 5) % 211) / 100.0f - 1.05f) * 3.0f;
  for (i = 0; i < m * n; ++i) c[i] = -7;
  gscf_a = host_quantize(a, ga, m * k, 2);
  gscf_b = host_quantize(b, gb, k * n, 2);
  for (j = 0; j < n; ++j) for (i = 0; i < m; ++i) {
    unsigned int sum = 0; /* beta = 0; the 32-bit sum wraps */
    for (p = 0; p < k; ++p) sum += (unsigned int)((int)ga[p * m + i] * (int)gb[j * k + p]);
    gold[j * m + i] = (int)sum;
  }

  libxsmm_init();
  libxsmm_dnn_quantize(a, qa, m * k, 2, &scf_a, LIBXSMM_DNN_QUANT_FPHW_ROUND);
  libxsmm_dnn_quantize(b, qb, k * n, 2, &scf_b, LIBXSMM_DNN_QUANT_FPHW_ROUND);
  libxsmm_wigemm("N", "N", &m, &n, &k, &ione, qa, &m, qb, &k, &izero, c, &m);
  libxsmm_dnn_dequantize(qa, deq, ndeq, scf_a);

  if (scf_a != gscf_a || scf_b != gscf_b) { fprintf(stderr, "quant_caller: scaling factors %d %d, expected %d %d\n", scf_a, scf_b, gscf_a, gscf_b); result = EXIT_FAILURE; }
  if (0 != memcmp(qa, ga, sizeof(short) * m * k) || 0 != memcmp(qb, gb, sizeof(short) * k * n)) { fprintf(stderr, "quant_caller: libxsmm_dnn_quantize differs\n"); result = EXIT_FAILURE; }
  if (0 != memcmp(c, gold, sizeof(int) * m * n)) { fprintf(stderr, "quant_caller: libxsmm_wigemm differs\n"); result = EXIT_FAILURE; }
  for (i = 0; i < ndeq; ++i) { /* the value a quantised element stands for: within half a quantum of the input */
    const float back = ldexpf((float)ga[i], -(int)gscf_a);
    if (deq[i] != back || fabsf(back - a[i]) > ldexpf(0.5f, -(int)gscf_a)) { fprintf(stderr, "quant_caller: libxsmm_dnn_dequantize differs at %d\n", i); result = EXIT_FAILURE; }
  }
  if (EXIT_SUCCESS == result) printf("quant_caller: ok (scf %d and %d, c[0] = %g)\n", scf_a, scf_b, ldexp((double)c[0], -(int)(scf_a + scf_b)));
  free(a); free(b); free(qa); free(qb); free(ga); free(gb); free(c); free(gold);
  libxsmm_finalize();
  return result;
}
