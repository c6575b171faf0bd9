/* lowp_gemm_caller.c -- a caller of the reference's GEMM front ends for 16-bit inputs (src/template/libxsmm.h:397-414),
 * written against the reference API only: libxsmm_bsgemm on a product beyond LIBXSMM_MAX_MNK and libxsmm_wigemm on a
 * transposed one, both on plain column-major operands in host memory, checked against plain loops.
 *   gcc -std=c99 -Wall -I include examples/lowp_gemm_caller.c -L libxsmm-1_amd/lib -lxsmm -lm */
#include <libxsmm.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

static float bf16_value(libxsmm_bfloat16 v) { libxsmm_bfloat16_hp hp; hp.i[0] = 0; hp.i[1] = v; return hp.f; }
static libxsmm_bfloat16 bf16_of(float f) { libxsmm_bfloat16_hp hp; hp.f = f; return hp.i[1]; }

int main(void)
{
  const libxsmm_blasint m = 200, n = 150, k = 75, lda = 203, ldb = 80, ldc = 201;
  const libxsmm_blasint ldat = 77; /* libxsmm_wigemm: A is stored k x m, transa = 'T' */
  const float one = 1, zero = 0;
  const int ione = 1;
  libxsmm_bfloat16 *a = (libxsmm_bfloat16*)malloc(sizeof(libxsmm_bfloat16) * lda * k), *b = (libxsmm_bfloat16*)malloc(sizeof(libxsmm_bfloat16) * ldb * n);
  short *ia = (short*)malloc(sizeof(short) * ldat * m), *ib = (short*)malloc(sizeof(short) * ldb * n);
  float *c = (float*)malloc(sizeof(float) * ldc * n), *gold = (float*)malloc(sizeof(float) * ldc * n);
  int *ic = (int*)malloc(sizeof(int) * ldc * n), *igold = (int*)malloc(sizeof(int) * ldc * n);
  double maxdiff = 0;
  int i, j, p, result = EXIT_SUCCESS;
  if (NULL == a || NULL == b || NULL == ia || NULL == ib || NULL == c || NULL == gold || NULL == ic || NULL == igold) return EXIT_FAILURE;
  for (i = 0; i < lda * k; ++i) a[i] = bf16_of(0.5f - (float)((i * 7) % 13) / 13.0f);
  for (i = 0; i < ldb * n; ++i) b[i] = bf16_of((float)((i * 5) % 11) / 11.0f - 0.5f);
  for (i = 0; i < ldat * m; ++i) ia[i] = (short)((i * 37) % 2001 - 1000);
  for (i = 0; i < ldb * n; ++i) ib[i] = (short)((i * 53) % 1801 - 900);
  for (i = 0; i < ldc * n; ++i) { c[i] = gold[i] = -7.f; ic[i] = igold[i] = i % 17; }
  for (j = 0; j < n; ++j) for (i = 0; i < m; ++i) {
    float sum = 0; /* beta = 0 */
    int isum = igold[j * ldc + i]; /* beta = 1 */
    for (p = 0; p < k; ++p) {
      sum += bf16_value(a[p * lda + i]) * bf16_value(b[j * ldb + p]);
      isum += (int)ia[i * ldat + p] * (int)ib[j * ldb + p];
    }
    gold[j * ldc + i] = sum; igold[j * ldc + i] = isum;
  }

  libxsmm_init();
  libxsmm_bsgemm("N", "N", &m, &n, &k, &one, a, &lda, b, &ldb, &zero, c, &ldc);
  libxsmm_wigemm("T", "N", &m, &n, &k, &ione, ia, &ldat, ib, &ldb, &ione, ic, &ldc);

  for (j = 0; j < n; ++j) for (i = 0; i < ldc; ++i) { /* (the padding between m and ldc included: it keeps its values) */
    const double d = fabs((double)c[j * ldc + i] - (double)gold[j * ldc + i]);
    if (d > maxdiff) maxdiff = d;
  }
  if (maxdiff > 1E-5 * k) { fprintf(stderr, "lowp_gemm_caller: libxsmm_bsgemm differs by %g\n", maxdiff); result = EXIT_FAILURE; }
  if (0 != memcmp(ic, igold, sizeof(int) * ldc * n)) { fprintf(stderr, "lowp_gemm_caller: libxsmm_wigemm differs\n"); result = EXIT_FAILURE; }
  if (EXIT_SUCCESS == result) printf("lowp_gemm_caller: ok (max difference %g)\n", maxdiff);
  free(a); free(b); free(ia); free(ib); free(c); free(gold); free(ic); free(igold);
  libxsmm_finalize();
  return result;
}
