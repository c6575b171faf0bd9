/* tgemm_caller.c -- a caller of the reference's tiled GEMM interface (src/template/libxsmm.h:365-383), written against the
 * reference API only: libxsmm_gemm_handle_init, libxsmm_gemm_handle_get_scratch_size, a loop of libxsmm_gemm_thread over
 * the tasks (what an application's threads or tasks would run), and libxsmm_dgemm_omp for the same product in one call.
 * The operands live in plain host memory, as they do in a CPU application.
 *   gcc -std=c99 -Wall -I include examples/tgemm_caller.c -L libxsmm-1_amd/lib -lxsmm -lm */
#include <libxsmm.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

int main(void)
{
  const libxsmm_blasint m = 200, n = 150, k = 75, lda = 77 /* A is stored k x m: transa = 'T' */, ldb = 80, ldc = 203;
  const double alpha = 1, beta = 1;
  const int ntasks = 4;
  double *a = (double*)malloc(sizeof(double) * lda * m), *b = (double*)malloc(sizeof(double) * ldb * n);
  double *c = (double*)malloc(sizeof(double) * ldc * n), *c2 = (double*)malloc(sizeof(double) * ldc * n);
  double *gold = (double*)malloc(sizeof(double) * ldc * n);
  libxsmm_gemm_blob blob;
  const libxsmm_gemm_handle* handle;
  void* scratch = NULL;
  size_t scratch_size;
  double maxdiff = 0;
  int i, j, p, tid, result = EXIT_SUCCESS;
  if (NULL == a || NULL == b || NULL == c || NULL == c2 || NULL == gold) return EXIT_FAILURE;
  for (i = 0; i < lda * m; ++i) a[i] = 0.5 - (double)((i * 7) % 13) / 13.0;
  for (i = 0; i < ldb * n; ++i) b[i] = (double)((i * 5) % 11) / 11.0 - 0.5;
  for (i = 0; i < ldc * n; ++i) c[i] = c2[i] = gold[i] = (double)(i % 17) / 17.0;
  for (j = 0; j < n; ++j) for (i = 0; i < m; ++i) {
    double sum = gold[j * ldc + i];
    for (p = 0; p < k; ++p) sum += a[i * lda + p] * b[j * ldb + p];
    gold[j * ldc + i] = sum;
  }

  libxsmm_init();
  handle = libxsmm_gemm_handle_init(&blob, LIBXSMM_GEMM_PRECISION_F64, LIBXSMM_GEMM_PRECISION_F64, "T", "N",
    &m, &n, &k, &lda, &ldb, &ldc, &alpha, &beta, LIBXSMM_GEMM_HANDLE_FLAG_AUTO, ntasks);
  if (NULL == handle) { fprintf(stderr, "tgemm_caller: no handle\n"); return EXIT_FAILURE; }
  scratch_size = libxsmm_gemm_handle_get_scratch_size(handle);
  if (0 < scratch_size) scratch = malloc(scratch_size * ntasks);
  for (tid = 0; tid < ntasks; ++tid) { /* (an application runs this body on its own threads) */
    libxsmm_gemm_thread(handle, NULL != scratch ? ((char*)scratch + scratch_size * tid) : NULL, a, b, c, tid, ntasks);
  }
  libxsmm_dgemm_omp("T", "N", &m, &n, &k, &alpha, a, &lda, b, &ldb, &beta, c2, &ldc);

  for (j = 0; j < n; ++j) for (i = 0; i < ldc; ++i) {
    const double d = fabs(c[j * ldc + i] - gold[j * ldc + i]);
    if (d > maxdiff) maxdiff = d;
  }
  if (maxdiff > 1E-12 * k) { fprintf(stderr, "tgemm_caller: difference %g\n", maxdiff); result = EXIT_FAILURE; }
  if (0 != memcmp(c, c2, sizeof(double) * ldc * n)) { fprintf(stderr, "tgemm_caller: the task loop and libxsmm_dgemm_omp differ\n"); result = EXIT_FAILURE; }
  if (EXIT_SUCCESS == result) printf("tgemm_caller: ok (max difference %g, scratch %lu bytes)\n", maxdiff, (unsigned long)scratch_size);
  free(scratch); free(a); free(b); free(c); free(c2); free(gold);
  libxsmm_finalize();
  return result;
}
