/* The per-shape loop of the reference's samples/cp2k/cp2k.cpp (:328-360) on device memory: one libxsmm_gemm_batch call
 * (index arrays) per shape (M, N, K) in {13, 23, 32}^3, every u consecutive products of a shape accumulating into one C
 * block. Run twice: as it stands -- a launch per shape -- and with the two lines libxsmm_amd_defer_begin() /
 * libxsmm_amd_defer_end() around the loop, which let the 27 calls leave as one fused launch. The index arrays live in one
 * host buffer that the loop refills for every shape, as a caller with stack buffers does: a recorded call has copied its
 * arrays when it returns. The two runs must agree bit for bit, and with a plain loop on the host within rounding.
 * Build: gcc -I include examples/cp2k_bracket_caller.c -L libxsmm-1_amd/lib -lxsmm -Wl,-rpath,$PWD/libxsmm-1_amd/lib -lm */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NSHAPES 27
#define PRODUCTS 1200 /* per shape */
#define RUN 20       /* consecutive products per C block */

static const int sizes[3] = { 13, 23, 32 };

typedef struct shape_t {
  int m, n, k;
  double *a, *b, *c;    /* device */
  double *ha, *hb, *hc; /* host images (hc: the initial C) */
} shape_t;

static void fill(double* x, size_t n, unsigned seed)
{
  size_t i;
  for (i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; x[i] = (double)(seed >> 8) / (double)(1u << 24) - 0.5; }
}

/* the caller's loop: one call per shape, the index arrays in buffers that are reused from shape to shape */
static void per_shape_loop(const shape_t* sh, libxsmm_blasint* ia, libxsmm_blasint* ib, libxsmm_blasint* ic)
{
  const double alpha = 1, beta = 1;
  int g, i;
  for (g = 0; g < NSHAPES; ++g) {
    const int m = sh[g].m, n = sh[g].n, k = sh[g].k;
    for (i = 0; i < PRODUCTS; ++i) {
      ia[i] = (libxsmm_blasint)((PRODUCTS - 1 - i) * m * k); ib[i] = (libxsmm_blasint)(i * k * n); ic[i] = (libxsmm_blasint)((i / RUN) * m * n);
    }
    libxsmm_gemm_batch(LIBXSMM_GEMM_PRECISION_F64, LIBXSMM_GEMM_PRECISION_F64, "N", "N", m, n, k, &alpha, sh[g].a, NULL, sh[g].b, NULL,
      &beta, sh[g].c, NULL, 0, (libxsmm_blasint)sizeof(libxsmm_blasint), ia, ib, ic, PRODUCTS);
  }
}

int main(void)
{
  shape_t sh[NSHAPES];
  libxsmm_blasint ia[PRODUCTS], ib[PRODUCTS], ic[PRODUCTS];
  const int nc = (PRODUCTS + RUN - 1) / RUN;
  int g, i, result = 0;
  unsigned long long launches_plain, launches_bracket;
  double worst = 0;
  libxsmm_init();
  if (1 > libxsmm_amd_device_count()) { fprintf(stderr, "cp2k_bracket_caller: no device\n"); return 1; }
  memset(sh, 0, sizeof(sh));
  for (g = 0; g < NSHAPES; ++g) {
    const int m = sizes[g / 9], n = sizes[(g / 3) % 3], k = sizes[g % 3];
    const size_t na = (size_t)PRODUCTS * m * k, nb = (size_t)PRODUCTS * k * n, ncc = (size_t)nc * m * n;
    sh[g].m = m; sh[g].n = n; sh[g].k = k;
    sh[g].ha = (double*)malloc(sizeof(double) * na); sh[g].hb = (double*)malloc(sizeof(double) * nb); sh[g].hc = (double*)malloc(sizeof(double) * ncc);
    sh[g].a = (double*)libxsmm_amd_device_malloc(sizeof(double) * na); sh[g].b = (double*)libxsmm_amd_device_malloc(sizeof(double) * nb);
    sh[g].c = (double*)libxsmm_amd_device_malloc(sizeof(double) * ncc);
    if (NULL == sh[g].ha || NULL == sh[g].hb || NULL == sh[g].hc || NULL == sh[g].a || NULL == sh[g].b || NULL == sh[g].c) return 100;
    fill(sh[g].ha, na, 3u * g + 1); fill(sh[g].hb, nb, 3u * g + 2); fill(sh[g].hc, ncc, 3u * g + 3);
    result |= libxsmm_amd_memcpy_h2d(sh[g].a, sh[g].ha, sizeof(double) * na) | libxsmm_amd_memcpy_h2d(sh[g].b, sh[g].hb, sizeof(double) * nb);
    result |= libxsmm_amd_memcpy_h2d(sh[g].c, sh[g].hc, sizeof(double) * ncc);
  }
  if (0 != result) { fprintf(stderr, "cp2k_bracket_caller: copies to the device failed\n"); return 101; }

  /* the loop as it stands */
  per_shape_loop(sh, ia, ib, ic); /* (warm-up: kernels are specialised on first use) */
  launches_plain = libxsmm_amd_launch_count();
  per_shape_loop(sh, ia, ib, ic);
  launches_plain = libxsmm_amd_launch_count() - launches_plain;
  libxsmm_amd_synchronize();
  /* keep the result (two passes over the initial C) and start over */
  {
    double* plain[NSHAPES];
    for (g = 0; g < NSHAPES; ++g) {
      const size_t bytes = sizeof(double) * nc * sh[g].m * sh[g].n;
      plain[g] = (double*)malloc(bytes);
      if (NULL == plain[g] || 0 != libxsmm_amd_memcpy_d2h(plain[g], sh[g].c, bytes) || 0 != libxsmm_amd_memcpy_h2d(sh[g].c, sh[g].hc, bytes)) return 102;
    }

    /* the same loop inside the bracket: the calls are recorded and leave together */
    libxsmm_amd_defer_begin();
    per_shape_loop(sh, ia, ib, ic);
    libxsmm_amd_defer_end();
    libxsmm_amd_jit_wait(); /* (the fused kernel of the 27 shapes, unless the code-object cache held it, is built on a helper thread) */
    launches_bracket = libxsmm_amd_launch_count();
    libxsmm_amd_defer_begin();
    per_shape_loop(sh, ia, ib, ic);
    libxsmm_amd_defer_end();
    launches_bracket = libxsmm_amd_launch_count() - launches_bracket;
    libxsmm_amd_synchronize();

    for (g = 0; g < NSHAPES; ++g) {
      const int m = sh[g].m, n = sh[g].n, k = sh[g].k;
      const size_t ncc = (size_t)nc * m * n;
      double* const got = (double*)malloc(sizeof(double) * ncc);
      double* const gold = (double*)malloc(sizeof(double) * ncc);
      int pass, j, p, r;
      if (NULL == got || NULL == gold || 0 != libxsmm_amd_memcpy_d2h(got, sh[g].c, sizeof(double) * ncc)) return 103;
      if (0 != memcmp(got, plain[g], sizeof(double) * ncc)) { fprintf(stderr, "%dx%dx%d: bracketed and plain loop differ\n", m, n, k); result |= 2; }
      memcpy(gold, sh[g].hc, sizeof(double) * ncc);
      for (pass = 0; pass < 2; ++pass) for (i = 0; i < PRODUCTS; ++i) {
        const double* const pa = sh[g].ha + (size_t)(PRODUCTS - 1 - i) * m * k; const double* const pb = sh[g].hb + (size_t)i * k * n;
        double* const pc = gold + (size_t)(i / RUN) * m * n;
        for (j = 0; j < n; ++j) for (p = 0; p < k; ++p) for (r = 0; r < m; ++r) pc[j * m + r] += pa[p * m + r] * pb[j * k + p];
      }
      for (j = 0; j < (int)ncc; ++j) { const double d = fabs(got[j] - gold[j]); if (d > worst) worst = d; }
      free(got); free(gold); free(plain[g]);
    }
  }
  if (!(worst <= 1e-11)) { fprintf(stderr, "difference to the plain loop on the host: %g\n", worst); result |= 4; }
  if (launches_bracket >= launches_plain) { fprintf(stderr, "bracket: %llu launches, plain loop: %llu\n", launches_bracket, launches_plain); result |= 8; }
  for (g = 0; g < NSHAPES; ++g) {
    libxsmm_amd_device_free(sh[g].a); libxsmm_amd_device_free(sh[g].b); libxsmm_amd_device_free(sh[g].c);
    free(sh[g].ha); free(sh[g].hb); free(sh[g].hc);
  }
  libxsmm_finalize();
  if (0 == result) {
    printf("cp2k_bracket_caller: 27 shapes, %llu launches per pass in the plain loop, %llu inside the bracket, the same bits (last kernel %s)\n",
      launches_plain, launches_bracket, libxsmm_amd_last_kernel());
  }
  return result;
}
