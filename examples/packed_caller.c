/* A caller of the packed ("compact") kernels written against the reference API: descriptor init, dispatch, a loop of kernel
 * calls over the packs, for pgemm, getrf, trmm and trsm in fp64 (the flow of the reference's samples/packed drivers). The
 * operands are plain malloc memory, as in a CPU program: every call is complete when it returns. Each result is checked
 * with a residual the caller computes itself. The last part repeats the trsm loop on device memory between
 * libxsmm_amd_defer_begin() / libxsmm_amd_defer_end() -- the two lines that turn the loop into one launch -- and expects
 * the same bits.
 * Build: gcc -I include examples/packed_caller.c -L libxsmm-1_amd/lib -lxsmm -Wl,-rpath,$PWD/libxsmm-1_amd/lib -lm */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define VLEN 8      /* matrices per fp64 pack (the reference's AVX-512 width; libxsmm_amd_packed_width(8)) */
#define NPACKS 37
#define M 7
#define N 5
#define K 6
#define LD 9        /* leading dimension of every operand (column major, layout 102) */

/* element (i,j) of matrix v of pack p; an operand with `cols` columns */
static size_t at(int p, int cols, int i, int j, int v) { return ((size_t)p * LD * cols + (size_t)i + (size_t)j * LD) * VLEN + v; }

static double rnd(void) { return 2.0 * rand() / RAND_MAX - 1.0; }

static double* operand(int cols, int dominant)
{ /* uniform in (-1, 1); dominant: a heavy diagonal (LU without pivoting, well-conditioned triangles) */
  const size_t n = (size_t)NPACKS * LD * cols * VLEN;
  double* const x = (double*)malloc(sizeof(double) * n);
  int p, i, j, v;
  if (NULL == x) exit(100);
  for (p = 0; p < NPACKS; ++p) for (j = 0; j < cols; ++j) for (i = 0; i < LD; ++i) for (v = 0; v < VLEN; ++v) {
    x[at(p, cols, i, j, v)] = rnd() + ((0 != dominant && i == j) ? (double)(LD + 1) : 0.0);
  }
  return x;
}

static double* copy_of(const double* x, int cols)
{
  const size_t bytes = sizeof(double) * NPACKS * LD * cols * VLEN;
  double* const y = (double*)malloc(bytes);
  if (NULL == y) exit(100);
  memcpy(y, x, bytes);
  return y;
}

int main(void)
{
  const double one = 1.0, half = 0.5, tol = 1e-12;
  libxsmm_descriptor_blob blob;
  double worst = 0.0;
  int p, i, j, l, v, result = 0;
  srand(1);

  { /* pgemm: C += A * B */
    double *a = operand(K, 0), *b = operand(N, 0), *c = operand(N, 0), *c0 = copy_of(c, N);
    const libxsmm_pgemm_descriptor* const desc = libxsmm_pgemm_descriptor_init(&blob, 8, M, N, K, LD, LD, LD, &one, 'N', 'N', 102);
    const libxsmm_pgemm_xfunction kernel = libxsmm_dispatch_pgemm(desc);
    if (NULL == kernel) { fprintf(stderr, "no pgemm kernel\n"); return 1; }
    for (p = 0; p < NPACKS; ++p) kernel(a + at(p, K, 0, 0, 0), b + at(p, N, 0, 0, 0), c + at(p, N, 0, 0, 0));
    for (p = 0; p < NPACKS; ++p) for (v = 0; v < VLEN; ++v) for (j = 0; j < N; ++j) for (i = 0; i < M; ++i) {
      double s = c0[at(p, N, i, j, v)];
      for (l = 0; l < K; ++l) s += a[at(p, K, i, l, v)] * b[at(p, N, l, j, v)];
      worst = fmax(worst, fabs(s - c[at(p, N, i, j, v)]));
    }
    free(a); free(b); free(c); free(c0);
  }
  { /* getrf: A = L * U in place */
    double *a = operand(N, 1), *a0 = copy_of(a, N);
    const libxsmm_getrf_descriptor* const desc = libxsmm_getrf_descriptor_init(&blob, 8, M, N, LD, 102);
    const libxsmm_getrf_xfunction kernel = libxsmm_dispatch_getrf(desc);
    if (NULL == kernel) { fprintf(stderr, "no getrf kernel\n"); return 2; }
    for (p = 0; p < NPACKS; ++p) kernel(a + at(p, N, 0, 0, 0), a + at(p, N, 0, 0, 0), NULL);
    for (p = 0; p < NPACKS; ++p) for (v = 0; v < VLEN; ++v) for (j = 0; j < N; ++j) for (i = 0; i < M; ++i) {
      double s = 0.0; /* (L U)(i,j) with the unit diagonal of L */
      for (l = 0; l <= (i < j ? i : j); ++l) s += (l == i ? 1.0 : a[at(p, N, i, l, v)]) * a[at(p, N, l, j, v)];
      worst = fmax(worst, fabs(s - a0[at(p, N, i, j, v)]) / (LD + 1));
    }
    free(a); free(a0);
  }
  { /* trmm: B := 0.5 * A * B, A upper triangular of order M */
    double *a = operand(M, 1), *b = operand(N, 0), *b0 = copy_of(b, N);
    const libxsmm_trmm_descriptor* const desc = libxsmm_trmm_descriptor_init(&blob, 8, M, N, LD, LD, &half, 'N', 'N', 'L', 'U', 102);
    const libxsmm_trmm_xfunction kernel = libxsmm_dispatch_trmm(desc);
    double tmp[LD * N * VLEN];
    if (NULL == kernel) { fprintf(stderr, "no trmm kernel\n"); return 3; }
    for (p = 0; p < NPACKS; ++p) kernel(a + at(p, M, 0, 0, 0), b + at(p, N, 0, 0, 0), tmp);
    for (p = 0; p < NPACKS; ++p) for (v = 0; v < VLEN; ++v) for (j = 0; j < N; ++j) for (i = 0; i < M; ++i) {
      double s = 0.0;
      for (l = i; l < M; ++l) s += a[at(p, M, i, l, v)] * b0[at(p, N, l, j, v)];
      worst = fmax(worst, fabs(0.5 * s - b[at(p, N, i, j, v)]) / (LD + 1));
    }
    free(a); free(b); free(b0);
  }
  { /* trsm: A * X = B, A lower triangular of order M; once on host memory, once on device memory inside the bracket */
    double *a = operand(M, 1), *b = operand(N, 0), *b0 = copy_of(b, N);
    const size_t bytes_a = sizeof(double) * NPACKS * LD * M * VLEN, bytes_b = sizeof(double) * NPACKS * LD * N * VLEN;
    const libxsmm_trsm_descriptor* const desc = libxsmm_trsm_descriptor_init(&blob, 8, M, N, LD, LD, &one, 'N', 'N', 'L', 'L', 102);
    const libxsmm_trsm_xfunction kernel = libxsmm_dispatch_trsm(desc);
    double *da, *db, *x2 = (double*)malloc(bytes_b);
    libxsmm_kernel_kind kind;
    if (NULL == kernel || NULL == x2) { fprintf(stderr, "no trsm kernel\n"); return 4; }
    if (0 != libxsmm_get_kernel_kind((const void*)kernel, &kind) || LIBXSMM_KERNEL_KIND_TRSM != kind) return 5;
    for (p = 0; p < NPACKS; ++p) kernel(a + at(p, M, 0, 0, 0), b + at(p, N, 0, 0, 0), NULL);
    for (p = 0; p < NPACKS; ++p) for (v = 0; v < VLEN; ++v) for (j = 0; j < N; ++j) for (i = 0; i < M; ++i) {
      double s = 0.0;
      for (l = 0; l <= i; ++l) s += a[at(p, M, i, l, v)] * b[at(p, N, l, j, v)];
      worst = fmax(worst, fabs(s - b0[at(p, N, i, j, v)]) / (LD + 1));
    }
    /* the same loop on device memory: two lines around it, one launch instead of NPACKS */
    if (VLEN != libxsmm_amd_packed_width(8)) return 6;
    da = (double*)libxsmm_amd_device_malloc(bytes_a); db = (double*)libxsmm_amd_device_malloc(bytes_b);
    if (NULL == da || NULL == db || 0 != libxsmm_amd_memcpy_h2d(da, a, bytes_a) || 0 != libxsmm_amd_memcpy_h2d(db, b0, bytes_b)) return 7;
    libxsmm_amd_defer_begin();
    for (p = 0; p < NPACKS; ++p) kernel(da + at(p, M, 0, 0, 0), db + at(p, N, 0, 0, 0), NULL);
    libxsmm_amd_defer_end();
    if (0 != libxsmm_amd_memcpy_d2h(x2, db, bytes_b)) return 8;
    if (0 != memcmp(x2, b, bytes_b)) { fprintf(stderr, "bracketed trsm differs from the per-call results\n"); result = 9; }
    libxsmm_amd_device_free(da); libxsmm_amd_device_free(db);
    free(a); free(b); free(b0); free(x2);
  }
  libxsmm_finalize();
  printf("packed_caller: pgemm, getrf, trmm, trsm over %d packs of %d matrices, worst residual %.3g (%s)\n", NPACKS, VLEN, worst,
    (worst <= tol && 0 == result) ? "ok" : "FAILED");
  return (worst <= tol && 0 == result) ? 0 : (0 != result ? result : 10);
}
