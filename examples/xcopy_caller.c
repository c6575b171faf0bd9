/* xcopy_caller.c -- a caller of the copy / transposition interface, written against the reference API only.
 *
 * Four steps, each checked against plain loops (exit status 0: all equal, 1: a difference):
 *   1. out-of-place transposition over a list of shapes with tight and padded leading dimensions (the flow of the
 *      reference's tests/otrans.c), including the in-place form for the square ones; the padding of the destination must
 *      keep its contents;
 *   2. libxsmm_matcopy of a padded matrix, then the zero fill (in == NULL);
 *   3. a dispatched transposition kernel, called through its bare pointer;
 *   4. a dispatched matcopy kernel (plain, and with LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE and a prefetch argument).
 * Buffers come from libxsmm_malloc, as in the reference's tests.
 */
#include <libxsmm.h>
#include <stdio.h>
#include <string.h>

typedef double elem_t;

static void fill(elem_t* x, int count, int seed)
{
  int i;
  for (i = 0; i < count; ++i) x[i] = (elem_t)((i * 37 + seed * 101) % 1009) - 504.5;
}

/* number of positions where got differs from what a transposition of src (m x n, ldi) into a copy of before (ldo) gives */
static int check_trans(const elem_t* got, const elem_t* before, const elem_t* src, int m, int n, int ldi, int ldo, int count)
{
  int i, j, v, errors = 0;
  for (v = 0; v < count; ++v) {
    elem_t want = before[v];
    j = v % (0 < ldo ? ldo : 1); i = v / (0 < ldo ? ldo : 1); /* element (j, i) of the destination, which is n x m */
    if (j < n && i < m) want = src[j * ldi + i];
    if (0 != memcmp(&want, got + v, sizeof(elem_t))) ++errors;
  }
  return errors;
}

int main(void)
{
  static const int ms[] = { 0, 1, 1, 2, 3, 5, 5, 13, 16, 22, 63, 64, 16, 75, 300 };
  static const int ns[] = { 0, 1, 7, 2, 3, 1, 13, 5, 16, 22, 31, 64, 500, 130, 257 };
  static const int pi[] = { 0, 0, 2, 0, 0, 3, 0, 0, 0, 0, 1, 0, 0, 12, 20 };
  static const int po[] = { 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 12, 6, 63 };
  const int ntests = (int)(sizeof(ms) / sizeof(*ms));
  int t, i, j, errors = 0, max_a = 1, max_b = 1;
  elem_t *a, *b, *c;

  for (t = 0; t < ntests; ++t) {
    const int size_a = (ms[t] + pi[t]) * ns[t], size_b = (ns[t] + po[t]) * ms[t];
    if (max_a < size_a) max_a = size_a;
    if (max_b < size_b) max_b = size_b;
  }
  if (max_b < max_a) max_b = max_a;
  a = (elem_t*)libxsmm_malloc(sizeof(elem_t) * max_a);
  b = (elem_t*)libxsmm_malloc(sizeof(elem_t) * max_b);
  c = (elem_t*)libxsmm_malloc(sizeof(elem_t) * max_b);
  if (NULL == a || NULL == b || NULL == c) { fprintf(stderr, "xcopy_caller: out of memory\n"); return 1; }

  /* 1. transposition */
  for (t = 0; t < ntests; ++t) {
    const int m = ms[t], n = ns[t], ldi = m + pi[t], ldo = n + po[t], count = ldo * m;
    int e;
    fill(a, max_a, t); fill(b, max_b, 50 + t);
    memcpy(c, b, sizeof(elem_t) * max_b);
    libxsmm_otrans(b, a, sizeof(elem_t), m, n, ldi, ldo);
    e = check_trans(b, c, a, m, n, ldi, ldo, count);
    if (m == n && 0 < m && ldi == ldo) { /* the same in place */
      memcpy(c, a, sizeof(elem_t) * max_a);
      libxsmm_otrans(a, a, sizeof(elem_t), m, n, ldi, ldo);
      for (j = 0; j < n; ++j) for (i = 0; i < ldi; ++i) {
        const elem_t want = (i < m ? c[i * ldi + j] : c[j * ldi + i]);
        if (0 != memcmp(&want, a + j * ldi + i, sizeof(elem_t))) ++e;
      }
    }
    if (0 != e) fprintf(stderr, "xcopy_caller: transposition %d (%d x %d): %d differences\n", t, m, n, e);
    errors += e;
  }

  /* 2. matcopy and zero fill */
  {
    const int m = 45, n = 37, ldi = 50, ldo = 61;
    int e = 0;
    fill(a, max_a, 7); fill(b, max_b, 8);
    memcpy(c, b, sizeof(elem_t) * max_b);
    libxsmm_matcopy(b, a, sizeof(elem_t), m, n, ldi, ldo, NULL);
    for (j = 0; j < n; ++j) for (i = 0; i < ldo; ++i) {
      const elem_t want = (i < m ? a[j * ldi + i] : c[j * ldo + i]);
      if (0 != memcmp(&want, b + j * ldo + i, sizeof(elem_t))) ++e;
    }
    libxsmm_matcopy(b, NULL, sizeof(elem_t), m, n, ldi, ldo, NULL);
    for (j = 0; j < n; ++j) for (i = 0; i < ldo; ++i) {
      const elem_t want = (i < m ? (elem_t)0 : c[j * ldo + i]);
      if (0 != memcmp(&want, b + j * ldo + i, sizeof(elem_t))) ++e;
    }
    if (0 != e) fprintf(stderr, "xcopy_caller: matcopy: %d differences\n", e);
    errors += e;
  }

  /* 3. a dispatched transposition kernel */
  {
    const unsigned int m = 23, n = 17, ldi = 24, ldo = 19;
    libxsmm_descriptor_blob blob;
    const libxsmm_xtransfunction kernel = libxsmm_dispatch_trans(libxsmm_trans_descriptor_init(&blob, sizeof(elem_t), m, n, ldo));
    libxsmm_transkernel_info info;
    libxsmm_kernel_kind kind;
    int e = 0;
    if (NULL == kernel || EXIT_SUCCESS != libxsmm_get_transkernel_info(kernel, &info, NULL) || m != info.m || n != info.n || ldo != info.ldo
      || EXIT_SUCCESS != libxsmm_get_kernel_kind((const void*)kernel, &kind) || LIBXSMM_KERNEL_KIND_TRANS != kind)
    {
      fprintf(stderr, "xcopy_caller: transposition kernel: dispatch or info failed\n"); ++errors;
    }
    else {
      fill(a, max_a, 9); fill(b, max_b, 10);
      memcpy(c, b, sizeof(elem_t) * max_b);
      kernel(a, &ldi, b, &ldo);
      e = check_trans(b, c, a, (int)m, (int)n, (int)ldi, (int)ldo, (int)(ldo * m));
      if (0 != e) fprintf(stderr, "xcopy_caller: transposition kernel: %d differences\n", e);
      errors += e;
    }
  }

  /* 4. dispatched matcopy kernels */
  {
    const unsigned int m = 19, n = 11, ldi = 21, ldo = 26;
    libxsmm_descriptor_blob blob;
    const libxsmm_xmcopyfunction copy = libxsmm_dispatch_mcopy(libxsmm_mcopy_descriptor_init(&blob, sizeof(elem_t), m, n, ldo, ldi, 0, 0, NULL));
    const libxsmm_xmcopyfunction zero = libxsmm_dispatch_mcopy(libxsmm_mcopy_descriptor_init(&blob, sizeof(elem_t), m, n, ldo, ldi,
      LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE, 1, NULL));
    int e = 0;
    if (NULL == copy || NULL == zero || copy == zero) { fprintf(stderr, "xcopy_caller: matcopy kernel: dispatch failed\n"); ++errors; }
    else {
      fill(a, max_a, 11); fill(b, max_b, 12);
      memcpy(c, b, sizeof(elem_t) * max_b);
      copy(a, &ldi, b, &ldo);
      for (j = 0; j < (int)n; ++j) for (i = 0; i < (int)ldo; ++i) {
        const elem_t want = (i < (int)m ? a[j * ldi + i] : c[j * ldo + i]);
        if (0 != memcmp(&want, b + j * ldo + i, sizeof(elem_t))) ++e;
      }
      zero(a, &ldi, b, &ldo, a + ldi); /* the source is ignored, the prefetch argument too */
      for (j = 0; j < (int)n; ++j) for (i = 0; i < (int)ldo; ++i) {
        const elem_t want = (i < (int)m ? (elem_t)0 : c[j * ldo + i]);
        if (0 != memcmp(&want, b + j * ldo + i, sizeof(elem_t))) ++e;
      }
      if (0 != e) fprintf(stderr, "xcopy_caller: matcopy kernel: %d differences\n", e);
      errors += e;
    }
  }

  libxsmm_free(a); libxsmm_free(b); libxsmm_free(c);
  libxsmm_finalize();
  printf("xcopy_caller: %s (%d differences)\n", 0 == errors ? "ok" : "FAILED", errors);
  return 0 == errors ? 0 : 1;
}
