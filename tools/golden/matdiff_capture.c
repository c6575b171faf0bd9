/* matdiff_capture.c -- calls libxsmm_matdiff and libxsmm_matdiff_reduce of the unmodified reference and writes what they
 * return as raw binary, for tools/golden/matdiff_capture.py to pack into tests/golden/matdiff.npz. It includes the reference
 * header-only, as the reference's own tests/matdiff.c does, so it needs the reference's generated headers (its make writes
 * include/libxsmm.h and include/libxsmm_config.h) and no library:
 *   gcc -O1 -I<reference>/include matdiff_capture.c -lm -lpthread -ldl -lrt -o matdiff_capture
 * Usage: matdiff_capture single dt m n ldref ldtst ref|- tst|- out      a file of elements per operand, "-" for NULL
 *        matdiff_capture batch  dt m n ldref ldtst stride_ref stride_tst batch ref tst out
 * dt: the value of libxsmm_datatype. out: per info 22 doubles -- the 19 fields in the order of the struct, m, n, the return
 * value; batch writes one info per item and then the info that libxsmm_matdiff_reduce forms of them from a cleared one. */
#include <libxsmm_source.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void* slurp(const char* path)
{
  FILE* f;
  long bytes;
  void* p;
  if (0 == strcmp(path, "-")) return NULL;
  f = fopen(path, "rb");
  if (NULL == f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END); bytes = ftell(f); fseek(f, 0, SEEK_SET);
  p = malloc((size_t)bytes + 64);
  if (NULL == p || (size_t)bytes != fread(p, 1, (size_t)bytes, f)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
  return p;
}

static void put(FILE* f, const libxsmm_matdiff_info* d, int rc)
{
  double v[22];
  v[0] = d->norm1_abs; v[1] = d->norm1_rel; v[2] = d->normi_abs; v[3] = d->normi_rel; v[4] = d->normf_rel;
  v[5] = d->linf_abs; v[6] = d->linf_rel; v[7] = d->l2_abs; v[8] = d->l2_rel;
  v[9] = d->l1_ref; v[10] = d->min_ref; v[11] = d->max_ref; v[12] = d->avg_ref; v[13] = d->var_ref;
  v[14] = d->l1_tst; v[15] = d->min_tst; v[16] = d->max_tst; v[17] = d->avg_tst; v[18] = d->var_tst;
  v[19] = (double)d->m; v[20] = (double)d->n; v[21] = (double)rc;
  if (22 != fwrite(v, sizeof(double), 22, f)) { fprintf(stderr, "cannot write\n"); exit(2); }
}

int main(int argc, char* argv[])
{
  const char* const what = (1 < argc ? argv[1] : "");
  libxsmm_matdiff_info info;
  if (0 == strcmp(what, "single") && 10 == argc) {
    const libxsmm_datatype dt = (libxsmm_datatype)atoi(argv[2]);
    const libxsmm_blasint m = atoi(argv[3]), n = atoi(argv[4]), ldr = atoi(argv[5]), ldt = atoi(argv[6]);
    const void *const ref = slurp(argv[7]), *const tst = slurp(argv[8]);
    FILE* const f = fopen(argv[9], "wb");
    int rc;
    if (NULL == f) return 2;
    libxsmm_matdiff_clear(&info);
    rc = libxsmm_matdiff(&info, dt, m, n, ref, tst, &ldr, &ldt);
    put(f, &info, rc);
    fclose(f);
    return 0;
  }
  if (0 == strcmp(what, "batch") && 13 == argc) {
    const libxsmm_datatype dt = (libxsmm_datatype)atoi(argv[2]);
    const libxsmm_blasint m = atoi(argv[3]), n = atoi(argv[4]), ldr = atoi(argv[5]), ldt = atoi(argv[6]);
    const long sr = atol(argv[7]), st = atol(argv[8]), batch = atol(argv[9]);
    const char *const ref = (const char*)slurp(argv[10]), *const tst = (const char*)slurp(argv[11]);
    const size_t ts = libxsmm_typesize(dt);
    FILE* const f = fopen(argv[12], "wb");
    libxsmm_matdiff_info total;
    long i;
    if (NULL == f || NULL == ref || NULL == tst) return 2;
    libxsmm_matdiff_clear(&total);
    for (i = 0; i < batch; ++i) {
      const int rc = libxsmm_matdiff(&info, dt, m, n, ref + (size_t)i * (size_t)sr * ts, tst + (size_t)i * (size_t)st * ts, &ldr, &ldt);
      put(f, &info, rc);
      libxsmm_matdiff_reduce(&total, &info);
    }
    put(f, &total, 0);
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: see the head of matdiff_capture.c\n");
  return 1;
}
