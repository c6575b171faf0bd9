/* matdiff_caller.c -- the last hop of a device-resident workflow (the end of samples/smm/specialized.cpp:224-238 and
 * samples/cp2k/cp2k.cpp:370-374): a batch of small products stays in device memory and is compared there against the expected
 * results with libxsmm_amd_matdiff_batch; only the filled libxsmm_matdiff_info comes back. One item is disturbed on purpose
 * and must be the one that is reported.
 *   gcc -std=c89 -Wall -I include examples/matdiff_caller.c -L libxsmm-1_amd/lib -lxsmm -lm */
#include <libxsmm.h>
#include <libxsmm_amd.h>
#include <stdio.h>
#include <stdlib.h>

int main(void)
{
  const libxsmm_blasint m = 32, n = 32;
  const long long batch = 1000, stride = 32 * 32, disturbed = 617;
  const size_t count = (size_t)(batch * stride), bytes = sizeof(double) * count;
  double *ref = (double*)malloc(bytes), *tst = (double*)malloc(bytes), *dref, *dtst;
  libxsmm_matdiff_info info, one;
  long long item = -2;
  size_t i;
  int result = EXIT_SUCCESS;
  if (NULL == ref || NULL == tst) return EXIT_FAILURE;
  for (i = 0; i < count; ++i) tst[i] = ref[i] = 0.5 - (double)((i * 7) % 113) / 150.0;
  tst[disturbed * stride + 5 * m + 3] += 0.25; /* line 5, element 3 of one item */

  libxsmm_init();
  dref = (double*)libxsmm_amd_device_malloc(bytes);
  dtst = (double*)libxsmm_amd_device_malloc(bytes);
  if (NULL == dref || NULL == dtst) { fprintf(stderr, "matdiff_caller: no device memory\n"); return EXIT_FAILURE; }
  libxsmm_amd_memcpy_h2d(dref, ref, bytes);
  libxsmm_amd_memcpy_h2d(dtst, tst, bytes);

  /* the whole batch by one set of launches; info is host memory: the call waits for it */
  if (EXIT_SUCCESS != libxsmm_amd_matdiff_batch(&info, NULL, &item, LIBXSMM_DATATYPE_F64, m, n, dref, dtst, NULL, NULL, stride, stride, batch)) {
    fprintf(stderr, "matdiff_caller: libxsmm_amd_matdiff_batch failed\n"); result = EXIT_FAILURE;
  }
  /* the plain call takes device operands as well */
  if (EXIT_SUCCESS != libxsmm_matdiff(&one, LIBXSMM_DATATYPE_F64, m, n, dref + disturbed * stride, dtst + disturbed * stride, NULL, NULL)) {
    fprintf(stderr, "matdiff_caller: libxsmm_matdiff failed\n"); result = EXIT_FAILURE;
  }
  if (disturbed != item || 3 != info.m || 5 != info.n || info.linf_abs < 0.2499 || info.linf_abs > 0.2501 || one.linf_abs != info.linf_abs
    || one.m != info.m || one.n != info.n || one.l2_abs != info.l2_abs)
  {
    fprintf(stderr, "matdiff_caller: item %ld at (%d, %d) with linf_abs %g, expected item %ld at (3, 5) with 0.25\n",
      (long)item, (int)info.m, (int)info.n, info.linf_abs, (long)disturbed);
    result = EXIT_FAILURE;
  }
  if (EXIT_SUCCESS == result) {
    printf("matdiff_caller: ok (item %ld, m %d, n %d)\n", (long)item, (int)info.m, (int)info.n);
    printf("  norm1_abs %g norm1_rel %g normi_abs %g normi_rel %g normf_rel %g\n", info.norm1_abs, info.norm1_rel, info.normi_abs, info.normi_rel, info.normf_rel);
    printf("  linf_abs %g linf_rel %g l2_abs %g l2_rel %g\n", info.linf_abs, info.linf_rel, info.l2_abs, info.l2_rel);
    printf("  l1_ref %g min_ref %g max_ref %g avg_ref %g var_ref %g\n", info.l1_ref, info.min_ref, info.max_ref, info.avg_ref, info.var_ref);
    printf("  l1_tst %g min_tst %g max_tst %g avg_tst %g var_tst %g\n", info.l1_tst, info.min_tst, info.max_tst, info.avg_tst, info.var_tst);
  }
  libxsmm_amd_device_free(dref); libxsmm_amd_device_free(dtst);
  free(ref); free(tst);
  libxsmm_finalize();
  return result;
}
