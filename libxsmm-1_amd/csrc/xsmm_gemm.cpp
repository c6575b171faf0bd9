// xsmm_gemm.cpp -- the public entry points of the batched SMM front end: libxsmm_mmbatch / gemm_batch(_omp) / ?gemm_batch /
// ?gemm, the BLAS call wrappers and the diagnostic exports. Each job they share has a file of its own: address arithmetic
// xsmm_batch.hpp, launch chain, residency and staging xsmm_batch.cpp, recorders xsmm_batch_record.cpp, thunks xsmm_call.cpp.
// Reference: src/libxsmm_gemm.c (libxsmm_mmbatch_kernel :1315-1608, libxsmm_mmbatch :1809-1875,
// libxsmm_gemm_batch :1878-1888, ?gemm_batch :1231-1262, ?gemm :1265-1290) and src/libxsmm_ext_gemm.c
// (OpenMP batch driver :758-1013, auto-batch :1016-1135).
#include "xsmm_internal.hpp"
#include "xsmm_batch.hpp"

#include <cstring>

using namespace xsmm;

// ---- public batch interface ------------------------------------------------------------------------------------
LIBXSMM_API int libxsmm_mmbatch_kernel(libxsmm_xmmfunction kernel, libxsmm_blasint index_base,
  libxsmm_blasint index_stride, const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  const void* a, const void* b, void* c, libxsmm_blasint batchsize, /*unsigned*/int tid, /*unsigned*/int ntasks,
  unsigned char itypesize, unsigned char otypesize, int flags)
{ // reference src/libxsmm_gemm.c:1315-1324: task `tid` of `ntasks` owns the slice [tid*tasksize, min(...))
  (void)itypesize; (void)otypesize; (void)flags;
  Kernel* const k = kernel_from_pointer(reinterpret_cast<const void*>(kernel.xmm));
  if (nullptr == k || KC_CSR_REG == k->kclass || KC_TEXT == k->kclass || KC_PACKED == k->kclass || KC_XCOPY == k->kclass || nullptr == a || nullptr == b || nullptr == c || ntasks < 1 || tid < 0 || tid >= ntasks) return EXIT_FAILURE;
  const TaskSlice slice = task_slice(batch_size(batchsize), tid, ntasks);
  if (KC_LOWP == k->kclass) return lowp_batch_execute(k, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, slice.begin, slice.end);
  // inside a libxsmm_amd_defer_begin/end bracket: recorded, leaves with its neighbours at the flush
  if (record_batch_call(k, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, batchsize, ntasks)) return EXIT_SUCCESS;
  record_flush(); // a call that is not recorded runs behind the recorded ones
  SmmBatch s = from_descriptor(k->desc);
  s.relaxed = relaxed_order(ntasks, index_stride, c) ? 1 : 0;
  s.shared_across_calls = (1 < ntasks && 0 <= batchsize) ? 1 : 0; // (a negative batchsize is the caller's promise that nothing is shared)
  s.tasks = ntasks;
  // ntasks > 1: the tasks run concurrently on the caller's threads and may share C across slices; as in the
  // reference (lock per C, :1366-1423) correctness then needs atomic updates unless the caller opts out.
  // (batch-reduce: all products of the slice land in consecutive-equal C runs by construction, no opting out)
  const bool nosync = (batchsize < 0 && KC_REDUCE != k->kclass);
  return batch_execute(s, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, slice.begin, slice.end, nosync);
}

namespace {
// What BLAS checks before it computes (xerbla: "parameter ... had an illegal value"; the reference hands these calls to BLAS):
// a leading dimension smaller than the rows it has to hold is an error, never a launch -- the kernel would read beyond the operands.
bool blas_lds_valid(const char* who, int flags, long long m, long long n, long long k, long long lda, long long ldb, long long ldc)
{
  const long long rows_a = (0 == (LIBXSMM_GEMM_FLAG_TRANS_A & flags)) ? m : k, rows_b = (0 == (LIBXSMM_GEMM_FLAG_TRANS_B & flags)) ? k : n;
  if (lda >= (rows_a > 1 ? rows_a : 1) && ldb >= (rows_b > 1 ? rows_b : 1) && ldc >= (m > 1 ? m : 1)) return true;
  static int error_once = 0;
  if (once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: %s: illegal leading dimension (lda=%lld ldb=%lld ldc=%lld for m=%lld n=%lld k=%lld)\n", who, lda, ldb, ldc, m, n, k);
  return false;
}
LeadingDims lds_of(int flags, long long m, long long n, long long k, const libxsmm_blasint* lda, const libxsmm_blasint* ldb, const libxsmm_blasint* ldc)
{ // the leading dimensions of a call: the caller's, or what BLAS assumes for these transposes
  LeadingDims ld = default_lds(0 != (LIBXSMM_GEMM_FLAG_TRANS_A & flags), 0 != (LIBXSMM_GEMM_FLAG_TRANS_B & flags), m, n, k);
  if (nullptr != lda) ld.a = *lda;
  if (nullptr != ldb) ld.b = *ldb;
  if (nullptr != ldc) ld.c = *ldc;
  return ld;
}

// C = alpha*op(A)*op(B) + beta*C for every item -- what the reference delegates to BLAS
// (libxsmm_mmbatch_blas, src/libxsmm_gemm.c:1778-1806): shapes/scalars outside the SMM domain.
int batch_general(int typesize, const char* transa, const char* transb, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k,
  const void* alpha, const void* a, const libxsmm_blasint* lda, const void* b, const libxsmm_blasint* ldb,
  const void* beta, void* c, const libxsmm_blasint* ldc, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  long long begin, long long end, int ntasks = 1)
{
  const int flags = LIBXSMM_GEMM_PFLAGS(transa, transb, LIBXSMM_FLAGS);
  SmmBatch s; memset(&s, 0, sizeof(s));
  s.tasks = ntasks;
  s.typesize = typesize; s.m = m; s.n = n; s.k = k;
  const LeadingDims ld = lds_of(flags, m, n, k, lda, ldb, ldc);
  s.lda = (int)ld.a; s.ldb = (int)ld.b; s.ldc = (int)ld.c;
  s.flags = flags & (LIBXSMM_GEMM_FLAG_TRANS_A | LIBXSMM_GEMM_FLAG_TRANS_B);
  s.general = 1;
  if (8 == typesize) { s.alpha = (nullptr != alpha ? *static_cast<const double*>(alpha) : 1.0); s.beta = (nullptr != beta ? *static_cast<const double*>(beta) : 1.0); }
  else { s.alpha = (nullptr != alpha ? *static_cast<const float*>(alpha) : 1.f); s.beta = (nullptr != beta ? *static_cast<const float*>(beta) : 1.f); }
  if (m <= 0 || n <= 0 || k < 0) return EXIT_SUCCESS;
  if (!blas_lds_valid("batch of general products", s.flags, m, n, k, s.lda, s.ldb, s.ldc)) return EXIT_FAILURE;
  return batch_execute(s, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, begin, end, true);
}
} // namespace

LIBXSMM_API int libxsmm_mmbatch_blas(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec,
  const char* transa, const char* transb, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k,
  const void* alpha, const void* a, const libxsmm_blasint* lda, const void* b, const libxsmm_blasint* ldb,
  const void* beta, void* c, const libxsmm_blasint* ldc, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  libxsmm_blasint batchsize)
{
  if (nullptr == a || nullptr == b || nullptr == c || iprec != oprec ||
      (LIBXSMM_GEMM_PRECISION_F64 != iprec && LIBXSMM_GEMM_PRECISION_F32 != iprec)) return EXIT_FAILURE;
  return batch_general(LIBXSMM_GEMM_PRECISION_F64 == iprec ? 8 : 4, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc,
    index_base, index_stride, stride_a, stride_b, stride_c, 0, batch_size(batchsize));
}

LIBXSMM_API void libxsmm_mmbatch(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec,
  const char* transa, const char* transb, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k,
  const void* alpha, const void* a, const libxsmm_blasint* lda, const void* b, const libxsmm_blasint* ldb,
  const void* beta, void* c, const libxsmm_blasint* ldc, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  libxsmm_blasint batchsize, /*unsigned*/int tid, /*unsigned*/int nthreads)
{ // reference src/libxsmm_gemm.c:1809-1875
  static int error_once = 0;
  if (nullptr == a || nullptr == b || nullptr == c || tid < 0 || tid >= nthreads) {
    if (0 != libxsmm_verbosity && once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: incorrect arguments (libxsmm_mmbatch)!\n");
    return;
  }
  libxsmm_init();
  int result = EXIT_FAILURE;
  const unsigned char otypesize = libxsmm_typesize((libxsmm_datatype)oprec);
  const int gemm_flags = LIBXSMM_GEMM_PFLAGS(transa, transb, LIBXSMM_FLAGS);
  libxsmm_descriptor_blob blob;
  const LeadingDims ld = lds_of(gemm_flags, m, n, k, lda, ldb, ldc);
  libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_init2(&blob, iprec, oprec, m, n, k,
    (libxsmm_blasint)ld.a, (libxsmm_blasint)ld.b, (libxsmm_blasint)ld.c, alpha, beta, gemm_flags, libxsmm_get_gemm_auto_prefetch());
  if (nullptr != desc) { // the AI gate of the reference (:1827) selects BLAS for large shapes; one device path serves both here
    const libxsmm_xmmfunction kernel = libxsmm_xmmdispatch(desc);
    if (nullptr != kernel.xmm) {
      result = libxsmm_mmbatch_kernel(kernel, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, batchsize,
        tid, nthreads, libxsmm_typesize((libxsmm_datatype)iprec), otypesize, desc->flags);
    }
  }
  if (EXIT_SUCCESS != result && iprec == oprec && (LIBXSMM_GEMM_PRECISION_F64 == iprec || LIBXSMM_GEMM_PRECISION_F32 == iprec)) {
    // quiet fall-back (:1842-1866): general alpha/beta/transposes
    const TaskSlice slice = task_slice(batch_size(batchsize), tid, nthreads);
    result = batch_general(LIBXSMM_GEMM_PRECISION_F64 == iprec ? 8 : 4, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc,
      index_base, index_stride, stride_a, stride_b, stride_c, slice.begin, slice.end, nthreads);
  }
  if (EXIT_SUCCESS != result && 0 != libxsmm_verbosity && once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: libxsmm_mmbatch failed!\n");
}

LIBXSMM_API void libxsmm_gemm_batch(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec,
  const char* transa, const char* transb, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k,
  const void* alpha, const void* a, const libxsmm_blasint* lda, const void* b, const libxsmm_blasint* ldb,
  const void* beta, void* c, const libxsmm_blasint* ldc, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  libxsmm_blasint batchsize)
{
  libxsmm_mmbatch(iprec, oprec, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, index_base, index_stride,
    stride_a, stride_b, stride_c, batchsize, 0/*tid*/, 1/*nthreads*/);
}

LIBXSMM_APIEXT void libxsmm_gemm_batch_omp(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec,
  const char* transa, const char* transb, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k,
  const void* alpha, const void* a, const libxsmm_blasint* lda, const void* b, const libxsmm_blasint* ldb,
  const void* beta, void* c, const libxsmm_blasint* ldc, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  libxsmm_blasint batchsize)
{ // the reference spreads the batch over OpenMP threads (src/libxsmm_ext_gemm.c:758-972); the device grid is the
  // parallel loop here, so the whole batch is one launch
  ++tl_relaxed_order;
  libxsmm_mmbatch(iprec, oprec, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, index_base, index_stride,
    stride_a, stride_b, stride_c, batchsize, 0, 1);
  --tl_relaxed_order;
}

namespace {
// libxsmm_?gemm_batch[_omp] with several groups whose matrices live on the device: the groups as one fused launch (run_groups)
// instead of one batch call after the other. Only when every group is in the SMM domain and no C matrix of one group overlaps
// the C matrices of another (the reference works the groups off one after the other, so overlapping groups must stay in that
// order). false: not applicable, nothing was done.
template<typename T>
bool try_grouped_pointer_batches(libxsmm_gemm_precision prec, bool relaxed, const char transa_array[], const char transb_array[],
  const libxsmm_blasint m_array[], const libxsmm_blasint n_array[], const libxsmm_blasint k_array[],
  const T alpha_array[], const T* a_array[], const libxsmm_blasint lda_array[], const T* b_array[], const libxsmm_blasint ldb_array[],
  const T beta_array[], T* c_array[], const libxsmm_blasint ldc_array[], libxsmm_blasint ngroups, const libxsmm_blasint group_size[])
{
  if (ngroups < 2 || !device_ready()) return false;
  if (is_device_ptr(a_array) || is_device_ptr(b_array) || is_device_ptr(c_array)) return false; // (pointer arrays the CPU cannot read: group by group)
  std::vector<SmmBatch> groups; groups.reserve((size_t)ngroups);
  struct Hulls { unsigned long long of[6]; }; // {a_lo, a_hi, b_lo, b_hi, c_lo, c_hi}: the address ranges the matrices of a group occupy
  std::vector<Hulls> hulls; hulls.reserve((size_t)ngroups);
  long long j = 0;
  for (libxsmm_blasint g = 0; g < ngroups; ++g) {
    const long long size = LIBXSMM_ABS(group_size[g]);
    if (0 == size) continue;
    const int flags = LIBXSMM_GEMM_PFLAGS(transa_array + g, transb_array + g, LIBXSMM_FLAGS);
    libxsmm_descriptor_blob blob;
    const libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_init2(&blob, prec, prec, m_array[g], n_array[g], k_array[g],
      lda_array[g], ldb_array[g], ldc_array[g], alpha_array + g, beta_array + g, flags, LIBXSMM_GEMM_PREFETCH_NONE);
    const Kernel* const kern = (nullptr != desc ? kernel_from_pointer(reinterpret_cast<const void*>(libxsmm_xmmdispatch(desc).xmm)) : nullptr);
    if (nullptr == kern || KC_DENSE != kern->kclass) return false;
    const int kc = pointer_kind(c_array[j]);
    if (0 == (pointer_kind(a_array[j]) & pointer_kind(b_array[j]) & kc & 1) || 0 != (kc & 2)) return false; // host matrices: the staging path
    SmmBatch s = from_descriptor(kern->desc);
    s.mode = ADDR_POINTER; s.sa = s.sb = s.sc = (long long)sizeof(void*); s.batch = size;
    s.relaxed = relaxed_order(relaxed ? 2 : 1, 0, c_array + j) ? 1 : 0; s.c_atomics = 1;
    s.sync = c_verdict_needed(0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0), group_size[g]) ? SYNC_DEVICE : SYNC_NONE;
    Hulls hull;
    hull_of_pointers(hull.of + 0, reinterpret_cast<const void* const*>(a_array + j), (size_t)size, (int)sizeof(T), span_a(s));
    hull_of_pointers(hull.of + 2, reinterpret_cast<const void* const*>(b_array + j), (size_t)size, (int)sizeof(T), span_b(s));
    hull_of_pointers(hull.of + 4, reinterpret_cast<const void* const*>(c_array + j), (size_t)size, (int)sizeof(T), span_c(s));
    hulls.push_back(hull);
    s.a = a_array + j; s.b = b_array + j; s.c = c_array + j; // (host arrays for now: uploaded below, once all groups have passed)
    groups.push_back(s);
    j += size;
  }
  // The reference runs the groups strictly one after the other: a later group may read (as A or B) or update what an earlier
  // one wrote. Fused, the groups run side by side -- only if no group's C meets another group's C, A or B.
  std::vector<int> segment(groups.size());
  if (!groups.empty() && 1 < merge_segments((int)groups.size(), hulls.data()->of, segment.data())) return false;
  bool ok = true;
  for (SmmBatch& s : groups) {
    if (!upload_pointer_arrays(s, device().stream, s.a, (size_t)s.batch, s.b, (size_t)s.batch, s.c, (size_t)s.batch)) { ok = false; break; }
  }
  if (ok) ok = (0 == run_groups(groups));
  index_upload_commit();
  if (!ok) { static int error_once = 0; if (0 != libxsmm_verbosity && once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: libxsmm_?gemm_batch failed!\n"); }
  return true;
}
}

#define XSMM_GROUP_BATCH(NAME, T, PREC, CALL, RELAXED)                                                                     \
LIBXSMM_API void NAME(const char transa_array[], const char transb_array[],                                   \
  const libxsmm_blasint m_array[], const libxsmm_blasint n_array[], const libxsmm_blasint k_array[],         \
  const T alpha_array[], const T* a_array[], const libxsmm_blasint lda_array[],                              \
  const T* b_array[], const libxsmm_blasint ldb_array[],                                                     \
  const T beta_array[], T* c_array[], const libxsmm_blasint ldc_array[],                                     \
  const libxsmm_blasint* group_count, const libxsmm_blasint group_size[])                                    \
{ /* reference src/libxsmm_gemm.c:1231-1262: one pointer-array batch per homogeneous group */                \
  const libxsmm_blasint ngroups = LIBXSMM_ABS(*group_count), ptrsize = (libxsmm_blasint)sizeof(void*);       \
  libxsmm_blasint i, j = 0;                                                                                    \
  libxsmm_init();                                                                                              \
  if (try_grouped_pointer_batches<T>(PREC, RELAXED, transa_array, transb_array, m_array, n_array, k_array, alpha_array, a_array, lda_array, \
        b_array, ldb_array, beta_array, c_array, ldc_array, ngroups, group_size)) return;                      \
  for (i = 0; i < ngroups; ++i) {                                                                              \
    const libxsmm_blasint size = group_size[i];                                                                \
    CALL(PREC, PREC, transa_array + i, transb_array + i, m_array[i], n_array[i], k_array[i],  \
      alpha_array + i, a_array + j, lda_array + i, b_array + j, ldb_array + i, beta_array + i, c_array + j,  \
      ldc_array + i, 0/*index_base*/, 0/*index_stride*/, &ptrsize, &ptrsize, &ptrsize, size);                \
    j += LIBXSMM_ABS(size);                                                                                    \
  }                                                                                                            \
}
XSMM_GROUP_BATCH(libxsmm_dgemm_batch, double, LIBXSMM_GEMM_PRECISION_F64, libxsmm_gemm_batch, false)
XSMM_GROUP_BATCH(libxsmm_sgemm_batch, float, LIBXSMM_GEMM_PRECISION_F32, libxsmm_gemm_batch, false)
XSMM_GROUP_BATCH(libxsmm_dgemm_batch_omp, double, LIBXSMM_GEMM_PRECISION_F64, libxsmm_gemm_batch_omp, true)
XSMM_GROUP_BATCH(libxsmm_sgemm_batch_omp, float, LIBXSMM_GEMM_PRECISION_F32, libxsmm_gemm_batch_omp, true)

LIBXSMM_API int libxsmm_amd_gemm_batch_strided(const libxsmm_gemm_descriptor* descriptor,
  const void* a, const void* b, void* c, long long stride_a, long long stride_b, long long stride_c, long long batchsize)
{
  if (nullptr == descriptor || nullptr == a || nullptr == b || nullptr == c || batchsize < 0) return EXIT_FAILURE;
  const libxsmm_xmmfunction kernel = libxsmm_xmmdispatch(descriptor); // validates like any dispatch
  if (nullptr == kernel.xmm) return EXIT_FAILURE;
  if (!device_ready()) { fail_no_device("libxsmm_amd_gemm_batch_strided"); return EXIT_FAILURE; }
  const Residency where = classify(a, b, c);
  if (!where.device()) {
    fprintf(stderr, "LIBXSMM-AMD ERROR: libxsmm_amd_gemm_batch_strided needs device-resident operands\n");
    return EXIT_FAILURE;
  }
  if (0 == batchsize) return EXIT_SUCCESS;
  const Kernel* const k = kernel_from_pointer(reinterpret_cast<const void*>(kernel.xmm));
  if (nullptr != k && KC_LOWP == k->kclass) { // i16 / bf16 inputs: independent C operands (strides in elements of the respective type)
    if (0 == stride_c && 1 < batchsize) return EXIT_FAILURE;
    if (0 != (k->desc.flags & LIBXSMM_GEMM_FLAG_BATCH_REDUCE)) return EXIT_FAILURE;
    if (LIBXSMM_GEMM_PRECISION_I16 == LIBXSMM_GETENUM_INP(k->desc.datatype) && LIBXSMM_GEMM_PRECISION_F32 == LIBXSMM_GETENUM_OUT(k->desc.datatype)) return EXIT_FAILURE; // no way to pass the scaling factor
    SmmBatch s = lowp_from_descriptor(k->desc, 1.f);
    s.mode = ADDR_STRIDED; s.a = a; s.b = b; s.c = c; s.sa = stride_a; s.sb = stride_b; s.sc = stride_c; s.batch = batchsize; s.sync = SYNC_NONE;
    return 0 == lowp_launch(s) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  SmmBatch s = from_descriptor(*descriptor);
  s.mode = ADDR_STRIDED; s.a = a; s.b = b; s.c = c; s.sa = stride_a; s.sb = stride_b; s.sc = stride_c; s.batch = batchsize;
  s.sync = (0 == stride_c && 0 == (s.flags & LIBXSMM_GEMM_FLAG_BETA_0) && 1 < batchsize) ? SYNC_RUNS : SYNC_NONE;
  return 0 == run_smm(s, where.visible()) ? EXIT_SUCCESS : EXIT_FAILURE;
}

LIBXSMM_API int libxsmm_amd_gemm_batch_groups(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, int ngroups,
  const char transa[], const char transb[], const libxsmm_blasint m[], const libxsmm_blasint n[], const libxsmm_blasint k[],
  const libxsmm_blasint lda[], const libxsmm_blasint ldb[], const libxsmm_blasint ldc[], const void* alpha, const void* beta,
  const void* const a[], const void* const b[], void* const c[], libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* const stride_a[], const libxsmm_blasint* const stride_b[], const libxsmm_blasint* const stride_c[],
  const libxsmm_blasint group_size[], int relaxed)
{ // ngroups calls of libxsmm_gemm_batch (index arrays) as one call, see include/libxsmm_amd.h
  if (ngroups < 0 || (0 < ngroups && (nullptr == m || nullptr == n || nullptr == k || nullptr == a || nullptr == b || nullptr == c || nullptr == group_size)) || 0 == index_stride) return EXIT_FAILURE;
  if (0 == ngroups) return EXIT_SUCCESS;
  libxsmm_init();
  if (!device_ready()) { fail_no_device("libxsmm_amd_gemm_batch_groups"); return EXIT_FAILURE; }
  std::vector<SmmBatch> groups; groups.reserve((size_t)ngroups);
  bool ok = true, host_visible = false;
  const int order_env = batch_order_env();
  for (int g = 0; g < ngroups && ok; ++g) {
    const char ta = (nullptr != transa ? transa[g] : 'N'), tb = (nullptr != transb ? transb[g] : 'N');
    const int flags = LIBXSMM_GEMM_PFLAGS(&ta, &tb, LIBXSMM_FLAGS);
    libxsmm_descriptor_blob blob;
    const LeadingDims ld = lds_of(flags, m[g], n[g], k[g], nullptr != lda ? lda + g : nullptr, nullptr != ldb ? ldb + g : nullptr, nullptr != ldc ? ldc + g : nullptr);
    const libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_init2(&blob, iprec, oprec, m[g], n[g], k[g],
      (libxsmm_blasint)ld.a, (libxsmm_blasint)ld.b, (libxsmm_blasint)ld.c, alpha, beta, flags, LIBXSMM_GEMM_PREFETCH_NONE);
    const Kernel* const kern = (nullptr != desc ? kernel_from_pointer(reinterpret_cast<const void*>(libxsmm_xmmdispatch(desc).xmm)) : nullptr);
    if (nullptr == kern || KC_DENSE != kern->kclass) { ok = false; break; } // outside the SMM domain (alpha, beta, TRANS_A, precision)
    const long long size = batch_size(group_size[g]);
    const int ka = pointer_kind(a[g]), kb = pointer_kind(b[g]), kc = pointer_kind(c[g]); // (one driver query per operand)
    if (0 == (ka & kb & kc & 1)) {
      fprintf(stderr, "LIBXSMM-AMD ERROR: libxsmm_amd_gemm_batch_groups needs operands the GPU can reach (device memory or libxsmm_malloc)\n");
      ok = false; break;
    }
    host_visible = host_visible || 0 != ((ka | kb | kc) & 2);
    SmmBatch s = from_descriptor(kern->desc);
    s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride; s.a = a[g]; s.b = b[g]; s.c = c[g]; s.batch = size;
    // any order of the sums only where the caller allows it (or LIBXSMM_AMD_BATCH_ORDER=relaxed) and never for C the CPU addresses
    s.relaxed = ((0 != relaxed || 0 < order_env) && 0 <= order_env && 0 == (kc & 2)) ? 1 : 0;
    s.c_atomics = (0 != (kc & 2)) ? 0 : 1;
    if (0 < size) {
      s.ia = device_indexes(nullptr != stride_a ? stride_a[g] : nullptr, index_stride, size, &ok);
      s.ib = device_indexes(nullptr != stride_b ? stride_b[g] : nullptr, index_stride, size, &ok);
      s.ic = device_indexes(nullptr != stride_c ? stride_c[g] : nullptr, index_stride, size, &ok);
    }
    s.sync = c_verdict_needed(0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0), group_size[g]) ? SYNC_DEVICE : SYNC_NONE;
    groups.push_back(s);
  }
  int e = -1;
  if (ok) e = run_groups(groups);
  index_upload_commit();
  if (0 != e) return EXIT_FAILURE;
  if (host_visible) (void)stream_sync(); // operands the CPU addresses directly are done with when the call returns
  return EXIT_SUCCESS;
}

namespace {
void copy_text(const std::string& text, char* buffer, size_t buffer_size)
{ // as much of the text as the caller's buffer holds, terminated
  if (nullptr == buffer || 0 == buffer_size) return;
  const size_t n = (text.size() < buffer_size - 1 ? text.size() : buffer_size - 1);
  memcpy(buffer, text.data(), n); buffer[n] = 0;
}

// Kernel text into the caller's buffer; compile != 0 additionally runs hiprtc for gfx950 (no device needed) and returns its
// result, 2 == compile leaves the text the library builds (hand-wait guard applied) in the buffer. Else: the length of the text.
int emit_source(const std::string& src, char* buffer, size_t buffer_size, int compile)
{
  copy_text(src, buffer, buffer_size);
  if (0 == compile) return (int)src.size();
  std::string log, built;
  const int rc = jit_check_source(src, &log, &built);
  if (0 != rc && 0 != libxsmm_verbosity) fprintf(stderr, "LIBXSMM-AMD: hiprtc: %s\n", log.c_str());
  if (0 == rc && 2 == compile) copy_text(built, buffer, buffer_size);
  return rc;
}
} // namespace

LIBXSMM_API int libxsmm_amd_smm_plan_describe(const libxsmm_gemm_descriptor* descriptor, int mode, int sync, long long batch,
  long long stride_a, long long stride_b, long long stride_c, unsigned int address_bits, int relaxed, long long uniform_run, int mfma, int lowp,
  char* buffer, size_t buffer_size, int compile_tiles)
{ // see include/libxsmm_amd.h
  if (nullptr == descriptor || mode < ADDR_STRIDED || mode > ADDR_POINTER || sync < SYNC_NONE || sync > SYNC_DEVICE || batch < 0) return -1;
  if (0 != lowp && 1 != lowp && 3 != lowp && 4 != lowp) return -1;
  SmmBatch s = from_descriptor(*descriptor);
  if (0 != lowp) { s.typesize = 2; s.lowp = lowp; s.flags &= LIBXSMM_GEMM_FLAG_BETA_0; } // (as lowp_from_descriptor)
  s.mode = mode; s.sync = sync; s.batch = batch; s.sa = stride_a; s.sb = stride_b; s.sc = stride_c;
  s.a = s.b = s.c = reinterpret_cast<void*>(static_cast<uintptr_t>(address_bits)); // (never followed: the planner looks at the low bits only)
  s.index_stride = (int)sizeof(int); s.relaxed = relaxed; s.uniform_run = uniform_run; s.use_mfma = mfma; s.c_atomics = 1;
  int failed = 0;
  const std::string text = smm_plan_describe(s, 0 != compile_tiles, &failed);
  copy_text(text, buffer, buffer_size);
  return 0 != failed ? -2 : (int)text.size();
}

// ---- BLAS-like single GEMM (reference LIBXSMM_XGEMM, include/libxsmm_frontend.h:371-411) ---------------------------
namespace {
template<typename T>
void xgemm(int prec, const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
           const T* alpha, const T* a, const libxsmm_blasint* lda, const T* b, const libxsmm_blasint* ldb, const T* beta, T* c, const libxsmm_blasint* ldc)
{
  if (nullptr == m || nullptr == a || nullptr == b || nullptr == c) return;
  libxsmm_init();
  const int flags = LIBXSMM_GEMM_PFLAGS(transa, transb, LIBXSMM_FLAGS);
  const libxsmm_blasint kk = (nullptr != k ? *k : *m), nn = (nullptr != n ? *n : kk), mm = *m;
  const LeadingDims ld = lds_of(flags, mm, nn, kk, lda, ldb, ldc);
  const libxsmm_blasint ilda = LIBXSMM_MAX((libxsmm_blasint)ld.a, 1), ildb = LIBXSMM_MAX((libxsmm_blasint)ld.b, 1), ildc = LIBXSMM_MAX((libxsmm_blasint)ld.c, 1);
  const T aa = (nullptr != alpha ? *alpha : (T)LIBXSMM_ALPHA), bb = (nullptr != beta ? *beta : (T)LIBXSMM_BETA);
  if (mm <= 0 || nn <= 0) return;
  // opt-in (LIBXSMM_AMD_TGEMM=1): a large product with alpha = 1 and beta in {0, 1} on the tiled matrix-core kernel (xsmm_tgemm.cpp)
  if (tgemm_route((int)sizeof(T), flags, mm, nn, kk, ilda, ildb, ildc, (double)aa, (double)bb, a, b, c)) return;
  libxsmm_descriptor_blob blob;
  const libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_dinit(&blob, (libxsmm_gemm_precision)prec, mm, nn, kk,
    ilda, ildb, ildc, (double)aa, (double)bb, flags, LIBXSMM_GEMM_PREFETCH_NONE);
  const libxsmm_xmmfunction kernel = libxsmm_xmmdispatch(desc);
  if (nullptr != kernel.xmm) { kernel.xmm(a, b, c); return; } // SMM domain (goes through the thunk: recording works)
  SmmBatch s; memset(&s, 0, sizeof(s)); // BLAS domain: alpha/beta/TRANS_A
  s.typesize = (int)sizeof(T); s.m = mm; s.n = nn; s.k = kk; s.lda = ilda; s.ldb = ildb; s.ldc = ildc;
  s.flags = flags & (LIBXSMM_GEMM_FLAG_TRANS_A | LIBXSMM_GEMM_FLAG_TRANS_B);
  s.general = 1; s.alpha = (double)aa; s.beta = (double)bb;
  if (0 >= kk) { s.k = 0; }
  if (!blas_lds_valid("libxsmm_?gemm", s.flags, mm, nn, s.k, ilda, ildb, ildc)) return;
  (void)single_execute(s, a, b, c);
}
} // namespace

#define XSMM_GEMM(API, NAME, T, PREC)                                                                          \
API void NAME(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k, \
  const T* alpha, const T* a, const libxsmm_blasint* lda, const T* b, const libxsmm_blasint* ldb, const T* beta, T* c, const libxsmm_blasint* ldc) \
{ xgemm<T>(PREC, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }
XSMM_GEMM(LIBXSMM_API, libxsmm_dgemm, double, LIBXSMM_GEMM_PRECISION_F64)
XSMM_GEMM(LIBXSMM_API, libxsmm_sgemm, float, LIBXSMM_GEMM_PRECISION_F32)
// libxsmm_blas_?gemm (reference src/libxsmm_gemm.c:703-760): "the BLAS the library falls back to". There is no host BLAS
// behind this engine; the general-form kernel (any alpha/beta/transposes) is that fallback, so these are the same call.
XSMM_GEMM(LIBXSMM_API, libxsmm_blas_dgemm, double, LIBXSMM_GEMM_PRECISION_F64)
XSMM_GEMM(LIBXSMM_API, libxsmm_blas_sgemm, float, LIBXSMM_GEMM_PRECISION_F32)

LIBXSMM_API int libxsmm_amd_smm_kernel_source(const libxsmm_gemm_descriptor* descriptor, int variant, char* buffer, size_t buffer_size, int compile)
{ // the HIP text a dense descriptor is specialised to (reference counterpart: libxsmm_generator_gemm_kernel's noarch
  // text output, src/generator_gemm_noarch.c); compile != 0 additionally runs hiprtc for gfx950 (no device needed).
  // variant: bit 0 = element-wide accesses (index/pointer batches), bit 1 = runs of equal C accumulate in registers
  if (nullptr == descriptor) return -1;
  const libxsmm_gemm_descriptor& d = *descriptor;
  const int ip = LIBXSMM_GETENUM_INP(d.datatype);
  if (LIBXSMM_GEMM_PRECISION_F64 != ip && LIBXSMM_GEMM_PRECISION_F32 != ip) return -1;
  const std::string src = gen_smm_source(LIBXSMM_GEMM_PRECISION_F64 == ip ? 8 : 4, (int)d.m, (int)d.n, (int)d.k, d.flags, variant & 0x1FFFF, (int)d.lda, (int)d.ldb, (int)d.ldc);
  return emit_source(src, buffer, buffer_size, compile);
}

LIBXSMM_API int libxsmm_amd_smm_grouped_kernel_source(const libxsmm_gemm_descriptor* const descriptors[], int ndescriptors, char* buffer, size_t buffer_size, int compile)
{ // the HIP text one grouped launch (libxsmm_amd_gemm_batch_groups) of index batches with these descriptors compiles: the run
  // forms of every shape behind one dispatcher; same buffer/compile/return conventions as libxsmm_amd_smm_kernel_source
  if (nullptr == descriptors || ndescriptors < 1) return -1;
  std::vector<SmmBatch> groups;
  for (int i = 0; i < ndescriptors; ++i) {
    if (nullptr == descriptors[i]) return -1;
    const int ip = LIBXSMM_GETENUM_INP(descriptors[i]->datatype);
    if (LIBXSMM_GEMM_PRECISION_F64 != ip && LIBXSMM_GEMM_PRECISION_F32 != ip) return -1;
    SmmBatch s = from_descriptor(*descriptors[i]);
    s.mode = ADDR_INDEX; s.batch = 1 << 20; s.sync = SYNC_DEVICE;
    groups.push_back(s);
  }
  const std::string src = gen_smm_grouped_source_for(groups.data(), (int)groups.size());
  if (src.empty()) return -1;
  return emit_source(src, buffer, buffer_size, compile);
}

LIBXSMM_API int libxsmm_amd_jit_prebuild(const libxsmm_gemm_descriptor* const descriptors[], int ndescriptors, int grouped)
{ // see include/libxsmm_amd.h
  if (nullptr == descriptors || ndescriptors < 1) return -1;
  std::vector<SmmBatch> shapes;
  for (int i = 0; i < ndescriptors; ++i) {
    if (nullptr == descriptors[i]) return -1;
    const int ip = LIBXSMM_GETENUM_INP(descriptors[i]->datatype), op = LIBXSMM_GETENUM_OUT(descriptors[i]->datatype);
    if (ip != op || (LIBXSMM_GEMM_PRECISION_F64 != ip && LIBXSMM_GEMM_PRECISION_F32 != ip)) continue;
    shapes.push_back(from_descriptor(*descriptors[i]));
  }
  if (shapes.empty()) return 0;
  int built = 0;
  const int failed = smm_jit_prebuild(shapes.data(), (int)shapes.size(), grouped, &built);
  return 0 == failed ? built : -failed;
}

LIBXSMM_API void libxsmm_amd_jit_wait(void) { jit_async_wait(); }
LIBXSMM_API void libxsmm_amd_jit_drain(void) { jit_async_drain(); }

// ---- measurement aid -----------------------------------------------------------------------------------------------
namespace xsmm { int launch_stream_abc(const void* a, const void* b, void* c, long long bytes, void* stream); }

LIBXSMM_API int libxsmm_amd_stream_probe(const void* a, const void* b, void* c, long long bytes)
{ // c += a + b over `bytes` bytes per operand (device memory, 16-byte aligned, a multiple of 4 KiB): pure
  // 3-read/1-write streaming
  if (nullptr == a || nullptr == b || nullptr == c || bytes < 0 || 0 != (bytes % 4096)) return EXIT_FAILURE;
  if (!device_ready()) { fail_no_device("libxsmm_amd_stream_probe"); return EXIT_FAILURE; }
  const int e = xsmm::launch_stream_abc(a, b, c, bytes, device().stream);
  note_launch("stream_abc");
  return 0 == e ? EXIT_SUCCESS : EXIT_FAILURE;
}

// ---- BLAS call wrapper (reference src/libxsmm_ext_gemm.c:256-660, documentation/libxsmm_mm.md "Call Wrapper") ------------
// An application that calls the Fortran BLAS symbols is relinked with -Wl,--wrap=dgemm_,--wrap=sgemm_ (and optionally
// --wrap=dgemm_batch_,--wrap=sgemm_batch_,--wrap=dgemm_batch,--wrap=sgemm_batch): its calls then arrive here. The
// reference decides per call between its SMM kernels and the original BLAS (__real_?gemm_); here every call is served
// by the device path (general alpha/beta/transposes included), so no __real_ symbol -- no BLAS library -- is needed.
// Inside libxsmm_mmbatch_begin/end the calls are recorded and executed as one batch, as in the reference.
extern "C" {
XSMM_GEMM(LIBXSMM_APIEXT, __wrap_dgemm_, double, LIBXSMM_GEMM_PRECISION_F64) // (what libxsmm_dgemm / libxsmm_sgemm do)
XSMM_GEMM(LIBXSMM_APIEXT, __wrap_sgemm_, float, LIBXSMM_GEMM_PRECISION_F32)

// (what libxsmm_dgemm_batch_omp / libxsmm_sgemm_batch_omp do)
XSMM_GROUP_BATCH(__wrap_dgemm_batch_, double, LIBXSMM_GEMM_PRECISION_F64, libxsmm_gemm_batch_omp, true)
XSMM_GROUP_BATCH(__wrap_sgemm_batch_, float, LIBXSMM_GEMM_PRECISION_F32, libxsmm_gemm_batch_omp, true)
XSMM_GROUP_BATCH(__wrap_dgemm_batch, double, LIBXSMM_GEMM_PRECISION_F64, libxsmm_gemm_batch_omp, true)
XSMM_GROUP_BATCH(__wrap_sgemm_batch, float, LIBXSMM_GEMM_PRECISION_F32, libxsmm_gemm_batch_omp, true)
}
