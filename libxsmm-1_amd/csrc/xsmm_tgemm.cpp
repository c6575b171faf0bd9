// xsmm_tgemm.cpp -- the tiled GEMM: libxsmm_gemm_handle_init / _get_scratch_size, libxsmm_gemm_thread, libxsmm_xgemm_omp and
// the partition query libxsmm_amd_gemm_task.
//
// Reference: src/libxsmm_gemm.c:790-1228 (handle and task) and src/libxsmm_ext_gemm.c:666-755 (the OpenMP driver). There a
// task walks tiles of C with JIT-generated SMM kernels -- the beta kernel on the first k-chunk, the beta = 1 kernel
// afterwards (:1158-1201) -- after copying (and transposing) tiles into scratch. Here a task is one launch of
// kernels/tgemm.hip over its rectangle of C: the operands are re-laid on their way into LDS, so no scratch is
// needed, and k is never split (the reference's kt > 1 path is unsynchronised, :1202). The handle is plain data in the
// caller's blob. Arguments are checked before any device probe; the memory rules are those of the other entry points:
// memory the GPU reaches is processed in place, host-visible memory is complete on return, pageable memory is staged.
#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

struct libxsmm_gemm_handle {
  unsigned int magic;
  int typesize;           // 8: F64, 4: F32
  int gemm_flags;         // LIBXSMM_GEMM_FLAG_TRANS_A | _TRANS_B | _BETA_0
  int flags;              // libxsmm_gemm_handle_flags as given (the operands are re-laid inside the kernel whatever they say)
  int m, n, k;
  int lda, ldb, ldc;
  int ntasks;
};
static_assert(sizeof(libxsmm_gemm_handle) <= sizeof(libxsmm_gemm_blob), "the handle lives in the caller's blob");

namespace {

constexpr unsigned int HANDLE_MAGIC = 0x74474d4du;

void complain(int* flag, const char* msg)
{
  if (0 != libxsmm_verbosity && once(flag)) fprintf(stderr, "LIBXSMM ERROR: %s\n", msg);
}

bool value_of(int prec, const void* p, double dflt, double* out)
{
  if (nullptr == p) { *out = dflt; return true; }
  if (LIBXSMM_GEMM_PRECISION_F64 == prec) { *out = *static_cast<const double*>(p); return true; }
  if (LIBXSMM_GEMM_PRECISION_F32 == prec) { *out = (double)*static_cast<const float*>(p); return true; }
  return false;
}

// The rectangle of task tid: the tiles of C (TGEMM_TILE x TGEMM_TILE) form a grid that is cut into mt x nt parts with
// mt * nt <= nthreads as large as the grid allows; tasks beyond mt * nt have no work.
bool task_rect(const libxsmm_gemm_handle& h, int tid, int nthreads, unsigned int rect[4])
{
  const long long tm = ((long long)h.m + TGEMM_TILE - 1) / TGEMM_TILE, tn = ((long long)h.n + TGEMM_TILE - 1) / TGEMM_TILE;
  long long mt = 1, nt = 1;
  for (long long j = 1; j <= tn && j <= nthreads; ++j) {
    long long i = nthreads / j;
    if (i > tm) i = tm;
    if (i * j > mt * nt || (i * j == mt * nt && (i > j ? i - j : j - i) < (mt > nt ? mt - nt : nt - mt))) { mt = i; nt = j; }
  }
  rect[0] = rect[1] = rect[2] = rect[3] = 0;
  if (tid >= mt * nt) return false;
  const long long im = tid % mt, in = tid / mt;
  long long m0 = tm * im / mt * TGEMM_TILE, m1 = tm * (im + 1) / mt * TGEMM_TILE;
  long long n0 = tn * in / nt * TGEMM_TILE, n1 = tn * (in + 1) / nt * TGEMM_TILE;
  if (m1 > h.m) m1 = h.m;
  if (n1 > h.n) n1 = h.n;
  rect[0] = (unsigned int)m0; rect[1] = (unsigned int)m1; rect[2] = (unsigned int)n0; rect[3] = (unsigned int)n1;
  return m0 < m1 && n0 < n1;
}

} // namespace

int xsmm::run_rect(size_t ti, size_t to, bool ta, bool tb, int beta0, long long k, long long lda, long long ldb, long long ldc,
  const unsigned int rect[4], const void* a, const void* b, void* c, const RectLaunch& launch, const char* what)
{
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  const hipStream_t st = (hipStream_t)stream;
  const size_t m0 = rect[0], n0 = rect[2];
  const int m = (int)(rect[1] - rect[0]), n = (int)(rect[3] - rect[2]);
  // what the rectangle reads and writes: rows m0 ... of op(A), columns n0 ... of op(B)
  const char* pa = static_cast<const char*>(a) + (ta ? m0 * (size_t)lda : m0) * ti;
  const char* pb = static_cast<const char*>(b) + (tb ? n0 : n0 * (size_t)ldb) * ti;
  char* const pc = static_cast<char*>(c) + (n0 * (size_t)ldc + m0) * to;
  const int ka = pointer_kind(pa), kb = pointer_kind(pb), kc = pointer_kind(pc);
  const bool visible = (0 != ((ka | kb | kc) & 2));
  bool staged = false;
  if (0 == (ka & 1)) { // the span of A the task reads, as it lies
    const size_t nbytes = (ta ? ((size_t)(m - 1) * lda + k) : ((size_t)(k - 1) * lda + m)) * ti;
    void* const p = scratch(3, nbytes);
    if (nullptr == p || 0 != h2d(p, pa, nbytes)) return EXIT_FAILURE;
    pa = static_cast<const char*>(p); staged = true;
  }
  if (0 == (kb & 1)) {
    const size_t nbytes = (tb ? ((size_t)(k - 1) * ldb + n) : ((size_t)(n - 1) * ldb + k)) * ti;
    void* const p = scratch(4, nbytes);
    if (nullptr == p || 0 != h2d(p, pb, nbytes)) return EXIT_FAILURE;
    pb = static_cast<const char*>(p); staged = true;
  }
  char* dc = pc;
  long long dldc = ldc;
  const size_t tight = (size_t)m * to; // bytes of a column of the rectangle
  if (0 == (kc & 1)) { // a tight image of the rectangle: only the rectangle travels, what lies between m and ldc keeps its bytes
    dc = static_cast<char*>(scratch(5, tight * n));
    if (nullptr == dc) return EXIT_FAILURE;
    dldc = m;
    if (0 == beta0 && hipSuccess != hipMemcpy2DAsync(dc, tight, pc, (size_t)ldc * to, tight, (size_t)n, hipMemcpyHostToDevice, st)) {
      (void)hipGetLastError(); return EXIT_FAILURE;
    }
  }
  const char* name = "";
  const int e = launch(stream, pa, pb, dc, dldc, m, n, &name);
  note_launch(name);
  if (0 != e) { fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e); return EXIT_FAILURE; }
  if (dc != pc) {
    if (hipSuccess != hipMemcpy2DAsync(pc, (size_t)ldc * to, dc, tight, tight, (size_t)n, hipMemcpyDeviceToHost, st)) { (void)hipGetLastError(); return EXIT_FAILURE; }
    return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  if (staged || visible) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

namespace {

// one rectangle of C through kernels/tgemm.hip
int run_handle(const libxsmm_gemm_handle& h, const unsigned int rect[4], const void* a, const void* b, void* c, const char* what)
{
  const bool ta = (0 != (h.gemm_flags & LIBXSMM_GEMM_FLAG_TRANS_A)), tb = (0 != (h.gemm_flags & LIBXSMM_GEMM_FLAG_TRANS_B));
  const int beta0 = (0 != (h.gemm_flags & LIBXSMM_GEMM_FLAG_BETA_0)) ? 1 : 0;
  return run_rect((size_t)h.typesize, (size_t)h.typesize, ta, tb, beta0, h.k, h.lda, h.ldb, h.ldc, rect, a, b, c,
    [&](void* stream, const void* da, const void* db, void* dc, long long ldc, int m, int n, const char** name) {
      TgemmArgs g; memset(&g, 0, sizeof(g));
      g.typesize = h.typesize; g.transa = ta ? 1 : 0; g.transb = tb ? 1 : 0; g.beta0 = beta0;
      g.m = m; g.n = n; g.k = h.k; g.lda = h.lda; g.ldb = h.ldb; g.ldc = ldc;
      g.a = da; g.b = db; g.c = dc;
      return launch_tgemm(g, stream, name);
    }, what);
}

bool handle_fill(libxsmm_gemm_handle* h, int iprec, int oprec, const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const libxsmm_blasint* lda, const libxsmm_blasint* ldb, const libxsmm_blasint* ldc, const void* alpha, const void* beta, int flags, int ntasks)
{
  if (nullptr == m || ntasks < 1) return false;
  if (iprec != oprec || (LIBXSMM_GEMM_PRECISION_F64 != iprec && LIBXSMM_GEMM_PRECISION_F32 != iprec)) return false;
  double dalpha = 1, dbeta = 1;
  if (!value_of(iprec, alpha, LIBXSMM_ALPHA, &dalpha) || !value_of(oprec, beta, LIBXSMM_BETA, &dbeta)) return false;
  if (1.0 != dalpha || (0.0 != dbeta && 1.0 != dbeta)) return false; // the reference's descriptor rule (src/libxsmm_gemm.c:978-992)
  const int gemm_flags = LIBXSMM_GEMM_PFLAGS(transa, transb, LIBXSMM_FLAGS) & (LIBXSMM_GEMM_FLAG_TRANS_A | LIBXSMM_GEMM_FLAG_TRANS_B);
  const long long mm = *m, kk = (nullptr != k ? *k : mm), nn = (nullptr != n ? *n : kk); // (:820)
  if (mm < 1 || nn < 1 || kk < 1) return false;
  const bool ta = (0 != (gemm_flags & LIBXSMM_GEMM_FLAG_TRANS_A)), tb = (0 != (gemm_flags & LIBXSMM_GEMM_FLAG_TRANS_B));
  const long long ilda = (nullptr != lda ? *lda : (ta ? kk : mm)), ildb = (nullptr != ldb ? *ldb : (tb ? nn : kk)), ildc = (nullptr != ldc ? *ldc : mm); // (:888-890)
  if (ilda < (ta ? kk : mm) || ildb < (tb ? nn : kk) || ildc < mm) return false;
  memset(h, 0, sizeof(*h));
  h->magic = HANDLE_MAGIC; h->typesize = (LIBXSMM_GEMM_PRECISION_F64 == iprec ? 8 : 4);
  h->gemm_flags = gemm_flags | (0.0 == dbeta ? LIBXSMM_GEMM_FLAG_BETA_0 : 0);
  h->flags = flags; h->m = (int)mm; h->n = (int)nn; h->k = (int)kk; h->lda = (int)ilda; h->ldb = (int)ildb; h->ldc = (int)ildc; h->ntasks = ntasks;
  return true;
}

bool handle_valid(const libxsmm_gemm_handle* h) { return nullptr != h && HANDLE_MAGIC == h->magic; }

} // namespace

namespace xsmm {

bool tgemm_route(int typesize, int flags, int m, int n, int k, int lda, int ldb, int ldc, double alpha, double beta, const void* a, const void* b, void* c)
{
  static const bool enabled = []() { const char* const e = getenv("LIBXSMM_AMD_TGEMM"); return nullptr != e && 0 != atoi(e); }();
  if (!enabled || 1.0 != alpha || (0.0 != beta && 1.0 != beta)) return false;
  // large: where a single product leaves the SMM kernels today (xsmm_call.cpp: single_execute)
  if (!(2.0 * m * n * k >= 2.0 * 256 * 256 * 256 && m >= 64 && n >= 64 && k >= 32)) return false;
  const bool ta = (0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_A)), tb = (0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_B));
  if (lda < (ta ? k : m) || ldb < (tb ? n : k) || ldc < m) return false;
  libxsmm_gemm_handle h; memset(&h, 0, sizeof(h));
  h.magic = HANDLE_MAGIC; h.typesize = typesize; h.gemm_flags = (flags & (LIBXSMM_GEMM_FLAG_TRANS_A | LIBXSMM_GEMM_FLAG_TRANS_B)) | (0.0 == beta ? LIBXSMM_GEMM_FLAG_BETA_0 : 0);
  h.m = m; h.n = n; h.k = k; h.lda = lda; h.ldb = ldb; h.ldc = ldc; h.ntasks = 1;
  const unsigned int rect[4] = { 0, (unsigned int)m, 0, (unsigned int)n };
  (void)run_handle(h, rect, a, b, c, "libxsmm_?gemm");
  return true;
}

} // namespace xsmm

LIBXSMM_API libxsmm_gemm_handle* libxsmm_gemm_handle_init(libxsmm_gemm_blob* blob, libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec,
  const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const libxsmm_blasint* lda, const libxsmm_blasint* ldb, const libxsmm_blasint* ldc, const void* alpha, const void* beta, int flags, int ntasks)
{ // src/libxsmm_gemm.c:790-1048 (no device is asked for: a handle can be made anywhere)
  if (nullptr == blob) return nullptr;
  libxsmm_gemm_handle h;
  if (!handle_fill(&h, (int)iprec, (int)oprec, transa, transb, m, n, k, lda, ldb, ldc, alpha, beta, flags, ntasks)) return nullptr;
  memcpy(blob->data, &h, sizeof(h));
  return reinterpret_cast<libxsmm_gemm_handle*>(blob->data);
}

LIBXSMM_API size_t libxsmm_gemm_handle_get_scratch_size(const libxsmm_gemm_handle* handle)
{ // src/libxsmm_gemm.c:1051-1064: the reference's tile copies need scratch; the kernel here re-lays the operands in LDS
  (void)handle;
  return 0;
}

LIBXSMM_API int libxsmm_amd_gemm_task(const libxsmm_gemm_handle* handle, int tid, int nthreads, unsigned int rect[4])
{ // see include/libxsmm_amd.h
  if (nullptr == rect) return EXIT_FAILURE;
  rect[0] = rect[1] = rect[2] = rect[3] = 0;
  if (!handle_valid(handle) || nthreads < 1 || tid < 0 || tid >= nthreads) return EXIT_FAILURE;
  (void)task_rect(*handle, tid, nthreads, rect);
  return EXIT_SUCCESS;
}

LIBXSMM_API int libxsmm_amd_gemm_tile(void) { return TGEMM_TILE; }

LIBXSMM_API void libxsmm_gemm_thread(const libxsmm_gemm_handle* handle, void* scratch, const void* a, const void* b, void* c, int tid, int nthreads)
{ // src/libxsmm_gemm.c:1067-1228
  static int error_once = 0;
  (void)scratch;
  if (!handle_valid(handle) || nthreads < 1 || tid < 0 || tid >= nthreads) {
    complain(&error_once, "libxsmm_gemm_thread: invalid handle, thread-id or number of threads!");
    return;
  }
  if (nullptr == a || nullptr == b || nullptr == c) { complain(&error_once, "libxsmm_gemm_thread: an operand is NULL!"); return; }
  unsigned int rect[4];
  if (!task_rect(*handle, tid, nthreads, rect)) return; // a task without work
  (void)run_handle(*handle, rect, a, b, c, "libxsmm_gemm_thread");
}

LIBXSMM_APIEXT void libxsmm_xgemm_omp(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k, const void* alpha, const void* a, const libxsmm_blasint* lda,
  const void* b, const libxsmm_blasint* ldb, const void* beta, void* c, const libxsmm_blasint* ldc)
{ // src/libxsmm_ext_gemm.c:666-755 (the reference spreads tasks over OpenMP threads; one launch covers C here)
  static int error_once = 0;
  libxsmm_gemm_blob blob;
  const libxsmm_gemm_handle* const handle = libxsmm_gemm_handle_init(&blob, iprec, oprec, transa, transb, m, n, k, lda, ldb, ldc, alpha, beta,
    LIBXSMM_GEMM_HANDLE_FLAG_AUTO, 1);
  if (nullptr != handle) { libxsmm_gemm_thread(handle, nullptr, a, b, c, 0, 1); return; }
  // outside the handle's domain: the path of libxsmm_blas_?gemm, as the reference falls back to BLAS (:739-753)
  if (LIBXSMM_GEMM_PRECISION_F64 == iprec && LIBXSMM_GEMM_PRECISION_F64 == oprec) {
    libxsmm_blas_dgemm(transa, transb, m, n, k, static_cast<const double*>(alpha), static_cast<const double*>(a), lda,
      static_cast<const double*>(b), ldb, static_cast<const double*>(beta), static_cast<double*>(c), ldc);
  }
  else if (LIBXSMM_GEMM_PRECISION_F32 == iprec && LIBXSMM_GEMM_PRECISION_F32 == oprec) {
    libxsmm_blas_sgemm(transa, transb, m, n, k, static_cast<const float*>(alpha), static_cast<const float*>(a), lda,
      static_cast<const float*>(b), ldb, static_cast<const float*>(beta), static_cast<float*>(c), ldc);
  }
  else complain(&error_once, "libxsmm_xgemm_omp: unsupported precision!");
}
