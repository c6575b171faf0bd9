// xsmm_lowp_gemm.cpp -- GEMM for 16-bit inputs: the reference's front ends libxsmm_wigemm / libxsmm_wsgemm / libxsmm_bsgemm
// and the one-layout entry libxsmm_amd_lowp_gemm / _thread behind them (kernels/tgemm_lowp.hip).
//
// Reference: src/libxsmm_gemm.c:1265-1320 expands LIBXSMM_XGEMM (include/libxsmm_frontend.h:371-411) for each front end: a
// product within LIBXSMM_MAX_MNK goes to the dispatched kernel, everything else to LIBXSMM_INLINE_XGEMM (:213-245). The
// first half is reproduced as it is (the dispatched kernel reads A in pairs of k); the second is not a contract -- it is NN
// only, multiplies bf16 bit patterns as integers and with beta = 0 keeps only the last k term -- so the GEMM it stands for
// is computed instead: plain column-major operands, all four transposes, the arithmetic of the dispatched kernels.
// A task is one launch over its rectangle of C; the memory rules and the behaviour inside the defer bracket are those of
// the tiled GEMM (xsmm_tgemm.cpp): memory the GPU reaches is processed in place, host-visible memory is complete on return,
// pageable memory is staged, the call seals an open burst and is not recorded.
#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"

#include <atomic>
#include <cstring>

using namespace xsmm;

namespace {

std::atomic<int>& fast_mode()
{
  static std::atomic<int> mode([]() { const char* const e = getenv("LIBXSMM_AMD_LOWP_FAST"); return (nullptr != e && 0 != atoi(e)) ? 1 : 0; }());
  return mode;
}

struct Problem {
  int kind;               // LowpGemmKind (LOWP_BF16 here: the mode is looked up at launch)
  bool ta, tb; int beta0;
  long long m, n, k, lda, ldb, ldc;
};

// every argument error, before any device probe
bool problem_fill(Problem* p, int iprec, int oprec, char transa, char transb, long long m, long long n, long long k,
  const void* a, long long lda, const void* b, long long ldb, int beta, const void* c, long long ldc)
{
  if (LIBXSMM_GEMM_PRECISION_I16 == iprec && LIBXSMM_GEMM_PRECISION_I32 == oprec) p->kind = LOWP_I16_I32;
  else if (LIBXSMM_GEMM_PRECISION_I16 == iprec && LIBXSMM_GEMM_PRECISION_F32 == oprec) p->kind = LOWP_I16_F32;
  else if (LIBXSMM_GEMM_PRECISION_BF16 == iprec && LIBXSMM_GEMM_PRECISION_F32 == oprec) p->kind = LOWP_BF16;
  else return false;
  if ('N' != transa && 'n' != transa && 'T' != transa && 't' != transa) return false;
  if ('N' != transb && 'n' != transb && 'T' != transb && 't' != transb) return false;
  p->ta = ('T' == transa || 't' == transa); p->tb = ('T' == transb || 't' == transb);
  if (0 != beta && 1 != beta) return false;
  p->beta0 = (0 == beta ? 1 : 0);
  if (m < 0 || n < 0 || k < 0 || m > 0x7fffffffLL || n > 0x7fffffffLL || k > 0x7fffffffLL) return false;
  if (nullptr == a || nullptr == b || nullptr == c) return false;
  if (lda < (p->ta ? k : m) || ldb < (p->tb ? n : k) || ldc < m || lda < 1 || ldb < 1 || ldc < 1) return false;
  p->m = m; p->n = n; p->k = k; p->lda = lda; p->ldb = ldb; p->ldc = ldc;
  return true;
}

// one rectangle of C through kernels/tgemm_lowp.hip: 2-byte inputs, 4-byte C
int run_problem(const Problem& h, const unsigned int rect[4], const void* a, const void* b, void* c, const char* what)
{
  return run_rect(2, 4, h.ta, h.tb, h.beta0, h.k, h.lda, h.ldb, h.ldc, rect, a, b, c,
    [&](void* stream, const void* da, const void* db, void* dc, long long ldc, int m, int n, const char** name) {
      TgemmLowpArgs g; memset(&g, 0, sizeof(g));
      g.kind = (LOWP_BF16 == h.kind && 0 != fast_mode().load()) ? LOWP_BF16_FAST : h.kind;
      g.transa = h.ta ? 1 : 0; g.transb = h.tb ? 1 : 0; g.beta0 = h.beta0;
      g.m = m; g.n = n; g.k = (int)h.k; g.lda = h.lda; g.ldb = h.ldb; g.ldc = ldc;
      g.a = da; g.b = db; g.c = dc;
      return launch_tgemm_lowp(g, stream, name);
    }, what);
}

// the rectangle of task tid: the partition rule of libxsmm_amd_gemm_task, asked of a handle with the extents of this C
bool task_rect(const Problem& p, int tid, int nthreads, unsigned int rect[4])
{
  const libxsmm_blasint m = (libxsmm_blasint)p.m, n = (libxsmm_blasint)p.n, one = 1;
  libxsmm_gemm_blob blob;
  const libxsmm_gemm_handle* const handle = libxsmm_gemm_handle_init(&blob, LIBXSMM_GEMM_PRECISION_F32, LIBXSMM_GEMM_PRECISION_F32, "N", "N",
    &m, &n, &one, nullptr, nullptr, nullptr, nullptr, nullptr, LIBXSMM_GEMM_HANDLE_FLAG_AUTO, 1);
  if (nullptr == handle || EXIT_SUCCESS != libxsmm_amd_gemm_task(handle, tid, nthreads, rect)) return false;
  return rect[0] < rect[1] && rect[2] < rect[3];
}

// LIBXSMM_XGEMM (include/libxsmm_frontend.h:371-411) for a 16-bit input type: IT is short or libxsmm_bfloat16, OT int or float
template<typename IT, typename OT, typename FN>
void front_end(int iprec, int oprec, FN dispatch, const char* what, const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k, const OT* alpha, const IT* a, const libxsmm_blasint* lda,
  const IT* b, const libxsmm_blasint* ldb, const OT* beta, OT* c, const libxsmm_blasint* ldc)
{
  static int error_once = 0;
  if (nullptr == m || nullptr == a || nullptr == b || nullptr == c) {
    if (0 != libxsmm_verbosity && once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: %s: invalid arguments!\n", what);
    return;
  }
  const int flags = LIBXSMM_GEMM_PFLAGS(transa, transb, LIBXSMM_FLAGS) & (LIBXSMM_GEMM_FLAG_TRANS_A | LIBXSMM_GEMM_FLAG_TRANS_B);
  const bool ta = (0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_A)), tb = (0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_B));
  const libxsmm_blasint mm = *m, kk = (nullptr != k ? *k : mm), nn = (nullptr != n ? *n : kk); // (:373-374)
  libxsmm_blasint ilda = (nullptr != lda ? *lda : (ta ? kk : mm)), ildb = (nullptr != ldb ? *ldb : (tb ? nn : kk)), ildc = (nullptr != ldc ? *ldc : mm);
  if (ilda < 1) ilda = 1;
  if (ildb < 1) ildb = 1;
  if (ildc < 1) ildc = 1; // (:375-379)
  const OT aa = (nullptr != alpha ? *alpha : (OT)LIBXSMM_ALPHA), bb = (nullptr != beta ? *beta : (OT)LIBXSMM_BETA);
  if ((OT)1 != aa || ((OT)0 != bb && (OT)1 != bb)) { // no low-precision kernel of the reference takes anything else: C stays as it is
    static int scalar_once = 0;
    if (0 != libxsmm_verbosity && once(&scalar_once)) fprintf(stderr, "LIBXSMM ERROR: %s: alpha must be 1 and beta 0 or 1; C is left untouched!\n", what);
    return;
  }
  if (LIBXSMM_SMM(mm, nn, kk, 2 /*RFO*/, sizeof(OT))) { // (:380-387) the dispatched kernel, which reads A in pairs of k
    const auto kernel = dispatch(mm, nn, kk, &ilda, &ildb, &ildc, &aa, &bb, &flags, nullptr);
    if (nullptr != kernel) {
      // i16 -> f32: the kernel takes its scaling factor as the 7th argument. The reference's LIBXSMM_MMCALL_LDX passes
      // none and the kernel reads an indeterminate word; 1 is what a caller of libxsmm_wsgemm can mean.
      static const float one = 1.f;
      if (LIBXSMM_GEMM_PRECISION_I16 == iprec && LIBXSMM_GEMM_PRECISION_F32 == oprec) kernel(a, b, c, nullptr, nullptr, nullptr, &one);
      else kernel(a, b, c);
      return;
    }
  }
  (void)libxsmm_amd_lowp_gemm((libxsmm_gemm_precision)iprec, (libxsmm_gemm_precision)oprec, ta ? 'T' : 'N', tb ? 'T' : 'N', mm, nn, kk,
    a, ilda, b, ildb, (OT)0 == bb ? 0 : 1, c, ildc);
}

} // namespace

LIBXSMM_API int libxsmm_amd_set_lowp_fast(int on) { return fast_mode().exchange(0 != on ? 1 : 0); }
LIBXSMM_API int libxsmm_amd_get_lowp_fast(void) { return fast_mode().load(); }

LIBXSMM_API int libxsmm_amd_lowp_gemm_chunk(libxsmm_gemm_precision iprec)
{
  return LIBXSMM_GEMM_PRECISION_BF16 == iprec ? TGEMM_LOWP_BK : (LIBXSMM_GEMM_PRECISION_I16 == iprec ? TGEMM_LOWP_BK / 2 : 0);
}

LIBXSMM_API int libxsmm_amd_lowp_gemm_thread(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, char transa, char transb,
  libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k, const void* a, libxsmm_blasint lda, const void* b, libxsmm_blasint ldb,
  int beta, void* c, libxsmm_blasint ldc, int tid, int nthreads)
{ // see include/libxsmm_amd.h
  Problem p;
  if (!problem_fill(&p, (int)iprec, (int)oprec, transa, transb, m, n, k, a, lda, b, ldb, beta, c, ldc)) return EXIT_FAILURE;
  if (nthreads < 1 || tid < 0 || tid >= nthreads) return EXIT_FAILURE;
  if (0 == m || 0 == n || 0 == k) return EXIT_SUCCESS;
  unsigned int rect[4];
  if (!task_rect(p, tid, nthreads, rect)) return EXIT_SUCCESS; // a task without work
  return run_problem(p, rect, a, b, c, "libxsmm_amd_lowp_gemm");
}

LIBXSMM_API int libxsmm_amd_lowp_gemm(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, char transa, char transb,
  libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k, const void* a, libxsmm_blasint lda, const void* b, libxsmm_blasint ldb,
  int beta, void* c, libxsmm_blasint ldc)
{ return libxsmm_amd_lowp_gemm_thread(iprec, oprec, transa, transb, m, n, k, a, lda, b, ldb, beta, c, ldc, 0, 1); }

LIBXSMM_API void libxsmm_wigemm(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const int* alpha, const short* a, const libxsmm_blasint* lda, const short* b, const libxsmm_blasint* ldb, const int* beta, int* c, const libxsmm_blasint* ldc)
{ front_end<short, int>(LIBXSMM_GEMM_PRECISION_I16, LIBXSMM_GEMM_PRECISION_I32, libxsmm_wimmdispatch, "libxsmm_wigemm", transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

LIBXSMM_API void libxsmm_wsgemm(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const float* alpha, const short* a, const libxsmm_blasint* lda, const short* b, const libxsmm_blasint* ldb, const float* beta, float* c, const libxsmm_blasint* ldc)
{ front_end<short, float>(LIBXSMM_GEMM_PRECISION_I16, LIBXSMM_GEMM_PRECISION_F32, libxsmm_wsmmdispatch, "libxsmm_wsgemm", transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

LIBXSMM_API void libxsmm_bsgemm(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const float* alpha, const libxsmm_bfloat16* a, const libxsmm_blasint* lda, const libxsmm_bfloat16* b, const libxsmm_blasint* ldb, const float* beta, float* c, const libxsmm_blasint* ldc)
{ front_end<libxsmm_bfloat16, float>(LIBXSMM_GEMM_PRECISION_BF16, LIBXSMM_GEMM_PRECISION_F32, libxsmm_bsmmdispatch, "libxsmm_bsgemm", transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }
