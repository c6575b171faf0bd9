// xsmm_call.cpp -- what a kernel thunk does when user code calls the bare function pointer (call_kernel, for every kernel
// class), and the single products behind it: one operand triple wherever it lives (single_execute, lowp_single_execute).
// (The reference's JIT kernels are called as kernel(a, b, c, ...); here the thunk of xsmm_main.cpp lands in call_kernel.)
#include "xsmm_internal.hpp"

#include <cstring>

namespace xsmm {

SmmBatch from_descriptor(const libxsmm_gemm_descriptor& d)
{
  SmmBatch s; memset(&s, 0, sizeof(s));
  s.typesize = (LIBXSMM_GEMM_PRECISION_F64 == LIBXSMM_GETENUM_INP(d.datatype)) ? 8 : 4;
  s.m = (int)d.m; s.n = (int)d.n; s.k = (int)d.k; s.lda = (int)d.lda; s.ldb = (int)d.ldb; s.ldc = (int)d.ldc;
  s.flags = d.flags & (LIBXSMM_GEMM_FLAG_TRANS_B | LIBXSMM_GEMM_FLAG_BETA_0);
  s.use_mfma = libxsmm_amd_get_mfma();
  s.alpha = 1.0; s.beta = (0 != (d.flags & LIBXSMM_GEMM_FLAG_BETA_0)) ? 0.0 : 1.0;
  return s;
}

// One product of a low-precision kernel, or a batch of them with independent C operands (device-reachable operands).
SmmBatch lowp_from_descriptor(const libxsmm_gemm_descriptor& d, float scf)
{
  SmmBatch s; memset(&s, 0, sizeof(s));
  const int ip = LIBXSMM_GETENUM_INP(d.datatype), op = LIBXSMM_GETENUM_OUT(d.datatype);
  s.lowp = (LIBXSMM_GEMM_PRECISION_I16 == ip) ? (LIBXSMM_GEMM_PRECISION_I32 == op ? 1 : 2) : (LIBXSMM_GEMM_PRECISION_F32 == op ? 3 : 4);
  s.scf = scf; s.typesize = 2;
  s.m = (int)d.m; s.n = (int)d.n; s.k = (int)d.k; s.lda = (int)d.lda; s.ldb = (int)d.ldb; s.ldc = (int)d.ldc;
  s.flags = d.flags & LIBXSMM_GEMM_FLAG_BETA_0;
  s.use_mfma = libxsmm_amd_get_mfma();
  return s;
}

int lowp_launch(const SmmBatch& s)
{
  const char* name = "";
  int e = launch_smm_jit(s, device().stream, &name); // large strided batches of small tight items: specialised streaming form
  if (e < 0) e = launch_smm_lowp(s, device().stream, &name);
  note_launch(name);
  if (0 != e) launch_failed(name, e);
  return e;
}

namespace {
// One launch over operands the GPU does not reach: the three spans (a NULL one is left out) travel through scratch, C comes
// back. launch receives the device copies and returns 0 if the kernel was queued.
template<typename Launch>
int staged_call(const void* a, size_t bytes_a, const void* b, size_t bytes_b, void* c, size_t bytes_c, Launch launch)
{
  const void* const host[3] = { a, b, c }; const size_t bytes[3] = { bytes_a, bytes_b, bytes_c };
  char* dev[3];
  if (!stage_in(host, bytes, dev)) return EXIT_FAILURE;
  if (0 != launch(dev[0], dev[1], dev[2])) return EXIT_FAILURE;
  return 0 == stage_out(c, dev[2], bytes_c) ? EXIT_SUCCESS : EXIT_FAILURE;
}

int lowp_single_execute(SmmBatch s, const void* a, const void* b, void* c)
{
  if (!device_ready()) { fail_no_device("a dispatched low-precision kernel"); return EXIT_FAILURE; }
  s.mode = ADDR_STRIDED; s.batch = 1; s.sync = SYNC_NONE;
  const Residency where = classify(a, b, c);
  if (where.device()) {
    s.a = a; s.b = b; s.c = c;
    if (0 != lowp_launch(s)) return EXIT_FAILURE;
    if (0 != where.visible()) (void)stream_sync();
    return EXIT_SUCCESS;
  }
  const size_t csize = (4 == s.lowp ? 2 : 4);
  const size_t ba = ((size_t)(s.k / 2 - 1) * s.lda + s.m) * 2 * 2, bb = ((size_t)(s.n - 1) * s.ldb + s.k) * 2, bc = ((size_t)(s.n - 1) * s.ldc + s.m) * csize;
  return staged_call(a, ba, b, bb, c, bc, [&](char* da, char* db, char* dc) { s.a = da; s.b = db; s.c = dc; return lowp_launch(s); });
}
} // namespace

// single operand triple, wherever it lives (used by the per-call thunk and by libxsmm_?gemm)
int single_execute(SmmBatch s, const void* a, const void* b, void* c)
{
  if (!device_ready()) { fail_no_device("a dispatched SMM kernel"); return EXIT_FAILURE; }
  s.mode = ADDR_STRIDED; s.batch = 1; s.sa = s.sb = s.sc = 0; s.sync = SYNC_NONE;
  const int ka = pointer_kind(a), kb = pointer_kind(b), kc = pointer_kind(c); // (one driver query per operand: this is the per-call path)
  if (0 != (ka & kb & kc & 1)) {
    const int visible = (0 != ((ka | kb | kc) & 2)) ? 1 : 0;
    // one product far outside the SMM domain: the plain library GEMM (what the reference hands to its BLAS)
    if (2.0 * s.m * s.n * s.k >= 2.0 * 256 * 256 * 256 && s.m >= 64 && s.n >= 64 && s.k >= 32) {
      const double al = (0 != s.general ? s.alpha : 1.0), be = (0 != s.general ? s.beta : ((s.flags & LIBXSMM_GEMM_FLAG_BETA_0) ? 0.0 : 1.0));
      const int e = library_gemm(s.typesize, 0 != s.general && 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_A), 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B),
        s.m, s.n, s.k, al, a, s.lda, b, s.ldb, be, c, s.ldc);
      if (0 == e) { note_launch(8 == s.typesize ? "rocblas_dgemm" : "rocblas_sgemm"); if (0 != visible) (void)stream_sync(); return EXIT_SUCCESS; }
    }
    s.a = a; s.b = b; s.c = c;
    // (a kernel that is called product by product is called again: specialise it whatever the batch size -- 8 instead of 12 us on the
    // GPU per call, which is what paces a loop of calls; the compiler runs on the helper thread, the generic kernel serves meanwhile)
    // (only with the helper thread: a caller must never wait for hiprtc inside a per-product call)
    if (0 == s.general && jit_async_enabled()) s.jit_always = 1;
    return 0 == run_smm(s, visible) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  const int ts = s.typesize;
  return staged_call(a, span_a(s) * ts, b, span_b(s) * ts, c, span_c(s) * ts,
    [&](char* da, char* db, char* dc) { s.a = da; s.b = db; s.c = dc; return run_smm(s, 0); }); // (scratch is plain device memory)
}

void call_kernel(Kernel* k, const void* a, const void* b, void* c, const void* x3, const void* x6)
{
  if (nullptr == k) return;
  if (KC_PACKED == k->kclass) { packed_call(k, a, b, c); return; } // kernel(a, b, c) over one pack (xsmm_packed.cpp)
  if (KC_XCOPY == k->kclass) { xcopy_call(k, a, b, c, x3); return; } // kernel(in, &ldi, out, &ldo) (xsmm_xcopy.cpp)
  if (KC_LOWP == k->kclass && 0 != (k->desc.flags & LIBXSMM_GEMM_FLAG_BATCH_REDUCE)) { // kernel(a[], b[], c, &count): bf16 batch-reduce
    if (nullptr == x3 || nullptr == a || nullptr == b || nullptr == c) return;
    const unsigned long long count = *static_cast<const unsigned long long*>(x3);
    if (0 == count) return;
    if (!device_ready()) { fail_no_device("a low-precision batch-reduce kernel"); return; }
    SmmBatch s = lowp_from_descriptor(k->desc, 1.f);
    s.mode = ADDR_POINTER; s.sa = s.sb = (long long)sizeof(void*); s.sc = 0; s.batch = (long long)count; s.sync = SYNC_NONE; s.c = c;
    const int kc = pointer_kind(c);
    bool ok = 0 != (kc & 1);
    if (ok && is_device_ptr(a) && is_device_ptr(b)) { s.a = a; s.b = b; } // pointer arrays the GPU reaches
    else if (ok) { // host arrays of pointers to device matrices: the arrays travel through the pinned ring
      const void* const a0 = *static_cast<const void* const*>(a); const void* const b0 = *static_cast<const void* const*>(b);
      ok = is_device_ptr(a0) && is_device_ptr(b0);
      if (ok) { s.a = index_upload(a, (size_t)count * sizeof(void*)); s.b = index_upload(b, (size_t)count * sizeof(void*)); ok = (nullptr != s.a && nullptr != s.b); }
    }
    if (!ok) {
      index_upload_commit();
      fprintf(stderr, "LIBXSMM-AMD ERROR: low-precision batch-reduce kernels need matrices the GPU can reach (libxsmm_malloc or device memory)\n");
      return;
    }
    const char* name = "";
    const int e = launch_smm_lowp_reduce(s, device().stream, &name); note_launch(name);
    index_upload_commit();
    if (0 != e) launch_failed(name, e);
    else if (0 != (kc & 2)) (void)stream_sync();
    return;
  }
  if (KC_LOWP == k->kclass) { // i16 -> f32 kernels are called as kernel(a, b, c, pa, pb, pc, &scf) (samples/xgemm/kernel.c:262)
    const bool scaled = (LIBXSMM_GEMM_PRECISION_I16 == LIBXSMM_GETENUM_INP(k->desc.datatype) && LIBXSMM_GEMM_PRECISION_F32 == LIBXSMM_GETENUM_OUT(k->desc.datatype));
    if (scaled && nullptr == x6) return;
    (void)lowp_single_execute(lowp_from_descriptor(k->desc, scaled ? *static_cast<const float*>(x6) : 1.f), a, b, c);
    return;
  }
  if (KC_DENSE == k->kclass) {
    if (try_record(k->desc, a, b, c)) return;
    if (defer_call(k, a, b, c)) return; // device operands: recorded, runs in stream order without a launch of its own (xsmm_defer.cpp)
    (void)single_execute(from_descriptor(k->desc), a, b, c);
  }
  else if (KC_REDUCE == k->kclass) { // xbm(const void** a, const void** b, void* c, const unsigned long long* count)
    if (nullptr == x3 || nullptr == a || nullptr == b || nullptr == c) return;
    const unsigned long long count = *static_cast<const unsigned long long*>(x3);
    if (0 == count) return;
    const libxsmm_blasint ptrsize = (libxsmm_blasint)sizeof(void*);
    SmmBatch s = from_descriptor(k->desc);
    s.jit_always = 1; // a batch-reduce kernel is dispatched once and called over and over with short batches
    void* cc = c;
    // one run: every product lands in the same C (stride_c == NULL), accumulated in batch order. beta = 0: only the first
    // product overwrites C and the chain goes on from there (the reference's kernel zeroes its accumulators once) -- a batch of
    // beta = 0 products is a batch of independent overwrites, so the first product goes ahead on its own
    long long first = 0;
    if (0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0)) {
      if (EXIT_SUCCESS != batch_execute(s, 0, 0, &ptrsize, &ptrsize, nullptr, a, b, &cc, 0, 1, false)) return;
      s.flags &= ~LIBXSMM_GEMM_FLAG_BETA_0; s.beta = 1.0; first = 1;
    }
    (void)batch_execute(s, 0, 0, &ptrsize, &ptrsize, nullptr, a, b, &cc, first, (long long)count, false);
  }
  else if (KC_TEXT == k->kclass) { // kernel(a, b, c) of the SOA family: one product (batch form: libxsmm_amd_kernel_execute_batch)
    (void)text_kernel_execute(k->text, a, b, c, 0, 0, 1);
  }
  else if (KC_CSR_REG == k->kclass) { // kernel(ignored, B, C) -- reference fsspmdm call site src/libxsmm_fsspmdm.c:267
    if (!device_ready()) { fail_no_device("a csr_reg kernel"); return; }
    const int ts = (LIBXSMM_GEMM_PRECISION_F64 == LIBXSMM_GETENUM_INP(k->desc.datatype)) ? 8 : 4;
    CsrPanels p; memset(&p, 0, sizeof(p));
    p.typesize = ts; p.m = (int)k->desc.m; p.k = (int)k->desc.k; p.n = (int)k->desc.n; p.ldb = (int)k->desc.ldb; p.ldc = (int)k->desc.ldc;
    p.beta0 = (0 != (k->desc.flags & LIBXSMM_GEMM_FLAG_BETA_0)); p.skip_empty_rows = 1;
    p.rowptr = k->d_rowptr; p.colidx = k->d_colidx; p.values = k->d_values; p.nnz = k->nnz; p.batch = 1;
    auto launch = [&](const void* pb, void* pc) {
      const char* name = "";
      p.b = pb; p.c = pc;
      const int e = launch_csr_panels(p, device().stream, &name); note_launch(name);
      if (0 != e) launch_failed(name, e);
      return e;
    };
    const int kb = pointer_kind(b), kc = (0 != (kb & 1) ? pointer_kind(c) : 0);
    if (0 != (kb & kc & 1)) { if (0 == launch(b, c) && 0 != ((kb | kc) & 2)) (void)stream_sync(); }
    else {
      const size_t eb = (size_t)(p.k - 1) * p.ldb + p.n, ec = (size_t)(p.m - 1) * p.ldc + p.n;
      (void)staged_call(nullptr, 0, b, eb * ts, c, ec * ts, [&](char*, char* db, char* dc) { return launch(db, dc); });
    }
  }
}

} // namespace xsmm
