// xsmm_gemm.cpp -- batched SMM front end: libxsmm_mmbatch / gemm_batch(_omp) / ?gemm_batch / ?gemm, the
// per-call kernel thunks, and the staging path for host-resident operands.
//
// Reference: src/libxsmm_gemm.c (libxsmm_mmbatch_kernel :1315-1608, libxsmm_mmbatch :1809-1875,
// libxsmm_gemm_batch :1878-1888, ?gemm_batch :1231-1262, ?gemm :1265-1290) and src/libxsmm_ext_gemm.c
// (OpenMP batch driver :758-1013, auto-batch :1016-1135). The reference iterates the batch on the CPU and
// calls one JIT kernel per item; here the batch *is* the launch: one grid over all items, three addressing
// modes resolved on the device.
#include "xsmm_internal.hpp"

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace xsmm {
int launch_smm_generic(const SmmBatch& s, void* stream, const char** name);
int launch_smm_special(const SmmBatch& s, void* stream, const char** name); // returns -1 if no specialised variant applies
}

namespace xsmm { bool relaxed_order(int ntasks, libxsmm_blasint index_stride, const void* c); }

using namespace xsmm;

namespace {

// host_visible: -1 = look at the operands (a driver query each), 0 = the caller knows they are plain device memory, 1 = some
// operand is memory the CPU addresses as well (the call waits for the stream)
int run_smm(const SmmBatch& s, int host_visible = -1)
{
  const char* name = "";
  int e = -1;
  e = launch_smm_jit_mfma(s, device().stream, &name);                               // matrix-core kernels of this very descriptor
  if (e < 0 && 0 == s.general && 0 == (smm_skip_mask() & SMM_SKIP_SPECIAL)) e = launch_smm_special(s, device().stream, &name);  // hand-tuned shapes; the same kernels for any descriptor
  if (e < 0) e = launch_smm_jit(s, device().stream, &name);                         // shape-specialised via hiprtc (SYNC_DEVICE: whatever the verdict on the device, one of its kernels works)
  if (e < 0) e = launch_smm_generic(s, device().stream, &name);                     // any descriptor
  if (SYNC_DEVICE == s.sync) flag_slot_commit(); // the launches that read the verdict are queued
  note_launch(name);
  if (0 != e) fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
  else if (0 <= host_visible) { if (0 != host_visible) (void)stream_sync(); }
  else if (ADDR_POINTER == s.mode) { // arrays of pointers: look at the first operands if the arrays can be read here
    if (is_host_visible(s.a) && is_host_visible(s.b) && is_host_visible(s.c)) {
      settle(*static_cast<const void* const*>(s.a), *static_cast<const void* const*>(s.b), *static_cast<void* const*>(s.c));
    }
  }
  else settle(s.a, s.b, s.c);
  return e;
}

size_t span_a(const SmmBatch& s) { // elements touched by one A operand
  return (0 != s.general && 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_A)) ? ((size_t)(s.m - 1) * s.lda + s.k) : ((size_t)(s.k - 1) * s.lda + s.m);
}
size_t span_b(const SmmBatch& s) {
  return (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B)) ? ((size_t)(s.k - 1) * s.ldb + s.n) : ((size_t)(s.n - 1) * s.ldb + s.k);
}
size_t span_c(const SmmBatch& s) { return (size_t)(s.n - 1) * s.ldc + s.m; }

// Decide how C operands alias (see SyncMode). beta == 0 or a negative batchsize (caller's promise, reference
// src/libxsmm_gemm.c:1338,1430) need no care. Otherwise adjacent C operands are inspected on the device:
// strictly increasing => independent; non-decreasing => runs; anything else => atomics.
int choose_sync(SmmBatch& s, bool nosync)
{
  s.sync = SYNC_NONE;
  if (nosync || 0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0) || s.batch < 2 || 0 != s.general) return 0;
  if (0 == s.shared_across_calls) {
    if (ADDR_STRIDED == s.mode) { s.sync = (0 == s.sc ? SYNC_RUNS : SYNC_NONE); return 0; }
    if (ADDR_INDEX == s.mode && nullptr == s.ic) { s.sync = SYNC_RUNS; return 0; }
    if (ADDR_POINTER == s.mode && 0 == s.sc) { s.sync = SYNC_RUNS; return 0; }
  }
  // The verdict stays on the device: the check kernel leaves its counts in a flag slot and the compute kernels launched
  // behind it on the same stream read them. No host round trip, the call returns while the GPU is still working.
  int* const d_flags = flag_slot();
  if (nullptr == d_flags) return -1;
  if (0 != s.shared_across_calls) {
    // Task `tid` of `ntasks`: the other slices of the batch are in flight on other threads' streams and may update the same
    // C blocks (the reference takes a lock per C, src/libxsmm_gemm.c:1366-1423). No look at this slice alone can rule
    // that out, so the verdict is fixed to "C repeats out of order": every update of C is an atomic add.
    const int e = flag_slot_set(d_flags, 0, 1);
    if (0 != e) return e;
  }
  else {
    const int e = launch_c_order_check(s, d_flags, device().stream);
    if (0 != e) return e;
  }
  s.sync = SYNC_DEVICE; s.devflags = d_flags;
  // C blocks that repeat out of order are summed with floating-point atomics, which do not reach host memory
  if (ADDR_POINTER != s.mode) s.c_atomics = is_host_visible(s.c) ? 0 : 1;
  else s.c_atomics = (is_host_visible(s.c) && is_host_visible(*static_cast<void* const*>(s.c))) ? 0 : 1;
  return 0;
}

// General form (alpha, beta, TRANS_A outside the SMM domain): C = alpha * op(A_i) * op(B_i) + beta * C item by item, in batch
// order -- what the reference's libxsmm_mmbatch_blas does in a sequential loop (src/libxsmm_gemm.c:1778-1806). Items that
// share a C cannot be done side by side (and no atomic expresses the scaling by beta): consecutive repeats are walked as
// runs by one unit (SYNC_RUNS, the value of C carried from item to item); repeats out of order cut the batch into groups
// without a repeat, launched one after the other in stream order. The verdict needs a host round trip here: this is the
// BLAS-fallback path, not the hot path.
int run_general(SmmBatch s)
{
  s.sync = SYNC_NONE;
  if (s.batch < 2) return run_smm(s);
  if ((ADDR_STRIDED == s.mode && 0 != s.sc)) return run_smm(s);
  if ((ADDR_STRIDED == s.mode && 0 == s.sc) || (ADDR_INDEX == s.mode && nullptr == s.ic) || (ADDR_POINTER == s.mode && 0 == s.sc)) {
    s.sync = SYNC_RUNS; return run_smm(s); // one C for the whole batch
  }
  int* const d_flags = flag_slot();
  int verdict[2] = { 0, 1 };
  if (nullptr == d_flags || 0 != launch_c_order_check(s, d_flags, device().stream)) return -1;
  flag_slot_commit();
  if (0 != d2h(verdict, d_flags, sizeof(verdict))) return -1;
  if (0 == verdict[1]) { s.sync = (0 != verdict[0]) ? SYNC_RUNS : SYNC_NONE; return run_smm(s); }
  // C blocks repeat out of order: where they are, item by item
  std::vector<unsigned long long> key((size_t)s.batch);
  if (ADDR_INDEX == s.mode) {
    std::vector<char> raw((size_t)(s.batch - 1) * s.index_stride + sizeof(int));
    if (0 != d2h(raw.data(), s.ic, raw.size())) return -1;
    for (long long i = 0; i < s.batch; ++i) key[(size_t)i] = (unsigned long long)(long long)(*reinterpret_cast<const int*>(raw.data() + i * s.index_stride));
  }
  else { // ADDR_POINTER
    std::vector<char> raw((size_t)(s.batch - 1) * s.sc + sizeof(void*));
    if (0 != d2h(raw.data(), s.c, raw.size())) return -1;
    for (long long i = 0; i < s.batch; ++i) key[(size_t)i] = (unsigned long long)reinterpret_cast<uintptr_t>(*reinterpret_cast<void* const*>(raw.data() + i * s.sc));
  }
  std::unordered_map<unsigned long long, char> seen;
  long long begin = 0;
  auto launch_group = [&](long long b0, long long b1) -> int {
    SmmBatch g = s; g.batch = b1 - b0; g.sync = SYNC_NONE;
    if (ADDR_INDEX == s.mode) {
      if (nullptr != s.ia) g.ia = reinterpret_cast<const int*>(reinterpret_cast<const char*>(s.ia) + b0 * s.index_stride);
      if (nullptr != s.ib) g.ib = reinterpret_cast<const int*>(reinterpret_cast<const char*>(s.ib) + b0 * s.index_stride);
      g.ic = reinterpret_cast<const int*>(reinterpret_cast<const char*>(s.ic) + b0 * s.index_stride);
    }
    else { g.a = static_cast<const char*>(s.a) + b0 * s.sa; g.b = static_cast<const char*>(s.b) + b0 * s.sb; g.c = static_cast<char*>(s.c) + b0 * s.sc; }
    return run_smm(g);
  };
  for (long long i = 0; i < s.batch; ++i) {
    if (seen.end() != seen.find(key[(size_t)i])) { // item i's C is already part of the open group: close it
      const int e = launch_group(begin, i);
      if (0 != e) return e;
      seen.clear(); begin = i;
    }
    seen.emplace(key[(size_t)i], 1);
  }
  return launch_group(begin, s.batch);
}

int choose_sync(SmmBatch& s, bool nosync);
// decides how the C operands of a batch are kept apart, then launches
int sync_and_run(SmmBatch& s, bool nosync)
{
  if (0 != s.general) return run_general(s);
  if (0 != choose_sync(s, nosync)) return -1;
  return run_smm(s);
}

// Several batches of one precision whose operands the GPU reaches, independent of each other (no C block is written by two
// of them): the batches that need the C-ordering verdict are checked with one launch and -- where the shape-specialised run
// kernels apply -- multiplied with one launch (launch_smm_jit_grouped), so that the chains of all batches are resident
// together. Whatever does not fit that form is launched batch by batch. Every s[i] arrives with its addressing resolved
// (device index / pointer arrays) and s[i].sync == SYNC_DEVICE (verdict needed) or SYNC_NONE.
int run_groups(std::vector<SmmBatch>& groups)
{ // The launches follow the caller's group order: groups that need the verdict are collected while they follow each other
  // and leave as one fused launch as soon as a group of the other kind (beta == 0, the caller's promise of a negative size,
  // a single item) comes up -- which is launched behind them, where the caller put it. (The reference works its groups off
  // one after the other, src/libxsmm_gemm.c:1231-1262; groups inside one fused launch run side by side, which is why the
  // callers of this function have made sure that those neither write the same C blocks nor read what another one writes.)
  int result = 0;
  std::vector<SmmBatch> wanted;
  auto flush_wanted = [&]() -> int {
    for (size_t first = 0; first < wanted.size(); first += 32) { // (a check launch takes up to 32 batches)
      const int n = (int)((wanted.size() - first < 32) ? (wanted.size() - first) : 32);
      SmmBatch* const g = wanted.data() + first;
      bool ok = true;
      for (int i = 0; i < n && ok; ++i) {
        int* const slot = flag_slot();
        if (nullptr == slot) { ok = false; break; }
        g[i].devflags = slot; // (c_atomics: set by the caller, who has looked at where C lives)
      }
      if (ok) ok = (0 == launch_c_order_check_groups(g, n, device().stream));
      if (!ok) { flag_slot_commit(); wanted.clear(); return -1; }
      const char* name = "";
      int e = launch_smm_jit_grouped(g, n, device().stream, &name);
      if (0 <= e) { note_launch(name); if (0 != e) { fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e); result = e; } }
      else { // batch by batch (each reads its verdict slot)
        for (int i = 0; i < n; ++i) { e = run_smm(g[i]); if (0 != e) result = e; }
      }
      flag_slot_commit();
    }
    wanted.clear();
    return 0;
  };
  for (size_t i = 0; i < groups.size(); ++i) {
    if (SYNC_DEVICE == groups[i].sync && 1 < groups[i].batch && 0 == groups[i].general) wanted.push_back(groups[i]);
    else if (0 < groups[i].batch) {
      if (0 != flush_wanted()) return -1;
      groups[i].sync = SYNC_NONE;
      const int e = run_smm(groups[i]);
      if (0 != e) result = e;
    }
  }
  if (0 != flush_wanted()) return -1;
  return result;
}

// Slices of one libxsmm_mmbatch call that run on several threads AND stage C through private device copies (operands in
// pageable host memory) must not overlap in time: a slice's copy-back would overwrite what another slice has just
// written (the reference takes a lock per C, src/libxsmm_gemm.c:1366-1423; here the staged slices take turns).
std::mutex g_staged_tasks_lock;

struct IndexRange { long long lo, hi; }; // element index range [lo, hi] used by an index array

IndexRange index_range(const int* idx, int index_stride, int index_base, long long n)
{
  IndexRange r = { 0, 0 };
  if (nullptr == idx || 0 == n) return r;
  r.lo = r.hi = (long long)(*idx) - index_base;
  for (long long i = 1; i < n; ++i) {
    const long long v = (long long)(*reinterpret_cast<const int*>(reinterpret_cast<const char*>(idx) + i * index_stride)) - index_base;
    if (v < r.lo) r.lo = v;
    if (v > r.hi) r.hi = v;
  }
  return r;
}

// Bring an index array to the device if it lives in host memory (12 bytes per item at most: negligible next
// to the 16 KiB of operands of a 32^3 item, but it must not be dereferenced by the GPU in place).
const int* device_indexes(const int* idx, int index_stride, long long n, int slot, bool* ok)
{
  if (nullptr == idx) return nullptr;
  if (is_device_ptr(idx)) return idx;
  const size_t bytes = (size_t)(n - 1) * index_stride + sizeof(int);
  (void)slot;
  void* const d = index_upload(idx, bytes); // pinned ring + asynchronous copy: the call does not wait for the GPU
  if (nullptr == d) { *ok = false; return nullptr; }
  return static_cast<const int*>(d);
}

// The core of libxsmm_mmbatch for a validated problem: resolves where everything lives, stages what the GPU
// cannot reach, launches, and copies C back when it was staged. Returns EXIT_SUCCESS/EXIT_FAILURE.
int batch_execute(SmmBatch s, libxsmm_blasint index_base, libxsmm_blasint index_stride,
                  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
                  const void* a, const void* b, void* c, long long begin, long long end, bool nosync)
{
  if (end <= begin) return EXIT_SUCCESS;
  if (!device_ready()) { fail_no_device("libxsmm_mmbatch"); return EXIT_FAILURE; }
  const long long n = end - begin;
  const int ts = s.typesize;
  s.batch = n;
  bool ok = true;
  if (0 != index_stride) { // ---------------- index arrays ----------------
    s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride;
    const int* const sa = (nullptr != stride_a ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_a) + begin * index_stride) : nullptr);
    const int* const sb = (nullptr != stride_b ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_b) + begin * index_stride) : nullptr);
    const int* const sc = (nullptr != stride_c ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_c) + begin * index_stride) : nullptr);
    const bool dev_ops = is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(c);
    if (dev_ops) {
      s.a = a; s.b = b; s.c = c;
      s.ia = device_indexes(sa, index_stride, n, 0, &ok);
      s.ib = device_indexes(sb, index_stride, n, 1, &ok);
      s.ic = device_indexes(sc, index_stride, n, 2, &ok);
      if (!ok) { index_upload_commit(); return EXIT_FAILURE; }
      const int e = sync_and_run(s, nosync);
      index_upload_commit();
      return 0 == e ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    // host operands (an unchanged CPU caller): stage the touched element ranges over PCIe
    if (is_device_ptr(sa) || is_device_ptr(sb) || is_device_ptr(sc)) {
      fprintf(stderr, "LIBXSMM-AMD ERROR: host matrices with device index arrays are not supported\n");
      return EXIT_FAILURE;
    }
    std::unique_lock<std::mutex> turn(g_staged_tasks_lock, std::defer_lock);
    if (1 < s.tasks) { turn.lock(); s.shared_across_calls = 0; } // staged slices of one call take turns: nothing is shared meanwhile
    const IndexRange ra = index_range(sa, index_stride, index_base, n), rb = index_range(sb, index_stride, index_base, n),
                     rc = index_range(sc, index_stride, index_base, n);
    const size_t ea = (size_t)(ra.hi - ra.lo) + span_a(s), eb = (size_t)(rb.hi - rb.lo) + span_b(s), ec = (size_t)(rc.hi - rc.lo) + span_c(s);
    char* const da = static_cast<char*>(scratch(3, ea * ts));
    char* const db = static_cast<char*>(scratch(4, eb * ts));
    char* const dc = static_cast<char*>(scratch(5, ec * ts));
    if (nullptr == da || nullptr == db || nullptr == dc) return EXIT_FAILURE;
    const char* const ha = static_cast<const char*>(a) + ra.lo * ts;
    const char* const hb = static_cast<const char*>(b) + rb.lo * ts;
    char* const hc = static_cast<char*>(c) + rc.lo * ts;
    if (0 != h2d(da, ha, ea * ts) || 0 != h2d(db, hb, eb * ts)) return EXIT_FAILURE;
    if (0 != h2d(dc, hc, ec * ts)) return EXIT_FAILURE; // also for beta == 0: untouched gaps must survive the copy back
    s.a = da - ra.lo * ts; s.b = db - rb.lo * ts; s.c = dc - rc.lo * ts; // index arithmetic stays valid
    s.ia = device_indexes(sa, index_stride, n, 0, &ok);
    s.ib = device_indexes(sb, index_stride, n, 1, &ok);
    s.ic = device_indexes(sc, index_stride, n, 2, &ok);
    if (!ok) { index_upload_commit(); return EXIT_FAILURE; }
    const int e = sync_and_run(s, nosync);
    index_upload_commit();
    if (0 != e) return EXIT_FAILURE;
    return 0 == d2h(hc, dc, ec * ts) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // ---------------- arrays of pointers ----------------
  // *stride is the byte distance between consecutive pointers (reference :1426-1428, including its
  // index_base*sizeof(void*) correction)
  const long long da = (nullptr != stride_a ? ((long long)*stride_a - (long long)index_base * (long long)sizeof(void*)) : 0);
  const long long db = (nullptr != stride_b ? ((long long)*stride_b - (long long)index_base * (long long)sizeof(void*)) : 0);
  const long long dc = (nullptr != stride_c ? ((long long)*stride_c - (long long)index_base * (long long)sizeof(void*)) : 0);
  s.mode = ADDR_POINTER; s.sa = da; s.sb = db; s.sc = dc;
  const char* const pa = static_cast<const char*>(a) + da * begin;
  const char* const pb = static_cast<const char*>(b) + db * begin;
  char* const pc = static_cast<char*>(c) + dc * begin;
  if (is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(c)) { // pointer arrays already on the device
    s.a = pa; s.b = pb; s.c = pc;
    return 0 == sync_and_run(s, nosync) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // host arrays of pointers: look at the first operand of each to see where the matrices live
  const void* const a0 = *reinterpret_cast<const void* const*>(pa);
  const void* const b0 = *reinterpret_cast<const void* const*>(pb);
  void* const c0 = *reinterpret_cast<void* const*>(pc);
  const size_t na = (0 != da ? (size_t)n : 1), nb = (0 != db ? (size_t)n : 1), nc = (0 != dc ? (size_t)n : 1);
  if (is_device_ptr(a0) && is_device_ptr(b0) && is_device_ptr(c0)) { // device matrices, host pointer arrays: upload the arrays
    std::vector<const void*> ta(na), tb(nb); std::vector<void*> tc(nc);
    for (size_t i = 0; i < na; ++i) ta[i] = *reinterpret_cast<const void* const*>(pa + da * (long long)i);
    for (size_t i = 0; i < nb; ++i) tb[i] = *reinterpret_cast<const void* const*>(pb + db * (long long)i);
    for (size_t i = 0; i < nc; ++i) tc[i] = *reinterpret_cast<void* const*>(pc + dc * (long long)i);
    // (pinned ring + asynchronous copies: the temporaries are copied before this returns, the call does not wait for the GPU)
    void* const xa = index_upload(ta.data(), na * sizeof(void*)); void* const xb = index_upload(tb.data(), nb * sizeof(void*));
    void* const xc = index_upload(tc.data(), nc * sizeof(void*));
    if (nullptr == xa || nullptr == xb || nullptr == xc) { index_upload_commit(); return EXIT_FAILURE; }
    s.a = xa; s.b = xb; s.c = xc;
    s.sa = (0 != da ? (long long)sizeof(void*) : 0); s.sb = (0 != db ? (long long)sizeof(void*) : 0); s.sc = (0 != dc ? (long long)sizeof(void*) : 0);
    const int e = sync_and_run(s, nosync);
    index_upload_commit();
    return 0 == e ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // host matrices behind host pointer arrays: pack every operand into a dense device buffer, keep aliasing of C
  {
    std::unique_lock<std::mutex> turn(g_staged_tasks_lock, std::defer_lock);
    if (1 < s.tasks) { turn.lock(); s.shared_across_calls = 0; } // staged slices of one call take turns
    const size_t sza = span_a(s), szb = span_b(s), szc = span_c(s);
    char* const ba = static_cast<char*>(scratch(3, na * sza * ts));
    char* const bb = static_cast<char*>(scratch(4, nb * szb * ts));
    if (nullptr == ba || nullptr == bb) return EXIT_FAILURE;
    std::vector<const void*> ta(na), tb(nb); std::vector<void*> tc(nc);
    // one host image and one copy per operand array (a copy per matrix is a driver call per matrix: 10^5 recorded calls took seconds)
    std::vector<char> ha(na * sza * ts), hb(nb * szb * ts), hc;
    for (size_t i = 0; i < na; ++i) {
      memcpy(ha.data() + i * sza * ts, *reinterpret_cast<const void* const*>(pa + da * (long long)i), sza * ts);
      ta[i] = ba + i * sza * ts;
    }
    for (size_t i = 0; i < nb; ++i) {
      memcpy(hb.data() + i * szb * ts, *reinterpret_cast<const void* const*>(pb + db * (long long)i), szb * ts);
      tb[i] = bb + i * szb * ts;
    }
    if (0 != h2d(ba, ha.data(), ha.size()) || 0 != h2d(bb, hb.data(), hb.size())) return EXIT_FAILURE;
    // distinct host C matrices get distinct device copies; repeated pointers share one
    std::vector<void*> uniq; std::vector<size_t> slot_of(nc);
    {
      std::unordered_map<void*, size_t> seen; seen.reserve(nc);
      for (size_t i = 0; i < nc; ++i) {
        void* const hp = *reinterpret_cast<void* const*>(pc + dc * (long long)i);
        size_t j;
        if (!uniq.empty() && uniq.back() == hp) j = uniq.size() - 1; // consecutive duplicates are the common case (CP2K stacks)
        else {
          const auto it = seen.find(hp);
          if (it != seen.end()) j = it->second; else { j = uniq.size(); uniq.push_back(hp); seen.emplace(hp, j); }
        }
        slot_of[i] = j;
      }
    }
    char* const bc = static_cast<char*>(scratch(5, uniq.size() * szc * ts));
    if (nullptr == bc) return EXIT_FAILURE;
    hc.resize(uniq.size() * szc * ts);
    for (size_t j = 0; j < uniq.size(); ++j) memcpy(hc.data() + j * szc * ts, uniq[j], szc * ts);
    if (0 != h2d(bc, hc.data(), hc.size())) return EXIT_FAILURE;
    for (size_t i = 0; i < nc; ++i) tc[i] = bc + slot_of[i] * szc * ts;
    void* const xa = scratch(0, na * sizeof(void*)); void* const xb = scratch(1, nb * sizeof(void*)); void* const xc = scratch(2, nc * sizeof(void*));
    if (nullptr == xa || nullptr == xb || nullptr == xc) return EXIT_FAILURE;
    if (0 != h2d(xa, ta.data(), na * sizeof(void*)) || 0 != h2d(xb, tb.data(), nb * sizeof(void*)) || 0 != h2d(xc, tc.data(), nc * sizeof(void*))) return EXIT_FAILURE;
    if (0 != stream_sync()) return EXIT_FAILURE;
    s.a = xa; s.b = xb; s.c = xc;
    s.sa = (0 != da ? (long long)sizeof(void*) : 0); s.sb = (0 != db ? (long long)sizeof(void*) : 0); s.sc = (0 != dc ? (long long)sizeof(void*) : 0);
    if (0 != sync_and_run(s, nosync)) return EXIT_FAILURE;
    if (0 != d2h(hc.data(), bc, hc.size())) return EXIT_FAILURE; // (synchronises)
    for (size_t j = 0; j < uniq.size(); ++j) memcpy(uniq[j], hc.data() + j * szc * ts, szc * ts);
    return EXIT_SUCCESS;
  }
}

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
  const size_t ea = span_a(s), eb = span_b(s), ec = span_c(s);
  char* const da = static_cast<char*>(scratch(3, ea * ts));
  char* const db = static_cast<char*>(scratch(4, eb * ts));
  char* const dc = static_cast<char*>(scratch(5, ec * ts));
  if (nullptr == da || nullptr == db || nullptr == dc) return EXIT_FAILURE;
  if (0 != h2d(da, a, ea * ts) || 0 != h2d(db, b, eb * ts) || 0 != h2d(dc, c, ec * ts)) return EXIT_FAILURE;
  s.a = da; s.b = db; s.c = dc;
  if (0 != run_smm(s)) return EXIT_FAILURE;
  return 0 == d2h(c, dc, ec * ts) ? EXIT_SUCCESS : EXIT_FAILURE;
}

// ---- auto-batch recording (reference src/libxsmm_ext_gemm.c:1016-1135) -----------------------------------------
struct Recorded { const void* a; const void* b; void* c; };
struct Recorder {
  std::mutex lock;
  bool active = false;
  int precision = 0;
  bool have[8] = { false }; int flags = 0, m = 0, n = 0, k = 0, lda = 0, ldb = 0, ldc = 0; double alpha = 1, beta = 1;
  libxsmm_gemm_descriptor desc; bool desc_set = false;
  std::vector<Recorded> items;
};
Recorder& recorder() { static Recorder* r = new Recorder(); return *r; }

bool try_record(const libxsmm_gemm_descriptor& d, const void* a, const void* b, void* c)
{
  Recorder& r = recorder();
  if (!r.active) return false;
  std::lock_guard<std::mutex> guard(r.lock);
  if (!r.active) return false;
  const int prec = LIBXSMM_GETENUM_INP(d.datatype);
  if (prec != r.precision) return false;
  if ((r.have[0] && (int)(d.flags & 3) != (r.flags & 3)) || (r.have[1] && (int)d.m != r.m) || (r.have[2] && (int)d.n != r.n) ||
      (r.have[3] && (int)d.k != r.k) || (r.have[4] && (int)d.lda != r.lda) || (r.have[5] && (int)d.ldb != r.ldb) ||
      (r.have[6] && (int)d.ldc != r.ldc)) return false;
  if (r.desc_set && 0 != memcmp(&r.desc, &d, sizeof(d))) return false; // one shape per recording
  if (!r.desc_set) { r.desc = d; r.desc_set = true; }
  r.items.push_back(Recorded{ a, b, c });
  return true;
}

// ---- batch calls inside a libxsmm_amd_defer_begin/end bracket ---------------------------------------------------------
// A caller's loop of libxsmm_gemm_batch calls, one per shape (samples/cp2k/cp2k.cpp:328-360), launches shape after shape:
// the chains of one shape do not fill the chip and launches on one stream do not overlap. Inside a bracket the calls are
// recorded -- each as the fully resolved batch libxsmm_amd_gemm_batch_groups would build for it -- and leave together at
// the flush (batch_flush_record). Index and pointer arrays the CPU addresses are copied at the call (the caller may reuse
// its buffers as soon as the call returns, as with the reference's synchronous calls); the staged copies stay uncommitted
// until the flush has queued the launches that read them.
constexpr int MERGE_MAX_CALLS = 64;                         // calls a record holds (two check launches' worth): the 65th flushes it first
constexpr int MERGE_MAX_UPLOADS = INDEX_UPLOAD_RING - 16;  // staged arrays a record may hold (three per call at most)

struct MergeRecord {
  std::vector<SmmBatch> calls;
  std::vector<unsigned long long> hulls;  // six per call: {a_lo, a_hi, b_lo, b_hi, c_lo, c_hi}; filled at the call where the host can read the arrays
  std::vector<char> on_device;            // != 0: the call's arrays live in device memory, its hulls come from the hull kernel
  int uploads = 0;
  std::vector<unsigned long long> table;  // the hull kernel's tables, copied back (the device side lives in the thread's scratch)
  // what the last flush did (libxsmm_amd_merge_last_plan)
  std::vector<unsigned long long> plan_hulls; std::vector<int> plan_segment; int plan_device = 0;
};
thread_local MergeRecord tl_merge;

bool host_readable(int kind) { return 0 == kind || 0 != (kind & 2); } // plain host memory, or pinned / managed memory

void hull_of_indexes(unsigned long long* out, const void* base, const int* idx, int index_stride, int index_base, long long n, int typesize, size_t span)
{ // (a NULL index array: every item uses the base itself, see resolve() in kernels/smm_common.cuh)
  const IndexRange r = index_range(idx, index_stride, index_base, n);
  const unsigned long long p = reinterpret_cast<uintptr_t>(base);
  out[0] = p + (unsigned long long)(r.lo * typesize);
  out[1] = p + (unsigned long long)(r.hi * typesize) + (unsigned long long)span * typesize;
}

void hull_of_pointers(unsigned long long* out, const void* const* ptrs, size_t n, int typesize, size_t span)
{
  unsigned long long lo = reinterpret_cast<uintptr_t>(ptrs[0]), hi = lo;
  for (size_t i = 1; i < n; ++i) { const unsigned long long q = reinterpret_cast<uintptr_t>(ptrs[i]); if (q < lo) lo = q; if (q > hi) hi = q; }
  out[0] = lo; out[1] = hi + (unsigned long long)span * typesize;
}

// Recorded calls leave in segments: consecutive calls that may run side by side. The rule is the one the grouped pointer batches
// follow (try_grouped_pointer_batches): a call's C must not meet another member's A, B or C. A call that conflicts with a member
// of the open segment opens a new one -- it then runs behind all of them, in call order.
// hulls: {a_lo, a_hi, b_lo, b_hi, c_lo, c_hi} per call, byte addresses, half-open. segment_of[i] receives the segment of call i
// (0, 1, ...; non-decreasing); returns the number of segments.
int merge_segments(int n, const unsigned long long* hulls, int* segment_of)
{
  auto meet = [](const unsigned long long* x, const unsigned long long* y) { return x[0] < y[1] && y[0] < x[1]; }; // half-open ranges
  int first = 0, segment = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned long long* const hi = hulls + 6 * (size_t)i;
    for (int j = first; j < i; ++j) {
      const unsigned long long* const hj = hulls + 6 * (size_t)j;
      if (meet(hi + 4, hj + 0) || meet(hi + 4, hj + 2) || meet(hi + 4, hj + 4) || meet(hj + 4, hi + 0) || meet(hj + 4, hi + 2)) {
        first = i; ++segment;
        break;
      }
    }
    segment_of[i] = segment;
  }
  return 0 < n ? segment + 1 : 0;
}

// true: the call was recorded and runs at the next flush. false: nothing was done, the call takes the ordinary path (which
// flushes the record on its way: it asks for the stream).
bool record_batch_call(const Kernel* k, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, libxsmm_blasint batchsize, int ntasks)
{
  if (!defer_bracket_open() || nullptr == k || KC_DENSE != k->kclass || 1 != ntasks || 0 == batchsize || !device_ready()) return false;
  const long long size = (batchsize < 0 ? -(long long)batchsize : batchsize);
  void* const stream = device_raw().stream;
  if (defer_capturing(stream)) return false;
  SmmBatch s = from_descriptor(k->desc);
  const int ts = s.typesize;
  const int ka = pointer_kind(a), kb = pointer_kind(b), kc = pointer_kind(c);
  std::vector<const void*> ta, tb, tc; // host pointer arrays, gathered
  const int* host_idx[3] = { nullptr, nullptr, nullptr };
  bool on_device = false;
  if (0 != index_stride) { // index arrays: a, b, c are the matrices
    if (0 == (ka & kb & kc & 1) || 0 != (kc & 2)) return false; // host matrices (staged), or a C the CPU reads on return
    s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride; s.a = a; s.b = b; s.c = c;
    const int* const idx[3] = { reinterpret_cast<const int*>(stride_a), reinterpret_cast<const int*>(stride_b), reinterpret_cast<const int*>(stride_c) };
    for (int o = 0; o < 3; ++o) {
      if (nullptr == idx[o]) continue;
      if (host_readable(pointer_kind(idx[o]))) host_idx[o] = idx[o]; else on_device = true;
    }
    s.ia = idx[0]; s.ib = idx[1]; s.ic = idx[2]; // (host arrays: replaced by their staged copies below)
  }
  else { // arrays of pointers: a, b, c are the arrays (byte distances as in batch_execute)
    s.mode = ADDR_POINTER;
    s.sa = (nullptr != stride_a ? ((long long)*stride_a - (long long)index_base * (long long)sizeof(void*)) : 0);
    s.sb = (nullptr != stride_b ? ((long long)*stride_b - (long long)index_base * (long long)sizeof(void*)) : 0);
    s.sc = (nullptr != stride_c ? ((long long)*stride_c - (long long)index_base * (long long)sizeof(void*)) : 0);
    if (1 == ka && 1 == kb && 1 == kc) { s.a = a; s.b = b; s.c = c; on_device = true; } // device arrays: the matrices live on the device as well
    else if (host_readable(ka) && host_readable(kb) && host_readable(kc)) {
      const size_t na = (0 != s.sa ? (size_t)size : 1), nb = (0 != s.sb ? (size_t)size : 1), nc = (0 != s.sc ? (size_t)size : 1);
      ta.resize(na); tb.resize(nb); tc.resize(nc);
      for (size_t i = 0; i < na; ++i) ta[i] = *reinterpret_cast<const void* const*>(static_cast<const char*>(a) + s.sa * (long long)i);
      for (size_t i = 0; i < nb; ++i) tb[i] = *reinterpret_cast<const void* const*>(static_cast<const char*>(b) + s.sb * (long long)i);
      for (size_t i = 0; i < nc; ++i) tc[i] = *reinterpret_cast<const void* const*>(static_cast<const char*>(c) + s.sc * (long long)i);
      const int k0 = pointer_kind(tc[0]); // (the first operand of each tells where the matrices live, as in batch_execute)
      if (0 == (pointer_kind(ta[0]) & pointer_kind(tb[0]) & k0 & 1) || 0 != (k0 & 2)) return false;
    }
    else return false;
  }
  s.batch = size; s.tasks = 1; s.c_atomics = 1;
  s.relaxed = relaxed_order(ntasks, index_stride, c) ? 1 : 0;
  s.sync = (0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0) || batchsize < 0 || size < 2) ? SYNC_NONE : SYNC_DEVICE; // (one C for the whole batch is found out on the device as well)
  MergeRecord& r = tl_merge;
  record_begin(OPEN_BATCH); // a burst of per-call kernels, recorded spmdm blocks: they come first
  if (!r.calls.empty()) { // one fused launch takes one precision, one policy, one order of the sums; the staging ring must hold the record
    const SmmBatch& f = r.calls.front();
    // (a change of stream needs no test here: libxsmm_amd_set_stream asks for the stream, which flushes)
    if (f.typesize != ts || f.use_mfma != s.use_mfma || f.relaxed != s.relaxed
      || MERGE_MAX_CALLS <= (int)r.calls.size() || MERGE_MAX_UPLOADS < r.uploads + 3) { record_flush(); record_begin(OPEN_BATCH); }
  }
  unsigned long long hull[6] = { 0, 0, 0, 0, 0, 0 };
  const size_t span[3] = { span_a(s), span_b(s), span_c(s) };
  bool ok = true; int uploads = 0; // (staged on the stream as it is: asking for it would launch the record that is being extended)
  if (ADDR_INDEX == s.mode) {
    const int** const dst[3] = { &s.ia, &s.ib, &s.ic };
    for (int o = 0; o < 3 && ok; ++o) {
      if (nullptr == host_idx[o]) continue;
      void* const d = index_upload_on(stream, host_idx[o], (size_t)(size - 1) * index_stride + sizeof(int));
      ++uploads; ok = (nullptr != d);
      *dst[o] = static_cast<const int*>(d);
    }
    if (ok && !on_device) {
      hull_of_indexes(hull + 0, a, host_idx[0], index_stride, index_base, size, ts, span[0]);
      hull_of_indexes(hull + 2, b, host_idx[1], index_stride, index_base, size, ts, span[1]);
      hull_of_indexes(hull + 4, c, host_idx[2], index_stride, index_base, size, ts, span[2]);
    }
  }
  else if (!on_device) {
    s.a = index_upload_on(stream, ta.data(), ta.size() * sizeof(void*)); s.b = index_upload_on(stream, tb.data(), tb.size() * sizeof(void*));
    s.c = index_upload_on(stream, tc.data(), tc.size() * sizeof(void*));
    uploads = 3; ok = (nullptr != s.a && nullptr != s.b && nullptr != s.c);
    s.sa = (0 != s.sa ? (long long)sizeof(void*) : 0); s.sb = (0 != s.sb ? (long long)sizeof(void*) : 0); s.sc = (0 != s.sc ? (long long)sizeof(void*) : 0);
    hull_of_pointers(hull + 0, ta.data(), ta.size(), ts, span[0]);
    hull_of_pointers(hull + 2, tb.data(), tb.size(), ts, span[1]);
    hull_of_pointers(hull + 4, tc.data(), tc.size(), ts, span[2]);
  }
  if (!ok) return false; // (entries a failed upload has filled: the ordinary path's commit releases them)
  r.uploads += uploads;
  r.calls.push_back(s); r.hulls.insert(r.hulls.end(), hull, hull + 6); r.on_device.push_back(on_device ? 1 : 0);
  return true;
}

} // namespace

namespace xsmm {

// Launches the batch calls recorded on this thread. The hulls of calls whose arrays live in device memory come from the hull
// kernel and one small copy back -- the only wait for the device this path knows, once per flush and only then. The calls are
// cut into segments of independent calls (merge_segments); every segment is one run_groups, segment after segment on the stream:
// dependent calls keep the call order, a segment of one call is the launch it would have been on its own.
void batch_flush_record()
{ // (reached through record_flush() alone: nothing is open while the launches below ask for the stream)
  MergeRecord& r = tl_merge;
  const int n = (int)r.calls.size();
  if (0 == n) return; // (opened for a call whose staging failed)
  void* const stream = device().stream;
  bool hulls_ok = true;
  std::vector<int> dev; // the calls the hull kernel looks at
  for (int i = 0; i < n; ++i) if (0 != r.on_device[(size_t)i]) dev.push_back(i);
  if (!dev.empty()) {
    constexpr size_t TABLE = 2 * 3 * BATCH_HULL_CALLS, TABLES = (MERGE_MAX_CALLS + BATCH_HULL_CALLS - 1) / BATCH_HULL_CALLS;
    // (a capture that began with the record open: nothing may be waited for -- the calls run one after the other)
    unsigned long long* const d_hulls = defer_capturing(stream) ? nullptr : static_cast<unsigned long long*>(scratch(7, TABLES * TABLE * sizeof(unsigned long long)));
    r.table.resize(TABLES * TABLE);
    hulls_ok = (nullptr != d_hulls);
    size_t tables = 0;
    for (size_t first = 0; first < dev.size() && hulls_ok; first += BATCH_HULL_CALLS, ++tables) {
      const int m = (int)((dev.size() - first < (size_t)BATCH_HULL_CALLS) ? (dev.size() - first) : (size_t)BATCH_HULL_CALLS);
      SmmBatch chunk[BATCH_HULL_CALLS]; unsigned long long spans[3 * BATCH_HULL_CALLS];
      for (int j = 0; j < m; ++j) {
        const SmmBatch& s = r.calls[(size_t)dev[first + (size_t)j]];
        chunk[j] = s;
        spans[3 * j + 0] = (unsigned long long)span_a(s) * s.typesize; spans[3 * j + 1] = (unsigned long long)span_b(s) * s.typesize;
        spans[3 * j + 2] = (unsigned long long)span_c(s) * s.typesize;
      }
      hulls_ok = (0 == launch_batch_hulls(chunk, spans, m, d_hulls + tables * TABLE, stream));
    }
    if (hulls_ok) hulls_ok = (0 == d2h(r.table.data(), d_hulls, tables * TABLE * sizeof(unsigned long long))); // (waits for the stream)
    for (size_t j = 0; j < dev.size() && hulls_ok; ++j) {
      const unsigned long long* const t = r.table.data() + (j / BATCH_HULL_CALLS) * TABLE;
      const size_t e = 3 * (j % BATCH_HULL_CALLS);
      unsigned long long* const h = r.hulls.data() + 6 * (size_t)dev[j];
      for (int o = 0; o < 3; ++o) { h[2 * o] = t[e + (size_t)o]; h[2 * o + 1] = t[3 * BATCH_HULL_CALLS + e + (size_t)o]; }
    }
  }
  std::vector<int> segment((size_t)n, 0);
  if (hulls_ok) (void)merge_segments(n, r.hulls.data(), segment.data());
  else for (int i = 0; i < n; ++i) segment[(size_t)i] = i; // no verdict: call after call, which is always right
  bool ok = true;
  for (int first = 0; first < n;) {
    int last = first + 1;
    while (last < n && segment[(size_t)last] == segment[(size_t)first]) ++last;
    std::vector<SmmBatch> groups(r.calls.begin() + first, r.calls.begin() + last);
    if (0 != run_groups(groups)) ok = false;
    first = last;
  }
  index_upload_commit(); // the launches that read the staged arrays are queued
  if (!ok) { static int error_once = 0; if (0 != libxsmm_verbosity && once(&error_once)) fprintf(stderr, "LIBXSMM ERROR: recorded libxsmm_gemm_batch calls failed!\n"); }
  r.plan_hulls.swap(r.hulls); r.plan_segment.swap(segment); r.plan_device = (hulls_ok ? (int)dev.size() : -1);
  r.calls.clear(); r.hulls.clear(); r.on_device.clear(); r.uploads = 0;
}

// What a kernel thunk does when user code calls the bare function pointer.
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
  if (0 != e) fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
  return e;
}

int lowp_single_execute(SmmBatch s, const void* a, const void* b, void* c)
{
  if (!device_ready()) { fail_no_device("a dispatched low-precision kernel"); return EXIT_FAILURE; }
  s.mode = ADDR_STRIDED; s.batch = 1; s.sync = SYNC_NONE;
  if (is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(c)) {
    s.a = a; s.b = b; s.c = c;
    if (0 != lowp_launch(s)) return EXIT_FAILURE;
    settle(a, b, c);
    return EXIT_SUCCESS;
  }
  const size_t csize = (4 == s.lowp ? 2 : 4);
  const size_t ba = ((size_t)(s.k / 2 - 1) * s.lda + s.m) * 2 * 2, bb = ((size_t)(s.n - 1) * s.ldb + s.k) * 2, bc = ((size_t)(s.n - 1) * s.ldc + s.m) * csize;
  char* const da = static_cast<char*>(scratch(3, ba)); char* const db = static_cast<char*>(scratch(4, bb)); char* const dc = static_cast<char*>(scratch(5, bc));
  if (nullptr == da || nullptr == db || nullptr == dc) return EXIT_FAILURE;
  if (0 != h2d(da, a, ba) || 0 != h2d(db, b, bb) || 0 != h2d(dc, c, bc)) return EXIT_FAILURE;
  s.a = da; s.b = db; s.c = dc;
  if (0 != lowp_launch(s)) return EXIT_FAILURE;
  return 0 == d2h(c, dc, bc) ? EXIT_SUCCESS : EXIT_FAILURE;
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
    bool ok = is_device_ptr(c);
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
    if (0 != e) fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
    else settle(c);
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
    const char* name = "";
    if (is_device_ptr(b) && is_device_ptr(c)) {
      p.b = b; p.c = c;
      const int e = launch_csr_panels(p, device().stream, &name); note_launch(name);
      if (0 != e) fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
      else settle(b, c);
    }
    else {
      const size_t eb = (size_t)(p.k - 1) * p.ldb + p.n, ec = (size_t)(p.m - 1) * p.ldc + p.n;
      char* const db = static_cast<char*>(scratch(4, eb * ts)); char* const dc = static_cast<char*>(scratch(5, ec * ts));
      if (nullptr == db || nullptr == dc || 0 != h2d(db, b, eb * ts) || 0 != h2d(dc, c, ec * ts)) return;
      p.b = db; p.c = dc;
      const int e = launch_csr_panels(p, device().stream, &name); note_launch(name);
      if (0 != e) { fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e); return; }
      (void)d2h(c, dc, ec * ts);
    }
  }
}

// Whether the products that share a C may be summed in any order. The reference's sequential entry points
// (libxsmm_gemm_batch, mmbatch with one task) add them in batch order; its multi-threaded ones (libxsmm_gemm_batch_omp,
// ?gemm_batch_omp, mmbatch with several tasks: a lock per C, src/libxsmm_gemm.c:1366-1423) in whatever order the threads
// arrive. Only the latter may be served by the segment/atomic form of the run kernels. LIBXSMM_AMD_BATCH_ORDER=relaxed
// (strict) overrides for all entry points. Floating-point atomics do not reach host memory: C the CPU addresses stays strict.
thread_local int tl_relaxed_order = 0;
bool relaxed_order(int ntasks, libxsmm_blasint index_stride, const void* c)
{
  static const int env = []() { const char* e = getenv("LIBXSMM_AMD_BATCH_ORDER"); return (nullptr == e || 0 == *e) ? 0 : (('r' == *e || 'R' == *e) ? 1 : -1); }();
  if (0 > env || (0 == env && ntasks <= 1 && 0 == tl_relaxed_order)) return false;
  if (0 != index_stride) return !is_host_visible(c);
  if (is_device_ptr(c) && !is_host_visible(c)) return true; // device array of pointers: the matrices live on the device as well
  const void* const c0 = *static_cast<const void* const*>(c);
  return !is_host_visible(c0);
}

} // namespace xsmm

// ---- public batch interface ------------------------------------------------------------------------------------
LIBXSMM_API int libxsmm_mmbatch_kernel(libxsmm_xmmfunction kernel, libxsmm_blasint index_base,
  libxsmm_blasint index_stride, const libxsmm_blasint stride_a[], const libxsmm_blasint stride_b[], const libxsmm_blasint stride_c[],
  const void* a, const void* b, void* c, libxsmm_blasint batchsize, /*unsigned*/int tid, /*unsigned*/int ntasks,
  unsigned char itypesize, unsigned char otypesize, int flags)
{ // reference src/libxsmm_gemm.c:1315-1324: task `tid` of `ntasks` owns the slice [tid*tasksize, min(...))
  (void)itypesize; (void)otypesize; (void)flags;
  Kernel* const k = kernel_from_pointer(reinterpret_cast<const void*>(kernel.xmm));
  if (nullptr == k || KC_CSR_REG == k->kclass || KC_TEXT == k->kclass || KC_PACKED == k->kclass || KC_XCOPY == k->kclass || nullptr == a || nullptr == b || nullptr == c || ntasks < 1 || tid < 0 || tid >= ntasks) return EXIT_FAILURE;
  const long long size = (batchsize < 0 ? -(long long)batchsize : batchsize);
  const long long tasksize = (size + ntasks - 1) / ntasks;
  const long long begin = (long long)tid * tasksize, span = begin + tasksize, end = (span < size ? span : size);
  if (KC_LOWP == k->kclass) { // batches of low-precision products: independent C operands, everything device-reachable
    if (0 != (k->desc.flags & LIBXSMM_GEMM_FLAG_BATCH_REDUCE)) return EXIT_FAILURE; // (a batch-reduce kernel is called with its own argument list)
    if (!device_ready()) { fail_no_device("libxsmm_mmbatch_kernel"); return EXIT_FAILURE; }
    if (end <= begin) return EXIT_SUCCESS;
    if (LIBXSMM_GEMM_PRECISION_I16 == LIBXSMM_GETENUM_INP(k->desc.datatype) && LIBXSMM_GEMM_PRECISION_F32 == LIBXSMM_GETENUM_OUT(k->desc.datatype)) return EXIT_FAILURE; // no way to pass the scaling factor
    SmmBatch s = lowp_from_descriptor(k->desc, 1.f);
    s.batch = end - begin; s.sync = SYNC_NONE;
    bool ok = is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(c);
    if (ok && 0 != index_stride) {
      s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride; s.a = a; s.b = b; s.c = c;
      s.ia = device_indexes(nullptr != stride_a ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_a) + begin * index_stride) : nullptr, index_stride, s.batch, 0, &ok);
      s.ib = device_indexes(nullptr != stride_b ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_b) + begin * index_stride) : nullptr, index_stride, s.batch, 1, &ok);
      s.ic = device_indexes(nullptr != stride_c ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(stride_c) + begin * index_stride) : nullptr, index_stride, s.batch, 2, &ok);
    }
    else if (ok) { // arrays of pointers in device-reachable memory
      s.mode = ADDR_POINTER;
      s.sa = (nullptr != stride_a ? ((long long)*stride_a - (long long)index_base * (long long)sizeof(void*)) : 0);
      s.sb = (nullptr != stride_b ? ((long long)*stride_b - (long long)index_base * (long long)sizeof(void*)) : 0);
      s.sc = (nullptr != stride_c ? ((long long)*stride_c - (long long)index_base * (long long)sizeof(void*)) : 0);
      s.a = static_cast<const char*>(a) + s.sa * begin; s.b = static_cast<const char*>(b) + s.sb * begin; s.c = static_cast<char*>(c) + s.sc * begin;
    }
    if (!ok) {
      fprintf(stderr, "LIBXSMM-AMD ERROR: batches of low-precision products need operands the GPU can reach (libxsmm_malloc or device memory)\n");
      return EXIT_FAILURE;
    }
    const int le = lowp_launch(s);
    index_upload_commit();
    if (0 != le) return EXIT_FAILURE;
    if (ADDR_INDEX == s.mode) settle(a, b, c);
    else (void)stream_sync();
    return EXIT_SUCCESS;
  }
  // inside a libxsmm_amd_defer_begin/end bracket: recorded, leaves with its neighbours at the flush
  if (record_batch_call(k, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, batchsize, ntasks)) return EXIT_SUCCESS;
  record_flush(); // a call that is not recorded runs behind the recorded ones
  SmmBatch s = from_descriptor(k->desc);
  s.relaxed = relaxed_order(ntasks, index_stride, c) ? 1 : 0;
  s.shared_across_calls = (1 < ntasks && 0 <= batchsize) ? 1 : 0; // (a negative batchsize is the caller's promise that nothing is shared)
  s.tasks = ntasks;
  // ntasks > 1: the tasks run concurrently on the caller's threads and may share C across slices; as in the
  // reference (lock per C, :1366-1423) correctness then needs atomic updates unless the caller opts out.
  const bool nosync = (batchsize < 0);
  if (KC_REDUCE == k->kclass) { // all products of the slice land in consecutive-equal C runs by construction
    return batch_execute(s, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, begin, end, false);
  }
  return batch_execute(s, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, begin, end, nosync);
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
  s.lda = (nullptr != lda ? *lda : (0 == (LIBXSMM_GEMM_FLAG_TRANS_A & flags) ? m : k));
  s.ldb = (nullptr != ldb ? *ldb : (0 == (LIBXSMM_GEMM_FLAG_TRANS_B & flags) ? k : n));
  s.ldc = (nullptr != ldc ? *ldc : m);
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
  const long long size = (batchsize < 0 ? -(long long)batchsize : batchsize);
  return batch_general(LIBXSMM_GEMM_PRECISION_F64 == iprec ? 8 : 4, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc,
    index_base, index_stride, stride_a, stride_b, stride_c, 0, size);
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
  libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_init2(&blob, iprec, oprec, m, n, k,
    nullptr != lda ? *lda : (0 == (LIBXSMM_GEMM_FLAG_TRANS_A & gemm_flags) ? m : k),
    nullptr != ldb ? *ldb : (0 == (LIBXSMM_GEMM_FLAG_TRANS_B & gemm_flags) ? k : n),
    nullptr != ldc ? *ldc : m, alpha, beta, gemm_flags, libxsmm_get_gemm_auto_prefetch());
  if (nullptr != desc) { // the AI gate of the reference (:1827) selects BLAS for large shapes; one device path serves both here
    const libxsmm_xmmfunction kernel = libxsmm_xmmdispatch(desc);
    if (nullptr != kernel.xmm) {
      result = libxsmm_mmbatch_kernel(kernel, index_base, index_stride, stride_a, stride_b, stride_c, a, b, c, batchsize,
        tid, nthreads, libxsmm_typesize((libxsmm_datatype)iprec), otypesize, desc->flags);
    }
  }
  if (EXIT_SUCCESS != result && iprec == oprec && (LIBXSMM_GEMM_PRECISION_F64 == iprec || LIBXSMM_GEMM_PRECISION_F32 == iprec)) {
    // quiet fall-back (:1842-1866): general alpha/beta/transposes
    const long long size = (batchsize < 0 ? -(long long)batchsize : batchsize);
    const long long tasksize = (size + nthreads - 1) / nthreads;
    const long long begin = (long long)tid * tasksize, span = begin + tasksize, end = (span < size ? span : size);
    result = batch_general(LIBXSMM_GEMM_PRECISION_F64 == iprec ? 8 : 4, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc,
      index_base, index_stride, stride_a, stride_b, stride_c, begin, end, nthreads);
  }
  if (EXIT_SUCCESS != result && 0 != libxsmm_verbosity && once(&error_once)) {
    fprintf(stderr, "LIBXSMM ERROR: libxsmm_mmbatch failed!\n");
  }
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
  struct Range { uintptr_t lo, hi; };
  struct Hulls { Range a, b, c; };
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
    s.sync = (0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0) || group_size[g] < 0 || size < 2) ? SYNC_NONE : SYNC_DEVICE;
    auto hull = [&](const T* const* p, size_t span) { // address range the matrices behind `size` pointers occupy
      uintptr_t lo = reinterpret_cast<uintptr_t>(p[0]), hi = lo;
      for (long long i = 1; i < size; ++i) { const uintptr_t q = reinterpret_cast<uintptr_t>(p[i]); if (q < lo) lo = q; if (q > hi) hi = q; }
      return Range{ lo, hi + span * sizeof(T) };
    };
    hulls.push_back(Hulls{ hull(a_array + j, span_a(s)), hull(b_array + j, span_b(s)), hull(const_cast<const T* const*>(c_array + j), span_c(s)) });
    s.a = a_array + j; s.b = b_array + j; s.c = c_array + j; // (host arrays for now: uploaded below, once all groups have passed)
    groups.push_back(s);
    j += size;
  }
  // The reference runs the groups strictly one after the other: a later group may read (as A or B) or update what an earlier
  // one wrote. Fused, the groups run side by side -- only if no group's C meets another group's C, A or B.
  auto meet = [](const Range& x, const Range& y) { return x.lo < y.hi && y.lo < x.hi; };
  for (size_t x = 0; x < hulls.size(); ++x) for (size_t y = 0; y < hulls.size(); ++y) {
    if (x != y && (meet(hulls[x].c, hulls[y].a) || meet(hulls[x].c, hulls[y].b) || (x < y && meet(hulls[x].c, hulls[y].c)))) return false;
  }
  bool ok = true;
  for (SmmBatch& s : groups) {
    void* const xa = index_upload(s.a, (size_t)s.batch * sizeof(void*)); void* const xb = index_upload(s.b, (size_t)s.batch * sizeof(void*));
    void* const xc = index_upload(s.c, (size_t)s.batch * sizeof(void*));
    if (nullptr == xa || nullptr == xb || nullptr == xc) { ok = false; break; }
    s.a = xa; s.b = xb; s.c = xc;
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
  if (!(is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(c))) {
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
  return 0 == run_smm(s) ? EXIT_SUCCESS : EXIT_FAILURE;
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
  static const int order_env = []() { const char* e = getenv("LIBXSMM_AMD_BATCH_ORDER"); return (nullptr == e || 0 == *e) ? 0 : (('r' == *e || 'R' == *e) ? 1 : -1); }();
  for (int g = 0; g < ngroups && ok; ++g) {
    const char ta = (nullptr != transa ? transa[g] : 'N'), tb = (nullptr != transb ? transb[g] : 'N');
    const int flags = LIBXSMM_GEMM_PFLAGS(&ta, &tb, LIBXSMM_FLAGS);
    libxsmm_descriptor_blob blob;
    const libxsmm_gemm_descriptor* const desc = libxsmm_gemm_descriptor_init2(&blob, iprec, oprec, m[g], n[g], k[g],
      nullptr != lda ? lda[g] : (0 == (LIBXSMM_GEMM_FLAG_TRANS_A & flags) ? m[g] : k[g]),
      nullptr != ldb ? ldb[g] : (0 == (LIBXSMM_GEMM_FLAG_TRANS_B & flags) ? k[g] : n[g]),
      nullptr != ldc ? ldc[g] : m[g], alpha, beta, flags, LIBXSMM_GEMM_PREFETCH_NONE);
    const Kernel* const kern = (nullptr != desc ? kernel_from_pointer(reinterpret_cast<const void*>(libxsmm_xmmdispatch(desc).xmm)) : nullptr);
    if (nullptr == kern || KC_DENSE != kern->kclass) { ok = false; break; } // outside the SMM domain (alpha, beta, TRANS_A, precision)
    const long long size = (group_size[g] < 0 ? -(long long)group_size[g] : group_size[g]);
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
      s.ia = device_indexes(nullptr != stride_a ? stride_a[g] : nullptr, index_stride, size, 0, &ok);
      s.ib = device_indexes(nullptr != stride_b ? stride_b[g] : nullptr, index_stride, size, 1, &ok);
      s.ic = device_indexes(nullptr != stride_c ? stride_c[g] : nullptr, index_stride, size, 2, &ok);
    }
    // how C blocks repeat inside the group: nobody cares (beta == 0, or the caller's promise of a negative size), one C for
    // the whole group (runs), or to be found out on the device
    if (0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0) || group_size[g] < 0 || size < 2) s.sync = SYNC_NONE;
    else s.sync = SYNC_DEVICE; // (stride_c == NULL -- one C for the group -- is found out on the device as well: all neighbours equal)
    groups.push_back(s);
  }
  int e = -1;
  if (ok) e = run_groups(groups);
  index_upload_commit();
  if (0 != e) return EXIT_FAILURE;
  if (host_visible) (void)stream_sync(); // operands the CPU addresses directly are done with when the call returns
  return EXIT_SUCCESS;
}

LIBXSMM_API int libxsmm_amd_merge_segments(int n, const unsigned long long hulls[], int segment_of[])
{ // see include/libxsmm_amd.h
  if (n < 0 || (0 < n && (nullptr == hulls || nullptr == segment_of))) return -1;
  return merge_segments(n, hulls, segment_of);
}

LIBXSMM_API int libxsmm_amd_merge_last_plan(int* ncalls, int* nsegments, int* ndevice_hulls, unsigned long long hulls[], int segment_of[], int capacity)
{ // see include/libxsmm_amd.h
  const MergeRecord& r = tl_merge;
  const int n = (int)r.plan_segment.size();
  if (nullptr != ncalls) *ncalls = n;
  if (nullptr != nsegments) *nsegments = (0 < n ? r.plan_segment.back() + 1 : 0);
  if (nullptr != ndevice_hulls) *ndevice_hulls = r.plan_device;
  const int m = (n < capacity ? n : capacity);
  for (int i = 0; i < m; ++i) {
    if (nullptr != segment_of) segment_of[i] = r.plan_segment[(size_t)i];
    if (nullptr != hulls) memcpy(hulls + 6 * (size_t)i, r.plan_hulls.data() + 6 * (size_t)i, 6 * sizeof(unsigned long long));
  }
  return 0 < m ? m : 0;
}

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
  if (nullptr != buffer && 0 < buffer_size) {
    const size_t n = (text.size() < buffer_size - 1 ? text.size() : buffer_size - 1);
    memcpy(buffer, text.data(), n); buffer[n] = 0;
  }
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
  const libxsmm_blasint ilda = LIBXSMM_MAX(nullptr != lda ? *lda : (0 == (LIBXSMM_GEMM_FLAG_TRANS_A & flags) ? mm : kk), 1);
  const libxsmm_blasint ildb = LIBXSMM_MAX(nullptr != ldb ? *ldb : (0 == (LIBXSMM_GEMM_FLAG_TRANS_B & flags) ? kk : nn), 1);
  const libxsmm_blasint ildc = LIBXSMM_MAX(nullptr != ldc ? *ldc : mm, 1);
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

LIBXSMM_API void libxsmm_dgemm(const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const double* alpha, const double* a, const libxsmm_blasint* lda, const double* b, const libxsmm_blasint* ldb,
  const double* beta, double* c, const libxsmm_blasint* ldc)
{ xgemm<double>(LIBXSMM_GEMM_PRECISION_F64, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

LIBXSMM_API void libxsmm_sgemm(const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const float* alpha, const float* a, const libxsmm_blasint* lda, const float* b, const libxsmm_blasint* ldb,
  const float* beta, float* c, const libxsmm_blasint* ldc)
{ xgemm<float>(LIBXSMM_GEMM_PRECISION_F32, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

// libxsmm_blas_?gemm (reference src/libxsmm_gemm.c:703-760): "the BLAS the library falls back to". There is no host BLAS
// behind this engine; the general-form kernel (any alpha/beta/transposes) is that fallback, so these are the same call.
LIBXSMM_API void libxsmm_blas_dgemm(const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const double* alpha, const double* a, const libxsmm_blasint* lda, const double* b, const libxsmm_blasint* ldb,
  const double* beta, double* c, const libxsmm_blasint* ldc)
{ xgemm<double>(LIBXSMM_GEMM_PRECISION_F64, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

LIBXSMM_API void libxsmm_blas_sgemm(const char* transa, const char* transb,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const float* alpha, const float* a, const libxsmm_blasint* lda, const float* b, const libxsmm_blasint* ldb,
  const float* beta, float* c, const libxsmm_blasint* ldc)
{ xgemm<float>(LIBXSMM_GEMM_PRECISION_F32, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

// ---- auto-batch (reference src/libxsmm_ext_gemm.c:1016-1135) ---------------------------------------------------------
LIBXSMM_APIEXT void libxsmm_mmbatch_begin(libxsmm_gemm_precision precision, const int* flags,
  const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const libxsmm_blasint* lda, const libxsmm_blasint* ldb, const libxsmm_blasint* ldc, const void* alpha, const void* beta)
{ // non-NULL arguments filter which calls are recorded (NULL = "free value"); alpha/beta filters are implied by the
  // SMM domain (alpha == 1, beta in {0,1}) because only dispatched kernels are recorded.
  (void)alpha; (void)beta;
  Recorder& r = recorder();
  std::lock_guard<std::mutex> guard(r.lock);
  if (r.active) return; // nested begin: ignored, as the reference does for a batch that is already open
  r.precision = (int)precision;
  r.have[0] = (nullptr != flags); if (r.have[0]) r.flags = *flags;
  r.have[1] = (nullptr != m); if (r.have[1]) r.m = *m;
  r.have[2] = (nullptr != n); if (r.have[2]) r.n = *n;
  r.have[3] = (nullptr != k); if (r.have[3]) r.k = *k;
  r.have[4] = (nullptr != lda); if (r.have[4]) r.lda = *lda;
  r.have[5] = (nullptr != ldb); if (r.have[5]) r.ldb = *ldb;
  r.have[6] = (nullptr != ldc); if (r.have[6]) r.ldc = *ldc;
  r.items.clear(); r.desc_set = false; r.active = true;
}

LIBXSMM_APIEXT void libxsmm_mmbatch_end(void)
{
  Recorder& r = recorder();
  std::vector<Recorded> items; libxsmm_gemm_descriptor desc;
  {
    std::lock_guard<std::mutex> guard(r.lock);
    if (!r.active) return;
    r.active = false;
    items.swap(r.items); desc = r.desc;
    if (!r.desc_set) return;
  }
  if (items.empty()) return;
  // flush as one pointer-array batch; recorded order is kept, so products into the same C accumulate in call order
  std::vector<const void*> pa(items.size()), pb(items.size()); std::vector<void*> pc(items.size());
  for (size_t i = 0; i < items.size(); ++i) { pa[i] = items[i].a; pb[i] = items[i].b; pc[i] = items[i].c; }
  const libxsmm_blasint ptrsize = (libxsmm_blasint)sizeof(void*);
  SmmBatch s = from_descriptor(desc);
  (void)batch_execute(s, 0, 0, &ptrsize, &ptrsize, &ptrsize, pa.data(), pb.data(), pc.data(), 0, (long long)items.size(), false);
}

LIBXSMM_API int libxsmm_amd_smm_kernel_source(const libxsmm_gemm_descriptor* descriptor, int variant, char* buffer, size_t buffer_size, int compile)
{ // the HIP text a dense descriptor is specialised to (reference counterpart: libxsmm_generator_gemm_kernel's noarch
  // text output, src/generator_gemm_noarch.c); compile != 0 additionally runs hiprtc for gfx950 (no device needed).
  // variant: bit 0 = element-wide accesses (index/pointer batches), bit 1 = runs of equal C accumulate in registers
  if (nullptr == descriptor) return -1;
  const libxsmm_gemm_descriptor& d = *descriptor;
  const int ip = LIBXSMM_GETENUM_INP(d.datatype);
  if (LIBXSMM_GEMM_PRECISION_F64 != ip && LIBXSMM_GEMM_PRECISION_F32 != ip) return -1;
  const std::string src = gen_smm_source(LIBXSMM_GEMM_PRECISION_F64 == ip ? 8 : 4, (int)d.m, (int)d.n, (int)d.k, d.flags, variant & 0x1FFFF, (int)d.lda, (int)d.ldb, (int)d.ldc);
  if (nullptr != buffer && 0 < buffer_size) {
    const size_t n = (src.size() < buffer_size - 1 ? src.size() : buffer_size - 1);
    memcpy(buffer, src.data(), n); buffer[n] = 0;
  }
  if (0 != compile) {
    std::string log, built;
    const int rc = jit_check_source(src, &log, &built);
    if (0 != rc && 0 != libxsmm_verbosity) fprintf(stderr, "LIBXSMM-AMD: hiprtc: %s\n", log.c_str());
    if (0 == rc && 2 == compile && nullptr != buffer && 0 < buffer_size) { // the text the library builds (hand-wait guard applied)
      const size_t n = (built.size() < buffer_size - 1 ? built.size() : buffer_size - 1);
      memcpy(buffer, built.data(), n); buffer[n] = 0;
    }
    return rc;
  }
  return (int)src.size();
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
  if (nullptr != buffer && 0 < buffer_size) {
    const size_t n = (src.size() < buffer_size - 1 ? src.size() : buffer_size - 1);
    memcpy(buffer, src.data(), n); buffer[n] = 0;
  }
  if (0 != compile) {
    std::string log, built;
    const int rc = jit_check_source(src, &log, &built);
    if (0 != rc && 0 != libxsmm_verbosity) fprintf(stderr, "LIBXSMM-AMD: hiprtc: %s\n", log.c_str());
    if (0 == rc && 2 == compile && nullptr != buffer && 0 < buffer_size) { // the text the library builds (hand-wait guard applied)
      const size_t n = (built.size() < buffer_size - 1 ? built.size() : buffer_size - 1);
      memcpy(buffer, built.data(), n); buffer[n] = 0;
    }
    return rc;
  }
  return (int)src.size();
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
LIBXSMM_APIEXT void __wrap_dgemm_(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const double* alpha, const double* a, const libxsmm_blasint* lda, const double* b, const libxsmm_blasint* ldb,
  const double* beta, double* c, const libxsmm_blasint* ldc)
{ libxsmm_dgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

LIBXSMM_APIEXT void __wrap_sgemm_(const char* transa, const char* transb, const libxsmm_blasint* m, const libxsmm_blasint* n, const libxsmm_blasint* k,
  const float* alpha, const float* a, const libxsmm_blasint* lda, const float* b, const libxsmm_blasint* ldb,
  const float* beta, float* c, const libxsmm_blasint* ldc)
{ libxsmm_sgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc); }

#define XSMM_WRAP_BATCH(NAME, T, TARGET)                                                                      \
LIBXSMM_APIEXT void NAME(const char transa_array[], const char transb_array[],                                \
  const libxsmm_blasint m_array[], const libxsmm_blasint n_array[], const libxsmm_blasint k_array[],         \
  const T alpha_array[], const T* a_array[], const libxsmm_blasint lda_array[],                              \
  const T* b_array[], const libxsmm_blasint ldb_array[],                                                     \
  const T beta_array[], T* c_array[], const libxsmm_blasint ldc_array[],                                     \
  const libxsmm_blasint* group_count, const libxsmm_blasint group_size[])                                    \
{ TARGET(transa_array, transb_array, m_array, n_array, k_array, alpha_array, a_array, lda_array, b_array, ldb_array, \
    beta_array, c_array, ldc_array, group_count, group_size); }
XSMM_WRAP_BATCH(__wrap_dgemm_batch_, double, libxsmm_dgemm_batch_omp)
XSMM_WRAP_BATCH(__wrap_sgemm_batch_, float, libxsmm_sgemm_batch_omp)
XSMM_WRAP_BATCH(__wrap_dgemm_batch, double, libxsmm_dgemm_batch_omp)
XSMM_WRAP_BATCH(__wrap_sgemm_batch, float, libxsmm_sgemm_batch_omp)
}
