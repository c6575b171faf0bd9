// xsmm_batch.cpp -- how a batch leaves: the launch chain and the C-ordering verdict (run_smm, choose_sync, run_general,
// run_groups), and the core of libxsmm_mmbatch (batch_execute): where everything lives, staging of what the GPU cannot reach.
// Reference: src/libxsmm_gemm.c (libxsmm_mmbatch_kernel :1315-1608). The reference iterates the batch on the CPU and calls
// one JIT kernel per item; here the batch *is* the launch: one grid over all items, three addressing modes resolved on the device.
#include "xsmm_internal.hpp"
#include "xsmm_batch.hpp"

#include <cstring>
#include <mutex>
#include <unordered_map>

namespace xsmm {

void launch_failed(const char* name, int hip_error) { fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, hip_error); }

Residency classify(const void* a, const void* b, const void* c)
{ // (in turn, and only while all so far are GPU-reachable)
  Residency r = { pointer_kind(a), 0, 0 };
  if (0 != (r.a & 1)) r.b = pointer_kind(b);
  if (0 != (r.b & 1)) r.c = pointer_kind(c);
  return r;
}

int run_smm(const SmmBatch& s, int host_visible)
{
  const char* name = "";
  int e = launch_smm_jit_mfma(s, device().stream, &name);                           // matrix-core kernels of this very descriptor
  if (e < 0 && 0 == s.general && 0 == (smm_skip_mask() & SMM_SKIP_SPECIAL)) e = launch_smm_special(s, device().stream, &name);  // hand-tuned shapes; the same kernels for any descriptor
  if (e < 0) e = launch_smm_jit(s, device().stream, &name);                         // shape-specialised via hiprtc (SYNC_DEVICE: whatever the verdict on the device, one of its kernels works)
  if (e < 0) e = launch_smm_generic(s, device().stream, &name);                     // any descriptor
  if (SYNC_DEVICE == s.sync) flag_slot_commit(); // the launches that read the verdict are queued
  note_launch(name);
  if (0 != e) launch_failed(name, e);
  else if (0 <= host_visible) { if (0 != host_visible) (void)stream_sync(); }
  else if (ADDR_POINTER != s.mode) settle(s.a, s.b, s.c);
  else if (is_host_visible(s.a) && is_host_visible(s.b) && is_host_visible(s.c)) { // arrays of pointers the CPU reads: look at the first operands
    settle(*static_cast<const void* const*>(s.a), *static_cast<const void* const*>(s.b), *static_cast<void* const*>(s.c));
  }
  return e;
}

size_t span_a(const SmmBatch& s) {
  return (0 != s.general && 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_A)) ? ((size_t)(s.m - 1) * s.lda + s.k) : ((size_t)(s.k - 1) * s.lda + s.m);
}
size_t span_b(const SmmBatch& s) {
  return (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B)) ? ((size_t)(s.k - 1) * s.ldb + s.n) : ((size_t)(s.n - 1) * s.ldb + s.k);
}
size_t span_c(const SmmBatch& s) { return (size_t)(s.n - 1) * s.ldc + s.m; }

namespace {
// Decide how C operands alias (see SyncMode). beta == 0 or a negative batchsize (caller's promise, reference
// src/libxsmm_gemm.c:1338,1430) need no care. Otherwise adjacent C operands are inspected on the device:
// strictly increasing => independent; non-decreasing => runs; anything else => atomics.
// c_visible: the CPU addresses the C matrices as well (the caller has looked).
int choose_sync(SmmBatch& s, bool nosync, bool c_visible)
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
  // Task `tid` of `ntasks` (shared_across_calls): the other slices of the batch are in flight on other threads' streams and may
  // update the same C blocks (the reference takes a lock per C, src/libxsmm_gemm.c:1366-1423). No look at this slice alone can
  // rule that out, so the verdict is fixed to "C repeats out of order": every update of C is an atomic add.
  const int e = (0 != s.shared_across_calls) ? flag_slot_set(d_flags, 0, 1) : launch_c_order_check(s, d_flags, device().stream);
  if (0 != e) return e;
  s.sync = SYNC_DEVICE; s.devflags = d_flags;
  s.c_atomics = c_visible ? 0 : 1; // C blocks that repeat out of order are summed with floating-point atomics, which do not reach host memory
  return 0;
}

// General form (alpha, beta, TRANS_A outside the SMM domain): C = alpha * op(A_i) * op(B_i) + beta * C item by item, in batch
// order -- what the reference's libxsmm_mmbatch_blas does in a sequential loop (src/libxsmm_gemm.c:1778-1806). Items that
// share a C cannot be done side by side (and no atomic expresses the scaling by beta): consecutive repeats are walked as
// runs by one unit (SYNC_RUNS, the value of C carried from item to item); repeats out of order cut the batch into groups
// without a repeat, launched one after the other in stream order. The verdict needs a host round trip here: this is the
// BLAS-fallback path, not the hot path.
int run_general(SmmBatch s, int visible)
{
  s.sync = SYNC_NONE;
  if (s.batch < 2 || (ADDR_STRIDED == s.mode && 0 != s.sc)) return run_smm(s, visible);
  if ((ADDR_STRIDED == s.mode && 0 == s.sc) || (ADDR_INDEX == s.mode && nullptr == s.ic) || (ADDR_POINTER == s.mode && 0 == s.sc)) {
    s.sync = SYNC_RUNS; return run_smm(s, visible); // one C for the whole batch
  }
  int* const d_flags = flag_slot();
  int verdict[2] = { 0, 1 };
  if (nullptr == d_flags || 0 != launch_c_order_check(s, d_flags, device().stream)) return -1;
  flag_slot_commit();
  if (0 != d2h(verdict, d_flags, sizeof(verdict))) return -1;
  if (0 == verdict[1]) { s.sync = (0 != verdict[0]) ? SYNC_RUNS : SYNC_NONE; return run_smm(s, visible); }
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
    if (ADDR_INDEX == s.mode) { g.ia = index_at(s.ia, b0, s.index_stride); g.ib = index_at(s.ib, b0, s.index_stride); g.ic = index_at(s.ic, b0, s.index_stride); }
    else { g.a = static_cast<const char*>(s.a) + b0 * s.sa; g.b = static_cast<const char*>(s.b) + b0 * s.sb; g.c = static_cast<char*>(s.c) + b0 * s.sc; }
    return run_smm(g, visible);
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

// decides how the C operands of a batch are kept apart, then launches. visible, c_visible: the CPU addresses one of the
// matrices / the C matrices as well (the call waits at its end / atomics do not reach C)
int sync_and_run(SmmBatch& s, bool nosync, int visible, bool c_visible)
{
  if (0 != s.general) return run_general(s, visible);
  if (0 != choose_sync(s, nosync, c_visible)) return -1;
  return run_smm(s, visible);
}

// Slices of one libxsmm_mmbatch call that run on several threads AND stage C through private device copies (operands in
// pageable host memory) must not overlap in time: a slice's copy-back would overwrite what another slice has just
// written (the reference takes a lock per C, src/libxsmm_gemm.c:1366-1423; here the staged slices take turns).
std::mutex g_staged_tasks_lock;
} // namespace

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
      if (0 <= e) { note_launch(name); if (0 != e) { launch_failed(name, e); result = e; } }
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

// Bring an index array to the device if it lives in host memory (12 bytes per item at most: negligible next
// to the 16 KiB of operands of a 32^3 item, but it must not be dereferenced by the GPU in place).
const int* device_indexes(const int* idx, int index_stride, long long n, bool* ok)
{
  if (nullptr == idx) return nullptr;
  if (is_device_ptr(idx)) return idx;
  const size_t bytes = (size_t)(n - 1) * index_stride + sizeof(int);
  void* const d = index_upload(idx, bytes); // pinned ring + asynchronous copy: the call does not wait for the GPU
  if (nullptr == d) { *ok = false; return nullptr; }
  return static_cast<const int*>(d);
}

bool upload_pointer_arrays(SmmBatch& s, void* stream, const void* a, size_t na, const void* b, size_t nb, const void* c, size_t nc)
{ // (pinned ring + asynchronous copies: the arrays are copied before this returns, the call does not wait for the GPU)
  s.a = index_upload_on(stream, a, na * sizeof(void*)); s.b = index_upload_on(stream, b, nb * sizeof(void*));
  s.c = index_upload_on(stream, c, nc * sizeof(void*));
  s.sa = tight_step(s.sa); s.sb = tight_step(s.sb); s.sc = tight_step(s.sc);
  return nullptr != s.a && nullptr != s.b && nullptr != s.c;
}

bool stage_in(const void* const host[3], const size_t bytes[3], char* dev[3])
{
  for (int o = 0; o < 3; ++o) {
    dev[o] = (nullptr != host[o] ? static_cast<char*>(scratch(3 + o, bytes[o])) : nullptr);
    if (nullptr != host[o] && nullptr == dev[o]) return false;
  }
  for (int o = 0; o < 3; ++o) if (nullptr != host[o] && 0 != h2d(dev[o], host[o], bytes[o])) return false;
  return true;
}

int stage_out(void* host_c, const void* dev_c, size_t bytes) { return d2h(host_c, dev_c, bytes); }

// The core of libxsmm_mmbatch for a validated problem: resolves where everything lives, stages what the GPU
// cannot reach, launches, and copies C back when it was staged. Returns EXIT_SUCCESS/EXIT_FAILURE.
int batch_execute(SmmBatch s, libxsmm_blasint index_base, libxsmm_blasint index_stride,
                  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
                  const void* a, const void* b, void* c, long long begin, long long end, bool nosync)
{
  if (end <= begin) return EXIT_SUCCESS;
  if (!device_ready()) { fail_no_device("libxsmm_mmbatch"); return EXIT_FAILURE; }
  const long long n = end - begin;
  const int ts = s.typesize; s.batch = n;
  bool ok = true;
  const Residency where = classify(a, b, c); // the matrices (index arrays) or the arrays of pointers
  if (0 != index_stride) { // ---------------- index arrays ----------------
    s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride;
    const int* const sa = index_at(stride_a, begin, index_stride), * const sb = index_at(stride_b, begin, index_stride), * const sc = index_at(stride_c, begin, index_stride);
    int visible = where.visible(); bool c_visible = 0 != (where.c & 2);
    const void* host[3] = { nullptr, nullptr, nullptr }; size_t bytes[3] = { 0, 0, 0 }; char* dev[3] = { nullptr, nullptr, nullptr };
    std::unique_lock<std::mutex> turn(g_staged_tasks_lock, std::defer_lock);
    if (where.device()) { s.a = a; s.b = b; s.c = c; }
    else { // host operands (an unchanged CPU caller): stage the touched element ranges over PCIe
      if (is_device_ptr(sa) || is_device_ptr(sb) || is_device_ptr(sc)) {
        fprintf(stderr, "LIBXSMM-AMD ERROR: host matrices with device index arrays are not supported\n");
        return EXIT_FAILURE;
      }
      if (1 < s.tasks) { turn.lock(); s.shared_across_calls = 0; } // staged slices of one call take turns: nothing is shared meanwhile
      const IndexRange ra = index_range(sa, index_stride, index_base, n), rb = index_range(sb, index_stride, index_base, n), rc = index_range(sc, index_stride, index_base, n);
      bytes[0] = ((size_t)(ra.hi - ra.lo) + span_a(s)) * ts; bytes[1] = ((size_t)(rb.hi - rb.lo) + span_b(s)) * ts;
      bytes[2] = ((size_t)(rc.hi - rc.lo) + span_c(s)) * ts;
      host[0] = static_cast<const char*>(a) + ra.lo * ts; host[1] = static_cast<const char*>(b) + rb.lo * ts;
      host[2] = static_cast<char*>(c) + rc.lo * ts; // C also for beta == 0: untouched gaps must survive the copy back
      if (!stage_in(host, bytes, dev)) return EXIT_FAILURE;
      s.a = dev[0] - ra.lo * ts; s.b = dev[1] - rb.lo * ts; s.c = dev[2] - rc.lo * ts; // index arithmetic stays valid
      visible = 0; c_visible = false; // (scratch is plain device memory)
    }
    s.ia = device_indexes(sa, index_stride, n, &ok); s.ib = device_indexes(sb, index_stride, n, &ok); s.ic = device_indexes(sc, index_stride, n, &ok);
    if (!ok) { index_upload_commit(); return EXIT_FAILURE; }
    const int e = sync_and_run(s, nosync, visible, c_visible);
    index_upload_commit();
    if (0 != e) return EXIT_FAILURE;
    return (nullptr == dev[2] || 0 == stage_out(const_cast<void*>(host[2]), dev[2], bytes[2])) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // ---------------- arrays of pointers ----------------
  const long long da = pointer_step(stride_a, index_base), db = pointer_step(stride_b, index_base), dc = pointer_step(stride_c, index_base);
  s.mode = ADDR_POINTER; s.sa = da; s.sb = db; s.sc = dc;
  const char* const pa = static_cast<const char*>(a) + da * begin, * const pb = static_cast<const char*>(b) + db * begin;
  char* const pc = static_cast<char*>(c) + dc * begin;
  if (where.device()) { // pointer arrays already on the device
    s.a = pa; s.b = pb; s.c = pc;
    // arrays the CPU reads as well: what they point to tells whether atomics reach C (the array of C alone) and whether the
    // call waits at its end (only if all three arrays can be read here)
    const bool c_visible = 0 != (where.c & 2) && 0 != (pointer_kind(*reinterpret_cast<void* const*>(pc)) & 2);
    const bool visible = 0 != (where.a & where.b & where.c & 2) && (c_visible
      || 0 != ((pointer_kind(*reinterpret_cast<const void* const*>(pa)) | pointer_kind(*reinterpret_cast<const void* const*>(pb))) & 2));
    return 0 == sync_and_run(s, nosync, visible ? 1 : 0, c_visible) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // host arrays of pointers: look at the first operand of each to see where the matrices live
  const size_t na = pointer_count(da, n), nb = pointer_count(db, n), nc = pointer_count(dc, n);
  std::vector<const void*> ha(na), hb(nb); std::vector<void*> hc(nc);
  gather_pointers(ha, pa, da); gather_pointers(hb, pb, db); gather_pointers(hc, pc, dc);
  if (classify(ha[0], hb[0], hc[0]).device()) { // device matrices, host pointer arrays: upload the arrays
    ok = upload_pointer_arrays(s, device().stream, ha.data(), na, hb.data(), nb, hc.data(), nc);
    // (the uploaded arrays are plain device memory: the call does not wait, atomics are taken to reach C)
    const int e = ok ? sync_and_run(s, nosync, 0, false) : -1;
    index_upload_commit();
    return 0 == e ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  // host matrices behind host pointer arrays: pack every operand into a dense device buffer, keep aliasing of C
  std::unique_lock<std::mutex> turn(g_staged_tasks_lock, std::defer_lock);
  if (1 < s.tasks) { turn.lock(); s.shared_across_calls = 0; } // staged slices of one call take turns
  const size_t sza = span_a(s) * ts, szb = span_b(s) * ts, szc = span_c(s) * ts; // bytes per matrix
  // distinct host C matrices get distinct device copies; repeated pointers share one
  std::vector<void*> uniq; std::vector<size_t> slot_of(nc);
  unique_slots(hc, uniq, slot_of);
  // one host image and one copy per operand array (a copy per matrix is a driver call per matrix: 10^5 recorded calls took seconds)
  std::vector<char> image[3] = { std::vector<char>(na * sza), std::vector<char>(nb * szb), std::vector<char>(uniq.size() * szc) };
  for (size_t i = 0; i < na; ++i) memcpy(image[0].data() + i * sza, ha[i], sza);
  for (size_t i = 0; i < nb; ++i) memcpy(image[1].data() + i * szb, hb[i], szb);
  for (size_t j = 0; j < uniq.size(); ++j) memcpy(image[2].data() + j * szc, uniq[j], szc);
  const void* const host[3] = { image[0].data(), image[1].data(), image[2].data() };
  const size_t bytes[3] = { image[0].size(), image[1].size(), image[2].size() };
  char* dev[3];
  if (!stage_in(host, bytes, dev)) return EXIT_FAILURE;
  std::vector<const void*> ta(na), tb(nb); std::vector<void*> tc(nc);
  for (size_t i = 0; i < na; ++i) ta[i] = dev[0] + i * sza;
  for (size_t i = 0; i < nb; ++i) tb[i] = dev[1] + i * szb;
  for (size_t i = 0; i < nc; ++i) tc[i] = dev[2] + slot_of[i] * szc;
  void* const xa = scratch(0, na * sizeof(void*)); void* const xb = scratch(1, nb * sizeof(void*)); void* const xc = scratch(2, nc * sizeof(void*));
  if (nullptr == xa || nullptr == xb || nullptr == xc) return EXIT_FAILURE;
  if (0 != h2d(xa, ta.data(), na * sizeof(void*)) || 0 != h2d(xb, tb.data(), nb * sizeof(void*)) || 0 != h2d(xc, tc.data(), nc * sizeof(void*))) return EXIT_FAILURE;
  if (0 != stream_sync()) return EXIT_FAILURE;
  s.a = xa; s.b = xb; s.c = xc;
  s.sa = tight_step(da); s.sb = tight_step(db); s.sc = tight_step(dc);
  if (0 != sync_and_run(s, nosync, 0, false)) return EXIT_FAILURE;
  if (0 != stage_out(image[2].data(), dev[2], bytes[2])) return EXIT_FAILURE; // (synchronises)
  for (size_t j = 0; j < uniq.size(); ++j) memcpy(uniq[j], image[2].data() + j * szc, szc);
  return EXIT_SUCCESS;
}

// Batches of low-precision products (libxsmm_mmbatch_kernel with a kernel of 16-bit inputs): independent C operands,
// everything device-reachable.
int lowp_batch_execute(const Kernel* k, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, long long begin, long long end)
{
  if (0 != (k->desc.flags & LIBXSMM_GEMM_FLAG_BATCH_REDUCE)) return EXIT_FAILURE; // (a batch-reduce kernel is called with its own argument list)
  if (!device_ready()) { fail_no_device("libxsmm_mmbatch_kernel"); return EXIT_FAILURE; }
  if (end <= begin) return EXIT_SUCCESS;
  if (LIBXSMM_GEMM_PRECISION_I16 == LIBXSMM_GETENUM_INP(k->desc.datatype) && LIBXSMM_GEMM_PRECISION_F32 == LIBXSMM_GETENUM_OUT(k->desc.datatype)) return EXIT_FAILURE; // no way to pass the scaling factor
  SmmBatch s = lowp_from_descriptor(k->desc, 1.f);
  s.batch = end - begin; s.sync = SYNC_NONE;
  const Residency where = classify(a, b, c);
  bool ok = where.device();
  if (ok && 0 != index_stride) {
    s.mode = ADDR_INDEX; s.index_base = index_base; s.index_stride = index_stride; s.a = a; s.b = b; s.c = c;
    s.ia = device_indexes(index_at(stride_a, begin, index_stride), index_stride, s.batch, &ok);
    s.ib = device_indexes(index_at(stride_b, begin, index_stride), index_stride, s.batch, &ok);
    s.ic = device_indexes(index_at(stride_c, begin, index_stride), index_stride, s.batch, &ok);
  }
  else if (ok) { // arrays of pointers in device-reachable memory
    s.mode = ADDR_POINTER;
    s.sa = pointer_step(stride_a, index_base); s.sb = pointer_step(stride_b, index_base); s.sc = pointer_step(stride_c, index_base);
    s.a = static_cast<const char*>(a) + s.sa * begin; s.b = static_cast<const char*>(b) + s.sb * begin; s.c = static_cast<char*>(c) + s.sc * begin;
  }
  if (!ok) {
    fprintf(stderr, "LIBXSMM-AMD ERROR: batches of low-precision products need operands the GPU can reach (libxsmm_malloc or device memory)\n");
    return EXIT_FAILURE;
  }
  const int le = lowp_launch(s);
  index_upload_commit();
  if (0 != le) return EXIT_FAILURE;
  if (ADDR_POINTER == s.mode || 0 != where.visible()) (void)stream_sync();
  return EXIT_SUCCESS;
}

int batch_order_env()
{
  static const int env = []() { const char* e = getenv("LIBXSMM_AMD_BATCH_ORDER"); return (nullptr == e || 0 == *e) ? 0 : (('r' == *e || 'R' == *e) ? 1 : -1); }();
  return env;
}

// Whether the products that share a C may be summed in any order. The reference's sequential entry points
// (libxsmm_gemm_batch, mmbatch with one task) add them in batch order; its multi-threaded ones (libxsmm_gemm_batch_omp,
// ?gemm_batch_omp, mmbatch with several tasks: a lock per C, src/libxsmm_gemm.c:1366-1423) in whatever order the threads
// arrive. Only the latter may be served by the segment/atomic form of the run kernels. LIBXSMM_AMD_BATCH_ORDER=relaxed
// (strict) overrides for all entry points. Floating-point atomics do not reach host memory: C the CPU addresses stays strict.
thread_local int tl_relaxed_order = 0;
bool relaxed_order(int ntasks, libxsmm_blasint index_stride, const void* c)
{
  const int env = batch_order_env();
  if (0 > env || (0 == env && ntasks <= 1 && 0 == tl_relaxed_order)) return false;
  const int kc = pointer_kind(c);
  if (0 != index_stride) return 0 == (kc & 2);
  if (1 == kc) return true; // device array of pointers: the matrices live on the device as well
  const void* const c0 = *static_cast<const void* const*>(c);
  return !is_host_visible(c0);
}

} // namespace xsmm
