// xsmm_batch_record.cpp -- the two recorders of the batch front end: the auto-batch of libxsmm_mmbatch_begin/end (per-call
// kernels collected into one pointer-array batch) and the record of libxsmm_gemm_batch calls inside a
// libxsmm_amd_defer_begin/end bracket (MergeRecord: record_batch_call, batch_flush_record). The address arithmetic is that
// of xsmm_batch.hpp, the launches those of xsmm_batch.cpp.
#include "xsmm_internal.hpp"
#include "xsmm_batch.hpp"

#include <cstring>
#include <mutex>

using namespace xsmm;

namespace {
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
} // namespace

namespace xsmm {

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

// true: the call was recorded and runs at the next flush. false: nothing was done, the call takes the ordinary path (which
// flushes the record on its way: it asks for the stream).
bool record_batch_call(const Kernel* k, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, libxsmm_blasint batchsize, int ntasks)
{
  if (!defer_bracket_open() || nullptr == k || KC_DENSE != k->kclass || 1 != ntasks || 0 == batchsize || !device_ready()) return false;
  const long long size = batch_size(batchsize);
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
    s.sa = pointer_step(stride_a, index_base); s.sb = pointer_step(stride_b, index_base); s.sc = pointer_step(stride_c, index_base);
    if (1 == ka && 1 == kb && 1 == kc) { s.a = a; s.b = b; s.c = c; on_device = true; } // device arrays: the matrices live on the device as well
    else if (host_readable(ka) && host_readable(kb) && host_readable(kc)) {
      ta.resize(pointer_count(s.sa, size)); tb.resize(pointer_count(s.sb, size)); tc.resize(pointer_count(s.sc, size));
      gather_pointers(ta, a, s.sa); gather_pointers(tb, b, s.sb); gather_pointers(tc, c, s.sc);
      const int k0 = pointer_kind(tc[0]); // (the first operand of each tells where the matrices live, as in batch_execute)
      if (0 == (pointer_kind(ta[0]) & pointer_kind(tb[0]) & k0 & 1) || 0 != (k0 & 2)) return false;
    }
    else return false;
  }
  s.batch = size; s.tasks = 1; s.c_atomics = 1;
  s.relaxed = relaxed_order(ntasks, index_stride, c) ? 1 : 0;
  s.sync = c_verdict_needed(0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0), batchsize) ? SYNC_DEVICE : SYNC_NONE;
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
    const void* const base[3] = { a, b, c };
    for (int o = 0; o < 3 && ok && !on_device; ++o) hull_of_indexes(hull + 2 * o, base[o], host_idx[o], index_stride, index_base, size, ts, span[o]);
  }
  else if (!on_device) {
    ok = upload_pointer_arrays(s, stream, ta.data(), ta.size(), tb.data(), tb.size(), tc.data(), tc.size());
    uploads = 3;
    const std::vector<const void*>* const tight[3] = { &ta, &tb, &tc };
    for (int o = 0; o < 3; ++o) hull_of_pointers(hull + 2 * o, tight[o]->data(), tight[o]->size(), ts, span[o]);
  }
  if (!ok) return false; // (entries a failed upload has filled: the ordinary path's commit releases them)
  r.uploads += uploads;
  r.calls.push_back(s); r.hulls.insert(r.hulls.end(), hull, hull + 6); r.on_device.push_back(on_device ? 1 : 0);
  return true;
}

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

} // namespace xsmm

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
  const libxsmm_blasint* const filter[6] = { m, n, k, lda, ldb, ldc }; int* const value[6] = { &r.m, &r.n, &r.k, &r.lda, &r.ldb, &r.ldc };
  for (int i = 0; i < 6; ++i) { r.have[i + 1] = (nullptr != filter[i]); if (r.have[i + 1]) *value[i] = *filter[i]; }
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
