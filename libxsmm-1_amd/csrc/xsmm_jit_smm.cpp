// xsmm_jit_smm.cpp -- dense SMM kernels specialised per descriptor with hiprtc (the gfx950 analogue of
// libxsmm_build's JIT, reference src/libxsmm_main.c:1246-1683: one kernel per (precision, M, N, K, flags)).
//
// The pre-compiled kernels in kernels/smm_generic.hip serve every descriptor; for large batches of small, tightly
// packed matrices (lda == m, ldb == k, ldc == m) a kernel with M, N, K baked in is generated at first use:
//   * one wavefront per item, walking the batch with a stride of all resident waves;
//   * A, B, C are fetched as flat, fully coalesced, non-temporal loads (the widest access the alignment of the item
//     size allows) one item ahead of the arithmetic, parked in wave-private LDS, and C leaves the same way;
//   * 8x8 lanes, TM x TN register tile, v_fma in ascending k: the reference's per-element chain, bit for bit.
#include "xsmm_internal.hpp"
#include "kernels/smm_jit_geom.h"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>
#include <string>
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace xsmm {

// The text of the generated kernels: each file of kernels/ below is linked in as a string (Makefile, TEXTS); gen_smm_source and
// gen_smm_grouped_source put the #define block of a shape in front and assemble the files in the order a form needs
extern const char* const SMM_MFMA_WG_SOURCE;       // smm_mfma_wg.inc: the matrix-core work-group kernels (also pre-compiled, kernels/smm_special.hip)
extern const char* const SMM_JIT_GEOM_SOURCE;      // smm_jit_geom.h: DevAddr and the LDS geometry, in front of every generated kernel
extern const char* const SMM_JIT_PRELUDE;          // smm_jit_prelude.inc: what does not depend on the shape
extern const char* const SMM_JIT_SHAPE;            // smm_jit_shape.inc: the part that depends on the shape (macros XM, XN, XK, ...); XGROUPED: instantiated once per shape inside a namespace
extern const char* const SMM_JIT_CHAIN;            // smm_jit_chain.inc: walking a batch run by run (register-tiled and matrix-core run forms): needs T, DevAddr / resolve, XRUNS, XSPLIT, XDEPTH
extern const char* const SMM_JIT_SHAPE_KERNELS;    // smm_jit_shape_kernels.inc: the register-tiled kernels (streaming, wave runs, work-group runs)
extern const char* const SMM_JIT_MFMA_WAVE_BODY;   // smm_jit_mfma_wave.inc: 32 < max(M, N) <= 64 on the matrix cores, one wave per item
extern const char* const SMM_JIT_MFMA_RUNS_CONST;  // smm_jit_mfma_runs_const.inc: run and streaming forms on the matrix cores (M, N <= 32), the constants ...
extern const char* const SMM_JIT_MFMA_RUNS_KERNEL; // smm_jit_mfma_runs.inc: ... and, behind SMM_JIT_CHAIN, the kernels
extern const char* const SMM_JIT_BIG_BODY;         // smm_jit_big.inc: 32 < M or N <= 64, a work-group per item, K in chunks (behind the prelude with XFLAT 0)

namespace {

// A developer knob: the number in environment variable `name`, `dflt` if it is unset or empty. Most knobs are read once, into a
// static at the one place that uses them; those that tests and tools toggle inside a process are read on every call.
static long long knob(const char* name, long long dflt)
{
  const char* const e = getenv(name);
  return (nullptr != e && 0 != *e) ? atoll(e) : dflt;
}

// LDS bytes of a wave of that kernel (geom::mfma_wave, as the kernel lays them out); 0: the shape is not served
static size_t smm_mfma_wave_lds(int typesize, int m, int n, int k, int vec = 0, bool transb = false) // vec: elements per memory access (0: a 16-byte chunk)
{ return (size_t)geom::mfma_wave(typesize, m, n, k, (0 == vec) ? 16 / typesize : vec, transb).lds_bytes; }
// ... of the form that works on the columns of C in two halves (0: not served)
static size_t smm_mfma_wave2_lds(int typesize, int m, int n, int k) { return (size_t)geom::mfma_wave2(typesize, m, n, k).lds_bytes; }
// waves per SIMD the kernel is compiled for: two where LDS leaves room for eight waves per CU, else one (the register file
// then holds an item's operands, the next item's and the accumulators without spilling)
static int smm_mfma_wave_wpe(size_t lds, int typesize = 0, int m = 0, int n = 0, int k = 0, int vec = 0, int lda = 0, int ldb = 0, int ldc = 0)
{
  if (lda < m) lda = m;
  if (ldb < k) ldb = k;
  if (ldc < m) ldc = m;
  static const int env = (int)knob("XSMM_SMMJIT_WAVE_WPE", 0);
  if (0 < env) return env;
  if (8 * lds > 160u * 1024u) return 1;
  if (1 == vec) { // element-wise form: a register per element in flight plus what parking them costs (45^3 fp32 spills at two waves per SIMD)
    const int w = typesize / 4, regs = w * ((lda * (k - 1) + m + 63) / 64 + (ldb * (n - 1) + k + 63) / 64 + (ldc * (n - 1) + m + 63) / 64) + w * 4 * ((m + 15) / 16) * ((n + 15) / 16);
    if (regs > 125) return 1;
  }
  return 2;
}

// ---- the run form on the matrix cores (SMM_JIT_MFMA_RUNS_*): LDS bytes of a wave (geom::mfma_runs); 0: shape not served
static size_t smm_mfma_runs_lds(int typesize, int m, int n, int k, int ldb, bool stream = false) // stream: the streaming form (every item owns its C)
{ return (size_t)geom::mfma_runs_lds_bytes(typesize, m, n, k, ldb, stream); }
// products in flight per wave (register sets): as many as fit ~80 registers, four at most
static int smm_mfma_runs_depth(int typesize, int m, int n, int k, int ldb, bool deep = false)
{ // deep: the tiles of a batch of few runs (smm_tile_split) -- a wave or two per SIMD, the registers are there
  static const int env = (int)knob("XSMM_SMMJIT_MFMA_RUNS_DEPTH", 0);
  if (0 < env) return env > 4 ? 4 : env;
  if (ldb < k) ldb = k;
  const int regs = (typesize / 4) * (((k + 3) / 4) * ((m + 15) / 16) + (ldb * (n - 1) + k + 63) / 64);
  const int d = (deep ? 128 : 80) / (regs > 0 ? regs : 1);
  return d < 1 ? 1 : (d > 4 ? 4 : d);
}
// hand-counted waits in the software pipeline of the run form (XSMM_SMMJIT_HANDWAIT=0: the compiler's: developer knob)
static int smm_mfma_handwait()
{
  static const int env = (int)knob("XSMM_SMMJIT_HANDWAIT", 1);
  return 0 != env ? 1 : 0;
}
// XSMM_SMMJIT_TILESPLIT=2 (developer knob, re-read on every call): the tiles of a run as the waves of ONE work-group instead of work-groups
// of one wave wherever the dispatcher puts them. Measured (profiles/r3_tile_split.txt): the tiles then share a CU's memory pipeline -- 10-20 %
// faster for batches of 16 000-30 000 items in short runs (the halves of A and B two tiles share are requested from one CU), but a long run
// is walked SLOWER than by a single wave (runs of 256: 0.41 ms against 0.18 ms for the tiles as groups and 0.31 ms for a wave per run; one
// CP2K stack 0.19 against 0.14 ms): not the default.
// (0: the tiles of a batch of few runs are not split off at all, smm_tile_split)
static int smm_tilesplit() { return (int)knob("XSMM_SMMJIT_TILESPLIT", 1); }
static int smm_mfma_runs_waves(size_t lds) { return (0 == lds) ? 0 : ((4 * lds <= 65536) ? 4 : ((2 * lds <= 65536) ? 2 : 1)); }
// may batch s take that form? stream: the streaming form (items that own their C; K up to 256), else the run form (shared C)
static bool smm_mfma_runs_ok(const SmmBatch& s, bool stream = false)
{
  static const int on = (int)knob("XSMM_SMMJIT_MFMA_RUNS", 1);
  if (0 == on || 0 == s.use_mfma || 0 != s.lowp || 0 != s.general || 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) || (stream && SYNC_NONE != s.sync)) return false;
  if (s.lda < s.m || s.ldb < s.k || s.ldc < s.m) return false;
  return 0 != smm_mfma_runs_lds(s.typesize, s.m, s.n, s.k, s.ldb, stream);
}

struct SmmKey {
  int typesize, m, n, k, flags, variant, lda, ldb, ldc;
  bool operator==(const SmmKey& o) const { return typesize == o.typesize && m == o.m && n == o.n && k == o.k && flags == o.flags && variant == o.variant
                                               && lda == o.lda && ldb == o.ldb && ldc == o.ldc; }
};
struct SmmKeyHash { size_t operator()(const SmmKey& k) const { return (size_t)(((((k.m * 131 + k.n) * 131 + k.k) * 8 + k.flags * 2 + (k.typesize == 8)) * 64 + k.variant) * 31 + k.lda * 7 + k.ldb * 3 + k.ldc); } };

// A specialised kernel is absent (never asked for), being compiled on the helper thread, ready, or failed (not retried).
struct JitSlot { int state; JitKernel* kernel; }; // state 0: compiling, 1: ready, 2: failed
std::mutex g_smm_lock;
std::unordered_map<SmmKey, JitSlot, SmmKeyHash> g_smm_cache;

// The kernel for `key`: from the table, else from the code-object cache on disk (milliseconds), else from the compiler -- on
// the helper thread (nullptr now: the caller falls back to the next best kernel, a later call finds this one ready) unless
// LIBXSMM_AMD_JIT_ASYNC=0 or `wait`.
template<typename KEY, typename MAP, typename GEN>
JitKernel* jit_resolve(MAP& table, const KEY& key, const char* fname, bool wait, GEN gen_source)
{
  {
    std::lock_guard<std::mutex> guard(g_smm_lock);
    auto it = table.find(key);
    if (it != table.end()) return (1 == it->second.state) ? it->second.kernel : nullptr;
    table.emplace(key, JitSlot{ 0, nullptr }); // this caller is in charge of it
  }
  const std::string src = gen_source();
  auto publish = [&table, key](JitKernel* k) {
    std::lock_guard<std::mutex> guard(g_smm_lock);
    JitSlot& slot = table[key];
    slot.kernel = k; slot.state = (nullptr != k ? 1 : 2);
  };
  JitKernel* k = jit_from_cache(src, fname);
  if (nullptr != k) { publish(k); return k; }
  auto compile = [src, fname, publish]() {
    std::string log;
    JitKernel* const kk = jit_compile(src, fname, &log);
    if (nullptr == kk && 0 != verbosity()) fprintf(stderr, "LIBXSMM WARNING: SMM JIT failed (%s); using the pre-compiled kernel\n", log.c_str());
    publish(kk);
    return kk;
  };
  if (wait || !jit_async_enabled()) return compile();
  jit_async([compile]() { (void)compile(); });
  return nullptr;
}

} // namespace

static int smm_jit_waves(int typesize, int m, int n, int k, int flags, int pack = 1, bool runs = false);

// k-chunk of the work-group-per-item form: the largest of 32/16/8 whose two LDS buffers fit 64 KiB (0: none does)
static size_t smm_jit_big_buf(int typesize, int m, int n, int kc) { return (size_t)geom::big(typesize, m, n, kc).buf * typesize; }
static int smm_jit_big_kc(int typesize, int m, int n, int k)
{
  for (int kc = 32; kc >= 8; kc /= 2) {
    if (kc / 2 >= k && kc > 8) continue; // a shorter chunk already covers K
    if (2 * smm_jit_big_buf(typesize, m, n, kc) <= 65536) return kc;
  }
  return 0;
}

// Products whose operands a run kernel keeps in flight (register stages). Measured on CP2K stacks (MI355X): once the
// per-item index loads are off the critical path (address windows) a run is bound by its on-chip work per product, not by
// the HBM round trip -- depths 2 and 4 were no faster (work-group form) or slower (wave form: register pressure).
// The ring stays in the source as a developer knob (XSMM_SMMJIT_DEPTH).
static int smm_jit_depth(int typesize, int m, int n, int k, int variant)
{
  if (0 == (variant & (SMM_JIT_RUNS | SMM_JIT_WGRUNS))) return 1;
  static const int env = (int)knob("XSMM_SMMJIT_DEPTH", 0);
  static const int env_bytes = (int)knob("XSMM_SMMJIT_DEPTH_BYTES", 0); // (only products up to this many operand bytes)
  if (0 < env_bytes && (long long)typesize * ((long long)m * k + (long long)k * n) > env_bytes) return 1;
  return (0 < env && env <= 8) ? env : 1;
}

// items per wave pass, encoded in the variant as log2 << 8
static int smm_jit_pack_of(int variant) { return 1 << ((variant >> 8) & 7); }
static int smm_jit_pack_bits(int pack) { int l = 0; while ((1 << l) < pack) ++l; return l << 8; }

// The #define block of one kernel body: the macros the texts of kernels/ read, (name, value) in the order of the lines.
struct SmmMacros {
  std::vector<std::pair<std::string, std::string>> defs;
  void set(const std::string& name, long long value) // (a name that is set again keeps its place and takes the new value)
  {
    for (auto& d : defs) if (d.first == name) { d.second = std::to_string(value); return; }
    defs.emplace_back(name, std::to_string(value));
  }
  std::string lines(const char* directive, bool values) const
  {
    std::string s;
    for (const auto& d : defs) s += std::string(directive) + " " + d.first + (values ? " " + d.second : std::string()) + "\n";
    return s;
  }
};

// The one place that turns (typesize, shape, flags, variant, leading dimensions) into macros, for the text of one kernel and for a body
// of a grouped text alike. body: one of several bodies in namespaces of their own -- what such a text defines once at file scope, in
// front of the prelude, is left to its builder (XLOWP, XFLAT, XGROUPED, XTILEWG).
static SmmMacros smm_macro_block(int typesize, int m, int n, int k, int flags, int variant, int lda, int ldb, int ldc, bool body)
{
  SmmMacros d;
  const bool transb = (0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_B));
  int flat = 0; // address space of the operand accesses: global, but see the streaming form below
  d.set("XM", m); d.set("XN", n); d.set("XK", k);
  d.set("XBETA0", (flags & LIBXSMM_GEMM_FLAG_BETA_0) ? 1 : 0);
  d.set("XTRANSB", transb ? 1 : 0);
  d.set("XLDA", lda); d.set("XLDB", ldb); d.set("XLDC", ldc); // leading dimensions in memory (the tight forms below: their own)
  if (0 != (variant & SMM_JIT_MFMA_RUNS)) { // run form on the matrix cores (a wave per run); without the run bit: every item owns its C
    const bool stream = (0 == (variant & SMM_JIT_RUNS));
    d.set("XWAVES", smm_mfma_runs_waves(smm_mfma_runs_lds(typesize, m, n, k, ldb, stream)));
    d.set("XRUNS", 1);
    d.set("XSTREAM", stream ? 1 : 0);
    d.set("XHANDWAIT", smm_mfma_handwait());
    d.set("XDEPTH", smm_mfma_runs_depth(typesize, m, n, k, ldb, 0 != (variant & SMM_JIT_DEEP)));
    d.set("XSPLIT", (variant & SMM_JIT_SPLIT) ? 1 : 0);
  }
  else if (0 != (variant & SMM_JIT_MFMA_WAVE2)) { // matrix-core kernel, one wave per item, the columns of C in two halves (tight operands)
    d.set("XLDA", m); d.set("XLDB", k); d.set("XLDC", m);
    d.set("XWPE", 1); d.set("XNSPLIT", 2); d.set("XVEC", 16 / typesize);
  }
  else if (0 != (variant & SMM_JIT_MFMA_WAVE)) { // matrix-core kernel, one wave per item
    const int wvec = (0 != (variant & SMM_JIT_SCALAR)) ? 1 : 16 / typesize;
    if (1 != wvec) { d.set("XLDA", m); d.set("XLDB", transb ? n : k); d.set("XLDC", m); }
    d.set("XNSPLIT", 1); d.set("XVEC", wvec);
    d.set("XWPE", smm_mfma_wave_wpe(smm_mfma_wave_lds(typesize, m, n, k, wvec, transb), typesize, m, n, k, wvec, lda, transb ? 0 : ldb, ldc));
  }
  else if (0 != (variant & SMM_JIT_MFMA)) { // matrix-core work-group kernel (kernels/smm_mfma_wg.inc), shape and leading dimensions baked in
    d.set("XMW_JIT", 1);
    d.set("XTIGHT", (variant & SMM_JIT_MFMA_TIGHT) ? 1 : 0);
    d.set("XTIGHTC", (variant & SMM_JIT_MFMA_TIGHTC) ? 1 : 0);
    d.set("XMW_FORM", 8 == typesize ? (k > 32 ? 2 : 1) : 0);
  }
  else if (0 != (variant & SMM_JIT_BIG)) d.set("XKC", smm_jit_big_kc(typesize, m, n, k)); // work-group per item, K chunked
  else { // the register-tiled forms
    const int pack = smm_jit_pack_of(variant);
    static const int defer_env = (int)knob("XSMM_SMMJIT_DEFER", 1); // deferred stores of the streaming form
    const bool wave_runs = (0 != (variant & SMM_JIT_RUNS) && 0 == (variant & SMM_JIT_WGRUNS)); // (the wave run form keeps C's image over the operands')
    d.set("XPACK", pack); // items per wave pass (streaming form of tight strided batches)
    d.set("XWAVES", smm_jit_waves(typesize, m, n, k, flags, pack, wave_runs));
    d.set("XSCALAR", (variant & SMM_JIT_SCALAR) ? 1 : 0); // element-wide loads/stores only
    // runs of equal C accumulate in registers: 1 = a wave per run, 2 = a work-group per run (long runs)
    d.set("XRUNS", (variant & SMM_JIT_WGRUNS) ? 2 : ((variant & SMM_JIT_RUNS) ? 1 : 0));
    { // global for the run forms; the streaming (one wave per item) form measured faster with generic pointers, i.e. FLAT
      // instructions (f64 13^3: 60.7 vs 55.3 %, the fp32 32^3 kernels 72.5 vs 69 %)
      static const int flat_env = (int)knob("XSMM_SMMJIT_FLAT", -1);
      // (with the stores deferred the global form is the faster one: tools/sweep_defer.sh, profiles/r2_sweep_defer.txt)
      flat = (0 <= flat_env) ? (0 != flat_env ? 1 : 0) : ((0 != (variant & (SMM_JIT_RUNS | SMM_JIT_WGRUNS)) || 0 != defer_env) ? 0 : 1);
    }
    d.set("XDEPTH", smm_jit_depth(typesize, m, n, k, variant)); // register stages of the run forms
    d.set("XSPLIT", (variant & SMM_JIT_SPLIT) ? 1 : 0); // relaxed order: few long runs are cut into segments (atomics)
    d.set("XHASWG", (variant & SMM_JIT_HASWG) ? 1 : 0); // wave form: leave long runs to the work-group form
    d.set("XDEFER", defer_env ? 1 : 0);
  }
  if (!body) {
    d.set("XLOWP", (variant >> 11) & 3); // 16-bit inputs: 1 = i16 -> i32, 2 = bf16 -> bf16, 3 = bf16 -> f32 (0: none)
    d.set("XFLAT", flat); d.set("XGROUPED", 0); d.set("XTILEWG", 0);
  }
  return d;
}

// The text of one kernel: the macro block, then kernels/smm_jit_geom.h and the prelude, then the files of the variant's form
std::string gen_smm_source(int typesize, int m, int n, int k, int flags, int variant, int lda, int ldb, int ldc)
{
  if (lda <= 0) lda = m;
  if (ldb <= 0) ldb = (flags & LIBXSMM_GEMM_FLAG_TRANS_B) ? n : k;
  if (ldc <= 0) ldc = m;
  std::string s = "// generated by libxsmm-amd (dense SMM kernel, shape baked in)\n";
  s += std::string("typedef ") + (8 == typesize ? "double" : (1 == ((variant >> 11) & 3) ? "int" : "float")) + " T;\n";
  s += smm_macro_block(typesize, m, n, k, flags, variant, lda, ldb, ldc, false).lines("#define", true);
  s += SMM_JIT_GEOM_SOURCE; s += SMM_JIT_PRELUDE;
  if (0 != (variant & SMM_JIT_MFMA_RUNS)) { s += SMM_JIT_MFMA_RUNS_CONST; s += SMM_JIT_CHAIN; s += SMM_JIT_MFMA_RUNS_KERNEL; }
  else if (0 != (variant & (SMM_JIT_MFMA_WAVE2 | SMM_JIT_MFMA_WAVE))) s += SMM_JIT_MFMA_WAVE_BODY;
  else if (0 != (variant & SMM_JIT_MFMA)) s += SMM_MFMA_WG_SOURCE;
  else if (0 != (variant & SMM_JIT_BIG)) s += SMM_JIT_BIG_BODY;
  else { s += SMM_JIT_SHAPE; s += SMM_JIT_CHAIN; s += SMM_JIT_SHAPE_KERNELS; }
  return s;
}

// LDS bytes one wave of the generated kernel needs (geom::tiled)
static size_t smm_jit_wave_lds(int typesize, int m, int n, int k, int flags, int pack = 1, bool runs = false) // runs: the wave run form (XRUNS 1)
{ return (size_t)geom::tiled(typesize, m, n, k, 0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_B), pack, runs ? 1 : 0).wave_lds * typesize; }

// wavefronts per work-group: as many (4, 2, 1) as fit 64 KiB of static LDS; 0 if even one wave does not fit
static int smm_jit_waves(int typesize, int m, int n, int k, int flags, int pack, bool runs)
{
  const size_t w = smm_jit_wave_lds(typesize, m, n, k, flags, pack, runs);
  return (4 * w <= 65536) ? 4 : ((2 * w <= 65536) ? 2 : ((w <= 65536) ? 1 : 0));
}

// LIBXSMM_AMD_JIT=0: no specialised dense kernel (read on every call: tests and tools toggle it)
static bool smm_jit_enabled()
{
  const char* const e = getenv("LIBXSMM_AMD_JIT");
  return nullptr == e || 0 != atoi(e);
}
// smallest batch that is specialised unless the caller asks for it (read on every call: tests set it)
static long long smm_jit_min_batch() { return knob("LIBXSMM_AMD_JIT_MINBATCH", 16); }

bool smm_jit_eligible(const SmmBatch& s)
{
  if (!smm_jit_enabled() || 0 != s.general || SYNC_ATOMIC == s.sync) return false;
  if (SYNC_NONE != s.sync && 0 != (s.flags & LIBXSMM_GEMM_FLAG_BETA_0)) return false; // (never chosen: beta == 0 needs no care)
  if (SYNC_DEVICE == s.sync && 0 == s.c_atomics) return false;  // C in host memory the GPU maps: the generic kernel adds by compare-and-swap (cas_add, kernels/smm_generic.hip)
  const bool tight = (s.lda == s.m && s.ldc == s.m && (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) ? (s.ldb == s.n) : (s.ldb == s.k)));
  if (!tight) { // leading dimensions with gaps: the wave forms fetch an operand's whole span -- as long as the gaps stay moderate
    if (s.m > 32 || s.n > 32 || (s.k > 64 && !smm_mfma_runs_ok(s, true))) return false;
    const long long span = (long long)s.lda * (s.k - 1) + s.m + (long long)s.ldb * ((0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) ? s.k : s.n) - 1)
                         + (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) ? s.n : s.k) + (long long)s.ldc * (s.n - 1) + s.m;
    const long long used = (long long)s.m * s.k + (long long)s.k * s.n + (long long)s.m * s.n;
    if (2 * used < span) return false;
    if (span * s.typesize > 40960 && !(s.k > 64 && smm_mfma_runs_ok(s, true))) return false; // (a long K in chunks: no whole operand is ever on chip)
  }
  if (s.m <= 32 && s.n <= 32 && s.k > 64 && smm_mfma_runs_ok(s, true)) { /* the matrix-core streaming form takes K in chunks of up to 64 */ }
  else if (s.m > 32 || s.n > 32 || s.k > 64) { // work-group-per-item form: 16x16 threads x (<=4x4) tile, K chunked (also small M, N with a long K)
    if (s.m > 64 || s.n > 64 || s.k > 1024) return false;
    if (SYNC_NONE != s.sync && !(0 < s.uniform_run && 0 == s.batch % s.uniform_run)) return false; // shared C only as runs of a known, uniform length
    if (0 == smm_jit_big_kc(s.typesize, s.m, s.n, s.k)) return false;
  }
  else {
    if (s.k > 64) return false;                                                // 8x8 lanes x (<=4x4) tile, whole K in LDS
    if (0 == smm_jit_waves(s.typesize, s.m, s.n, s.k, s.flags)) return false; // static LDS limit per work-group
  }
  // (the compiler works on a helper thread and its output is kept on disk, so a small batch is enough of a reason: the
  // specialised kernel is the faster one at every size measured -- fp64 23^3: 7.9 vs 12.2 us at 32 items, 8.4 vs 13.5 us at 1024,
  // 50 vs 77 us at 16 384; tools/bench_small_batches.py, profiles/r3_small_batches.txt)
  return s.batch >= smm_jit_min_batch() || 0 != s.jit_always;
}

// the work-group form (XRUNS 2) of a shape: wg_buf elements per operand buffer, wg_nbuf of them
static geom::Tiled smm_jit_wg(int typesize, int m, int n, int k, int flags) { return geom::tiled(typesize, m, n, k, 0 != (flags & LIBXSMM_GEMM_FLAG_TRANS_B), 1, 2); }

// Which flavour of the generated kernel a batch needs: strided batches of tightly packed items whose bases are 16-byte
// aligned use the widest loads the item size allows; index/pointer batches (and anything else) are only known to be
// element-aligned.
static int smm_jit_width_variant(const SmmBatch& s)
{
  bool wide = false;
  if (ADDR_STRIDED == s.mode) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(s.a) | reinterpret_cast<uintptr_t>(s.b) | reinterpret_cast<uintptr_t>(s.c);
    wide = (0 == (bits & 15))
        && (s.sa == (long long)s.m * s.k || 0 == s.sa) && (s.sb == (long long)s.k * s.n || 0 == s.sb)
        && (s.sc == (long long)s.m * s.n || 0 == s.sc);
  }
  return wide ? 0 : SMM_JIT_SCALAR;
}

static JitKernel* smm_jit_get(const SmmKey& key, bool wait = false)
{
  return jit_resolve(g_smm_cache, key, "xsmm_smm_op", wait, [&key]() {
    return gen_smm_source(key.typesize, key.m, key.n, key.k, key.flags, key.variant, key.lda, key.ldb, key.ldc); });
}

// ---- one launch of a generated kernel ----------------------------------------------------------------------------------
// DevAddr (kernels/smm_jit_geom.h: the one struct host and kernels compile), the first argument of every generated kernel
static DevAddr dev_addr(const SmmBatch& s)
{
  DevAddr ad;
  memset(&ad, 0, sizeof(ad));
  ad.a = (const char*)s.a; ad.b = (const char*)s.b; ad.c = (char*)s.c; ad.ia = (const char*)s.ia; ad.ib = (const char*)s.ib; ad.ic = (const char*)s.ic;
  ad.sa = s.sa; ad.sb = s.sb; ad.sc = s.sc; ad.index_base = s.index_base; ad.index_stride = s.index_stride; ad.mode = s.mode;
  ad.flags = (SYNC_DEVICE == s.sync ? s.devflags : nullptr); // the device-side verdict, read by the run forms
  return ad;
}

// work-groups per CU: as many as leave each `lds` bytes of the 160 KiB, `cap` at most, one at least
static long long smm_per_cu(size_t lds, long long cap)
{
  const long long per_cu = (long long)((160 * 1024) / (lds ? lds : 1));
  return per_cu > cap ? cap : (per_cu < 1 ? 1 : per_cu);
}

// Grid, work-group, dynamic LDS and third kernel argument of a launch of the generated kernel `variant` over batch s. The grids
// are persistent: at most 256 CUs times the work-groups per CU, each walks the batch with a stride of the grid.
struct SmmGeom { long long blocks; unsigned threads, lds; long long runlen; bool runlen64; };
static SmmGeom smm_jit_geometry(const SmmBatch& s, int variant, JitKernel* k)
{
  static const int bpc_env = (int)knob("XSMM_SMMJIT_BPC", 0);
  SmmGeom g = { 0, 256u, 0u, 1, false };
  const bool verdict = (SYNC_DEVICE == s.sync && nullptr != s.devflags);
  long long units = s.batch, per_cu = 1; // units: work-groups without the cap
  if (0 != (variant & SMM_JIT_BIG)) { // one work-group per item (per run of uniform length)
    per_cu = smm_per_cu(2 * smm_jit_big_buf(s.typesize, s.m, s.n, smm_jit_big_kc(s.typesize, s.m, s.n, s.k)), 4);
    // a persistent grid must not exceed what is resident: a work-group that starts after the others have finished their
    // share is pure tail (measured: f64 64^3 with 150 VGPRs fits 3 per CU; a grid of 4 per CU loses 12 %)
    const int occ = jit_blocks_per_cu(k, 256);
    if (0 < occ && occ < per_cu) per_cu = occ;
    if (0 < bpc_env) per_cu = bpc_env;
    g.runlen = (0 < s.uniform_run ? s.uniform_run : 1); g.runlen64 = true;
    units = s.batch / g.runlen;
  }
  else if (0 != (variant & SMM_JIT_WGRUNS)) { // work-groups of 256 threads, dealt chunks of 64 items
    const geom::Tiled wg = smm_jit_wg(s.typesize, s.m, s.n, s.k, s.flags);
    per_cu = smm_per_cu((size_t)wg.wg_nbuf * wg.wg_buf * s.typesize, 4);
    if (0 < bpc_env) per_cu = bpc_env;
    units = (s.batch + 63) / 64;
  }
  else if (0 != (variant & SMM_JIT_MFMA_RUNS)) { // a wave per run on the matrix cores, dealt chunks of 64 items (segments of 8 and more if the verdict cuts the batch up)
    const bool stream_form = (0 == (variant & SMM_JIT_RUNS)); // every item owns its C: a wave per item, stride of the resident waves
    const size_t wlds = smm_mfma_runs_lds(s.typesize, s.m, s.n, s.k, s.ldb, stream_form);
    const int waves = smm_mfma_runs_waves(wlds);
    per_cu = smm_per_cu(wlds * (size_t)waves, 16 / waves);
    if (stream_form) { const int occ = jit_blocks_per_cu(k, 64 * waves); if (0 < occ && occ < per_cu) per_cu = occ; } // (a persistent grid must not exceed what is resident)
    if (0 < bpc_env) per_cu = bpc_env;
    g.threads = 64u * (unsigned)waves;
    units = ((stream_form ? s.batch : (verdict ? (s.batch + 7) / 8 : (s.batch + 63) / 64)) + waves - 1) / waves;
  }
  else if (0 != (variant & SMM_JIT_MFMA_WAVE)) { // one wave per item on the matrix cores
    const bool transb = (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B)), wide = (0 == (variant & SMM_JIT_SCALAR));
    const int vec = wide ? 16 / s.typesize : 1;
    const size_t wlds = smm_mfma_wave_lds(s.typesize, s.m, s.n, s.k, vec, transb);
    g.threads = 64u; g.lds = (unsigned)wlds;
    if (0 != ((variant >> 11) & 3)) { // 16-bit inputs: eight waves per CU (tools/bench_dense.py lowp, XSMM_SMMJIT_WAVE_PERCU sweep, % of the HBM peak
      // at 8 / as many as LDS and registers allow: bf16 -> f32 48^3 70.5 / 67.4, 64^3 74.4 / 67.7; bf16 -> bf16 32^3 73.5 / 67.6, 48^3 73.5 / 62.5,
      // 64^3 60.3 / 54.7; three or four -- the optimum of the fp32 / fp64 wave kernels -- lose 5-30 points here: the widening and rounding
      // work per item wants more waves to overlap with) -- also where fewer fit: whatever is not resident at once starts as the others finish
      per_cu = 8;
    }
    else {
      const int by_regs = 4 * smm_mfma_wave_wpe(wlds, s.typesize, s.m, s.n, s.k, vec, s.lda, s.ldb, s.ldc);
      per_cu = smm_per_cu(wlds, by_regs);
      // The memory system is at its best with ~100 KB of operands in flight per CU (the fp32 32^3 kernel: twelve waves of 12 KB); a wave
      // here has a whole item of 19-55 KB in flight. Waves per CU, % of the HBM peak (tools/bench_dense.py, XSMM_SMMJIT_WAVE_PERCU sweep):
      // f32 40^3 3: 71.8, 4: 73.8, 8: 67.9, 12: 67.5 | f64 40^3 3: 72.2, 4: 69.3, 8: 69.0 | f32 48^3 3: 72.9, 4: 70.3, 8: 68.3 |
      // f64 48^3 3: 68.8, 8: 69.1, 12: 69.7 | f32 56^3 3: 69.8, 4: 68.6, 8: 67.6; five to seven waves (uneven over the four SIMDs) lose 3-15 points.
      const size_t item_bytes = (size_t)s.typesize * ((size_t)s.lda * s.k + (size_t)s.ldb * (transb ? s.k : s.n) + (size_t)s.ldc * s.n);
      if (wide && item_bytes >= 16384) { per_cu = (100u * 1024u / item_bytes >= 4) ? 4 : 3; if (per_cu > by_regs) per_cu = by_regs; }
    }
    const long long percu_env = knob("XSMM_SMMJIT_WAVE_PERCU", 0); // (read on every call)
    if (0 < percu_env) per_cu = percu_env;
  }
  else if (0 != (variant & SMM_JIT_MFMA_WAVE2)) { // ... the columns of C in two halves: four waves per CU
    g.threads = 64u; g.lds = (unsigned)smm_mfma_wave2_lds(s.typesize, s.m, s.n, s.k);
    per_cu = 4;
  }
  else if (0 != (variant & SMM_JIT_MFMA)) { // matrix-core work-group kernel: an item (a run of uniform length) per work-group
    static const int bpc64_env = (int)knob("XSMM_SMM64_BPC", 0);
    per_cu = (0 != (variant & SMM_JIT_MFMA_TIGHTC)) ? 3 : 4; // (48 KiB of LDS with the C image: three work-groups per CU)
    if (8 == s.typesize) { // (the sizes of the pre-compiled launch, kernels/smm_special.hip)
      g.lds = (unsigned)((s.k > 32) ? (size_t)2 * 32 * 64 * sizeof(double) : (size_t)2 * (4 * ((s.k + 3) / 4)) * 64 * sizeof(double));
      per_cu = smm_per_cu(g.lds, 3);
    }
    if (0 < bpc64_env) per_cu = bpc64_env;
    units = s.batch; // (the plan offers this kernel to independent items only: runs of one)
  }
  else { // the register-tiled streaming and wave run forms: work-groups of up to four waves
    const int pack = smm_jit_pack_of(variant);
    const bool wave_runs = (0 != (variant & SMM_JIT_RUNS));
    const int waves = smm_jit_waves(s.typesize, s.m, s.n, s.k, s.flags, pack, wave_runs);
    per_cu = smm_per_cu((size_t)waves * smm_jit_wave_lds(s.typesize, s.m, s.n, s.k, s.flags, pack, wave_runs), 16 / waves); // (the streaming rate peaks around 12-16 waves per CU)
    if (0 < bpc_env) per_cu = bpc_env;
    g.threads = 64u * (unsigned)waves;
    // run form: a wave scans chunks of 64 items for run heads, so the grid is sized by chunks
    // (the verdict is on the device: segments of 8 items and more if the batch is cut up -- waves without a chunk leave at once)
    units = ((wave_runs ? (verdict ? (s.batch + 7) / 8 : (s.batch + 63) / 64) : s.batch) + waves - 1) / waves;
  }
  g.blocks = (units > 256 * per_cu) ? 256 * per_cu : units;
  if (g.blocks < 1) g.blocks = 1;
  return g;
}

// one launch of kernel k (the generated kernel `variant`) over batch s
static int smm_jit_launch(const SmmBatch& s, int variant, JitKernel* k, void* stream)
{
  DevAddr ad = dev_addr(s);
  long long batch = s.batch;
  SmmGeom g = smm_jit_geometry(s, variant, k);
  int runlen = (int)g.runlen;
  void* args[] = { &ad, &batch, g.runlen64 ? (void*)&g.runlen : (void*)&runlen }; // (kernels of two arguments read two)
  return jit_launch_dyn(k, (unsigned)g.blocks, g.threads, g.lds, args, stream);
}

// Items a wave handles at a time. Only for batches laid out back to back (strided, tight, the "wide" flavour): a small or
// oddly sized item (5^3 doubles are 1000 bytes, 13^3 are 1352) leaves most of a wave's lanes and of every load instruction
// idle. Developer knob: XSMM_SMMJIT_PACK.
static int smm_jit_pack(const SmmBatch& s, int width)
{
  static const int env = (int)knob("XSMM_SMMJIT_PACK", 0);
  if (0 != width || ADDR_STRIDED != s.mode || 0 == s.sa || 0 == s.sb || 0 == s.sc) return 1;
  int pack = 1;
  if (0 < env) pack = env;
  else { // measured on MI355X (tools/bench_dense.py, XSMM_SMMJIT_PACK sweep): items of 6 KB and more gain nothing; below, as
    // many as make up 16 KB -- f64 5^3: 22 -> 69 % of the HBM peak, 8^3: 43 -> 72 %, 13^3: 61 -> 67 %; f32 5^3: 13 -> 58 %, 8^3: 25 -> 72 %
    const size_t item = ((size_t)s.m * s.k + (size_t)s.k * s.n + (size_t)s.m * s.n) * s.typesize;
    if (item < 6000) while (pack < 16 && 2 * pack * item <= 16384) pack *= 2;
    // items up to ~13 KB that do not end on a 128-byte line: two at a time, so that a line is not fetched by two waves (with
    // deferred stores, profiles/r2_sweep_pack.txt: f32 23^3 62.1 -> 63.4 %, f32 13x23x32 61.2 -> 63.6 %, f64 13x23x32 65.1 -> 66.5 %)
    else if (item < 14000 && 0 != item % 128) pack = 2;
  }
  if (pack > 16) pack = 16;
  while (0 != (pack & (pack - 1))) --pack; // power of two
  // operands of `pack` items in flight per lane (registers) and in LDS
  while (1 < pack && ((size_t)pack * ((size_t)s.m * s.k + (size_t)s.k * s.n + (size_t)s.m * s.n) * s.typesize > 28672
                   || 0 == smm_jit_waves(s.typesize, s.m, s.n, s.k, s.flags, pack))) pack /= 2;
  return pack;
}

// ---- one launch for several batches (CP2K-style stacks: a batch per shape) -----------------------------------------------
// A batch of few long runs leaves the chip nearly empty (one sequential chain per C block: 172 chains per shape in the
// per-GPU share of BASELINE config 5), and batches issued one after the other on a stream run one after the other. Here
// the run kernels of all batches of a call become ONE kernel: the shape-dependent part of the generated source is
// instantiated once per (shape, form) in a namespace of its own, a dispatcher maps every work-group to its batch by its
// index (a small table in device memory: addressing, batch size, first work-group, which body) and calls that body -- all
// chains of all shapes are resident at the same time. Same code per shape as the single-batch kernels, same chains, same
// bits; one verdict slot per batch (fused check kernel).
namespace {
struct GroupedBody { int m, n, k, flags, variant, lda, ldb, ldc; };
inline bool operator==(const GroupedBody& a, const GroupedBody& b) { return 0 == memcmp(&a, &b, sizeof(a)); }

constexpr int GROUPED_BYVAL = 32; // table entries a grouped launch carries as a kernel argument
std::string gen_smm_grouped_source(int typesize, const std::vector<GroupedBody>& bodies, int threads)
{
  std::string s = "// generated by libxsmm-amd (dense SMM run kernels of several shapes behind one dispatcher)\n";
  s += std::string("typedef ") + (8 == typesize ? "double" : "float") + " T;\n#define XLOWP 0\n#define XFLAT 0\n#define XGROUPED 1\n";
  // threads > 64 (XSMM_SMMJIT_TILESPLIT=2): the entries are the 16 x 16 tiles of C of ONE batch (smm_tile_split) and wave t of every
  // work-group walks entry t -- the waves of a work-group walk the same runs
  const bool tilewg = (threads > 64);
  s += std::string("#define XTILEWG ") + (tilewg ? "1" : "0") + "\n";
  bool all_mfma = true;
  for (const GroupedBody& b : bodies) all_mfma = all_mfma && 0 != (b.variant & SMM_JIT_MFMA_RUNS);
  // The register-tiled bodies are called (inlined, the dispatcher carries the registers of all of them at once: measured slower);
  // the matrix-core bodies are lean enough to be inlined into the switch -- no call, no callee-saved registers through scratch.
  static const int inline_env = (int)knob("XSMM_SMMJIT_GROUPED_INLINE", 1);
  const bool inlined = (all_mfma && 0 != inline_env);
  s += std::string("#define XENTRY_ATTR ") + (inlined ? "__forceinline__" : "__attribute__((noinline))") + "\n";
  // Hand-counted waits only in bodies inlined into a dispatcher without calls. A called body reads its DevAddr through a generic
  // pointer into the dispatcher's private copy of the table entry (FLAT loads from scratch, which retire out of order with the
  // other vector-memory operations) and spills through scratch: traffic the counts do not know (hand-counted waits).
  const int handwait = inlined ? smm_mfma_handwait() : 0;
  s += SMM_JIT_GEOM_SOURCE; s += SMM_JIT_PRELUDE;
  for (size_t i = 0; i < bodies.size(); ++i) {
    const GroupedBody& b = bodies[i];
    s += "namespace xg" + std::to_string(i) + " {\n";
    SmmMacros d = smm_macro_block(typesize, b.m, b.n, b.k, b.flags, b.variant, b.lda, b.ldb, b.ldc, true);
    d.set("XPACK", 1);
    d.set("XWAVES", 1); // (wave bodies: a work-group is one wave, see below)
    if (0 != (b.variant & SMM_JIT_MFMA_RUNS)) d.set("XHANDWAIT", handwait);
    s += d.lines("#define", true);
    if (0 != (b.variant & SMM_JIT_MFMA_RUNS)) { s += SMM_JIT_MFMA_RUNS_CONST; s += SMM_JIT_CHAIN; s += SMM_JIT_MFMA_RUNS_KERNEL; }
    else { s += SMM_JIT_SHAPE; s += SMM_JIT_CHAIN; s += SMM_JIT_SHAPE_KERNELS; }
    // nothing of this body reaches the next: the block's macros, and the macros the texts define themselves -- WINDOW_AB
    // (smm_jit_chain.inc) and XNROW (smm_jit_mfma_runs_const.inc)
    s += d.lines("#undef", false);
    s += "#undef WINDOW_AB\n#undef XNROW\n}\n";
  }
  s += "struct GroupEntry { DevAddr ad; long long batch; unsigned block_begin, nblocks; int body, pad; };\n";
  // Work-groups of ONE wave: a wave whose chunk holds no run head leaves at once and its slot goes to the next work-group --
  // with four waves per work-group the slot of a whole work-group stayed taken until its longest chain was done (measured
  // on the 27 CP2K shapes: 1.37 ms with four waves per work-group).
  // (two waves per SIMD: the bodies are called, not inlined; without the bound the kernel is given the registers of the
  // hungriest body plus its own -- 308 for the 27 CP2K shapes in fp64 -- and one wave per SIMD)
  static const int grouped_wpe_env = (int)knob("XSMM_SMMJIT_GROUPED_WPE", 0); // waves per SIMD the dispatcher is compiled for
  // (two waves per SIMD for either kind of body. The matrix-core bodies of 32 x 32 fp64 keep ~155 registers alive -- A fragments,
  // B's flat image, accumulators -- and would just fit three, but inlined next to 26 others they spill at that bound: 27 CP2K
  // shapes, 524 288 products, batch order: 0.80-0.81 ms per call with two waves per SIMD, 0.82 ms with three (1.00 ms when the
  // light bodies keep four products in flight as well), 1.46 ms with four; profiles/r3_cp2k_stacks.txt)
  const int grouped_wpe = (0 < grouped_wpe_env) ? grouped_wpe_env : 2;
  // The table travels as a kernel argument (up to GROUPED_BYVAL entries: 3.8 KiB of the 4 KiB a launch may carry; the callers fuse at
  // most that many batches per launch -- the ordering check carries its table the same way) -- no staging copy on the stream in front of
  // the launch (a blit kernel of ~5 us per call: 27 CP2K calls of ~90 us each paid it 27 times), nothing that a stream capture must not see.
  s += "struct GroupTab { GroupEntry e[" + std::to_string(GROUPED_BYVAL) + "]; };\n";
  s += "extern \"C\" __global__ __launch_bounds__(" + std::to_string(threads) + ", " + std::to_string(grouped_wpe) + ") void xsmm_smm_grouped(const GroupTab tabv, int nentries)\n{\n";
  s += "  extern __shared__ __attribute__((aligned(16))) unsigned char xsmm_dyn_lds[];\n";

  if (!tilewg) {
    s += "  int e = 0;\n  while (e + 1 < nentries && blockIdx.x >= tabv.e[e + 1].block_begin) ++e;\n";
    s += "  const GroupEntry g = tabv.e[e];\n  const unsigned bid = blockIdx.x - g.block_begin;\n  T* const lds = reinterpret_cast<T*>(xsmm_dyn_lds);\n";
  }
  else { // (pad: bytes of LDS per wave)
    s += "  const int e = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);\n  if (e >= nentries) return;\n";
    s += "  const GroupEntry g = tabv.e[e];\n  const unsigned bid = blockIdx.x;\n  T* const lds = reinterpret_cast<T*>(xsmm_dyn_lds + (size_t)e * g.pad);\n";
  }
  s += "  switch (g.body) {\n";
  for (size_t i = 0; i < bodies.size(); ++i) s += "    case " + std::to_string(i) + ": xg" + std::to_string(i) + "::xsmm_entry(g.ad, g.batch, bid, g.nblocks, lds); break;\n";
  s += "    default: break;\n  }\n}\n";
  return s;
}

struct GroupedKey {
  int typesize, threads; std::vector<GroupedBody> bodies;
  bool operator==(const GroupedKey& o) const { return typesize == o.typesize && threads == o.threads && bodies == o.bodies; }
};
struct GroupedKeyHash {
  size_t operator()(const GroupedKey& k) const {
    size_t h = (size_t)k.typesize * 1024 + (size_t)k.threads;
    for (const GroupedBody& b : k.bodies) h = h * 1000003u + (size_t)(((b.m * 131 + b.n) * 131 + b.k) * 64 + b.variant + b.flags * 7 + b.lda + b.ldb * 3 + b.ldc * 5);
    return h;
  }
};
std::unordered_map<GroupedKey, JitSlot, GroupedKeyHash> g_grouped_cache; // (guarded by g_smm_lock)

// work-groups and LDS bytes one batch needs under a run-form body (the sizing of smm_jit_geometry)
void grouped_geometry(const SmmBatch& s, int variant, long long* blocks, size_t* lds)
{
  if (0 != (variant & SMM_JIT_MFMA_RUNS)) *lds = smm_mfma_runs_lds(s.typesize, s.m, s.n, s.k, s.ldb);
  else *lds = smm_jit_wave_lds(s.typesize, s.m, s.n, s.k, s.flags, 1, true); // one wave per work-group (run form)
  // a wave per chunk of 64 items (a wave whose chunk holds no run head leaves at once; if the verdict on the device cuts the
  // batch into shorter segments, a wave takes several). Sized for segments of 8 -- eight times as many work-groups, most of
  // them without work -- the 27 CP2K shapes took 0.95 ms instead of 0.6: the dispatcher, not the chains, set the pace.
  long long b = (s.batch + 63) / 64;
  if (b > 256 * 16) b = 256 * 16;
  *blocks = (b < 1 ? 1 : b);
}
} // namespace

// Can batch s be part of a grouped launch? (the run forms of the wave / work-group kernels: M, N <= 32, K <= 64)
bool smm_jit_grouped_eligible(const SmmBatch& s)
{
  if (!smm_jit_eligible(s)) return false;
  if (s.m > 32 || s.n > 32 || s.k > 64 || 0 != s.lowp) return false;
  if (SYNC_DEVICE != s.sync) return false;
  return 0 != smm_jit_waves(s.typesize, s.m, s.n, s.k, s.flags, 1);
}

// The run form a batch of shared C gets (SYNC_RUNS, SYNC_DEVICE; alone or as a grouped body): a wave per run on the matrix
// cores where that form serves, else the register-tiled wave form. deep: a grouped body of a batch split into tiles.
static int smm_run_variant(const SmmBatch& s, bool deep)
{
  const int split = (0 != s.relaxed ? SMM_JIT_SPLIT : 0); // the caller's reference path is unordered as well: segments + atomics
  if (smm_mfma_runs_ok(s)) return SMM_JIT_SCALAR | split | SMM_JIT_RUNS | SMM_JIT_MFMA_RUNS | (deep ? SMM_JIT_DEEP : 0);
  return smm_jit_width_variant(s) | split | SMM_JIT_RUNS;
}

// All batches (same precision, each with its verdict slot in devflags) in one launch.
namespace {
struct GroupedEntry { int group, body; long long blocks; };
struct GroupedPlan { GroupedKey key; std::vector<GroupedEntry> entries; size_t lds_max = 0; };
// which bodies (one per shape) a set of batches needs and how many work-groups each batch gets. Only the wave form: the
// work-group form (four waves share a product; better for a batch of large shapes on its own) as a second kernel beside
// the first was measured slower -- 27 CP2K shapes, fp64: 1.36 ms with it (its kernel took 0.94 ms next to the wave kernel,
// 0.32 ms alone), 1.18 ms with all chains on the wave form.
bool grouped_plan(const SmmBatch* groups, int ngroups, bool check_eligible, GroupedPlan& plan, bool tiles = false)
{ // tiles: the groups are the tiles of one batch of few runs (smm_tile_split)
  plan.key.typesize = groups[0].typesize; plan.key.threads = (tiles && 2 == smm_tilesplit()) ? 64 * ngroups : 64; plan.key.bodies.clear(); plan.entries.clear(); plan.lds_max = 0;
  for (int g = 0; g < ngroups; ++g) {
    const SmmBatch& s = groups[g];
    if (s.typesize != groups[0].typesize || (check_eligible && !smm_jit_grouped_eligible(s))) return false;
    const int variant = smm_run_variant(s, tiles);
    const GroupedBody body = { s.m, s.n, s.k, s.flags & (LIBXSMM_GEMM_FLAG_BETA_0 | LIBXSMM_GEMM_FLAG_TRANS_B), variant, s.lda, s.ldb, s.ldc };
    size_t bi = 0;
    while (bi < plan.key.bodies.size() && !(plan.key.bodies[bi] == body)) ++bi;
    if (bi == plan.key.bodies.size()) plan.key.bodies.push_back(body);
    GroupedEntry e; e.group = g; e.body = (int)bi; size_t lds = 0;
    grouped_geometry(s, variant, &e.blocks, &lds);
    if (lds > plan.lds_max) plan.lds_max = lds;
    plan.entries.push_back(e);
  }
  { // bodies in a canonical order: the same set of shapes gives the same kernel (and cache file) whatever the order of the groups
    std::vector<size_t> order(plan.key.bodies.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return 0 > memcmp(&plan.key.bodies[x], &plan.key.bodies[y], sizeof(GroupedBody)); });
    std::vector<GroupedBody> sorted(order.size()); std::vector<int> where(order.size());
    for (size_t i = 0; i < order.size(); ++i) { sorted[i] = plan.key.bodies[order[i]]; where[order[i]] = (int)i; }
    plan.key.bodies.swap(sorted);
    for (GroupedEntry& e : plan.entries) e.body = where[(size_t)e.body];
  }
  // the work-groups of a launch start in the order of their indexes: the batches with the longest chains go first, the short
  // ones fill the tail
  std::stable_sort(plan.entries.begin(), plan.entries.end(), [&](const GroupedEntry& x, const GroupedEntry& y) {
    const SmmBatch& a = groups[x.group]; const SmmBatch& b = groups[y.group];
    return (long long)a.m * a.k + (long long)a.k * a.n + (long long)a.m * a.n > (long long)b.m * b.k + (long long)b.k * b.n + (long long)b.m * b.n;
  });
  return true;
}

// the grouped kernel of these batches (nullptr: not available -- the caller launches them one by one)
JitKernel* grouped_resolve(const SmmBatch* groups, int ngroups, bool check_eligible, bool tiles, GroupedPlan& plan)
{
  if (ngroups < 1 || !grouped_plan(groups, ngroups, check_eligible, plan, tiles) || plan.lds_max > 65536) return nullptr;
  const GroupedKey& key = plan.key;
  return jit_resolve(g_grouped_cache, key, "xsmm_smm_grouped", false, [&key]() { return gen_smm_grouped_source(key.typesize, key.bodies, key.threads); });
}

int grouped_launch(const SmmBatch* groups, const GroupedPlan& plan, JitKernel* kern, void* stream)
{
  struct GroupEntryH { DevAddr ad; long long batch; unsigned block_begin, nblocks; int body, pad; };
  struct GroupTabH { GroupEntryH e[GROUPED_BYVAL]; };
  static_assert(sizeof(GroupTabH) + 16 <= 4096, "kernel arguments of a launch");
  if (plan.entries.size() > (size_t)GROUPED_BYVAL) return -1; // (never: the callers fuse at most 32 batches per launch)
  GroupTabH tab; // (a kernel argument: see gen_smm_grouped_source)
  memset(&tab, 0, sizeof(tab));
  int nentries = (int)plan.entries.size();
  unsigned total = 0;
  for (int i = 0; i < nentries; ++i) {
    const SmmBatch& s = groups[plan.entries[(size_t)i].group];
    GroupEntryH& t = tab.e[i];
    t.ad = dev_addr(s);
    t.batch = s.batch; t.block_begin = total; t.nblocks = (unsigned)plan.entries[(size_t)i].blocks; t.body = plan.entries[(size_t)i].body;
    total += t.nblocks;
  }
  size_t lds_bytes = plan.lds_max;
  if (plan.key.threads > 64) { // a work-group per chunk of 64 items, a wave per tile
    const size_t per_wave = (plan.lds_max + 15) / 16 * 16;
    total = tab.e[0].nblocks;
    for (int i = 0; i < nentries; ++i) { tab.e[i].block_begin = 0; tab.e[i].nblocks = total; tab.e[i].pad = (int)per_wave; }
    lds_bytes = per_wave * (size_t)nentries;
  }
  void* args[] = { (void*)&tab, &nentries };
  return jit_launch_dyn(kern, total, (unsigned)plan.key.threads, (unsigned)lds_bytes, args, stream);
}
}

// the text a grouped launch of these batches compiles (tests: valid gfx950 code without a device)
std::string gen_smm_grouped_source_for(const SmmBatch* groups, int ngroups, bool tiles)
{
  GroupedPlan plan;
  if (ngroups < 1 || !grouped_plan(groups, ngroups, false, plan, tiles)) return std::string();
  return gen_smm_grouped_source(plan.key.typesize, plan.key.bodies, plan.key.threads);
}

int launch_smm_jit_grouped(const SmmBatch* groups, int ngroups, void* stream, const char** name)
{ // -1: not available (the caller launches the batches one by one)
  GroupedPlan plan;
  JitKernel* const kern = grouped_resolve(groups, ngroups, true, false, plan);
  if (nullptr == kern) return -1;
  *name = (8 == groups[0].typesize) ? "smm_f64_jit_shape_runs_grouped" : "smm_f32_jit_shape_runs_grouped";
  return grouped_launch(groups, plan, kern, stream);
}

// A batch of few runs whose C has several 16 x 16 tiles (one call per CP2K stack: 19 418 products of 32^3 are 172 runs -- 172 waves on
// a chip that holds thousands, each a chain of ~110 dependent products): every tile of C becomes a batch of its own -- the sub-matrices
// A(16 mi.., :), B(:, 16 ni..), C(16 mi.., 16 ni..) under the same leading dimensions, index arrays and ordering verdict -- and the
// tiles run as the groups of one grouped launch: a wave per run AND tile, a quarter of the matrix instructions and half of the
// operand loads per product and wave. Every element of C still receives its own chain in batch order: the same bits.
// Returns the number of tile batches written to out[<= 4] (0: not split).
static int smm_tile_split(const SmmBatch& s, SmmBatch* out)
{
  static const int max_waves = (int)knob("XSMM_SMMJIT_TILESPLIT_WAVES", 1280);
  const int mi = (s.m + 15) / 16, ni = (s.n + 15) / 16;
  if (0 == smm_tilesplit() || mi * ni < 2 || mi * ni > 4 || SYNC_DEVICE != s.sync || (ADDR_STRIDED != s.mode && ADDR_INDEX != s.mode)) return 0;
  // Every tile's wave fetches its rows of A and its columns of B: twice the requests of a wave per product. Measured (tools/bench_tile_split.py,
  // profiles/r3_tile_split.txt; fp64 32^3, ms split / not split): 2 000 items 0.08-0.16 / 0.12-0.31, 8 000 items 0.08-0.16 / 0.12-0.31, 16 000 items
  // equal for runs up to 32 and 0.17 / 0.31 for runs of 256, 30 000 items 0.20-0.28 / 0.13-0.27 for runs up to 32 (0.19 / 0.31 for runs of
  // 256), 60 000 items 0.37-0.61 / 0.18-0.37: split while the batch cannot fill the chip anyway (the run lengths are known on the device only).
  if (((s.batch + 63) / 64) * mi * ni > max_waves) return 0;
  int n = 0;
  for (int j = 0; j < ni; ++j) {
    for (int i = 0; i < mi; ++i) {
      SmmBatch t = s;
      t.m = (s.m - 16 * i < 16) ? (s.m - 16 * i) : 16; t.n = (s.n - 16 * j < 16) ? (s.n - 16 * j) : 16;
      t.a = static_cast<const char*>(s.a) + (size_t)16 * i * s.typesize;
      t.b = static_cast<const char*>(s.b) + (size_t)16 * j * s.ldb * s.typesize;
      t.c = static_cast<char*>(s.c) + ((size_t)16 * j * s.ldc + (size_t)16 * i) * s.typesize;
      // (the batch as a whole has passed smm_jit_eligible; its rule about leading dimensions with gaps -- an operand's whole span is
      // fetched -- does not apply to a tile: the matrix-core form requests A and C element by element through their leading dimensions,
      // and B's span of a tile is the tile's columns)
      if (!smm_mfma_runs_ok(t)) return 0;
      out[n++] = t;
    }
  }
  return n;
}

// ---- which generated kernels a batch gets ------------------------------------------------------------------------------
// A plan is the list of alternatives the launchers try, in order. An alternative is one or two launch parts -- a generated kernel
// over a slice of the batch, launched in order once the kernels of all parts are ready -- or the tiles of C as one grouped launch.
// run_smm tries the matrix-core tier before the hand-written kernels, the specialised tier after them.
namespace {
enum { SLICE_ALL, SLICE_PACKED, SLICE_REST };  // the whole batch; its groups of `pack` consecutive items; the items after them
enum { TIER_MFMA, TIER_JIT };
struct SmmPart { SmmKey key; int slice; };
struct SmmAlt { int tier; const char* name; int nparts; SmmPart part[2]; int ntiles; SmmBatch tiles[4]; };
struct SmmPlan {
  SmmBatch batch;         // as the generated kernels see it (16-bit inputs: typesize 4, strides in elements of the inputs)
  int ab_bytes, c_bytes;  // bytes per element of A and B, of C (where the remainder starts)
  int pack;               // items per wave pass of the SLICE_PACKED part
  int nalts; SmmAlt alts[8];
};

SmmAlt& plan_alt(SmmPlan& p, int tier, const char* name)
{
  SmmAlt& a = p.alts[p.nalts++];
  a.tier = tier; a.name = name; a.nparts = 0; a.ntiles = 0;
  return a;
}
void plan_part(const SmmPlan& p, SmmAlt& a, int variant, int slice)
{
  const SmmBatch& s = p.batch;
  a.part[a.nparts++] = SmmPart{ SmmKey{ s.typesize, s.m, s.n, s.k, s.flags & (LIBXSMM_GEMM_FLAG_BETA_0 | LIBXSMM_GEMM_FLAG_TRANS_B), variant, s.lda, s.ldb, s.ldc }, slice };
}
void plan_add(SmmPlan& p, int tier, const char* name, int variant) { plan_part(p, plan_alt(p, tier, name), variant, SLICE_ALL); }
// groups of `pack` consecutive items per wave pass (kernel `variant`), then the few items that are left (kernel `rest`)
void plan_packed(SmmPlan& p, const char* name, int variant, int pack, int rest)
{
  SmmAlt& a = plan_alt(p, TIER_JIT, name);
  p.pack = pack;
  if (p.batch.batch >= pack) plan_part(p, a, variant | smm_jit_pack_bits(pack), SLICE_PACKED);
  if (0 != p.batch.batch % pack) plan_part(p, a, rest, SLICE_REST);
}

// the matrix-core tier (32 < max(M, N) <= 64, K <= 64; independent items): the descriptor baked in
void plan_mfma(const SmmBatch& s, SmmPlan& p)
{
  static const int on = (int)knob("XSMM_SMMJIT_MFMA", 1);
  static const int wave_min = (int)knob("XSMM_SMMJIT_WAVE_MIN", 32); // the wave form below 33
  static const int wave_on = (int)knob("XSMM_SMMJIT_MFMA_WAVE", 1);
  static const int tightc_on = (int)knob("XSMM_SMM64_TIGHTC", 1);
  if (0 == on || 0 == s.use_mfma || 0 != s.general || 0 != s.lowp) return;
  const bool transb = (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B)); // (B^T in memory: served by the one-wave-per-item form only)
  if (!((wave_min < s.m || wave_min < s.n) && s.m <= 64 && s.n <= 64 && 0 < s.k && s.k <= 64 && s.lda >= s.m && s.ldb >= (transb ? s.n : s.k) && s.ldc >= s.m)) return;
  if (4 == s.typesize && 64 == s.m && 64 == s.n && 64 == s.k && 64 == s.lda && 64 == s.ldb && 64 == s.ldc && SYNC_NONE == s.sync) return; // the hand-tuned tight 64^3 kernel
  // (independent items only: runs of a uniform length come from blocked GEMM alone, which goes to the pre-compiled run kernels of
  // kernels/smm_special.hip and the specialised tier without asking this one -- DESIGN.md section 8k)
  if (SYNC_NONE != s.sync || s.batch < 1) return;
  if (s.batch < smm_jit_min_batch() && 0 == s.jit_always) return;
  const bool f64 = (8 == s.typesize);
  // 16-byte chunks for strided batches of suitably shaped and aligned items, else element by element (any shape, index and
  // pointer batches: the kernel resolves the addresses like every other batch kernel)
  const uintptr_t bits = reinterpret_cast<uintptr_t>(s.a) | reinterpret_cast<uintptr_t>(s.b) | reinterpret_cast<uintptr_t>(s.c)
                       | (uintptr_t)(s.sa * s.typesize) | (uintptr_t)(s.sb * s.typesize) | (uintptr_t)(s.sc * s.typesize);
  { // one wave per item: independent items, at least four waves per CU
    const int chunk = 16 / s.typesize;
    const int bdim = transb ? s.n : s.k, bcnt = transb ? s.k : s.n; // B in memory: bcnt columns of bdim elements at a distance of ldb
    const bool tight_ld = (s.lda == s.m && s.ldb == bdim && s.ldc == s.m);
    const bool wide = (tight_ld && ADDR_STRIDED == s.mode && 0 == (bits & 15) && 0 == s.m % chunk && 0 == s.k % 4 && (!transb || 0 == s.n % chunk));
    const size_t wlds = smm_mfma_wave_lds(s.typesize, s.m, s.n, s.k, wide ? chunk : 1, transb);
    // gaps in the leading dimensions: the element-wise build fetches the spans and drops the gaps (up to half as much again)
    // -- where the spans are short: with more than ~80 elements per lane in flight the work-group form is the faster one
    // (tools/bench_gaps.py: 43x9x27 ld 48/32/48 55.9 vs 51.4 %, 40x64x17 ld 40/17/44 48.6 vs 40.5 %, but 48^3 ld 56 28.8 vs 56.8 %)
    const long long span_loads = ((long long)s.lda * (s.k - 1) + s.m + 63) / 64 + ((long long)s.ldb * (bcnt - 1) + bdim + 63) / 64 + ((long long)s.ldc * (s.n - 1) + s.m + 63) / 64;
    const bool gaps_ok = tight_ld || (2 * s.lda <= 3 * s.m && 2 * s.ldb <= 3 * bdim && 2 * s.ldc <= 3 * s.m && span_loads <= 80);
    if (0 != wave_on && 0 != wlds && 4 * wlds <= 160u * 1024u && SYNC_NONE == s.sync && gaps_ok)
      plan_add(p, TIER_MFMA, f64 ? "smm_f64_mfma_wave_jit" : "smm_f32_mfma_wave_jit", SMM_JIT_MFMA_WAVE | (wide ? 0 : SMM_JIT_SCALAR));
  }
  if (transb) return; // (the forms below read B as stored column by column)
  // fp64 items too large for that: the two-halves form where it leaves room for four waves per CU (56^3: 66 % against 54-58 % on the
  // work-group form; 64 x 64 x K stays on the work-group form, which is the faster one there -- tools/probe/mfma_wave.hip)
  const size_t w2lds = f64 ? smm_mfma_wave2_lds(s.typesize, s.m, s.n, s.k) : 0;
  if (0 != wave_on && 0 != w2lds && 4 * w2lds <= 160u * 1024u && !(64 == s.m && 64 == s.n) && SYNC_NONE == s.sync && ADDR_STRIDED == s.mode && 0 == (bits & 15)
    && s.lda == s.m && s.ldb == s.k && s.ldc == s.m) plan_add(p, TIER_MFMA, "smm_f64_mfma_wave2_jit", SMM_JIT_MFMA_WAVE2);
  if (!(32 < s.m || 32 < s.n)) return; // (the work-group forms below are for shapes beyond 32)
  const bool tight = !f64 && s.lda == s.m && s.ldb == s.k && 0 == ((s.m * s.k) & 3) && 0 == ((s.k * s.n) & 3);
  const bool tightc = !f64 && s.ldc == s.m && 0 == ((s.m * s.n) & 3) && 0 != (s.m & 31) && 0 != tightc_on;
  plan_add(p, TIER_MFMA, f64 ? "smm_f64_mfma_wg_jit" : "smm_f32_mfma_wg_jit", SMM_JIT_MFMA | (tight ? SMM_JIT_MFMA_TIGHT : 0) | (tightc ? SMM_JIT_MFMA_TIGHTC : 0));
}

// 16-bit inputs (lowp 1: i16 -> i32, 3: bf16 -> f32, 4: bf16 -> bf16): tight items with independent C
void plan_lowp(const SmmBatch& s, SmmPlan& p)
{
  static const int wave_on = (int)knob("XSMM_SMMJIT_MFMA_WAVE", 1);
  static const int wave_min = (int)knob("XSMM_SMMJIT_LOWP_WAVE_MIN", 31); // (32^3: 73.8 vs 67.9 % for the fp32 result, 67.9 vs 49.5 % for bf16; 16^3 is better off on the streaming form)
  static const int big_i16 = (int)knob("XSMM_SMMJIT_LOWP_BIG", 1);
  if ((1 != s.lowp && 3 != s.lowp && 4 != s.lowp) || 0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) || (4 == s.lowp && 0 != (s.m & 1))) return;
  p.batch.typesize = 4; p.batch.lowp = 0; p.batch.sync = SYNC_NONE; // (the kernel itself addresses A and B -- and a bf16 C -- in elements of 16 bits)
  p.ab_bytes = 2; p.c_bytes = (4 == s.lowp ? 2 : 4);
  const int lowp_bits = ((4 == s.lowp ? 2 : s.lowp) << 11); // XLOWP: 1 i16 -> i32, 2 bf16 -> bf16, 3 bf16 -> f32
  const bool strided = (ADDR_STRIDED == s.mode); // (index and pointer batches: the streaming form with element-wide -- one k pair -- accesses)
  const bool tight = (s.lda == s.m && s.ldb == s.k && s.ldc == s.m);
  { // bf16 inputs beyond 32: the one-wave-per-item matrix-core kernel (fp32 instruction on the widened operands: the gold loop's
    // product-then-add bit for bit). Index and pointer batches as well: their items are whole numbers of 16-byte chunks long -- M % 4 == 0,
    // K % 8 == 0 -- so callers that lay items out back to back keep the chunks aligned; an item that does not start on 16 bytes costs speed
    const size_t wlds = smm_mfma_wave_lds(4, s.m, s.n, s.k);
    const uintptr_t bits = strided ? (reinterpret_cast<uintptr_t>(s.a) | reinterpret_cast<uintptr_t>(s.b) | reinterpret_cast<uintptr_t>(s.c)
                         | (uintptr_t)(s.sa * 2) | (uintptr_t)(s.sb * 2) | (uintptr_t)(s.sc * p.c_bytes)) : 0;
    if (0 != wave_on && 0 != s.use_mfma && 1 != s.lowp && (wave_min < s.m || wave_min < s.n) && 0 != wlds && 4 * wlds <= 160u * 1024u
      && 0 == (s.k & 7) && (3 == s.lowp || 0 == (s.m & 7)) && 0 == (bits & 15) && tight && s.batch >= smm_jit_min_batch())
      plan_add(p, TIER_JIT, (4 == s.lowp) ? "smm_bf16_mfma_wave_jit_lowp" : "smm_bf16f32_mfma_wave_jit_lowp", SMM_JIT_MFMA_WAVE | lowp_bits);
  }
  // (i16 -> i32 has no matrix-core form: beyond 32 the same streaming kernel with a larger tile per lane -- 48^3 18 -> 57 %,
  // 64^3 16 -> 56 % of the HBM peak; XSMM_SMMJIT_LOWP_BIG=0: the pre-compiled kernel)
  const int lim = (0 != big_i16) ? 64 : 32; // (bf16 shapes the matrix-core form above does not take -- M or K not a multiple of 4 / 8 -- come here as well)
  if (s.m > lim || s.n > lim || s.k > 64 || 0 != (s.k & 1) || !tight || s.batch < smm_jit_min_batch() || 0 == smm_jit_waves(4, s.m, s.n, s.k, s.flags)) return;
  // strided batches of items laid out back to back take 16-byte accesses; every other batch (other strides, index arrays -- in
  // elements of 16 bits, as the reference's libxsmm_mmbatch_kernel counts them --, arrays of pointers) one k pair per access
  const bool back_to_back = strided && s.sa == (long long)s.m * s.k && s.sb == (long long)s.k * s.n && s.sc == (long long)s.m * s.n;
  const bool wide = (back_to_back && 0 == ((reinterpret_cast<uintptr_t>(s.a) | reinterpret_cast<uintptr_t>(s.b) | reinterpret_cast<uintptr_t>(s.c)) & 15));
  const int variant = (wide ? 0 : SMM_JIT_SCALAR) | lowp_bits;
  const char* const name = (1 == s.lowp) ? "smm_i16i32_jit_shape_lowp" : (4 == s.lowp ? "smm_bf16_jit_shape_lowp" : "smm_bf16f32_jit_shape_lowp");
  if (wide) { // small items laid out back to back: several per wave and pass, as the fp32 / fp64 streaming form takes them (a 16^3 item is
    // 1.5-2 KB: one per wave leaves most lanes of every access idle and the kernel bound by its instruction count per item)
    const int pack_env = (int)knob("XSMM_SMMJIT_LOWP_PACK", 0); // (read on every call: the tests sweep it)
    const size_t item = 2 * ((size_t)s.m * s.k + (size_t)s.k * s.n) + (size_t)p.c_bytes * s.m * s.n;
    int pack = 1;
    if (0 < pack_env) pack = pack_env;
    else if (item < 6000) while (pack < 8 && 2 * pack * item <= 16384) pack *= 2;
    while (0 != (pack & (pack - 1))) --pack;
    while (1 < pack && ((size_t)pack * 4 * ((size_t)s.m * s.k + (size_t)s.k * s.n + (size_t)s.m * s.n) > 28672 || 0 == smm_jit_waves(4, s.m, s.n, s.k, s.flags, pack))) pack /= 2;
    if (1 < pack && s.batch >= pack) plan_packed(p, name, variant, pack, variant);
  }
  plan_add(p, TIER_JIT, name, variant);
}

// the specialised tier (the batch has passed smm_jit_eligible)
void plan_jit(const SmmBatch& s, SmmPlan& p)
{
  static const int wg_env = (int)knob("XSMM_SMMJIT_WG", 1);
  const bool f64 = (8 == s.typesize);
  const int width = smm_jit_width_variant(s);
  if (s.m <= 32 && s.n <= 32 && s.k > 64 && smm_mfma_runs_ok(s, true)) // long K, small M and N, every item its own C: K in chunks on the matrix cores
    plan_add(p, TIER_JIT, f64 ? "smm_f64_mfma_stream_jit" : "smm_f32_mfma_stream_jit", SMM_JIT_SCALAR | SMM_JIT_MFMA_RUNS);
  if (s.m > 32 || s.n > 32 || s.k > 64) { // (eligibility made sure of SYNC_NONE, or of runs of a uniform length)
    if (0 != smm_jit_big_kc(s.typesize, s.m, s.n, s.k) && (SYNC_NONE == s.sync || (0 < s.uniform_run && 0 == s.batch % s.uniform_run)))
      plan_add(p, TIER_JIT, f64 ? "smm_f64_jit_shape_wg" : "smm_f32_jit_shape_wg", SMM_JIT_BIG);
    return;
  }
  if (SYNC_NONE == s.sync) { // every item owns its C
    // leading dimensions with gaps: the matrix-core run form addresses A's fragments and C through their leading dimensions (no
    // gap element is requested) -- every item is a run of its own there. XSMM_SMMJIT_GAPS_MFMA (read on every call: tests and tools
    // toggle it): 0 off, 1 gaps only, 2 tight items too. (tools/bench_generic.py, fraction of the HBM peak in algorithmic bytes,
    // register-tiled streaming form -> this one: fp64 23^3 ld 24 54.1 -> 59.2 %, fp32 32^3 ld 40 42.3 -> 50.5 %, fp64 13^3 ld 16
    // 44.1 -> 51.6 %; tight fp64 23^3 64.5 -> 61.5 %: tight items stay)
    const int gaps_mfma = (int)knob("XSMM_SMMJIT_GAPS_MFMA", 1);
    const bool tight_ld = (s.lda == s.m && s.ldc == s.m && s.ldb == s.k);
    if (0 != gaps_mfma && (!tight_ld || 2 == gaps_mfma) && smm_mfma_runs_ok(s))
      plan_add(p, TIER_JIT, f64 ? "smm_f64_mfma_stream_jit" : "smm_f32_mfma_stream_jit", SMM_JIT_SCALAR | SMM_JIT_MFMA_RUNS);
    const char* const name = f64 ? "smm_f64_jit_shape" : "smm_f32_jit_shape";
    const int pack = smm_jit_pack(s, width);
    if (1 < pack) plan_packed(p, name, width, pack, SMM_JIT_SCALAR);
    plan_add(p, TIER_JIT, name, width);
    return;
  }
  const char* const runs_name = f64 ? "smm_f64_jit_shape_runs" : "smm_f32_jit_shape_runs";
  if (smm_mfma_runs_ok(s)) { // shared C on the matrix cores: a wave per run (batch order; segments + atomics if the verdict or a relaxed order say so)
    SmmBatch tiles[4];
    const int nt = smm_tile_split(s, tiles); // (at most four entries: the table is a kernel argument -- nothing staged, fine inside a stream capture)
    if (1 < nt) {
      SmmAlt& a = plan_alt(p, TIER_JIT, f64 ? "smm_f64_mfma_runs_tiles_jit" : "smm_f32_mfma_runs_tiles_jit");
      a.ntiles = nt; std::copy(tiles, tiles + nt, a.tiles);
    }
    plan_add(p, TIER_JIT, f64 ? "smm_f64_mfma_runs_jit" : "smm_f32_mfma_runs_jit", smm_run_variant(s, false));
  }
  // the work-group form pays off once a product's operands are large (measured on CP2K stacks: 32^3 f64 yes, 23^3 no)
  const bool tight = (s.lda == s.m && s.ldc == s.m && (0 != (s.flags & LIBXSMM_GEMM_FLAG_TRANS_B) ? (s.ldb == s.n) : (s.ldb == s.k)));
  const bool wg_fits = (tight && 0 != wg_env && smm_jit_wg(s.typesize, s.m, s.n, s.k, s.flags).wg_buf * s.typesize <= geom::LDS_STATIC
                     && (2 == wg_env || (size_t)s.typesize * ((size_t)s.m * s.k + (size_t)s.k * s.n) >= 12288));
  if (SYNC_RUNS == s.sync) { // the host knows that C repeats in runs (one C for the whole batch, batch-reduce): long runs
    if (wg_fits) plan_add(p, TIER_JIT, f64 ? "smm_f64_jit_shape_wgruns" : "smm_f32_jit_shape_wgruns", width | SMM_JIT_WGRUNS);
    plan_add(p, TIER_JIT, runs_name, width | SMM_JIT_RUNS);
    return;
  }
  // SYNC_DEVICE: both run forms are launched; each reads the device-side verdict (average run length) and one of them works.
  // (a wave form that leaves long runs to a companion that then fails to compile would have to be followed by a second wave-form
  // launch -- which would add the short runs twice: the executor launches nothing before the kernels of all parts are ready)
  const int split = (0 != s.relaxed ? SMM_JIT_SPLIT : 0);
  if (wg_fits) {
    SmmAlt& a = plan_alt(p, TIER_JIT, runs_name);
    plan_part(p, a, width | split | SMM_JIT_RUNS | SMM_JIT_HASWG, SLICE_ALL);
    plan_part(p, a, width | split | SMM_JIT_WGRUNS, SLICE_ALL);
  }
  plan_add(p, TIER_JIT, runs_name, width | split | SMM_JIT_RUNS); // the wave form alone takes long runs as well
}
} // namespace

// The alternatives of both tiers for batch s, in the order the launchers try them. Pure: no device, no kernel looked up.
static void smm_jit_plan(const SmmBatch& s, SmmPlan& p)
{
  p.batch = s; p.ab_bytes = p.c_bytes = s.typesize; p.pack = 1; p.nalts = 0;
  if (!smm_jit_enabled()) return;
  if (0 != s.lowp) { plan_lowp(s, p); return; }
  plan_mfma(s, p);
  if (smm_jit_eligible(s)) plan_jit(s, p);
}

// the part of the batch a launch part covers
static SmmBatch smm_slice(const SmmPlan& p, int slice)
{
  SmmBatch s = p.batch;
  const long long done = (s.batch / p.pack) * p.pack;
  if (SLICE_PACKED == slice) { s.sa *= p.pack; s.sb *= p.pack; s.sc *= p.pack; s.batch /= p.pack; } // the kernel takes `pack` items as one
  else if (SLICE_REST == slice) {
    s.a = (const char*)s.a + done * s.sa * p.ab_bytes; s.b = (const char*)s.b + done * s.sb * p.ab_bytes;
    s.c = (char*)s.c + done * s.sc * p.c_bytes; s.batch -= done;
  }
  return s;
}

// XSMM_SMMJIT_SKIP (developer knob, read on every call: the tests run every link of a launch chain alone): a bit mask of links that
// are treated as not ready. Bits 0-7: the alternatives of a plan by their position in SmmPlan::alts (both tiers counted); bit 8: the
// hand-written kernels (launch_smm_special). A skipped alternative is not asked for: nothing is compiled for it.
int smm_skip_mask() { return (int)knob("XSMM_SMMJIT_SKIP", 0); }

// Launches the first alternative of the tier whose kernels are all ready (every kernel of an alternative is asked for, so that
// the compiler thread builds them all). -1: none is (the caller's next tier serves, with the same bits).
static int smm_jit_execute(const SmmPlan& p, int tier, void* stream, const char** name)
{
  const int skip = smm_skip_mask();
  for (int i = 0; i < p.nalts; ++i) {
    const SmmAlt& a = p.alts[i];
    if (tier != a.tier || 0 != (skip & (1 << i))) continue;
    if (0 < a.ntiles) {
      GroupedPlan gp;
      JitKernel* const kern = grouped_resolve(a.tiles, a.ntiles, false, true, gp);
      if (nullptr == kern) continue;
      *name = a.name;
      return grouped_launch(a.tiles, gp, kern, stream);
    }
    JitKernel* kern[2] = { nullptr, nullptr };
    bool ready = true;
    for (int j = 0; j < a.nparts; ++j) ready = (nullptr != (kern[j] = smm_jit_get(a.part[j].key))) && ready;
    if (!ready) continue;
    *name = a.name;
    int e = 0;
    for (int j = 0; j < a.nparts && 0 == e; ++j) e = smm_jit_launch(smm_slice(p, a.part[j].slice), a.part[j].key.variant, kern[j], stream);
    return e;
  }
  return -1;
}

int launch_smm_jit_mfma(const SmmBatch& s, void* stream, const char** name)
{
  SmmPlan p;
  smm_jit_plan(s, p);
  return smm_jit_execute(p, TIER_MFMA, stream, name);
}

int launch_smm_jit(const SmmBatch& s, void* stream, const char** name)
{
  SmmPlan p;
  smm_jit_plan(s, p);
  return smm_jit_execute(p, TIER_JIT, stream, name);
}

// The plan of batch s as text, one line per alternative (libxsmm_amd_smm_plan_describe; no device needed):
//   <position> <mfma|jit> <name> parts=<n> [<variant>:<all|packed|rest> ...] tiles=<n> [<m>x<n>:<variant> ...]
// check_tiles: the grouped text of every alternative that runs the tiles of C is compiled as well; *failed counts those that do not.
std::string smm_plan_describe(const SmmBatch& s, bool check_tiles, int* failed)
{
  static const char* const slice_name[] = { "all", "packed", "rest" };
  SmmPlan p;
  smm_jit_plan(s, p);
  std::string out;
  char word[160];
  for (int i = 0; i < p.nalts; ++i) {
    const SmmAlt& a = p.alts[i];
    snprintf(word, sizeof(word), "%d %s %s parts=%d", i, TIER_MFMA == a.tier ? "mfma" : "jit", a.name, a.nparts); out += word;
    for (int j = 0; j < a.nparts; ++j) { snprintf(word, sizeof(word), " %d:%s", a.part[j].key.variant, slice_name[a.part[j].slice]); out += word; }
    snprintf(word, sizeof(word), " tiles=%d", a.ntiles); out += word;
    for (int j = 0; j < a.ntiles; ++j) { snprintf(word, sizeof(word), " %dx%d:%d", a.tiles[j].m, a.tiles[j].n, smm_run_variant(a.tiles[j], true)); out += word; }
    out += "\n";
    if (check_tiles && 0 < a.ntiles) {
      std::string log;
      const std::string src = gen_smm_grouped_source_for(a.tiles, a.ntiles, true);
      if ((src.empty() || 0 != jit_check_source(src, &log)) && nullptr != failed) ++*failed;
    }
  }
  return out;
}

// Code objects ahead of time (no device needed): every kernel the plans of a fixed set of batches per shape name -- strided
// batches (wide and element-wide accesses), index batches (independent items, runs, the verdict on the device in batch order
// and relaxed, a batch of few runs split into tiles) -- and, if `grouped`, the fused kernel of all shapes for index batches.
// Returns the number of code objects that could not be built.
int smm_jit_prebuild(const SmmBatch* shapes, int nshapes, int grouped, int* built)
{
  int failed = 0, done = 0;
  std::unordered_set<std::string> seen;
  auto build = [&](const std::string& src) {
    std::string log;
    if (src.empty() || !seen.insert(src).second) return;
    if (0 == jit_build_offline(src, &log)) ++done; else { ++failed; if (0 != verbosity()) fprintf(stderr, "LIBXSMM-AMD: prebuild: %s\n", log.c_str()); }
  };
  auto sample = [](const SmmBatch& shape, int mode, int sync, int relaxed) {
    SmmBatch s = shape;
    s.mode = mode; s.sync = sync; s.relaxed = relaxed; s.batch = 1 << 20; s.jit_always = 1; s.c_atomics = 1;
    s.use_mfma = 1; // (the default policy; a process that switches the matrix cores off compiles its own)
    s.a = s.b = s.c = nullptr; s.ia = s.ib = s.ic = nullptr; s.devflags = nullptr; s.uniform_run = 0;
    s.sa = (long long)s.m * s.k; s.sb = (long long)s.k * s.n; s.sc = (long long)s.m * s.n;
    return s;
  };
  for (int i = 0; i < nshapes; ++i) {
    SmmBatch kinds[8];
    kinds[0] = sample(shapes[i], ADDR_STRIDED, SYNC_NONE, 0); // tight, 16-byte aligned items back to back: wide accesses
    kinds[1] = kinds[0]; kinds[1].sa += 1;                      // element-wide accesses
    kinds[2] = sample(shapes[i], ADDR_INDEX, SYNC_NONE, 0);
    kinds[3] = sample(shapes[i], ADDR_INDEX, SYNC_RUNS, 0);
    kinds[4] = sample(shapes[i], ADDR_INDEX, SYNC_DEVICE, 0);
    kinds[5] = sample(shapes[i], ADDR_INDEX, SYNC_DEVICE, 1);
    kinds[6] = kinds[4]; kinds[6].batch = 64;                   // few runs: the tiles of C as groups (smm_tile_split)
    for (int j = 0; j < 7; ++j) {
      SmmPlan p;
      smm_jit_plan(kinds[j], p);
      for (int a = 0; a < p.nalts; ++a) {
        const SmmAlt& alt = p.alts[a];
        if (0 < alt.ntiles) build(gen_smm_grouped_source_for(alt.tiles, alt.ntiles, true));
        for (int q = 0; q < alt.nparts; ++q) {
          const SmmKey& k = alt.part[q].key;
          build(gen_smm_source(k.typesize, k.m, k.n, k.k, k.flags, k.variant, k.lda, k.ldb, k.ldc));
        }
      }
    }
  }
  if (0 != grouped && 1 < nshapes) {
    for (int relaxed = 0; relaxed < 2; ++relaxed) {
      std::vector<SmmBatch> g;
      for (int i = 0; i < nshapes; ++i) {
        const SmmBatch s = sample(shapes[i], ADDR_INDEX, SYNC_DEVICE, relaxed);
        if (smm_jit_grouped_eligible(s) && s.typesize == shapes[0].typesize) g.push_back(s);
      }
      if (1 < g.size()) build(gen_smm_grouped_source_for(g.data(), (int)g.size()));
    }
  }
  if (nullptr != built) *built = done;
  return failed;
}

} // namespace xsmm
