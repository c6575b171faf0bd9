// xsmm_internal.hpp -- shared declarations between the host runtime (.cpp, built with g++) and the
// device launchers (.hip, built with hipcc). Nothing here is part of the public C-ABI.
#ifndef XSMM_INTERNAL_HPP
#define XSMM_INTERNAL_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../../include/libxsmm.h"

// ---------------------------------------------------------------------------------------------------
// The GEMM descriptor. Layout follows the reference's packed POD (src/libxsmm_main.h:157-168): it is the
// registry key and what libxsmm_get_mmkernel_info decodes, so callers that memcpy/hash it keep working.
// ---------------------------------------------------------------------------------------------------
#pragma pack(push, 1)
struct libxsmm_gemm_descriptor {
  unsigned char datatype;   // inp | out << 4  (include/libxsmm_typedefs.h:91-95)
  unsigned short flags;     // libxsmm_gemm_flags
  unsigned int m, n, k;
  unsigned int lda, ldb, ldc;
  unsigned char prefetch;
};
#pragma pack(pop)
static_assert(sizeof(libxsmm_gemm_descriptor) == 28, "descriptor must stay packed (28 bytes)");

namespace xsmm {

// ---- device launch descriptions ------------------------------------------------------------------
enum AddrMode : int {
  ADDR_STRIDED = 0,   // item i: base + i*stride (elements)
  ADDR_INDEX = 1,     // item i: base + (idx[i*index_stride bytes] - index_base) elements; NULL idx => shared
  ADDR_POINTER = 2    // item i: *(T**)((char*)ptrs + i*stride bytes)
};

enum SyncMode : int {
  SYNC_NONE = 0,      // every item owns its C (or beta == 0)
  SYNC_RUNS = 1,      // equal C only in consecutive runs: one work-group walks a whole run in batch order
  SYNC_ATOMIC = 2,    // arbitrary duplicates: product from zero, then atomic add into C
  // Decided on the device, without a host round trip: a check kernel leaves {#equal neighbours, #out-of-order repeats}
  // in SmmBatch::devflags and the compute kernels read them -- the call stays asynchronous (and graph-capturable).
  SYNC_DEVICE = 3           // pick NONE / RUNS / ATOMIC from the flags (generic kernel); run kernels: runs in batch order, or
                            // segments whose sums join C with atomics ([1] != 0, or few long runs under a relaxed order)
};

struct SmmBatch {
  int typesize;             // 8: f64, 4: f32
  int m, n, k, lda, ldb, ldc;
  int flags;                // LIBXSMM_GEMM_FLAG_TRANS_B | LIBXSMM_GEMM_FLAG_BETA_0 (others ignored)
  int mode;                 // AddrMode
  const void* a; const void* b; void* c;
  const int* ia; const int* ib; const int* ic;  // ADDR_INDEX (device arrays)
  int index_base, index_stride;                 // ADDR_INDEX: base and byte step through the index arrays
  long long sa, sb, sc;     // ADDR_STRIDED: element strides; ADDR_POINTER: byte distance between pointers
  long long batch;
  int sync;                 // SyncMode
  const int* devflags;      // SYNC_DEVICE*: device int[2] written by the check kernel earlier on the same stream
  int c_atomics;            // SYNC_DEVICE: != 0 if floating-point atomics reach C (device memory, not host memory the GPU maps)
  int lowp; float scf;      // low-precision kernels (kernels/smm_lowp.hip): 1 i16->i32, 2 i16->f32 (times scf), 3 bf16->f32, 4 bf16->bf16; 0: f32/f64
  int shared_across_calls;  // != 0: other tasks of the same libxsmm_mmbatch update the same C blocks concurrently (ntasks > 1): atomics
  int tasks;                // number of tasks of the libxsmm_mmbatch call this slice belongs to (0/1: the whole batch)
  long long uniform_run;    // > 0: the batch consists of runs of exactly this many consecutive items per C (blocked GEMM work lists)
  int jit_always;           // != 0: specialise with hiprtc whatever the batch size (batch-reduce kernels: short batches, called over and over)
  int relaxed;              // != 0: sums into a shared C may be formed in any order (the caller's reference path is multi-threaded)
  int use_mfma;             // policy bit (0: scalar FMA only)
  const unsigned long long* batch_ptr; // != NULL: the number of items is read from here by the kernel (deferred per-call kernels); `batch` is the capacity
  // general form used by the BLAS-like fallback (libxsmm_?gemm with alpha/beta/trans outside the SMM domain)
  double alpha, beta; int general;              // general != 0: C = alpha*op(A)*op(B) + beta*C, flags may hold TRANS_A
};

// returns hipError_t as int (0 == success); *name receives a static string naming the kernel variant
int launch_smm_batch(const SmmBatch& args, void* stream, const char** name);
int launch_smm_lowp(const SmmBatch& args, void* stream, const char** name);  // args.lowp != 0; independent C operands
int launch_smm_lowp_reduce(const SmmBatch& args, void* stream, const char** name); // bf16 batch-reduce: one C, pointer arrays of A and B

constexpr int FLAG_SLOT_BLOCKS = 512; // work-groups of the C ordering check (each leaves a pair of counts in the flag slot)
// detects how C operands alias across the batch: out[0] = number of i with c_i == c_{i-1},
// out[1] = number of i with c_i < c_{i-1}. d_out is a slot of flag_slot().
int launch_c_order_check(const SmmBatch& args, int* d_out, void* stream);
int launch_defer_gate(unsigned long long* word, unsigned long long* count_out, void* stream); // see xsmm_defer.cpp
int launch_smm_generic(const SmmBatch& s, void* stream, const char** name);
int launch_smm_special(const SmmBatch& s, void* stream, const char** name); // returns -1 if no specialised variant applies

// ---- the batch front end: launch chain, resolver and staging (xsmm_batch.cpp), recorders (xsmm_batch_record.cpp), thunks (xsmm_call.cpp)
// Where the operands of a call live: pointer_kind of each, asked in turn and only while all before it are GPU-reachable (what
// the first one that is not says about the others does not matter to any caller). One driver query per operand per call.
struct Kernel;
struct Residency {
  int a, b, c;
  bool device() const { return 0 != (a & b & c & 1); }            // the GPU reaches all three
  int visible() const { return 0 != ((a | b | c) & 2) ? 1 : 0; }  // the CPU addresses one of them as well: the call waits at its end
};
Residency classify(const void* a, const void* b, const void* c);
// host_visible: -1 = look at the operands (a driver query each), 0 = the caller knows they are plain device memory, 1 = some
// operand is memory the CPU addresses as well (the call waits for the stream)
int run_smm(const SmmBatch& s, int host_visible = -1);
int run_groups(std::vector<SmmBatch>& groups);
void launch_failed(const char* name, int hip_error);      // the one message of a launch that failed
size_t span_a(const SmmBatch& s);                         // elements touched by one A operand (span_b, span_c: B, C)
size_t span_b(const SmmBatch& s);
size_t span_c(const SmmBatch& s);
const int* device_indexes(const int* idx, int index_stride, long long n, bool* ok); // an index array as the GPU reads it (uploaded if need be)
// Pointer arrays through the pinned ring, on `stream` (device().stream; a recorder passes the stream as it is: asking for it would
// launch the record): s.a, s.b, s.c become the uploaded copies, the steps those of tight arrays. false: an upload failed (the
// caller's commit releases the entries).
bool upload_pointer_arrays(SmmBatch& s, void* stream, const void* a, size_t na, const void* b, size_t nb, const void* c, size_t nc);
// Host spans into the thread's scratch slots 3, 4, 5 (a NULL span is left out); dev receives the device copies. false: failed.
bool stage_in(const void* const host[3], const size_t bytes[3], char* dev[3]);
int stage_out(void* host_c, const void* dev_c, size_t bytes); // C back where it came from (waits for the stream); 0: done
int batch_execute(SmmBatch s, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, long long begin, long long end, bool nosync);
int lowp_batch_execute(const Kernel* k, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, long long begin, long long end);
int batch_order_env();                                    // LIBXSMM_AMD_BATCH_ORDER: 1 relaxed, -1 strict, 0 not set
extern thread_local int tl_relaxed_order;                 // > 0: inside an entry point whose reference path is multi-threaded
bool relaxed_order(int ntasks, libxsmm_blasint index_stride, const void* c);
SmmBatch from_descriptor(const libxsmm_gemm_descriptor& d);
SmmBatch lowp_from_descriptor(const libxsmm_gemm_descriptor& d, float scf);
int lowp_launch(const SmmBatch& s);
int single_execute(SmmBatch s, const void* a, const void* b, void* c); // one operand triple, wherever it lives
bool try_record(const libxsmm_gemm_descriptor& d, const void* a, const void* b, void* c); // auto-batch: true if the call was recorded
bool record_batch_call(const Kernel* k, libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* stride_a, const libxsmm_blasint* stride_b, const libxsmm_blasint* stride_c,
  const void* a, const void* b, void* c, libxsmm_blasint batchsize, int ntasks);
// ---- calls recorded for later inside the opt-in bracket (xsmm_defer.cpp) --------------------------------------------------
// What is open on the calling thread: at most one kind, kept by xsmm_defer.cpp alone.
enum OpenKind : int { OPEN_NONE = 0,
  OPEN_BURST,   // per-call kernels or per-panel operator calls behind a gate on the stream (xsmm_defer.cpp)
  OPEN_BATCH,   // recorded libxsmm_gemm_batch calls (xsmm_batch_record.cpp)
  OPEN_SPMDM }; // recorded spmdm block calls (xsmm_sparse.cpp)
OpenKind record_open();
void record_begin(OpenKind kind);         // launches whatever other kind is open, then kind is open (nothing to do if it is already)
void record_flush();                      // nothing is open any more, then the flush function of the kind that was: it may ask for the stream
void batch_flush_record();                // the flush functions of the records, for record_flush() alone: launch what was recorded
void spmdm_flush_record();
struct Kernel;
bool defer_call(Kernel* k, const void* a, const void* b, void* c);  // true: recorded (runs later, in stream order)
struct JitKernel;
// per-panel calls of a fixed operator (libxsmm_?fsspmdm_execute) that walk along the rows of B and C: recorded like per-product calls
bool defer_panels(const void* handle, JitKernel* jit, const void* B, void* C, int typesize, int M, int N, int K, long long ldb, long long ldc, int vec);
bool defer_bracket_open();                // the calling thread is inside libxsmm_amd_defer_begin/end
bool defer_capturing(void* stream);       // the stream is being captured (or cannot be asked): nothing is recorded for later
constexpr int BATCH_HULL_CALLS = 32;      // calls per hull launch (as many as a C-ordering check launch takes)
// Address hulls of up to BATCH_HULL_CALLS index / pointer batches whose arrays live in device memory (kernels/batch_hull.hip).
// span_bytes: 3 per call (A, B, C); d_out: device unsigned long long [2][3 * BATCH_HULL_CALLS], initialised here on the stream:
// the lowest address of operand o of call c in d_out[3 * c + o], the highest (span included) in d_out[3 * BATCH_HULL_CALLS + 3 * c + o].
int launch_batch_hulls(const SmmBatch* calls, const unsigned long long* span_bytes, int ncalls, unsigned long long* d_out, void* stream);

// CSR "register" kernel family (fsspmdm sparse path, libxsmm_create_?csr_reg): row-major
// C[m*ldc+n] = (beta? C:0) + sum_p val[p]*B[col[p]*ldb+n], rows without nnz untouched.
struct CsrPanels {
  int typesize;
  int m, k;                  // operator shape
  int n;                     // panel width per item (multiple of the reference's chunk; any n >= 1 here)
  int ldb, ldc;
  int beta0;
  int skip_empty_rows;       // 1: reference's csr_reg quirk (rows without nnz are not written even when beta == 0)
  const unsigned* rowptr; const unsigned* colidx; const void* values; // device
  unsigned nnz;
  const void* b; void* c;    // device; panel i starts at column i*n
  long long batch;
};
int launch_csr_panels(const CsrPanels& args, void* stream, const char** name);

// run-time specialised operator kernels (xsmm_jit.cpp)
struct JitKernel;
std::string gen_csr_panels_source(int typesize, int M, int K, const unsigned* rowptr, const unsigned* colidx, const double* values,
                                  int beta0, int skip_empty_rows, int vec, const char* fname, bool burst_args = false);
JitKernel* jit_compile(const std::string& src, const char* fname, std::string* log);
JitKernel* jit_from_cache(const std::string& src, const char* fname); // only if the code-object cache on disk holds it
int jit_build_offline(const std::string& src, std::string* log);      // compile into the cache on disk (no device needed); 0: there
bool jit_async_enabled();                                             // LIBXSMM_AMD_JIT_ASYNC (default on)
void jit_async(std::function<void()> job);                            // run on the compiler thread
void jit_async_wait();
void jit_async_drain(); // drop queued compile jobs, wait for the running one                                                // until the compiler thread has nothing left to do
int jit_check_source(const std::string& src, std::string* log, std::string* built = nullptr); // *built: the text the library builds for src
void jit_release(JitKernel* k);
int jit_launch_panels(JitKernel* k, const void* B, void* C, long long ncols, long long ldb, long long ldc, int vec, void* stream,
                      const unsigned long long* npanels = nullptr, long long panel = 0);
int jit_blocks_per_cu(JitKernel* k, int threads); // occupancy of a generated kernel (0: unknown)
int jit_launch_args(JitKernel* k, unsigned blocks, unsigned threads, void** args, void* stream);
// dense SMM kernels specialised per shape (xsmm_jit_smm.cpp)
enum { SMM_JIT_SCALAR = 1, SMM_JIT_RUNS = 2, SMM_JIT_WGRUNS = 4, SMM_JIT_HASWG = 8, SMM_JIT_BIG = 16, SMM_JIT_SPLIT = 32,
       SMM_JIT_MFMA = 64 /* matrix-core work-group kernel (kernels/smm_mfma_wg.inc) with the shape baked in; + 128: tight fp32 operands as 16-byte chunks */, SMM_JIT_MFMA_TIGHT = 128, SMM_JIT_MFMA_TIGHTC = 8192 /* fp32: C as a contiguous array through LDS */,
       SMM_JIT_MFMA_WAVE = 16384 /* matrix-core kernel with one wave per item (16x16x4 tiles) */,
       SMM_JIT_MFMA_WAVE2 = 32768 /* ... the columns of C in two halves against one image of A (fp64 56^3: the images of a whole item leave no room for four waves per CU) */,
       SMM_JIT_MFMA_RUNS = 65536 /* run form on the matrix cores: a wave per run, A fragments straight from memory, B through LDS (M, N <= 32) */,
       SMM_JIT_DEEP = 131072 /* grouped bodies of a batch split into tiles of C: few waves on the chip, as many products in flight per wave as the wait counter allows */ }; // variant bits of the generated dense kernel
std::string gen_smm_source(int typesize, int m, int n, int k, int flags, int variant, int lda = 0, int ldb = 0, int ldc = 0); // (0: tight)
bool smm_jit_eligible(const SmmBatch& s);
int launch_smm_jit_mfma(const SmmBatch& s, void* stream, const char** name); // matrix-core kernels specialised per descriptor (before the hand-written ones); -1: none ready
int launch_smm_jit(const SmmBatch& s, void* stream, const char** name); // the other specialised kernels, 16-bit inputs included; -1: none ready
int smm_skip_mask(); // XSMM_SMMJIT_SKIP: links of the launch chains treated as not ready (bits 0-7: alternatives of a plan by position, bit 8: launch_smm_special)
constexpr int SMM_SKIP_SPECIAL = 256;
std::string smm_plan_describe(const SmmBatch& s, bool check_tiles, int* failed); // the plan of a batch as text (diagnostic; no device needed)
bool smm_jit_grouped_eligible(const SmmBatch& s);
int smm_jit_prebuild(const SmmBatch* shapes, int nshapes, int grouped, int* built); // code objects into the cache on disk; returns failures
std::string gen_smm_grouped_source_for(const SmmBatch* groups, int ngroups, bool tiles = false);
int launch_smm_jit_grouped(const SmmBatch* groups, int ngroups, void* stream, const char** name); // several batches, one launch; -1: not available
int launch_c_order_check_groups(const SmmBatch* groups, int ngroups, void* stream); // one check launch for up to 32 batches (each with its devflags slot)
int jit_launch_dyn(JitKernel* k, unsigned blocks, unsigned threads, unsigned lds_bytes, void** args, void* stream);

// spmdm batch
struct SpmdmGeom {
  int m, n, k; long long batch;
  int cap;      // colidx/values capacity per item (m*k rounded up to even: slots stay dword-aligned)
  int rstride;  // rowidx entries per item (m+1 rounded up to even)
};
int launch_spmdm_create(const SpmdmGeom& g, int transa, const float* a, uint16_t* rowidx, uint16_t* colidx, float* values,
                        void* stream, const char** name);
int launch_spmdm_compute(const SpmdmGeom& g, int transb, int transc, float beta, const uint16_t* rowidx, const uint16_t* colidx,
                         const float* values, const float* b, float* c, void* stream, const char** name);

// blocked_gemm helpers (layouts of template/libxsmm_blocked_gemm_copy*.tpl.c)
int launch_bf16_widen(const unsigned short* src, float* dst, long long count, void* stream); // dst[i] = float(bits(src[i]) << 16)
struct BgemmGeom { int typesize, m, n, k, bm, bn, bk, mb, nb, kb; };
int launch_bgemm_copy(const BgemmGeom& g, int which /*0:A 1:B 2:C-in 3:C-out 4:convert_b_to_a 5:transpose_b (blocked -> blocked)*/, const void* src, int ld, void* dst, void* stream);
int launch_bgemm_compute(const BgemmGeom& g, int beta0, const void* a, const void* b, void* c, void* stream, const char** name);

// ---- host runtime ------------------------------------------------------------------------------------
struct Device {
  int count = -1;           // -1: not probed
  void* stream = nullptr;   // hipStream_t
};
Device& device();
Device& device_raw();                     // the same without launching what is open on the thread (record_flush)
bool device_ready();                      // probes once; false if no HIP device
void fail_no_device(const char* what);    // prints a loud error (always) -- the product has no CPU compute path
bool is_device_ptr(const void* p);
int pointer_kind(const void* p);         // bit 0: the GPU reaches it; bit 1: pinned host / managed memory (the CPU addresses it as well)
bool is_host_visible(const void* p);      // pinned host or managed memory (processed in place, but the CPU reads it directly)
void settle(const void* p0, const void* p1 = nullptr, const void* p2 = nullptr); // wait for the stream if an operand is host-visible
int flag_slot_set(int* slot, int equal_pairs, int decreasing_pairs); // the verdict without a check kernel (0: ok)
constexpr int INDEX_UPLOAD_RING = 256;   // staged arrays a thread may hold before index_upload_commit (a grouped call stages three arrays per group plus its table)
void* index_upload(const void* host_array, size_t bytes); // async copy of a host index array to the device (nullptr: failed)
void* index_upload_on(void* stream, const void* host_array, size_t bytes); // the same without asking for the stream
void index_upload_commit();                                // after the launches that read uploaded arrays were queued
int library_gemm(int typesize, int transa, int transb, int m, int n, int k, double alpha, const void* a, int lda,
                 const void* b, int ldb, double beta, void* c, int ldc); // rocBLAS on the engine's stream; -1: not available
int* flag_slot();                         // device int[4] for one batch call's C-ordering verdict (nullptr: out of memory)
void flag_slot_commit();                  // after the launches that read the calling thread's latest slot were queued
void* dev_alloc(size_t bytes);
void dev_free(void* p);
int h2d(void* dst, const void* src, size_t bytes);
int d2h(void* dst, const void* src, size_t bytes);
int stream_sync();
void note_launch(const char* name);

// grow-only device scratch, one per thread-local slot id
void* scratch(int slot, size_t bytes);

enum KernelClass : int { KC_DENSE = 0, KC_REDUCE = 1, KC_CSR_REG = 2, KC_TEXT = 3 /* pattern kernel compiled from generated text (SOA family) */,
  KC_LOWP = 4 /* i16 / bf16 inputs (kernels/smm_lowp.hip) */,
  KC_PACKED = 5 /* pgemm / getrf / trmm / trsm over packs of interleaved matrices (xsmm_packed.cpp) */,
  KC_XCOPY = 6 /* matrix copy / transposition kernels (libxsmm_dispatch_mcopy / _trans, xsmm_xcopy.cpp) */ };

struct Kernel {                 // what a dispatched function pointer stands for
  libxsmm_gemm_descriptor desc;
  int kclass;
  bool registered;
  void* thunk;                  // the bare function pointer handed to the caller
  // KC_CSR_REG payload
  unsigned nnz = 0;
  unsigned* d_rowptr = nullptr; unsigned* d_colidx = nullptr; void* d_values = nullptr;
  // KC_TEXT payload: libxsmm_amd_spgemm* (xsmm_generator.cpp)
  void* text = nullptr;
  // KC_PACKED payload (xsmm_packed.cpp); desc is not used
  void* packed = nullptr;
  // KC_XCOPY payload: the descriptor's fields (mcopy: normalised to typesize 4 as the reference does); desc is not used
  int xkind = 0;                // LIBXSMM_KERNEL_KIND_MCOPY or _TRANS
  unsigned xm = 0, xn = 0, xldi = 0, xldo = 0, xtypesize = 0, xflags = 0, xprefetch = 0;
};

Kernel* kernel_from_pointer(const void* fn);           // NULL if fn is not one of ours
void* adopt_kernel(Kernel* k);                         // caller-owned kernel: make its thunk and index it; NULL on failure
int text_kernel_execute(void* text, const void* a, const void* b, void* c, long long stride_dense, long long stride_c, long long batch);
void text_kernel_destroy(void* text);
void* make_thunk(Kernel* k);                           // executable stub carrying k
void free_thunk(void* thunk);
void call_kernel(Kernel* k, const void* a, const void* b, void* c, const void* x3, const void* x6); // what a thunk does (x3, x6: the 4th and 7th argument of the call)

// packed kernels (xsmm_packed.cpp)
// Registered kernels whose key is not a GEMM descriptor: the kernel for these descriptor bytes (tag: kept apart from the GEMM keys),
// made by make(desc) if the registry does not hold it yet (nullptr: not supported). Returns the kernel's function pointer.
void* registry_dispatch(const void* desc, size_t size, int tag, Kernel* (*make)(const void* desc));
void packed_destroy(void* packed);                     // the payload of a packed kernel (Kernel::packed)
int packed_kind(const Kernel* k);                      // LIBXSMM_KERNEL_KIND_PGEMM ... TRSM
void packed_call(Kernel* k, const void* a, const void* b, void* c); // what the thunk of a packed kernel does
// the operands of one call as a burst sees them: rd[2] what is only read (bytes 0: none), wr what is written (and read)
struct PackedOps { const void* rd[2]; size_t rd_bytes[2]; void* wr; size_t wr_bytes; };
bool packed_operands(const Kernel* k, const void* a, const void* b, void* c, PackedOps* ops); // false: not fit for a burst (alignment)
// the batch kernel of a burst: pack p takes its operands from ring[3 * p ...], the number of packs from *count (at most capacity)
int packed_launch_burst(Kernel* k, const void* ring, const unsigned long long* count, int capacity, void* stream, const char** name);

// matrix copy / transposition (xsmm_xcopy.cpp, kernels/xcopy.hip)
void xcopy_call(Kernel* k, const void* in, const void* ldi, void* out, const void* ldo); // what the thunk of an mcopy / trans kernel does
// A stack of items for the kernels of kernels/xcopy.hip, every length in units of `unit` bytes (an element is P units).
struct StackMove {
  const void* in; void* out;    // first items, or arrays of item pointers (ptrs != 0)
  long long sin, sout;          // units from one item to the next (ptrs == 0)
  long long ldi, ldo;           // units from one column to the next
  int m, n, P;                  // rows, columns (of the input; copy: of both), units per element
  int mp, G;                    // through LDS: units per column of an item's image, items per chunk (0: not through LDS)
  long long batch;
  int ptrs;
  int s1[3], s2[4]; long long sg; // filled in by the launcher: the steps of the kernels' running indexes
};
enum { XCOPY_STACK_TRANS = 0, XCOPY_STACK_COPY = 1, XCOPY_STACK_SWAP = 2 };
// all return hipError_t as int; unit: 1, 2, 4, 8 or 16 bytes, every address and pitch a multiple of it
int launch_xcopy_trans(int unit, const void* in, void* out, int m, int n, long long ldi, long long ldo, bool vec_in, bool vec_out, void* stream); // element = unit; vec_*: that side's base and pitch are multiples of 16 bytes
int launch_xcopy_itrans(int unit, void* inout, int n, long long ld, bool vec, void* stream);
int launch_xcopy_copy(int unit, const void* in, void* out, long long rowbytes, long long ncols, long long pitch_in, long long pitch_out, void* stream); // pitches in bytes; in == nullptr: zeros
int launch_xcopy_stack(int unit, const StackMove& args, int op, void* stream, const char** name);

// tiled GEMM (xsmm_tgemm.cpp, kernels/tgemm.hip)
constexpr int TGEMM_TILE = 128;           // the work-group tile of C is TGEMM_TILE x TGEMM_TILE; tasks are cut on its multiples
struct TgemmArgs {                        // C(m x n) = op(A) * op(B) + (beta0 ? 0 : C); a: first row of op(A), b: first column of op(B)
  int typesize;                           // 8: f64, 4: f32
  int transa, transb, beta0;
  int m, n, k;
  long long lda, ldb, ldc;
  const void* a; const void* b; void* c;  // memory the GPU reaches
};
int launch_tgemm(const TgemmArgs& args, void* stream, const char** name); // returns hipError_t as int
// One rectangle {m0, m1, n0, n1} of C = op(A) * op(B) + (beta0 ? 0 : C) for a tiled kernel, operands in any memory and plain
// column-major: ti and to are the element sizes of A / B and of C. Memory the GPU reaches is processed in place, pageable
// spans of A and B are staged (scratch slots 3 and 4), a pageable C travels as a tight image of the rectangle (slot 5);
// host-visible memory is complete on return. launch queues the kernel for the rectangle's part of the operands as the GPU
// sees them and returns hipError_t as int plus the kernel's name. Returns EXIT_SUCCESS or EXIT_FAILURE.
typedef std::function<int(void* stream, const void* a, const void* b, void* c, long long ldc, int m, int n, const char** name)> RectLaunch;
int run_rect(size_t ti, size_t to, bool ta, bool tb, int beta0, long long k, long long lda, long long ldb, long long ldc,
  const unsigned int rect[4], const void* a, const void* b, void* c, const RectLaunch& launch, const char* what);
// the tiled GEMM for a libxsmm_?gemm call (opt-in LIBXSMM_AMD_TGEMM=1); false: not taken, the caller goes on as before
bool tgemm_route(int typesize, int flags, int m, int n, int k, int lda, int ldb, int ldc, double alpha, double beta, const void* a, const void* b, void* c);

// tiled GEMM for 16-bit inputs (xsmm_lowp_gemm.cpp, kernels/tgemm_lowp.hip); the first three are the kinds of the oracle's gold loops
enum LowpGemmKind : int { LOWP_I16_I32 = 0, LOWP_I16_F32 = 1, LOWP_BF16 = 2, LOWP_BF16_FAST = 3 /* v_mfma_f32_32x32x16_bf16: opt-in */ };
constexpr int TGEMM_LOWP_BK = 64;         // the k chunk of the bf16 kernels (the i16 kernels: half of it)
struct TgemmLowpArgs {                    // as TgemmArgs; a, b: 16-bit elements, c: 32-bit elements
  int kind;                               // LowpGemmKind
  int transa, transb, beta0;
  int m, n, k;
  long long lda, ldb, ldc;
  const void* a; const void* b; void* c;  // memory the GPU reaches
};
int launch_tgemm_lowp(const TgemmLowpArgs& args, void* stream, const char** name); // returns hipError_t as int

// quantisation and bf16 conversion (xsmm_quant.cpp, kernels/quant.hip)
enum QuantMode : int { QUANT_NO = 0, QUANT_BIAS = 1, QUANT_STOCH = 2, QUANT_NEAREST = 3, QUANT_FPHW = 4 }; // LIBXSMM_DNN_QUANT_*_ROUND - 80000
struct QuantHead {                        // what a quantise kernel needs besides its tensors
  int mode;                               // QuantMode
  unsigned add_shift, seed;               // seed: stochastic rounding
  const unsigned* maxword;                // device word written by launch_quant_absmax earlier on the same stream
  unsigned char* scf;                     // one byte the GPU reaches: written by the quantise kernel
};
struct QuantLayout {                      // libxsmm_dnn_quantize_act (fil == 0) / _fil (fil != 0; H, W stand for R, S)
  unsigned C, H, W, cb32, cb16, lp, cblk, kb32, kb16; // cblk = C / (cb16 * lp)
  int fil;
  long long total;                        // elements
};
struct QuantTiles { int CB, pitch, chunks; long long P, ptiles, ntiles; }; // filled in by launch_quant_act_tiled
// all return hipError_t as int; every pointer is memory the GPU reaches, aligned to its element
int launch_quant_absmax(const float* in, long long n, unsigned* maxword, void* stream); // zeroes the word on the stream first
int launch_quant_flat(const float* in, short* out, long long n, const QuantHead& h, void* stream);
int launch_quant_layout(const float* in, short* out, const QuantLayout& g, const QuantHead& h, void* stream); // any block sizes
// plain input (cb32 == 1), CB = cb16 * lp even, out aligned to 4 bytes: nblocks = N * C / CB slabs of CB rows of P = H * W pixels
int launch_quant_act_tiled(const float* in, short* out, long long nblocks, int CB, long long P, const QuantHead& h, void* stream);
int launch_dequant_flat(const short* in, float* out, long long n, float scale, void* stream);
int launch_bf16_narrow(int rounding /*0: truncate, 1: nearest-away, 2: nearest-even*/, const float* in, unsigned short* out, long long n, void* stream);

// matdiff on device operands (xsmm_matdiff.cpp, kernels/matdiff.hip)
constexpr int MATDIFF_FIELDS = 19;        // the doubles of libxsmm_matdiff_info, in its order
enum MatdiffField : int { MD_NORM1_ABS = 0, MD_NORM1_REL, MD_NORMI_ABS, MD_NORMI_REL, MD_NORMF_REL, MD_LINF_ABS, MD_LINF_REL, MD_L2_ABS, MD_L2_REL,
  MD_L1_REF, MD_MIN_REF, MD_MAX_REF, MD_AVG_REF, MD_VAR_REF, MD_L1_TST, MD_MIN_TST, MD_MAX_TST, MD_AVG_TST, MD_VAR_TST };
struct MatdiffRecord {                    // the finished statistics of one item, as the kernels pass them on
  double f[MATDIFF_FIELDS];
  long long m, n;                         // where linf_abs is (-1: nowhere), or the first non-finite test value (nan != 0)
  long long item;                         // the item that m, n belong to
  long long nan;
};
struct MatdiffArgs {                      // items of nn lines of mm contiguous elements; every length in elements
  int datatype;                           // libxsmm_datatype: F64, F32, I32, I16, I8
  int vec_ref, vec_tst;                   // that operand's base, pitch and stride allow one load per MATDIFF_VEC elements
  long long mm, nn, ldr, ldt;
  long long sr, st, batch, item0;         // item i at ref + i * sr and is reported as item0 + i
  const void* ref; const void* tst;       // memory the GPU reaches; tst may be NULL
};
bool matdiff_small(long long mm, long long nn);             // a wave takes a whole item (launch_matdiff_items), else tiles
size_t matdiff_tiled_workspace(const MatdiffArgs& a);       // bytes launch_matdiff_tiled needs
long long matdiff_reduce_records(long long count);          // records one level of launch_matdiff_reduce leaves
// all return hipError_t as int
int launch_matdiff_items(const MatdiffArgs& a, MatdiffRecord* rec /* [batch] */, void* stream);
int launch_matdiff_tiled(const MatdiffArgs& a /* batch == 1 */, void* workspace, MatdiffRecord* rec, void* stream);
int launch_matdiff_reduce(const MatdiffRecord* in, long long count, MatdiffRecord* out, void* stream);
int launch_matdiff_emit(const MatdiffRecord* rec, long long count, libxsmm_matdiff_info* out, long long* item_out, int swap_norms, int swap_ref,
  double avg_size, void* stream);
// libxsmm_matdiff with an operand in plain device memory; false: both are host memory (or there is no device), *rc untouched
bool matdiff_route(libxsmm_matdiff_info* info, libxsmm_datatype datatype, libxsmm_blasint m, libxsmm_blasint n, const void* ref, const void* tst,
  const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst, int* rc);

// hash and byte compare on device operands (xsmm_hash.cpp, kernels/hash.hip; the geometry is kernels/hash_plan.h)
struct HashArgs {
  const void* a; const void* b;           // memory the GPU reaches; b: the compare only
  unsigned long long line_bytes;          // an item is `lines` lines of line_bytes bytes, lda / ldb bytes apart, taken as one run of bytes
  long long lines, lda, ldb, stride_a, stride_b, batch;
  long long item0;                        // the index of the first item of this launch in the caller's batch
  unsigned int seed; int compare;         // compare: 0 / 1 per item instead of the hash
};
struct DiffKey { unsigned char b[256]; }; // the `a` of libxsmm_diff_n when it is host memory: it travels as a kernel argument
// all return hipError_t as int; first: a workspace word that takes the lowest differing item (or NULL)
int launch_hash_items(const HashArgs& a, unsigned int* results /* [batch] */, long long* first, void* stream);        // hash_small() items
int launch_hash_units(const HashArgs& a /* one item */, unsigned int* partial /* [HASH_MAX_BLOCKS] */, unsigned int* result, long long* first, void* stream);
int launch_hash_first(long long* first, long long* out, bool clear, void* stream); // clear: before the items; else *out = the index or -1
int launch_diff_n(const DiffKey& key, const void* a /* NULL: the key */, const void* bn, unsigned int size, unsigned int stride, unsigned int hint, unsigned int n,
  unsigned int* best /* workspace: the least (i - hint) mod n of a match, 0xffffffff if none */, void* stream);

// fully-connected layer (xsmm_dnn_fc.cpp, kernels/fc.hip): D(i, j) = chain over r of P(i, r) * Q(r, j), blocked operands
struct FcDim { int blk; long long outer, inner; }; // index x lies at (x / blk) * outer + (x % blk) * inner elements; a plain dimension: blk >= extent
constexpr int FC_PLAIN = 1 << 30;         // blk of a dimension that is not blocked
struct FcArgs {
  const void* p; const void* q; void* d;  // memory the GPU reaches
  FcDim pi, pr, qr, qj, di, dj;           // the address of an element is the sum of its two dimensions' parts
  int p_bf16, q_bf16, d_bf16;             // 16-bit elements: widened on load (bits << 16), rounded to nearest even on store
  int p_rfast, q_rfast;                   // the operand's fast dimension in memory is r: how a work-group's loads are laid over a chunk
  int R;                                  // length of the chains
  int i0, i1, j0, j1;                     // the rectangle of D this launch covers (tiles are laid out from i0, j0)
  // a share that is no rectangle: the element (i, j) belongs to block (i / sbi) * mi + (j / sbj) * mj and is stored if w0 <= block < w1
  int masked, sbi, mi, sbj, mj, w0, w1;
  int tile;                               // 64 or 128
};
int launch_fc(const FcArgs& args, void* stream, const char** name); // returns hipError_t as int

int verbosity();
bool once(int* flag);   // true the first time

} // namespace xsmm

#endif
