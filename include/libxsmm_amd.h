/*
 * libxsmm_amd.h -- engine-specific additions to the LIBXSMM C-ABI (no counterpart in the reference).
 *
 * The reference is a CPU library: a kernel call returns when C is written. On MI355X the operands
 * normally live in HBM and a call only enqueues work on a HIP stream. These entry points expose that
 * model (stream, synchronisation, device allocation) plus batch forms for the paths whose reference
 * API processes one problem per call (spmdm, fsspmdm) -- the batch axis is what fills 256 CUs.
 */
#ifndef LIBXSMM_AMD_H
#define LIBXSMM_AMD_H

#if !defined(LIBXSMM_H)
# include "libxsmm.h"
#endif

/* ---- device / stream ------------------------------------------------------------------------ */
/** Number of usable HIP devices (0: none; every compute entry point then fails loudly). */
LIBXSMM_API int libxsmm_amd_device_count(void);
/** HIP stream (hipStream_t) on which the calling thread's device-resident work is enqueued; NULL selects the default
 *  stream. The setting is per thread (every entry point may be called from any thread): independent batches can be put
 *  on different streams, by one thread switching streams between calls or by several threads. */
LIBXSMM_API void libxsmm_amd_set_stream(void* hip_stream);
LIBXSMM_API void* libxsmm_amd_get_stream(void);
/** Calls of a dispatched kernel on device memory, kernel(a, b, c) once per product (samples/smm/specialized.cpp:172-190;
 *  likewise libxsmm_?fsspmdm_execute once per panel, samples/pyfr/pyfr_driver_asp_reg.c:300-308).
 *  DEFAULT: every call is an asynchronous launch of its own on the calling thread's stream; stream order is call order,
 *  so work the caller queues on that stream between two calls (own kernels, hipMemcpyAsync, torch operations) is
 *  ordered between them exactly as it was issued.
 *  OPT-IN, no launch per call: between libxsmm_amd_defer_begin() and libxsmm_amd_defer_end() on the calling thread (the
 *  analogue of the reference's libxsmm_mmbatch_begin/end bracket, src/libxsmm_ext_gemm.c:1016-1135; brackets nest), or
 *  process-wide with LIBXSMM_AMD_DEFER=1, consecutive calls form a burst: the first call queues a gate kernel and the
 *  batch kernel behind it on the stream, the following calls only append their operands to a ring in pinned memory and
 *  RUN AT THE STREAM POSITION OF THE BURST'S FIRST CALL. The caller's side of the contract: inside the bracket, before
 *  queueing work of its own on that stream that reads or writes operands of the calls -- call libxsmm_amd_flush().
 *  Work queued or waited for after libxsmm_amd_defer_end() / libxsmm_amd_flush() / any other entry point of the library
 *  on the thread is ordered behind all recorded calls (an idle burst is also sealed by a helper thread after a few
 *  microseconds, so a caller's hipStreamSynchronize inside the bracket never hangs). Calls that depend on each other
 *  (a C read as A by a later call, a C written again later) are detected from the operand addresses and keep the call
 *  order. libxsmm_amd_defer_active(): 1 if calls of this thread are being recorded.
 *  Inside a bracket (not with the environment variable alone) the block calls of the spmdm interface on device operands,
 *  libxsmm_spmdm_createSparseSlice_*_thread / libxsmm_spmdm_compute_*_thread (samples/spmdm/spmdm.c:99-109), are recorded
 *  as well: consecutive calls of one kind on one handle with the same operands merge into rectangles of blocks, launched
 *  -- one kernel per rectangle, one for a full sweep -- by whatever ends the record (a call of another kind or with other
 *  operands, libxsmm_amd_flush / libxsmm_amd_defer_end, any other entry point of the library on the thread). They run at
 *  the stream position of THAT moment; every block still touches only its own slices / C tile.
 *  Inside a bracket (again not with the environment variable alone) batch calls are recorded too: libxsmm_gemm_batch,
 *  libxsmm_gemm_batch_omp, libxsmm_mmbatch[_kernel] with one task and the group loops of libxsmm_?gemm_batch[_omp] -- the
 *  caller's loop with one call per shape (samples/cp2k/cp2k.cpp:328-360). RECORDED is a call in the SMM domain (alpha 1,
 *  beta 0 or 1, no TRANS_A; f32 / f64) with index arrays or arrays of pointers, whose matrices the GPU reaches and whose C
 *  the CPU does not address, on a stream that is not being captured. Index / pointer arrays the CPU addresses are copied
 *  when the call is made: the caller may overwrite them as soon as the call returns. The MATRICES fall under the bracket's
 *  contract above (libxsmm_amd_flush() before the caller's own work on the stream touches them), and arrays in device
 *  memory are read at the flush, so they belong to the operands in this respect. The recorded calls RUN AT THE STREAM
 *  POSITION OF THE FLUSH: libxsmm_amd_flush, the outermost libxsmm_amd_defer_end (an inner one leaves the record open), a
 *  call that cannot be recorded (it runs behind the recorded ones), a change of precision, any other entry point of the
 *  library on the thread (libxsmm_amd_synchronize included), or a 65th call (a record holds at most 64 calls; the next one flushes it first). At the flush the calls are cut, in
 *  call order, into segments of consecutive calls that are independent of each other (libxsmm_amd_merge_segments); every
 *  segment is one fused launch like libxsmm_amd_gemm_batch_groups (one C-ordering check, one multiplication where the
 *  shape-specialised run kernels apply), segment after segment: calls that depend on each other keep the call order, and the
 *  sums per C block are formed as outside the bracket. Independence is judged by the address ranges the operands of a call
 *  span. For arrays the CPU addresses these were noted at the call; for arrays in device memory a small kernel computes them
 *  at the flush and the host reads its table back (48 bytes per call): THE ONE WAIT FOR THE STREAM this path adds, at most
 *  once per flush and only when a recorded call had its arrays in device memory. Do not begin a stream capture with a record
 *  open (flush first): calls recorded before the capture would become part of the graph, and since nothing may be waited for
 *  inside a capture, calls with arrays in device memory then run one after the other. A thread ends its brackets before it ends. */
LIBXSMM_API void libxsmm_amd_defer_begin(void);
LIBXSMM_API void libxsmm_amd_defer_end(void);
LIBXSMM_API int libxsmm_amd_defer_active(void);
LIBXSMM_API void libxsmm_amd_flush(void);
/** The segments recorded batch calls leave in (see above), as a pure function: n calls in call order, hulls[6 * i ...] =
 *  {a_lo, a_hi, b_lo, b_hi, c_lo, c_hi} of call i -- the byte addresses its A, B and C operands span, half-open ranges
 *  [lo, hi). Two ranges meet if they share a byte (ranges that only touch, hi == lo, do not). Call i joins the open segment
 *  unless its C meets the A, B or C of a member or its A or B meets the C of a member; then it opens a new segment.
 *  segment_of[i] receives the segment of call i (0, 1, ...); returns the number of segments (0 for n == 0), -1 for bad arguments. */
LIBXSMM_API int libxsmm_amd_merge_segments(int n, const unsigned long long hulls[], int segment_of[]);
/** DIAGNOSTIC, not a stable part of the interface (it may change or go without notice; the tests use it to see which path a
 *  flush took). What the calling thread's last flush of recorded batch calls did: the number of calls, of segments, of
 *  calls whose hulls the device computed (-1: the hulls could not be had and the calls ran one after the other), and -- for
 *  the first `capacity` calls -- the hulls (6 per call) and segments as for libxsmm_amd_merge_segments. Any pointer may be
 *  NULL. Returns the number of calls written. */
LIBXSMM_API int libxsmm_amd_merge_last_plan(int* ncalls, int* nsegments, int* ndevice_hulls, unsigned long long hulls[], int segment_of[], int capacity);
/** DIAGNOSTIC, not a stable part of the interface (the tests use it to hold the launch plans against a table of cases). The plan of a
 *  dense batch as text: the ordered alternatives of both tiers that a batch call tries before the pre-compiled kernels serve. No device
 *  is needed and nothing is compiled or launched. mode: 0 strided, 1 index arrays, 2 pointer arrays; sync: 0 every item its own C,
 *  1 C in runs known to the host, 3 the verdict on the device; the strides are those of a strided batch (elements); address_bits: the
 *  low bits of the operands' addresses (0: aligned to 16 bytes); mfma: matrix cores on or off; lowp: 0, or 1 i16 -> i32, 3 bf16 -> f32,
 *  4 bf16 -> bf16 (the descriptor then gives the shape and leading dimensions only). One line per alternative:
 *    <position> <mfma|jit> <name> parts=<n> [<variant bits>:<all|packed|rest> ...] tiles=<n> [<m>x<n>:<variant bits> ...]
 *  compile_tiles != 0: the grouped kernel text of an alternative that runs the tiles of C is compiled for gfx950 as well.
 *  Returns the length of the text (an empty plan: 0), -1 for arguments out of range, -2 if such a text did not compile. */
LIBXSMM_API int libxsmm_amd_smm_plan_describe(const libxsmm_gemm_descriptor* descriptor, int mode, int sync, long long batch,
  long long stride_a, long long stride_b, long long stride_c, unsigned int address_bits, int relaxed, long long uniform_run, int mfma, int lowp,
  char* buffer, size_t buffer_size, int compile_tiles);
/** Block until all work enqueued by this library on its stream has completed. Returns EXIT_SUCCESS/FAILURE. */
LIBXSMM_API int libxsmm_amd_synchronize(void);
/** Device memory (hipMalloc/hipFree) -- what libxsmm_malloc returns when a device is present is host-pinned
 *  memory (usable by unchanged callers); these return HBM. */
LIBXSMM_API void* libxsmm_amd_device_malloc(size_t size);
LIBXSMM_API void libxsmm_amd_device_free(void* ptr);
LIBXSMM_API int libxsmm_amd_memcpy_h2d(void* dst_device, const void* src_host, size_t size);
LIBXSMM_API int libxsmm_amd_memcpy_d2h(void* dst_host, const void* src_device, size_t size);
/** 1 if ptr is device-accessible memory (hipMalloc, managed, or pinned host), else 0. */
LIBXSMM_API int libxsmm_amd_is_device_pointer(const void* ptr);

/* ---- kernel selection ----------------------------------------------------------------------- */
/** MFMA policy for dense SMM: 0 = scalar-FMA kernels only (bit-identical to a k-ordered fma chain),
 *  1 = use v_mfma_* where the shape maps onto matrix-core tiles (default; env LIBXSMM_AMD_MFMA).
 *  Returns the previous value. */
LIBXSMM_API int libxsmm_amd_set_mfma(int mode);
LIBXSMM_API int libxsmm_amd_get_mfma(void);
/** Name of the device kernel variant chosen for the most recent launch of the calling thread
 *  (e.g. "smm_f32_32x32x32_mfma"); "" if nothing was launched. Used by the tests to prove that the
 *  native path ran. */
LIBXSMM_API const char* libxsmm_amd_last_kernel(void);
/** Number of device kernel launches issued by this process (monotonic). */
LIBXSMM_API unsigned long long libxsmm_amd_launch_count(void);
/** DIAGNOSTIC, not a stable part of the interface: the number of launches of run-time specialised dense kernels by this process
 *  (monotonic). An alternative of a launch plan that has two parts makes two, the pre-compiled kernels make none; the tests tell
 *  alternatives of one name apart by it. */
LIBXSMM_API unsigned long long libxsmm_amd_jit_launch_count(void);

/** Measurement aid: c[i] += a[i] + b[i] over `bytes` bytes per operand (device memory, 16-byte aligned) -- the
 *  3-read/1-write traffic mix of a beta=1 SMM batch with no arithmetic; bench.py reports its rate as the measured
 *  streaming ceiling next to the 8 TB/s datasheet peak. */
LIBXSMM_API int libxsmm_amd_stream_probe(const void* a, const void* b, void* c, long long bytes);

/* ---- batch forms ---------------------------------------------------------------------------- */
/** Constant-stride batch: item i uses a + i*stride_a, b + i*stride_b, c + i*stride_c (strides in elements,
 *  0 = operand shared). This is the layout of samples/smm/specialized.cpp:143-146,172-190 (contiguous
 *  A[s][m*k], B[s][k*n], C[s][m*n]) without materialising index arrays. Device-resident operands only.
 *  Returns EXIT_SUCCESS, or EXIT_FAILURE if the descriptor is not supported / no device. */
LIBXSMM_API int libxsmm_amd_gemm_batch_strided(const libxsmm_gemm_descriptor* descriptor,
  const void* a, const void* b, void* c, long long stride_a, long long stride_b, long long stride_c,
  long long batchsize);

/** Several index-array batches in one call -- CP2K-style stacks: one batch per shape (samples/cp2k/cp2k.cpp:328-360;
 *  the reference's one-call form for pointer arrays is libxsmm_?gemm_batch with its groups, src/libxsmm_gemm.c:1231-1262).
 *  Equivalent to libxsmm_gemm_batch(iprec, oprec, &transa[g], &transb[g], m[g], n[g], k[g], alpha, a[g], &lda[g], b[g],
 *  &ldb[g], beta, c[g], &ldc[g], index_base, index_stride, stride_a[g], stride_b[g], stride_c[g], group_size[g]) for every
 *  g < ngroups, with the groups' launches fused: the C-ordering check of all groups is one launch and, where the
 *  shape-specialised run kernels apply (M, N <= 32, K <= 64), so is the multiplication -- the accumulation chains of all
 *  shapes are resident at the same time instead of one shape after the other. Per C block the products are added in batch
 *  order as in libxsmm_gemm_batch (relaxed != 0: any order, as libxsmm_gemm_batch_omp). The groups must be independent of
 *  each other: no C block is written by two groups and no group reads (as A or B) what another group writes -- the
 *  fused groups run side by side (libxsmm_?gemm_batch with pointer arrays checks this itself and keeps dependent groups in
 *  order). transa/transb/lda/ldb/ldc may be NULL ('N', tight leading dimensions);
 *  alpha/beta: scalars of the precision (NULL: 1), the SMM domain only (alpha = 1, beta in {0, 1}, no TRANS_A). Matrices in
 *  device memory (or libxsmm_malloc memory); index arrays in device or host memory. Returns EXIT_SUCCESS/EXIT_FAILURE. */
LIBXSMM_API int libxsmm_amd_gemm_batch_groups(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, int ngroups,
  const char transa[], const char transb[], const libxsmm_blasint m[], const libxsmm_blasint n[], const libxsmm_blasint k[],
  const libxsmm_blasint lda[], const libxsmm_blasint ldb[], const libxsmm_blasint ldc[], const void* alpha, const void* beta,
  const void* const a[], const void* const b[], void* const c[], libxsmm_blasint index_base, libxsmm_blasint index_stride,
  const libxsmm_blasint* const stride_a[], const libxsmm_blasint* const stride_b[], const libxsmm_blasint* const stride_c[],
  const libxsmm_blasint group_size[], int relaxed);

/** Batched spmdm: `batch` independent problems of the handle's geometry (M,N,K), operands back to back
 *  (A: M*K, B: K*N, C: M*N elements per item, layouts/transposes as libxsmm_spmdm_*_thread).
 *  The CSR scratch lives in HBM and is owned by the returned object. */
typedef struct libxsmm_amd_spmdm_batch libxsmm_amd_spmdm_batch;
LIBXSMM_API libxsmm_amd_spmdm_batch* libxsmm_amd_spmdm_batch_create(int M, int N, int K, long long batch);
LIBXSMM_API void libxsmm_amd_spmdm_batch_destroy(libxsmm_amd_spmdm_batch* sb);
/** dense A (device) -> per-item CSR slices (uint16 column indexes, identical content/order to
 *  libxsmm_spmdm_createSparseSlice_fp32_thread on every item). */
LIBXSMM_API int libxsmm_amd_spmdm_batch_create_slices(libxsmm_amd_spmdm_batch* sb, char transa, const float* a);
/** C = beta*C + A_sparse*B for every item (alpha ignored as in the reference). */
LIBXSMM_API int libxsmm_amd_spmdm_batch_compute(libxsmm_amd_spmdm_batch* sb, char transb, const float* b,
  char transc, const float* beta, float* c);
/** Geometry and CSR access for tests: copies item `i`'s rowidx (M+1), and the first nnz colidx/values to host. */
LIBXSMM_API int libxsmm_amd_spmdm_batch_get_slice(const libxsmm_amd_spmdm_batch* sb, long long item,
  uint16_t* rowidx, uint16_t* colidx, float* values, int capacity);

/** The reference spmdm interface in one call per phase: what the caller's loop over block ids does
 *  (samples/spmdm/spmdm.c:74-112: libxsmm_spmdm_createSparseSlice_fp32_thread for every id below
 *  libxsmm_spmdm_get_num_createSparseSlice_blocks, then libxsmm_spmdm_compute_fp32_thread for every id below
 *  libxsmm_spmdm_get_num_compute_blocks), as one launch over the whole problem. The *_thread functions keep the reference's
 *  contract -- a call touches the slice resp. the C tile of its block id and nothing else -- and cost one launch per block;
 *  these are for callers that own the whole loop. Same operands and semantics (alpha ignored, beta == 0 never reads C);
 *  device or host operands. Returns EXIT_SUCCESS/EXIT_FAILURE. */
LIBXSMM_API int libxsmm_amd_spmdm_createSparseSlice_all(const libxsmm_spmdm_handle* handle, char transa, const float* a,
  libxsmm_CSR_sparseslice* libxsmm_output_csr_a);
LIBXSMM_API int libxsmm_amd_spmdm_compute_all(const libxsmm_spmdm_handle* handle, char transa, char transb, const float* alpha,
  libxsmm_CSR_sparseslice* a_sparse, const float* b, char transc, const float* beta, float* c);
LIBXSMM_API int libxsmm_amd_spmdm_createSparseSlice_bfloat16_all(const libxsmm_spmdm_handle* handle, char transa, const libxsmm_bfloat16* a,
  libxsmm_CSR_sparseslice* libxsmm_output_csr_a);
LIBXSMM_API int libxsmm_amd_spmdm_compute_bfloat16_all(const libxsmm_spmdm_handle* handle, char transa, char transb, const libxsmm_bfloat16* alpha,
  libxsmm_CSR_sparseslice* a_sparse, const libxsmm_bfloat16* b, char transc, const libxsmm_bfloat16* beta, float* c);

/** Batched fsspmdm: the operator of `handle` applied to `batch` column panels of width handle->N that sit
 *  side by side in B (K x ldb) / C (M x ldc): panel i = columns [i*N, (i+1)*N). Equivalent to calling
 *  libxsmm_?fsspmdm_execute(handle, B + i*N, C + i*N) for every i (samples/pyfr/pyfr_driver_asp_reg.c:295-309). */
LIBXSMM_API int libxsmm_amd_dfsspmdm_execute_batch(const libxsmm_dfsspmdm* handle, const double* B, double* C, long long batch);
LIBXSMM_API int libxsmm_amd_sfsspmdm_execute_batch(const libxsmm_sfsspmdm* handle, const float* B, float* C, long long batch);

/** Text generator: the HIP source a fixed-sparsity operator (CSR pattern + values) is specialised to -- every referenced B
 *  row is loaded once, every non-zero is one fma with an immediate. This is what libxsmm_?fsspmdm_create compiles through
 *  hiprtc (counterpart of the reference's libxsmm_generator_spgemm_csr_kernel text output). The source is copied into
 *  `buffer` (truncated to buffer_size). compile == 0: returns the source length; compile != 0: additionally compiles it for
 *  gfx950 (no device needed) and returns 0 on success, > 0 on a compile error, -1 if hiprtc is unavailable / bad arguments. */
LIBXSMM_API int libxsmm_amd_csr_kernel_source(int typesize, int M, int K, const unsigned int* row_ptr, const unsigned int* column_idx,
  const double* values, int beta0, int vec, char* buffer, size_t buffer_size, int compile);

/** Text generator for dense SMM: the HIP source a descriptor (tight leading dimensions) is specialised to when a large
 *  batch is launched (one wavefront per item, shape baked in). Same buffer/compile/return conventions as
 *  libxsmm_amd_csr_kernel_source (reference counterpart: libxsmm_generator_gemm_kernel's "noarch" C text).
 *  variant: 0 = strided batch of 16-byte aligned items (widest loads); bit 0 = element-wide accesses (index and pointer
 *  batches); bit 1 = consecutive items with one C accumulate in registers (CP2K stacks, batch-reduce).
 *  compile == 2: as compile != 0, and `buffer` then holds the text the library actually builds for it -- a text with
 *  hand-counted waits (XHANDWAIT 1) whose code object has a private segment or spilled VGPRs is built with the compiler's
 *  waits instead (XHANDWAIT 0). */
LIBXSMM_API int libxsmm_amd_smm_kernel_source(const libxsmm_gemm_descriptor* descriptor, int variant, char* buffer, size_t buffer_size, int compile);

/** The text a grouped launch (libxsmm_amd_gemm_batch_groups) compiles for index batches of these descriptors: the run forms
 *  of every shape, each in a namespace of its own, behind one dispatching kernel. Conventions as above (compile == 2 included). */
LIBXSMM_API int libxsmm_amd_smm_grouped_kernel_source(const libxsmm_gemm_descriptor* const descriptors[], int ndescriptors, char* buffer, size_t buffer_size, int compile);

/** Run-time specialisation off the caller's path. A batch call never waits for the compiler (hiprtc: 0.3-0.5 s per kernel,
 *  seconds for a grouped kernel of many shapes): the kernel is built on a helper thread while the call -- and the following
 *  ones -- are served by the next best kernel (pre-compiled; the same results bit for bit), and loaded from the code-object
 *  cache on disk when a previous process (or libxsmm_amd_jit_prebuild) has left it there. LIBXSMM_AMD_JIT_ASYNC=0 compiles
 *  in the calling thread instead. libxsmm_amd_jit_wait blocks until the helper thread has nothing left to do (benchmarks:
 *  after the warm-up). libxsmm_amd_jit_prebuild compiles, without needing a device, the code objects batch calls with these
 *  descriptors may ask for (strided, index and pointer batches, shared C in batch order and relaxed; grouped != 0: also the
 *  fused kernel of libxsmm_amd_gemm_batch_groups over all of them) into the cache directory (LIBXSMM_AMD_CACHE, default
 *  jit_cache/ next to the library); returns the number of code objects now present, or -(number of failures). */
LIBXSMM_API void libxsmm_amd_jit_wait(void);
/** Drops the compile jobs that have not started and waits for the one that is running. A process must not reach exit() while
 *  the helper thread is inside the compiler: the compiler's static objects, first constructed during that very job, are
 *  destroyed ahead of any exit handler this library could have registered earlier. libxsmm_finalize() calls it (the
 *  reference's callers end with libxsmm_finalize), the Python binding calls it from Python's own atexit; an exit handler of
 *  the library remains as the last line of defence. */
LIBXSMM_API void libxsmm_amd_jit_drain(void);
LIBXSMM_API int libxsmm_amd_jit_prebuild(const libxsmm_gemm_descriptor* const descriptors[], int ndescriptors, int grouped);

/** Executable form of the sparse text kernels (libxsmm_generator_spgemm_{csr,csc}_kernel): the pattern is compiled into
 *  a kernel with hiprtc, the values of the sparse operand stay a run-time argument (as for the reference's generated C
 *  functions, samples/generator/validation.c). descriptor: lda == 0 marks A sparse, ldb == 0 marks B sparse; is_csr != 0:
 *  row_idx = row pointers, column_idx = column of each entry; is_csr == 0: column_idx = column pointers, row_idx = row of
 *  each entry. fma: 1 = fused multiply-add, 0 = multiply then add (the statement as written), < 0 = default
 *  (LIBXSMM_AMD_SPGEMM_FMA, fused). One launch processes `batch` products that share the sparse operand: the dense
 *  operand and C advance by stride_dense / stride_c elements per item. Operands may live on the host (staged). */
typedef struct libxsmm_amd_spgemm libxsmm_amd_spgemm;
LIBXSMM_API libxsmm_amd_spgemm* libxsmm_amd_spgemm_create(const libxsmm_gemm_descriptor* descriptor, int is_csr,
  const unsigned int* row_idx, const unsigned int* column_idx, int fma);
LIBXSMM_API int libxsmm_amd_spgemm_execute_batch(const libxsmm_amd_spgemm* handle, const void* sparse_values, const void* dense, void* c,
  long long stride_dense, long long stride_c, long long batch);
LIBXSMM_API void libxsmm_amd_spgemm_destroy(const libxsmm_amd_spgemm* handle);
/** The text libxsmm_amd_spgemm_create compiles (buffer/compile/return conventions of libxsmm_amd_csr_kernel_source). */
LIBXSMM_API int libxsmm_amd_spgemm_source(const libxsmm_gemm_descriptor* descriptor, int is_csr, const unsigned int* row_idx,
  const unsigned int* column_idx, int fma, char* buffer, size_t buffer_size, int compile);
/** The text behind libxsmm_create_{xcsr,xcsc,rm_ac,rm_bc}_soa as a translation unit (kernel "xsmm_spgemm_op"), same conventions.
 *  form: 0 = CSR (ptr = row pointers, idx = columns), 1 = CSC (ptr = column pointers, idx = rows), 2 = rm_ac, 3 = rm_bc (ptr, idx
 *  ignored). The kernels the library launches are fused multiply-add (fma != 0); fma == 0 yields the same statements as multiply,
 *  then add -- for checks of the text on another compiler. Returns -1 where libxsmm_create_*_soa would return no kernel. */
LIBXSMM_API int libxsmm_amd_soa_source(const libxsmm_gemm_descriptor* descriptor, int form, const unsigned int* ptr, const unsigned int* idx,
  int fma, char* buffer, size_t buffer_size, int compile);

/** The MatrixMarket coordinate reader that libxsmm_generator_spgemm uses for its input file (reference:
 *  libxsmm_sparse_csr_reader / libxsmm_sparse_csc_reader, src/generator_spgemm_csr_reader.c:46-170 and
 *  src/generator_spgemm_csc_reader.c:46-170 -- internal to the reference's generator library). '%' lines are comments,
 *  the first other line is "rows cols nnz", then 1-based "row col value" triples grouped by row (is_csr != 0) or by
 *  column (is_csr == 0); rows / columns without an entry are back-filled. *o_ptr receives rows + 1 (columns + 1) offsets,
 *  *o_idx the 0-based column (row) of every entry, *o_values the values as double; the three arrays are the caller's, to be
 *  released with free(). Returns 0, or the reference's error code (LIBXSMM_ERR_CSR_INPUT 90035, _READ_LEN 90036,
 *  _READ_DESC 90037, _READ_ELEMS 90038, _LEN 90039; CSC: 90011 ... 90015; see libxsmm_strerror) with nothing allocated. */
LIBXSMM_API int libxsmm_amd_sparse_reader(const char* path, int is_csr, unsigned int** o_ptr, unsigned int** o_idx, double** o_values,
  unsigned int* o_row_count, unsigned int* o_column_count, unsigned int* o_element_count);

/** SOA width v of the libxsmm_create_*_soa kernels for a precision (8 for fp64, 16 for fp32; 0 if unsupported). */
LIBXSMM_API int libxsmm_amd_soa_width(libxsmm_gemm_precision precision);
/** Batch form of a kernel made by libxsmm_create_{xcsr,xcsc,rm_ac,rm_bc}_soa: `batch` products that share the operator
 *  (the sparse values / the plain dense matrix). a, b, c as in the kernel call; the SOA input and C advance by
 *  stride_dense / stride_c elements per item. */
LIBXSMM_API int libxsmm_amd_kernel_execute_batch(const void* kernel, const void* a, const void* b, void* c,
  long long stride_dense, long long stride_c, long long batch);

/* ---- packed kernels (libxsmm_dispatch_pgemm / getrf / trmm / trsm, see libxsmm.h) ----------------------- */
/** Pack width VLEN of the packed kernels for an element size in bytes: 8 for 8 (fp64), 16 for 4 (fp32), 0 otherwise. */
LIBXSMM_API int libxsmm_amd_packed_width(unsigned int typesize);
/** `npacks` packs in one launch: pack p of an operand starts p * ld * lines * VLEN elements behind the first one, where
 *  lines is the number of columns (layout 102) or rows (layout 101) of the operand as it is stored (A of pgemm with
 *  transa 'T' is stored k x m, B with transb 'T' n x k; A of trmm / trsm has the order of the triangle) -- the operands
 *  of consecutive packs lie back to back, which is what a caller's loop `for each pack: kernel(Ap, Bp, Cp)` walks.
 *  a, b, c as in the kernel call (getrf: b is ignored; trmm / trsm: c is ignored). Device operands: asynchronous on the
 *  calling thread's stream; operands the CPU addresses are staged and complete on return. The results equal those of
 *  the per-pack calls bit for bit. Returns EXIT_SUCCESS/EXIT_FAILURE. */
LIBXSMM_API int libxsmm_amd_packed_execute_batch(const void* kernel, const void* a, const void* b, void* c, long long npacks);
/** The HIP text a packed descriptor is specialised to (kind: LIBXSMM_KERNEL_KIND_PGEMM / GETRF / TRMM / TRSM selects the
 *  descriptor type). Buffer/compile/return conventions of libxsmm_amd_csr_kernel_source. The form follows
 *  LIBXSMM_AMD_PACKED_FORM as a launch does (unset or 0: chosen by shape; 1: packs staged through LDS; 2: every lane
 *  works on its matrix in global memory). */
LIBXSMM_API int libxsmm_amd_packed_kernel_source(const void* descriptor, int kind, char* buffer, size_t buffer_size, int compile);

/* ---- stacks of small matrices: copy and transposition (libxsmm_matcopy / libxsmm_otrans, see libxsmm.h) ---------- */
/** `batch` items of m x n elements of typesize bytes (1 ... 255), one launch. Item g of the strided forms starts
 *  g * stride_in (stride_out) elements behind `in` (`out`); the pointer forms take one pointer per item, the arrays in host
 *  or in device memory, the items in memory the GPU reaches, aligned to the largest power of two (up to 16) that divides
 *  typesize. matcopy: out_g[j*ldo+i] = in_g[j*ldi+i], m <= ldi and m <= ldo, `in` == NULL zeroes the items; otrans:
 *  out_g[i*ldo+j] = in_g[j*ldi+i], m <= ldi and n <= ldo. The items of `out` must not overlap each other (strided forms:
 *  stride_out is checked against the extent of an item) or any item of `in`, with one exception: otrans with out == in
 *  (pointer form: the same array), equal strides, ldi == ldo and m == n transposes every item in place. What lies between the
 *  items, and between the columns of an item, keeps its bytes. Device operands: asynchronous on the calling thread's stream;
 *  strided operands in pageable host memory are staged and complete on return. batch == 0 (or m == 0, or n == 0) succeeds
 *  and does nothing; a negative batch, a leading dimension or stride that is too small, or a NULL operand fails before
 *  anything is written. Inside libxsmm_amd_defer_begin/end the calls are not recorded: they seal the open burst and run in
 *  call order. Returns EXIT_SUCCESS/EXIT_FAILURE. */
LIBXSMM_API int libxsmm_amd_matcopy_batch(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, long long stride_in, long long stride_out, long long batch);
LIBXSMM_API int libxsmm_amd_otrans_batch(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, long long stride_in, long long stride_out, long long batch);
LIBXSMM_API int libxsmm_amd_matcopy_batch_ptr(void* const out[], const void* const in[], unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo, long long batch);
LIBXSMM_API int libxsmm_amd_otrans_batch_ptr(void* const out[], const void* const in[], unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo, long long batch);

/* ---- tiled GEMM (libxsmm_gemm_handle_init / libxsmm_gemm_thread, see libxsmm.h) ----------------------------------- */
/** The rectangle of C that task `tid` of `nthreads` computes with libxsmm_gemm_thread: rect = {m0, m1, n0, n1}, rows
 *  m0 <= i < m1 and columns n0 <= j < n1. A task without work gets an empty rectangle (all zeros, m0 == m1). For every
 *  nthreads >= 1 the rectangles of tid = 0 ... nthreads - 1 are pairwise disjoint and cover C; they are cut on multiples of
 *  the kernel's work-group tile (libxsmm_amd_gemm_tile); k is never split. No device is needed. Returns EXIT_SUCCESS, or
 *  EXIT_FAILURE (rectangle empty) for a NULL handle, nthreads < 1 or tid outside [0, nthreads). */
LIBXSMM_API int libxsmm_amd_gemm_task(const libxsmm_gemm_handle* handle, int tid, int nthreads, unsigned int rect[4]);
/** Extent (rows and columns alike) of the work-group tile of the tiled GEMM kernel. */
LIBXSMM_API int libxsmm_amd_gemm_tile(void);

/* ---- GEMM with 16-bit inputs (libxsmm_wigemm / libxsmm_wsgemm / libxsmm_bsgemm, see libxsmm.h) ------------------------ */
/** C(m x n) = op(A) * op(B) + beta * C with (iprec, oprec) one of (I16, I32), (I16, F32), (BF16, F32) and beta 0 or 1. The
 *  layout is always plain column-major: op(A) is m x k, op(B) is k x n (transa / transb 'N' or 'T'), whatever the size --
 *  unlike the front ends, which below LIBXSMM_MAX_MNK read A in pairs of k. Per element of C, from C (beta 1) or from 0:
 *  I16 -> I32 the wrapping 32-bit sum of the 32-bit products; I16 -> F32 acc = acc + (float)(a * b), k ascending, every add
 *  rounded; BF16 -> F32 acc = acc + a * b, k ascending, the product and the add rounded separately -- the bits of the kernels
 *  of libxsmm_wimmdispatch / wsmmdispatch (scaling factor 1) / bsmmdispatch, -0.0 included. ONE DIVERGENCE: the BF16 kernel
 *  runs on the fp32 matrix instruction, which is acc = fma(a, b, acc): one rounding per step. The product of two bf16 numbers
 *  is exact in fp32 -- and the two chains are the same -- unless it is subnormal (below 2^-126) or beyond FLT_MAX; an element
 *  of C whose chain meets such a product has the bits of the fma chain, not of the separately rounded one (a subnormal
 *  product is not rounded before it is added; a product beyond FLT_MAX is not Inf before it is added, so Inf - Inf = NaN of
 *  the gold loop can come out as +-Inf or a finite number). The batch calls over a bf16 descriptor (bsmmdispatch /
 *  bmmdispatch kinds) do the same on their matrix-core form only (one wave per item, smm_bf16f32/bf16_mfma_wave_jit_lowp),
 *  which serves a batch when all of this holds: matrix cores on (libxsmm_amd_set_mfma), M > 31 or N > 31, K % 8 == 0 (bf16
 *  output: M % 8 == 0 as well), tight leading dimensions, at least LIBXSMM_AMD_JIT_MINBATCH items and, in a strided batch,
 *  operands and byte strides that are multiples of 16. Otherwise the same descriptor is served by a kernel that rounds
 *  product and sum separately: the bits of such elements change with these conditions.
 *  beta = 0 never reads C; what lies between m and ldc keeps its bytes. Operands in memory the GPU reaches are
 *  processed in place, asynchronously on the calling thread's stream; host-visible memory is complete on return; pageable
 *  memory is staged. Inside libxsmm_amd_defer_begin/end the call is not recorded: it seals the open burst and runs in call
 *  order. A wrong type pair, transa / transb other than N, n, T, t, a negative extent, a leading dimension below the
 *  extent, a NULL operand or another beta returns EXIT_FAILURE before any device is asked for; m, n or k of 0 succeeds and
 *  does nothing. The _thread form computes the rectangle of task tid of nthreads: the partition of libxsmm_amd_gemm_task
 *  over the tiles of libxsmm_amd_gemm_tile with k never split, so the results do not depend on nthreads; tid outside
 *  [0, nthreads) returns EXIT_FAILURE and does nothing. */
LIBXSMM_API int libxsmm_amd_lowp_gemm(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, char transa, char transb,
  libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k, const void* a, libxsmm_blasint lda, const void* b, libxsmm_blasint ldb,
  int beta, void* c, libxsmm_blasint ldc);
LIBXSMM_API int libxsmm_amd_lowp_gemm_thread(libxsmm_gemm_precision iprec, libxsmm_gemm_precision oprec, char transa, char transb,
  libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint k, const void* a, libxsmm_blasint lda, const void* b, libxsmm_blasint ldb,
  int beta, void* c, libxsmm_blasint ldc, int tid, int nthreads);
/** BF16 -> F32 on the bf16 matrix instruction (v_mfma_f32_32x32x16_bf16), opt-in (environment LIBXSMM_AMD_LOWP_FAST=1,
 *  default 0): per element the sum of the exact products in the order the instruction takes, 16 products per step. The
 *  result is the same from call to call and equals the default wherever every partial sum is exactly representable, but
 *  its bits are not those of the default in general; the last step is padded with zeros, so a C of -0.0 whose products are
 *  all -0.0 comes out as +0.0. The other type pairs are not affected. set returns the previous value. */
LIBXSMM_API int libxsmm_amd_set_lowp_fast(int on);
LIBXSMM_API int libxsmm_amd_get_lowp_fast(void);
/** The k chunk of the kernels behind libxsmm_amd_lowp_gemm for an input precision (BF16: 64, I16: 32; 0 otherwise). */
LIBXSMM_API int libxsmm_amd_lowp_gemm_chunk(libxsmm_gemm_precision iprec);

/* ---- quantisation (libxsmm_dnn_quantize / _act / _fil, see libxsmm_dnn.h) ------------------------------------------------ */
/** The reference forms without their wait: the same arguments and arithmetic, but `scf` points to one byte the GPU reaches
 *  (device, pinned or managed memory). The last kernel of the call writes it and the call returns without waiting for the
 *  calling thread's stream (libxsmm_amd_set_stream): a consumer queued on that stream sees the quantised tensor and the byte.
 *  in / out in host memory are still staged or waited for as in the reference forms. A wrong call (see libxsmm_dnn.h) or an
 *  scf the GPU does not reach returns EXIT_FAILURE and writes nothing; an empty tensor returns EXIT_SUCCESS, writes nothing
 *  and leaves *scf alone. Inside libxsmm_amd_defer_begin/end the calls are not recorded: they seal the open burst and run
 *  in call order. */
LIBXSMM_API int libxsmm_amd_dnn_quantize_async(float* in_buffer, short* out_buffer, int length, unsigned char add_shift, unsigned char* scf, int round_mode);
LIBXSMM_API int libxsmm_amd_dnn_quantize_act_async(float* in_buffer, short* out_buffer, unsigned int N, unsigned int C, unsigned int H, unsigned int W,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode);
LIBXSMM_API int libxsmm_amd_dnn_quantize_fil_async(float* in_buffer, short* out_buffer, unsigned int K, unsigned int C, unsigned int R, unsigned int S,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int kblk_f32, unsigned int kblk_i16, unsigned int lp_blk, unsigned char add_shift,
  unsigned char* scf, int round_mode);
/** LIBXSMM_DNN_QUANT_STOCH_ROUND draws p of element i from a counter-based generator of (seed, i), i being the element's
 *  index in the output. seed == 0 (the default): every call takes a seed from libxsmm_timer_tick(), as the reference seeds
 *  rand(); any other value makes a call a pure function of its inputs. Process-wide. */
LIBXSMM_API void libxsmm_amd_dnn_quantize_set_seed(unsigned int seed);

/* ---- matdiff on operands in device memory (libxsmm_matdiff, see libxsmm.h) ------------------------------------------------- */
/** libxsmm_matdiff runs on the GPU whenever ref or tst is plain device memory (the other operand may be any memory; pageable
 *  memory is staged), waits and fills the caller's struct. Two host operands take the host loop as before. The device path
 *  follows the reference's definition: all five datatypes (F64, F32, I32, I16, I8), m <= ld required, the
 *  contiguous sums in normi_abs and the strided ones in norm1_abs. A non-finite test value gives its first location in m, n,
 *  +inf in norm1_abs, norm1_rel, normi_abs, normi_rel, normf_rel, linf_abs, linf_rel, l2_abs and l2_rel, and leaves the other
 *  fields as libxsmm_matdiff_clear sets them. The same call on the same data returns the same bytes.
 *
 *  libxsmm_amd_matdiff_async is the same call without its wait: `info` lies in memory the GPU reaches (device, pinned or
 *  managed), the last kernel of the call writes it, and the call returns without waiting for the calling thread's stream
 *  (libxsmm_amd_set_stream): a consumer queued on that stream sees it. A wrong call (NULL info, no operand, m > ld, a negative
 *  size, another datatype, an info the GPU does not reach) returns EXIT_FAILURE at once and writes nothing; m == 0 or n == 0
 *  writes a cleared info and launches nothing. A lone operand (ref == NULL and tst given, or the other way round) is walked by
 *  ldref, as the reference does. Inside libxsmm_amd_defer_begin/end the calls are not recorded: they seal the open burst
 *  and run in call order, so they see the results of the calls recorded before them. */
LIBXSMM_API int libxsmm_amd_matdiff_async(libxsmm_matdiff_info* info, libxsmm_datatype datatype, libxsmm_blasint m, libxsmm_blasint n,
  const void* ref, const void* tst, const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst);
/** `batch` pairs of m x n matrices, item i at ref + i * stride_ref and tst + i * stride_tst (strides in elements, not
 *  negative; a lone operand goes by ldref and stride_ref), compared by one set of launches. `items` is NULL or an array of
 *  `batch` infos in host or device memory: entry i is what a single call on item i gives. `info` is the combination of all
 *  items as libxsmm_matdiff_reduce of the reference forms it from a cleared info (src/libxsmm_math.c:182-238): every field on
 *  its own, the larger of the maxima and norms, the smaller of the minima, l1_ref and l1_tst summed; m, n are those of the
 *  first item with the largest linf_abs, whose index goes to *item (item may be NULL; -1 if nothing differs). One deviation:
 *  avg_ref and avg_tst are l1 / (m * n * batch), the mean over the batch -- the running half-sum of the reduce depends on the
 *  order of the items and forgets all but the last ones. A non-finite test value in any item gives `info` the nine +inf and
 *  the cleared fields of the single call, with m, n and *item of the first such item. batch == 0 is an empty comparison
 *  (cleared info, *item = -1), batch < 0 a wrong call. The call waits if info (or items, or item) is plain host memory;
 *  otherwise it returns without waiting, like libxsmm_amd_matdiff_async. */
LIBXSMM_API int libxsmm_amd_matdiff_batch(libxsmm_matdiff_info* info, libxsmm_matdiff_info* items, long long* item, libxsmm_datatype datatype,
  libxsmm_blasint m, libxsmm_blasint n, const void* ref, const void* tst, const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst,
  long long stride_ref, long long stride_tst, long long batch);

/* ---- hash and byte compare on operands in device memory (libxsmm_hash, libxsmm_memcmp, libxsmm_diff, libxsmm_diff_n) ---------- */
/** The reference's four functions (libxsmm.h) run on the GPU whenever an operand is plain device memory. These are the forms
 *  that do not wait, and the batches. All return EXIT_SUCCESS or EXIT_FAILURE; all arguments are checked before
 *  any device is probed and a refused call writes nothing: a NULL result, a NULL operand of a call that has bytes to read, a
 *  negative count or stride, ld < line_bytes with lines > 1, and, for the _async forms, a result the GPU does not reach. An
 *  item is `lines` lines of `line_bytes` bytes, `ld` bytes apart, hashed or compared as the concatenation of its lines; the
 *  bytes between line_bytes and ld are never read. Item i lies `i * stride` bytes after the first; stride == 0 is legal.
 *  batch == 0 writes nothing; an empty item gives `seed` (0 for the compares) and launches nothing. Inside
 *  libxsmm_amd_defer_begin/end these calls are not recorded: they seal the open burst and run in call order.
 *
 *  libxsmm_amd_hash_async: libxsmm_hash(data, size, seed) for any size_t size into `*result`, memory the GPU reaches (device,
 *  pinned or managed); the last kernel writes it and nobody waits. */
LIBXSMM_API int libxsmm_amd_hash_async(unsigned int* result, const void* data, size_t size, unsigned int seed);
/** One hash per item into results[0 .. batch). `results` in plain host memory is complete on return; memory the GPU reaches
 *  is written in stream order and nobody waits. */
LIBXSMM_API int libxsmm_amd_hash_batch(unsigned int* results, const void* data, size_t line_bytes, long long lines, long long ld,
  long long stride, long long batch, unsigned int seed);
/** libxsmm_memcmp(a, b, size) into `*result` (0 or 1), memory the GPU reaches; nobody waits. */
LIBXSMM_API int libxsmm_amd_memcmp_async(int* result, const void* a, const void* b, size_t size);
/** 0 or 1 per item into results[0 .. batch). `first_diff` is NULL or receives the lowest index of a differing item, -1 if all
 *  are equal. Either may be host or device memory, as for libxsmm_amd_hash_batch. */
LIBXSMM_API int libxsmm_amd_memcmp_batch(int* results, long long* first_diff, const void* a, const void* b, size_t line_bytes,
  long long lines, long long lda, long long ldb, long long stride_a, long long stride_b, long long batch);

/* ---- DNN tensor copy-in / copy-out (libxsmm_dnn_copyin_tensor / _copyout_tensor, see libxsmm_dnn_tensor.h) ------------------- */
#include "libxsmm_dnn_tensor.h"
/** The reference forms without their wait: the same checks in the same order and the same statuses, then both `tensor`'s
 *  data and `data` must be memory the GPU reaches (device, pinned or managed); otherwise, or without a device, the call
 *  returns LIBXSMM_DNN_ERR_GENERAL and writes nothing. Nothing is staged: one kernel is queued on the calling thread's
 *  stream (libxsmm_amd_set_stream) and the call returns without waiting for it, so a consumer queued on that stream sees
 *  the result. An empty tensor returns LIBXSMM_DNN_SUCCESS and launches nothing. Inside libxsmm_amd_defer_begin/end the
 *  calls are not recorded: they seal the open burst and run in call order. Operands that overlap are undefined. */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copyin_tensor_async(const libxsmm_dnn_tensor* tensor, const void* data, libxsmm_dnn_tensor_format in_format);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copyout_tensor_async(const libxsmm_dnn_tensor* tensor, void* data, libxsmm_dnn_tensor_format out_format);
/** The launch geometry of a copy between `layout` and `plain_format` (in != 0: copy-in), without a device: the status the copy
 *  would give for that layout and format, and on LIBXSMM_DNN_SUCCESS
 *    plan[0]  form: 0 the same order on both sides (channel tensors; activations of one pixel), 1 activation, 2 filter
 *    plan[1]  bytes per element
 *    plan[2]  independent blocks
 *    plan[3]  rows per block on the plain side
 *    plan[4]  contiguous run per row, in elements
 *    plan[5]  rows of a block held in LDS per pass (fewer than plan[3] where a block is cut; 0: the copy does not go through LDS)
 *    plan[6]  work items (tiles; 16-byte units of form 0; work-groups' worth of elements where plan[5] is 0 otherwise)
 *    plan[7]  work-groups launched
 *  The launcher takes its geometry from the same function. */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_amd_dnn_copy_plan(const libxsmm_dnn_tensor_datalayout* layout, libxsmm_dnn_tensor_format plain_format, int in, long long plan[8]);

#endif /* LIBXSMM_AMD_H */
