// smm_jit_chain.inc -- walking a batch run by run: run heads, the chunk a wave or work-group is dealt, segments of long runs, and the
// address windows of index and pointer batches. Shared by the register-tiled run forms (behind smm_jit_shape.inc) and the matrix-core
// run form (behind smm_jit_mfma_runs_const.inc): needs T, DevAddr / resolve, XRUNS, XSPLIT, XDEPTH.
// bit l: item first + l starts a run, i.e. its C differs from its predecessor's (item 0 always does)
__device__ __forceinline__ unsigned long long head_mask(const DevAddr& ad, long long first, int lane, long long batch)
{
  const long long j = first + lane;
  bool head = false;
  if (j < batch) head = (0 == j) || (resolve<T>(ad.c, ad.ic, ad.sc, ad, j - 1) != resolve<T>(ad.c, ad.ic, ad.sc, ad, j));
  return __ballot(head);
}

// Items [first, end) a wave / work-group walks when it is dealt the chunk [chunk, chunk + 64): from the chunk's first run
// head through the chunk's other runs to the end of the run that is still open at the chunk's end (the next head at or
// beyond chunk + 64). Returns false if the chunk holds no head (an earlier chunk's walk covers it).
__device__ __forceinline__ bool chain_of_chunk(const DevAddr& ad, long long chunk, int lane, long long batch,
                                               unsigned long long& heads, long long& first, long long& end)
{
  heads = head_mask(ad, chunk, lane, batch);
  if (0 == heads) return false;
  first = chunk + (__ffsll((long long)heads) - 1);
  end = chunk + 64;
  while (end < batch) {
    const unsigned long long mk = head_mask(ad, end, lane, batch);
    if (0 != mk) { end += (__ffsll((long long)mk) - 1); break; }
    end += 64;
  }
  if (end > batch) end = batch;
  return true;
}
__device__ __forceinline__ bool is_head(unsigned long long heads, long long chunk, long long i)
{ // beyond the chunk the walk only continues through non-heads
  return (i < chunk + 64) && (0 != ((heads >> (int)(i - chunk)) & 1ULL));
}

#if XRUNS
// When a batch is not walked run by run. (1) C blocks repeat out of order: no walk in batch order can keep them apart.
// (2) XSPLIT -- relaxed order, the caller's reference path is itself multi-threaded with a lock per C
// (libxsmm_gemm_batch_omp, mmbatch with several tasks) -- and the batch is a handful of long runs, i.e. of sequential
// chains that leave the chip idle. Such a batch is cut into segments of `len` items; a wave sums the products of a run
// inside its segment from zero and adds the sum to C with floating-point atomics (one C-sized atomic update per segment
// instead of a C read and write per run). Returns 0 when the batch is walked run by run, in batch order.
__device__ __forceinline__ int segment_len(const int* flags, long long batch)
{
  if (nullptr == flags) return 0;
  const long long peers = (0 < flags[3]) ? flags[3] : 1; // batches that run beside this one in the same (grouped) launch, about as large
  if (0 == flags[1]) {
    const long long runs = batch - flags[0];
    // (the runs of all batches of the launch fill the chip together: 27 CP2K groups of 172 runs each are 4644 chains, and walked in
    // batch order -- no C-sized atomic update per segment -- they are the faster form: 0.81 against 1.02 ms, profiles/r3_cp2k_stacks.txt)
    if (!XSPLIT || runs * peers >= 2048 || 16 * runs > batch) return 0;
  }
  const long long len = (batch * peers + 4095) / 4096;
  return (int)(len < 8 ? 8 : (len > 64 ? 64 : len));
}
#endif

constexpr int D = XDEPTH; // products whose operands are in flight (register stages)

// Operand addresses of 64 consecutive items, one item per lane. Index and pointer batches need a load per item and operand
// before the operand itself can be requested; done item by item that load is a full memory round trip on the critical
// path of a run. Here 64 of them travel together and single addresses are picked with v_readlane.
struct AddrWindow { long long base; unsigned long long a, b; };
__device__ __forceinline__ void window_fill(AddrWindow& w, const DevAddr& ad, long long base, int lane, long long end)
{
  const long long j = base + lane;
  w.base = base;
  w.a = (j < end) ? (unsigned long long)resolve<const T>(ad.a, ad.ia, ad.sa, ad, j) : 0ULL;
  w.b = (j < end) ? (unsigned long long)resolve<const T>(ad.b, ad.ib, ad.sb, ad, j) : 0ULL;
  // The addresses may be load results (pointer batches). Settle that here, once per 64 items: otherwise the compiler must
  // assume a pending load at every later v_readlane and drains vmcnt -- the prefetched operands -- before each item.
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(w.a), "+v"(w.b));
}
__device__ __forceinline__ const T* window_pick(unsigned long long v, int src)
{
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, src), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), src);
  return (const T*)(((unsigned long long)hi << 32) | lo);
}
// addresses of item i (i never decreases between calls; the window slides forward in steps that keep i inside)
#define WINDOW_AB(W, I, PA, PB) \
  if ((I) - (W).base >= 64) window_fill((W), ad, (I), lane, end); \
  const int w_src_ = __builtin_amdgcn_readfirstlane((int)((I) - (W).base)); \
  const T* const PA = window_pick((W).a, w_src_); const T* const PB = window_pick((W).b, w_src_)

