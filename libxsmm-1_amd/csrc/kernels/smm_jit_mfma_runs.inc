// smm_jit_mfma_runs.inc -- the kernels of the run and streaming forms on the matrix cores (the reasoning: smm_jit_mfma_runs_const.inc,
// which stands in front together with smm_jit_chain.inc): fragment loads, the software pipeline with its hand-counted waits (XHANDWAIT)
// fragment of A for k step ks, tile mi (rows beyond M repeat row M - 1: they only reach rows of C that are never stored)
__device__ __forceinline__ T load_a_frag(const T* pa, int ks, int moff, int lq, int k0 = 0)
{ // (k0: first k of the chunk, a constant after unrolling)
  const int k = k0 + 4 * ks + lq;
  const XGLOBAL T* const g = (const XGLOBAL T*)pa;
  if (k0 + 4 * ks + 3 < K) return __builtin_nontemporal_load(g + k * LDA + moff);
  const T v = __builtin_nontemporal_load(g + clampi(k, K - 1) * LDA + moff); // (no divergent control flow around the load)
  return (k < K) ? v : -T(0);
}
__device__ __forceinline__ void load_b_flat(const T* pb, int lane, T (&rb)[NLB])
{
  const XGLOBAL T* const g = (const XGLOBAL T*)pb;
#pragma unroll
  for (int j = 0; j < NLB; ++j) rb[j] = __builtin_nontemporal_load(g + clampi(64 * j + lane, BE - 1));
}
__device__ __forceinline__ void park_b(T* Bs, int lane, const T (&rb)[NLB])
{
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
    const int e = 64 * j + lane, n = e / LDB, k = e - n * LDB;
    if (e < BE && k < K) Bs[n * KSD + k] = rb[j];
  }
}
// chunk c of B (several chunks: K > 64): the KC x N window, lanes along k -- runs of KC elements of a column; k beyond K: +0
__device__ __forceinline__ void load_b_chunk(const T* pb, int c, int lane, T (&rb)[NLB])
{
  const XGLOBAL T* const g = (const XGLOBAL T*)pb;
  asm volatile("" : "+v"(lane)); // (the places are recomputed per chunk: hoisted out of the loop over the items they cost a register each)
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
    const int e = 64 * j + lane, n = e / KC, kk = e - n * KC, k = c * KC + kk;
    const T v = __builtin_nontemporal_load(g + clampi(n, N - 1) * LDB + clampi(k, K - 1)); // (no control flow around the load)
    rb[j] = (k < K) ? v : T(0);
  }
}
__device__ __forceinline__ void park_b_chunk(T* Bs, int lane, const T (&rb)[NLB])
{
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
    const int e = 64 * j + lane, n = e / KC, kk = e - n * KC;
    if (e < N * KC) Bs[n * KSD + kk] = rb[j];
  }
}
__device__ __forceinline__ void acc_load(const T* pc, int l16, int lq, ACC (&acc)[NI][MI])
{
  const XGLOBAL T* const g = (const XGLOBAL T*)pc;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * ni + XNROW(r), m = 16 * mi + l16;
        acc[ni][mi][r] = g[clampi(n, N - 1) * LDC + clampi(m, M - 1)];
      }
}
__device__ __forceinline__ void acc_store(T* pc, int l16, int lq, const ACC (&acc)[NI][MI], bool atomic)
{
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * ni + XNROW(r), m = 16 * mi + l16;
        if (n < N && m < M) {
          if (atomic) xatomic_add(pc + n * LDC + m, acc[ni][mi][r]);
          else ((XGLOBAL T*)pc)[n * LDC + m] = acc[ni][mi][r];
        }
      }
}

#if XHANDWAIT
// The compiler's own wait counts are useless for the software pipeline of the run form: in front of the first matrix instruction
// of a product it waits for ALL of the product's A fragments (vmcnt(#B loads just issued)) -- the ones requested at the very end of
// the previous product included: a memory round trip per product, 1.8 us for a 32^3 fp64 product whose matrix instructions take 0.9.
// The loads whose results live across iterations are therefore issued as inline assembly -- invisible to the compiler's
// scoreboard -- and waited for by hand: vmcnt retires in the order of issue, and the number of loads issued after the ones a step
// needs is a constant of the pipeline (below). Loads the compiler does see (C at a run head, address windows) are drained inside
// their branch, so that nothing pending escapes into the loop.
__device__ __forceinline__ T xload_nt(const XGLOBAL T* p, int off)
{ // off: bytes, a constant below 4096 after unrolling (the instruction's immediate: one address register pair serves a 4 KiB window)
  T v;
  if constexpr (F64) asm volatile("global_load_dwordx2 %0, %1, off offset:%2 nt" : "=v"(v) : "v"(p), "n"(off));
  else asm volatile("global_load_dword %0, %1, off offset:%2 nt" : "=v"(v) : "v"(p), "n"(off));
  return v;
}
// B's flat span, 64 elements per load; the last load of a span that does not end on 64 elements repeats the span's last element
__device__ __forceinline__ void xload_b(const T* pb, int lane, T (&rb)[NLB])
{
  const XGLOBAL T* const b0 = (const XGLOBAL T*)pb + lane;
#pragma unroll
  for (int jj = 0; jj < NLB; ++jj) {
    const int byte = jj * 64 * TS;
    if (64 * jj + 63 < BE) rb[jj] = xload_nt(b0 + (byte / 4096) * (4096 / TS), byte % 4096);
    else rb[jj] = xload_nt((const XGLOBAL T*)pb + clampi(64 * jj + lane, BE - 1), 0);
  }
}
// A's fragments of k step ks (rows beyond M repeat row M - 1, k beyond K repeats k = K - 1: replaced by -0 when used)
__device__ __forceinline__ void xload_a(const T* pa, int ks, const int (&moff)[MI], int lq, T (&af)[MI])
{
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int byte = 4 * ks * LDA * TS;
    if (4 * ks + 3 < K) af[mi] = xload_nt((const XGLOBAL T*)pa + lq * LDA + moff[mi] + (byte / 4096) * (4096 / TS), byte % 4096);
    else af[mi] = xload_nt((const XGLOBAL T*)pa + clampi(4 * ks + lq, K - 1) * LDA + moff[mi], 0);
  }
}
constexpr int vmc(int n) { return n < 63 ? n : 63; } // (the counter has six bits; fewer is stricter, never wrong)
template<int CNT> __device__ __forceinline__ void wait_on(T& a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(CNT)); }
template<int CNT> __device__ __forceinline__ void wait_on(T& a, T& b) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(CNT)); }
#endif

#if XSTREAM
// Every item owns its C (strided batches; index / pointer batches under the caller's promise): a wave per item, walking the batch with
// a stride of all resident waves. The next item's operands -- B's flat array, C in the layout of the accumulators, A's fragments
// behind the instructions that free their registers -- are in flight during this item's arithmetic; the stores of an item are
// issued behind the loads of the next (older loads: the wait for them is not a wait for the stores).
extern "C" __global__ __launch_bounds__(64 * XWAVES) void xsmm_smm_op(DevAddr ad, long long batch)
{
  __shared__ __attribute__((aligned(16))) T lds[XWAVES * WAVE_LDS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, l16 = lane & 15, lq = lane >> 4;
  T* const Bs = lds + wave * WAVE_LDS;
  const long long w = (long long)blockIdx.x * XWAVES + wave, W = (long long)gridDim.x * XWAVES;
  if (w >= batch) return;
  if (1 == NCH && KP4 > K) { // the padding of B's image (+0): written once, never parked over (several chunks: the loads deliver it)
    for (int e = lane; e < N * (KP4 - K); e += 64) Bs[(e / (KP4 - K)) * KSD + K + e % (KP4 - K)] = T(0);
  }
  int moff[MI], boff[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) moff[mi] = clampi(16 * mi + l16, M - 1);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) boff[ni] = clampi(16 * ni + l16, N - 1) * KSD + lq;
  T af[KS][MI], rb[NLB];
  ACC cn[NI][MI];
  T* pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, w);
  const T* pa_cur = resolve<const T>(ad.a, ad.ia, ad.sa, ad, w);
  const T* pb_cur = resolve<const T>(ad.b, ad.ib, ad.sb, ad, w);
  if (1 == NCH) load_b_flat(pb_cur, lane, rb); else load_b_chunk(pb_cur, 0, lane, rb);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) af[ks][mi] = load_a_frag(pa_cur, ks, moff[mi], lq);
  if (!XBETA0) acc_load(pc, l16, lq, cn);
  for (long long item = w; item < batch; item += W) {
    T* const pc_cur = pc;
    ACC acc[NI][MI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = XBETA0 ? ACC{ 0, 0, 0, 0 } : cn[ni][mi];
    // (no control flow around the loads: the last item of a wave fetches its own operands once more, never used)
    const long long next = (item + W < batch) ? (item + W) : item;
    const T* const pa_next = resolve<const T>(ad.a, ad.ia, ad.sa, ad, next);
    const T* const pb_next = resolve<const T>(ad.b, ad.ib, ad.sb, ad, next);
#pragma unroll
    for (int c = 0; c < NCH; ++c) { // (unrolled: which chunk comes next, and where K ends, are constants)
      if (1 == NCH) park_b(Bs, lane, rb); else park_b_chunk(Bs, lane, rb);
      const bool last = (c + 1 == NCH);
      const T* const pan = last ? pa_next : pa_cur;
      const int cnext = last ? 0 : c + 1;
      if (1 == NCH) load_b_flat(pb_next, lane, rb); else load_b_chunk(last ? pb_next : pb_cur, cnext, lane, rb);
      if (last) {
        pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, next);
        if (!XBETA0) acc_load(pc, l16, lq, cn);
      }
      wave_lds_sync();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        T bf[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) bf[ni] = Bs[boff[ni] + 4 * ks];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = xmfma(bf[ni], af[ks][mi], acc[ni][mi]);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[ks][mi] = load_a_frag(pan, ks, moff[mi], lq, cnext * KC);
      }
      wave_lds_sync(); // (B's image is parked over next)
    }
    pa_cur = pa_next; pb_cur = pb_next;
    acc_store(pc_cur, l16, lq, acc, false);
  }
}
#else
#if XGROUPED
__device__ XENTRY_ATTR void xsmm_entry(const DevAddr& ad, long long batch, unsigned xbid, unsigned xgrid, T* lds)
{
#if !XTILEWG
  if ((int)(threadIdx.x >> 6) >= XWAVES) return; // (the grouped kernel's work-groups may have more waves than this body uses)
#endif
#else
extern "C" __global__ __launch_bounds__(64 * XWAVES) void xsmm_smm_op(DevAddr ad, long long batch)
{
  __shared__ __attribute__((aligned(16))) T lds[XWAVES * WAVE_LDS];
  const unsigned xbid = blockIdx.x, xgrid = gridDim.x;
#endif
  // (XTILEWG: the waves of a work-group are the tiles of C of ONE walk -- each wave is the only wave of its body, lds is its own)
  const int wave = XTILEWG ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, l16 = lane & 15, lq = lane >> 4;
  T* const Bs = lds + wave * WAVE_LDS;
  const long long w = (long long)xbid * XWAVES + wave, W = (long long)xgrid * XWAVES;
  // (walking the batch: chunks of 64 items, run heads, segments -- see the register-tiled wave form)
  const int seg = segment_len(ad.flags, batch);
  const long long step = (0 != seg ? seg : 64);
  const long long nchunks = (batch + step - 1) / step, cpw = (nchunks + W - 1) / W;
  const long long c_end = ((w + 1) * cpw < nchunks) ? (w + 1) * cpw : nchunks;
  if (w * cpw >= c_end) return;
  if (KP4 > K) { // the padding of B's image (+0): written once, never parked over
    for (int e = lane; e < N * (KP4 - K); e += 64) Bs[(e / (KP4 - K)) * KSD + K + e % (KP4 - K)] = T(0);
  }
  int moff[MI], boff[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) moff[mi] = clampi(16 * mi + l16, M - 1);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) boff[ni] = clampi(16 * ni + l16, N - 1) * KSD + lq; // (columns beyond N repeat column N - 1: never stored)
  for (long long ci = w * cpw; ci < c_end; ++ci) {
    const long long chunk = ci * step;
    unsigned long long heads; long long first, end;
    if (0 != seg) { // a segment is walked from its first item, whoever opened the run it starts in
      heads = head_mask(ad, chunk, lane, batch) | 1ULL;
      first = chunk; end = (chunk + seg < batch ? chunk + seg : batch);
    }
    else if (!chain_of_chunk(ad, chunk, lane, batch, heads, first, end)) continue;
    AddrWindow win; window_fill(win, ad, first, lane, end);
    // D products in flight (register sets; the walk is unrolled over them so that every index is a constant): a light product's
    // arithmetic is over in a tenth of a microsecond -- one product ahead, a run of 13^3 products is a chain of memory round trips
    T af[D][KS][MI], rb[D][NLB];
#if XHANDWAIT
    constexpr int LSET = NLB + KS * MI;                                   // loads per product
    constexpr int CNT_B = vmc(KS * MI + (D - 1) * LSET);                  // issued after a product's B when it is parked
    constexpr int CNT_A = vmc((KS - 1) * MI + NLB + (D - 1) * LSET);      // issued after the fragments of k step ks when they are used (any ks)
#endif
#pragma unroll
    for (int s = 0; s < D; ++s) {
      const long long j = (first + s < end) ? (first + s) : (end - 1);
      WINDOW_AB(win, j, pa0, pb0);
#if XHANDWAIT
      xload_b(pb0, lane, rb[s]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xload_a(pa0, ks, moff, lq, af[s][ks]);
#else
      load_b_flat(pb0, lane, rb[s]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[s][ks][mi] = load_a_frag(pa0, ks, moff[mi], lq);
#endif
    }
    ACC acc[NI][MI];
    T* pc = nullptr;
    for (long long i0 = first; i0 < end; i0 += D) {
#pragma unroll
      for (int s = 0; s < D; ++s) {
        const long long i = i0 + s;
        if (i >= end) break;
        if (is_head(heads, chunk, i)) { // item i opens a run: close the previous one, take over its C
          if (nullptr != pc) acc_store(pc, l16, lq, acc, 0 != seg);
          pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, i);
          if (XBETA0 || 0 != seg) {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
              for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = ACC{ 0, 0, 0, 0 };
          }
          else {
            acc_load(pc, l16, lq, acc);
#if XHANDWAIT
            // (C has arrived before the branch ends: a load left pending here would make the compiler wait for everything in
            // front of the first matrix instruction of EVERY product, head or not)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
              for (int mi = 0; mi < MI; ++mi) asm volatile("" : "+v"(acc[ni][mi]));
#endif
          }
        }
#if XHANDWAIT
#pragma unroll
        for (int jj = 0; jj + 1 < NLB; jj += 2) wait_on<CNT_B>(rb[s][jj], rb[s][jj + 1]);
        if (NLB & 1) wait_on<CNT_B>(rb[s][NLB - 1]);
#endif
        park_b(Bs, lane, rb[s]);
        // The operands of the product D ahead take this set's place: B right away, A behind the instructions that free its
        // registers. No control flow around the loads -- the last D products of a walk fetch the last one's operands again (never
        // used): with conditional loads the compiler loses count of what is in flight and waits for everything, the operands just
        // requested included, in front of the first matrix instruction (one memory round trip per product: 1.4 instead of 0.8 us
        // for 13^3).
        const long long inext = (i + D < end) ? (i + D) : (end - 1);
        WINDOW_AB(win, inext, pa1, pb1);
#if XHANDWAIT
        xload_b(pb1, lane, rb[s]);
#else
        load_b_flat(pb1, lane, rb[s]);
#endif
        wave_lds_sync();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          T bf[NI];
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) bf[ni] = Bs[boff[ni] + 4 * ks];
#if XHANDWAIT
          if (1 == MI) wait_on<CNT_A>(af[s][ks][0]); else wait_on<CNT_A>(af[s][ks][0], af[s][ks][MI - 1]);
          T av[MI];
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) av[mi] = (4 * ks + 3 < K || 4 * ks + lq < K) ? af[s][ks][mi] : -T(0); // (K padded to four: A = -0)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = xmfma(bf[ni], av[mi], acc[ni][mi]);
          xload_a(pa1, ks, moff, lq, af[s][ks]);
#else
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = xmfma(bf[ni], af[s][ks][mi], acc[ni][mi]);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) af[s][ks][mi] = load_a_frag(pa1, ks, moff[mi], lq);
#endif
        }
        wave_lds_sync(); // (B's image is parked over next)
      }
    }
    acc_store(pc, l16, lq, acc, 0 != seg);
  }
}
#endif
