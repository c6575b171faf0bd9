// smm_jit_shape_kernels.inc -- the kernels of the register-tiled forms (behind smm_jit_shape.inc and smm_jit_chain.inc): the
// work-group run form (XRUNS 2), else the wave forms -- runs (XRUNS 1) and streaming (XRUNS 0); XGROUPED: an entry function a
// dispatcher calls instead of a kernel.
// Work-group form for long runs (CP2K stacks, batch-reduce): the four waves of a work-group share every product of a run.
// All 256 threads stream A and B of the products D ahead into register stages while the current one is multiplied out of
// LDS (two operand buffers when 64 KiB allow: one barrier per product); wave v owns columns [v*NQ, v*NQ + NQ) of C and
// keeps them in registers for the whole run, each element still receiving its products in batch order, k ascending --
// the sequential reference's chain. A long run is a latency chain (HBM round trip per product): the depth of the register
// ring, not the thread count, is what shortens it.
#if (2 == XRUNS)
#if XGROUPED
__device__ XENTRY_ATTR void xsmm_entry(const DevAddr& ad, long long batch, unsigned xbid, unsigned xgrid, T* lds)
{
#else
extern "C" __global__ __launch_bounds__(256) void xsmm_smm_op(DevAddr ad, long long batch)
{
  __shared__ __attribute__((aligned(16))) T lds[WG_NBUF * WG_BUF];
  const unsigned xbid = blockIdx.x, xgrid = gridDim.x;
#endif
  const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int tx = lane & (TGM - 1), ty = lane >> 4;
  const int ncol0 = wave * NQ + ty * TN;
  if (nullptr != ad.flags) {
    if (8LL * ad.flags[0] < 7LL * batch) return;                     // runs shorter than 8 on average: the wave form owns it
    if (0 != segment_len(ad.flags, batch)) return;                   // not walked run by run: the wave form cuts it into segments
  }
  T ra[D][NLA][VA], rb[D][NLB][VB];
  int buf = 0;
  // every work-group takes a contiguous range of chunks (dealt round-robin, runs of a uniform length of 128, 256, ... items
  // would put all run heads into the chunks of every 2nd, 4th, ... work-group)
  const long long nchunks = (batch + 63) / 64, cpw = (nchunks + xgrid - 1) / xgrid;
  const long long c_end = ((long long)(xbid + 1) * cpw < nchunks) ? (long long)(xbid + 1) * cpw : nchunks;
  for (long long ci = (long long)xbid * cpw; ci < c_end; ++ci) {
    const long long chunk = ci * 64;
    unsigned long long heads; long long first, end;
    if (!chain_of_chunk(ad, chunk, lane, batch, heads, first, end)) continue; // identical in the four waves
    AddrWindow win; window_fill(win, ad, first, lane, end);
#pragma unroll
    for (int s = 0; s < D; ++s) {
      if (first + s < end) {
        WINDOW_AB(win, first + s, pa, pb);
        load_flat<VA, NLA, AE>(pa, t, ra[s]);
        load_flat<VB, NLB, BE>(pb, t, rb[s]);
      }
    }
    T acc[TM][TN];
    T* pc = nullptr;
    for (long long i0 = first; i0 < end; i0 += D) {
#pragma unroll
      for (int s = 0; s < D; ++s) {
        const long long i = i0 + s;
        if (i < end) {
          if (is_head(heads, chunk, i)) { // item i opens a run: C goes straight between HBM and registers
            if (nullptr != pc) {
#pragma unroll
              for (int ii = 0; ii < TM; ++ii) {
#pragma unroll
                for (int j = 0; j < TN; ++j) { const int m = tx * TM + ii, n = ncol0 + j; if (m < M && ty * TN + j < NQ && n < N) ((XGLOBAL T*)pc)[n * LDC + m] = acc[ii][j]; }
              }
            }
            pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, i);
#pragma unroll
            for (int ii = 0; ii < TM; ++ii) {
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                const int m = tx * TM + ii, n = ncol0 + j;
                acc[ii][j] = (!XBETA0 && m < M && ty * TN + j < NQ && n < N) ? ((const XGLOBAL T*)pc)[n * LDC + m] : (T)0;
              }
            }
          }
          T* const As = lds + buf * WG_BUF;
          T* const Bs = As + AS_SIZE;
          if (1 == WG_NBUF) lds_barrier(); // single buffer: the previous product's readers must be done
          park_ab(As, Bs, t, ra[s], rb[s]);
          if (i + D < end) {
            WINDOW_AB(win, i + D, pa, pb);
            load_flat<VA, NLA, AE>(pa, t, ra[s]);
            load_flat<VB, NLB, BE>(pb, t, rb[s]);
          }
          lds_barrier();
          multiply_pipelined(As, Bs, tx, ncol0, acc);
          buf ^= (WG_NBUF - 1);
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) {
#pragma unroll
      for (int j = 0; j < TN; ++j) { const int m = tx * TM + ii, n = ncol0 + j; if (m < M && ty * TN + j < NQ && n < N) ((XGLOBAL T*)pc)[n * LDC + m] = acc[ii][j]; }
    }
  }
}
#else
#if XGROUPED
__device__ XENTRY_ATTR void xsmm_entry(const DevAddr& ad, long long batch, unsigned xbid, unsigned xgrid, T* lds)
{
  if ((int)(threadIdx.x >> 6) >= XWAVES) return; // (the grouped kernel's work-groups have four waves)
#else
extern "C" __global__ __launch_bounds__(64 * XWAVES) void xsmm_smm_op(DevAddr ad, long long batch)
{
  __shared__ __attribute__((aligned(16))) T lds[XWAVES * WAVE_LDS];
  const unsigned xbid = blockIdx.x, xgrid = gridDim.x;
#endif
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  constexpr int LPI = 64 / G;                      // lanes per item
  const int grp = lane / LPI, tx = (lane % LPI) % TGM, ty = (lane % LPI) / TGM;
  T* const As = lds + wave * WAVE_LDS;
  T* const Bs = As + AS_SIZE;
  T* const Cs = C_OVER_AB ? As : (Bs + BS_SIZE);
  const long long w = (long long)xbid * XWAVES + wave, W = (long long)xgrid * XWAVES;
#if XRUNS
  // Consecutive items that share one C form a run (CP2K stacks, batch-reduce): the wave that owns the run's first item
  // keeps C in registers and adds the products in batch order -- what the reference's sequential loop does. Chunks of 64
  // items are dealt round-robin to the waves; run heads are found 64 items at a time (one item per lane, __ballot). A
  // wave walks its chain (see chain_of_chunk) item by item with the operands of the next D items in flight (and the C of
  // the next item, if it starts a run). A batch of distinct C blocks is the special case "all heads". Batches that
  // cannot (or need not) be walked in batch order go segment by segment, see segment_len.
  const int seg = segment_len(ad.flags, batch);
  if (XHASWG && nullptr != ad.flags && 0 == seg && 8LL * ad.flags[0] >= 7LL * batch) return; // runs of 8 and more on average: the work-group form owns this batch
  const long long step = (0 != seg ? seg : 64);
  T ra[D][NLA][VA], rb[D][NLB][VB], rc[NLC][VC];
  // every wave takes a contiguous range of chunks (see the work-group form)
  const long long nchunks = (batch + step - 1) / step, cpw = (nchunks + W - 1) / W;
  const long long c_end = ((w + 1) * cpw < nchunks) ? (w + 1) * cpw : nchunks;
  for (long long ci = w * cpw; ci < c_end; ++ci) {
    const long long chunk = ci * step;
    unsigned long long heads; long long first, end;
    if (0 != seg) { // a segment is walked from its first item, whoever opened the run it starts in
      heads = head_mask(ad, chunk, lane, batch) | 1ULL;
      first = chunk; end = (chunk + seg < batch ? chunk + seg : batch);
    }
    else if (!chain_of_chunk(ad, chunk, lane, batch, heads, first, end)) continue;
    AddrWindow win; window_fill(win, ad, first, lane, end);
#pragma unroll
    for (int s = 0; s < D; ++s) {
      if (first + s < end) {
        WINDOW_AB(win, first + s, pa, pb);
        load_flat<VA, NLA, AE>(pa, lane, ra[s]);
        load_flat<VB, NLB, BE>(pb, lane, rb[s]);
      }
    }
    if (!XBETA0 && 0 == seg) load_flat<VC, NLC, CE>(resolve<const T>(ad.c, ad.ic, ad.sc, ad, first), lane, rc);
    T acc[TM][TN];
    T* pc = nullptr;
    for (long long i0 = first; i0 < end; i0 += D) {
#pragma unroll
      for (int s = 0; s < D; ++s) {
        const long long i = i0 + s;
        if (i < end) {
          if (is_head(heads, chunk, i)) { // item i opens a run: close the previous one, take over its C
            if (0 != seg) {
              if (nullptr != pc) atomic_c(Cs, pc, lane, tx, ty, acc);
              pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, i);
              acc_from_c(Cs, tx, ty, acc, true);
            }
            else {
              if (nullptr != pc) store_c(Cs, pc, lane, tx, ty, acc);
              pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, i);
              if (!XBETA0) { park_c(Cs, lane, rc); wave_lds_sync(); }
              acc_from_c(Cs, tx, ty, acc, XBETA0);
              if (!XBETA0) wave_lds_sync(); // (the operand images are parked over C's next)
            }
          }
          park_ab(As, Bs, lane, ra[s], rb[s]);
          if (i + D < end) {
            WINDOW_AB(win, i + D, pa, pb);
            load_flat<VA, NLA, AE>(pa, lane, ra[s]);
            load_flat<VB, NLB, BE>(pb, lane, rb[s]);
          }
          if (!XBETA0 && 0 == seg && i + 1 < end && is_head(heads, chunk, i + 1)) load_flat<VC, NLC, CE>(resolve<const T>(ad.c, ad.ic, ad.sc, ad, i + 1), lane, rc);
          wave_lds_sync();
          multiply_pipelined(As, Bs, tx, ty * TN, acc);
          wave_lds_sync();
        }
      }
    }
    if (0 != seg) atomic_c(Cs, pc, lane, tx, ty, acc);
    else store_c(Cs, pc, lane, tx, ty, acc);
  }
#else
  if (w >= batch) return;
#if XLOWP
  unsigned ra[NPA][VPA], rb[NPB][VPB];
#if (2 == XLOWP)
  unsigned rc[NPC][VPC];
#else
  T rc[NLC][VC];
#endif
  // (the batch addresses 16-bit operands in elements of 16 bits -- strides, index arrays -- whichever the addressing mode)
  load_pairs<VPA, NPA, PA>((const unsigned*)resolve<const unsigned short>(ad.a, ad.ia, ad.sa, ad, w), lane, ra);
  load_pairs<VPB, NPB, PB>((const unsigned*)resolve<const unsigned short>(ad.b, ad.ib, ad.sb, ad, w), lane, rb);
#else
  T ra[NLA][VA], rb[NLB][VB], rc[NLC][VC];
  load_flat<VA, NLA, AE>(resolve<const T>(ad.a, ad.ia, ad.sa, ad, w), lane, ra);
  load_flat<VB, NLB, BE>(resolve<const T>(ad.b, ad.ib, ad.sb, ad, w), lane, rb);
#endif
#if (2 == XLOWP)
  if (!XBETA0) load_pairs<VPC, NPC, PC>((const unsigned*)resolve<const unsigned short>(ad.c, ad.ic, ad.sc, ad, w), lane, rc);
#else
  if (!XBETA0) load_flat<VC, NLC, CE>(resolve<const T>(ad.c, ad.ic, ad.sc, ad, w), lane, rc);
#endif
#if (2 != XLOWP)
  T* pend = nullptr; // C block whose result waits in the LDS image
#endif
  for (long long item = w; item < batch; item += W) {
#if (2 == XLOWP)
    unsigned* const pc = (unsigned*)resolve<unsigned short>(ad.c, ad.ic, ad.sc, ad, item);
#else
    T* const pc = resolve<T>(ad.c, ad.ic, ad.sc, ad, item);
    if (XDEFER) {
      __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): this item's operands; the only other instructions in flight are older stores
      if (nullptr != pend) { lds_to_mem(Cs, pend, lane); wave_lds_sync(); }
    }
#endif
#if XLOWP
    park_pairs(As, Bs, lane, ra, rb);
#else
    park_ab(As, Bs, lane, ra, rb);
#endif
#if (2 == XLOWP)
    if (!XBETA0) park_c_pairs(Cs, lane, rc);
#else
    if (!XBETA0) park_c(Cs, lane, rc);
#endif
    // ---- next item's loads go out before this item's arithmetic
    const long long next = item + W;
    if (next < batch) {
#if XLOWP
      load_pairs<VPA, NPA, PA>((const unsigned*)resolve<const unsigned short>(ad.a, ad.ia, ad.sa, ad, next), lane, ra);
      load_pairs<VPB, NPB, PB>((const unsigned*)resolve<const unsigned short>(ad.b, ad.ib, ad.sb, ad, next), lane, rb);
#else
      load_flat<VA, NLA, AE>(resolve<const T>(ad.a, ad.ia, ad.sa, ad, next), lane, ra);
      load_flat<VB, NLB, BE>(resolve<const T>(ad.b, ad.ib, ad.sb, ad, next), lane, rb);
#endif
#if (2 == XLOWP)
      if (!XBETA0) load_pairs<VPC, NPC, PC>((const unsigned*)resolve<const unsigned short>(ad.c, ad.ic, ad.sc, ad, next), lane, rc);
#else
      if (!XBETA0) load_flat<VC, NLC, CE>(resolve<const T>(ad.c, ad.ic, ad.sc, ad, next), lane, rc);
#endif
    }
    wave_lds_sync();
    T acc[TM][TN];
    acc_from_c(Cs + grp * CT1, tx, ty, acc, XBETA0);
    multiply(As + grp * AS1, Bs + grp * BS1, tx, ty * TN, acc);
#if (2 == XLOWP)
    store_c_pairs(Cs, pc, lane, tx, ty, acc, Cs + grp * CT1);
#else
    if (XDEFER) { c_to_lds(Cs + grp * CT1, tx, ty, acc); pend = pc; }
    else store_c(Cs, pc, lane, tx, ty, acc, Cs + grp * CT1);
#endif
  }
#if (2 != XLOWP)
  if (XDEFER && nullptr != pend) lds_to_mem(Cs, pend, lane);
#endif
#endif
}
#endif
