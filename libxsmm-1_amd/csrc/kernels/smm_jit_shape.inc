// smm_jit_shape.inc -- the register-tiled forms, the part that depends on the shape (macros XM, XN, XK, ...): constants, LDS images,
// the transfers between memory, registers and LDS, the product out of LDS. Behind smm_jit_prelude.inc, in front of smm_jit_chain.inc
// and smm_jit_shape_kernels.inc; in a grouped text once per shape, inside the shape's namespace.
// (XLOWP 1, i16 -> i32: the k pairs stay packed -- one v_dot2_i32_i16 per pair -- so the kernel's k runs over pairs)
constexpr int M = XM, N = XN, K = (1 == XLOWP) ? (XK / 2) : XK;
// XPACK items that follow each other in memory (tight strided batches) are handled by a wave at a time: their operands are
// one contiguous piece (wider, fully used loads even when a single item is a few hundred bytes or not 16-byte sized), the
// 64 lanes split into XPACK groups with one item each. The host passes strides and the count in units of XPACK items.
constexpr int G = XPACK;
// Leading dimensions as in memory. LDS always holds the tight images; only the transfers know about the gaps: an operand is
// fetched as the one span of memory it occupies (gaps included), elements in the gaps are dropped on the way into LDS and
// never written on the way out.
constexpr int LDA = XLDA, LDB = XLDB, LDC = XLDC;
constexpr bool TIGHT_A = (LDA == M), TIGHT_B = (LDB == (XTRANSB ? N : K)), TIGHT_C = (LDC == M);
constexpr int AE1 = LDA * (K - 1) + M, BE1 = XTRANSB ? (LDB * (K - 1) + N) : (LDB * (N - 1) + K), CE1 = LDC * (N - 1) + M; // span of one item's operand
constexpr int CT1 = M * N;                                          // tight C image of one item
constexpr int AE = G * AE1, BE = G * BE1, CE = G * CE1;            // ... of what a wave handles at a time (G > 1: tight only)
constexpr int TS = (int)sizeof(T);
// lane tiles and LDS images: geom::tiled (kernels/smm_jit_geom.h), the numbers the host sizes the launch with
constexpr geom::Tiled GEO = geom::tiled(TS, M, N, K, 0 != XTRANSB, G, XRUNS);
#if (2 == XRUNS)
// work-group form: 4 waves share one product; a wave owns NQ = ceil(N/4) columns of C, its 64 lanes are 16 (along m) x 4
constexpr int UT = 256;                                            // threads that stream one item's operands
constexpr int NQ = GEO.nq;
#else
// wave form: one wave per item, 8 x 8 lanes (XPACK items: 64 / XPACK lanes each)
constexpr int UT = 64;
#endif
constexpr int TGM = GEO.tgm, TGN = GEO.tgn, TM = GEO.tm, TN = GEO.tn, NPAD = GEO.npad;
// widest access (in elements) that every item of a strided batch is aligned for
constexpr int vw(int elems) { return (0 == (elems * TS) % 16) ? 16 / TS : ((0 == (elems * TS) % 8) ? 8 / TS : 1); }
// XSCALAR: index/pointer batches guarantee element alignment only
constexpr int VA = XSCALAR ? 1 : vw(AE), VB = XSCALAR ? 1 : vw(BE), VC = (XSCALAR || !TIGHT_C) ? 1 : vw(CE);
constexpr int NLA = (AE + UT * VA - 1) / (UT * VA), NLB = (BE + UT * VB - 1) / (UT * VB), NLC = (CE + UT * VC - 1) / (UT * VC);
constexpr int KP = GEO.kp, AS1 = GEO.as1, BS1 = GEO.bs1;             // LDS, per item: A as [k][M], B as [n][KP] (TRANS_B: [k][N])
constexpr int AS_SIZE = G * AS1, BS_SIZE = G * BS1;
constexpr int CS_SIZE = GEO.cs;                                      // the items' C blocks stay contiguous (flat copy in and out)
constexpr bool C_OVER_AB = (1 == XRUNS);                             // wave run form: C's image lies over the operands'
constexpr int WAVE_LDS = GEO.wave_lds;                               // elements (wave form)
constexpr int WG_BUF = GEO.wg_buf, WG_NBUF = GEO.wg_nbuf;            // elements per operand buffer (work-group form); two when 64 KiB allow

template<int V> struct Vec { typedef T type __attribute__((ext_vector_type(V))); };
template<> struct Vec<1> { typedef T type; };

// Operands are in global memory, but their addresses come out of a run-time choice between three addressing modes (one of
// them loads the pointer): left generic, every access becomes a FLAT instruction, which also counts on lgkmcnt -- each wait
// for an LDS operation would then wait for the prefetched operands as well. Hence the explicit address space.
template<int V, int NL, int E> __device__ __forceinline__ void load_flat(const T* p, int lane, T (&r)[NL][V])
{
  const XGLOBAL T* const g = (const XGLOBAL T*)p;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    // lanes past the end fetch the last piece again (never used): no divergent control flow around the loads, so the
    // compiler's count of what is in flight at a wait stays exact instead of falling back to "everything"
    const int e0 = (UT * j + lane) * V, e = (e0 < E - V) ? e0 : (E - V);
    if constexpr (1 == V) r[j][0] = __builtin_nontemporal_load(g + e);
    else {
      const typename Vec<V>::type v = __builtin_nontemporal_load(reinterpret_cast<const XGLOBAL typename Vec<V>::type*>(g + e));
#pragma unroll
      for (int q = 0; q < V; ++q) r[j][q] = v[q];
    }
  }
}

// registers -> LDS (A as stored, B with the padded row stride); `lane` is the thread's index among the UT streaming threads
__device__ __forceinline__ void park_ab(T* As, T* Bs, int lane, const T (&ra)[NLA][VA], const T (&rb)[NLB][VB])
{
#pragma unroll
  for (int j = 0; j < NLA; ++j) {
#pragma unroll
    for (int q = 0; q < VA; ++q) {
      const int e = (UT * j + lane) * VA + q;
      if (e < AE) {
        if (TIGHT_A) As[(1 == G) ? e : ((e / AE1) * AS1 + (e % AE1))] = ra[j][q];
        else { const int k = e / LDA, m = e - k * LDA; if (m < M) As[k * M + m] = ra[j][q]; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
#pragma unroll
    for (int q = 0; q < VB; ++q) {
      const int e = (UT * j + lane) * VB + q;
      if (e < BE) {
        const int g = (1 == G) ? 0 : (e / BE1), r = (1 == G) ? e : (e % BE1);
        if (XTRANSB) { if (TIGHT_B) Bs[g * BS1 + r] = rb[j][q]; else { const int k = r / LDB, n = r - k * LDB; if (n < N) Bs[k * N + n] = rb[j][q]; } }
        else { const int n = r / LDB, k = r - n * LDB; if (k < K) Bs[g * BS1 + n * KP + k] = rb[j][q]; }
      }
    }
  }
}
__device__ __forceinline__ void park_c(T* Cs, int lane, const T (&rc)[NLC][VC])
{
#pragma unroll
  for (int j = 0; j < NLC; ++j) {
#pragma unroll
    for (int q = 0; q < VC; ++q) {
      const int e = (64 * j + lane) * VC + q;
      if (e < CE) { if (TIGHT_C) Cs[e] = rc[j][q]; else { const int n = e / LDC, m = e - n * LDC; if (m < M) Cs[n * M + m] = rc[j][q]; } }
    }
  }
}
#if XLOWP
// 16-bit inputs (XLOWP 1: i16, T = int; 3: bf16, T = float), stored as the reference's low-precision kernels expect them: A in
// pairs of k (a[(k/2)*M*2 + m*2 + k%2]), B column-major -- both are sequences of 32-bit k pairs. They are fetched as such and
// widened on the way into LDS, where the images are the ones of the fp32 / int kernels; everything after that is shared.
constexpr int PA1 = (M * XK) / 2, PB1 = (XK * N) / 2;              // k pairs per operand and item (XK is even)
constexpr int PA = G * PA1, PB = G * PB1;                          // ... of the XPACK items a wave handles at a time (back to back in memory)
constexpr int VPA = (0 == (PA * 4) % 16 && !XSCALAR) ? 4 : 1, VPB = (0 == (PB * 4) % 16 && !XSCALAR) ? 4 : 1;
constexpr int NPA = (PA + 64 * VPA - 1) / (64 * VPA), NPB = (PB + 64 * VPB - 1) / (64 * VPB);
template<int V> struct PVec { typedef unsigned type __attribute__((ext_vector_type(V))); };
template<> struct PVec<1> { typedef unsigned type; };
template<int V, int NL, int E> __device__ __forceinline__ void load_pairs(const unsigned* p, int lane, unsigned (&r)[NL][V])
{
  const XGLOBAL unsigned* const g = (const XGLOBAL unsigned*)p;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int e = (64 * j + lane) * V;
    if (e < E) {
      if constexpr (1 == V) r[j][0] = __builtin_nontemporal_load(g + e);
      else {
        const typename PVec<V>::type v = __builtin_nontemporal_load(reinterpret_cast<const XGLOBAL typename PVec<V>::type*>(g + e));
#pragma unroll
        for (int q = 0; q < V; ++q) r[j][q] = v[q];
      }
    }
  }
}
__device__ __forceinline__ T widen_lo(unsigned p) { return (1 == XLOWP) ? (T)(int)(short)(p & 0xFFFFu) : (T)__uint_as_float(p << 16); }
__device__ __forceinline__ T widen_hi(unsigned p) { return (1 == XLOWP) ? (T)(int)(short)(p >> 16) : (T)__uint_as_float(p & 0xFFFF0000u); }
__device__ __forceinline__ void park_pairs(T* As, T* Bs, int lane, const unsigned (&ra)[NPA][VPA], const unsigned (&rb)[NPB][VPB])
{
#pragma unroll
  for (int j = 0; j < NPA; ++j) {
#pragma unroll
    for (int q = 0; q < VPA; ++q) {
      const int e = (64 * j + lane) * VPA + q;
      if (e < PA) {
        const int it = e / PA1, e1 = e - it * PA1, sp = e1 / M, m = e1 - sp * M;
        T* const Ai = As + it * AS1;
        if (1 == XLOWP) Ai[sp * M + m] = (T)ra[j][q]; // packed pair
        else { Ai[(2 * sp) * M + m] = widen_lo(ra[j][q]); Ai[(2 * sp + 1) * M + m] = widen_hi(ra[j][q]); }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NPB; ++j) {
#pragma unroll
    for (int q = 0; q < VPB; ++q) {
      const int e = (64 * j + lane) * VPB + q;
      if (e < PB) {
        const int it = e / PB1, e1 = e - it * PB1, n = e1 / (XK / 2), sp = e1 - n * (XK / 2);
        T* const Bi = Bs + it * BS1;
        if (1 == XLOWP) Bi[n * KP + sp] = (T)rb[j][q];
        else { Bi[n * KP + 2 * sp] = widen_lo(rb[j][q]); Bi[n * KP + 2 * sp + 1] = widen_hi(rb[j][q]); }
      }
    }
  }
}
#if (2 == XLOWP)
// bf16 -> bf16: C travels as 32-bit pairs of bf16 as well (M is a multiple of 16: a pair never straddles a column); the sums
// are float, a result is the upper half of the float (truncation, as the reference's harness does)
constexpr int PC = G * ((M * N) / 2); // (the items' C blocks are contiguous in memory and in the wave's C buffer alike)
constexpr int VPC = (0 == (PC * 4) % 16 && !XSCALAR) ? 4 : 1;
constexpr int NPC = (PC + 64 * VPC - 1) / (64 * VPC);
template<int V> __device__ __forceinline__ void store_pvec(const unsigned* v, XGLOBAL unsigned* dst)
{
  typename PVec<V>::type w;
#pragma unroll
  for (int q = 0; q < V; ++q) w[q] = v[q];
  __builtin_nontemporal_store(w, reinterpret_cast<XGLOBAL typename PVec<V>::type*>(dst));
}
template<> __device__ __forceinline__ void store_pvec<1>(const unsigned* v, XGLOBAL unsigned* dst) { __builtin_nontemporal_store(v[0], dst); }
__device__ __forceinline__ void park_c_pairs(T* Cs, int lane, const unsigned (&rc)[NPC][VPC])
{
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
#pragma unroll
    for (int q = 0; q < VPC; ++q) { const int e = (64 * j + lane) * VPC + q; if (e < PC) { Cs[2 * e] = widen_lo(rc[j][q]); Cs[2 * e + 1] = widen_hi(rc[j][q]); } }
  }
}
__device__ __forceinline__ void store_c_pairs(T* Cs, unsigned* pc, int lane, int tx, int ty, const T (&acc)[TM][TN], T* Ci)
{ // (Ci: this lane's item inside the wave's C buffer Cs)
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) Ci[n * M + m] = acc[i][j]; }
  }
  wave_lds_sync();
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int e = (64 * j + lane) * VPC;
    if (e < PC) {
      unsigned v[VPC];
#pragma unroll
      for (int q = 0; q < VPC; ++q) v[q] = (__float_as_uint(Cs[2 * (e + q)]) >> 16) | (__float_as_uint(Cs[2 * (e + q) + 1]) & 0xFFFF0000u);
      store_pvec<VPC>(v, (XGLOBAL unsigned*)pc + e);
    }
  }
  wave_lds_sync();
}
#endif
#endif
#if (2 == XLOWP || 3 == XLOWP)
// bf16 inputs: product and sum are rounded one after the other, as in the gold loop and in the pre-compiled kernel (smm_lowp.hip).
// The product of two bf16 numbers is exact in float32 unless it is subnormal or beyond FLT_MAX; there an fma has other bits, and a
// descriptor must not change its result with the size of the batch. (The pragma: the compiler's default contracts a * b + c.)
__device__ __forceinline__ float xstep(float a, float b, float c)
{
#pragma clang fp contract(off)
  const float p = a * b;
  return c + p;
}
#else
template<typename X> __device__ __forceinline__ X xstep(X a, X b, X c) { return xfma(a, b, c); }
#endif
// acc(i,j) = fma(A(m,k), B(k,n), acc(i,j)) for k ascending: the reference's per-element chain
__device__ __forceinline__ void multiply(const T* As, const T* Bs, int tx, int ncol0, T (&acc)[TM][TN])
{
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    T av[TM], bv[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) av[i] = As[k * M + tx * TM + i];
#pragma unroll
    for (int j = 0; j < TN; ++j) bv[j] = XTRANSB ? Bs[k * N + ncol0 + j] : Bs[(ncol0 + j) * KP + k];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = xstep(av[i], bv[j], acc[i][j]);
    }
  }
}
#if XRUNS
// The run forms keep few waves per CU busy (a run is a sequential chain), so nothing hides the LDS round trip between an
// operand read and its fma. Software pipeline over groups of KU k-steps: the reads of group g+1 are issued before the fmas
// of group g (two register sets, fully unrolled: all indices are compile-time constants).
constexpr int KU = (2 == XRUNS) ? 4 : 2;
constexpr int NG = (K + KU - 1) / KU;
__device__ __forceinline__ void read_group(const T* As, const T* Bs, int tx, int ncol0, int g, T (&av)[KU][TM], T (&bv)[KU][TN])
{
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int k = g * KU + u;
    if (k < K) {
#pragma unroll
      for (int i = 0; i < TM; ++i) av[u][i] = As[k * M + tx * TM + i];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[u][j] = XTRANSB ? Bs[k * N + ncol0 + j] : Bs[(ncol0 + j) * KP + k];
    }
  }
}
__device__ __forceinline__ void fma_group(int g, const T (&av)[KU][TM], const T (&bv)[KU][TN], T (&acc)[TM][TN])
{
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    if (g * KU + u < K) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = xfma(av[u][i], bv[u][j], acc[i][j]);
      }
    }
  }
}
__device__ __forceinline__ void multiply_pipelined(const T* As, const T* Bs, int tx, int ncol0, T (&acc)[TM][TN])
{
  T a0[KU][TM], b0[KU][TN], a1[KU][TM], b1[KU][TN];
  read_group(As, Bs, tx, ncol0, 0, a0, b0);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (0 == (g & 1)) { if (g + 1 < NG) read_group(As, Bs, tx, ncol0, g + 1, a1, b1); fma_group(g, a0, b0, acc); }
    else { if (g + 1 < NG) read_group(As, Bs, tx, ncol0, g + 1, a0, b0); fma_group(g, a1, b1, acc); }
  }
}
#endif

__device__ __forceinline__ void acc_from_c(const T* Cs, int tx, int ty, T (&acc)[TM][TN], bool zero)
{
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int m = tx * TM + i, n = ty * TN + j;
      acc[i][j] = (!zero && m < M && n < N) ? Cs[n * M + m] : (T)0;
    }
  }
}
// C leaves through LDS so that the stores are flat and coalesced
// (Ci: this lane's item inside the wave's C buffer Cs; the two are the same unless XPACK > 1)
__device__ __forceinline__ void store_c(T* Cs, T* pc, int lane, int tx, int ty, const T (&acc)[TM][TN], T* Ci = nullptr)
{
  if (nullptr == Ci) Ci = Cs;
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) Ci[n * M + m] = acc[i][j]; }
  }
  wave_lds_sync();
#pragma unroll
  for (int j = 0; j < NLC; ++j) {
    const int e = (64 * j + lane) * VC;
    if (e < CE) {
      if constexpr (!TIGHT_C) { const int n = e / LDC, m = e - n * LDC; if (m < M) __builtin_nontemporal_store(Cs[n * M + m], (XGLOBAL T*)pc + e); } // (VC == 1)
      else if constexpr (1 == VC) __builtin_nontemporal_store(Cs[e], (XGLOBAL T*)pc + e);
      else __builtin_nontemporal_store(*reinterpret_cast<const typename Vec<VC>::type*>(Cs + e), reinterpret_cast<XGLOBAL typename Vec<VC>::type*>((XGLOBAL T*)pc + e));
    }
  }
  wave_lds_sync();
}

// The streaming form defers the stores of an item to the top of the next iteration, in front of that iteration's loads:
// vmcnt retires loads and stores in the order of issue, so stores issued right behind the arithmetic -- younger than the
// prefetched operands -- made the wait for the operands a wait for the previous item's C to reach memory as well (measured
// on tools/probe/mfma_wave.hip: 7.3 -> 2.2 us per item and wave).
__device__ __forceinline__ void c_to_lds(T* Ci, int tx, int ty, const T (&acc)[TM][TN])
{
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) Ci[n * M + m] = acc[i][j]; }
  }
  wave_lds_sync();
}
__device__ __forceinline__ void lds_to_mem(const T* Cs, T* pc, int lane)
{
#pragma unroll
  for (int j = 0; j < NLC; ++j) {
    if constexpr (!TIGHT_C) { const int e = 64 * j + lane; if (e < CE) { const int n = e / LDC, m = e - n * LDC; if (m < M) __builtin_nontemporal_store(Cs[n * M + m], (XGLOBAL T*)pc + e); } } // (VC == 1)
    else { // (lanes past the end repeat the last piece: same data to the same place)
      const int e0 = (64 * j + lane) * VC, e = (e0 < CE - VC) ? e0 : (CE - VC);
      if constexpr (1 == VC) __builtin_nontemporal_store(Cs[e], (XGLOBAL T*)pc + e);
      else __builtin_nontemporal_store(*reinterpret_cast<const typename Vec<VC>::type*>(Cs + e), reinterpret_cast<XGLOBAL typename Vec<VC>::type*>((XGLOBAL T*)pc + e));
    }
  }
}

#if XRUNS
// a segment's sum joins C: through LDS so that the atomics of a wave cover consecutive addresses
__device__ __forceinline__ void atomic_c(T* Cs, T* pc, int lane, int tx, int ty, const T (&acc)[TM][TN])
{
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) Cs[n * M + m] = acc[i][j]; }
  }
  wave_lds_sync();
  for (int e = lane; e < M * N; e += 64) xatomic_add(pc + (TIGHT_C ? e : ((e / M) * LDC + (e % M))), Cs[e]);
  wave_lds_sync();
}
#endif

