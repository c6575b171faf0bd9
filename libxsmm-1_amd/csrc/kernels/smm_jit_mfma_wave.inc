// smm_jit_mfma_wave.inc -- generated dense SMM kernel on the matrix cores, one wave per item (behind smm_jit_prelude.inc)
// ---- 32 < max(M, N) <= 64 on the matrix cores with ONE WAVE PER ITEM (tight operands, M and K multiples of four) --------
// The work-group-per-item kernels (kernels/smm_mfma_wg.inc) synchronise four waves twice per item and keep few items in
// flight per CU; below 64^3 they are latency-bound (40^3: 46 % of the HBM peak). Here a wave owns an item: C, A and B
// arrive as whole 16-byte chunks of the contiguous arrays (lanes past the end of an array repeat its last chunk: no
// divergent control flow around memory instructions, so the compiler's wait counts stay exact), C is redistributed through
// LDS into the tile layout of the accumulators, A and B are parked as LDS images that the operand fetches of
// v_mfma_{f32,f64}_16x16x4 read conflict-free (A: [k][MS], rows of 16 lanes at a stride that spreads the four k of a fetch
// over the banks; B: [n][KSD] with KSD/VEC odd), the result goes back through LDS and leaves as whole lines. Both
// instructions are k-ordered fma chains (tools/probe/mfma_f64_chain.hip; kernels/sparse.hip uses the fp32 one): C equals
// the reference's per-element chain bit for bit. The stores of item i are issued at the top of iteration i + 1, before
// the loads of item i + 2: vmcnt retires in the order of issue, so whenever the wave waits for its operands nothing younger
// is in flight and it never waits for a store to reach memory (tools/probe/mfma_wave.hip: 7.3 -> 2.2 us per item and wave).
constexpr int M = XM, N = XN, K = XK;
constexpr int TS = (int)sizeof(T);
// XVEC: elements per memory access -- a 16-byte chunk where the shape and the operands' alignment allow it (M a multiple of the
// chunk, K of four, 16-byte aligned items), else 1: any M, N, K and element-aligned operands (index and pointer batches)
constexpr int VEC = XVEC;
template<int W> struct VecOf { typedef T type __attribute__((ext_vector_type(W))); };
template<> struct VecOf<1> { typedef T type; };
typedef VecOf<VEC>::type V;
typedef T ACC __attribute__((ext_vector_type(4)));
constexpr bool F64 = (8 == TS);
// K is padded to a multiple of four with A = -0 and B = +0: the product -0 is the identity of the addition for every sum,
// signs of zeros included, so the chain stays the reference's bit for bit (as in kernels/smm_mfma_wg.inc)
constexpr int MI = (M + 15) / 16, NI = (N + 15) / 16, KP4 = geom::kp4(K), KS = KP4 / 4;
// the LDS images: geom::mfma_wave (kernels/smm_jit_geom.h) -- the host passes its lds_bytes as the dynamic LDS of the launch
constexpr geom::MfmaWave GEO = geom::mfma_wave(TS, M, N, K, VEC, 0 != XTRANSB);
// TRANS_B (memory holds B^T: element (k, n) at k * ldb + n): the image is k-major like A's, [k][NS], fetched the same way
constexpr int MS = GEO.ms, NS = GEO.ns, KSD = GEO.ksd, CSD = GEO.csd;
constexpr bool ASWZ = (64 == MS), BSWZ = (64 == NS);
constexpr int C_ELEMS = GEO.c_elems, A_ELEMS = GEO.a_elems, B_ELEMS = GEO.b_elems;
#if XLOWP
// bf16 inputs (XLOWP 3: fp32 result, 2: bf16 result) as the reference's low-precision kernels store them: A in pairs of k
// (a[(k/2)*M*2 + m*2 + k%2]), B column-major -- both sequences of 32-bit k pairs. A 16-byte chunk is four pairs (A: four
// rows m of one pair of k; B: eight consecutive k of one column); the halves are widened on the way into the same fp32 LDS
// images (a bf16 product is exact in fp32 unless it is subnormal or beyond FLT_MAX, so fma(a, b, acc) is the gold loop's
// product-then-add, samples/xgemm/kernel.c, everywhere else; the exception is pinned and documented, DESIGN.md 8j).
typedef unsigned UV __attribute__((ext_vector_type(4)));
constexpr int LDA = M, LDB = K, LDC = M;
constexpr bool TIGHT = true;
constexpr int NCA = M * K / 8, NCB = K * N / 8;                    // chunks per operand
constexpr int NCC = (2 == XLOWP) ? (M * N / 8) : (M * N / 4);
static_assert(0 == M % 4 && 0 == K % 8 && (2 != XLOWP || 0 == M % 8), "shape");
__device__ __forceinline__ V widen_lo(UV p) { return V{ __uint_as_float(p[0] << 16), __uint_as_float(p[1] << 16), __uint_as_float(p[2] << 16), __uint_as_float(p[3] << 16) }; }
__device__ __forceinline__ V widen_hi(UV p) { return V{ __uint_as_float(p[0] & 0xFFFF0000u), __uint_as_float(p[1] & 0xFFFF0000u), __uint_as_float(p[2] & 0xFFFF0000u), __uint_as_float(p[3] & 0xFFFF0000u) }; }
// eight consecutive bf16 (four pairs) as two vectors of four floats in memory order
__device__ __forceinline__ void widen8(UV p, V& v0, V& v1)
{
  v0 = V{ __uint_as_float(p[0] << 16), __uint_as_float(p[0] & 0xFFFF0000u), __uint_as_float(p[1] << 16), __uint_as_float(p[1] & 0xFFFF0000u) };
  v1 = V{ __uint_as_float(p[2] << 16), __uint_as_float(p[2] & 0xFFFF0000u), __uint_as_float(p[3] << 16), __uint_as_float(p[3] & 0xFFFF0000u) };
}
#else
// Leading dimensions as in memory (gaps only in the element-wise build): an operand is fetched as the one span of memory it
// occupies, elements in the gaps are dropped on the way into the images and never written on the way out.
constexpr int LDA = XLDA, LDB = XLDB, LDC = XLDC;
constexpr bool TIGHT = (LDA == M && LDB == (XTRANSB ? N : K) && LDC == M);
constexpr int NCA = (LDA * (K - 1) + M) / VEC, NCB = (XTRANSB ? (LDB * (K - 1) + N) : (LDB * (N - 1) + K)) / VEC, NCC = (LDC * (N - 1) + M) / VEC;
typedef V UV;
static_assert((1 == VEC || TIGHT) && geom::mfma_wave_served(M, N, K, VEC, 0 != XTRANSB), "shape");
#endif
constexpr int CA = (NCA + 63) / 64, CB = (NCB + 63) / 64, CC = (NCC + 63) / 64;
// row of C a lane's accumulator register r belongs to (the fp32 and fp64 instructions differ)
#define XNROW(r) (F64 ? (lq + 4 * (r)) : (4 * lq + (r)))
// what the batch's strides and index arrays count: elements of the operands' types (16-bit inputs, and a bf16 result, in 16-bit elements)
#if XLOWP
typedef unsigned short XOPI;
#if (2 == XLOWP)
typedef unsigned short XOPC;
#else
typedef T XOPC;
#endif
#else
typedef T XOPI; typedef T XOPC;
#endif

#if (2 != XNSPLIT)
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(XWPE))) void xsmm_smm_op(DevAddr ad, long long batch, int runlen)
{
  extern __shared__ __align__(16) unsigned char smem[];
  T* const As = reinterpret_cast<T*>(smem);
  T* const Bs = As + A_ELEMS;
  T* const Cs = As;                      // the image of C shares the place of A's (never alive together)
  T* const dummy = Bs + B_ELEMS;         // a word per lane for the writes of lanes outside C
  const int lane = threadIdx.x, l16 = lane & 15, lq = lane >> 4;
  (void)runlen;
  UV ra[CA], rb[CB], rc[CC]; // (strides of the batch are in 32-bit words: the host halves those of 16-bit operands)
  auto load_ab = [&](long long item) {
    const XGLOBAL UV* const pa = (const XGLOBAL UV*)resolve<const XOPI>(ad.a, ad.ia, ad.sa, ad, item);
    const XGLOBAL UV* const pb = (const XGLOBAL UV*)resolve<const XOPI>(ad.b, ad.ib, ad.sb, ad, item);
#pragma unroll
    for (int j = 0; j < CA; ++j) ra[j] = __builtin_nontemporal_load(pa + clampi(64 * j + lane, NCA - 1));
#pragma unroll
    for (int j = 0; j < CB; ++j) rb[j] = __builtin_nontemporal_load(pb + clampi(64 * j + lane, NCB - 1));
  };
  auto load_c = [&](long long item) {
    const XGLOBAL UV* const pc = (const XGLOBAL UV*)resolve<const XOPC>(ad.c, ad.ic, ad.sc, ad, item);
#pragma unroll
    for (int j = 0; j < CC; ++j) rc[j] = __builtin_nontemporal_load(pc + clampi(64 * j + lane, NCC - 1));
  };
  auto store_c = [&](long long item) { // the image of C -> memory, whole lines
    XGLOBAL UV* const pc = (XGLOBAL UV*)resolve<XOPC>(ad.c, ad.ic, ad.sc, ad, item);
#pragma unroll
    for (int j = 0; j < CC; ++j) {
      const int ch = clampi(64 * j + lane, NCC - 1);
#if (2 == XLOWP)
      const int e = ch * 8, n = e / M, m = e % M; // a bf16 result is the upper half of the float sum (truncation, as the harness does)
      const V v0 = *reinterpret_cast<const V*>(Cs + n * CSD + m), v1 = *reinterpret_cast<const V*>(Cs + n * CSD + m + 4);
      const UV w = UV{ (__float_as_uint(v0[0]) >> 16) | (__float_as_uint(v0[1]) & 0xFFFF0000u), (__float_as_uint(v0[2]) >> 16) | (__float_as_uint(v0[3]) & 0xFFFF0000u),
                       (__float_as_uint(v1[0]) >> 16) | (__float_as_uint(v1[1]) & 0xFFFF0000u), (__float_as_uint(v1[2]) >> 16) | (__float_as_uint(v1[3]) & 0xFFFF0000u) };
      __builtin_nontemporal_store(w, pc + ch);
#else
      const int e = ch * VEC, n = e / LDC, m = e % LDC;
      if (TIGHT || m < M) __builtin_nontemporal_store(*reinterpret_cast<const UV*>(Cs + n * CSD + (TIGHT ? m : clampi(m, M - 1))), pc + ch);
#endif
    }
  };
  long long item = blockIdx.x, prev = -1;
  if (item >= batch) return;
  load_ab(item);
  if (!XBETA0) load_c(item);
  if (KP4 > K) { // the padding of B's image: written once (its place is not shared)
    if (XTRANSB) { for (int e = lane; e < (KP4 - K) * NS; e += 64) Bs[K * NS + e] = T(0); }
    else { for (int e = lane; e < N * (KP4 - K); e += 64) Bs[(e / (KP4 - K)) * KSD + K + e % (KP4 - K)] = T(0); }
  }
  for (;;) {
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): this item's operands (the only other instructions in flight are older stores)
    if (0 <= prev) { store_c(prev); wave_lds_sync(); }
    // (the places in the images a lane parks its pieces at do not change from item to item: left to the compiler they are all
    // computed once and kept in registers -- a hundred of them in the element-wise form, which then spills. Recomputed per item
    // from a lane index the compiler cannot see through.)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    ACC acc[NI][MI];
    if (!XBETA0) {
#pragma unroll
      for (int j = 0; j < CC; ++j) {
        const int ch = clampi(64 * j + ln, NCC - 1);
#if (2 == XLOWP)
        const int e = ch * 8, n = e / M, m = e % M;
        V v0, v1; widen8(rc[j], v0, v1);
        *reinterpret_cast<V*>(Cs + n * CSD + m) = v0; *reinterpret_cast<V*>(Cs + n * CSD + m + 4) = v1;
#else
        const int e = ch * VEC, n = e / LDC, m = e % LDC;
        *reinterpret_cast<UV*>((TIGHT || m < M) ? Cs + n * CSD + m : dummy + lane) = rc[j];
#endif
      }
      wave_lds_sync();
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = clampi(16 * ni + XNROW(r), N - 1), m = clampi(16 * mi + l16, M - 1);
            acc[ni][mi][r] = Cs[n * CSD + m];
          }
      wave_lds_sync();
    }
    else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = ACC{ 0, 0, 0, 0 };
    }
    if (KP4 > K) { // the padding rows of A's image (the image of C has been lying over them)
      for (int e = lane; e < (KP4 - K) * MS; e += 64) As[K * MS + e] = -T(0);
    }
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const int ch = clampi(64 * j + ln, NCA - 1);
#if XLOWP
      const int w = ch * 4, sp = w / M, m = w % M, k0 = 2 * sp, k1 = 2 * sp + 1; // four rows of the k pair (2 sp, 2 sp + 1)
      *reinterpret_cast<V*>(As + k0 * MS + (ASWZ ? (m ^ ((k0 & 3) << 4)) : m)) = widen_lo(ra[j]);
      *reinterpret_cast<V*>(As + k1 * MS + (ASWZ ? (m ^ ((k1 & 3) << 4)) : m)) = widen_hi(ra[j]);
#else
      const int e = ch * VEC, k = e / LDA, m = e % LDA;
      *reinterpret_cast<V*>((TIGHT || m < M) ? As + k * MS + (ASWZ ? (m ^ ((k & 3) << 4)) : m) : dummy + lane) = ra[j];
#endif
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int ch = clampi(64 * j + ln, NCB - 1);
#if XLOWP
      const int e = ch * 8, n = e / K, k = e % K; // eight consecutive k of column n
      V v0, v1; widen8(rb[j], v0, v1);
      *reinterpret_cast<V*>(Bs + n * KSD + k) = v0; *reinterpret_cast<V*>(Bs + n * KSD + k + 4) = v1;
#else
#if XTRANSB
      const int e = ch * VEC, k = e / LDB, n = e % LDB;
      *reinterpret_cast<V*>((TIGHT || n < N) ? Bs + k * NS + (BSWZ ? (n ^ ((k & 3) << 4)) : n) : dummy + lane) = rb[j];
#else
      const int e = ch * VEC, n = e / LDB, k = e % LDB;
      *reinterpret_cast<V*>((TIGHT || k < K) ? Bs + n * KSD + k : dummy + lane) = rb[j];
#endif
#endif
    }
    const long long next = item + gridDim.x;
    if (next < batch) { load_ab(next); if (!XBETA0) load_c(next); }
    wave_lds_sync();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      T af[MI], bf[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) { const int m = 16 * mi + l16; af[mi] = As[(4 * ks + lq) * MS + (ASWZ ? (m ^ (lq << 4)) : m)]; }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int n = XTRANSB ? (16 * ni + l16) : clampi(16 * ni + l16, N - 1);
        bf[ni] = XTRANSB ? Bs[(4 * ks + lq) * NS + (BSWZ ? (n ^ (lq << 4)) : n)] : Bs[n * KSD + 4 * ks + lq];
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = xmfma(bf[ni], af[mi], acc[ni][mi]);
    }
    wave_lds_sync(); // (the images are dead now)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = 16 * ni + XNROW(r), m = 16 * mi + l16;
          const bool inside = (16 * ni + 15 < N || n < N) && (16 * mi + 15 < M || m < M);
          T* const dst = inside ? Cs + n * CSD + m : dummy + lane;
          *dst = acc[ni][mi][r];
        }
    wave_lds_sync();
    prev = item;
    if (next >= batch) break;
    item = next;
  }
  store_c(prev);
}
#else
// XNSPLIT 2: the columns of C are worked on in two halves against one image of A (items whose images would not leave room
// for four waves per CU: fp64 56^3 needs 55 KB). Per half: its C and B columns arrive, C goes through the place of B's half
// image into the accumulators, B is parked there, after the arithmetic the result waits there for the deferred stores. The
// operands of the next half -- or the next item's A and first half -- are in flight meanwhile. A's image is tight (stride M:
// two-way bank conflicts on its fetches, irrelevant next to 64-cycle fp64 matrix instructions).
constexpr geom::MfmaWave2 GEO2 = geom::mfma_wave2(TS, M, N, K);
constexpr int AMS = M;
constexpr int NH = N / 2, NIH = (NH + 15) / 16;
constexpr int CSH = M;
constexpr int BH_ELEMS = GEO2.bh_elems;
constexpr int CBH = (K * NH / VEC + 63) / 64, CCH = (M * NH / VEC + 63) / 64;
static_assert(geom::mfma_wave2_served(TS, M, N, K) && 16 == VEC * TS && K * AMS == GEO2.a_elems && 0 == XLOWP, "shape");
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(XWPE))) void xsmm_smm_op(DevAddr ad, long long batch, int runlen)
{
  extern __shared__ __align__(16) unsigned char smem[];
  T* const As = reinterpret_cast<T*>(smem);
  T* const Bs = As + K * AMS;
  T* const Cs = Bs;                      // the half image of C shares the place of B's half (never alive together)
  T* const dummy = Bs + BH_ELEMS;
  const int lane = threadIdx.x, l16 = lane & 15, lq = lane >> 4;
  (void)runlen;
  V ra[CA], rb[CBH], rc[CCH];
  auto load_a = [&](long long item) {
    const XGLOBAL V* const pa = (const XGLOBAL V*)resolve<const T>(ad.a, ad.ia, ad.sa, ad, item);
#pragma unroll
    for (int j = 0; j < CA; ++j) ra[j] = __builtin_nontemporal_load(pa + clampi(64 * j + lane, M * K / VEC - 1));
  };
  auto load_bc = [&](long long item, int h) {
    const XGLOBAL V* const pb = (const XGLOBAL V*)(resolve<const T>(ad.b, ad.ib, ad.sb, ad, item) + h * (K * NH));
#pragma unroll
    for (int j = 0; j < CBH; ++j) rb[j] = __builtin_nontemporal_load(pb + clampi(64 * j + lane, K * NH / VEC - 1));
    if (!XBETA0) {
      const XGLOBAL V* const pc = (const XGLOBAL V*)(resolve<const T>(ad.c, ad.ic, ad.sc, ad, item) + h * (M * NH));
#pragma unroll
      for (int j = 0; j < CCH; ++j) rc[j] = __builtin_nontemporal_load(pc + clampi(64 * j + lane, M * NH / VEC - 1));
    }
  };
  auto store_c = [&](long long item, int h) {
    XGLOBAL V* const pc = (XGLOBAL V*)(resolve<T>(ad.c, ad.ic, ad.sc, ad, item) + h * (M * NH));
#pragma unroll
    for (int j = 0; j < CCH; ++j) {
      const int ch = clampi(64 * j + lane, M * NH / VEC - 1), e = ch * VEC, n = e / M, m = e % M;
      __builtin_nontemporal_store(*reinterpret_cast<const V*>(Cs + n * CSH + m), pc + ch);
    }
  };
  long long item = blockIdx.x, prev = -1; int prevh = 0;
  if (item >= batch) return;
  load_a(item); load_bc(item, 0);
  for (;;) {
    const long long next = item + gridDim.x;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): this half's operands (the only other instructions in flight are older stores)
      if (0 <= prev) { store_c(prev, prevh); wave_lds_sync(); }
      ACC acc[NIH][MI];
      if (!XBETA0) {
#pragma unroll
        for (int j = 0; j < CCH; ++j) {
          const int ch = clampi(64 * j + lane, M * NH / VEC - 1), e = ch * VEC, n = e / M, m = e % M;
          *reinterpret_cast<V*>(Cs + n * CSH + m) = rc[j];
        }
        wave_lds_sync();
#pragma unroll
        for (int ni = 0; ni < NIH; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int n = clampi(16 * ni + XNROW(r), NH - 1), m = clampi(16 * mi + l16, M - 1);
              acc[ni][mi][r] = Cs[n * CSH + m];
            }
        wave_lds_sync();
      }
      else {
#pragma unroll
        for (int ni = 0; ni < NIH; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = ACC{ 0, 0, 0, 0 };
      }
      if (0 == h) {
#pragma unroll
        for (int j = 0; j < CA; ++j) {
          const int ch = clampi(64 * j + lane, M * K / VEC - 1), e = ch * VEC, k = e / M, m = e % M;
          *reinterpret_cast<V*>(As + k * AMS + m) = ra[j];
        }
      }
#pragma unroll
      for (int j = 0; j < CBH; ++j) {
        const int ch = clampi(64 * j + lane, K * NH / VEC - 1), e = ch * VEC, n = e / K, k = e % K;
        *reinterpret_cast<V*>(Bs + n * KSD + k) = rb[j];
      }
      if (0 == h) load_bc(item, 1);
      else if (next < batch) { load_a(next); load_bc(next, 0); }
      wave_lds_sync();
#pragma unroll 2
      for (int ks = 0; ks < KS; ++ks) { // (limited unrolling: with the whole k loop unrolled the operand fetches are hoisted and the registers spill)
        T af[MI], bf[NIH];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) { const int m = clampi(16 * mi + l16, M - 1); af[mi] = As[(4 * ks + lq) * AMS + m]; }
#pragma unroll
        for (int ni = 0; ni < NIH; ++ni) { const int n = clampi(16 * ni + l16, NH - 1); bf[ni] = Bs[n * KSD + 4 * ks + lq]; }
#pragma unroll
        for (int ni = 0; ni < NIH; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = xmfma(bf[ni], af[mi], acc[ni][mi]);
      }
      wave_lds_sync();
#pragma unroll
      for (int ni = 0; ni < NIH; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = 16 * ni + XNROW(r), m = 16 * mi + l16;
            const bool inside = (16 * ni + 15 < NH || n < NH) && (16 * mi + 15 < M || m < M);
            T* const dst = inside ? Cs + n * CSH + m : dummy + lane;
            *dst = acc[ni][mi][r];
          }
      wave_lds_sync();
      prev = item; prevh = h;
    }
    if (next >= batch) break;
    item = next;
  }
  store_c(prev, prevh);
}
#endif
