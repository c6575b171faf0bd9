// smm_jit_big.inc -- shapes with 32 < M or N <= 64 (and small M, N with a long K): one work-group (256 threads, 16 x 16) per item,
// K in chunks of KC through two LDS buffers. Behind smm_jit_prelude.inc with XFLAT 0: DevAddr, resolve, xfma, lds_barrier.
constexpr int M = XM, N = XN, K = XK, KC = XKC;
constexpr geom::Big GEO = geom::big((int)sizeof(T), M, N, KC);    // (kernels/smm_jit_geom.h)
constexpr int TM = GEO.tm, TN = GEO.tn;                            // register tile of a thread (tx = t & 15 along m, ty = t >> 4 along n)
constexpr int NCH = (K + KC - 1) / KC;                             // k-chunks per item
constexpr int AEL = KC * M, BEL = KC * N;                          // elements of one chunk
constexpr int NLA = (AEL + 255) / 256, NLB = (BEL + 255) / 256;    // per thread
// LDS images of a chunk: A as [kk][MP], B as [kk][NPP] (a row padded by 16 bytes), two buffers of BUF elements
constexpr int MP = GEO.mp, NP = GEO.np, NPP = GEO.npp, AS = GEO.as, BS = GEO.bs, BUF = GEO.buf;

// chunk ch of one item: A rows k0..k0+KC (contiguous KC*M elements), B rows k0..k0+KC of every column (TRANS_B: contiguous)
__device__ __forceinline__ void load_chunk(const T* pa, const T* pb, int ch, int t, T (&ra)[NLA], T (&rb)[NLB])
{
  const int k0 = ch * KC, kc = (K - k0 < KC) ? (K - k0) : KC;
  const XGLOBAL T* const ga = (const XGLOBAL T*)pa + (long long)k0 * M;
#pragma unroll
  for (int j = 0; j < NLA; ++j) { const int e = 256 * j + t; if (e < kc * M) ra[j] = __builtin_nontemporal_load(ga + e); }
  if (XTRANSB) {
    const XGLOBAL T* const gb = (const XGLOBAL T*)pb + (long long)k0 * N;
#pragma unroll
    for (int j = 0; j < NLB; ++j) { const int e = 256 * j + t; if (e < kc * N) rb[j] = __builtin_nontemporal_load(gb + e); }
  }
  else {
    const XGLOBAL T* const gb = (const XGLOBAL T*)pb + k0;
#pragma unroll
    for (int j = 0; j < NLB; ++j) { const int e = 256 * j + t, n = e / KC, kk = e - n * KC; if (e < BEL && kk < kc) rb[j] = __builtin_nontemporal_load(gb + (long long)n * K + kk); }
  }
}
__device__ __forceinline__ void park_chunk(T* As, T* Bs, int ch, int t, const T (&ra)[NLA], const T (&rb)[NLB])
{
  const int k0 = ch * KC, kc = (K - k0 < KC) ? (K - k0) : KC;
#pragma unroll
  for (int j = 0; j < NLA; ++j) { const int e = 256 * j + t; if (e < kc * M) { const int kk = e / M, m = e - kk * M; As[kk * MP + m] = ra[j]; } }
  if (XTRANSB) {
#pragma unroll
    for (int j = 0; j < NLB; ++j) { const int e = 256 * j + t; if (e < kc * N) { const int kk = e / N, n = e - kk * N; Bs[kk * NPP + n] = rb[j]; } }
  }
  else {
#pragma unroll
    for (int j = 0; j < NLB; ++j) { const int e = 256 * j + t, n = e / KC, kk = e - n * KC; if (e < BEL && kk < kc) Bs[kk * NPP + n] = rb[j]; }
  }
}

// runlen: the batch is a sequence of runs of `runlen` consecutive items that share one C (blocked GEMM: the k blocks of a C
// block; 1: every item owns its C). A work-group keeps C in registers across a run: the chain of the sequential reference.
extern "C" __global__ __launch_bounds__(256) void xsmm_smm_op(DevAddr ad, long long batch, long long runlen)
{
  __shared__ __attribute__((aligned(16))) T lds[2 * BUF];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const long long nruns = batch / runlen, G = gridDim.x;
  long long run = blockIdx.x;
  if (run >= nruns) return;
  long long item = run * runlen, p = 0;
  T ra[NLA], rb[NLB], rc[TM][TN], acc[TM][TN];
  // software pipeline over (item, chunk): the registers hold the chunk after the one that is being multiplied
  load_chunk(resolve<const T>(ad.a, ad.ia, ad.sa, ad, item), resolve<const T>(ad.b, ad.ib, ad.sb, ad, item), 0, t, ra, rb);
  if (!XBETA0) {
    const XGLOBAL T* const gc = (const XGLOBAL T*)resolve<T>(ad.c, ad.ic, ad.sc, ad, item);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
      for (int i = 0; i < TM; ++i) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) rc[i][j] = gc[n * M + m]; }
    }
  }
  int buf = 0;
  for (;;) {
    if (0 == p) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = XBETA0 ? (T)0 : rc[i][j];
      }
    }
    const bool same_run = (p + 1 < runlen), has_next = same_run || (run + G < nruns);
    const long long next = same_run ? (item + 1) : ((run + G) * runlen);
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
      T* const As = lds + buf * BUF;
      T* const Bs = As + AS;
      park_chunk(As, Bs, ch, t, ra, rb);
      if (ch + 1 < NCH) load_chunk(resolve<const T>(ad.a, ad.ia, ad.sa, ad, item), resolve<const T>(ad.b, ad.ib, ad.sb, ad, item), ch + 1, t, ra, rb);
      else if (has_next) { // first chunk of the next item, and its C if it opens a run
        load_chunk(resolve<const T>(ad.a, ad.ia, ad.sa, ad, next), resolve<const T>(ad.b, ad.ib, ad.sb, ad, next), 0, t, ra, rb);
        if (!XBETA0 && !same_run) {
          const XGLOBAL T* const gc = (const XGLOBAL T*)resolve<T>(ad.c, ad.ic, ad.sc, ad, next);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int i = 0; i < TM; ++i) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) rc[i][j] = gc[n * M + m]; }
          }
        }
      }
      lds_barrier();
      const int k0 = ch * KC, kc = (K - k0 < KC) ? (K - k0) : KC;
#pragma unroll 4
      for (int kk = 0; kk < kc; ++kk) {
        T av[TM], bv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) av[i] = As[kk * MP + tx * TM + i];
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = Bs[kk * NPP + ty * TN + j];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = xfma(av[i], bv[j], acc[i][j]);
        }
      }
      buf ^= 1;
    }
    if (!same_run) { // the run is complete
      XGLOBAL T* const gc = (XGLOBAL T*)resolve<T>(ad.c, ad.ic, ad.sc, ad, item);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
#pragma unroll
        for (int i = 0; i < TM; ++i) { const int m = tx * TM + i, n = ty * TN + j; if (m < M && n < N) __builtin_nontemporal_store(acc[i][j], gc + n * M + m); }
      }
    }
    if (!has_next) break;
    if (same_run) ++p; else { p = 0; run += G; }
    item = next;
  }
}
