// tile_gemm.cuh -- what the tiled kernels on the matrix cores share (tgemm.hip, tgemm_lowp.hip, fc.hip): the
// arithmetic of a wave, the movement of a plain column-major C, the software-pipelined k loop and the band launch. Each
// kernel file keeps what really differs: its LDS image with the bank analysis, its loader and its store.
//
// The block: 256 threads, four waves as 2 x 2; a wave owns TW x TW tiles of the matrix instruction. k advances in chunks
// of BK through LDS; the next chunk travels from memory into registers while the current one is computed.
//
// Swapped operands. The "A" operand of the matrix instruction comes from the image of B: a lane then holds one row m of C
// and its registers walk n (Mfma*::nrow), so that loads and stores of C run along m, the fast dimension, 128 bytes per group.
//
// The k tail. Every element of C is one chain acc = fma(a, b, acc) over k in ascending order, which is what
// v_mfma_f32_32x32x2_f32 and v_mfma_f64_16x16x4_f64 compute per element (tests/test_mfma_runs_gpu.py). What is left after
// the last whole matrix step (k mod 2 for fp32, k mod 4 for fp64) is finished with fma on the vector ALU, accumulator
// element by element, in ascending k. A zero-padded matrix step would not do: fma(0, 0, -0.0) is +0.0.
#ifndef XSMM_TILE_GEMM_CUH
#define XSMM_TILE_GEMM_CUH

#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"

namespace tile {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int BT = xsmm::TGEMM_TILE; // extent of the work-group tile of the GEMM kernels (both ways)
constexpr int NTHREADS = 256;
static_assert(128 == BT, "the thread maps are written for 128 x 128");

#define TILE_INLINE __attribute__((always_inline)) // for the lambdas handed to k_loop and each

// The matrix instructions: TS x TS results from DEPTH values of k, NR of them per lane. Lane l holds row l % TS, supplies
// k = l / TS (kl) of a step, and its register r is column nrow(r, kl).
struct MfmaF32 { // v_mfma_f32_32x32x2_f32
  typedef float elem_t;
  typedef f32x16 acc_t;
  static constexpr int TS = 32, DEPTH = 2, NR = 16;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int nrow(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; }
  static __device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
};
struct MfmaF64 { // v_mfma_f64_16x16x4_f64
  typedef double elem_t;
  typedef f64x4 acc_t;
  static constexpr int TS = 16, DEPTH = 4, NR = 4;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int nrow(int r, int kl) { return kl + 4 * r; }
  static __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
};

// Element e of a thread's share of a chunk (BK x BT elements) of an operand in plain column-major layout. KFAST (the
// operand's fast dimension in memory is k): a wave fetches LI rows of 64 / LI consecutive k; otherwise 64 consecutive i
// of one k.
template<int BK, int LI, bool KFAST> __device__ __forceinline__ void where(int e, int& i, int& kk)
{
  i = KFAST ? ((e % LI) + LI * (e / (LI * BK))) : (e % BT);
  kk = KFAST ? ((e / LI) % BK) : (e / BT);
}

// One element of a plain column-major C rectangle of em x en elements: the load clamps its address into the rectangle
// (em, en >= 1; what it fetches beyond is never stored), the store is guarded.
template<typename E, typename O> __device__ __forceinline__ E c_get(const O* __restrict__ gc, long long ldc, int em, int en, int m, int n)
{
  return (E)gc[(size_t)(n < en ? n : en - 1) * (size_t)ldc + (size_t)(m < em ? m : em - 1)];
}
template<typename E, typename O> __device__ __forceinline__ void c_put(O* __restrict__ gc, long long ldc, int em, int en, int m, int n, E v)
{
  if (m < em && n < en) gc[(size_t)n * (size_t)ldc + (size_t)m] = (O)v;
}

// The fragment fetch of an image Xs[kk][i] with pitch P: a plain read.
template<typename T, int P> struct Plain {
  static __device__ __forceinline__ T at(const T* __restrict__ s, int i, int kk) { return s[kk * P + i]; }
};

// The arithmetic of a wave: instruction I, TW x TW tiles (a part of TW * TS both ways), chunks of BK. FETCH::at(s, i, kk)
// reads element (i, kk) of an operand's LDS image; UNROLL is the unroll factor of the loop over a full chunk.
template<typename I, int TW, int BK, typename FETCH, int UNROLL = BK / I::DEPTH> struct MatrixCores {
  typedef typename I::elem_t T;
  static constexpr int TS = I::TS, WT = TW * I::TS;
  typename I::acc_t acc[TW][TW]; // [j: along n][i: along m]
  int lm, kl, wm, wn;            // the lane's row inside a tile and its k inside a matrix step; the wave's origin
  __device__ __forceinline__ int row(int i) const { return wm + i * TS + lm; }
  __device__ __forceinline__ int col(int j, int r) const { return wn + j * TS + I::nrow(r, kl); }
  __device__ __forceinline__ void init(int t)
  {
    const int lane = t & 63, wave = t >> 6;
    lm = lane % TS; kl = lane / TS; wm = WT * (wave & 1); wn = WT * (wave >> 1);
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int i = 0; i < TW; ++i) {
#pragma unroll
        for (int r = 0; r < I::NR; ++r) acc[j][i][r] = (T)0;
      }
    }
  }
  // f(i, j, r, value) for every accumulator element: row(i), col(j, r)
  template<typename F> __device__ __forceinline__ void each(F f) const
  {
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int r = 0; r < I::NR; ++r) {
#pragma unroll
        for (int i = 0; i < TW; ++i) f(i, j, r, acc[j][i][r]);
      }
    }
  }
  template<typename O> __device__ __forceinline__ void c_load(const O* __restrict__ gc, long long ldc, int em, int en)
  {
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int r = 0; r < I::NR; ++r) {
#pragma unroll
        for (int i = 0; i < TW; ++i) acc[j][i][r] = c_get<T>(gc, ldc, em, en, row(i), col(j, r));
      }
    }
  }
  template<typename O> __device__ __forceinline__ void c_store(O* __restrict__ gc, long long ldc, int em, int en) const
  {
    each([&](int i, int j, int r, T v) TILE_INLINE { c_put(gc, ldc, em, en, row(i), col(j, r), v); });
  }
  template<typename S> __device__ __forceinline__ void step(const S* __restrict__ As, const S* __restrict__ Bs, int s)
  { // one matrix instruction per tile: the lane supplies k = DEPTH s + kl
    const int kk = s * I::DEPTH + kl;
    T av[TW], bv[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i) { av[i] = FETCH::at(As, wm + i * TS + lm, kk); bv[i] = FETCH::at(Bs, wn + i * TS + lm, kk); }
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int i = 0; i < TW; ++i) acc[j][i] = I::mma(bv[j], av[i], acc[j][i]);
    }
  }
  // kc <= BK values of k from the images As (of op(A): rows of C) and Bs (of op(B): columns of C)
  template<typename S> __device__ __forceinline__ void chunk(const S* __restrict__ As, const S* __restrict__ Bs, int kc)
  {
    if (BK == kc) {
#pragma unroll UNROLL
      for (int s = 0; s < BK / I::DEPTH; ++s) step(As, Bs, s);
    }
    else { // the last chunk: whole matrix steps first, then the tail on the vector ALU (no zero-padded step: see above)
      const int steps = kc / I::DEPTH;
      for (int s = 0; s < steps; ++s) step(As, Bs, s);
      for (int kk = steps * I::DEPTH; kk < kc; ++kk) {
        T av[TW];
#pragma unroll
        for (int i = 0; i < TW; ++i) av[i] = FETCH::at(As, wm + i * TS + lm, kk);
#pragma unroll
        for (int j = 0; j < TW; ++j) {
#pragma unroll
          for (int r = 0; r < I::NR; ++r) {
            const T bn = FETCH::at(Bs, col(j, r), kk);
#pragma unroll
            for (int i = 0; i < TW; ++i) acc[j][i][r] = I::fma_(av[i], bn, acc[j][i][r]);
          }
        }
      }
    }
  }
};

// The k loop: load(k0) fetches the chunk that starts at k0 into registers, store() writes the fetched chunk into LDS,
// chunk(kc) computes kc values of k from LDS.
template<int BK, typename LOAD, typename STORE, typename CHUNK>
__device__ __forceinline__ void k_loop(int k, LOAD load, STORE store, CHUNK chunk)
{
  load(0);
  for (int k0 = 0; k0 < k; k0 += BK) {
    __syncthreads(); // the previous chunk has been consumed
    store();
    __syncthreads();
    if (k0 + BK < k) load(k0 + BK); // the next chunk travels during this chunk's arithmetic
    chunk((k - k0 < BK) ? (k - k0) : BK);
  }
}

// The launch of a GEMM kernel family over C(m x n): KERNEL::get<TA, TB>() is the kernel of a pair of transposes, taking
// (a, b, c, mr, nr, k, lda, ldb, ldc, beta0); IN and OUT are the element types of A / B and C. Returns hipError_t as int.
template<typename KERNEL, typename IN, typename OUT, typename ARGS>
int band_launch(const ARGS& g, void* stream)
{
  const unsigned tiles_m = (unsigned)((g.m + BT - 1) / BT);
  const bool ta = (0 != g.transa), tb = (0 != g.transb);
  const auto kernel = ta ? (tb ? KERNEL::template get<true, true>() : KERNEL::template get<true, false>())
                         : (tb ? KERNEL::template get<false, true>() : KERNEL::template get<false, false>());
  constexpr int BAND = 65535 * BT; // columns of C one grid covers (gridDim.y); a wider rectangle goes band by band
  for (long long n0 = 0; n0 < g.n; n0 += BAND) {
    const int nb = (int)((g.n - n0 < BAND) ? (g.n - n0) : BAND);
    const dim3 grid(tiles_m, (unsigned)((nb + BT - 1) / BT)), block(NTHREADS);
    const IN* const a = static_cast<const IN*>(g.a);
    const IN* const b = static_cast<const IN*>(g.b) + (tb ? (size_t)n0 : (size_t)n0 * (size_t)g.ldb);
    OUT* const c = static_cast<OUT*>(g.c) + (size_t)n0 * (size_t)g.ldc;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0);
    const int e = (int)hipGetLastError();
    if (0 != e) return e;
  }
  return 0;
}

} // namespace tile

#endif
