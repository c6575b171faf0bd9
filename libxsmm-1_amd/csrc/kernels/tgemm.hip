// tgemm.hip -- the tiled GEMM on the matrix cores: C(m x n) = op(A) * op(B) + beta * C, beta in {0, 1}, fp32 and fp64,
// behind libxsmm_gemm_thread / libxsmm_xgemm_omp (xsmm_tgemm.cpp).
//
// Reference: libxsmm_gemm_thread (src/libxsmm_gemm.c:1067-1228) walks tiles of C and calls an SMM kernel per k-chunk: the
// beta kernel on the first chunk, the beta = 1 kernel afterwards (:1158-1201). Every element of C therefore is one fused
// multiply-add chain over k in ascending order that starts from C (beta = 1) or from 0 (beta = 0), whatever the tiles are.
// That is what v_mfma_f32_32x32x2_f32 and v_mfma_f64_16x16x4_f64 compute per element (tests/test_mfma_runs_gpu.py), so
// this kernel carries the bits of the SMM kernels at any size.
//
// A work-group of 256 threads (four waves, 2 x 2) owns a 128 x 128 tile of C; a wave holds its 64 x 64 quarter in
// accumulators (fp32: 2 x 2 tiles of 32 x 32, 64 registers; fp64: 4 x 4 tiles of 16 x 16, 128 registers). k advances in
// chunks of BK (fp32: 32, fp64: 16) through LDS; the next chunk travels from memory into registers while the matrix
// cores work on the current one.
//
// LDS image, the same for every combination of transposes: As[kk][i] = op(A)(i, kk) and Bs[kk][j] = op(B)(kk, j), pitch P
// elements per kk. An operand whose fast dimension is i (A 'N', B 'T') is read and written along i. One whose fast
// dimension is k (A 'T', B 'N') is read by a wave as LI columns of 64 / LI consecutive k and written column-wise.
// Banks (MI355X: ds_read_b32 / ds_write_b32 serve lanes {0-31}, {32-63} against 32 banks of 4 bytes; ds_read_b64 the same
// groups against 64 banks; ds_write_b64 groups of 16 consecutive lanes against 32 banks):
//   fp32, P = 136 = 8 mod 32.  operand read: a group is 32 consecutive floats of one kk: 32 banks. Write along i: the same.
//     Write along k (LI = 8): a group is 8 i x 4 kk at banks 8 kk + i: 32 banks.
//   fp64, P = 144: two rows are 288 = 32 mod 64 words apart.  operand read: a group is 16 doubles of row kk (32 banks)
//     and 16 of row kk + 1 (the other 32). Write along i, and along k (LI = 16): a group is 16 consecutive doubles: 32 banks.
//
// The matrix instruction's swapped operands and the k tail (k mod 2 for fp32, k mod 4 for fp64, on the vector ALU): tile_gemm.cuh.
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::BT;
using tile::NTHREADS;

template<typename T> struct Cfg;
template<> struct Cfg<float> { typedef tile::MfmaF32 I; static constexpr int BK = 32, P = BT + 8, LI = 8; };
template<> struct Cfg<double> { typedef tile::MfmaF64 I; static constexpr int BK = 16, P = BT + 16, LI = 16; };

// One chunk of an operand: BK x BT elements, NL per thread. KFAST: the operand's fast dimension in memory is k.
// g points at element (i = 0, k = 0) of the work-group's part; ext_i and ext_k are what is left of the extents from there.
template<typename T, bool KFAST>
__device__ __forceinline__ void chunk_load(T (&r)[Cfg<T>::BK * BT / NTHREADS], const T* __restrict__ g, long long ld, int ext_i, int ext_k, int t)
{
  typedef Cfg<T> K;
  constexpr int NL = K::BK * BT / NTHREADS;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    int i, kk;
    tile::where<K::BK, K::LI, KFAST>(t + NTHREADS * j, i, kk);
    // beyond the extents nothing is read: the address is clamped to the last element (ext_i, ext_k >= 1) and the image gets a
    // zero, which only reaches accumulators that are never stored (i) or steps that are never run (kk)
    const bool in = (i < ext_i && kk < ext_k);
    const int ic = (i < ext_i ? i : ext_i - 1), kc = (kk < ext_k ? kk : ext_k - 1);
    const size_t off = KFAST ? ((size_t)ic * (size_t)ld + (size_t)kc) : ((size_t)kc * (size_t)ld + (size_t)ic);
    const T v = g[off];
    r[j] = in ? v : (T)0;
  }
}

template<typename T, bool KFAST>
__device__ __forceinline__ void chunk_store(T* __restrict__ s, const T (&r)[Cfg<T>::BK * BT / NTHREADS], int t)
{
  typedef Cfg<T> K;
  constexpr int NL = K::BK * BT / NTHREADS;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    int i, kk;
    tile::where<K::BK, K::LI, KFAST>(t + NTHREADS * j, i, kk);
    s[kk * K::P + i] = r[j];
  }
}

// C rectangle of mr x nr elements at c, A and B pointing at the first row of op(A) / first column of op(B) the rectangle needs.
template<typename T, bool TA, bool TB>
__global__ __launch_bounds__(NTHREADS) void tgemm_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ c,
  int mr, int nr, int k, long long lda, long long ldb, long long ldc, int beta0)
{
  typedef Cfg<T> K;
  constexpr int NL = K::BK * BT / NTHREADS;
  constexpr bool AK = TA, BKF = !TB; // fast dimension k: A transposed, B not transposed
  __shared__ T As[K::BK * K::P];
  __shared__ T Bs[K::BK * K::P];
  const int t = (int)threadIdx.x;
  const int m0 = BT * (int)blockIdx.x, n0 = BT * (int)blockIdx.y;
  const int em = mr - m0, en = nr - n0; // what is left of the rectangle from this tile's origin (>= 1)
  const T* const ga = a + (TA ? (size_t)m0 * (size_t)lda : (size_t)m0);
  const T* const gb = b + (TB ? (size_t)n0 : (size_t)n0 * (size_t)ldb);
  T* const gc = c + (size_t)n0 * (size_t)ldc + (size_t)m0;

  // a wave holds its 64 x 64 quarter: fp32 2 x 2 tiles of 32 x 32, fp64 4 x 4 tiles of 16 x 16
  tile::MatrixCores<typename K::I, 64 / K::I::TS, K::BK, tile::Plain<T, K::P> > eng;
  eng.init(t);
  if (0 == beta0) eng.c_load(gc, ldc, em, en); // beta = 1: C is where the chains start (beta = 0 never reads C)

  T ra[NL], rb[NL];
  tile::k_loop<K::BK>(k,
    [&](int k0) TILE_INLINE {
      chunk_load<T, AK>(ra, ga + (TA ? (size_t)k0 : (size_t)k0 * (size_t)lda), lda, em, k - k0, t);
      chunk_load<T, BKF>(rb, gb + (TB ? (size_t)k0 * (size_t)ldb : (size_t)k0), ldb, en, k - k0, t);
    },
    [&]() TILE_INLINE { chunk_store<T, AK>(As, ra, t); chunk_store<T, BKF>(Bs, rb, t); },
    [&](int kc) TILE_INLINE { eng.chunk(As, Bs, kc); });
  eng.c_store(gc, ldc, em, en);
}

template<typename T> struct Pick {
  template<bool TA, bool TB> static auto get() { return &tgemm_kernel<T, TA, TB>; }
};

} // namespace

namespace xsmm {

int launch_tgemm(const TgemmArgs& g, void* stream, const char** name)
{
  static const char* const names[2][4] = { { "tgemm_f32_nn", "tgemm_f32_tn", "tgemm_f32_nt", "tgemm_f32_tt" },
                                           { "tgemm_f64_nn", "tgemm_f64_tn", "tgemm_f64_nt", "tgemm_f64_tt" } };
  if (nullptr != name) *name = names[8 == g.typesize ? 1 : 0][(0 != g.transa ? 1 : 0) | (0 != g.transb ? 2 : 0)];
  if (g.m < 1 || g.n < 1 || g.k < 1) return 0;
  return 8 == g.typesize ? tile::band_launch<Pick<double>, double, double>(g, stream) : tile::band_launch<Pick<float>, float, float>(g, stream);
}

} // namespace xsmm
