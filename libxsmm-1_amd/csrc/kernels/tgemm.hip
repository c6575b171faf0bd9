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
// The operands of the matrix instruction are swapped (the "A" operand comes from Bs): a lane then holds one row index m
// of C and its registers walk n, so that loads and stores of C run along m, the fast dimension, 128 bytes per group.
//
// The k tail: what is left after the last whole matrix instruction (k mod 2 for fp32, k mod 4 for fp64) is finished with
// fma on the vector ALU, accumulator element by element. A zero-padded matrix step would not do: fma(0, 0, -0.0) is +0.0.
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int BT = xsmm::TGEMM_TILE; // extent of the work-group tile (both ways)
constexpr int WT = 64;               // extent of a wave's part
constexpr int NTHREADS = 256;
static_assert(128 == BT, "the thread maps below are written for 128 x 128");

template<typename T> struct Cfg;
template<> struct Cfg<float> {
  typedef f32x16 acc_t;
  static constexpr int BK = 32, DEPTH = 2, TS = 32, NR = 16, P = BT + 8, LI = 8;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int nrow(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; } // n inside a tile: register r, lane half kl
  static __device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
};
template<> struct Cfg<double> {
  typedef f64x4 acc_t;
  static constexpr int BK = 16, DEPTH = 4, TS = 16, NR = 4, P = BT + 16, LI = 16;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int nrow(int r, int kl) { return kl + 4 * r; }
  static __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
};

// One chunk of an operand: BK x BT elements, NL per thread. KFAST: the operand's fast dimension in memory is k.
// g points at element (i = 0, k = 0) of the work-group's part; ext_i and ext_k are what is left of the extents from there.
template<typename T, bool KFAST>
__device__ __forceinline__ void chunk_load(T (&r)[Cfg<T>::BK * BT / NTHREADS], const T* __restrict__ g, long long ld, int ext_i, int ext_k, int t)
{
  typedef Cfg<T> K;
  constexpr int NL = K::BK * BT / NTHREADS;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int e = t + NTHREADS * j;
    const int i = KFAST ? ((e % K::LI) + K::LI * (e / (K::LI * K::BK))) : (e % BT);
    const int kk = KFAST ? ((e / K::LI) % K::BK) : (e / BT);
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
    const int e = t + NTHREADS * j;
    const int i = KFAST ? ((e % K::LI) + K::LI * (e / (K::LI * K::BK))) : (e % BT);
    const int kk = KFAST ? ((e / K::LI) % K::BK) : (e / BT);
    s[kk * K::P + i] = r[j];
  }
}

// C rectangle of mr x nr elements at c, A and B pointing at the first row of op(A) / first column of op(B) the rectangle needs.
template<typename T, bool TA, bool TB>
__global__ __launch_bounds__(NTHREADS) void tgemm_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ c,
  int mr, int nr, int k, long long lda, long long ldb, long long ldc, int beta0)
{
  typedef Cfg<T> K;
  typedef typename K::acc_t acc_t;
  constexpr int TW = WT / K::TS;                   // tiles per side of a wave's part
  constexpr int NL = K::BK * BT / NTHREADS;
  constexpr bool AK = TA, BKF = !TB;               // fast dimension k: A transposed, B not transposed
  __shared__ T As[K::BK * K::P];
  __shared__ T Bs[K::BK * K::P];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lm = lane % K::TS, kl = lane / K::TS;  // the lane's row inside a tile; its k inside a matrix step
  const int wm = WT * (wave & 1), wn = WT * (wave >> 1);
  {
    const int m0 = BT * (int)blockIdx.x, n0 = BT * (int)blockIdx.y;
    const int em = mr - m0, en = nr - n0;          // what is left of the rectangle from this tile's origin (>= 1)
    const T* const ga = a + (TA ? (size_t)m0 * (size_t)lda : (size_t)m0);
    const T* const gb = b + (TB ? (size_t)n0 : (size_t)n0 * (size_t)ldb);
    T* const gc = c + (size_t)n0 * (size_t)ldc + (size_t)m0;

    acc_t acc[TW][TW]; // [j: along n][i: along m]
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int i = 0; i < TW; ++i) {
#pragma unroll
        for (int r = 0; r < K::NR; ++r) acc[j][i][r] = (T)0;
      }
    }

    if (0 == beta0) { // beta = 1: C is where the chains start (beta = 0 never reads C); addresses clamped into the tile's part
#pragma unroll
      for (int j = 0; j < TW; ++j) {
#pragma unroll
        for (int r = 0; r < K::NR; ++r) {
          const int n = wn + j * K::TS + K::nrow(r, kl);
          const T* const col = gc + (size_t)(n < en ? n : en - 1) * (size_t)ldc;
#pragma unroll
          for (int i = 0; i < TW; ++i) {
            const int m = wm + i * K::TS + lm;
            acc[j][i][r] = col[m < em ? m : em - 1];
          }
        }
      }
    }

    T ra[NL], rb[NL];
    chunk_load<T, AK>(ra, ga, lda, em, k, t);
    chunk_load<T, BKF>(rb, gb, ldb, en, k, t);
    for (int k0 = 0; k0 < k; k0 += K::BK) {
      __syncthreads(); // the previous chunk has been consumed
      chunk_store<T, AK>(As, ra, t);
      chunk_store<T, BKF>(Bs, rb, t);
      __syncthreads();
      if (k0 + K::BK < k) { // the next chunk travels during this chunk's matrix instructions
        const int k1 = k0 + K::BK;
        chunk_load<T, AK>(ra, ga + (TA ? (size_t)k1 : (size_t)k1 * (size_t)lda), lda, em, k - k1, t);
        chunk_load<T, BKF>(rb, gb + (TB ? (size_t)k1 * (size_t)ldb : (size_t)k1), ldb, en, k - k1, t);
      }
      const int kc = (k - k0 < K::BK) ? (k - k0) : K::BK;
      if (K::BK == kc) {
#pragma unroll
        for (int s = 0; s < K::BK / K::DEPTH; ++s) {
          const int kk = s * K::DEPTH + kl;
          T av[TW], bv[TW];
#pragma unroll
          for (int i = 0; i < TW; ++i) { av[i] = As[kk * K::P + wm + i * K::TS + lm]; bv[i] = Bs[kk * K::P + wn + i * K::TS + lm]; }
#pragma unroll
          for (int j = 0; j < TW; ++j) {
#pragma unroll
            for (int i = 0; i < TW; ++i) acc[j][i] = K::mma(bv[j], av[i], acc[j][i]);
          }
        }
      }
      else { // the last chunk: whole matrix steps first, then the tail on the vector ALU (no zero-padded step: see above)
        const int steps = kc / K::DEPTH;
        for (int s = 0; s < steps; ++s) {
          const int kk = s * K::DEPTH + kl;
          T av[TW], bv[TW];
#pragma unroll
          for (int i = 0; i < TW; ++i) { av[i] = As[kk * K::P + wm + i * K::TS + lm]; bv[i] = Bs[kk * K::P + wn + i * K::TS + lm]; }
#pragma unroll
          for (int j = 0; j < TW; ++j) {
#pragma unroll
            for (int i = 0; i < TW; ++i) acc[j][i] = K::mma(bv[j], av[i], acc[j][i]);
          }
        }
        for (int kk = steps * K::DEPTH; kk < kc; ++kk) {
          T av[TW];
#pragma unroll
          for (int i = 0; i < TW; ++i) av[i] = As[kk * K::P + wm + i * K::TS + lm];
#pragma unroll
          for (int j = 0; j < TW; ++j) {
#pragma unroll
            for (int r = 0; r < K::NR; ++r) {
              const T bn = Bs[kk * K::P + wn + j * K::TS + K::nrow(r, kl)];
#pragma unroll
              for (int i = 0; i < TW; ++i) acc[j][i][r] = K::fma_(av[i], bn, acc[j][i][r]);
            }
          }
        }
      }
    }

#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int i = 0; i < TW; ++i) {
#pragma unroll
        for (int r = 0; r < K::NR; ++r) {
          const int m = wm + i * K::TS + lm, n = wn + j * K::TS + K::nrow(r, kl);
          if (m < em && n < en) gc[(size_t)n * (size_t)ldc + (size_t)m] = acc[j][i][r];
        }
      }
    }
  }
}

template<typename T>
int launch_typed(const xsmm::TgemmArgs& g, void* stream)
{
  const unsigned tiles_m = (unsigned)((g.m + BT - 1) / BT);
  const hipStream_t st = (hipStream_t)stream;
  const int sel = (0 != g.transa ? 1 : 0) | (0 != g.transb ? 2 : 0);
  constexpr int BAND = 65535 * BT; // columns of C one grid covers (gridDim.y); a wider rectangle goes band by band
  for (long long n0 = 0; n0 < g.n; n0 += BAND) {
    const int nb = (int)((g.n - n0 < BAND) ? (g.n - n0) : BAND);
    const dim3 grid(tiles_m, (unsigned)((nb + BT - 1) / BT)), block(NTHREADS);
    const T* const a = static_cast<const T*>(g.a);
    const T* const b = static_cast<const T*>(g.b) + (0 != g.transb ? (size_t)n0 : (size_t)n0 * (size_t)g.ldb);
    T* const c = static_cast<T*>(g.c) + (size_t)n0 * (size_t)g.ldc;
    switch (sel) {
      case 0: hipLaunchKernelGGL((tgemm_kernel<T, false, false>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      case 1: hipLaunchKernelGGL((tgemm_kernel<T, true, false>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      case 2: hipLaunchKernelGGL((tgemm_kernel<T, false, true>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      default: hipLaunchKernelGGL((tgemm_kernel<T, true, true>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
    }
    const int e = (int)hipGetLastError();
    if (0 != e) return e;
  }
  return 0;
}

} // namespace

namespace xsmm {

int launch_tgemm(const TgemmArgs& g, void* stream, const char** name)
{
  static const char* const names[2][4] = { { "tgemm_f32_nn", "tgemm_f32_tn", "tgemm_f32_nt", "tgemm_f32_tt" },
                                           { "tgemm_f64_nn", "tgemm_f64_tn", "tgemm_f64_nt", "tgemm_f64_tt" } };
  if (nullptr != name) *name = names[8 == g.typesize ? 1 : 0][(0 != g.transa ? 1 : 0) | (0 != g.transb ? 2 : 0)];
  if (g.m < 1 || g.n < 1 || g.k < 1) return 0;
  return 8 == g.typesize ? launch_typed<double>(g, stream) : launch_typed<float>(g, stream);
}

} // namespace xsmm
