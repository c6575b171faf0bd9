// tgemm_lowp.hip -- the tiled GEMM for 16-bit inputs: C(m x n) = op(A) * op(B) + beta * C, beta in {0, 1}, plain
// column-major operands and all four transposes, behind libxsmm_amd_lowp_gemm and the front ends libxsmm_wigemm /
// libxsmm_wsgemm / libxsmm_bsgemm (xsmm_lowp_gemm.cpp). Four kinds:
//   LOWP_I16_I32   wrapping 32-bit sum of the 32-bit products                                        (vector ALU)
//   LOWP_I16_F32   acc = fadd(acc, (float)(a * b as int32)), k ascending                             (vector ALU)
//   LOWP_BF16      acc = fma(a, b, acc) over the widened operands, k ascending: v_mfma_f32_32x32x2_f32, which computes that
//                  chain per element (tests/test_mfma_runs_gpu.py). A bf16 x bf16 product is exact in fp32 unless it is
//                  subnormal or beyond FLT_MAX, so this is the chain acc = fadd(acc, fmul(a, b)) of the bf16 SMM kernels
//                  (smm_lowp.hip) everywhere else; where a chain meets such a product it keeps the fma's bits (pinned by
//                  tests/test_hostile_operands_gpu.py::test_values_tgemm_bf16).
//   LOWP_BF16_FAST v_mfma_f32_32x32x16_bf16: 16 products per step, summed in the order the instruction takes. Opt-in.
//
// The block, the k loop and the arithmetic of LOWP_BF16 are those of tile_gemm.cuh: 256 threads own a 128 x 128 tile of C,
// operands are re-laid on their way into LDS, so the four transposes differ only in how a chunk is fetched. Elements stay
// 16 bits wide in LDS.
//
// LDS images (u16 index of element (i, kk) of a chunk; i: row of op(A) / column of op(B), kk: k inside the chunk), and the
// banks they meet (MI355X: ds_read_u16 / ds_write_b16 / ds_read_b32 serve lanes {0-31}, {32-63} against 32 banks of 4
// bytes -- 64 for ds_read_b64 and ds_read_b128 --, ds_read_b128 four groups of 16 lanes; two lanes on the halves of one
// word read one address):
//   LOWP_BF16, BK = 64: kk * 136 + i (68 words per kk).  Fragment read (ds_read_u16, widened by a 16-bit shift): a group is
//     32 consecutive i of one kk: 16 words, 16 banks, two lanes per word. Write along i: the same. Write along k (a group is
//     4 i x 8 kk): word 68 kk + i / 2, banks 4 kk + {0, 1}: 16 banks, two lanes per word.
//   LOWP_BF16_FAST, BK = 64: i * 72 + kk (144 bytes per i, k-fast: a lane's fragment is 8 consecutive k, 16 bytes).
//     Fragment read (ds_read_b128 at 144 i + 32 s + 16 h): a group holds 16 rows that differ mod 16, all with one h; the
//     16-byte slot is (9 i + h + 2 s) mod 16 and 9 is odd: 16 slots, all 64 banks, no conflict. Write along k (4 i x 8 kk):
//     word 36 i + kk / 2, banks 4 i + {0 ... 3}: 16 banks. Write along i (operands whose memory is i-fast, A 'N' and B 'T',
//     are transposed here): 32 i of one kk, banks 4 i mod 32: 8 banks, 4 lanes each -- the price of the transposing fill.
//   i16, BK = 32: 32-bit k pairs as in smm_lowp.hip, (kk / 2) * 272 + 2 i + (kk & 1) (136 words per pair).  Operand read
//     (ds_read_b128: 4 consecutive i of a pair, at most 16 different addresses per wave): no conflict. Write along i: 32
//     words, 32 banks. Write along k (4 i x 8 kk): word 136 (kk / 2) + i, banks 8 (kk / 2) + i: 16 banks, two lanes per word.
//
// The k tail. LOWP_BF16 keeps the rule of tile_gemm.cuh: the last odd k goes to the vector ALU. LOWP_BF16_FAST pads the last
// step with zeros (bits are not promised there): a C of -0.0 whose products are all -0.0 comes out as +0.0. The i16 kinds pad the
// last pair with a zero: the integer sum does not see it, and in the float chain the extra term is +0.0 behind at least
// one real term, none of which is -0.0 ((float) of an int), so the sum is never -0.0 when it arrives and stays as it is.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../xsmm_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::BT;
using tile::NTHREADS;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef unsigned short u16;

constexpr int LI = 4; // rows a wave fetches side by side from an operand whose fast dimension is k

template<int KIND> struct Cfg;
template<> struct Cfg<xsmm::LOWP_I16_I32> { typedef int out_t; static constexpr int BK = 32, LDS = (BK / 2) * 2 * (BT + 8); };
template<> struct Cfg<xsmm::LOWP_I16_F32> { typedef float out_t; static constexpr int BK = 32, LDS = (BK / 2) * 2 * (BT + 8); };
template<> struct Cfg<xsmm::LOWP_BF16> { typedef float out_t; static constexpr int BK = xsmm::TGEMM_LOWP_BK, LDS = BK * (BT + 8); };
template<> struct Cfg<xsmm::LOWP_BF16_FAST> { typedef float out_t; static constexpr int BK = xsmm::TGEMM_LOWP_BK, LDS = BT * (BK + 8); };

template<int KIND> __device__ __forceinline__ int image(int i, int kk)
{
  if (xsmm::LOWP_BF16 == KIND) return kk * (BT + 8) + i;
  if (xsmm::LOWP_BF16_FAST == KIND) return i * (Cfg<KIND>::BK + 8) + kk;
  return (kk >> 1) * (2 * (BT + 8)) + 2 * i + (kk & 1);
}

// One chunk of an operand: BK x BT elements, NL per thread. g points at element (i = 0, k = 0) of the work-group's part;
// ext_i and ext_k are what is left of the extents from there.
template<int BK, bool KFAST>
__device__ __forceinline__ void chunk_load(unsigned (&r)[BK * BT / NTHREADS / 2], const u16* __restrict__ g, long long ld, int ext_i, int ext_k, int t)
{
  constexpr int NL = BK * BT / NTHREADS;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    int i, kk;
    tile::where<BK, LI, KFAST>(t + NTHREADS * j, i, kk);
    // beyond the extents nothing is read: the address is clamped to the last element (ext_i, ext_k >= 1) and the image gets a
    // zero, which reaches accumulators that are never stored (i), steps that are never run or steps that are padded (kk)
    const bool in = (i < ext_i && kk < ext_k);
    const int ic = (i < ext_i ? i : ext_i - 1), kc = (kk < ext_k ? kk : ext_k - 1);
    const size_t off = KFAST ? ((size_t)ic * (size_t)ld + (size_t)kc) : ((size_t)kc * (size_t)ld + (size_t)ic);
    const unsigned v = in ? (unsigned)g[off] : 0u; // two elements per register
    r[j / 2] = (0 == (j & 1)) ? v : (r[j / 2] | (v << 16));
  }
}

template<int KIND, bool KFAST>
__device__ __forceinline__ void chunk_store(u16* __restrict__ s, const unsigned (&r)[Cfg<KIND>::BK * BT / NTHREADS / 2], int t)
{
  constexpr int BK = Cfg<KIND>::BK, NL = BK * BT / NTHREADS;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    int i, kk;
    tile::where<BK, LI, KFAST>(t + NTHREADS * j, i, kk);
    s[image<KIND>(i, kk)] = (u16)(r[j / 2] >> (16 * (j & 1)));
  }
}

// LOWP_BF16: the engine of tile_gemm.cuh, 2 x 2 tiles of v_mfma_f32_32x32x2_f32 per wave, over 16-bit fragments widened by
// a shift; the loop over a full chunk of 32 steps is unrolled by 8
template<int KIND> struct Widened {
  static __device__ __forceinline__ float at(const u16* __restrict__ s, int i, int kk) { return __uint_as_float((unsigned)s[image<KIND>(i, kk)] << 16); }
};
template<int KIND> using MatrixCores = tile::MatrixCores<tile::MfmaF32, 2, Cfg<KIND>::BK, Widened<KIND>, 8>;

// LOWP_BF16_FAST: the same accumulators and C movement, its own steps
struct MatrixCoresFast : MatrixCores<xsmm::LOWP_BF16_FAST> {
  static constexpr int KIND = xsmm::LOWP_BF16_FAST, BK = Cfg<KIND>::BK;
  __device__ __forceinline__ void step16(const u16* __restrict__ As, const u16* __restrict__ Bs, int s)
  { // v_mfma_f32_32x32x16_bf16: the lane half kl supplies k = 16 s + 8 kl ... + 7, 16 bytes of the k-fast image
    bf16x8 av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      av[i] = *reinterpret_cast<const bf16x8*>(As + image<KIND>(wm + i * TS + lm, 16 * s + 8 * kl));
      bv[i] = *reinterpret_cast<const bf16x8*>(Bs + image<KIND>(wn + i * TS + lm, 16 * s + 8 * kl));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bv[j], av[i], acc[j][i], 0, 0, 0);
    }
  }
  __device__ __forceinline__ void chunk(const u16* __restrict__ As, const u16* __restrict__ Bs, int kc)
  {
    if (BK == kc) {
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) step16(As, Bs, s);
    }
    else { // the last step is padded with the zeros of the image
      const int steps = (kc + 15) / 16;
      for (int s = 0; s < steps; ++s) step16(As, Bs, s);
    }
  }
};

// The arithmetic of a work-group on the vector ALU (there is no i16 matrix instruction): thread (tx, ty) of 16 x 16 holds
// 8 x 8 elements of C, rows 4 tx ... + 3 and 64 + 4 tx ... + 3, columns 4 ty ... + 3 and 64 + 4 ty ... + 3. A k pair of
// four consecutive rows is one ds_read_b128.
template<int KIND> struct VectorAlu {
  typedef typename Cfg<KIND>::out_t out_t;
  typedef typename std::conditional<xsmm::LOWP_I16_I32 == KIND, unsigned, float>::type acc_t; // (the integer sum wraps: unsigned arithmetic)
  acc_t acc[8][8]; // [along n][along m]
  int tx, ty;
  static __device__ __forceinline__ int at(int base, int u) { return 4 * base + (u & 3) + 64 * (u >> 2); }
  __device__ __forceinline__ void init(int t)
  {
    tx = t & 15; ty = t >> 4;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[v][u] = 0;
    }
  }
  __device__ __forceinline__ void c_load(const out_t* __restrict__ gc, long long ldc, int em, int en)
  {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[v][u] = tile::c_get<acc_t>(gc, ldc, em, en, at(tx, u), at(ty, v));
    }
  }
  __device__ __forceinline__ void c_store(out_t* __restrict__ gc, long long ldc, int em, int en) const
  {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
      for (int u = 0; u < 8; ++u) tile::c_put(gc, ldc, em, en, at(tx, u), at(ty, v), acc[v][u]);
    }
  }
  __device__ __forceinline__ void chunk(const u16* __restrict__ As, const u16* __restrict__ Bs, int kc)
  {
    const int pairs = (kc + 1) / 2; // an odd k: the upper half of the last pair is the zero of the image
    const uint4* const pa = reinterpret_cast<const uint4*>(As) + tx;
    const uint4* const pb = reinterpret_cast<const uint4*>(Bs) + ty;
    constexpr int PQ = (BT + 8) / 4; // uint4 per pair
#pragma unroll 2
    for (int p = 0; p < pairs; ++p) {
      const uint4 a0 = pa[p * PQ], a1 = pa[p * PQ + 16], b0 = pb[p * PQ], b1 = pb[p * PQ + 16];
      const unsigned av[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
      const unsigned bv[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int bl = (int)(short)(bv[v] & 0xFFFFu), bh = (int)bv[v] >> 16;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p0 = (int)(short)(av[u] & 0xFFFFu) * bl, p1 = ((int)av[u] >> 16) * bh;
          if (xsmm::LOWP_I16_I32 == KIND) acc[v][u] += (acc_t)((unsigned)p0 + (unsigned)p1);
          else { acc[v][u] = (acc_t)__fadd_rn((float)acc[v][u], (float)p0); acc[v][u] = (acc_t)__fadd_rn((float)acc[v][u], (float)p1); }
        }
      }
    }
  }
};

template<int KIND> struct Engine { typedef VectorAlu<KIND> type; };
template<> struct Engine<xsmm::LOWP_BF16> { typedef MatrixCores<xsmm::LOWP_BF16> type; };
template<> struct Engine<xsmm::LOWP_BF16_FAST> { typedef MatrixCoresFast type; };

// C rectangle of mr x nr elements at c, A and B pointing at the first row of op(A) / first column of op(B) the rectangle needs.
template<int KIND, bool TA, bool TB>
__global__ __launch_bounds__(NTHREADS) void tgemm_lowp_kernel(const u16* __restrict__ a, const u16* __restrict__ b, typename Cfg<KIND>::out_t* __restrict__ c,
  int mr, int nr, int k, long long lda, long long ldb, long long ldc, int beta0)
{
  typedef Cfg<KIND> K;
  constexpr int NL = K::BK * BT / NTHREADS;
  constexpr bool AK = TA, BKF = !TB; // fast dimension k: A transposed, B not transposed
  __shared__ __align__(16) u16 As[K::LDS];
  __shared__ __align__(16) u16 Bs[K::LDS];
  const int t = (int)threadIdx.x;
  const int m0 = BT * (int)blockIdx.x, n0 = BT * (int)blockIdx.y;
  const int em = mr - m0, en = nr - n0; // what is left of the rectangle from this tile's origin (>= 1)
  const u16* const ga = a + (TA ? (size_t)m0 * (size_t)lda : (size_t)m0);
  const u16* const gb = b + (TB ? (size_t)n0 : (size_t)n0 * (size_t)ldb);
  typename K::out_t* const gc = c + (size_t)n0 * (size_t)ldc + (size_t)m0;

  typename Engine<KIND>::type eng;
  eng.init(t);
  if (0 == beta0) eng.c_load(gc, ldc, em, en); // beta = 1: C is where the sums start (beta = 0 never reads C)

  unsigned ra[NL / 2], rb[NL / 2];
  tile::k_loop<K::BK>(k,
    [&](int k0) TILE_INLINE {
      chunk_load<K::BK, AK>(ra, ga + (TA ? (size_t)k0 : (size_t)k0 * (size_t)lda), lda, em, k - k0, t);
      chunk_load<K::BK, BKF>(rb, gb + (TB ? (size_t)k0 * (size_t)ldb : (size_t)k0), ldb, en, k - k0, t);
    },
    [&]() TILE_INLINE { chunk_store<KIND, AK>(As, ra, t); chunk_store<KIND, BKF>(Bs, rb, t); },
    [&](int kc) TILE_INLINE { eng.chunk(As, Bs, kc); });
  eng.c_store(gc, ldc, em, en);
}

template<int KIND> struct Pick {
  template<bool TA, bool TB> static auto get() { return &tgemm_lowp_kernel<KIND, TA, TB>; }
};
template<int KIND> int launch_kind(const xsmm::TgemmLowpArgs& g, void* stream)
{
  return tile::band_launch<Pick<KIND>, u16, typename Cfg<KIND>::out_t>(g, stream);
}

} // namespace

namespace xsmm {

int launch_tgemm_lowp(const TgemmLowpArgs& g, void* stream, const char** name)
{
  static const char* const names[4][4] = { { "tgemm_i16i32_nn", "tgemm_i16i32_tn", "tgemm_i16i32_nt", "tgemm_i16i32_tt" },
                                           { "tgemm_i16f32_nn", "tgemm_i16f32_tn", "tgemm_i16f32_nt", "tgemm_i16f32_tt" },
                                           { "tgemm_bf16_nn", "tgemm_bf16_tn", "tgemm_bf16_nt", "tgemm_bf16_tt" },
                                           { "tgemm_bf16fast_nn", "tgemm_bf16fast_tn", "tgemm_bf16fast_nt", "tgemm_bf16fast_tt" } };
  if (g.kind < LOWP_I16_I32 || g.kind > LOWP_BF16_FAST) return (int)hipErrorInvalidValue;
  if (nullptr != name) *name = names[g.kind][(0 != g.transa ? 1 : 0) | (0 != g.transb ? 2 : 0)];
  if (g.m < 1 || g.n < 1 || g.k < 1) return 0;
  switch (g.kind) {
    case LOWP_I16_I32: return launch_kind<LOWP_I16_I32>(g, stream);
    case LOWP_I16_F32: return launch_kind<LOWP_I16_F32>(g, stream);
    case LOWP_BF16: return launch_kind<LOWP_BF16>(g, stream);
    default: return launch_kind<LOWP_BF16_FAST>(g, stream);
  }
}

} // namespace xsmm
