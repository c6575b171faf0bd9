// tgemm_lowp.hip -- the tiled GEMM for 16-bit inputs: C(m x n) = op(A) * op(B) + beta * C, beta in {0, 1}, plain
// column-major operands and all four transposes, behind libxsmm_amd_lowp_gemm and the front ends libxsmm_wigemm /
// libxsmm_wsgemm / libxsmm_bsgemm (xsmm_lowp_gemm.cpp). Four kinds:
//   LOWP_I16_I32   wrapping 32-bit sum of the 32-bit products                                        (vector ALU)
//   LOWP_I16_F32   acc = fadd(acc, (float)(a * b as int32)), k ascending                             (vector ALU)
//   LOWP_BF16      acc = fma(a, b, acc) over the widened operands, k ascending: v_mfma_f32_32x32x2_f32, which computes that
//                  chain per element (tests/test_mfma_runs_gpu.py). A bf16 x bf16 product is exact in fp32 unless it
//                  underflows, so this is the chain acc = fadd(acc, fmul(a, b)) of the bf16 SMM kernels (smm_lowp.hip).
//   LOWP_BF16_FAST v_mfma_f32_32x32x16_bf16: 16 products per step, summed in the order the instruction takes. Opt-in.
//
// The block is that of tgemm.hip: 256 threads own a 128 x 128 tile of C, k advances in chunks through LDS, the next chunk
// travels from memory into registers during the current one's arithmetic, operands are re-laid on their way into LDS, so
// the four transposes differ only in how a chunk is fetched. Elements stay 16 bits wide in LDS.
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
// The k tail. LOWP_BF16 keeps the rule of tgemm.hip: whole matrix steps only, then the last odd k by fma on the vector ALU,
// because a zero-padded step through a live accumulator, fma(0, 0, -0.0), gives +0.0. LOWP_BF16_FAST pads the last step with
// zeros (bits are not promised there): a C of -0.0 whose products are all -0.0 comes out as +0.0. The i16 kinds pad the
// last pair with a zero: the integer sum does not see it, and in the float chain the extra term is +0.0 behind at least
// one real term, none of which is -0.0 ((float) of an int), so the sum is never -0.0 when it arrives and stays as it is.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../xsmm_internal.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef unsigned short u16;

constexpr int BT = xsmm::TGEMM_TILE; // extent of the work-group tile (both ways)
constexpr int WT = 64;               // extent of a wave's part (matrix-core kinds)
constexpr int NTHREADS = 256;
constexpr int TS = 32;               // extent of a matrix-instruction tile
constexpr int LI = 4;                // rows a wave fetches side by side from an operand whose fast dimension is k
static_assert(128 == BT, "the thread maps below are written for 128 x 128");

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

// element e of a thread's share of a chunk: KFAST (the operand's fast dimension in memory is k): a wave fetches LI rows of
// 64 / LI consecutive k; otherwise 64 consecutive i of one k
template<int BK, bool KFAST> __device__ __forceinline__ void where(int e, int& i, int& kk)
{
  i = KFAST ? ((e % LI) + LI * (e / (LI * BK))) : (e % BT);
  kk = KFAST ? ((e / LI) % BK) : (e / BT);
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
    where<BK, KFAST>(t + NTHREADS * j, i, kk);
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
    where<BK, KFAST>(t + NTHREADS * j, i, kk);
    s[image<KIND>(i, kk)] = (u16)(r[j / 2] >> (16 * (j & 1)));
  }
}

__device__ __forceinline__ float widen(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ int nrow(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; } // n inside a tile: register r, lane half kl

// The arithmetic of a work-group on the matrix cores: four waves, 2 x 2, a wave holds its 64 x 64 quarter as 2 x 2 tiles of
// 32 x 32. The operands of the matrix instruction are swapped as in tgemm.hip: a lane holds one row m of C and its
// registers walk n, so that loads and stores of C run along m.
template<int KIND> struct MatrixCores {
  f32x16 acc[2][2]; // [j: along n][i: along m]
  int lm, kl, wm, wn;
  __device__ __forceinline__ void init(int t)
  {
    const int lane = t & 63, wave = t >> 6;
    lm = lane % TS; kl = lane / TS; wm = WT * (wave & 1); wn = WT * (wave >> 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
      }
    }
  }
  template<bool LOAD> __device__ __forceinline__ void c_move(float* __restrict__ gc, long long ldc, int em, int en)
  {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = wn + j * TS + nrow(r, kl);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int m = wm + i * TS + lm;
          if (LOAD) acc[j][i][r] = gc[(size_t)(n < en ? n : en - 1) * (size_t)ldc + (size_t)(m < em ? m : em - 1)]; // clamped into the tile's part
          else if (m < em && n < en) gc[(size_t)n * (size_t)ldc + (size_t)m] = acc[j][i][r];
        }
      }
    }
  }
  __device__ __forceinline__ void step2(const u16* __restrict__ As, const u16* __restrict__ Bs, int s)
  { // v_mfma_f32_32x32x2_f32: the lane half kl supplies k = 2 s + kl
    const int kk = 2 * s + kl;
    float av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { av[i] = widen(As[image<KIND>(wm + i * TS + lm, kk)]); bv[i] = widen(Bs[image<KIND>(wn + i * TS + lm, kk)]); }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[j], av[i], acc[j][i], 0, 0, 0);
    }
  }
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
    constexpr int BK = Cfg<KIND>::BK;
    if (xsmm::LOWP_BF16_FAST == KIND) {
      if (BK == kc) {
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) step16(As, Bs, s);
      }
      else { // the last step is padded with the zeros of the image
        const int steps = (kc + 15) / 16;
        for (int s = 0; s < steps; ++s) step16(As, Bs, s);
      }
    }
    else if (BK == kc) {
#pragma unroll 8
      for (int s = 0; s < BK / 2; ++s) step2(As, Bs, s);
    }
    else { // the last chunk: whole matrix steps first, then the odd k on the vector ALU (no zero-padded step: see above)
      const int steps = kc / 2;
      for (int s = 0; s < steps; ++s) step2(As, Bs, s);
      if (0 != (kc & 1)) {
        const int kk = kc - 1;
        float av[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = widen(As[image<KIND>(wm + i * TS + lm, kk)]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float bn = widen(Bs[image<KIND>(wn + j * TS + nrow(r, kl), kk)]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i][r] = __builtin_fmaf(av[i], bn, acc[j][i][r]);
          }
        }
      }
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
  template<bool LOAD> __device__ __forceinline__ void c_move(out_t* __restrict__ gc, long long ldc, int em, int en)
  {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int n = at(ty, v);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int m = at(tx, u);
        if (LOAD) acc[v][u] = (acc_t)gc[(size_t)(n < en ? n : en - 1) * (size_t)ldc + (size_t)(m < em ? m : em - 1)];
        else if (m < em && n < en) gc[(size_t)n * (size_t)ldc + (size_t)m] = (out_t)acc[v][u];
      }
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

template<int KIND> struct Engine { typedef typename std::conditional<(KIND >= xsmm::LOWP_BF16), MatrixCores<KIND>, VectorAlu<KIND> >::type type; };

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
  if (0 == beta0) eng.template c_move<true>(gc, ldc, em, en); // beta = 1: C is where the sums start (beta = 0 never reads C)

  unsigned ra[NL / 2], rb[NL / 2];
  chunk_load<K::BK, AK>(ra, ga, lda, em, k, t);
  chunk_load<K::BK, BKF>(rb, gb, ldb, en, k, t);
  for (int k0 = 0; k0 < k; k0 += K::BK) {
    __syncthreads(); // the previous chunk has been consumed
    chunk_store<KIND, AK>(As, ra, t);
    chunk_store<KIND, BKF>(Bs, rb, t);
    __syncthreads();
    if (k0 + K::BK < k) { // the next chunk travels during this chunk's arithmetic
      const int k1 = k0 + K::BK;
      chunk_load<K::BK, AK>(ra, ga + (TA ? (size_t)k1 : (size_t)k1 * (size_t)lda), lda, em, k - k1, t);
      chunk_load<K::BK, BKF>(rb, gb + (TB ? (size_t)k1 * (size_t)ldb : (size_t)k1), ldb, en, k - k1, t);
    }
    eng.chunk(As, Bs, (k - k0 < K::BK) ? (k - k0) : K::BK);
  }
  eng.template c_move<false>(gc, ldc, em, en);
}

template<int KIND>
int launch_kind(const xsmm::TgemmLowpArgs& g, void* stream)
{
  typedef typename Cfg<KIND>::out_t out_t;
  const unsigned tiles_m = (unsigned)((g.m + BT - 1) / BT);
  const hipStream_t st = (hipStream_t)stream;
  const int sel = (0 != g.transa ? 1 : 0) | (0 != g.transb ? 2 : 0);
  constexpr int BAND = 65535 * BT; // columns of C one grid covers (gridDim.y); a wider rectangle goes band by band
  for (long long n0 = 0; n0 < g.n; n0 += BAND) {
    const int nb = (int)((g.n - n0 < BAND) ? (g.n - n0) : BAND);
    const dim3 grid(tiles_m, (unsigned)((nb + BT - 1) / BT)), block(NTHREADS);
    const u16* const a = static_cast<const u16*>(g.a);
    const u16* const b = static_cast<const u16*>(g.b) + (0 != g.transb ? (size_t)n0 : (size_t)n0 * (size_t)g.ldb);
    out_t* const c = static_cast<out_t*>(g.c) + (size_t)n0 * (size_t)g.ldc;
    switch (sel) {
      case 0: hipLaunchKernelGGL((tgemm_lowp_kernel<KIND, false, false>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      case 1: hipLaunchKernelGGL((tgemm_lowp_kernel<KIND, true, false>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      case 2: hipLaunchKernelGGL((tgemm_lowp_kernel<KIND, false, true>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
      default: hipLaunchKernelGGL((tgemm_lowp_kernel<KIND, true, true>), grid, block, 0, st, a, b, c, g.m, nb, g.k, g.lda, g.ldb, g.ldc, g.beta0); break;
    }
    const int e = (int)hipGetLastError();
    if (0 != e) return e;
  }
  return 0;
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
