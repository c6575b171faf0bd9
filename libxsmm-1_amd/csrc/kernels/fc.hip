// fc.hip -- the three passes of the fully-connected layer (libxsmm_dnn_fullyconnected_execute_st, xsmm_dnn_fc.cpp,
// DESIGN.md 8g) as one kernel family: D(i, j) = chain over r = 0 .. R-1 of P(i, r) * Q(r, j), fused multiply-add in fp32,
// r ascending, started from +0.0; D is never read.
//
// Reference: src/template/libxsmm_dnn_fullyconnected_st_{fwd,bwd,upd}_{custom,ncnc_kcck}_generic.tpl.c -- one SMM or
// batch-reduce SMM call with beta = 0 per block of the output, after a transposed copy of the filter (bwd) or of the input
// (upd) into scratch. Here the operands are addressed where they lie: every tensor of both storage formats is, per index,
// a two-level strided function (x / blk) * outer + (x % blk) * inner (FcDim), and the address of an element is the sum over
// its two indices. A work-group re-lays its part on the way into LDS, so no transposed copy and no scratch exist.
//
// The tile scheme, the arithmetic of a wave and the r loop are those of tile_gemm.cuh: 256 threads (four waves, 2 x 2) own
// a BT x BT tile of D, BT = 128 (a wave holds 2 x 2 tiles of 32 x 32 in 64 accumulator registers) or BT = 64 (one tile per
// wave, 16 registers: more work-groups for layers that are small in one dimension -- R is never split, so tiles of D are
// all the parallelism there is). r advances in chunks of 32 through LDS.
//
// Loads. A thread takes BK * BT / 256 elements per operand and chunk. If the operand's fast dimension in memory is the
// tile index (i or j), the thread keeps one tile index and walks r; if it is r, the thread keeps one r and walks the tile
// index in steps of 8. The kept index is decomposed once per thread (tile index) or once per chunk (r); the walked one
// starts from one division and advances by adding the decomposed step -- no division per element. Beyond the extents the
// address falls back to the operand's first element and the LDS image gets a zero, which only reaches accumulators that
// are never stored (tile index) or steps that are never run (r).
//
// LDS image: Ps[kk][i] = P(i, kk) and Qs[kk][j] = Q(kk, j), pitch BT + 8 floats (136 or 72, both 8 mod 32). Banks (MI355X:
// ds_read_b32 / ds_write_b32 serve lanes {0-31}, {32-63} against 32 banks of 4 bytes):
//   operand read: a group is 32 consecutive floats of one kk: 32 banks.
//   write, tile index fast: 32 consecutive floats of one kk (BT = 64: lanes 0-31 and 32-63 are the halves of one kk): 32 banks.
//   write, r fast: a group is 8 tile indices x 4 kk at banks 8 kk + i: 32 banks.
// The table of the tile's output offsets (one division per column, computed by the first BT threads) is read by all lanes
// of a group at one address per register: a broadcast.
//
// The r tail (R mod 2, on the vector ALU): tile_gemm.cuh.
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::NTHREADS;
constexpr int BK = 32;   // r per chunk
constexpr int LI = 8;    // tile indices per group of loads when r is the fast dimension

struct Walk { int q, rem; }; // an index as (x / blk, x % blk)
__device__ __forceinline__ Walk walk_init(int x, int blk) { Walk w; w.q = x / blk; w.rem = x - w.q * blk; return w; }
__device__ __forceinline__ void walk_step(Walk& w, const Walk& step, int blk)
{
  w.q += step.q; w.rem += step.rem;
  if (w.rem >= blk) { w.rem -= blk; ++w.q; }
}
__device__ __forceinline__ long long walk_off(const Walk& w, const xsmm::FcDim& d) { return (long long)w.q * d.outer + (long long)w.rem * d.inner; }

template<bool BF> __device__ __forceinline__ float load_elem(const void* __restrict__ base, long long off)
{
  if (BF) return __uint_as_float((unsigned)static_cast<const unsigned short*>(base)[off] << 16);
  return static_cast<const float*>(base)[off];
}

__device__ __forceinline__ unsigned short rne_bf16(float x)
{ // libxsmm_rne_convert_fp32_bfp16: NaN and Inf are only shifted
  unsigned u = __float_as_uint(x);
  if (0x7f800000u != (u & 0x7f800000u)) u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

// What a thread keeps of one operand for the whole kernel.
template<int BT> struct Loader {
  const void* base;
  xsmm::FcDim dt, dr;   // tile dimension (i or j), r
  bool rfast;
  int t_lo, t_end;      // tile index of the thread's first element, end of the valid tile indices
  long long off_t;      // !rfast: the part of the kept tile index
  Walk wt0, step_t;     // rfast: the first tile index and the step of 8
  Walk step_r;          // !rfast: the step of NTHREADS / BT
  __device__ __forceinline__ void init(const void* b, const xsmm::FcDim& dt_, const xsmm::FcDim& dr_, bool rf, int tile0, int tend, int t)
  {
    base = b; dt = dt_; dr = dr_; rfast = rf; t_end = tend;
    t_lo = tile0 + (rf ? (t % LI) : (t % BT));
    wt0 = walk_init(t_lo < tend ? t_lo : tile0, dt.blk); // (tile0 < tend)
    off_t = walk_off(wt0, dt);
    step_t = walk_init(LI, dt.blk);
    step_r = walk_init(NTHREADS / BT, dr.blk);
  }
  template<bool BF> __device__ __forceinline__ void load(float (&r)[BK * BT / NTHREADS], int k0, int R, int t) const
  {
    constexpr int NL = BK * BT / NTHREADS;
    if (!rfast) { // element j: tile index t % BT, kk = t / BT + (NTHREADS / BT) * j
      const int r0 = k0 + t / BT;
      Walk w = walk_init(r0 < R ? r0 : k0, dr.blk);
      const bool tin = (t_lo < t_end);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const bool in = (tin && r0 + (NTHREADS / BT) * j < R);
        const long long off = in ? (off_t + walk_off(w, dr)) : 0;
        const float v = load_elem<BF>(base, off);
        r[j] = in ? v : 0.f;
        walk_step(w, step_r, dr.blk);
      }
    }
    else { // element j: tile index t % LI + LI * j, kk = t / LI
      const int rr = k0 + t / LI;
      const bool rin = (rr < R);
      const long long off_r = walk_off(walk_init(rin ? rr : k0, dr.blk), dr);
      Walk w = wt0;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const bool in = (rin && t_lo + LI * j < t_end);
        const long long off = in ? (off_r + walk_off(w, dt)) : 0;
        const float v = load_elem<BF>(base, off);
        r[j] = in ? v : 0.f;
        walk_step(w, step_t, dt.blk);
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ s, const float (&r)[BK * BT / NTHREADS], int t) const
  {
    constexpr int NL = BK * BT / NTHREADS, P = BT + 8;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = rfast ? (t % LI + LI * j) : (t % BT);
      const int kk = rfast ? (t / LI) : (t / BT + (NTHREADS / BT) * j);
      s[kk * P + i] = r[j];
    }
  }
};

template<int BT, bool PB, bool QB, bool DB>
__global__ __launch_bounds__(NTHREADS) void fc_kernel(const xsmm::FcArgs g)
{
  constexpr int P = BT + 8, NL = BK * BT / NTHREADS, TW = BT / 2 / tile::MfmaF32::TS; // tiles per side of a wave's part
  __shared__ float Ps[BK * P];
  __shared__ float Qs[BK * P];
  __shared__ long long offj[BT]; // where column j of the tile lies in D
  __shared__ int linj[BT];       // its part of the share's block number
  const int t = (int)threadIdx.x;
  const int tiles_i = (g.i1 - g.i0 + BT - 1) / BT;
  const int tj = (int)blockIdx.x / tiles_i, ti = (int)blockIdx.x - tj * tiles_i;
  const int it0 = g.i0 + BT * ti, jt0 = g.j0 + BT * tj;
  const int iend = (it0 + BT < g.i1 ? it0 + BT : g.i1), jend = (jt0 + BT < g.j1 ? jt0 + BT : g.j1);
  if (0 != g.masked) { // the block numbers of a tile lie between those of its corners: a tile outside the share has nothing to do
    const int lo = (it0 / g.sbi) * g.mi + (jt0 / g.sbj) * g.mj, hi = ((iend - 1) / g.sbi) * g.mi + ((jend - 1) / g.sbj) * g.mj;
    if (hi < g.w0 || lo >= g.w1) return;
  }
  if (t < BT) {
    const int j = (jt0 + t < jend ? jt0 + t : jt0);
    offj[t] = walk_off(walk_init(j, g.dj.blk), g.dj);
    linj[t] = (0 != g.masked ? (j / g.sbj) * g.mj : 0);
  }

  Loader<BT> lp, lq;
  lp.init(g.p, g.pi, g.pr, 0 != g.p_rfast, it0, iend, t);
  lq.init(g.q, g.qj, g.qr, 0 != g.q_rfast, jt0, jend, t);

  tile::MatrixCores<tile::MfmaF32, TW, BK, tile::Plain<float, P> > eng;
  eng.init(t);

  const int R = g.R;
  float rp[NL], rq[NL];
  tile::k_loop<BK>(R,
    [&](int k0) TILE_INLINE { lp.template load<PB>(rp, k0, R, t); lq.template load<QB>(rq, k0, R, t); },
    [&]() TILE_INLINE { lp.store(Ps, rp, t); lq.store(Qs, rq, t); },
    [&](int kc) TILE_INLINE { eng.chunk(Ps, Qs, kc); });

  // only valid elements of the share are stored (R >= 1: the barriers of the loop have published offj and linj)
  long long off_i[TW];
  int lin_i[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int ii = it0 + eng.row(i);
    off_i[i] = walk_off(walk_init(ii, g.di.blk), g.di);
    lin_i[i] = (0 != g.masked ? (ii / g.sbi) * g.mi : 0);
  }
  eng.each([&](int i, int j, int r, float v) TILE_INLINE {
    const int jl = eng.col(j, r);
    if (it0 + eng.row(i) >= iend || jt0 + jl >= jend) return;
    if (0 != g.masked) { const int lin = lin_i[i] + linj[jl]; if (lin < g.w0 || lin >= g.w1) return; }
    const long long off = off_i[i] + offj[jl];
    if (DB) static_cast<unsigned short*>(g.d)[off] = rne_bf16(v);
    else static_cast<float*>(g.d)[off] = v;
  });
}

template<int BT, bool PB, bool QB, bool DB>
int launch_one(const xsmm::FcArgs& g, void* stream)
{
  const long long tiles = (long long)((g.i1 - g.i0 + BT - 1) / BT) * ((g.j1 - g.j0 + BT - 1) / BT);
  if (tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((fc_kernel<BT, PB, QB, DB>), dim3((unsigned)tiles), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

} // namespace

namespace xsmm {

int launch_fc(const FcArgs& g, void* stream, const char** name)
{
  // the combinations the layer has: f32 (all passes), bf16 fwd (both inputs 16-bit, f32 out), bf16 bwd (filter 16-bit, dy f32,
  // dx 16-bit) and bf16 upd (dy f32, input 16-bit, dw 16-bit)
  static const char* const names[4][2] = { { "fc_f32_t64", "fc_f32_t128" }, { "fc_bf16_fwd_t64", "fc_bf16_fwd_t128" },
                                           { "fc_bf16_bwd_t64", "fc_bf16_bwd_t128" }, { "fc_bf16_upd_t64", "fc_bf16_upd_t128" } };
  const int pb = (0 != g.p_bf16), qb = (0 != g.q_bf16), db = (0 != g.d_bf16);
  int sel = -1;
  if (!pb && !qb && !db) sel = 0;
  else if (pb && qb && !db) sel = 1;
  else if (pb && !qb && db) sel = 2;
  else if (!pb && qb && db) sel = 3;
  if (sel < 0 || (64 != g.tile && 128 != g.tile)) return (int)hipErrorInvalidValue;
  const int big = (128 == g.tile ? 1 : 0);
  if (nullptr != name) *name = names[sel][big];
  if (g.i1 <= g.i0 || g.j1 <= g.j0 || g.R < 1) return 0;
  switch (2 * sel + big) {
    case 0: return launch_one<64, false, false, false>(g, stream);
    case 1: return launch_one<128, false, false, false>(g, stream);
    case 2: return launch_one<64, true, true, false>(g, stream);
    case 3: return launch_one<128, true, true, false>(g, stream);
    case 4: return launch_one<64, true, false, true>(g, stream);
    case 5: return launch_one<128, true, false, true>(g, stream);
    case 6: return launch_one<64, false, true, true>(g, stream);
    default: return launch_one<128, false, true, true>(g, stream);
  }
}

} // namespace xsmm
