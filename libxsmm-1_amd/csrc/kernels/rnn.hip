// rnn.hip -- the forward pass of the RNN cell layer (libxsmm_dnn_rnncell_execute_st, xsmm_dnn_rnn.cpp) in fp32 on
// the plain tensors: activations [step][row][C or K], filters [C or K][G * K] with the gate columns side by side.
//
// The contract (the reference's generic templates, src/template/libxsmm_dnn_rnncell_st_{rnn,lstm,gru}_fwd_nc_ck_generic.tpl.c, which
// are calls of SMM and batch-reduce SMM kernels followed by the loops of src/libxsmm_dnn_elementwise.c): every pre-activation
// (row n, output k) of a gate is one chain acc = fma(w or r, x or h, acc), started from the bias, over the segments of the
// reduction in the order the host lists them (RnnArgs::seg), inside a segment with the reduction index ascending; then the
// elementwise steps of the cell, each operation rounded on its own.
//
// One kernel family serves every launch of the layer. A work-group of 256 threads owns a 64 x 64 tile of (k, n) -- one 32 x 32 tile of
// the matrix instruction per wave and gate; a minibatch rarely has more than 64 rows -- and computes ALL G gates of that tile, one
// accumulator set (tile_gemm.cuh: MatrixCores on v_mfma_f32_32x32x2_f32) per gate: the epilogue has every gate of an element in one
// thread and stores all per-step tensors, with no second pass over memory. The reduction advances in chunks of BK through LDS; what is
// left of an odd segment ends on the vector ALU (tile_gemm.cuh: the k tail), never in a zero-padded matrix step, and the next segment
// continues the same accumulators. blockIdx.z is a step: the launch that computes bias + w.x for all steps at once (the split plan)
// uses it, the step launches have one.
//
// Loads. Of w or r a thread keeps one column (k, the fast dimension in memory: a wave reads 64 consecutive floats of one row) and
// walks the rows of the chunk; of x or h it keeps one reduction index and walks the tile's rows n in steps of LI = 8, so that the 32
// threads that share a row read a run of 32 consecutive floats. Beyond the extents the address falls back to element 0 and the LDS
// image gets +0.0, which only reaches accumulators that are never stored or steps that never run.
// LDS images: Ws[g][kk][k] and Xs[kk][n], pitch BT + 8 = 72 floats (8 mod 32), as in fc.hip and conv.hip: operand reads are 32
// consecutive floats of one kk (32 banks); writes of w are 32 consecutive floats of one kk; writes of x are 8 rows x 4 values of kk
// at banks 8 kk + n (32 banks). Five images (four gates and x) are 46080 bytes.
//
// Bounds. Every address is formed from indices compared against K, the share's rows [n0, n1) and the segment's length first;
// stores are guarded by the same comparisons. Offsets are 64-bit; every tensor has fewer than 2^31 elements (checked by the host).
//
// Elementwise arithmetic. exp and tanh are evaluated in double precision and converted once, as the reference's (float)exp((double)
// -v) and (float)tanh((double)v); 1.0f + e and 1.0f / s are fp32 operations (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt makes the divide the correctly rounded one: the v_div_scale / v_div_fmas / v_div_fixup
// sequence, which tests/test_rnn_cpu.py looks for in the assembly). The whole file is compiled with contraction off, so a * b + c
// below is a multiply and an add: that is what the reference's captured outputs say about its `dst += src0 * src1` loops.
#include <hip/hip_runtime.h>

#include "../xsmm_dnn_internal.hpp"
#include "tile_gemm.cuh"

#pragma clang fp contract(off)

namespace {

using tile::NTHREADS;
using xsmm::RnnArgs;

__device__ __forceinline__ float sigmoid_(float v)
{
  const float e = (float)exp((double)-v);
  return 1.0f / (1.0f + e);
}
__device__ __forceinline__ float tanh_(float v) { return (float)tanh((double)v); }

constexpr int BT = 64;            // extent of the work-group tile, both ways
constexpr int BK = 32;            // rows of w or r per chunk
constexpr int LI = NTHREADS / BK; // rows n per group of loads of x
constexpr int P = BT + 8, NL = BK * BT / NTHREADS, TW = BT / 2 / tile::MfmaF32::TS;

template<int G>
__global__ __launch_bounds__(NTHREADS) void rnn_step(const RnnArgs g)
{
  constexpr int NR = tile::MfmaF32::NR;
  __shared__ float Ws[G][BK * P];
  __shared__ float Xs[BK * P];
  const int t = (int)threadIdx.x;
  const int it0 = BT * (int)blockIdx.x, jt0 = g.n0 + BT * (int)blockIdx.y;
  if (it0 >= g.K || jt0 >= g.n1) return;
  const int iend = (it0 + BT < g.K ? it0 + BT : g.K), jend = (jt0 + BT < g.n1 ? jt0 + BT : g.n1);
  const long long zx = (long long)blockIdx.z * g.zx, zo = (long long)blockIdx.z * g.zo;

  tile::MatrixCores<tile::MfmaF32, TW, BK, tile::Plain<float, P> > eng[G];
#pragma unroll
  for (int s = 0; s < G; ++s) eng[s].init(t);

  // the tile as the accumulators see it: output k along the rows of the matrix instruction, row n of the minibatch along its columns
  const auto stored = [&](int i, int j, int r) TILE_INLINE { return it0 + eng[0].row(i) < iend && jt0 + eng[0].col(j, r) < jend; };
  const auto offset = [&](int i, int j, int r) TILE_INLINE { return (long long)(jt0 + eng[0].col(j, r)) * g.K + it0 + eng[0].row(i); };

  // the start of the chains: the bias, or what an earlier launch left
#pragma unroll
  for (int s = 0; s < G; ++s) {
    if (0 != g.from_bias) {
#pragma unroll
      for (int i = 0; i < TW; ++i) {
        const int k = it0 + eng[s].row(i);
        float v = (k < iend) ? g.b[g.gcol[s] + k] : 0.f;
        if (s == g.fgate) v = v + g.forget_bias; // one rounded add, before the first product
#pragma unroll
        for (int j = 0; j < TW; ++j) {
#pragma unroll
          for (int r = 0; r < NR; ++r) eng[s].acc[j][i][r] = v;
        }
      }
    }
    else {
      const float* __restrict__ const src = g.pre[s] + zo;
#pragma unroll
      for (int j = 0; j < TW; ++j) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
#pragma unroll
          for (int i = 0; i < TW; ++i) {
            const bool in = stored(i, j, r);
            const float v = src[in ? offset(i, j, r) : 0];
            eng[s].acc[j][i][r] = in ? v : 0.f;
          }
        }
      }
    }
  }

  const int wi = it0 + t % BT; // the thread's column of w / r
  const bool win = (wi < iend);
  float rw[G][NL], rx[NL];
  for (int sg = 0; sg < g.nseg; ++sg) {
    const bool recur = (0 != g.seg[sg].which);
    const float* __restrict__ const a = recur ? g.r : g.w;
    const float* __restrict__ const bsrc = recur ? g.hsrc : g.x + zx;
    const int ldb = recur ? g.K : g.C, start = g.seg[sg].start, len = g.seg[sg].len;
    tile::k_loop<BK>(len,
      [&](int k0) TILE_INLINE {
        { // w / r: element e: column t % BT, kk = t / BT + (NTHREADS / BT) * e
          const int r0 = k0 + t / BT;
#pragma unroll
          for (int e = 0; e < NL; ++e) {
            const int rr = r0 + (NTHREADS / BT) * e;
            const bool in = (win && rr < len);
            const long long row = in ? (long long)(start + rr) * g.ldw + wi : 0;
#pragma unroll
            for (int s = 0; s < G; ++s) {
              const float v = a[in ? row + g.gcol[s] : 0];
              rw[s][e] = in ? v : 0.f;
            }
          }
        }
        { // x / h: element e: row t % LI + LI * e of the tile, kk = t / LI
          const int rr = k0 + t / LI;
          const bool rin = (rr < len);
#pragma unroll
          for (int e = 0; e < NL; ++e) {
            const int n = jt0 + t % LI + LI * e;
            const bool in = (rin && n < jend);
            const float v = bsrc[in ? (long long)n * ldb + start + rr : 0];
            rx[e] = in ? v : 0.f;
          }
        }
      },
      [&]() TILE_INLINE {
#pragma unroll
        for (int e = 0; e < NL; ++e) {
#pragma unroll
          for (int s = 0; s < G; ++s) Ws[s][(t / BT + (NTHREADS / BT) * e) * P + t % BT] = rw[s][e];
          Xs[(t / LI) * P + t % LI + LI * e] = rx[e];
        }
      },
      [&](int kc) TILE_INLINE {
#pragma unroll
        for (int s = 0; s < G; ++s) eng[s].chunk(Ws[s], Xs, kc);
      });
  }

  // the epilogue: every gate of an element is in this thread
  const int epi = g.epi;
  eng[0].each([&](int i, int j, int r, float a0) TILE_INLINE {
    if (!stored(i, j, r)) return;
    const long long off = offset(i, j, r);
    if (xsmm::RNN_EPI_NONE == epi) {
#pragma unroll
      for (int s = 0; s < G; ++s) g.pre[s][zo + off] = eng[s].acc[j][i][r];
    }
    else if (xsmm::RNN_EPI_RNN == epi) {
      g.pre[0][off] = a0; // z
      float hv;
      if (0 == g.act) hv = (a0 < 0.f) ? 0.f : a0; // (a NaN and a -0.0 pass)
      else if (1 == g.act) hv = sigmoid_(a0);
      else hv = tanh_(a0);
      g.h[off] = hv;
    }
    else if (xsmm::RNN_EPI_LSTM == epi) {
      if (4 == G) { // sets: i, ci, f, o
        const float iv = sigmoid_(a0), fv = sigmoid_(eng[G > 2 ? 2 : 0].acc[j][i][r]), ov = sigmoid_(eng[G > 3 ? 3 : 0].acc[j][i][r]);
        const float civ = tanh_(eng[G > 1 ? 1 : 0].acc[j][i][r]);
        float csv = fv * g.csprev[off];
        csv = csv + iv * civ;
        const float cov = tanh_(csv);
        g.gi[off] = iv; g.gf[off] = fv; g.go[off] = ov; g.gci[off] = civ; g.cs[off] = csv; g.gco[off] = cov;
        g.h[off] = ov * cov;
      }
    }
    else if (xsmm::RNN_EPI_GRU1 == epi) {
      if (2 == G) { // sets: i, c
        const float iv = sigmoid_(a0), cv = sigmoid_(eng[G > 1 ? 1 : 0].acc[j][i][r]);
        g.gi[off] = iv; g.gci[off] = cv;
        g.go[off] = g.hprev[off] * iv;
      }
    }
    else { // RNN_EPI_GRU2, set: f
      const float fv = tanh_(a0), cv = g.gci[off];
      float hv = (1.0f - cv) * fv;
      hv = hv + cv * g.hprev[off];
      g.gf[off] = fv; g.h[off] = hv;
    }
  });
}

template<int G>
int launch_one(const RnnArgs& g, void* stream)
{
  const long long tk = ((long long)g.K + BT - 1) / BT, tn = ((long long)(g.n1 - g.n0) + BT - 1) / BT;
  if (tk > 0x7fffffffLL || tn > 65535 || g.nz > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((rnn_step<G>), dim3((unsigned)tk, (unsigned)tn, (unsigned)g.nz), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

} // namespace

namespace xsmm {

int launch_rnn(const RnnArgs& g, void* stream, const char** name)
{
  static const char* const names[4] = { "rnn_g1", "rnn_g2", "rnn_g3", "rnn_g4" };
  if (g.G < 1 || g.G > 4 || g.nseg < 0 || g.nseg > RNN_MAX_SEG) return (int)hipErrorInvalidValue;
  // an epilogue needs the sets it names
  if ((RNN_EPI_LSTM == g.epi && 4 != g.G) || (RNN_EPI_GRU1 == g.epi && 2 != g.G) || ((RNN_EPI_RNN == g.epi || RNN_EPI_GRU2 == g.epi) && 1 != g.G)) return (int)hipErrorInvalidValue;
  if (nullptr != name) *name = names[g.G - 1];
  if (g.n1 <= g.n0 || g.K < 1 || g.nz < 1) return 0;
  switch (g.G) {
    case 1: return launch_one<1>(g, stream);
    case 2: return launch_one<2>(g, stream);
    case 3: return launch_one<3>(g, stream);
    default: return launch_one<4>(g, stream);
  }
}

} // namespace xsmm
