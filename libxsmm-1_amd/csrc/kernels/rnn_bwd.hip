// rnn_bwd.hip -- the backward and update passes of the RNN cell layer (libxsmm_dnn_rnncell_execute_st with BWD, UPD, BWDUPD;
// xsmm_dnn_rnn.cpp) for the simple cells and the LSTM, in fp32 on the plain tensors.
//
// The contract (src/template/libxsmm_dnn_rnncell_st_{rnn,lstm}_bwdupd_nc_ck_generic.tpl.c with ..._lstm_bwdupd_nc_kcck_core.tpl.c and
// the loops of src/libxsmm_dnn_elementwise.c): every product sum is one chain acc = fma(a, b, acc) in a stated order, every
// elementwise multiply, add and subtraction is rounded on its own (the file is compiled with contraction off, as rnn.hip is).
//
// Three kernels, all on tile_gemm.cuh's MatrixCores (v_mfma_f32_32x32x2_f32, a 64 x 64 tile per work-group of 256 threads, chunks of
// BK = 32 through LDS images of pitch 72, the k tail on the vector ALU):
//   rnn_bwd_chain   out[row][m] = start continued by sum over segments, over columns q of a segment, of filt[m][q] * delta[row][q].
//                   The reduction runs along the contiguous dimension of BOTH operands (the filter is read transposed), so both are
//                   loaded as rnn.hip loads x: a thread keeps one reduction index and walks eight rows. It serves the step recurrence
//                   (filt = r; the cell's epilogue writes the step's deltas), the LSTM's dhp and dx of all steps at once (blockIdx.z).
//   rnn_bwd_weight  out[m][j] = +0.0 continued by the chain over the steps descending and the rows ascending of act_t[row][m] *
//                   delta_t[row][j]: the reduction index is the slow dimension of both operands, which are loaded as rnn.hip loads w.
//   rnn_bwd_bias    db[j] = +0.0 + delta_t[row][j] in the same order, one thread per column.
//
// Bounds. Every address is formed from indices compared against the extents first (beyond them: element 0 of the operand and +0.0 in
// the image, which only reaches accumulators that are never stored); stores are guarded by the same comparisons. Offsets are 64-bit:
// the delta buffer may exceed 2^31 elements.
#include <hip/hip_runtime.h>

#include "../xsmm_dnn_internal.hpp"
#include "tile_gemm.cuh"

#pragma clang fp contract(off)

namespace {

using tile::NTHREADS;
using xsmm::RnnBwdChainArgs;
using xsmm::RnnBwdWeightArgs;

constexpr int BT = 64;            // extent of the work-group tile, both ways
constexpr int BK = 32;            // reduction indices per chunk
constexpr int LI = NTHREADS / BK; // rows per group of loads of an operand whose fast dimension is the reduction
constexpr int P = BT + 8, NL = BK * BT / NTHREADS, TW = BT / 2 / tile::MfmaF32::TS;

typedef tile::MatrixCores<tile::MfmaF32, TW, BK, tile::Plain<float, P> > Engine;

// act'(z) of the simple cells (libxsmm_internal_matrix_{relu,sigmoid,tanh}_inverse*_ld)
__device__ __forceinline__ float inverse_(int act, float z)
{
  if (0 == act) return (z < 0.f) ? 0.f : 1.f;
  if (1 == act) {
    const float e = (float)exp((double)-z);
    const float s = 1.0f / (1.0f + e);
    return (1.0f - s) * s;
  }
  const float t = (float)tanh((double)z);
  return 1.0f - (t * t);
}

template<int EPI>
__global__ __launch_bounds__(NTHREADS) void rnn_bwd_chain(const RnnBwdChainArgs g)
{
  __shared__ float Fs[BK * P];
  __shared__ float Ds[BK * P];
  const int t = (int)threadIdx.x;
  const int it0 = BT * (int)blockIdx.x, jt0 = g.n0 + BT * (int)blockIdx.y;
  if (it0 >= g.M || jt0 >= g.n1) return;
  const int iend = (it0 + BT < g.M ? it0 + BT : g.M), jend = (jt0 + BT < g.n1 ? jt0 + BT : g.n1);
  const float* __restrict__ const delta = g.delta + (long long)blockIdx.z * g.zd;

  Engine eng;
  eng.init(t);
  // the tile as the accumulators see it: feature m along the rows of the matrix instruction, row of the minibatch along its columns
  const auto stored = [&](int i, int j, int r) TILE_INLINE { return it0 + eng.row(i) < iend && jt0 + eng.col(j, r) < jend; };
  const auto offset = [&](int i, int j, int r) TILE_INLINE { return (long long)(jt0 + eng.col(j, r)) * g.M + it0 + eng.row(i); };

  if (xsmm::RNN_BWD_EPI_SIMPLE == EPI) { // delta = dh, then += R^T . delta of the step after
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int r = 0; r < tile::MfmaF32::NR; ++r) {
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          const bool in = stored(i, j, r);
          const float v = g.dh[in ? offset(i, j, r) : 0];
          eng.acc[j][i][r] = in ? v : 0.f;
        }
      }
    }
  }

  const int kk = t / LI, lr = t % LI; // the thread's reduction index inside a chunk and its first row of either tile
  float rf[NL], rd[NL];
  for (int sg = 0; sg < g.nseg; ++sg) {
    const int start = g.seg[sg].start, len = g.seg[sg].len;
    tile::k_loop<BK>(len,
      [&](int k0) TILE_INLINE {
        const int q = k0 + kk;
        const bool qin = (q < len);
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          const int m = it0 + lr + LI * e, n = jt0 + lr + LI * e;
          const bool fin = (qin && m < iend), din = (qin && n < jend);
          const float fv = g.filt[fin ? (long long)m * g.ld + start + q : 0];
          const float dv = delta[din ? (long long)n * g.ld + start + q : 0];
          rf[e] = fin ? fv : 0.f;
          rd[e] = din ? dv : 0.f;
        }
      },
      [&]() TILE_INLINE {
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          Fs[kk * P + lr + LI * e] = rf[e];
          Ds[kk * P + lr + LI * e] = rd[e];
        }
      },
      [&](int kc) TILE_INLINE { eng.chunk(Fs, Ds, kc); });
  }

  eng.each([&](int i, int j, int r, float a) TILE_INLINE {
    if (!stored(i, j, r)) return;
    const long long off = offset(i, j, r);
    if (xsmm::RNN_BWD_EPI_STORE == EPI) {
      g.out[(long long)blockIdx.z * g.zo + off] = a;
    }
    else if (xsmm::RNN_BWD_EPI_SIMPLE == EPI) {
      g.dstep[off] = a * inverse_(g.act, g.z[off]); // (ld == M == K)
    }
    else { // the LSTM's elementwise steps in the order of the core template; t1, t2 are its scratch tensors
      const float iv = g.gi[off], fv = g.gf[off], ov = g.go[off], civ = g.gci[off], cov = g.gco[off];
      const float dout = (0 != g.last) ? g.dh[off] : a + g.dh[off];
      float t1 = dout * ov, t2 = 1.0f - (cov * cov);
      t1 = t1 * t2;
      const float dcp = ((0 != g.last) ? g.dcs[off] : g.dcsp[off]) + t1;
      t1 = dcp * iv; t2 = 1.0f - (civ * civ);
      const float dci = t1 * t2;
      t1 = dcp * civ; t2 = 1.0f - iv;
      float di = iv * t2;
      di = t1 * di;
      t1 = dcp * g.csprev[off]; t2 = 1.0f - fv;
      float df = fv * t2;
      df = t1 * df;
      t1 = dout * cov; t2 = 1.0f - ov;
      t2 = ov * t2;
      const float dp = t1 * t2;
      g.dcsp[off] = fv * dcp;
      float* __restrict__ const d = g.dstep + (long long)(jt0 + eng.col(j, r)) * g.ld + it0 + eng.row(i);
      d[0] = di; d[g.M] = dci; d[2 * (long long)g.M] = df; d[3 * (long long)g.M] = dp;
    }
  });
}

__global__ __launch_bounds__(NTHREADS) void rnn_bwd_weight(const RnnBwdWeightArgs g)
{
  __shared__ float Ds[BK * P];
  __shared__ float As[BK * P];
  const int t = (int)threadIdx.x;
  const int it0 = BT * (int)blockIdx.x, jt0 = BT * (int)blockIdx.y; // column j of the deltas, feature m of the activations
  if (it0 >= g.ld || jt0 >= g.M) return;
  const int iend = (it0 + BT < g.ld ? it0 + BT : g.ld), jend = (jt0 + BT < g.M ? jt0 + BT : g.M);

  Engine eng;
  eng.init(t); // +0.0

  const int lc = t % BT; // the thread's column of either tile
  const bool din = (it0 + lc < iend), ain = (jt0 + lc < jend);
  float rd[NL], ra[NL];
  for (int s = g.T - 1; s >= 0; --s) {
    const float* __restrict__ const dl = g.delta + (long long)s * g.N * g.ld;
    const float* __restrict__ const ac = (0 == g.shift) ? g.act + (long long)s * g.N * g.M : (0 == s ? g.act0 : g.act + (long long)(s - 1) * g.N * g.M);
    tile::k_loop<BK>(g.N,
      [&](int k0) TILE_INLINE { // element e: column t % BT, row k0 + t / BT + (NTHREADS / BT) * e
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          const int n = k0 + t / BT + (NTHREADS / BT) * e;
          const bool nin = (n < g.N);
          const float dv = dl[(nin && din) ? (long long)n * g.ld + it0 + lc : 0];
          const float av = ac[(nin && ain) ? (long long)n * g.M + jt0 + lc : 0];
          rd[e] = (nin && din) ? dv : 0.f;
          ra[e] = (nin && ain) ? av : 0.f;
        }
      },
      [&]() TILE_INLINE {
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          Ds[(t / BT + (NTHREADS / BT) * e) * P + lc] = rd[e];
          As[(t / BT + (NTHREADS / BT) * e) * P + lc] = ra[e];
        }
      },
      [&](int kc) TILE_INLINE { eng.chunk(Ds, As, kc); });
  }

  eng.each([&](int i, int j, int r, float a) TILE_INLINE {
    const int col = it0 + eng.row(i), m = jt0 + eng.col(j, r);
    if (col < iend && m < jend) g.out[(long long)m * g.ld + col] = a;
  });
}

__global__ __launch_bounds__(NTHREADS) void rnn_bwd_bias(const float* __restrict__ delta, float* __restrict__ db, int ld, int N, int T)
{
  const long long j = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= ld) return;
  float s = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const float* __restrict__ const d = delta + (long long)t * N * ld + j;
    for (int n = 0; n < N; ++n) s = s + d[(long long)n * ld];
  }
  db[j] = s;
}

template<int EPI>
int launch_chain(const RnnBwdChainArgs& g, void* stream)
{
  const long long tm = ((long long)g.M + BT - 1) / BT, tn = ((long long)(g.n1 - g.n0) + BT - 1) / BT;
  if (tm > 0x7fffffffLL || tn > 65535 || g.nz > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((rnn_bwd_chain<EPI>), dim3((unsigned)tm, (unsigned)tn, (unsigned)g.nz), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

} // namespace

namespace xsmm {

int launch_rnn_bwd_chain(const RnnBwdChainArgs& g, void* stream, const char** name)
{
  static const char* const names[3] = { "rnn_bwd_chain", "rnn_bwd_step_rnn", "rnn_bwd_step_lstm" };
  if (g.epi < 0 || g.epi > 2 || g.nseg < 0 || g.nseg > RNN_BWD_MAX_SEG) return (int)hipErrorInvalidValue;
  if (RNN_BWD_EPI_STORE != g.epi && (1 != g.nz || g.ld != (RNN_BWD_EPI_LSTM == g.epi ? 4 : 1) * g.M)) return (int)hipErrorInvalidValue;
  if (nullptr != name) *name = names[g.epi];
  if (g.n1 <= g.n0 || g.M < 1 || g.nz < 1) return 0;
  switch (g.epi) {
    case RNN_BWD_EPI_STORE: return launch_chain<RNN_BWD_EPI_STORE>(g, stream);
    case RNN_BWD_EPI_SIMPLE: return launch_chain<RNN_BWD_EPI_SIMPLE>(g, stream);
    default: return launch_chain<RNN_BWD_EPI_LSTM>(g, stream);
  }
}

int launch_rnn_bwd_weight(const RnnBwdWeightArgs& g, void* stream, const char** name)
{
  if (nullptr != name) *name = "rnn_bwd_weight";
  if (g.M < 1 || g.ld < 1 || g.N < 1 || g.T < 1) return 0;
  const long long tj = ((long long)g.ld + BT - 1) / BT, tm = ((long long)g.M + BT - 1) / BT;
  if (tj > 0x7fffffffLL || tm > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rnn_bwd_weight, dim3((unsigned)tj, (unsigned)tm), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_rnn_bwd_bias(const float* delta, float* db, int ld, int N, int T, void* stream, const char** name)
{
  if (nullptr != name) *name = "rnn_bwd_bias";
  if (ld < 1 || N < 1 || T < 1) return 0;
  hipLaunchKernelGGL(rnn_bwd_bias, dim3((unsigned)(((long long)ld + NTHREADS - 1) / NTHREADS)), dim3(NTHREADS), 0, (hipStream_t)stream, delta, db, ld, N, T);
  return (int)hipGetLastError();
}

} // namespace xsmm
