// conv_upd_mfma.hip -- UPD of the convolution layer on the matrix cores (LIBXSMM_AMD_CONV_UPD=mfma; the contract
// and the tensors are those of conv.hip, the bits those of its conv_upd).
//
// The kernel is a GEMM D(k, q) on tile_gemm.cuh: rows k = (ofm1, ofm2), columns q = (ifm1, kj, ki, ifm2) -- for a fixed ofm1
// dfilter is a q x ofmblock matrix that is contiguous in memory -- and the reduction l = (img, oj, oi) ascending. The operands are
// dout(k, l) and x(l, q): the input of term l for column q lies at row oy(l) + dy(q), column ox(l) + dx(q) of the input buffer,
// with oy = oj * u - py, ox = oi * v - px and dy = kj * u, dx = ki * v (GEMM form: the reference's transposed copy) or dy = kj,
// dx = ki (per-image form). A term outside [0, rows) x [0, cols) is a product with +0.0 that the contract computes: it is fed as
// a zero. v_mfma_f32_32x32x2_f32 is one fma per term, l ascending; a reduction of odd length ends on the vector ALU
// (tile_gemm.cuh: the k tail), never in a zero-padded matrix step.
//   GEMM form (IMAGE = false): one chain over all N * ofh * ofw terms, started from +0.0 or from the value in memory.
//   Per-image form (IMAGE = true): the same kernel with a second accumulator set of 16 registers. Per image one chain from +0.0
//     over ofh * ofw terms, then one rounded add per element into the running sum; the pipeline restarts per image, so that no
//     chunk straddles two images.
//
// Tile: 64 x 64 only. 256 threads own a 64 x 64 tile of D, each of the four waves one 32 x 32 tile of the matrix instruction.
// There is no 128 tile and LIBXSMM_AMD_CONV_TILE is not read: only C * K * R * S chains are independent and none may be split,
// so the scarce thing is work-groups, and the smallest tile that still shares its loads among four waves gives the most of them.
// The grid is the linear tile index on blockIdx.x (a filter has fewer than 2^31 elements, hence fewer than 2^19 tiles): one
// launch per call. A tile none of whose items (ofm1, ifm1) lies in the share [w0, w1) leaves at once.
//
// Loads. Both operands are fast along the tile index, not along the reduction: dout is contiguous along ofm2, x along ifm2. So
// lanes run along k and q -- thread t keeps tile index t % 64 of both operands and takes the 16 terms t / 64 + 4 e of a chunk of
// BK = 64 -- and a wave reads runs of a block (up to 64 bytes). What belongs to a q (dy, dx, its offset in the input relative to
// a term's origin, its offset in dfilter, its ifm1) and to a k goes once per tile into LDS tables, filled by the first 64 threads
// with three divisions per q and one per k. What belongs to an l (the offset of the output pixel in doutput, the origin's row,
// column and offset in the input) goes into a ring of four per-chunk tables of 64 entries, filled by the first 64 threads with
// two divisions per l four chunks ahead of the arithmetic, one trip ahead of the loads that read it. Nothing is divided per
// element.
//
// The pipeline. There may be four work-groups on the whole device, so the work-group hides the latency of its loads by itself:
// while chunk c multiplies out of LDS, chunk c + 1 lies in the other LDS image of the ring of two and the loads of chunks c + 2
// and c + 3 are in flight into two register stages (2 x 2 x 16 registers). A trip is: write the older stage (chunk c + 1) into
// the image that chunk c - 1 was read from, issue the loads of chunk c + 3 into the stage just freed, fill the table of chunk
// c + 4, multiply chunk c, one barrier. The barrier at the end of trip c - 1 is what frees the image and the table slot that trip c
// overwrites, and what publishes the image that trip c reads; every load has two trips of arithmetic to arrive. The loop is
// unrolled by two so that the stages are named registers. Plain C++ loads and the compiler's waits; BK = 64 by the compile record
// (no scratch, no spills; BK = 128 would need 132 KiB of LDS and 128 staged registers for the same two chunks ahead).
//
// LDS images and their banks (pitch 64; ds_read_b32 / ds_write_b32 serve lanes {0-31}, {32-63} against 32 banks of 4 bytes): a
// wave writes the 64 consecutive floats of one term, its halves 32 consecutive floats each: 32 banks. Operand reads of a matrix
// step are 32 consecutive floats of term 2 s (lanes 0-31) and of term 2 s + 1 (lanes 32-63): 32 banks at any pitch, so none is
// added. The tail reads one address per half wave, and the per-chunk table one 16-byte entry per wave: broadcasts.
//
// Bounds. An l past the end of the reduction, a k past K or a q past C * R * S is read as the first of its range -- a valid
// address -- and is never multiplied as a term (the last chunk is short) or stored; a term outside the input plane reads element
// 0 and feeds +0.0 (the stage carries 16 bits that say which). Stores are guarded per element by the tile's valid part and the
// share, as conv_fwd's. Offsets fit 32 bits (checked at create).
#include <hip/hip_runtime.h>

#include "../xsmm_dnn_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::NTHREADS;
using xsmm::ConvArgs;
constexpr int BT = 64;             // the tile, both ways
constexpr int BK = 64;             // terms per chunk
constexpr int P = BT;              // pitch of the LDS images
constexpr int KS = NTHREADS / BT;  // terms a pass of the 256 threads covers
constexpr int NL = BK / KS;        // elements per thread, operand and chunk
constexpr int SLOTS = 4;           // per-chunk tables in the ring
using i32x4 = __attribute__((ext_vector_type(4))) int;

template<bool IMAGE>
__global__ __launch_bounds__(NTHREADS) void conv_upd_mfma(const ConvArgs g, const int tiles_k)
{
  typedef tile::MatrixCores<tile::MfmaF32, 1, BK, tile::Plain<float, P> > Engine;
  constexpr int NR = tile::MfmaF32::NR;
  __shared__ float Ds[2][BK * P]; // dout(k, l) as [l][k], two chunks
  __shared__ float Xs[2][BK * P]; // x(l, q) as [l][q]
  __shared__ i32x4 s_l[SLOTS][BK]; // per term: offset in doutput (block 0, channel 0), origin row, origin column, origin offset in the input
  __shared__ int s_qoff[BT], s_qdy[BT], s_qdx[BT]; // per q: offset in the input relative to a term's origin, its row and column there
  __shared__ int s_qw[BT], s_qi[BT];               // ... its offset in dfilter (of ofm1 = 0, ofm2 = 0), its ifm1 (-1: past the end)
  __shared__ int s_koff[BT], s_kw[BT], s_k1[BT];   // per k: offset in doutput relative to a term's pixel, in dfilter, its ofm1 (-1)
  const int t = (int)threadIdx.x;
  const int plane = g.ofh * g.ofw, QTOT = g.C * g.R * g.S;
  const int kt0 = BT * ((int)blockIdx.x % tiles_k), qt0 = BT * ((int)blockIdx.x / tiles_k);
  if (kt0 >= g.K || qt0 >= QTOT) return;
  const int kend = (kt0 + BT < g.K ? kt0 + BT : g.K), qend = (qt0 + BT < QTOT ? qt0 + BT : QTOT);
  { // a tile none of whose items lies in the share has nothing to do
    const int per_ifm1 = g.R * g.S * g.ifmblock, i_lo = qt0 / per_ifm1, i_hi = (qend - 1) / per_ifm1;
    bool any = false;
    for (int o = kt0 / g.ofmblock; o <= (kend - 1) / g.ofmblock; ++o) {
      const long long lo = (long long)o * g.blocksifm + i_lo, hi = (long long)o * g.blocksifm + i_hi;
      any = any || (hi >= g.w0 && lo < g.w1);
    }
    if (!any) return;
  }
  const bool lg = (0 != g.logical);
  const int py = lg ? g.pad_h : 0, px = lg ? g.pad_w : 0;
  const int rows = (IMAGE || lg) ? g.ifhp : (g.ifhp / g.u) * g.u, cols = (IMAGE || lg) ? g.ifwp : (g.ifwp / g.v) * g.v;
  if (t < BT) {
    { // q as (ifm1, kj, ki, ifm2)
      const bool in = (qt0 + t < qend);
      const int q = in ? qt0 + t : qt0;
      const int a = q / g.ifmblock, ifm2 = q - a * g.ifmblock, b = a / g.S, ki = a - b * g.S, ifm1 = b / g.R, kj = b - ifm1 * g.R;
      const int dy = IMAGE ? kj : kj * g.u, dx = IMAGE ? ki : ki * g.v;
      s_qdy[t] = dy; s_qdx[t] = dx;
      s_qoff[t] = ((ifm1 * g.ifhp + dy) * g.ifwp + dx) * g.ifmblock + ifm2;
      s_qw[t] = q * g.ofmblock;
      s_qi[t] = in ? ifm1 : -1;
    }
    { // k as (ofm1, ofm2)
      const bool in = (kt0 + t < kend);
      const int k = in ? kt0 + t : kt0;
      const int ofm1 = k / g.ofmblock, ofm2 = k - ofm1 * g.ofmblock;
      s_koff[t] = ofm1 * g.ofhp * g.ofwp * g.ofmblock + ofm2;
      s_kw[t] = ofm1 * QTOT * g.ofmblock + ofm2;
      s_k1[t] = in ? ofm1 : -1;
    }
  }
  __syncthreads();

  const float* __restrict__ const x = static_cast<const float*>(g.in);
  const float* __restrict__ const dout = static_cast<const float*>(g.out);
  float* __restrict__ const dw = static_cast<float*>(g.flt);

  // the loads: the thread's tile index of both operands, and its first term of a chunk
  const int ti = t % BT, tk = t / BT;
  const int koff = s_koff[ti], qoff = s_qoff[ti], qdy = s_qdy[ti], qdx = s_qdx[ti];

  Engine eng;
  eng.init(t);
  // the stores: the thread's row of D
  const int k1 = s_k1[eng.row(0)], kw = s_kw[eng.row(0)];
  const auto stored = [&](int n) TILE_INLINE {
    const int qi = s_qi[n];
    if (k1 < 0 || qi < 0) return false;
    const long long item = (long long)k1 * g.blocksifm + qi;
    return item >= g.w0 && item < g.w1;
  };
  // the start of the chains: +0.0 or what dfilter holds (per-image form: of the running sum; its chains start from +0.0)
  tile::f32x16 sum;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int n = eng.col(0, r);
    const bool in = (0 == g.overwrite && stored(n));
    const float v = dw[in ? kw + s_qw[n] : 0];
    sum[r] = in ? v : 0.f;
  }
  if (!IMAGE) eng.acc[0][0] = sum;

  // the chain over the terms [l0, l0 + len), len >= 1, continued in eng.acc
  const auto reduce = [&](const int l0, const int len) TILE_INLINE {
    const int nch = (len + BK - 1) / BK;
    const auto fill = [&](int c, int e) TILE_INLINE { // entry e of the table of chunk c
      const long long ll = (long long)l0 + (long long)c * BK + e;
      const int l = (c < nch && ll < (long long)l0 + len) ? (int)ll : l0;
      const int img = l / plane, p = l - img * plane, oj = p / g.ofw, oi = p - oj * g.ofw;
      const int oy = oj * g.u - py, ox = oi * g.v - px;
      s_l[c % SLOTS][e] = i32x4{ ((img * g.blocksofm * g.ofhp + g.oph + oj) * g.ofwp + g.opw + oi) * g.ofmblock, oy, ox,
                                 ((img * g.blocksifm * g.ifhp + oy) * g.ifwp + ox) * g.ifmblock };
    };
    // element e: tile index ti, term tk + KS * e. A term outside the plane reads element 0 and is noted in the mask: it becomes +0.0
    // where the stage is written into LDS (a product with +0.0, and it is computed), so that no load of a stage is conditional
    const auto load = [&](int c, float (&rd)[NL], float (&rx)[NL], unsigned& inside) TILE_INLINE {
      inside = 0;
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        const i32x4 m = s_l[c % SLOTS][tk + KS * e]; // the same entry in every lane of the wave: kept in scalar registers
        const int ld = __builtin_amdgcn_readfirstlane(m.x), ly = __builtin_amdgcn_readfirstlane(m.y);
        const int lx = __builtin_amdgcn_readfirstlane(m.z), lo = __builtin_amdgcn_readfirstlane(m.w);
        rd[e] = dout[ld + koff];
        const bool in = ((unsigned)(ly + qdy) < (unsigned)rows) & ((unsigned)(lx + qdx) < (unsigned)cols);
        rx[e] = x[in ? lo + qoff : 0];
        inside |= (in ? 1u : 0u) << e;
      }
    };
    const auto store = [&](int c, const float (&rd)[NL], const float (&rx)[NL], unsigned inside) TILE_INLINE {
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        Ds[c & 1][(tk + KS * e) * P + ti] = rd[e];
        Xs[c & 1][(tk + KS * e) * P + ti] = (0 != (inside & (1u << e))) ? rx[e] : 0.f;
      }
    };
    // trip c: the stage holds chunk c + 1 on entry and chunk c + 3 on exit. Nothing in it depends on whether those chunks exist: a
    // chunk past the end is the table's clamped term 64 times, travels like any other and is never multiplied. So the loads are
    // unconditional and the compiler's count of what is in flight is exact on every path (a skipped load would make it wait for
    // both stages).
    const auto trip = [&](int c, float (&rd)[NL], float (&rx)[NL], unsigned& inside) TILE_INLINE {
      store(c + 1, rd, rx, inside);
      load(c + 3, rd, rx, inside);
      if (t < BK) fill(c + 4, t);
      const int left = len - c * BK;
      eng.chunk(Ds[c & 1], Xs[c & 1], left < BK ? (left > 0 ? left : 0) : BK);
      __syncthreads();
    };
    float rda[NL], rxa[NL], rdb[NL], rxb[NL];
    unsigned ina, inb;
    for (int i = t; i < SLOTS * BK; i += NTHREADS) fill(i / BK, i % BK);
    __syncthreads();
    load(0, rdb, rxb, inb);
    store(0, rdb, rxb, inb);
    load(1, rda, rxa, ina);
    load(2, rdb, rxb, inb);
    __syncthreads();
#pragma nounroll
    for (int c = 0; c < nch; c += 2) { // (an odd count of chunks ends on a trip that multiplies nothing)
      trip(c, rda, rxa, ina);
      trip(c + 1, rdb, rxb, inb);
    }
  };

  if (!IMAGE) reduce(0, g.N * plane);
  else {
    for (int img = 0; img < g.N; ++img) {
      reduce(img * plane, plane);
#pragma unroll
      for (int r = 0; r < NR; ++r) { sum[r] = __fadd_rn(sum[r], eng.acc[0][0][r]); eng.acc[0][0][r] = 0.f; }
    }
    eng.acc[0][0] = sum;
  }

  eng.each([&](int, int j, int r, float v) TILE_INLINE {
    const int n = eng.col(j, r);
    if (stored(n)) dw[kw + s_qw[n]] = v;
  });
}

} // namespace

namespace xsmm {

int launch_conv_upd_mfma(const ConvArgs& g, void* stream, const char** name)
{
  *name = (0 != g.per_image ? "conv_upd_mfma_image" : "conv_upd_mfma_gemm");
  if (g.w1 <= g.w0) return 0;
  const long long tiles_k = ((long long)g.K + BT - 1) / BT, tiles_q = ((long long)g.C * g.R * g.S + BT - 1) / BT;
  if (tiles_k * tiles_q > 0x7fffffffLL || (long long)g.N * g.ofh * g.ofw > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(tiles_k * tiles_q));
  if (0 != g.per_image) hipLaunchKernelGGL((conv_upd_mfma<true>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g, (int)tiles_k);
  else hipLaunchKernelGGL((conv_upd_mfma<false>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g, (int)tiles_k);
  return (int)hipGetLastError();
}

} // namespace xsmm
