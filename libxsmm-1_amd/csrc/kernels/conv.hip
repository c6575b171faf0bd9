// conv.hip -- the three passes of the convolution layer (libxsmm_dnn_execute_st, xsmm_dnn_conv.cpp) in fp32 on
// the blocked tensors: activations [image][block][row][column][block size], filter [ofm1][ifm1][kj][ki][ifm2][ofm2].
//
// The contract (the reference's generic templates, src/template/libxsmm_dnn_convolve_st_{fwd,bwd,upd}_custom_custom_generic.tpl.c,
// which are nothing but calls of SMM kernels: one fused multiply-add per term, the reduction index ascending):
//   FWD  out(k, pixel) = chain over r = (ifm1, kj, ki, ifm2) ascending of W(k, r) * X(r, pixel), started from the bias, from
//        +0.0 (overwrite) or from the value in memory; then the ReLU. Rim terms of a logical padding are products with +0.0.
//   BWD  din(c, pixel) = chain over (ofm1, oj ascending, ki ascending, ofm2) of the terms whose (oj, oi) lies inside the output;
//        the others are NOT computed (0 * Inf would be NaN, fma(0, w, -0.0) would be +0.0).
//   UPD  dW(k, (c, kj, ki)) = chain over (img, oj, oi); or, for strides above 1 with a window above 1 x 1, one chain from +0.0
//        per image and one rounded add per image. The reduction is never split and there are no atomics.
//
// FWD is an implicit GEMM on the matrix cores through tile_gemm.cuh: a work-group of 256 threads owns a BT x BT tile of
// D(k, pixel), BT = 128 or 64; r advances in chunks of 32 through LDS; what is left of an odd reduction length (3 * 7 * 7) ends on
// the vector ALU (tile_gemm.cuh: the k tail), never in a zero-padded matrix step. For a fixed ofm1 the filter is an r x ofmblock
// matrix that is contiguous in memory: W(k, r) lies at ofm1 * RTOT * ofmblock + r * ofmblock + ofm2; a thread keeps one k and walks
// r. Of X a thread keeps one r of the chunk -- decomposed into (ifm1, kj, ki, ifm2) with three divisions per chunk -- and walks the
// tile's pixels in steps of 8; what belongs to a pixel (its origin in the input, the rows and columns left to the rim, its place
// in the output, its image) is decomposed once per tile by the first BT threads into LDS tables. A pixel's ifmblock channels are
// one contiguous piece and so are the S pieces of a filter row, so the 8 lanes that share a pixel group read runs of r.
// LDS images and their banks: as in fc.hip (pitch BT + 8; reads of 32 consecutive floats; writes of X as 8 pixels x 4 r at banks
// 8 r + pixel; the tables are read at one address per register: broadcasts).
//
// BWD and UPD run on the vector ALU, one thread per element of dinput / dfilter, because the matrix instruction cannot leave a
// term out for some of its elements (BWD) and because only C * K * R * S chains are independent (UPD): DESIGN.md 8n says what
// that costs. Index arithmetic is per thread (a few divisions), the loops add strides.
//
// Bounds. Every address is formed from indices that were compared against their extents first; an element outside its tile's
// valid part, outside the share [w0, w1) or (FWD, logical padding) outside the input plane reads element 0 of its tensor and
// uses +0.0 instead. Stores are guarded by the same comparisons. Offsets fit 32 bits: every tensor has fewer than 2^31 elements
// (checked at create).
#include <hip/hip_runtime.h>

#include <climits>

#include "../xsmm_dnn_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::NTHREADS;
using xsmm::ConvArgs;
constexpr int BK = 32; // r per chunk
constexpr int LI = 8;  // pixels per group of loads of X

// (two waves per SIMD asked for: the compiler then keeps the accumulators in VGPRs, 224 registers at BT = 128, and spills nothing)
template<int BT>
__global__ __launch_bounds__(NTHREADS, 2) void conv_fwd(const ConvArgs g, const int img0, const int npix, const int jtile0)
{
  constexpr int P = BT + 8, NL = BK * BT / NTHREADS, TW = BT / 2 / tile::MfmaF32::TS;
  __shared__ float Ws[BK * P];
  __shared__ float Xs[BK * P];
  __shared__ int s_py[BT], s_px[BT]; // row and column of the pixel's window origin in the input buffer
  __shared__ int s_in[BT];           // offset of that origin in the input (of block 0, channel 0)
  __shared__ int s_out[BT];          // offset of the pixel in the output (of block 0, channel 0)
  __shared__ int s_img[BT];
  const int t = (int)threadIdx.x;
  const int plane = g.ofh * g.ofw, RTOT = g.C * g.R * g.S;
  const int it0 = BT * (int)blockIdx.x;
  const long long jt0l = (long long)BT * ((long long)jtile0 + blockIdx.y);
  if (it0 >= g.K || jt0l >= npix) return;
  const int jt0 = (int)jt0l;
  const int iend = (it0 + BT < g.K ? it0 + BT : g.K), jend = (jt0l + BT < npix ? jt0 + BT : npix);
  { // the items of a tile lie between those of its corners: a tile outside the share has nothing to do
    const long long lo = (long long)(img0 + jt0 / plane) * g.blocksofm + it0 / g.ofmblock;
    const long long hi = (long long)(img0 + (jend - 1) / plane) * g.blocksofm + (iend - 1) / g.ofmblock;
    if (hi < g.w0 || lo >= g.w1) return;
  }
  if (t < BT) {
    const bool in = (jt0 + t < jend);
    const int j = in ? jt0 + t : jt0;
    const int im = j / plane, p = j - im * plane, oj = p / g.ofw, oi = p - oj * g.ofw, img = img0 + im;
    const int py = oj * g.u - (0 != g.logical ? g.pad_h : 0), px = oi * g.v - (0 != g.logical ? g.pad_w : 0);
    s_py[t] = in ? py : INT_MIN / 2; // (no row of such a column is ever inside the plane)
    s_px[t] = px;
    s_in[t] = (img * g.blocksifm * g.ifhp + py) * g.ifwp * g.ifmblock + px * g.ifmblock;
    s_out[t] = ((img * g.blocksofm * g.ofhp + g.oph + oj) * g.ofwp + g.opw + oi) * g.ofmblock;
    s_img[t] = img;
  }
  __syncthreads();

  const float* __restrict__ const w = static_cast<const float*>(g.flt);
  const float* __restrict__ const x = static_cast<const float*>(g.in);
  float* __restrict__ const out = static_cast<float*>(g.out);

  // W: the thread's k and where its row of the filter starts
  const int wi = it0 + t % BT;
  const bool win = (wi < iend);
  const int wbase = win ? (wi / g.ofmblock) * RTOT * g.ofmblock + wi % g.ofmblock : 0;

  tile::MatrixCores<tile::MfmaF32, TW, BK, tile::Plain<float, P> > eng;
  eng.init(t);

  // rows of the tile as the accumulators see them
  int row_off[TW], row_blk[TW];
  bool row_in[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int k = it0 + eng.row(i);
    row_in[i] = (k < iend);
    const int ofm1 = (row_in[i] ? k : it0) / g.ofmblock;
    row_blk[i] = ofm1;
    row_off[i] = ofm1 * g.ofhp * g.ofwp * g.ofmblock + (row_in[i] ? k : it0) % g.ofmblock;
  }
  const auto stored = [&](int i, int jl) TILE_INLINE {
    if (!row_in[i] || jt0 + jl >= jend) return false;
    const long long item = (long long)s_img[jl] * g.blocksofm + row_blk[i];
    return item >= g.w0 && item < g.w1;
  };
  // the start of the chains: the bias, +0.0, or what the output holds
  if (0 != g.bias_on) {
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      const float b = row_in[i] ? static_cast<const float*>(g.bias)[it0 + eng.row(i)] : 0.f;
#pragma unroll
      for (int j = 0; j < TW; ++j) {
#pragma unroll
        for (int r = 0; r < tile::MfmaF32::NR; ++r) eng.acc[j][i][r] = b;
      }
    }
  }
  else if (0 == g.overwrite) {
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int r = 0; r < tile::MfmaF32::NR; ++r) {
        const int jl = eng.col(j, r);
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          const bool in = stored(i, jl);
          const float v = out[in ? s_out[jl] + row_off[i] : 0];
          eng.acc[j][i][r] = in ? v : 0.f;
        }
      }
    }
  }

  float rw[NL], rx[NL];
  tile::k_loop<BK>(RTOT,
    [&](int k0) TILE_INLINE {
      { // W: element e: k = t % BT, kk = t / BT + (NTHREADS / BT) * e
        const int r0 = k0 + t / BT;
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          const int r = r0 + (NTHREADS / BT) * e;
          const bool in = (win && r < RTOT);
          const float v = w[in ? wbase + r * g.ofmblock : 0];
          rw[e] = in ? v : 0.f;
        }
      }
      { // X: element e: pixel t % LI + LI * e, kk = t / LI
        const int r = k0 + t / LI;
        const bool rin = (r < RTOT);
        const int rr = rin ? r : 0;
        const int q = rr / g.ifmblock, ifm2 = rr - q * g.ifmblock;
        const int q2 = q / g.S, ki = q - q2 * g.S;
        const int ifm1 = q2 / g.R, kj = q2 - ifm1 * g.R;
        const int roff = ((ifm1 * g.ifhp + kj) * g.ifwp + ki) * g.ifmblock + ifm2;
#pragma unroll
        for (int e = 0; e < NL; ++e) {
          const int jl = t % LI + LI * e;
          const bool in = (rin && (unsigned)(s_py[jl] + kj) < (unsigned)g.ifhp && (unsigned)(s_px[jl] + ki) < (unsigned)g.ifwp);
          const float v = x[in ? s_in[jl] + roff : 0];
          rx[e] = in ? v : 0.f; // (a rim term of a logical padding is a product with +0.0, and it is computed)
        }
      }
    },
    [&]() TILE_INLINE {
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        Ws[(t / BT + (NTHREADS / BT) * e) * P + t % BT] = rw[e];
        Xs[(t / LI) * P + t % LI + LI * e] = rx[e];
      }
    },
    [&](int kc) TILE_INLINE { eng.chunk(Ws, Xs, kc); });

  const bool relu = (0 != g.relu);
  eng.each([&](int i, int j, int r, float v) TILE_INLINE {
    const int jl = eng.col(j, r);
    if (!stored(i, jl)) return;
    out[s_out[jl] + row_off[i]] = (relu && v < 0.f) ? 0.f : v; // (NaN and -0.0 pass)
  });
}

// BWD: a thread owns one element of dinput. Physical padding: the grid covers the whole padded plane and the rim is set to +0.0;
// logical padding: it covers the H x W interior, at (yy, xx) = (row + pad_h, column + pad_w) of the padded plane the reference
// works on.
__global__ __launch_bounds__(NTHREADS) void conv_bwd(const ConvArgs g)
{
  const long long item = (long long)g.w0 + blockIdx.y + (long long)blockIdx.z * gridDim.y;
  const int ph = g.ifhp, pw = g.ifwp; // the extents the grid covers (logical: ifhp == H)
  const long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  if (item >= g.w1 || e >= (long long)ph * pw * g.ifmblock) return;
  const int pix = (int)(e / g.ifmblock), ifm2 = (int)(e - (long long)pix * g.ifmblock);
  const int by = pix / pw, bx = pix - by * pw; // in the buffer
  const int img = (int)(item / g.blocksifm), ifm1 = (int)(item - (long long)img * g.blocksifm);
  float* __restrict__ const din = static_cast<float*>(g.in);
  const float* __restrict__ const dout = static_cast<const float*>(g.out);
  const float* __restrict__ const w = static_cast<const float*>(g.flt);
  const int off = ((int)item * ph * pw + pix) * g.ifmblock + ifm2;
  int yy = by, xx = bx;
  if (0 != g.logical) { yy += g.pad_h; xx += g.pad_w; }
  else if (by < g.pad_h || by >= g.H + g.pad_h || bx < g.pad_w || bx >= g.W + g.pad_w) { din[off] = 0.f; return; } // (pad_*_in == pad_*)
  // the outputs that reach the element: oj * u + kj == yy with kj in [0, R); oi * v + ki == xx with ki in [0, S)
  const int oj_lo = (yy - g.R + 1 > 0) ? (yy - g.R + g.u) / g.u : 0, oj_hi = (yy / g.u < g.ofh - 1) ? yy / g.u : g.ofh - 1;
  const int oi_top = xx / g.v, ki0 = xx - oi_top * g.v; // ki = ki0 + n * v meets oi = oi_top - n
  float acc = (0 != g.overwrite) ? 0.f : din[off];
  bool any = false;
  for (int ofm1 = 0; ofm1 < g.blocksofm; ++ofm1) {
    const int dbase = (img * g.blocksofm + ofm1) * g.ofhp;
    for (int oj = oj_lo; oj <= oj_hi; ++oj) {
      const int kj = yy - oj * g.u;
      for (int ki = ki0, oi = oi_top; ki < g.S && oi >= 0; ki += g.v, --oi) {
        if (oi >= g.ofw) continue;
        const float* const d = dout + ((dbase + g.oph + oj) * g.ofwp + g.opw + oi) * g.ofmblock;
        int woff, wstep;
        if (0 == g.flt_trans) { woff = ((((ofm1 * g.blocksifm + ifm1) * g.R + kj) * g.S + ki) * g.ifmblock + ifm2) * g.ofmblock; wstep = 1; }
        else { woff = (((ifm1 * g.blocksofm + ofm1) * g.R + g.R - 1 - kj) * g.S + g.S - 1 - ki) * g.ofmblock * g.ifmblock + ifm2; wstep = g.ifmblock; }
        for (int ofm2 = 0; ofm2 < g.ofmblock; ++ofm2) acc = __builtin_fmaf(w[woff + ofm2 * wstep], d[ofm2], acc);
        any = true;
      }
    }
  }
  if (any || 0 != g.overwrite) din[off] = acc; // (an element no term reaches keeps its start value)
}

// UPD: a thread owns one element of dfilter: item (ofm1, ifm1), then (kj, ki, ifm2, ofm2).
template<bool PER_IMAGE>
__global__ __launch_bounds__(NTHREADS) void conv_upd(const ConvArgs g)
{
  const long long item = (long long)g.w0 + blockIdx.y + (long long)blockIdx.z * gridDim.y;
  const int per_item = g.R * g.S * g.ifmblock * g.ofmblock;
  const long long el = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  if (item >= g.w1 || el >= per_item) return;
  const int e = (int)el;
  const int ofm2 = e % g.ofmblock, e1 = e / g.ofmblock, ifm2 = e1 % g.ifmblock, e2 = e1 / g.ifmblock, ki = e2 % g.S, kj = e2 / g.S;
  const int ofm1 = (int)(item / g.blocksifm), ifm1 = (int)(item - (long long)ofm1 * g.blocksifm);
  const float* __restrict__ const x = static_cast<const float*>(g.in);
  const float* __restrict__ const dout = static_cast<const float*>(g.out);
  float* __restrict__ const dw = static_cast<float*>(g.flt);
  const int off = (int)item * per_item + e;
  float acc = (0 != g.overwrite) ? 0.f : dw[off];
  // the input of term (oj, oi) lies at row (oj + kj) * su - py, column (oi + ki) * sv - px of the buffer, if that is inside
  // [0, rows) x [0, cols); else the term is a product with +0.0. PER_IMAGE: the window of output (oj, oi): rows oj * u + kj.
  // Otherwise the reference's transposed copy: row (oj + kj) of it holds buffer row (oj + kj) * u while oj + kj < ifhp / u.
  const bool lg = (0 != g.logical);
  const int py = lg ? g.pad_h : 0, px = lg ? g.pad_w : 0;
  const int rows = PER_IMAGE ? g.ifhp : (lg ? g.ifhp : (g.ifhp / g.u) * g.u), cols = PER_IMAGE ? g.ifwp : (lg ? g.ifwp : (g.ifwp / g.v) * g.v);
  for (int img = 0; img < g.N; ++img) {
    float loc = 0.f;
    const int xb = (img * g.blocksifm + ifm1) * g.ifhp, db = (img * g.blocksofm + ofm1) * g.ofhp;
    for (int oj = 0; oj < g.ofh; ++oj) {
      const int y = (PER_IMAGE ? oj * g.u + kj : (oj + kj) * g.u) - py;
      const bool yin = (y >= 0 && y < rows);
      const float* const d = dout + ((db + g.oph + oj) * g.ofwp + g.opw) * g.ofmblock + ofm2;
      const float* const xr = x + (xb + (yin ? y : 0)) * g.ifwp * g.ifmblock + ifm2;
      int xc = (PER_IMAGE ? ki : ki * g.v) - px;
      for (int oi = 0; oi < g.ofw; ++oi, xc += g.v) {
        const bool in = (yin && xc >= 0 && xc < cols);
        const float xv = in ? xr[xc * g.ifmblock] : 0.f;
        if (PER_IMAGE) loc = __builtin_fmaf(xv, d[oi * g.ofmblock], loc);
        else acc = __builtin_fmaf(d[oi * g.ofmblock], xv, acc);
      }
    }
    if (PER_IMAGE) acc = __fadd_rn(acc, loc);
  }
  dw[off] = acc;
}

// REGULAR_FILTER_TRANS[ifm1][ofm1][R-1-kj][S-1-ki][ofm2][ifm2] = REGULAR_FILTER[ofm1][ifm1][kj][ki][ifm2][ofm2]
__global__ __launch_bounds__(NTHREADS) void conv_trans_filter(const ConvArgs g, const long long total)
{
  const long long el = ((long long)blockIdx.x + (long long)blockIdx.y * gridDim.x) * NTHREADS + threadIdx.x;
  if (el >= total) return;
  int e = (int)el;
  const int ofm2 = e % g.ofmblock; e /= g.ofmblock;
  const int ifm2 = e % g.ifmblock; e /= g.ifmblock;
  const int ki = e % g.S; e /= g.S;
  const int kj = e % g.R; e /= g.R;
  const int ifm1 = e % g.blocksifm, ofm1 = e / g.blocksifm;
  const int to = ((((ifm1 * g.blocksofm + ofm1) * g.R + g.R - 1 - kj) * g.S + g.S - 1 - ki) * g.ofmblock + ofm2) * g.ifmblock + ifm2;
  static_cast<float*>(g.out)[to] = static_cast<const float*>(g.flt)[el];
}

// grid: x over the elements of an item, y and z over the items of the share (as pool.hip and bn.hip)
bool item_grid(long long per_item, long long items, dim3* grid)
{
  const long long gx = (per_item + NTHREADS - 1) / NTHREADS, gy = items < 32768 ? items : 32768, gz = (items + gy - 1) / gy;
  if (per_item < 1 || items < 1 || gx > 0x7fffffffLL || gz > 65535) return false;
  *grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
  return true;
}

template<int BT>
int launch_fwd(const ConvArgs& g, void* stream, const char* name)
{
  const int img0 = g.w0 / g.blocksofm, img1 = (g.w1 - 1) / g.blocksofm + 1;
  const long long npix = (long long)(img1 - img0) * g.ofh * g.ofw;
  if (npix > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long tiles_j = (npix + BT - 1) / BT;
  const unsigned tiles_i = (unsigned)((g.K + BT - 1) / BT);
  constexpr long long SLAB = 65535; // tiles of pixels one grid covers (gridDim.y); more go slab by slab
  for (long long j0 = 0; j0 < tiles_j; j0 += SLAB) {
    const unsigned ny = (unsigned)(tiles_j - j0 < SLAB ? tiles_j - j0 : SLAB);
    hipLaunchKernelGGL((conv_fwd<BT>), dim3(tiles_i, ny), dim3(NTHREADS), 0, (hipStream_t)stream, g, img0, (int)npix, (int)j0);
    const int e = (int)hipGetLastError();
    if (0 != e) return e;
    if (0 < j0) xsmm::note_launch(name); // (the caller counts one launch per pass: libxsmm_amd_launch_count is one per slab)
  }
  return 0;
}

} // namespace

namespace xsmm {

int launch_conv_fwd(const ConvArgs& g, void* stream, const char** name)
{
  *name = (128 == g.tile ? "conv_fwd_t128" : "conv_fwd_t64");
  if (64 != g.tile && 128 != g.tile) return (int)hipErrorInvalidValue;
  if (g.w1 <= g.w0) return 0;
  return 128 == g.tile ? launch_fwd<128>(g, stream, *name) : launch_fwd<64>(g, stream, *name);
}

int launch_conv_bwd(const ConvArgs& g, void* stream, const char** name)
{
  *name = "conv_bwd";
  dim3 grid;
  if (!item_grid((long long)g.ifhp * g.ifwp * g.ifmblock, (long long)g.w1 - g.w0, &grid)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_bwd, grid, dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_conv_upd(const ConvArgs& g, void* stream, const char** name)
{
  *name = (0 != g.per_image ? "conv_upd_image" : "conv_upd_gemm");
  dim3 grid;
  if (!item_grid((long long)g.R * g.S * g.ifmblock * g.ofmblock, (long long)g.w1 - g.w0, &grid)) return (int)hipErrorInvalidValue;
  if (0 != g.per_image) hipLaunchKernelGGL((conv_upd<true>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((conv_upd<false>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_conv_trans_filter(const ConvArgs& g, void* stream, const char** name)
{
  *name = "conv_trans_filter";
  const long long total = (long long)g.C * g.K * g.R * g.S, blocks = (total + NTHREADS - 1) / NTHREADS;
  const long long gx = blocks < 65536 ? blocks : 65536, gy = (blocks + gx - 1) / gx;
  if (total < 1 || gy > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_trans_filter, dim3((unsigned)gx, (unsigned)gy), dim3(NTHREADS), 0, (hipStream_t)stream, g, total);
  return (int)hipGetLastError();
}

} // namespace xsmm
