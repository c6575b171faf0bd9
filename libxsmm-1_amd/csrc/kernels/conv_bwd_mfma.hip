// conv_bwd_mfma.hip -- BWD of the convolution layer on the matrix cores, for the pixels of dinput that have all their terms
// (the contract and the tensors are those of conv.hip).
//
// Which pixels. At u == v == 1, on the padded plane the reference works on (hp = H + 2 pad_h rows, ofh = hp - R + 1), a pixel
// (yy, xx) with R - 1 <= yy <= ofh - 1 and S - 1 <= xx <= ofw - 1 is reached by every one of its K * R * S terms: it is full.
// The full pixels inside the H x W interior are one rectangle, the same in every image (conv_bwd_full_rect, in the
// coordinates of the dinput buffer). This kernel computes that rectangle; the frame around it and a physical rim stay with
// conv.hip's predicated conv_bwd, whose threads leave the rectangle alone. No term is ever fed as a zero.
//
// The kernel is an implicit GEMM D(c, pixel) on tile_gemm.cuh, as conv_fwd: M = C as (ifm1, ifm2); N = the rectangle's pixels
// of the share's images, image after image; the reduction r = (ofm1, a, ki, ofm2) ascending, K * R * S long, where a = 0 ..
// R - 1 stands for kj = R - 1 - a, so that oj = yy - (R - 1) + a ascends as the reference's loop does, and oi = xx - ki. That is
// conv_bwd's chain per element, hence its bits (v_mfma_f32_32x32x2_f32 is one fma per term, k ascending; an odd K * R * S
// ends on the vector ALU: tile_gemm.cuh, the k tail). 256 threads own a BT x BT tile, BT = 64 or 128; r advances in chunks of
// 32 through LDS, the next chunk in flight while the current one multiplies.
//
// What belongs to a pixel is decomposed once per tile by the first BT threads (two divisions) into LDS tables: the offset in
// doutput of (img, ofm1 = 0, oph + yy - (R - 1), opw + xx), the offset of the pixel in dinput, the image. Of doutput a thread
// keeps one r of the chunk, decomposed into (ofm1, a, ki, ofm2) with three divisions per chunk -- its offset from the pixel's
// entry is ((ofm1 * ofhp + a) * ofwp - ki) * ofmblock + ofm2 -- and walks the tile's pixels in steps of 8. Every pixel of
// the tile is full, so no load of doutput is predicated: an r past K * R * S (never multiplied: the last chunk is short) is
// read as r = 0, a pixel or a channel past the tile's valid part as the tile's first.
//
// The filter, W(c, r), has two load maps (TRANS):
//   REGULAR_FILTER[ofm1][ifm1][kj][ki][ifm2][ofm2] is contiguous along ofm2, so lanes run along r exactly as for doutput: the
//     thread's one r, channels in steps of 8 through a table of the channels' offsets (one division per channel and tile).
//   REGULAR_FILTER_TRANS[ifm1][ofm1][a][S-1-ki][ofm2][ifm2] (OPTION_BWD_NO_FILTER_TRANSPOSE) is contiguous along ifm2, so lanes
//     run along c: a thread keeps one channel and takes 32 * BT / 256 values of r per chunk. Those r are the same for a whole
//     wave; their offsets come from a table of the chunk's 32 r that the first 32 threads fill one chunk ahead (two halves
//     in turn: the half a load reads was written before the two barriers of the k loop's previous trip).
//
// LDS images and their banks (pitch BT + 8 = 8 mod 32; ds_read_b32 / ds_write_b32 serve lanes {0-31}, {32-63} against 32
// banks of 4 bytes): operand reads are 32 consecutive floats of one kk: 32 banks. Writes of doutput and of the regular
// filter are 8 tile indices x 4 kk at banks 8 kk + index: 32 banks. Writes of the transposed filter are 32 consecutive floats
// of one kk (BT = 64: lanes 0-31 and 32-63 are the halves of one kk): 32 banks. The tables are read at one address per
// register or at 8 consecutive ones shared by four lanes each: broadcasts.
//
// Bounds. Every address is formed from clamped indices (above) or is a store guarded by the tile's valid part and the share
// [w0, w1), per element as conv_fwd's; a tile wholly outside the share leaves at once. Offsets fit 32 bits (checked at create).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "../xsmm_dnn_internal.hpp"
#include "tile_gemm.cuh"

namespace {

using tile::NTHREADS;
using xsmm::ConvArgs;
constexpr int BK = 32; // r per chunk
constexpr int LI = 8;  // tile indices per group of loads along r

// (two waves per SIMD asked for, as conv_fwd: the accumulators of BT = 128 then stay in VGPRs and nothing spills)
template<int BT, bool TRANS>
__global__ __launch_bounds__(NTHREADS, 2) void conv_bwd_mfma(const ConvArgs g, const int img0, const int npix, const int jtile0)
{
  constexpr int P = BT + 8, NL = BK * BT / NTHREADS, TW = BT / 2 / tile::MfmaF32::TS, KS = NTHREADS / BT;
  __shared__ float Ws[BK * P];
  __shared__ float Ds[BK * P];
  __shared__ int s_do[BT];  // offset in doutput of the first term's output pixel (of block 0, channel 0)
  __shared__ int s_di[BT];  // offset of the pixel in dinput (of block 0, channel 0)
  __shared__ int s_img[BT];
  __shared__ int s_cw[TRANS ? 1 : BT];     // regular filter: offset of the channel (ifm1, ifm2)
  __shared__ int s_rw[TRANS ? 2 * BK : 1]; // transposed filter: offsets of the r of a chunk, two chunks
  const int t = (int)threadIdx.x;
  const int cols = g.fx1 - g.fx0, plane = (g.fy1 - g.fy0) * cols, RTOT = g.K * g.R * g.S;
  const int it0 = BT * (int)blockIdx.x;
  const long long jt0l = (long long)BT * ((long long)jtile0 + blockIdx.y);
  if (it0 >= g.C || jt0l >= npix) return;
  const int jt0 = (int)jt0l;
  const int iend = (it0 + BT < g.C ? it0 + BT : g.C), jend = (jt0l + BT < npix ? jt0 + BT : npix);
  { // the items of a tile lie between those of its corners: a tile outside the share has nothing to do
    const long long lo = (long long)(img0 + jt0 / plane) * g.blocksifm + it0 / g.ifmblock;
    const long long hi = (long long)(img0 + (jend - 1) / plane) * g.blocksifm + (iend - 1) / g.ifmblock;
    if (hi < g.w0 || lo >= g.w1) return;
  }
  // r as (ofm1, a, ki, ofm2); an r past the end (or wrapped) is read as r = 0
  const auto split = [&](int r, int& ofm1, int& a, int& ki, int& ofm2) TILE_INLINE {
    const int rr = ((unsigned)r < (unsigned)RTOT) ? r : 0;
    const int q = rr / g.ofmblock, q2 = q / g.S;
    ofm2 = rr - q * g.ofmblock; ki = q - q2 * g.S; ofm1 = q2 / g.R; a = q2 - ofm1 * g.R;
  };
  const auto trans_off = [&](int r) TILE_INLINE { // of REGULAR_FILTER_TRANS[0][ofm1][a][S-1-ki][ofm2][0]
    int ofm1, a, ki, ofm2;
    split(r, ofm1, a, ki, ofm2);
    return ((((ofm1 * g.R + a) * g.S + g.S - 1 - ki) * g.ofmblock) + ofm2) * g.ifmblock;
  };
  if (t < BT) {
    const int j = (jt0l + t < jend) ? jt0 + t : jt0;
    const int im = j / plane, p = j - im * plane, ry = p / cols, rx = p - ry * cols, img = img0 + im;
    const int by = g.fy0 + ry, bx = g.fx0 + rx; // in the buffer; on the padded plane:
    const int yy = by + (0 != g.logical ? g.pad_h : 0), xx = bx + (0 != g.logical ? g.pad_w : 0);
    s_do[t] = ((img * g.blocksofm * g.ofhp + g.oph + yy - (g.R - 1)) * g.ofwp + g.opw + xx) * g.ofmblock;
    s_di[t] = ((img * g.blocksifm * g.ifhp + by) * g.ifwp + bx) * g.ifmblock;
    s_img[t] = img;
    if (!TRANS) {
      const int c = (it0 + t < iend) ? it0 + t : it0, ifm1 = c / g.ifmblock;
      s_cw[t] = (ifm1 * g.R * g.S * g.ifmblock + c - ifm1 * g.ifmblock) * g.ofmblock;
    }
  }
  if (TRANS && t < BK) s_rw[t] = trans_off(t);
  __syncthreads();

  const float* __restrict__ const w = static_cast<const float*>(g.flt);
  const float* __restrict__ const dout = static_cast<const float*>(g.out);
  float* __restrict__ const din = static_cast<float*>(g.in);

  // transposed filter: the thread's channel and where its part of the filter starts
  int wbase = 0;
  if (TRANS) {
    const int c = (it0 + t % BT < iend) ? it0 + t % BT : it0, ifm1 = c / g.ifmblock;
    wbase = ifm1 * g.blocksofm * g.R * g.S * g.ofmblock * g.ifmblock + c - ifm1 * g.ifmblock;
  }

  tile::MatrixCores<tile::MfmaF32, TW, BK, tile::Plain<float, P> > eng;
  eng.init(t);

  // rows of the tile as the accumulators see them
  int row_off[TW], row_blk[TW];
  bool row_in[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int c = it0 + eng.row(i);
    row_in[i] = (c < iend);
    const int ifm1 = (row_in[i] ? c : it0) / g.ifmblock;
    row_blk[i] = ifm1;
    row_off[i] = ifm1 * g.ifhp * g.ifwp * g.ifmblock + (row_in[i] ? c : it0) % g.ifmblock;
  }
  const auto stored = [&](int i, int jl) TILE_INLINE {
    if (!row_in[i] || jt0l + jl >= jend) return false;
    const long long item = (long long)s_img[jl] * g.blocksifm + row_blk[i];
    return item >= g.w0 && item < g.w1;
  };
  // the start of the chains: +0.0 (init) or what dinput holds
  if (0 == g.overwrite) {
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
      for (int r = 0; r < tile::MfmaF32::NR; ++r) {
        const int jl = eng.col(j, r);
#pragma unroll
        for (int i = 0; i < TW; ++i) {
          const bool in = stored(i, jl);
          const float v = din[in ? s_di[jl] + row_off[i] : 0];
          eng.acc[j][i][r] = in ? v : 0.f;
        }
      }
    }
  }

  float rw[NL], rd[NL];
  tile::k_loop<BK>(RTOT,
    [&](int k0) TILE_INLINE {
      int ofm1, a, ki, ofm2; // the thread's r: kk = t / LI; element e: tile index t % LI + LI * e
      split(k0 + t / LI, ofm1, a, ki, ofm2);
      const int doff = ((ofm1 * g.ofhp + a) * g.ofwp - ki) * g.ofmblock + ofm2;
#pragma unroll
      for (int e = 0; e < NL; ++e) rd[e] = dout[s_do[t % LI + LI * e] + doff];
      if (!TRANS) {
        const int woff = ((ofm1 * g.blocksifm * g.R + g.R - 1 - a) * g.S + ki) * g.ifmblock * g.ofmblock + ofm2;
#pragma unroll
        for (int e = 0; e < NL; ++e) rw[e] = w[s_cw[t % LI + LI * e] + woff];
      }
      else { // element e: channel t % BT, kk = t / BT + KS * e
        const int half = (k0 / BK) & 1;
#pragma unroll
        for (int e = 0; e < NL; ++e) rw[e] = w[wbase + s_rw[half * BK + t / BT + KS * e]];
        if (t < BK) s_rw[(half ^ 1) * BK + t] = trans_off(k0 + BK + t); // the next chunk's, read after two barriers
      }
    },
    [&]() TILE_INLINE {
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        Ds[(t / LI) * P + t % LI + LI * e] = rd[e];
        if (!TRANS) Ws[(t / LI) * P + t % LI + LI * e] = rw[e];
        else Ws[(t / BT + KS * e) * P + t % BT] = rw[e];
      }
    },
    [&](int kc) TILE_INLINE { eng.chunk(Ws, Ds, kc); });

  eng.each([&](int i, int j, int r, float v) TILE_INLINE {
    const int jl = eng.col(j, r);
    if (stored(i, jl)) din[s_di[jl] + row_off[i]] = v;
  });
}

template<int BT>
int launch_mfma(const ConvArgs& g, void* stream, const char* name)
{
  const int img0 = g.w0 / g.blocksifm, img1 = (g.w1 - 1) / g.blocksifm + 1;
  const long long npix = (long long)(img1 - img0) * (g.fy1 - g.fy0) * (g.fx1 - g.fx0);
  if (npix < 1 || npix > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long tiles_j = (npix + BT - 1) / BT;
  const unsigned tiles_i = (unsigned)((g.C + BT - 1) / BT);
  const auto kernel = (0 != g.flt_trans) ? conv_bwd_mfma<BT, true> : conv_bwd_mfma<BT, false>;
  constexpr long long SLAB = 65535; // tiles of pixels one grid covers (gridDim.y); more go slab by slab, as conv_fwd's
  for (long long j0 = 0; j0 < tiles_j; j0 += SLAB) {
    const unsigned ny = (unsigned)(tiles_j - j0 < SLAB ? tiles_j - j0 : SLAB);
    hipLaunchKernelGGL(kernel, dim3(tiles_i, ny), dim3(NTHREADS), 0, (hipStream_t)stream, g, img0, (int)npix, (int)j0);
    const int e = (int)hipGetLastError();
    if (0 != e) return e;
    if (0 < j0) xsmm::note_launch(name); // (the caller counts one launch per pass)
  }
  return 0;
}

} // namespace

namespace xsmm {

bool conv_bwd_full_rect(ConvArgs* g)
{
  const char* const e = getenv("LIBXSMM_AMD_CONV_BWD"); // read per call, as LIBXSMM_AMD_CONV_TILE
  if (nullptr == e || 0 != strcmp(e, "mfma") || 1 != g->u || 1 != g->v || 0 == libxsmm_amd_get_mfma()) return false;
  // full on the padded plane: [R - 1, ofh) x [S - 1, ofw); the interior there: [pad_h, pad_h + H) x [pad_w, pad_w + W)
  const int oy = (0 != g->logical ? g->pad_h : 0), ox = (0 != g->logical ? g->pad_w : 0); // buffer = padded plane - (oy, ox)
  const int y0 = (g->R - 1 > g->pad_h ? g->R - 1 : g->pad_h), y1 = (g->ofh < g->pad_h + g->H ? g->ofh : g->pad_h + g->H);
  const int x0 = (g->S - 1 > g->pad_w ? g->S - 1 : g->pad_w), x1 = (g->ofw < g->pad_w + g->W ? g->ofw : g->pad_w + g->W);
  if (y1 <= y0 || x1 <= x0) return false;
  g->fy0 = y0 - oy; g->fy1 = y1 - oy; g->fx0 = x0 - ox; g->fx1 = x1 - ox;
  return true;
}

int launch_conv_bwd_mfma(const ConvArgs& g, void* stream, const char** name)
{
  *name = (128 == g.tile ? "conv_bwd_mfma_t128" : "conv_bwd_mfma_t64");
  if (64 != g.tile && 128 != g.tile) return (int)hipErrorInvalidValue;
  if (g.w1 <= g.w0) return 0;
  return 128 == g.tile ? launch_mfma<128>(g, stream, *name) : launch_mfma<64>(g, stream, *name);
}

} // namespace xsmm
