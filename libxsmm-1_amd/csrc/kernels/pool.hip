// pool.hip -- the pooling layer (include/libxsmm_dnn_pooling.h): FWD and BWD of max and average pooling on the blocked
// activations [item][row][column][16], item = image * channel blocks + channel block, in fp32 and bf16. One source, eight
// instantiations.
//
// The contract (the reference's generic templates, src/template/libxsmm_dnn_pooling_st_{fwd,bwd}_custom_generic.tpl.c):
//   FWD MAX  every output starts at -FLT_MAX; the window is walked kh ascending, then kw ascending, positions outside the
//            plane are skipped, a strict > replaces value and index. The mask element is written only if something won.
//   FWD AVG  an fp32 sum from +0.0 in the same order, then one multiply by 1 / (R * S).
//   BWD      written as a gather: an input element visits the outputs whose window covers it, ho ascending, then wo ascending
//            (the order in which the reference's scatter reaches it), and accumulates from +0.0; MAX adds dout where the mask
//            names the element, AVG adds dout * recp as a SEPARATE multiply and add (what the reference's build does: DESIGN 8h).
//   bf16     widened by a shift, computed in fp32, stored by truncation.
// Every add and multiply goes through add_rn / mul_rn of dnn_pixel.cuh, compiled with fp contraction off (why the __f*_rn
// intrinsics are not enough: there). No instantiation may hold an fma.
//
// Mapping. A pixel's 16 channels are contiguous: 64 bytes in fp32, 32 in bf16. A thread owns a 16-byte piece of one pixel --
// four lanes in fp32, eight in bf16 -- of the output (FWD) or of the input (BWD); consecutive threads own consecutive pieces,
// pixels in row-major order of the unpadded plane, so a wave's stores cover 1 KiB of consecutive pixels (less the physical
// padding at a row's end) and its loads are 16-byte pieces, 64 / 32 bytes contiguous per pixel and dense along W for stride 1.
// The pixel index is decomposed once per thread (one division); the window is walked by adding row and pixel strides. BWD
// derives its range of covering outputs with two more divisions per thread. Nothing is shared, so there is no LDS and no
// barrier: overlapping windows are served by the caches (measured or not: DESIGN 8h).
//
// Bounds. A thread leaves unless its pixel lies inside the plane and its item inside [w0, w1); every address it forms is that of
// an element inside the interior of an item's plane. A mask value is only compared, never used as an address.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../xsmm_dnn_internal.hpp"
#include "dnn_pixel.cuh"

namespace {

using xsmm::PoolArgs;

constexpr int NTHREADS = 256;

// one rounding each, never fused (the pragma covers what is defined from here to the end of the file)
#pragma clang fp contract(off)
using pixel::Piece;
using pixel::add_rn;
using pixel::mul_rn;

// the item and the piece of a thread; false: nothing to do
template<int LANES>
__device__ __forceinline__ bool locate(const PoolArgs& g, int pixels, long long* item, int* pixel, int* lane0)
{
  constexpr int PIECES = 16 / LANES;
  const long long it = (long long)g.w0 + blockIdx.y + (long long)blockIdx.z * gridDim.y;
  const int p = (int)(blockIdx.x * (NTHREADS / PIECES) + threadIdx.x / PIECES);
  *item = it; *pixel = p; *lane0 = (int)(threadIdx.x % PIECES) * LANES;
  return it < g.w1 && p < pixels;
}

template<bool BF16, bool IS_MAX>
__global__ __launch_bounds__(NTHREADS) void pool_fwd(const PoolArgs g)
{
  typedef Piece<BF16> P;
  constexpr int L = P::LANES;
  long long item; int pixel, lane0;
  if (!locate<L>(g, g.ofh * g.ofw, &item, &pixel, &lane0)) return;
  const int ho = pixel / g.ofw, wo = pixel - ho * g.ofw;
  const int hi0 = ho * g.u - g.pad_h, wi0 = wo * g.v - g.pad_w;
  // the window clipped to the plane: kh in [kh0, kh1), kw in [kw0, kw1)
  const int kh0 = hi0 < 0 ? -hi0 : 0, kh1 = (g.H - hi0 < g.R) ? g.H - hi0 : g.R;
  const int kw0 = wi0 < 0 ? -wi0 : 0, kw1 = (g.W - wi0 < g.S) ? g.W - wi0 : g.S;
  const int ifwp = g.W + 2 * g.ipw;
  const long long in_item = item * ((long long)(g.H + 2 * g.iph) * ifwp * 16);
  float acc[L];
  int idx[L];
#pragma unroll
  for (int l = 0; l < L; ++l) { acc[l] = IS_MAX ? -FLT_MAX : 0.0f; idx[l] = -1; }
  for (int kh = kh0; kh < kh1; ++kh) {
    const int hi = hi0 + kh;
    long long elem = in_item + ((long long)(hi + g.iph) * ifwp + (wi0 + kw0 + g.ipw)) * 16 + lane0;
    int here = (hi * g.W + wi0 + kw0) * 16 + lane0;   // the mask's index: relative to the unpadded plane
    for (int kw = kw0; kw < kw1; ++kw, elem += 16, here += 16) {
      float x[L];
      P::load(g.in, elem, x);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if (IS_MAX) { if (x[l] > acc[l]) { acc[l] = x[l]; idx[l] = here + l; } }
        else acc[l] = add_rn(acc[l], x[l]);
      }
    }
  }
  if (!IS_MAX) {
#pragma unroll
    for (int l = 0; l < L; ++l) acc[l] = mul_rn(acc[l], g.recp);
  }
  const long long out_elem = item * ((long long)(g.ofh + 2 * g.oph) * (g.ofw + 2 * g.opw) * 16)
    + ((long long)(ho + g.oph) * (g.ofw + 2 * g.opw) + (wo + g.opw)) * 16 + lane0;
  P::store(g.out, out_elem, acc);
  if (IS_MAX) {
    int* const m = static_cast<int*>(g.mask) + (item * ((long long)g.ofh * g.ofw) + pixel) * 16 + lane0;
    bool all = true;
#pragma unroll
    for (int l = 0; l < L; ++l) all = all && (0 <= idx[l]);
    if (all) {
#pragma unroll
      for (int l = 0; l < L; l += 4) *reinterpret_cast<int4*>(m + l) = make_int4(idx[l], idx[l + 1], idx[l + 2], idx[l + 3]);
    }
    else { // a lane no input of which exceeded -FLT_MAX keeps what the mask held
#pragma unroll
      for (int l = 0; l < L; ++l) if (0 <= idx[l]) m[l] = idx[l];
    }
  }
}

// floor(a / b) for b > 0
__device__ __forceinline__ int floor_div(int a, int b) { const int q = a / b; return (a % b < 0) ? q - 1 : q; }

template<bool BF16, bool IS_MAX>
__global__ __launch_bounds__(NTHREADS) void pool_bwd(const PoolArgs g)
{
  typedef Piece<BF16> P;
  constexpr int L = P::LANES;
  long long item; int pixel, lane0;
  if (!locate<L>(g, g.H * g.W, &item, &pixel, &lane0)) return;
  const int hi = pixel / g.W, wi = pixel - hi * g.W;
  // the outputs whose window covers (hi, wi): ho * u - pad_h <= hi <= ho * u - pad_h + R - 1
  int ho0 = floor_div(hi + g.pad_h - g.R, g.u) + 1, ho1 = floor_div(hi + g.pad_h, g.u) + 1;
  int wo0 = floor_div(wi + g.pad_w - g.S, g.v) + 1, wo1 = floor_div(wi + g.pad_w, g.v) + 1;
  ho0 = ho0 < 0 ? 0 : ho0; ho1 = ho1 > g.ofh ? g.ofh : ho1;
  wo0 = wo0 < 0 ? 0 : wo0; wo1 = wo1 > g.ofw ? g.ofw : wo1;
  const int ofwp = g.ofw + 2 * g.opw;
  const long long out_item = item * ((long long)(g.ofh + 2 * g.oph) * ofwp * 16);
  const long long mask_item = item * ((long long)g.ofh * g.ofw * 16);
  const int me = pixel * 16 + lane0;   // what the mask says if this element won
  float acc[L];
#pragma unroll
  for (int l = 0; l < L; ++l) acc[l] = 0.0f;
  for (int ho = ho0; ho < ho1; ++ho) {
    long long elem = out_item + ((long long)(ho + g.oph) * ofwp + (wo0 + g.opw)) * 16 + lane0;
    long long melem = mask_item + ((long long)ho * g.ofw + wo0) * 16 + lane0;
    for (int wo = wo0; wo < wo1; ++wo, elem += 16, melem += 16) {
      float d[L];
      P::load(g.out, elem, d);
      if (IS_MAX) {
        int m[L];
#pragma unroll
        for (int l = 0; l < L; l += 4) {
          const int4 v = *reinterpret_cast<const int4*>(static_cast<const int*>(g.mask) + melem + l);
          m[l] = v.x; m[l + 1] = v.y; m[l + 2] = v.z; m[l + 3] = v.w;
        }
#pragma unroll
        for (int l = 0; l < L; ++l) if (m[l] == me + l) acc[l] = add_rn(acc[l], d[l]);
      }
      else {
#pragma unroll
        for (int l = 0; l < L; ++l) acc[l] = add_rn(acc[l], mul_rn(d[l], g.recp));
      }
    }
  }
  const long long in_elem = item * ((long long)(g.H + 2 * g.iph) * (g.W + 2 * g.ipw) * 16)
    + ((long long)(hi + g.iph) * (g.W + 2 * g.ipw) + (wi + g.ipw)) * 16 + lane0;
  P::store(g.in, in_elem, acc);
}

template<bool BF16, bool IS_MAX>
int launch(const PoolArgs& g, void* stream)
{
  constexpr int PIXELS = NTHREADS / (16 / Piece<BF16>::LANES); // pixels of a work-group
  const long long pixels = g.bwd ? (long long)g.H * g.W : (long long)g.ofh * g.ofw;
  const long long items = (long long)g.w1 - g.w0;
  const long long gx = (pixels + PIXELS - 1) / PIXELS, gy = items < 32768 ? items : 32768, gz = (items + gy - 1) / gy;
  if (pixels < 1 || items < 1 || gx > 0x7fffffffLL || gz > 65535) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
  if (g.bwd) hipLaunchKernelGGL((pool_bwd<BF16, IS_MAX>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((pool_fwd<BF16, IS_MAX>), grid, dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

} // namespace

namespace xsmm {

int launch_pool(const PoolArgs& g, void* stream, const char** name)
{
  static const char* const names[8] = { "pool_fwd_avg_f32", "pool_fwd_max_f32", "pool_fwd_avg_bf16", "pool_fwd_max_bf16",
                                        "pool_bwd_avg_f32", "pool_bwd_max_f32", "pool_bwd_avg_bf16", "pool_bwd_max_bf16" };
  *name = names[(g.bwd ? 4 : 0) + (g.bf16 ? 2 : 0) + (g.is_max ? 1 : 0)];
  if (g.bf16) return g.is_max ? launch<true, true>(g, stream) : launch<true, false>(g, stream);
  return g.is_max ? launch<false, true>(g, stream) : launch<false, false>(g, stream);
}

} // namespace xsmm
