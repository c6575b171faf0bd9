// bn.hip -- the fused batch-norm layer (include/libxsmm_dnn_fusedbatchnorm.h): FWD and BWD on the blocked activations
// [item][row][column][16], item = image * channel blocks + channel block, in fp32 and bf16, as three kernels: the ordered
// partial sums of one (channel block, image) plane, the sum over images with the statistics, and the streaming apply.
//
// The contract (the reference's generic templates, src/template/libxsmm_dnn_fusedbatchnorm_st_{fwd,bwd}_custom_generic.tpl.c):
//   FWD stats  per item and lane sum += x, sumsq += x * x from +0.0 over every pixel of the unpadded plane in row-major order;
//              per channel the images in order from +0.0; mean = recp_nhw * sum, var = recp_nhw * sumsq - mean * mean,
//              rstd = (float)(1.0 / sqrt((double)var + (double)1e-7f)).
//   FWD apply  strided pixels: o = ((gamma * (x - mean)) * rstd) + beta; ELTWISE o += add; RELU o = (o < 0) ? 0 : o.
//   BWD stats  strided pixels in row-major order: RELU dout = (out == 0) ? 0 : dout, stored back; ELTWISE dinput_add = dout;
//              dgamma += ((x - mean) * dout) * rstd, dbeta += dout from +0.0; per channel the images in order from +0.0.
//   BWD apply  strided pixels: din = ((gamma * rstd) * recp_nhw) * (nhw * dout - (dbeta + ((x - mean) * dgamma) * rstd)).
//   bf16       widened by a shift, computed in fp32, stored by truncation.
// Every add, subtract and multiply goes through add_rn / sub_rn / mul_rn of dnn_pixel.cuh, compiled with fp contraction off
// (the compiler's default would fuse them: see there). No instantiation may hold an fp32 fma.
//
// Partial sums. The sums are ordered: per item there are 2 x 16 chains, each as long as the plane, and nothing may be
// reassociated. So moving the bytes is separated from adding them. One work-group owns one plane. All 256 threads fetch
// 16-byte pieces of a chunk of CH consecutive pixels (rows are contiguous only without pad_w, so every piece is addressed from
// its own pixel index), do whatever is independent per element (x * x; in BWD the RELU select with its store back, the
// dinput_add store and ((x - mean) * dout) * rstd) and leave two fp32 values per channel in LDS, [pixel][2][16]. The pieces of
// the next chunk are loaded into registers before the barrier, so they are in flight while 32 lanes of the first wave -- one
// per chain -- add the chunk in pixel order: one LDS read and one dependent add per pixel. Two LDS buffers, one barrier per
// chunk. No atomics, no tree. The partial sums go to the call's own region of the handle's buffer, [touched block][image][2][16].
//
// Apply. As pool.hip: a thread owns a 16-byte piece of one strided pixel, consecutive threads own consecutive pieces, the
// pixel index is decomposed once per thread, the channel scalars of the piece are loaded once into registers, no division per
// element. Items are blockIdx.y/z.
//
// Bounds. A thread touches memory only for a pixel index below the plane's pixel count and an item inside the share (apply) or
// a (touched block, image) pair inside the grid (partial, finish); every address it forms is that of an element inside the
// interior of an item's plane, or of one of the 16 channel scalars of the item's block.
#include <hip/hip_runtime.h>

#include "../xsmm_dnn_internal.hpp"
#include "dnn_pixel.cuh"

namespace {

using xsmm::BnArgs;

constexpr int NTHREADS = 256;
constexpr int CH = 128; // pixels of a chunk of the partial sums: 8 KiB of fp32 pixels, 4 KiB of bf16 ones; 16 KiB of LDS each

// one rounding each, never fused (the pragma covers what is defined from here to the end of the file)
#pragma clang fp contract(off)
using pixel::Piece;
using pixel::add_rn;
using pixel::sub_rn;
using pixel::mul_rn;

// LANES channel scalars of a block, from lane0 on
template<int L>
__device__ __forceinline__ void scalars(const float* p, int fm, int lane0, float (&f)[L])
{
#pragma unroll
  for (int l = 0; l < L; l += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + fm * 16 + lane0 + l);
    f[l] = v.x; f[l + 1] = v.y; f[l + 2] = v.z; f[l + 3] = v.w;
  }
}

// ---- partial sums: one work-group per (touched block, image) ---------------------------------------------------------------
template<bool BF16, bool BWD, bool ELT, bool RELU>
__global__ __launch_bounds__(NTHREADS) void bn_partial(const BnArgs g)
{
  typedef Piece<BF16> P;
  constexpr int L = P::LANES, PP = 16 / L, PER = CH * PP / NTHREADS; // pieces of a pixel; pieces of a chunk per thread (2 / 1)
  __shared__ float lds[2][CH * 32];
  const int tid = (int)threadIdx.x;
  const int j = (int)(blockIdx.x / (unsigned)g.N), img = (int)(blockIdx.x % (unsigned)g.N);
  const int fm = (g.fm0 + j) % g.blocks;
  const long long item = (long long)img * g.blocks + fm;
  const int npix = BWD ? g.ofh * g.ofw : g.H * g.W, row = BWD ? g.ofw : g.W;
  const int ifwp = g.W + 2 * g.ipw, ofwp = g.ofw + 2 * g.opw;
  const long long in_item = item * ((long long)(g.H + 2 * g.iph) * ifwp * 16);
  const long long out_item = item * ((long long)(g.ofh + 2 * g.oph) * ofwp * 16);
  const int lane0 = (tid % PP) * L; // (NTHREADS is a multiple of PP: the same for all pieces of a thread)
  float mean[L], rstd[L];
  if (BWD) { scalars<L>(g.mean, fm, lane0, mean); scalars<L>(g.rstd, fm, lane0, rstd); }

  float x[PER][L], d[PER][L], o[PER][L];   // the pieces in flight (d, o: BWD only)
  long long xe[PER], oe[PER];              // their element offsets
  bool live[PER];

  auto fetch = [&](int chunk) {
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int p = chunk * CH + (tid + r * NTHREADS) / PP;
      live[r] = p < npix;
      if (!live[r]) continue;
      const int a = p / row, b = p - a * row;   // FWD: every input pixel (hi, wi); BWD: output pixel (ho, wo) and input pixel (ho * u, wo * v)
      const int hi = BWD ? a * g.u : a, wi = BWD ? b * g.v : b;
      xe[r] = in_item + ((long long)(hi + g.iph) * ifwp + (wi + g.ipw)) * 16 + lane0;
      P::load(g.in, xe[r], x[r]);
      if (BWD) {
        oe[r] = out_item + ((long long)(a + g.oph) * ofwp + (b + g.opw)) * 16 + lane0;
        P::load(g.dout, oe[r], d[r]);
        if (RELU) P::load(g.out, oe[r], o[r]);
      }
    }
  };
  auto leave = [&](int chunk, float* buf) { // what is independent per element, then [pixel][2][16] in LDS
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      if (!live[r]) continue;
      float* const at = buf + ((tid + r * NTHREADS) / PP) * 32 + lane0;
      float first[L], second[L];
      if (!BWD) {
#pragma unroll
        for (int l = 0; l < L; ++l) { first[l] = x[r][l]; second[l] = mul_rn(x[r][l], x[r][l]); }
      }
      else {
        if (RELU) {
#pragma unroll
          for (int l = 0; l < L; ++l) d[r][l] = (o[r][l] == 0.0f) ? 0.0f : d[r][l];
          P::store(g.dout, oe[r], d[r]);
        }
        if (ELT) P::store(g.add, xe[r], d[r]);
#pragma unroll
        for (int l = 0; l < L; ++l) { first[l] = mul_rn(mul_rn(sub_rn(x[r][l], mean[l]), d[r][l]), rstd[l]); second[l] = d[r][l]; }
      }
#pragma unroll
      for (int l = 0; l < L; l += 4) {
        *reinterpret_cast<float4*>(at + l) = make_float4(first[l], first[l + 1], first[l + 2], first[l + 3]);
        *reinterpret_cast<float4*>(at + 16 + l) = make_float4(second[l], second[l + 1], second[l + 2], second[l + 3]);
      }
    }
    (void)chunk;
  };

  const int nchunks = (npix + CH - 1) / CH;
  float acc = 0.0f; // lanes 0..15: sum / dgamma of channel lane tid; lanes 16..31: sumsq / dbeta of channel lane tid - 16
  fetch(0);
  for (int c = 0; c < nchunks; ++c) {
    float* const buf = lds[c & 1];
    leave(c, buf);
    if (c + 1 < nchunks) fetch(c + 1);  // in flight while the chunk is added
    __syncthreads();                    // the chunk is in LDS; the buffer written next was read before the previous barrier
    if (tid < 32) {
      const int n = (npix - c * CH < CH) ? npix - c * CH : CH;
      const float* const b = buf + tid;
#pragma unroll 8
      for (int p = 0; p < n; ++p) acc = add_rn(acc, b[p * 32]);
    }
  }
  if (tid < 32) g.part[((long long)j * g.N + img) * 32 + tid] = acc;
}

// ---- finish: one wave per touched block; lane l < 32 adds chain l over the images in order -----------------------------------
template<bool BWD>
__global__ __launch_bounds__(64) void bn_finish(const BnArgs g)
{
  const int j = (int)blockIdx.x, l = (int)threadIdx.x;
  const int fm = (g.fm0 + j) % g.blocks;
  float acc = 0.0f;
  if (l < 32) {
    const float* const p = g.part + (long long)j * g.N * 32 + l;
    for (int img = 0; img < g.N; ++img) acc = add_rn(acc, p[(long long)img * 32]);
  }
  if (BWD) {
    if (l < 16) g.dgamma[fm * 16 + l] = acc;
    else if (l < 32) g.dbeta[fm * 16 + l - 16] = acc;
  }
  else {
    const float sumsq = __shfl(acc, (l + 16) & 63);
    if (l < 16) {
      const float mean = mul_rn(g.recp_nhw, acc);
      const float var = sub_rn(mul_rn(g.recp_nhw, sumsq), mul_rn(mean, mean));
      const float rstd = (float)(1.0 / sqrt((double)var + (double)1e-7f));
      g.mean[fm * 16 + l] = mean; g.rstd[fm * 16 + l] = rstd; g.var[fm * 16 + l] = var;
    }
  }
}

// ---- apply: the items [w0, w1), a thread per 16-byte piece of a strided pixel ----------------------------------------------
template<bool BF16, bool BWD, bool ELT, bool RELU>
__global__ __launch_bounds__(NTHREADS) void bn_apply(const BnArgs g)
{
  typedef Piece<BF16> P;
  constexpr int L = P::LANES, PP = 16 / L;
  const long long item = (long long)g.w0 + blockIdx.y + (long long)blockIdx.z * gridDim.y;
  const int p = (int)(blockIdx.x * (NTHREADS / PP) + threadIdx.x / PP);
  const int lane0 = (int)(threadIdx.x % PP) * L;
  if (item >= g.w1 || p >= g.ofh * g.ofw) return;
  const int fm = (int)(item % g.blocks);
  const int ho = p / g.ofw, wo = p - ho * g.ofw;
  const int ifwp = g.W + 2 * g.ipw, ofwp = g.ofw + 2 * g.opw;
  const long long xe = item * ((long long)(g.H + 2 * g.iph) * ifwp * 16) + ((long long)(ho * g.u + g.iph) * ifwp + (wo * g.v + g.ipw)) * 16 + lane0;
  const long long oe = item * ((long long)(g.ofh + 2 * g.oph) * ofwp * 16) + ((long long)(ho + g.oph) * ofwp + (wo + g.opw)) * 16 + lane0;
  float gamma[L], mean[L], rstd[L], x[L], res[L];
  scalars<L>(g.gamma, fm, lane0, gamma); scalars<L>(g.mean, fm, lane0, mean); scalars<L>(g.rstd, fm, lane0, rstd);
  P::load(g.in, xe, x);
  if (!BWD) {
    float beta[L], a[L];
    scalars<L>(g.beta, fm, lane0, beta);
    if (ELT) P::load(g.add, xe, a);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      float v = add_rn(mul_rn(mul_rn(gamma[l], sub_rn(x[l], mean[l])), rstd[l]), beta[l]);
      if (ELT) v = add_rn(v, a[l]);
      if (RELU) v = (v < 0.0f) ? 0.0f : v;
      res[l] = v;
    }
    P::store(g.out, oe, res);
  }
  else {
    float dgamma[L], dbeta[L], d[L];
    scalars<L>(g.dgamma, fm, lane0, dgamma); scalars<L>(g.dbeta, fm, lane0, dbeta);
    P::load(g.dout, oe, d);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const float scale = mul_rn(mul_rn(gamma[l], rstd[l]), g.recp_nhw);
      res[l] = mul_rn(scale, sub_rn(mul_rn(g.nhw, d[l]), add_rn(dbeta[l], mul_rn(mul_rn(sub_rn(x[l], mean[l]), dgamma[l]), rstd[l]))));
    }
    P::store(g.din, xe, res);
  }
}

template<bool BF16, bool BWD, bool ELT, bool RELU>
int partial(const BnArgs& g, void* stream)
{
  const long long groups = (long long)g.nfm * g.N;
  if (groups < 1 || groups > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((bn_partial<BF16, BWD, ELT, RELU>), dim3((unsigned)groups), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

template<bool BF16, bool BWD, bool ELT, bool RELU>
int apply(const BnArgs& g, void* stream)
{
  constexpr int PIXELS = NTHREADS / (16 / Piece<BF16>::LANES); // pixels of a work-group
  const long long pixels = (long long)g.ofh * g.ofw, items = (long long)g.w1 - g.w0;
  const long long gx = (pixels + PIXELS - 1) / PIXELS, gy = items < 32768 ? items : 32768, gz = (items + gy - 1) / gy;
  if (pixels < 1 || items < 1 || gx > 0x7fffffffLL || gz > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((bn_apply<BF16, BWD, ELT, RELU>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(NTHREADS), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

} // namespace

namespace xsmm {

int launch_bn_partial(const BnArgs& g, void* stream, const char** name)
{
  if (!g.bwd) {
    *name = g.bf16 ? "bn_fwd_partial_bf16" : "bn_fwd_partial_f32";
    return g.bf16 ? partial<true, false, false, false>(g, stream) : partial<false, false, false, false>(g, stream);
  }
  *name = g.bf16 ? "bn_bwd_partial_bf16" : "bn_bwd_partial_f32";
  switch ((g.bf16 ? 4 : 0) + (g.eltwise ? 2 : 0) + (g.relu ? 1 : 0)) {
    case 0: return partial<false, true, false, false>(g, stream);
    case 1: return partial<false, true, false, true>(g, stream);
    case 2: return partial<false, true, true, false>(g, stream);
    case 3: return partial<false, true, true, true>(g, stream);
    case 4: return partial<true, true, false, false>(g, stream);
    case 5: return partial<true, true, false, true>(g, stream);
    case 6: return partial<true, true, true, false>(g, stream);
    default: return partial<true, true, true, true>(g, stream);
  }
}

int launch_bn_finish(const BnArgs& g, void* stream, const char** name)
{
  *name = g.bwd ? "bn_bwd_finish" : "bn_fwd_finish";
  if (g.nfm < 1) return (int)hipErrorInvalidValue;
  if (g.bwd) hipLaunchKernelGGL(bn_finish<true>, dim3((unsigned)g.nfm), dim3(64), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(bn_finish<false>, dim3((unsigned)g.nfm), dim3(64), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_bn_apply(const BnArgs& g, void* stream, const char** name)
{
  if (g.bwd) {
    *name = g.bf16 ? "bn_bwd_apply_bf16" : "bn_bwd_apply_f32";
    return g.bf16 ? apply<true, true, false, false>(g, stream) : apply<false, true, false, false>(g, stream);
  }
  *name = g.bf16 ? "bn_fwd_apply_bf16" : "bn_fwd_apply_f32";
  switch ((g.bf16 ? 4 : 0) + (g.eltwise ? 2 : 0) + (g.relu ? 1 : 0)) {
    case 0: return apply<false, false, false, false>(g, stream);
    case 1: return apply<false, false, false, true>(g, stream);
    case 2: return apply<false, false, true, false>(g, stream);
    case 3: return apply<false, false, true, true>(g, stream);
    case 4: return apply<true, false, false, false>(g, stream);
    case 5: return apply<true, false, false, true>(g, stream);
    case 6: return apply<true, false, true, false>(g, stream);
    default: return apply<true, false, true, true>(g, stream);
  }
}

} // namespace xsmm
