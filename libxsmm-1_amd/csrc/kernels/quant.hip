// kernels/quant.hip -- fp32 -> int16 quantisation, its inverse, and the fp32 -> bf16 converters (include/libxsmm_dnn.h).
//
// Reference: src/libxsmm_dnn.c:2394-2907. Everything here is a stream bound by HBM: grid-stride loops over at
// most QUANT_MAX_BLOCKS work-groups, 64-bit element indices, four elements per lane and step -- 16 bytes of fp32, 8 bytes of
// 16-bit data -- wherever the address allows, element by element in front of and behind that. The arithmetic is integer bit
// manipulation (and, for FPHW_ROUND, one fp32 product that is never contracted), so the results equal the reference's bits.
//
//   quant_absmax        largest (bits & 0x7fffffff) of a tensor: lane, wave, work-group, one atomic maximum per work-group
//   quant_flat<MODE>    out[i] = q(in[i]); derives max_exp / scfq from the maximum word itself, one lane writes the scf byte
//   quant_act<MODE>     output walked linearly, source index by the fi* maps (:2616-2634), pairs of shorts as one 32-bit store
//   quant_act_tiled     plain input (cblk_f32 == 1): 64 pixels x up to 64 channels turned through LDS
//   quant_fil<MODE>     as quant_act with the maps of :2741-2762
//   dequant_flat, bf16_truncate, bf16_rnaz, bf16_rne   element-wise
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"

namespace xsmm {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int QUANT_THREADS = 256;
constexpr int QUANT_MAX_BLOCKS = 2048;     // 256 CUs x 8 work-groups: the rest of a tensor is walked by the grid-stride loops

__device__ __forceinline__ unsigned f2u(float x) { return __float_as_uint(x); }
__device__ __forceinline__ float u2f(unsigned x) { return __uint_as_float(x); }

// libxsmm_sexp2_i8 (src/libxsmm_math.c:489-513): 2^x, with 2^-127 as the denormal 1 / 2^127 and the constant 0x200000 for -128
__device__ __forceinline__ float sexp2_i8(int x /* -128 ... 127 */)
{
  return u2f(-128 == x ? 0x200000u : (-127 == x ? 0x400000u : (unsigned)(x + 127) << 23));
}

// the exponent frexpf gives for a non-negative finite float (0 for 0); denormals by their leading bit
__device__ __forceinline__ int frexp_exponent(unsigned bits)
{
  const unsigned e = bits >> 23;
  if (0 != e) return (int)e - 126;
  return 0 == bits ? 0 : (31 - __clz((int)bits)) - 148;
}

// roundf: halves away from zero, exactly (x + 0.5f is wrong next to a half)
__device__ __forceinline__ float round_away(float x)
{
  float t = truncf(x);
  if (fabsf(x - t) >= 0.5f) t += copysignf(1.f, x); // (x - t is exact: both share an exponent or |x| < 1)
  return t;
}

// counter-based generator: 32 bits out of (seed, element index); the finaliser of MurmurHash3 over both halves of the index
__device__ __forceinline__ unsigned mix32(unsigned h)
{
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ float uniform01(unsigned seed, unsigned long long idx)
{
  const unsigned h = mix32(mix32((unsigned)idx ^ seed) + 0x9e3779b9u * (unsigned)(idx >> 32) + 0x7f4a7c15u);
  return (float)(h >> 8) / 16777215.f; // [0, 1], both ends included, as rand() / RAND_MAX
}

// ---- the element operations ---------------------------------------------------------------------------------------------
// What every lane of a quantise kernel derives from the maximum word (wave-uniform), and the map of one element.
template<int MODE> struct QuantOp {
  float scfq; unsigned max_exp, add_shift, seed;
  __device__ __forceinline__ void init(const QuantHead& h)
  {
    const unsigned maxbits = *h.maxword;
    unsigned char scf;
    add_shift = h.add_shift; seed = h.seed; scfq = 0.f; max_exp = 0;
    if (QUANT_FPHW == MODE) { // :2525-2530, :2558
      const int maxexp = frexp_exponent(maxbits) - (15 - (int)h.add_shift);
      scfq = sexp2_i8((int)(signed char)(-maxexp));
      scf = (unsigned char)(-maxexp);
    }
    else { // :2435, :2575
      max_exp = (maxbits >> 23) & 0xffu;
      scf = (unsigned char)(14 - (int)h.add_shift - ((int)max_exp - 127));
    }
    if (0 == blockIdx.x && 0 == threadIdx.x) *h.scf = scf;
  }
  __device__ __forceinline__ unsigned short operator()(float input, unsigned long long idx) const
  {
    if (QUANT_FPHW == MODE) { // (short)roundf(in * scfq): float -> int32 (the x86 conversion: out of range gives 0x80000000) -> low 16 bits
      const float t = round_away(__fmul_rn(input, scfq));
      const int q = (fabsf(t) < 2147483648.f) ? (int)t : (int)0x80000000u;
      return (unsigned short)q;
    }
    // libxsmm_internal_quantize_scalar_no_scf (:2441-2515)
    if (input == 0.f) return 0;
    const unsigned ui = f2u(input);
    const unsigned exp_off = (max_exp - ((ui & 0x7fffffffu) >> 23)) & 0xffu;
    const unsigned mant = 0x800000u | (ui & 0x007fffffu);
    unsigned rhs = (24u - 15u + exp_off + add_shift) & 0xffu;
    if (rhs > 24u) rhs = 24u;
    unsigned qvalue = mant >> rhs;
    if (0 != (ui >> 31) && qvalue > 0) qvalue = ~qvalue + 1u;
    if (QUANT_BIAS == MODE) { // (a shift count below zero: what the x86 shift does, the count modulo 32)
      if (0 < (int)(mant & (3u << ((rhs - 2u) & 31u)))) ++qvalue;
    }
    else if (QUANT_NEAREST == MODE) {
      if (0 < (int)(mant & (1u << ((rhs - 1u) & 31u))) && rhs > 1u) ++qvalue;
    }
    else if (QUANT_STOCH == MODE) { // :2494-2508 with p from the counter-based generator
      const float eps = 1.f / 32768.f; // LIXSMMM_DNN_RES_DFP16
      const float fvalue = u2f(ui & (0xffffffffu << rhs));
      const float p = uniform01(seed, idx);
      const float q = __fdiv_rn(__fsub_rn(input, fvalue), eps);
      if (__fadd_rn(p, q) > 0.5f) ++qvalue;
    }
    return (unsigned short)qvalue;
  }
};

struct DequantOp { float scale; __device__ __forceinline__ float operator()(unsigned short x, unsigned long long) const { return __fmul_rn((float)(short)x, scale); } };
struct TruncOp { __device__ __forceinline__ unsigned short operator()(float x, unsigned long long) const { return (unsigned short)(f2u(x) >> 16); } };
struct RnazOp { __device__ __forceinline__ unsigned short operator()(float x, unsigned long long) const
  { unsigned u = f2u(x); if (0x7f800000u != (u & 0x7f800000u)) u += 0x8000u; return (unsigned short)(u >> 16); } };
struct RneOp { __device__ __forceinline__ unsigned short operator()(float x, unsigned long long) const
  { unsigned u = f2u(x); if (0x7f800000u != (u & 0x7f800000u)) u += 0x7fffu + ((u >> 16) & 1u); return (unsigned short)(u >> 16); } };

// ---- four elements at a time ----------------------------------------------------------------------------------------------
template<typename T> struct Quad;
template<> struct Quad<float> { // 16 bytes
  float e[4];
  __device__ __forceinline__ void load(const float* p, bool vec)
  { if (vec) { const u32x4 v = *reinterpret_cast<const u32x4*>(p); e[0] = u2f(v.x); e[1] = u2f(v.y); e[2] = u2f(v.z); e[3] = u2f(v.w); }
    else { e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; e[3] = p[3]; } }
  __device__ __forceinline__ void store(float* p, bool vec) const
  { if (vec) { u32x4 v; v.x = f2u(e[0]); v.y = f2u(e[1]); v.z = f2u(e[2]); v.w = f2u(e[3]); *reinterpret_cast<u32x4*>(p) = v; }
    else { p[0] = e[0]; p[1] = e[1]; p[2] = e[2]; p[3] = e[3]; } }
};
template<> struct Quad<unsigned short> { // 8 bytes
  unsigned short e[4];
  __device__ __forceinline__ void load(const unsigned short* p, bool vec)
  { if (vec) { const u32x2 v = *reinterpret_cast<const u32x2*>(p); e[0] = (unsigned short)v.x; e[1] = (unsigned short)(v.x >> 16); e[2] = (unsigned short)v.y; e[3] = (unsigned short)(v.y >> 16); }
    else { e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; e[3] = p[3]; } }
  __device__ __forceinline__ void store(unsigned short* p, bool vec) const
  { if (vec) { u32x2 v; v.x = (unsigned)e[0] | ((unsigned)e[1] << 16); v.y = (unsigned)e[2] | ((unsigned)e[3] << 16); *reinterpret_cast<u32x2*>(p) = v; }
    else { p[0] = e[0]; p[1] = e[1]; p[2] = e[2]; p[3] = e[3]; } }
};

// out[i] = op(in[i], i) for i < n: `head` elements one by one, then quads (vin / vout: that side of a quad is aligned to its
// 16 or 8 bytes), then the last n - head - 4 * nquads elements one by one. head < 4 and the tail < 4: the first lanes take them.
template<typename TI, typename TO, typename OP>
__device__ __forceinline__ void stream_map(const TI* __restrict__ in, TO* __restrict__ out, long long n, int head, bool vin, bool vout, const OP& op)
{
  const long long nquads = (n - head) / 4, tail0 = head + 4 * nquads;
  const long long tid = (long long)blockIdx.x * QUANT_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * QUANT_THREADS;
  if (tid < head) out[tid] = op(in[tid], (unsigned long long)tid);
  if (tid < n - tail0) out[tail0 + tid] = op(in[tail0 + tid], (unsigned long long)(tail0 + tid));
  for (long long q = tid; q < nquads; q += nthreads) {
    const long long i = head + 4 * q;
    Quad<TI> x; Quad<TO> y;
    x.load(in + i, vin);
#pragma unroll
    for (int j = 0; j < 4; ++j) y.e[j] = op(x.e[j], (unsigned long long)(i + j));
    y.store(out + i, vout);
  }
}

template<typename TI, typename TO, typename OP>
__global__ __launch_bounds__(QUANT_THREADS) void map_kernel(const TI* in, TO* out, long long n, int head, int vin, int vout, OP op)
{
  stream_map(in, out, n, head, 0 != vin, 0 != vout, op);
}

template<int MODE>
__global__ __launch_bounds__(QUANT_THREADS) void quant_flat_kernel(const float* in, unsigned short* out, long long n, int head, int vin, int vout, QuantHead h)
{
  QuantOp<MODE> op; op.init(h);
  stream_map(in, out, n, head, 0 != vin, 0 != vout, op);
}

// ---- the maximum ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QUANT_THREADS) void quant_absmax_kernel(const unsigned* in, long long n, int head, int vin, unsigned* maxword)
{
  __shared__ unsigned wave_max[QUANT_THREADS / 64];
  const long long nquads = (n - head) / 4, tail0 = head + 4 * nquads;
  const long long tid = (long long)blockIdx.x * QUANT_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * QUANT_THREADS;
  unsigned m = 0; // (bits & 0x7fffffff) as an unsigned integer: monotonic in |x| for finite x
  if (tid < head) m = in[tid] & 0x7fffffffu;
  if (tid < n - tail0) m = max(m, in[tail0 + tid] & 0x7fffffffu);
  for (long long q = tid; q < nquads; q += nthreads) {
    const unsigned* const p = in + head + 4 * q;
    u32x4 v;
    if (0 != vin) v = *reinterpret_cast<const u32x4*>(p);
    else { v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3]; }
    v &= 0x7fffffffu;
    m = max(max(m, max(v.x, v.y)), max(v.z, v.w));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, s, 64));
  if (0 == (threadIdx.x & 63)) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (0 == threadIdx.x) {
#pragma unroll
    for (int w = 1; w < QUANT_THREADS / 64; ++w) m = max(m, wave_max[w]);
    if (0 != m) atomicMax(maxword, m); // (the word was zeroed on the stream: a maximum does not depend on who comes first)
  }
}

// ---- layouts: the output walked linearly ------------------------------------------------------------------------------------
// IDX: unsigned int while every index fits 31 bits (the divisions are 32-bit then), unsigned long long otherwise
template<typename IDX> __device__ __forceinline__ IDX act_source(IDX o, const QuantLayout& g)
{ // out [N][C/(cb16*lp)][H][W][cb16][lp]; in [N][C/cb32][H][W][cb32] (:2616-2628)
  const IDX cb = (IDX)g.cb16 * g.lp, cin = (IDX)(o % cb); o /= cb;
  const IDX i4 = o % g.W; o /= g.W;
  const IDX i3 = o % g.H; o /= g.H;
  const IDX i2 = o % g.cblk, i1 = o / g.cblk;
  const IDX c = i2 * cb + cin, fi2 = c / g.cb32, fi5 = c % g.cb32;
  return (((i1 * (g.C / g.cb32) + fi2) * g.H + i3) * g.W + i4) * g.cb32 + fi5;
}
template<typename IDX> __device__ __forceinline__ IDX fil_source(IDX o, const QuantLayout& g)
{ // out [K/kb16][C/(cb16*lp)][R][S][cb16][kb16][lp]; in [K/kb32][C/cb32][R][S][cb32][kb32] (:2741-2755; H, W stand for R, S)
  const IDX i7 = o % g.lp; o /= g.lp;
  const IDX i6 = o % g.kb16; o /= g.kb16;
  const IDX i5 = o % g.cb16; o /= g.cb16;
  const IDX i4 = o % g.W; o /= g.W;
  const IDX i3 = o % g.H; o /= g.H;
  const IDX i2 = o % g.cblk, i1 = o / g.cblk;
  const IDX k = i1 * g.kb16 + i6, fi1 = k / g.kb32, fi6 = k % g.kb32;
  const IDX c = (i2 * g.cb16 + i5) * g.lp + i7, fi2 = c / g.cb32, fi5 = c % g.cb32;
  return ((((fi1 * (g.C / g.cb32) + fi2) * g.H + i3) * g.W + i4) * g.cb32 + fi5) * g.kb32 + fi6;
}

// pair: two neighbours of the output (an even total, out aligned to 4 bytes) leave as one 32-bit store. The layout (g.fil) and
// pair are arguments, uniform over the launch, not template parameters: five modes times two index widths are kernels enough.
template<int MODE, typename IDX>
__global__ __launch_bounds__(QUANT_THREADS) void quant_layout_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, QuantLayout g, QuantHead h, int pair)
{
  QuantOp<MODE> op; op.init(h);
  const bool fil = (0 != g.fil);
  const IDX total = (IDX)g.total, width = (0 != pair ? 2 : 1), step = (IDX)gridDim.x * QUANT_THREADS * width;
  for (IDX o = ((IDX)blockIdx.x * QUANT_THREADS + threadIdx.x) * width; o < total; o += step) {
    const unsigned short q0 = op(in[fil ? fil_source<IDX>(o, g) : act_source<IDX>(o, g)], o);
    if (0 != pair) {
      const unsigned short q1 = op(in[fil ? fil_source<IDX>(o + 1, g) : act_source<IDX>(o + 1, g)], o + 1);
      *reinterpret_cast<unsigned*>(out + o) = (unsigned)q0 | ((unsigned)q1 << 16);
    }
    else out[o] = q0;
  }
}

// ---- plain input through LDS --------------------------------------------------------------------------------------------------
// in [N][C][P] (P = H * W pixels: h and w are neighbours on both sides), out [N][C/CB][P][CB] with CB = cb16 * lp channels, CB even
// and out aligned to 4 bytes. A work-group takes 64 pixels of CC <= 64 channels of one (n, channel block): it reads the CC rows
// along the pixels (a wave: 256 contiguous bytes), keeps them as tile[channel][pitch] and writes the [pixel][channel] run, two
// channels per lane as one 32-bit store (a wave: 256 contiguous bytes where CC == CB). Banks (ds_write_b32 and ds_read_b32:
// (address / 4) mod 32 within a half wave): the fill runs along a row, consecutive addresses; the read has lane l at channel
// pair l % (CC/2) of pixel l / (CC/2), address 2 * pitch * (l % (CC/2)) + l / (CC/2): with CC/2 = 2^j <= 16 and
// pitch = 64 + 16 / (CC/2) the 32 lanes of a half wave hit 2 * pitch mod 32 = 32 / (CC/2) apart per pair and 1 apart per pixel
// -- 32 different banks (CB = 16: pitch 66, banks 4 * pair + pixel). Other CC: pitch 65, conflicts on the read side.
constexpr int QT_PIX = 64, QT_CH = 64, QT_PITCH_MAX = 80;
template<int MODE>
__global__ __launch_bounds__(QUANT_THREADS) void quant_act_tiled_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, QuantTiles g, QuantHead h)
{
  __shared__ float tile[QT_CH * QT_PITCH_MAX];
  QuantOp<MODE> op; op.init(h);
  const int lane_p = threadIdx.x % QT_PIX, row0 = threadIdx.x / QT_PIX; // fill: pixel, first channel (4 rows per pass)
  for (long long t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    long long r = t;
    const int chunk = (int)(r % g.chunks); r /= g.chunks;
    const long long ptile = r % g.ptiles; r /= g.ptiles; // r: n * cblk + channel block
    const int c0 = chunk * QT_CH, cc = min(QT_CH, g.CB - c0), half = cc / 2;
    const long long p0 = ptile * QT_PIX;
    const int np = (int)min((long long)QT_PIX, g.P - p0);
    const float* const src = in + (r * g.CB + c0) * g.P + p0;
    if (lane_p < np) {
      for (int c = row0; c < cc; c += QUANT_THREADS / QT_PIX) tile[c * g.pitch + lane_p] = src[(long long)c * g.P + lane_p];
    }
    __syncthreads();
    const long long obase = (r * g.P + p0) * g.CB + c0;
    for (int d = threadIdx.x; d < np * half; d += QUANT_THREADS) {
      const int pix = d / half, pr = d % half;
      const long long o = obase + (long long)pix * g.CB + 2 * pr;
      const unsigned short q0 = op(tile[(2 * pr) * g.pitch + pix], (unsigned long long)o);
      const unsigned short q1 = op(tile[(2 * pr + 1) * g.pitch + pix], (unsigned long long)(o + 1));
      *reinterpret_cast<unsigned*>(out + o) = (unsigned)q0 | ((unsigned)q1 << 16);
    }
    __syncthreads();
  }
}

int blocks_for(long long items_per_thread_units)
{
  const long long b = (items_per_thread_units + QUANT_THREADS - 1) / QUANT_THREADS;
  return (int)(b < 1 ? 1 : (b > QUANT_MAX_BLOCKS ? QUANT_MAX_BLOCKS : b));
}

// elements in front of the first quad so that `in` is aligned to 16 bytes (elements of TI bytes)
template<typename TI, typename TO> void quad_plan(const TI* in, const TO* out, long long n, int* head, int* vin, int* vout)
{
  const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out);
  int hd = (int)(((4 * sizeof(TI) - (ai % (4 * sizeof(TI)))) % (4 * sizeof(TI))) / sizeof(TI));
  if (0 != ai % sizeof(TI)) hd = 0; // (not even element-aligned: nothing is vectorised)
  if (hd > n) hd = (int)n;
  *head = hd;
  *vin = (0 == (ai + hd * sizeof(TI)) % (4 * sizeof(TI))) ? 1 : 0;
  *vout = (0 == (ao + hd * sizeof(TO)) % (4 * sizeof(TO))) ? 1 : 0;
}

template<typename TI, typename TO, typename OP> int launch_map(const TI* in, TO* out, long long n, OP op, void* stream)
{
  int head, vin, vout;
  quad_plan(in, out, n, &head, &vin, &vout);
  hipLaunchKernelGGL((map_kernel<TI, TO, OP>), dim3(blocks_for((n + 3) / 4)), dim3(QUANT_THREADS), 0, (hipStream_t)stream, in, out, n, head, vin, vout, op);
  return (int)hipGetLastError();
}

template<int MODE> int launch_layout_mode(const float* in, unsigned short* out, const QuantLayout& g, const QuantHead& h, hipStream_t st)
{
  const int pair = (0 == g.total % 2 && 0 == g.lp % 2 && 0 == reinterpret_cast<uintptr_t>(out) % 4) ? 1 : 0;
  const dim3 grid(blocks_for(0 != pair ? g.total / 2 : g.total)), block(QUANT_THREADS);
  if (g.total < (1LL << 31)) hipLaunchKernelGGL((quant_layout_kernel<MODE, unsigned int>), grid, block, 0, st, in, out, g, h, pair);
  else hipLaunchKernelGGL((quant_layout_kernel<MODE, unsigned long long>), grid, block, 0, st, in, out, g, h, pair);
  return (int)hipGetLastError();
}

} // namespace

int launch_quant_absmax(const float* in, long long n, unsigned* maxword, void* stream)
{
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(maxword, 0, sizeof(unsigned), st);
  if (hipSuccess != e) return (int)e;
  int head, vin, vout;
  quad_plan(in, in, n, &head, &vin, &vout);
  hipLaunchKernelGGL(quant_absmax_kernel, dim3(blocks_for((n + 3) / 4)), dim3(QUANT_THREADS), 0, st, reinterpret_cast<const unsigned*>(in), n, head, vin, maxword);
  return (int)hipGetLastError();
}

int launch_quant_flat(const float* in, short* out, long long n, const QuantHead& h, void* stream)
{
  int head, vin, vout;
  unsigned short* const o = reinterpret_cast<unsigned short*>(out);
  quad_plan(in, o, n, &head, &vin, &vout);
  const dim3 grid(blocks_for((n + 3) / 4)), block(QUANT_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  switch (h.mode) {
    case QUANT_NO: hipLaunchKernelGGL(quant_flat_kernel<QUANT_NO>, grid, block, 0, st, in, o, n, head, vin, vout, h); break;
    case QUANT_BIAS: hipLaunchKernelGGL(quant_flat_kernel<QUANT_BIAS>, grid, block, 0, st, in, o, n, head, vin, vout, h); break;
    case QUANT_STOCH: hipLaunchKernelGGL(quant_flat_kernel<QUANT_STOCH>, grid, block, 0, st, in, o, n, head, vin, vout, h); break;
    case QUANT_NEAREST: hipLaunchKernelGGL(quant_flat_kernel<QUANT_NEAREST>, grid, block, 0, st, in, o, n, head, vin, vout, h); break;
    case QUANT_FPHW: hipLaunchKernelGGL(quant_flat_kernel<QUANT_FPHW>, grid, block, 0, st, in, o, n, head, vin, vout, h); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_quant_layout(const float* in, short* out, const QuantLayout& g, const QuantHead& h, void* stream)
{
  unsigned short* const o = reinterpret_cast<unsigned short*>(out);
  const hipStream_t st = (hipStream_t)stream;
  switch (h.mode) {
    case QUANT_NO: return launch_layout_mode<QUANT_NO>(in, o, g, h, st);
    case QUANT_BIAS: return launch_layout_mode<QUANT_BIAS>(in, o, g, h, st);
    case QUANT_STOCH: return launch_layout_mode<QUANT_STOCH>(in, o, g, h, st);
    case QUANT_NEAREST: return launch_layout_mode<QUANT_NEAREST>(in, o, g, h, st);
    case QUANT_FPHW: return launch_layout_mode<QUANT_FPHW>(in, o, g, h, st);
    default: return (int)hipErrorInvalidValue;
  }
}

int launch_quant_act_tiled(const float* in, short* out, long long nblocks, int CB, long long P, const QuantHead& h, void* stream)
{
  QuantTiles g;
  g.CB = CB; g.P = P;
  g.chunks = (CB + QT_CH - 1) / QT_CH; g.ptiles = (P + QT_PIX - 1) / QT_PIX;
  g.ntiles = nblocks * g.ptiles * g.chunks;
  const int half = (CB < QT_CH ? CB : QT_CH) / 2;
  g.pitch = QT_PIX + ((0 == (half & (half - 1)) && half <= 16) ? 16 / half : 1); // (see the kernel: banks)
  unsigned short* const o = reinterpret_cast<unsigned short*>(out);
  const dim3 grid((unsigned)(g.ntiles < QUANT_MAX_BLOCKS ? g.ntiles : QUANT_MAX_BLOCKS)), block(QUANT_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  switch (h.mode) {
    case QUANT_NO: hipLaunchKernelGGL(quant_act_tiled_kernel<QUANT_NO>, grid, block, 0, st, in, o, g, h); break;
    case QUANT_BIAS: hipLaunchKernelGGL(quant_act_tiled_kernel<QUANT_BIAS>, grid, block, 0, st, in, o, g, h); break;
    case QUANT_STOCH: hipLaunchKernelGGL(quant_act_tiled_kernel<QUANT_STOCH>, grid, block, 0, st, in, o, g, h); break;
    case QUANT_NEAREST: hipLaunchKernelGGL(quant_act_tiled_kernel<QUANT_NEAREST>, grid, block, 0, st, in, o, g, h); break;
    case QUANT_FPHW: hipLaunchKernelGGL(quant_act_tiled_kernel<QUANT_FPHW>, grid, block, 0, st, in, o, g, h); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_dequant_flat(const short* in, float* out, long long n, float scale, void* stream)
{ DequantOp op; op.scale = scale; return launch_map(reinterpret_cast<const unsigned short*>(in), out, n, op, stream); }

int launch_bf16_narrow(int rounding, const float* in, unsigned short* out, long long n, void* stream)
{
  if (0 == rounding) return launch_map(in, out, n, TruncOp(), stream);
  if (1 == rounding) return launch_map(in, out, n, RnazOp(), stream);
  return launch_map(in, out, n, RneOp(), stream);
}

} // namespace xsmm
