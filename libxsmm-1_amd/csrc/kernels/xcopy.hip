// kernels/xcopy.hip -- matrix copy and transposition (libxsmm_matcopy / otrans / itrans and the stack forms of libxsmm_amd.h).
//
// Pre-compiled kernels with run-time extents: the work is pure data movement, a shape baked into the text buys
// nothing the memory system would notice, and a copy must not wait for a compiler. Everything moves as unsigned integers of
// 1, 2, 4, 8 or 16 bytes ("units"): no value ever passes through a floating-point type. Offsets are 64-bit throughout.
//
//   xcopy_trans_tile   one large matrix, element = unit: T x T tiles through LDS; both global sides run along their fast
//                      dimension, 16 bytes per lane where base and pitch allow (VI / VO, chosen per launch and per side)
//   xcopy_itrans_tile  in place, square: the two tiles of a pair across the diagonal are read, then written to each other's place
//   xcopy_copy         rows of bytes with two pitches (or zeros), 16 bytes per lane where bases and pitches allow
//   xcopy_stack_trans  a stack of small items: a work-group moves whole items through LDS (as many as fit 16 KiB), both global
//                      sides in the order the items lie in memory; elements may consist of P units (any typesize)
//   xcopy_generic      without LDS, an index per unit: stack copy / zero fill, transposition of items too large for LDS,
//                      in-place swap of elements that are not a native unit
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"

namespace xsmm {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template<int B> struct UnitOf;
template<> struct UnitOf<1> { typedef unsigned char T; };
template<> struct UnitOf<2> { typedef unsigned short T; };
template<> struct UnitOf<4> { typedef unsigned int T; };
template<> struct UnitOf<8> { typedef unsigned long long T; };
template<> struct UnitOf<16> { typedef u32x4 T; };

// ---- tiles ---------------------------------------------------------------------------------------------------------------
// A tile in LDS is [column][row] with PITCH elements per column. 64 banks of 4 bytes: the fill runs along a column
// (consecutive addresses), the transposed read walks across columns, PITCH * sizeof(E) bytes apart; with PITCH * sizeof(E) / 4
// odd (elements up to 4 bytes: 68, 132, 260 bytes) or an odd number of elements (8 and 16 bytes) the lanes of one LDS
// instruction fall into different banks on both sides.
template<typename E> struct Tile {
  static constexpr int T = (sizeof(E) <= 4 ? 64 : 32);
  static constexpr int PITCH = T + (sizeof(E) >= 4 ? 1 : 4 / (int)sizeof(E));
  static constexpr int VFULL = 16 / (int)sizeof(E);
};

template<typename E, int V> union Vec { u32x4 v; E e[V]; };

// rows [0, mi) x columns [0, nj) of the matrix at src (columns ld elements apart) -> tile
template<typename E, int V> __device__ __forceinline__ void tile_load(E* tile, const E* __restrict__ src, long long ld, int mi, int nj)
{
  constexpr int T = Tile<E>::T, P = Tile<E>::PITCH, TV = T / V;
#pragma unroll 4
  for (int idx = (int)threadIdx.x; idx < TV * T; idx += 256) {
    const int i = (idx % TV) * V, j = idx / TV;
    if (j < nj && i < mi) {
      const E* const p = src + (long long)j * ld + i;
      if (V > 1 && i + V <= mi) {
        Vec<E, V> x; x.v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int q = 0; q < V; ++q) tile[j * P + i + q] = x.e[q];
      }
      else {
#pragma unroll
        for (int q = 0; q < V; ++q) if (i + q < mi) tile[j * P + i + q] = p[q];
      }
    }
  }
}

// tile -> its transpose at dst: dst[i * ld + j] = tile[j][i] for i < mi, j < nj
template<typename E, int V> __device__ __forceinline__ void tile_store_t(const E* tile, E* __restrict__ dst, long long ld, int mi, int nj)
{
  constexpr int T = Tile<E>::T, P = Tile<E>::PITCH, TV = T / V;
#pragma unroll 4
  for (int idx = (int)threadIdx.x; idx < TV * T; idx += 256) {
    const int j = (idx % TV) * V, i = idx / TV;
    if (i < mi && j < nj) {
      E* const p = dst + (long long)i * ld + j;
      if (V > 1 && j + V <= nj) {
        Vec<E, V> x;
#pragma unroll
        for (int q = 0; q < V; ++q) x.e[q] = tile[(j + q) * P + i];
        *reinterpret_cast<u32x4*>(p) = x.v;
      }
      else {
#pragma unroll
        for (int q = 0; q < V; ++q) if (j + q < nj) p[q] = tile[(j + q) * P + i];
      }
    }
  }
}

template<typename E, int VI, int VO> __global__ __launch_bounds__(256) void xcopy_trans_tile(const E* __restrict__ in, E* __restrict__ out,
  int m, int n, long long ldi, long long ldo, int ntm, long long ntiles)
{
  constexpr int T = Tile<E>::T;
  __shared__ __attribute__((aligned(16))) E tile[T * Tile<E>::PITCH];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int i0 = (int)(t % ntm) * T, j0 = (int)(t / ntm) * T;
    const int mi = (m - i0 < T ? m - i0 : T), nj = (n - j0 < T ? n - j0 : T);
    tile_load<E, VI>(tile, in + (long long)j0 * ldi + i0, ldi, mi, nj);
    __syncthreads();
    tile_store_t<E, VO>(tile, out + (long long)i0 * ldo + j0, ldo, mi, nj);
    __syncthreads();
  }
}

template<typename E, int V> __global__ __launch_bounds__(256) void xcopy_itrans_tile(E* a, int n, long long ld, int nt)
{
  constexpr int T = Tile<E>::T;
  __shared__ __attribute__((aligned(16))) E ta[T * Tile<E>::PITCH];
  __shared__ __attribute__((aligned(16))) E tb[T * Tile<E>::PITCH];
  const long long ntiles = (long long)nt * nt;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int bi = (int)(t % nt), bj = (int)(t / nt);
    if (bi > bj) continue; // (the same for the whole work-group) the pair is the work of (bj, bi)
    const int i0 = bi * T, j0 = bj * T;
    const int mi = (n - i0 < T ? n - i0 : T), nj = (n - j0 < T ? n - j0 : T);
    E* const pa = a + (long long)j0 * ld + i0; // rows i0 ..., columns j0 ...
    E* const pb = a + (long long)i0 * ld + j0; // rows j0 ..., columns i0 ...
    tile_load<E, V>(ta, pa, ld, mi, nj);
    if (bi != bj) tile_load<E, V>(tb, pb, ld, nj, mi);
    __syncthreads();
    tile_store_t<E, V>(ta, pb, ld, mi, nj);
    if (bi != bj) tile_store_t<E, V>(tb, pa, ld, nj, mi);
    __syncthreads();
  }
}

// ---- rows of bytes -------------------------------------------------------------------------------------------------------
// Column j: rowbytes bytes from in + j * pin to out + j * pout (in == nullptr: zeros), as rowbytes / sizeof(E) units and a tail
// of single bytes. A work-group is 2^lx lanes along the row by 256 >> lx columns; a lane moves up to four units.
template<typename E> __global__ __launch_bounds__(256) void xcopy_copy(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
  long long rowbytes, long long ncols, long long pin, long long pout, int lx)
{
  constexpr int W = (int)sizeof(E);
  const long long nv = rowbytes / W, per = nv + (rowbytes - nv * W);
  const int TX = 1 << lx, TY = 256 >> lx;
  const int tx = (int)threadIdx.x & (TX - 1), ty = (int)threadIdx.x >> lx;
  for (long long j = (long long)blockIdx.y * TY + ty; j < ncols; j += (long long)gridDim.y * TY) {
    const unsigned char* const pi = (nullptr != in ? in + j * pin : nullptr);
    unsigned char* const po = out + j * pout;
    const long long x0 = (long long)blockIdx.x * (TX * 4) + tx;
    E v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long x = x0 + u * TX;
      v[u] = E{};
      if (x < nv && nullptr != pi) v[u] = reinterpret_cast<const E*>(pi)[x];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long x = x0 + u * TX;
      if (x < nv) reinterpret_cast<E*>(po)[x] = v[u];
      else if (x < per) { const long long b = nv * W + (x - nv); po[b] = (nullptr != pi ? pi[b] : (unsigned char)0); }
    }
  }
}

// ---- stacks --------------------------------------------------------------------------------------------------------------
// An index that counts through (d0, d1, d2, d3) with extents (e0, e1, e2, -), advanced by a fixed step without a division.
struct Odo { int d0, d1, d2; long long d3; };
__device__ __forceinline__ void odo_add(Odo& o, const Odo& s, int e0, int e1, int e2)
{
  o.d0 += s.d0; int c = (o.d0 >= e0 ? 1 : 0); o.d0 -= (0 != c ? e0 : 0);
  o.d1 += s.d1 + c; c = (o.d1 >= e1 ? 1 : 0); o.d1 -= (0 != c ? e1 : 0);
  o.d2 += s.d2 + c; c = (o.d2 >= e2 ? 1 : 0); o.d2 -= (0 != c ? e2 : 0);
  o.d3 += s.d3 + c;
}
__device__ __forceinline__ Odo odo_of(long long idx, int e0, int e1, int e2)
{
  Odo o;
  o.d0 = (int)(idx % e0); idx /= e0;
  o.d1 = (int)(idx % e1); idx /= e1;
  o.d2 = (int)(idx % e2); o.d3 = idx / e2;
  return o;
}

template<typename E> __device__ __forceinline__ E* item_of(const void* base, long long stride, int ptrs, long long g)
{
  return (0 != ptrs) ? static_cast<E* const*>(base)[g] : const_cast<E*>(static_cast<const E*>(base)) + g * stride;
}

extern __shared__ __attribute__((aligned(16))) unsigned char xcopy_lds[];

// Items of m x n elements of P units each. A chunk of up to G items is read in the order it lies in memory (unit x of column
// j of item g) into LDS images with mp units per column, then written in the order the output lies in memory (unit p of
// element (i, j) at out[i * ldo + j * P + p]). Every item is complete in LDS before any of it is written: out == in is fine.
template<typename E> __global__ __launch_bounds__(256) void xcopy_stack_trans(StackMove a)
{
  E* const lds = reinterpret_cast<E*>(xcopy_lds);
  const int mP = a.m * a.P, iteml = a.n * a.mp;
  const Odo t1 = odo_of(threadIdx.x, mP, a.n, 1 << 30), t2 = odo_of(threadIdx.x, a.P, a.n, a.m);
  const Odo s1 = { a.s1[0], a.s1[1], a.s1[2], 0 }, s2 = { a.s2[0], a.s2[1], a.s2[2], a.s2[3] };
  const long long nchunks = (a.batch + a.G - 1) / a.G;
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long long g0 = c * a.G;
    const int ng = (int)(a.batch - g0 < a.G ? a.batch - g0 : a.G);
    const int total = ng * a.n * mP;
    Odo o = t1; // (x, j, g)
#pragma unroll 4
    for (int idx = (int)threadIdx.x; idx < total; idx += 256) {
      const E* const src = item_of<E>(a.in, a.sin, a.ptrs, g0 + o.d2);
      lds[o.d2 * iteml + o.d1 * a.mp + o.d0] = src[(long long)o.d1 * a.ldi + o.d0];
      odo_add(o, s1, mP, a.n, 1 << 30);
    }
    __syncthreads();
    o = t2; // (p, j, i, g)
#pragma unroll 4
    for (int idx = (int)threadIdx.x; idx < total; idx += 256) {
      E* const dst = item_of<E>(a.out, a.sout, a.ptrs, g0 + o.d3);
      dst[(long long)o.d2 * a.ldo + o.d1 * a.P + o.d0] = lds[(int)o.d3 * iteml + o.d1 * a.mp + o.d2 * a.P + o.d0];
      odo_add(o, s2, a.P, a.n, a.m);
    }
    __syncthreads();
  }
}

// OP 0: out[i * ldo + j * P + p] = in[j * ldi + i * P + p], index (p, j, i, g)
// OP 1: out[j * ldo + x] = in[j * ldi + x] (in == nullptr: zeros), index (x, j, -, g) with x < m * P
// OP 2: in place, m == n: the units of elements (i, j) and (j, i) change places for i < j, index (p, j, i, g)
template<typename E, int OP> __global__ __launch_bounds__(256) void xcopy_generic(StackMove a)
{
  const int e0 = (1 == OP ? a.m * a.P : a.P), e1 = a.n, e2 = (1 == OP ? 1 : a.m);
  const long long total = a.batch * e2 * e1 * e0;
  const long long step = (long long)gridDim.x * 256;
  const Odo s = { a.s2[0], a.s2[1], a.s2[2], a.sg };
  long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  Odo o = odo_of(idx, e0, e1, e2);
  for (; idx < total; idx += step) {
    E* const dst = item_of<E>(a.out, a.sout, a.ptrs, o.d3);
    if (0 == OP) {
      const E* const src = item_of<E>(a.in, a.sin, a.ptrs, o.d3);
      dst[(long long)o.d2 * a.ldo + o.d1 * a.P + o.d0] = src[(long long)o.d1 * a.ldi + o.d2 * a.P + o.d0];
    }
    else if (1 == OP) {
      E v = E{};
      if (nullptr != a.in) v = item_of<E>(a.in, a.sin, a.ptrs, o.d3)[(long long)o.d1 * a.ldi + o.d0];
      dst[(long long)o.d1 * a.ldo + o.d0] = v;
    }
    else if (o.d2 < o.d1) {
      E* const x = dst + (long long)o.d1 * a.ldo + o.d2 * a.P + o.d0;
      E* const y = dst + (long long)o.d2 * a.ldo + o.d1 * a.P + o.d0;
      const E vx = *x, vy = *y;
      *x = vy; *y = vx;
    }
    odo_add(o, s, e0, e1, e2);
  }
}

// idx = d0 + e0 * (d1 + e1 * (d2 + e2 * d3))
void decompose(long long idx, int e0, int e1, int e2, int d[3], long long* d3)
{
  d[0] = (int)(idx % e0); idx /= e0;
  d[1] = (int)(idx % e1); idx /= e1;
  d[2] = (int)(idx % e2); *d3 = idx / e2;
}

template<typename E> int trans_tile(const void* in, void* out, int m, int n, long long ldi, long long ldo, bool vi, bool vo, hipStream_t st)
{
  constexpr int T = Tile<E>::T, VF = Tile<E>::VFULL;
  const int ntm = (m + T - 1) / T;
  const long long ntiles = (long long)ntm * ((n + T - 1) / T);
  const unsigned blocks = (unsigned)(ntiles < (1LL << 22) ? ntiles : (1LL << 22));
  const E* const pi = static_cast<const E*>(in); E* const po = static_cast<E*>(out);
  if (vi && vo) hipLaunchKernelGGL((xcopy_trans_tile<E, VF, VF>), dim3(blocks), dim3(256), 0, st, pi, po, m, n, ldi, ldo, ntm, ntiles);
  else if (vi) hipLaunchKernelGGL((xcopy_trans_tile<E, VF, 1>), dim3(blocks), dim3(256), 0, st, pi, po, m, n, ldi, ldo, ntm, ntiles);
  else if (vo) hipLaunchKernelGGL((xcopy_trans_tile<E, 1, VF>), dim3(blocks), dim3(256), 0, st, pi, po, m, n, ldi, ldo, ntm, ntiles);
  else hipLaunchKernelGGL((xcopy_trans_tile<E, 1, 1>), dim3(blocks), dim3(256), 0, st, pi, po, m, n, ldi, ldo, ntm, ntiles);
  return (int)hipGetLastError();
}

template<typename E> int itrans_tile(void* inout, int n, long long ld, bool vec, hipStream_t st)
{
  constexpr int T = Tile<E>::T, VF = Tile<E>::VFULL;
  const int nt = (n + T - 1) / T;
  const long long ntiles = (long long)nt * nt;
  const unsigned blocks = (unsigned)(ntiles < (1LL << 22) ? ntiles : (1LL << 22));
  if (vec) hipLaunchKernelGGL((xcopy_itrans_tile<E, VF>), dim3(blocks), dim3(256), 0, st, static_cast<E*>(inout), n, ld, nt);
  else hipLaunchKernelGGL((xcopy_itrans_tile<E, 1>), dim3(blocks), dim3(256), 0, st, static_cast<E*>(inout), n, ld, nt);
  return (int)hipGetLastError();
}

template<typename E> int copy_rows(const void* in, void* out, long long rowbytes, long long ncols, long long pin, long long pout, hipStream_t st)
{
  const long long nv = rowbytes / (long long)sizeof(E), per = nv + (rowbytes - nv * (long long)sizeof(E));
  int lx = 0;
  while (lx < 8 && (1LL << lx) * 4 < per) ++lx;
  const int TX = 1 << lx, TY = 256 >> lx;
  const long long bx = (per + TX * 4 - 1) / (TX * 4), by = (ncols + TY - 1) / TY;
  if (bx > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((xcopy_copy<E>), dim3((unsigned)bx, (unsigned)(by < 65535 ? by : 65535)), dim3(256), 0, st,
    static_cast<const unsigned char*>(in), static_cast<unsigned char*>(out), rowbytes, ncols, pin, pout, lx);
  return (int)hipGetLastError();
}

template<typename E> int stack_any(StackMove a, int op, hipStream_t st, const char** name)
{
  if (XCOPY_STACK_TRANS == op && 0 < a.G) { // through LDS
    const int mP = a.m * a.P;
    long long d3 = 0;
    decompose(256, mP, a.n, 1 << 30, a.s1, &d3);
    decompose(256, a.P, a.n, a.m, a.s2, &d3); a.s2[3] = (int)d3;
    const long long nchunks = (a.batch + a.G - 1) / a.G;
    const unsigned blocks = (unsigned)(nchunks < 16384 ? nchunks : 16384);
    const size_t lds_bytes = (size_t)a.G * a.n * a.mp * sizeof(E);
    *name = "xcopy_stack_trans";
    hipLaunchKernelGGL((xcopy_stack_trans<E>), dim3(blocks), dim3(256), lds_bytes, st, a);
    return (int)hipGetLastError();
  }
  const int e0 = (XCOPY_STACK_COPY == op ? a.m * a.P : a.P), e1 = a.n, e2 = (XCOPY_STACK_COPY == op ? 1 : a.m);
  const long long total = a.batch * e2 * e1 * e0;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  decompose(blocks * 256, e0, e1, e2, a.s2, &a.sg);
  if (XCOPY_STACK_TRANS == op) { *name = "xcopy_generic_trans"; hipLaunchKernelGGL((xcopy_generic<E, 0>), dim3((unsigned)blocks), dim3(256), 0, st, a); }
  else if (XCOPY_STACK_COPY == op) { *name = "xcopy_generic_copy"; hipLaunchKernelGGL((xcopy_generic<E, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a); }
  else { *name = "xcopy_generic_swap"; hipLaunchKernelGGL((xcopy_generic<E, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a); }
  return (int)hipGetLastError();
}

} // namespace

#define XCOPY_BY_UNIT(UNIT, CALL) \
  switch (UNIT) { \
    case 1: { typedef UnitOf<1>::T E; return CALL; } \
    case 2: { typedef UnitOf<2>::T E; return CALL; } \
    case 4: { typedef UnitOf<4>::T E; return CALL; } \
    case 8: { typedef UnitOf<8>::T E; return CALL; } \
    case 16: { typedef UnitOf<16>::T E; return CALL; } \
    default: return (int)hipErrorInvalidValue; \
  }

int launch_xcopy_trans(int unit, const void* in, void* out, int m, int n, long long ldi, long long ldo, bool vec_in, bool vec_out, void* stream)
{
  XCOPY_BY_UNIT(unit, (trans_tile<E>(in, out, m, n, ldi, ldo, vec_in, vec_out, (hipStream_t)stream)))
}

int launch_xcopy_itrans(int unit, void* inout, int n, long long ld, bool vec, void* stream)
{
  XCOPY_BY_UNIT(unit, (itrans_tile<E>(inout, n, ld, vec, (hipStream_t)stream)))
}

int launch_xcopy_copy(int unit, const void* in, void* out, long long rowbytes, long long ncols, long long pitch_in, long long pitch_out, void* stream)
{
  XCOPY_BY_UNIT(unit, (copy_rows<E>(in, out, rowbytes, ncols, pitch_in, pitch_out, (hipStream_t)stream)))
}

int launch_xcopy_stack(int unit, const StackMove& args, int op, void* stream, const char** name)
{
  XCOPY_BY_UNIT(unit, (stack_any<E>(args, op, (hipStream_t)stream, name)))
}

} // namespace xsmm
