// kernels/hash.hip -- libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n on operands in device memory
// (include/libxsmm.h, include/libxsmm_amd.h). The definition and the algebra are restated in kernels/hash_plan.h and DESIGN.md 8u.
//
// Reference: src/libxsmm_hash.c (CRC-32C), src/libxsmm_diff.c, src/libxsmm_diff.h:76-98. Both jobs are streams bound by HBM. A
// wave takes a byte range: the bytes up to the first multiple of 16 and the bytes after the last whole word go one by one, lane l
// takes the 16-byte words l, l + 64, ... in between with one load each. For the hash a lane keeps crc(0, its words with the gaps
// between them as zeros): state = adv(state, 1024) ^ crc(0, word), sixteen look-ups of the slicing-by-four tables and four of the
// tables of the fixed advance, all eight (8 KiB) copied into LDS when the kernel starts. At the end of the range a lane multiplies
// by x^(128 * words after its last one), the wave XORs by butterflies, and what came before the range (the seed, the bytes in
// front of the first word) was folded into the first four bytes of word 0. XOR has no order: every split gives the same bits.
// The compare keeps the OR of the XORed words instead and needs no table.
//
//   hash_items<CMP>   the batch forms, items up to HASH_ITEM_MAX bytes: a wave per item, line after line, the grid strides
//   hash_units<CMP>   one large item: its lines cut into units (hash_plan.h), waves take units in turn and carry their value
//                     forward by the distance between two units; one partial per work-group
//   hash_close<CMP>   one work-group: the partials, the seed advanced by the length, the result; the lowest differing item
//   hash_first        the lowest differing item as the caller sees it (-1: none)
//   diff_n            libxsmm_diff_n: a thread per item of at most 255 bytes, the nearest match after the hint by atomicMin
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"
#include "hash_plan.h"

namespace xsmm {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__constant__ HashTables HASH_TABLES = hash_tables();
__constant__ HashPowers HASH_POWERS = hash_powers();

constexpr long long FIRST_NONE = 0x7f7f7f7f7f7f7f7fLL; // what hipMemsetAsync(0x7f) leaves

struct HashLds { uint32_t t[4 * 256]; uint32_t adv[4 * 256]; };

__device__ __forceinline__ void tables_to_lds(HashLds& lds)
{ // 2048 entries, 256 threads: two loads of 16 bytes each (every thread calls; a barrier follows)
  const u32x4* const src = reinterpret_cast<const u32x4*>(&HASH_TABLES);
  u32x4* const dst = reinterpret_cast<u32x4*>(&lds);
  dst[threadIdx.x] = src[threadIdx.x];
  dst[threadIdx.x + HASH_THREADS] = src[threadIdx.x + HASH_THREADS];
}

__device__ __forceinline__ uint64_t uniform(uint64_t x)
{ // the same in every lane of the wave: say so, loops over it are scalar then
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t x)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x ^= __shfl_xor(x, o, 64);
  return x;
}

// crc(init, the n bytes at p), the same in every lane. p and n are the same in every lane; all 64 lanes call.
__device__ __forceinline__ uint32_t wave_hash(const HashLds& lds, const unsigned char* p, uint64_t n, uint32_t init, int lane)
{
  const HashParts parts = hash_parts(reinterpret_cast<uint64_t>(p), n);
  uint32_t v = init;
  for (unsigned int k = 0; k < parts.head; ++k) v = hash_byte(lds.t, v, p[k]);
  if (0 != parts.words) {
    const u32x4* const w = reinterpret_cast<const u32x4*>(p + parts.head);
    uint32_t state = 0;
    uint64_t i = (uint64_t)lane;
    if (i < parts.words) { // the first word of every lane; what came before the words enters word 0
      u32x4 x = w[i];
      x.x ^= (0 == lane ? v : 0u);
      state = hash_word(lds.t, x.x, x.y, x.z, x.w);
      i += 64;
    }
    for (; i + 192 < parts.words; i += 256) { // four loads in flight
      const u32x4 x0 = w[i], x1 = w[i + 64], x2 = w[i + 128], x3 = w[i + 192];
      state = hash_adv_pass(lds.adv, state) ^ hash_word(lds.t, x0.x, x0.y, x0.z, x0.w);
      state = hash_adv_pass(lds.adv, state) ^ hash_word(lds.t, x1.x, x1.y, x1.z, x1.w);
      state = hash_adv_pass(lds.adv, state) ^ hash_word(lds.t, x2.x, x2.y, x2.z, x2.w);
      state = hash_adv_pass(lds.adv, state) ^ hash_word(lds.t, x3.x, x3.y, x3.z, x3.w);
    }
    for (; i < parts.words; i += 64) {
      const u32x4 x = w[i];
      state = hash_adv_pass(lds.adv, state) ^ hash_word(lds.t, x.x, x.y, x.z, x.w);
    }
    const int rest = hash_lane_rest(parts.words, lane);
    state = (0 <= rest ? hash_gfmul(state, HASH_POWERS.lane[rest]) : 0u);
    v = wave_xor(state);
  }
  const unsigned char* const tail = p + parts.head + parts.words * HASH_WORD;
  for (unsigned int k = 0; k < parts.tail; ++k) v = hash_byte(lds.t, v, tail[k]);
  return v;
}

// non-zero if the n bytes at a and at b differ, the same in every lane. The split follows a: its words are loaded aligned, those
// of b by a 16-byte load of any alignment (the hardware's unaligned access; no byte outside the range is read).
__device__ __forceinline__ uint32_t wave_cmp(const unsigned char* a, const unsigned char* b, uint64_t n, int lane)
{
  const HashParts parts = hash_parts(reinterpret_cast<uint64_t>(a), n);
  uint32_t d = 0;
  for (unsigned int k = 0; k < parts.head; ++k) d |= (uint32_t)(a[k] ^ b[k]);
  const u32x4* const wa = reinterpret_cast<const u32x4*>(a + parts.head);
  const unsigned char* const wb = b + parts.head;
  for (uint64_t i = (uint64_t)lane; i < parts.words; i += 64) {
    const u32x4 x = wa[i];
    u32x4 y;
    __builtin_memcpy(&y, wb + i * HASH_WORD, HASH_WORD);
    d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
  }
  const uint64_t done = parts.head + parts.words * HASH_WORD;
  for (unsigned int k = 0; k < parts.tail; ++k) d |= (uint32_t)(a[done + k] ^ b[done + k]);
  return 0 != __ballot(0 != d) ? 1u : 0u;
}

// ---- a wave per item -------------------------------------------------------------------------------------------------------
template<bool CMP>
__global__ __launch_bounds__(HASH_THREADS) void hash_items_kernel(HashArgs a, unsigned int* results, long long* first)
{
  __shared__ HashLds lds;
  if (!CMP) { tables_to_lds(lds); __syncthreads(); }
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * HASH_WAVES;
  const unsigned char* const pa = static_cast<const unsigned char*>(a.a);
  const unsigned char* const pb = static_cast<const unsigned char*>(a.b);
  for (long long item = (long long)uniform((uint64_t)((long long)blockIdx.x * HASH_WAVES + (threadIdx.x >> 6))); item < a.batch; item += waves) {
    uint32_t v = CMP ? 0u : a.seed;
    for (long long line = 0; line < a.lines; ++line) {
      const unsigned char* const la = pa + item * a.stride_a + line * a.lda;
      if (CMP) v |= wave_cmp(la, pb + item * a.stride_b + line * a.ldb, a.line_bytes, lane);
      else v = wave_hash(lds, la, a.line_bytes, v, lane);
    }
    if (0 == lane) {
      results[item] = v;
      if (CMP && 0 != v && nullptr != first) atomicMin(first, a.item0 + item);
    }
  }
}

// ---- the units of one large item ---------------------------------------------------------------------------------------------
template<bool CMP>
__global__ __launch_bounds__(HASH_THREADS) void hash_units_kernel(HashArgs a, HashPlan plan, unsigned int* partial)
{
  __shared__ HashLds lds;
  __shared__ uint32_t wave_value[HASH_WAVES];
  if (!CMP) tables_to_lds(lds);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long waves = (long long)gridDim.x * HASH_WAVES;
  const unsigned char* const pa = static_cast<const unsigned char*>(a.a);
  const unsigned char* const pb = static_cast<const unsigned char*>(a.b);
  uint32_t acc = 0, mult = HASH_ONE;
  uint64_t acc_end = 0, mult_gap = 0; // acc is crc(0, the wave's units so far with zeros between them) up to byte acc_end of the item
  for (long long u = (long long)uniform((uint64_t)((long long)blockIdx.x * HASH_WAVES + wave)); u < plan.units; u += waves) {
    const long long line = u / plan.per_line, part = u % plan.per_line;
    const unsigned char* const la = pa + line * a.lda;
    const HashRange r = hash_unit(plan, reinterpret_cast<uint64_t>(la), a.line_bytes, part);
    if (CMP) acc |= wave_cmp(la + r.begin, pb + line * a.ldb + r.begin, r.end - r.begin, lane);
    else {
      const uint64_t end = (uint64_t)line * a.line_bytes + r.end;
      if (0 != acc) {
        if (end - acc_end != mult_gap) { mult_gap = end - acc_end; mult = hash_xpow(HASH_POWERS.pow2, mult_gap); }
        acc = hash_gfmul(acc, mult);
      }
      acc ^= wave_hash(lds, la + r.begin, r.end - r.begin, 0u, lane);
      acc_end = end;
    }
  }
  if (!CMP) acc = hash_adv(HASH_POWERS.pow2, acc, a.line_bytes * (uint64_t)a.lines - acc_end);
  if (0 == lane) wave_value[wave] = acc;
  __syncthreads();
  if (0 == threadIdx.x) {
#pragma unroll
    for (int w = 1; w < HASH_WAVES; ++w) acc = CMP ? (acc | wave_value[w]) : (acc ^ wave_value[w]);
    partial[blockIdx.x] = acc;
  }
}

template<bool CMP>
__global__ __launch_bounds__(HASH_THREADS) void hash_close_kernel(HashArgs a, const unsigned int* partial, int count, unsigned int* result, long long* first)
{
  __shared__ uint32_t wave_value[HASH_WAVES];
  uint32_t v = 0;
  for (int g = threadIdx.x; g < count; g += HASH_THREADS) v = CMP ? (v | partial[g]) : (v ^ partial[g]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_xor(v, o, 64); v = CMP ? (v | x) : (v ^ x); }
  if (0 == (threadIdx.x & 63)) wave_value[threadIdx.x >> 6] = v;
  __syncthreads();
  if (0 == threadIdx.x) {
#pragma unroll
    for (int w = 1; w < HASH_WAVES; ++w) v = CMP ? (v | wave_value[w]) : (v ^ wave_value[w]);
    if (CMP) {
      *result = (0 != v ? 1u : 0u);
      if (0 != v && nullptr != first) atomicMin(first, a.item0);
    }
    else *result = v ^ hash_adv(HASH_POWERS.pow2, a.seed, a.line_bytes * (uint64_t)a.lines);
  }
}

__global__ void hash_first_kernel(const long long* first, long long* out) { *out = (FIRST_NONE == *first ? -1 : *first); }

// ---- libxsmm_diff_n --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HASH_THREADS) void diff_n_kernel(DiffKey key, const unsigned char* a, const unsigned char* bn, unsigned int size, unsigned int stride,
  unsigned int hint, unsigned int n, unsigned int* best)
{
  __shared__ unsigned char k[256];
  k[threadIdx.x] = (nullptr != a ? (threadIdx.x < size ? a[threadIdx.x] : (unsigned char)0) : key.b[threadIdx.x]);
  __syncthreads();
  unsigned int m = 0xffffffffu; // the distance from the hint, going round
  const uint64_t step = (uint64_t)gridDim.x * HASH_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * HASH_THREADS + threadIdx.x; i < n; i += step) {
    const unsigned char* const p = bn + i * stride;
    unsigned int d = 0;
    for (unsigned int j = 0; j < size; ++j) d |= (unsigned int)(p[j] ^ k[j]);
    if (0 == d) {
      const unsigned int r = (unsigned int)(i >= hint ? i - hint : i + n - hint);
      if (r < m) m = r;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const unsigned int x = __shfl_xor(m, o, 64); if (x < m) m = x; }
  if (0 == (threadIdx.x & 63) && 0xffffffffu != m) atomicMin(best, m);
}

} // namespace

int launch_hash_items(const HashArgs& a, unsigned int* results, long long* first, void* stream)
{
  const dim3 grid((unsigned)hash_items_grid(a.batch)), block(HASH_THREADS);
  if (0 != a.compare) hipLaunchKernelGGL(hash_items_kernel<true>, grid, block, 0, (hipStream_t)stream, a, results, first);
  else hipLaunchKernelGGL(hash_items_kernel<false>, grid, block, 0, (hipStream_t)stream, a, results, first);
  return (int)hipGetLastError();
}

int launch_hash_units(const HashArgs& a, unsigned int* partial, unsigned int* result, long long* first, void* stream)
{
  const HashPlan plan = hash_plan(a.line_bytes, a.lines);
  const dim3 grid((unsigned)plan.grid), block(HASH_THREADS), one(1);
  if (0 != a.compare) {
    hipLaunchKernelGGL(hash_units_kernel<true>, grid, block, 0, (hipStream_t)stream, a, plan, partial);
    hipLaunchKernelGGL(hash_close_kernel<true>, one, block, 0, (hipStream_t)stream, a, partial, plan.grid, result, first);
  }
  else {
    hipLaunchKernelGGL(hash_units_kernel<false>, grid, block, 0, (hipStream_t)stream, a, plan, partial);
    hipLaunchKernelGGL(hash_close_kernel<false>, one, block, 0, (hipStream_t)stream, a, partial, plan.grid, result, first);
  }
  return (int)hipGetLastError();
}

int launch_hash_first(long long* first, long long* out, bool clear, void* stream)
{
  if (clear) return (int)hipMemsetAsync(first, 0x7f, sizeof(*first), (hipStream_t)stream);
  hipLaunchKernelGGL(hash_first_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, first, out);
  return (int)hipGetLastError();
}

int launch_diff_n(const DiffKey& key, const void* a, const void* bn, unsigned int size, unsigned int stride, unsigned int hint, unsigned int n,
  unsigned int* best, void* stream)
{
  const hipError_t e = hipMemsetAsync(best, 0xff, sizeof(*best), (hipStream_t)stream);
  if (hipSuccess != e) return (int)e;
  long long blocks = ((long long)n + HASH_THREADS - 1) / HASH_THREADS;
  if (blocks > HASH_MAX_BLOCKS) blocks = HASH_MAX_BLOCKS;
  hipLaunchKernelGGL(diff_n_kernel, dim3((unsigned)blocks), dim3(HASH_THREADS), 0, (hipStream_t)stream, key, static_cast<const unsigned char*>(a),
    static_cast<const unsigned char*>(bn), size, stride, hint, n, best);
  return (int)hipGetLastError();
}

} // namespace xsmm
