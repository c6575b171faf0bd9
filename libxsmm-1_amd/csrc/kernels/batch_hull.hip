// batch_hull.hip -- address hulls of batch calls (gfx950): for every recorded libxsmm_gemm_batch call the lowest and the
// highest byte address its A, B and C operands touch, reduced on the device over the call's index or pointer arrays.
//
// Batch calls recorded inside a libxsmm_amd_defer_begin/end bracket leave as fused launches whose groups run side by side
// (xsmm_batch_record.cpp: batch_flush_record), which is only right for calls that neither write the same C blocks nor read what
// another one writes. Where the arrays live in host memory the host forms the hulls while it stages them; arrays in device
// memory are walked here -- 12 bytes per product, read once, coalesced (consecutive lanes take consecutive entries).
#include "smm_common.cuh"

#include <cstring>

namespace xsmm {

namespace {

constexpr int HULL_CALLS = BATCH_HULL_CALLS, HULL_CALL_BLOCKS = 16;
struct HullCall {
  const char* base[3]; const char* idx[3];  // A, B, C: matrix base / pointer array; index array (ADDR_INDEX, NULL: one shared operand)
  long long stride[3];                      // ADDR_POINTER: byte distance between pointers (0: one shared operand)
  unsigned long long span[3];               // bytes one operand occupies
  long long batch;
  int index_base, index_stride, mode, typesize;
};
struct HullCalls { HullCall g[HULL_CALLS]; };
static_assert(sizeof(HullCalls) + sizeof(void*) <= 4096, "passed by value");

// out: [3 * HULL_CALLS] lowest addresses (initialised to all ones), then [3 * HULL_CALLS] highest addresses, spans included
// (initialised to zero); entry 3 * call + operand. A wave reduces its lanes' values across the lanes and issues one atomic per
// operand and direction.
__global__ __launch_bounds__(256) void batch_hull_kernel(HullCalls tab, unsigned long long* out)
{
  const unsigned call = blockIdx.x / HULL_CALL_BLOCKS, bid = blockIdx.x % HULL_CALL_BLOCKS;
  const HullCall& g = tab.g[call];
  unsigned long long lo[3] = { ~0ULL, ~0ULL, ~0ULL }, hi[3] = { 0, 0, 0 };
  for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < g.batch; i += (long long)HULL_CALL_BLOCKS * blockDim.x) {
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      unsigned long long p;
      if (ADDR_INDEX == g.mode) {
        p = reinterpret_cast<unsigned long long>(g.base[o]);
        if (nullptr != g.idx[o]) {
          const int v = *reinterpret_cast<const int*>(g.idx[o] + i * (long long)g.index_stride);
          p += (unsigned long long)(((long long)v - g.index_base) * (long long)g.typesize);
        }
      }
      else p = *reinterpret_cast<const unsigned long long*>(g.base[o] + i * g.stride[o]); // ADDR_POINTER
      lo[o] = (p < lo[o]) ? p : lo[o];
      hi[o] = (p > hi[o]) ? p : hi[o];
    }
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long l = __shfl_xor(lo[o], d), h = __shfl_xor(hi[o], d);
      lo[o] = (l < lo[o]) ? l : lo[o];
      hi[o] = (h > hi[o]) ? h : hi[o];
    }
  }
  if (0 == (threadIdx.x & 63) && lo[0] <= hi[0]) { // (a wave without an item has nothing to say)
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      atomicMin(out + 3 * call + o, lo[o]);
      atomicMax(out + 3 * HULL_CALLS + 3 * call + o, hi[o] + g.span[o]);
    }
  }
}

} // namespace

int launch_batch_hulls(const SmmBatch* calls, const unsigned long long* span_bytes, int ncalls, unsigned long long* d_out, void* stream)
{
  if (ncalls < 1 || ncalls > HULL_CALLS || nullptr == d_out) return -1;
  HullCalls tab; memset(&tab, 0, sizeof(tab));
  for (int c = 0; c < ncalls; ++c) {
    const SmmBatch& s = calls[c];
    if ((ADDR_INDEX != s.mode && ADDR_POINTER != s.mode) || s.batch < 1) return -1;
    HullCall& g = tab.g[c];
    g.base[0] = (const char*)s.a; g.base[1] = (const char*)s.b; g.base[2] = (const char*)s.c;
    g.idx[0] = (const char*)s.ia; g.idx[1] = (const char*)s.ib; g.idx[2] = (const char*)s.ic;
    g.stride[0] = s.sa; g.stride[1] = s.sb; g.stride[2] = s.sc;
    for (int o = 0; o < 3; ++o) g.span[o] = span_bytes[3 * c + o];
    g.batch = s.batch; g.index_base = s.index_base; g.index_stride = s.index_stride; g.mode = s.mode; g.typesize = s.typesize;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t plane = sizeof(unsigned long long) * 3 * HULL_CALLS;
  hipError_t e = hipMemsetAsync(d_out, 0xFF, plane, st);
  if (hipSuccess == e) e = hipMemsetAsync(d_out + 3 * HULL_CALLS, 0, plane, st);
  if (hipSuccess != e) return (int)e;
  hipLaunchKernelGGL(batch_hull_kernel, dim3((unsigned)(ncalls * HULL_CALL_BLOCKS)), dim3(256), 0, st, tab, d_out);
  return (int)hipGetLastError();
}

} // namespace xsmm
