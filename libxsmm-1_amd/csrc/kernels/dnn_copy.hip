// kernels/dnn_copy.hip -- libxsmm_dnn_copyin_tensor / _copyout_tensor for operands the GPU reaches (include/libxsmm_dnn_tensor.h).
//
// Reference: src/template/libxsmm_dnn_tensor_{buffer_copy_{in,out}_nchw,filter_copy_{in,out}_kcrs,bias_copy_{in,out}_nchw}.tpl.c --
// permutations of 2- or 4-byte elements, nothing is rounded. The geometry is kernels/dnn_copy_plan.h: a tile of a
// block is rows x run positions; it travels through LDS as [row][pitch], is moved along its rows on the plain side and along
// its contiguous pieces on the blocked side, 16 bytes per lane where the call's bases, runs and pitches allow (vp, vb: elements
// per access of the plain and of the blocked side, 16 / sizeof(T) or 1). Copy-in and copy-out are one text: IN says which of
// the two sides is read. Element offsets are 64-bit, offsets within a tile are int.
//
//   dnn_copy_tiled<T, IN>    a work-group per tile, grid-stride over the tiles
//   dnn_copy_direct<T, IN>   a row that does not fit the LDS budget: an element per lane and trip, coalesced on the plain side
//   dnn_copy_flat<T>         the same order on both sides (channel tensors, activations of one pixel)
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"
#include "dnn_copy_plan.h"

namespace xsmm {
namespace {

template<typename T> struct alignas(16) Pack { T e[16 / sizeof(T)]; };

// the rows of a tile between the plain side and LDS; LOAD: memory -> LDS
template<typename T, bool LOAD>
__device__ __forceinline__ void rows_side(T* __restrict__ prow, T* __restrict__ tile, const DnnCopyGeom& g, const DnnCopyTile& t, int vp)
{
  constexpr int V = 16 / sizeof(T);
  const int units = dnn_copy_row_units(t, vp);
  for (int u = threadIdx.x; u < units; u += DNN_COPY_THREADS) {
    int jj, l, cnt;
    dnn_copy_row_unit(t, vp, u, &jj, &l, &cnt);
    T* const gp = prow + (long long)jj * g.rowpitch + l;
    T* const lp = tile + jj * g.pitch + l;
    if (V == cnt) {
      Pack<T> x;
      if (LOAD) {
        x = *reinterpret_cast<const Pack<T>*>(gp);
#pragma unroll
        for (int k = 0; k < V; ++k) lp[k] = x.e[k];
      }
      else {
#pragma unroll
        for (int k = 0; k < V; ++k) x.e[k] = lp[k];
        *reinterpret_cast<Pack<T>*>(gp) = x;
      }
    }
    else {
      for (int k = 0; k < cnt; ++k) { if (LOAD) lp[k] = gp[k]; else gp[k] = lp[k]; }
    }
  }
}

// the contiguous pieces of a tile between the blocked side and LDS; LOAD: memory -> LDS
template<typename T, bool LOAD>
__device__ __forceinline__ void permuted_side(T* __restrict__ bpc, T* __restrict__ tile, const DnnCopyGeom& g, const DnnCopyTile& t, int vb)
{
  constexpr int V = 16 / sizeof(T);
  const int units = dnn_copy_piece_units(t, vb);
  for (int u = threadIdx.x; u < units; u += DNN_COPY_THREADS) {
    int piece, e, cnt;
    dnn_copy_piece_unit(t, vb, u, &piece, &e, &cnt);
    T* const gp = bpc + piece * t.piece_step + e;
    DnnCopyCursor c = dnn_copy_cursor(g, t, piece, e);
    if (V == cnt) {
      Pack<T> x;
      if (LOAD) x = *reinterpret_cast<const Pack<T>*>(gp);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        T& w = tile[dnn_copy_lds_of(g, t, c)];
        if (LOAD) w = x.e[k]; else x.e[k] = w;
        dnn_copy_advance(g, t, c);
      }
      if (!LOAD) *reinterpret_cast<Pack<T>*>(gp) = x;
    }
    else {
      for (int k = 0; k < cnt; ++k) {
        T& w = tile[dnn_copy_lds_of(g, t, c)];
        if (LOAD) w = gp[k]; else gp[k] = w;
        dnn_copy_advance(g, t, c);
      }
    }
  }
}

template<typename T, bool IN>
__global__ __launch_bounds__(DNN_COPY_THREADS) void dnn_copy_tiled(T* __restrict__ blocked, T* __restrict__ plain, const DnnCopyGeom g, int vp, int vb)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char dnn_copy_smem[];
  T* const tile = reinterpret_cast<T*>(dnn_copy_smem);
  for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const DnnCopyTile t = dnn_copy_tile(g, item);
    if (IN) rows_side<T, true>(plain + t.plain0, tile, g, t, vp); else permuted_side<T, true>(blocked + t.blocked0, tile, g, t, vb);
    __syncthreads();
    if (IN) permuted_side<T, false>(blocked + t.blocked0, tile, g, t, vb); else rows_side<T, false>(plain + t.plain0, tile, g, t, vp);
    __syncthreads();
  }
}

template<typename T, bool IN>
__global__ __launch_bounds__(DNN_COPY_THREADS) void dnn_copy_direct(T* __restrict__ blocked, T* __restrict__ plain, const DnnCopyGeom g)
{
  const long long per = g.J * g.L, nthreads = (long long)gridDim.x * DNN_COPY_THREADS;
  for (long long i = (long long)blockIdx.x * DNN_COPY_THREADS + threadIdx.x; i < g.total; i += nthreads) {
    const long long blk = i / per, r = i % per, j = r / g.L, l = r % g.L;
    T* const p = plain + dnn_copy_plain_block(g, blk) + j * g.rowpitch + l;
    T* const b = blocked + blk * per + dnn_copy_blocked_of(g, j, l);
    if (IN) *b = *p; else *p = *b;
  }
}

template<typename T>
__global__ __launch_bounds__(DNN_COPY_THREADS) void dnn_copy_flat(const T* __restrict__ in, T* __restrict__ out, long long n, int vec)
{
  constexpr int V = 16 / sizeof(T);
  const long long units = (0 != vec ? n / V : 0), tail0 = units * V;
  const long long tid = (long long)blockIdx.x * DNN_COPY_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * DNN_COPY_THREADS;
  for (long long q = tid; q < units; q += nthreads) reinterpret_cast<Pack<T>*>(out)[q] = reinterpret_cast<const Pack<T>*>(in)[q];
  for (long long i = tail0 + tid; i < n; i += nthreads) out[i] = in[i];
}

template<typename T> int launch_t(const DnnCopyGeom& g, void* blocked_, void* plain_, bool in, hipStream_t st, const char** name)
{
  T* const blocked = static_cast<T*>(blocked_);
  T* const plain = static_cast<T*>(plain_);
  const bool ab = (0 == reinterpret_cast<uintptr_t>(blocked) % 16), ap = (0 == reinterpret_cast<uintptr_t>(plain) % 16);
  const dim3 grid((unsigned)g.grid), block(DNN_COPY_THREADS);
  if (DNN_COPY_FLAT == g.form) {
    *name = "dnn_copy_flat";
    hipLaunchKernelGGL(dnn_copy_flat<T>, grid, block, 0, st, in ? plain : blocked, in ? blocked : plain, g.total, (ab && ap) ? 1 : 0);
  }
  else if (0 == g.lds) {
    *name = in ? "dnn_copy_in_direct" : "dnn_copy_out_direct";
    if (in) hipLaunchKernelGGL((dnn_copy_direct<T, true>), grid, block, 0, st, blocked, plain, g);
    else hipLaunchKernelGGL((dnn_copy_direct<T, false>), grid, block, 0, st, blocked, plain, g);
  }
  else {
    const int vp = dnn_copy_plain_width(g, ap), vb = dnn_copy_blocked_width(g, ab);
    *name = in ? "dnn_copy_in_tiled" : "dnn_copy_out_tiled";
    if (in) hipLaunchKernelGGL((dnn_copy_tiled<T, true>), grid, block, (unsigned)g.lds_bytes, st, blocked, plain, g, vp, vb);
    else hipLaunchKernelGGL((dnn_copy_tiled<T, false>), grid, block, (unsigned)g.lds_bytes, st, blocked, plain, g, vp, vb);
  }
  return (int)hipGetLastError();
}

} // namespace

int launch_dnn_copy(const DnnCopyGeom& g, void* blocked, void* plain, bool in, void* stream, const char** name)
{
  if (4 == g.ts) return launch_t<unsigned int>(g, blocked, plain, in, (hipStream_t)stream, name);
  if (2 == g.ts) return launch_t<unsigned short>(g, blocked, plain, in, (hipStream_t)stream, name);
  return (int)hipErrorInvalidValue;
}

} // namespace xsmm
