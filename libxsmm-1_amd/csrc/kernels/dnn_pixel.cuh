// dnn_pixel.cuh -- what the kernels of the DNN layers on blocked activations share (pool.hip, bn.hip): the 16-byte piece of a
// 16-channel pixel, and fp32 arithmetic of one rounding each.
//
// A pixel's 16 channels are contiguous: 64 bytes in fp32, 32 in bf16. A thread owns a 16-byte piece of it: four lanes in fp32,
// eight in bf16, widened by a shift, computed in fp32 and stored by truncation.
//
// Every add, subtract and multiply of those kernels goes through add_rn / sub_rn / mul_rn, compiled with fp contraction off. The
// __fadd_rn / __fmul_rn intrinsics are not enough: they are plain operators in the HIP headers, and the compiler's default
// (contract = fast) turned add_rn(acc, mul_rn(d, recp)) into v_pk_fma_f32 -- other bits than the reference's. The pragma covers
// what is defined from it to the end of the including file; a file that includes this header repeats it for its own code.
#ifndef XSMM_DNN_PIXEL_CUH
#define XSMM_DNN_PIXEL_CUH

#include <hip/hip_runtime.h>

namespace pixel {

#pragma clang fp contract(off)
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }

template<bool BF16> struct Piece;
template<> struct Piece<false> {      // four fp32 lanes
  static constexpr int LANES = 4;
  static __device__ __forceinline__ void load(const void* base, long long elem, float (&f)[4])
  {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(base) + elem);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
  static __device__ __forceinline__ void store(void* base, long long elem, const float (&f)[4])
  {
    *reinterpret_cast<float4*>(static_cast<float*>(base) + elem) = make_float4(f[0], f[1], f[2], f[3]);
  }
};
template<> struct Piece<true> {       // eight bf16 lanes
  static constexpr int LANES = 8;
  static __device__ __forceinline__ void load(const void* base, long long elem, float (&f)[8])
  {
    const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(base) + elem);
    const unsigned int w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void store(void* base, long long elem, const float (&f)[8])
  {
    unsigned int w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (__float_as_uint(f[2 * i]) >> 16) | (__float_as_uint(f[2 * i + 1]) & 0xffff0000u);
    *reinterpret_cast<uint4*>(static_cast<unsigned short*>(base) + elem) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

} // namespace pixel

#endif
