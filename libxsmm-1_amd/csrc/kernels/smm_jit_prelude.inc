// smm_jit_prelude.inc -- what every generated dense SMM kernel shares and no shape changes: the address space of the operand accesses
// (XFLAT), batch addressing, the arithmetic instructions by type, the LDS synchronisation. Stands once behind kernels/smm_jit_geom.h
// (DevAddr) at file scope, in front of the form's own text (a grouped text: in front of all per-shape namespaces).
#if XFLAT
#define XGLOBAL
#else
#define XGLOBAL __attribute__((address_space(1)))
#endif
// ---- batch addressing (DevAddr: kernels/smm_jit_geom.h) ----
template<typename P> __device__ __forceinline__ P* resolve(const char* base, const char* idx, long long stride, const DevAddr& ad, long long i)
{
  if (0 == ad.mode) return (P*)base + i * stride;
  if (1 == ad.mode) { if (nullptr == idx) return (P*)base; const int v = *(const XGLOBAL int*)(idx + i * (long long)ad.index_stride); return (P*)base + ((long long)v - ad.index_base); }
  return *(P* const XGLOBAL*)(base + i * stride);
}
__device__ __forceinline__ float xfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double xfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
typedef short xs16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int xfma(int a, int b, int c) { return __builtin_amdgcn_sdot2(__builtin_bit_cast(xs16x2, a), __builtin_bit_cast(xs16x2, b), c, false); } // two i16 x i16 products + i32, wrapping
__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the matrix-core instructions (k-ordered fma chains, tools/probe/mfma_f64_chain.hip) and their accumulators
typedef float ACC32 __attribute__((ext_vector_type(4)));
typedef double ACC64 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ACC32 xmfma(float a, float b, ACC32 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ ACC64 xmfma(double a, double b, ACC64 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < hi ? v : hi; }
__device__ __forceinline__ void xatomic_add(double* p, double v) { (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double*)p, v); }
__device__ __forceinline__ void xatomic_add(float* p, float v) { (void)__builtin_amdgcn_global_atomic_fadd_f32((__attribute__((address_space(1))) float*)p, v); }
// Work-group barrier that orders LDS traffic only. __syncthreads() carries a work-group-scope fence, which on gfx9 drains
// vmcnt -- i.e. every global load in flight, the whole register ring of prefetched products -- before each s_barrier and
// turns the D-deep prefetch into depth one (measured: 2.2 us per 32^3 product instead of well under one).
__device__ __forceinline__ void lds_barrier()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

