// packed_jit.inc -- the one text of all packed kernels (pgemm, getrf, trmm, trsm; forms 1 and 2), behind the #define block of a
// descriptor (csrc/xsmm_packed.cpp, gen_source): every dimension, flag and alpha is a constant of the text
typedef __attribute__((address_space(1))) T GT;     // T in global memory
typedef __attribute__((address_space(1))) uint4 GV;
#define IDX(i, j, s) (ROWMAJOR ? ((j) + (i) * (s)) : ((i) + (j) * (s)))
#define A_AT(i, j) pa[IDX(i, j, A_S) * VLEN]
#define B_AT(i, j) pb[IDX(i, j, B_S) * VLEN]
#define C_AT(i, j) pc[IDX(i, j, C_S) * VLEN]

__device__ __forceinline__ T xsmm_amul(T x)
{
#if ALPHA_KIND == 0
  return x;
#elif ALPHA_KIND == 1
  return -x;
#else
  return ALPHA_VAL * x;
#endif
}

// The work of one lane on its matrix: pa, pb, pc point at element (0,0) of the lane's matrix, lines A_S / B_S / C_S apart.
// RESIDENT: the triangle / A / the LU matrix in registers, every loop over its indexes unrolled. Otherwise loops that run, on
// the operands where they lie (LDS or global memory). Either way every element sees the same operations in the same order.
// P: T* (images in LDS) or a pointer into the global address space.
template<typename P> __device__ __forceinline__ void xsmm_packed_lane(P __restrict__ pa, P __restrict__ pb, P __restrict__ pc)
{
#if KIND == 3 /* pgemm: C += alpha * op(A) * op(B), every element one fma chain over l = 0 ... k-1 */
#define OPA(i, l) (TRANSA ? A_AT(l, i) : A_AT(i, l))
#define OPB(l, j) (TRANSB ? B_AT(j, l) : B_AT(l, j))
#if RESIDENT
  T ra[M_ * K_];
#pragma unroll
  for (int i = 0; i < M_; ++i) {
#pragma unroll
    for (int l = 0; l < K_; ++l) ra[i * K_ + l] = (1 == ALPHA_KIND ? -OPA(i, l) : OPA(i, l));
  }
#pragma unroll 1
  for (int j = 0; j < N_; ++j) {
    T acc[M_];
#pragma unroll
    for (int i = 0; i < M_; ++i) acc[i] = C_AT(i, j);
#pragma unroll
    for (int l = 0; l < K_; ++l) {
      const T bv = OPB(l, j);
#pragma unroll
      for (int i = 0; i < M_; ++i) acc[i] = XFMA(ra[i * K_ + l], bv, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < M_; ++i) C_AT(i, j) = acc[i];
  }
#else
#pragma unroll 1
  for (int j = 0; j < N_; ++j) {
#pragma unroll 1
    for (int i = 0; i < M_; ++i) {
      T acc = C_AT(i, j);
#pragma unroll 4
      for (int l = 0; l < K_; ++l) acc = XFMA((1 == ALPHA_KIND ? -OPA(i, l) : OPA(i, l)), OPB(l, j), acc);
      C_AT(i, j) = acc;
    }
  }
#endif
#elif KIND == 4 /* getrf: A = L * U in place, no pivoting (right-looking; every element takes its updates in the order of the pivots) */
  (void)pb; (void)pc;
#define MN_ (M_ < N_ ? M_ : N_)
#if RESIDENT
  T w[M_ * N_];
#pragma unroll
  for (int r = 0; r < M_; ++r) {
#pragma unroll
    for (int j = 0; j < N_; ++j) w[r * N_ + j] = A_AT(r, j);
  }
#define W(r, j) w[(r) * N_ + (j)]
#define PK_UNROLL_OUTER _Pragma("unroll")
#define PK_UNROLL_INNER _Pragma("unroll")
#else
#define W(r, j) A_AT(r, j)
#define PK_UNROLL_OUTER _Pragma("unroll 1")
#define PK_UNROLL_INNER _Pragma("unroll 4")
#endif
  PK_UNROLL_OUTER
  for (int c = 0; c < MN_; ++c) {
    const T rinv = (T)1 / W(c, c);
    PK_UNROLL_OUTER
    for (int r = c + 1; r < M_; ++r) {
      const T l = W(r, c) * rinv;
      W(r, c) = l;
      PK_UNROLL_INNER
      for (int j = c + 1; j < N_; ++j) W(r, j) = XFMA(-l, W(c, j), W(r, j));
    }
  }
#if RESIDENT
#pragma unroll
  for (int r = 0; r < M_; ++r) {
#pragma unroll
    for (int j = 0; j < N_; ++j) A_AT(r, j) = w[r * N_ + j];
  }
#endif
#else /* trmm (5), trsm (6): the vectors are the columns (side L) or rows (side R) of B, E = op(A) or its transpose */
  (void)pc;
#define NT_ (SIDE_R ? N_ : M_)
#define NV_ (SIDE_R ? M_ : N_)
#define TEFF ((TRANSA ? 1 : 0) ^ (SIDE_R ? 1 : 0))
#define LOWEFF ((UPPER ? 0 : 1) ^ TEFF)
#define EM(r, c) (TEFF ? A_AT(c, r) : A_AT(r, c))
#define V_AT(r, q) (SIDE_R ? B_AT(q, r) : B_AT(r, q))
#define INTRI(r, c) (LOWEFF ? ((c) < (r)) : ((c) > (r)))
#if RESIDENT
  T te[NT_ * NT_]; // (only the entries of the triangle are ever touched: the others take no register)
#pragma unroll
  for (int r = 0; r < NT_; ++r) {
#pragma unroll
    for (int c = 0; c < NT_; ++c) if (INTRI(r, c)) te[r * NT_ + c] = EM(r, c);
  }
#if !UNITDIAG
  T dg[NT_]; // trsm: the reciprocals of the diagonal; trmm: the diagonal
#pragma unroll
  for (int r = 0; r < NT_; ++r) dg[r] = (6 == KIND ? (T)1 / EM(r, r) : EM(r, r));
#endif
#pragma unroll 1
  for (int q = 0; q < NV_; ++q) {
    T x[NT_];
#if KIND == 6 /* substitution by columns of E: x[c] is final when its turn comes, then leaves every later unknown */
#pragma unroll
    for (int r = 0; r < NT_; ++r) x[r] = xsmm_amul(V_AT(r, q));
#pragma unroll
    for (int cc = 0; cc < NT_; ++cc) {
      const int c = (LOWEFF ? cc : NT_ - 1 - cc);
#if !UNITDIAG
      x[c] = x[c] * dg[c];
#endif
#pragma unroll
      for (int r = 0; r < NT_; ++r) if (INTRI(r, c)) x[r] = XFMA(-te[r * NT_ + c], x[c], x[r]);
    }
#pragma unroll
    for (int r = 0; r < NT_; ++r) V_AT(r, q) = x[r];
#else /* the diagonal term first, then the row of the triangle from left to right */
    T y[NT_];
#pragma unroll
    for (int r = 0; r < NT_; ++r) x[r] = V_AT(r, q);
#pragma unroll
    for (int r = 0; r < NT_; ++r) {
#if UNITDIAG
      T s = x[r];
#else
      T s = dg[r] * x[r];
#endif
#pragma unroll
      for (int c = 0; c < NT_; ++c) if (INTRI(r, c)) s = XFMA(te[r * NT_ + c], x[c], s);
      y[r] = s;
    }
#pragma unroll
    for (int r = 0; r < NT_; ++r) V_AT(r, q) = xsmm_amul(y[r]);
#endif
  }
#else /* the same operations in place: B holds the vectors */
#if KIND == 6 /* column by column of E for all vectors at once: one reciprocal per pivot */
#if ALPHA_KIND != 0
#pragma unroll 1
  for (int q = 0; q < NV_; ++q) {
#pragma unroll 1
    for (int r = 0; r < NT_; ++r) V_AT(r, q) = xsmm_amul(V_AT(r, q));
  }
#endif
#pragma unroll 1
  for (int cc = 0; cc < NT_; ++cc) {
    const int c = (LOWEFF ? cc : NT_ - 1 - cc);
    const int r0 = (LOWEFF ? c + 1 : 0), r1 = (LOWEFF ? NT_ : c);
#if !UNITDIAG
    const T rinv = (T)1 / EM(c, c);
#endif
#pragma unroll 1
    for (int q = 0; q < NV_; ++q) {
#if UNITDIAG
      const T xc = V_AT(c, q);
#else
      const T xc = V_AT(c, q) * rinv;
      V_AT(c, q) = xc;
#endif
#pragma unroll 4
      for (int r = r0; r < r1; ++r) V_AT(r, q) = XFMA(-EM(r, c), xc, V_AT(r, q));
    }
  }
#else /* a row needs the old entries on its side of the diagonal only: from the far end towards them */
#pragma unroll 1
  for (int q = 0; q < NV_; ++q) {
#pragma unroll 1
    for (int rr = 0; rr < NT_; ++rr) {
      const int r = (LOWEFF ? NT_ - 1 - rr : rr);
#if UNITDIAG
      T s = V_AT(r, q);
#else
      T s = EM(r, r) * V_AT(r, q);
#endif
      const int c0 = (LOWEFF ? 0 : r + 1), c1 = (LOWEFF ? r : NT_);
#pragma unroll 4
      for (int c = c0; c < c1; ++c) s = XFMA(EM(r, c), V_AT(c, q), s);
      V_AT(r, q) = xsmm_amul(s);
    }
  }
#endif
#endif
#endif
}

#if FORM == 1
// The lines of npk packs between global memory and their tight images in LDS: the whole work-group moves, 16 bytes per lane and
// piece, four pieces per lane in flight. (Pointers out of the ring are cast into the global address space: global_load, not flat.)
template<int CD, int NL, int LD, int LS>
__device__ __forceinline__ void xsmm_packed_move(T* lds, GT* gbase, const void* const* ring, int slot, long long p0, int npk, bool out)
{
  constexpr int CPL = CD * (VLEN * (int)sizeof(T) / 16); // 16-byte pieces per line
  constexpr int CH = CPL * NL;
  constexpr int U = 4;
  const int total = npk * CH;
  for (int i0 = (int)threadIdx.x; i0 < total; i0 += THREADS * U) {
    GV* gp[U]; uint4* lp[U]; uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = (i0 + u * THREADS < total) ? i0 + u * THREADS : i0; // (beyond the end: the lane's first piece once more, not stored)
      const int g = idx / CH, rem = idx - g * CH, line = rem / CPL, off = rem - line * CPL;
      GT* const base = (nullptr != ring) ? (GT*)ring[3 * (p0 + g) + slot] : gbase + (p0 + g) * (long long)LD * (NL * VLEN);
      gp[u] = (GV*)(base + (long long)line * (LD * VLEN)) + off;
      lp[u] = reinterpret_cast<uint4*>(lds + (long long)g * LS) + rem;
    }
    if (!out) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = *gp[u];
#pragma unroll
      for (int u = 0; u < U; ++u) if (i0 + u * THREADS < total) *lp[u] = r[u];
    }
    else {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = *lp[u];
#pragma unroll
      for (int u = 0; u < U; ++u) if (i0 + u * THREADS < total) *gp[u] = r[u];
    }
  }
}
#endif

extern "C" __global__ __launch_bounds__(THREADS) void xsmm_packed_op(const T* a, const T* b, T* c, long long npacks,
  const unsigned long long* count_ptr, const void* const* ring)
{
  // (a burst of deferred calls: the gate in front of this launch has left the number of recorded calls in *count_ptr)
  if (nullptr != count_ptr) { const long long n = (long long)count_ptr[0]; if (n < npacks) npacks = n; }
  GT* const ga = (GT*)a; GT* const gb = (GT*)b; GT* const gc = (GT*)c;
#if FORM == 1
  __shared__ __attribute__((aligned(16))) T lds[G * (A_LS + B_LS + C_LS)];
  T* const la = lds; T* const lb = la + G * A_LS; T* const lc = lb + G * B_LS;
  for (long long p0 = (long long)blockIdx.x * G; p0 < npacks; p0 += (long long)gridDim.x * G) {
    const int npk = (int)(npacks - p0 < G ? npacks - p0 : G);
#if A_USED
    xsmm_packed_move<A_CD, A_NL, A_LD, A_LS>(la, ga, ring, 0, p0, npk, false);
#endif
#if B_USED
    xsmm_packed_move<B_CD, B_NL, B_LD, B_LS>(lb, gb, ring, 1, p0, npk, false);
#endif
#if C_USED
    xsmm_packed_move<C_CD, C_NL, C_LD, C_LS>(lc, gc, ring, 2, p0, npk, false);
#endif
    __syncthreads();
    if ((int)threadIdx.x < npk * VLEN) {
      const int g = (int)threadIdx.x / VLEN, v = (int)threadIdx.x % VLEN;
      xsmm_packed_lane<T*>(la + g * A_LS + v, lb + g * B_LS + v, lc + g * C_LS + v);
    }
    __syncthreads();
#if WRITTEN == 0
    xsmm_packed_move<A_CD, A_NL, A_LD, A_LS>(la, ga, ring, 0, p0, npk, true);
#elif WRITTEN == 1
    xsmm_packed_move<B_CD, B_NL, B_LD, B_LS>(lb, gb, ring, 1, p0, npk, true);
#else
    xsmm_packed_move<C_CD, C_NL, C_LD, C_LS>(lc, gc, ring, 2, p0, npk, true);
#endif
    __syncthreads();
  }
#else
  const long long lane = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long p = lane / VLEN; const int v = (int)(lane % VLEN);
  if (p < npacks) {
    GT* const pa = (A_USED ? ((nullptr != ring) ? (GT*)ring[3 * p + 0] : ga + p * (long long)A_LD * (A_NL * VLEN)) + v : (GT*)nullptr);
    GT* const pb = (B_USED ? ((nullptr != ring) ? (GT*)ring[3 * p + 1] : gb + p * (long long)B_LD * (B_NL * VLEN)) + v : (GT*)nullptr);
    GT* const pc = (C_USED ? ((nullptr != ring) ? (GT*)ring[3 * p + 2] : gc + p * (long long)C_LD * (C_NL * VLEN)) + v : (GT*)nullptr);
    xsmm_packed_lane<GT*>(pa, pb, pc);
  }
#endif
}
