// kernels/matdiff.hip -- libxsmm_matdiff on operands in device memory (include/libxsmm.h, include/libxsmm_amd.h).
//
// Reference: src/libxsmm_math.c:48-238 and src/template/libxsmm_matdiff.tpl.c. The definition is restated in DESIGN.md 8f.
// The work is a stream bound by HBM with a reduction over many fields and no matrix-core work. Every element is widened to
// double; a lane takes MATDIFF_VEC neighbours of a line (16 bytes of fp32 / i32, 2 x 16 bytes of fp64, 8 bytes of i16, 4 of
// i8) in one load where the base, the pitch and the width allow, element by element otherwise. Nothing between m and ld is
// read. All sums are formed in an order fixed by the shape alone -- lane, wave (shuffles), work-group (LDS), then partial
// records in a workspace that a finishing kernel walks in index order: no floating-point atomic anywhere, the same call gives
// the same bytes. The only atomics are integer maxima of the bit patterns of non-negative doubles (matdiff_norms).
//
//   matdiff_items<T>   small items (mm <= MATDIFF_STRIP, mm * nn <= MATDIFF_ITEM_MAX): a wave per item, several lines per step,
//                      both passes (the second one re-reads the item from cache) and the finished record of the item
//   matdiff_tiles<T>   first pass over tiles of MATDIFF_STRIP columns x `lines` lines: a record of scalars per work-group, the
//                      partial sum of every line per strip, the partial sum of every column per tile row
//   matdiff_norms      sums those partial line / column sums in index order, maximum by integer atomics
//   matdiff_mid        one work-group: the work-groups' records in index order; leaves the averages in device memory
//   matdiff_var<T>     second pass: squared distances from the averages, a pair of partial sums per work-group
//   matdiff_close      one work-group: the variance partials in index order, then the finished record
//   matdiff_reduce     records of a batch, 1024 to one per work-group and level, as libxsmm_matdiff_reduce combines them
//   matdiff_emit       records to libxsmm_matdiff_info bytes
#include <hip/hip_runtime.h>

#include "../xsmm_internal.hpp"

namespace xsmm {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int MATDIFF_THREADS = 256;
constexpr int MATDIFF_WAVES = MATDIFF_THREADS / 64;
constexpr int MATDIFF_VEC = 4;                     // elements of a line per lane
constexpr int MATDIFF_STRIP = 64 * MATDIFF_VEC;    // columns of a tile: one wave across
constexpr int MATDIFF_LINES = 16;                  // lines of a tile: a multiple of this (4 per wave)
constexpr int MATDIFF_ITEM_MAX = 4096;             // elements of an item that a single wave takes
constexpr int MATDIFF_MAX_BLOCKS = 2048;           // 256 CUs x 8 work-groups
constexpr int MATDIFF_REDUCE_CHUNK = 1024;         // records per work-group of matdiff_reduce
constexpr long long NONE = 0x7fffffffffffffffLL;

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---- what a lane, a wave, a work-group and the whole call accumulate ---------------------------------------------------------
struct Sums {
  double minr, maxr, mint, maxt, linf, linfrel, l2rel, l1r, l1t, fr, ft, l2abs;
  long long linf_idx, nan_idx; // traversal index i * mm + j of the first largest difference / the first non-finite test value
};

__device__ __forceinline__ void sums_clear(Sums& s)
{
  s.minr = s.mint = pos_inf(); s.maxr = s.maxt = -pos_inf();
  s.linf = s.linfrel = s.l2rel = s.l1r = s.l1t = s.fr = s.ft = s.l2abs = 0;
  s.linf_idx = s.nan_idx = NONE;
}

// commutative: both sides of an exchange arrive at the same bits (but for the sign of a zero minimum / maximum)
__device__ __forceinline__ void sums_merge(Sums& a, const Sums& b)
{
  if (b.minr < a.minr) a.minr = b.minr;
  if (b.maxr > a.maxr) a.maxr = b.maxr;
  if (b.mint < a.mint) a.mint = b.mint;
  if (b.maxt > a.maxt) a.maxt = b.maxt;
  if (a.linf < b.linf || (a.linf == b.linf && b.linf_idx < a.linf_idx)) { a.linf = b.linf; a.linf_idx = b.linf_idx; }
  if (a.linfrel < b.linfrel) a.linfrel = b.linfrel;
  a.l2rel += b.l2rel; a.l1r += b.l1r; a.l1t += b.l1t; a.fr += b.fr; a.ft += b.ft; a.l2abs += b.l2abs;
  if (b.nan_idx < a.nan_idx) a.nan_idx = b.nan_idx;
}

__device__ __forceinline__ void sums_exchange(Sums& s, int offset)
{
  Sums o;
  o.minr = __shfl_xor(s.minr, offset, 64); o.maxr = __shfl_xor(s.maxr, offset, 64);
  o.mint = __shfl_xor(s.mint, offset, 64); o.maxt = __shfl_xor(s.maxt, offset, 64);
  o.linf = __shfl_xor(s.linf, offset, 64); o.linfrel = __shfl_xor(s.linfrel, offset, 64);
  o.l2rel = __shfl_xor(s.l2rel, offset, 64); o.l1r = __shfl_xor(s.l1r, offset, 64); o.l1t = __shfl_xor(s.l1t, offset, 64);
  o.fr = __shfl_xor(s.fr, offset, 64); o.ft = __shfl_xor(s.ft, offset, 64); o.l2abs = __shfl_xor(s.l2abs, offset, 64);
  o.linf_idx = __shfl_xor(s.linf_idx, offset, 64); o.nan_idx = __shfl_xor(s.nan_idx, offset, 64);
  sums_merge(s, o);
}

__device__ __forceinline__ void sums_wave(Sums& s)
{ // butterfly: every lane ends with the wave's record
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) sums_exchange(s, o);
}

// the work-group's record in thread 0 (every thread calls)
__device__ __forceinline__ void sums_block(Sums& s, Sums* shared /* [MATDIFF_WAVES] */)
{
  sums_wave(s);
  if (0 == (threadIdx.x & 63)) shared[threadIdx.x >> 6] = s;
  __syncthreads();
  if (0 == threadIdx.x) {
#pragma unroll
    for (int w = 1; w < MATDIFF_WAVES; ++w) sums_merge(s, shared[w]);
  }
  __syncthreads();
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// three sums over the wave for seven exchanges: lane 0 ends with a, lane 1 with b, lane 2 with c
__device__ __forceinline__ double wave_sum3(double a, double b, double c)
{
  const int lane = threadIdx.x & 63;
  const bool odd = (0 != (lane & 1)), hi = (0 != (lane & 2));
  double x = odd ? b : a; const double sx = odd ? a : b;
  x += __shfl_xor(sx, 1, 64);                       // even lanes: a of the pair, odd lanes: b
  double y = odd ? 0.0 : c; const double sy = odd ? c : 0.0;
  y += __shfl_xor(sy, 1, 64);                       // even lanes: c of the pair, odd lanes: 0
  double k = hi ? y : x; const double sk = hi ? x : y;
  k += __shfl_xor(sk, 2, 64);                       // lanes 4q: a, 4q + 1: b, 4q + 2: c of the four
#pragma unroll
  for (int o = 4; o < 64; o <<= 1) k += __shfl_xor(k, o, 64);
  return k;
}

// ---- elements ------------------------------------------------------------------------------------------------------------
// MATDIFF_VEC elements at p as doubles; whole: one load (the address is aligned for it and all four are inside the line)
__device__ __forceinline__ void load_vec(const float* p, double (&x)[4])
{ const u32x4 v = *reinterpret_cast<const u32x4*>(p); x[0] = __uint_as_float(v.x); x[1] = __uint_as_float(v.y); x[2] = __uint_as_float(v.z); x[3] = __uint_as_float(v.w); }
__device__ __forceinline__ void load_vec(const double* p, double (&x)[4])
{ const f64x2 a = *reinterpret_cast<const f64x2*>(p), b = *reinterpret_cast<const f64x2*>(p + 2); x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; }
__device__ __forceinline__ void load_vec(const int* p, double (&x)[4])
{ const u32x4 v = *reinterpret_cast<const u32x4*>(p); x[0] = (int)v.x; x[1] = (int)v.y; x[2] = (int)v.z; x[3] = (int)v.w; }
__device__ __forceinline__ void load_vec(const short* p, double (&x)[4])
{ const u32x2 v = *reinterpret_cast<const u32x2*>(p); x[0] = (short)(v.x & 0xffffu); x[1] = (short)(v.x >> 16); x[2] = (short)(v.y & 0xffffu); x[3] = (short)(v.y >> 16); }
__device__ __forceinline__ void load_vec(const signed char* p, double (&x)[4])
{ const unsigned v = *reinterpret_cast<const unsigned*>(p); x[0] = (signed char)(v & 0xffu); x[1] = (signed char)((v >> 8) & 0xffu); x[2] = (signed char)((v >> 16) & 0xffu); x[3] = (signed char)(v >> 24); }

template<typename T> __device__ __forceinline__ void load4(const T* p, bool whole, int valid, double (&x)[4])
{
  if (whole) load_vec(p, x);
  else {
#pragma unroll
    for (int k = 0; k < MATDIFF_VEC; ++k) x[k] = (k < valid ? (double)p[k] : 0.0);
  }
}

// one element of the first pass (tpl.c:44-119): d, ra, ta are what enters the line and column sums
__device__ __forceinline__ void element(Sums& s, double r, double t, bool has_tst, long long idx, double& d, double& ra, double& ta)
{
  if (r < s.minr) s.minr = r;
  if (r > s.maxr) s.maxr = r;
  ta = fabs(t);
  if (!(ta < pos_inf())) { // NaN or infinite: the call reports this place (the first one) and nothing else
    if (idx < s.nan_idx) s.nan_idx = idx;
    d = ra = ta = 0;
    return;
  }
  d = has_tst ? (r < t ? t - r : r - t) : 0.0;
  ra = fabs(r);
  if (t < s.mint) s.mint = t;
  if (t > s.maxt) s.maxt = t;
  if (s.linf < d) { s.linf = d; s.linf_idx = idx; } // (a lane walks in traversal order: strict < keeps the first)
  if (0 < ra) {
    const double dri = __ddiv_rn(d, ra);
    if (s.linfrel < dri) s.linfrel = dri;
    const double v = __dmul_rn(dri, dri);
    if (v < pos_inf()) s.l2rel += v;
  }
  s.l1r += ra; s.l1t += ta;
  s.fr += __dmul_rn(r, r); s.ft += __dmul_rn(t, t);
  const double v = __dmul_rn(d, d);
  if (v < pos_inf()) s.l2abs += v;
}

// the lane's MATDIFF_VEC elements of one line: ls the line's sums of d, |r|, |t|; cs the same per column
template<typename T>
__device__ __forceinline__ void quad(Sums& s, double (&cs)[3 * MATDIFF_VEC], double (&ls)[3], const T* r, const T* t, bool vec_r, bool vec_t, int valid, long long idx)
{
  double xr[MATDIFF_VEC], xt[MATDIFF_VEC] = { 0, 0, 0, 0 };
  const bool has_tst = (nullptr != t);
  load4(r, vec_r && MATDIFF_VEC == valid, valid, xr);
  if (has_tst) load4(t, vec_t && MATDIFF_VEC == valid, valid, xt);
#pragma unroll
  for (int k = 0; k < MATDIFF_VEC; ++k) {
    if (k < valid) {
      double d, ra, ta;
      element(s, xr[k], xt[k], has_tst, idx + k, d, ra, ta);
      ls[0] += d; ls[1] += ra; ls[2] += ta;
      cs[k] += d; cs[MATDIFF_VEC + k] += ra; cs[2 * MATDIFF_VEC + k] += ta;
    }
  }
}

template<typename T>
__device__ __forceinline__ void quad_var(double& vr, double& vt, double avg_r, double avg_t, const T* r, const T* t, bool vec_r, bool vec_t, int valid)
{
  double xr[MATDIFF_VEC], xt[MATDIFF_VEC] = { 0, 0, 0, 0 };
  load4(r, vec_r && MATDIFF_VEC == valid, valid, xr);
  if (nullptr != t) load4(t, vec_t && MATDIFF_VEC == valid, valid, xt);
#pragma unroll
  for (int k = 0; k < MATDIFF_VEC; ++k) {
    if (k < valid) {
      const double a = xr[k] - avg_r, b = xt[k] - avg_t;
      vr += __dmul_rn(a, a); vt += __dmul_rn(b, b);
    }
  }
}

__device__ __forceinline__ double rel_to(double x, double by_ref, double by_tst)
{ // relative to the reference's, or to the test set's if that is 0, or 0 (tpl.c:157-176,222-230)
  return 0 < by_ref ? __ddiv_rn(x, by_ref) : (0 < by_tst ? __ddiv_rn(x, by_tst) : 0.0);
}

// nrm: the largest line sum of d, |r|, |t|, then the largest column sum of d, |r|, |t|
__device__ void finalize(const Sums& s, const double* nrm, double var_r, double var_t, long long mm, long long size, long long item, MatdiffRecord* out)
{
  MatdiffRecord r;
  for (int i = 0; i < MATDIFF_FIELDS; ++i) r.f[i] = 0;
  r.item = item; r.nan = 0; r.m = r.n = -1;
  if (NONE != s.nan_idx) { r.nan = 1; r.m = s.nan_idx % mm; r.n = s.nan_idx / mm; *out = r; return; }
  r.f[MD_NORMI_ABS] = nrm[0]; r.f[MD_NORMI_REL] = rel_to(nrm[0], nrm[1], nrm[2]);
  r.f[MD_NORM1_ABS] = nrm[3]; r.f[MD_NORM1_REL] = rel_to(nrm[3], nrm[4], nrm[5]);
  r.f[MD_NORMF_REL] = __dsqrt_rn(rel_to(s.l2abs, s.fr, s.ft));
  r.f[MD_LINF_ABS] = s.linf; r.f[MD_LINF_REL] = s.linfrel;
  r.f[MD_L2_ABS] = __dsqrt_rn(s.l2abs); r.f[MD_L2_REL] = __dsqrt_rn(s.l2rel);
  r.f[MD_L1_REF] = s.l1r; r.f[MD_MIN_REF] = s.minr; r.f[MD_MAX_REF] = s.maxr;
  r.f[MD_L1_TST] = s.l1t; r.f[MD_MIN_TST] = s.mint; r.f[MD_MAX_TST] = s.maxt;
  r.f[MD_AVG_REF] = __ddiv_rn(s.l1r, (double)size); r.f[MD_AVG_TST] = __ddiv_rn(s.l1t, (double)size);
  r.f[MD_VAR_REF] = __ddiv_rn(var_r, (double)size); r.f[MD_VAR_TST] = __ddiv_rn(var_t, (double)size);
  if (NONE != s.linf_idx) { r.m = s.linf_idx % mm; r.n = s.linf_idx / mm; }
  *out = r;
}

// ---- a wave per item ---------------------------------------------------------------------------------------------------------
// 2^lw lanes lie along a line (4 * 2^lw >= mm), the 64 >> lw groups of lanes take neighbouring lines. Wave-uniform loops: the
// exchanges are reached by all 64 lanes.
template<typename T>
__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_items_kernel(MatdiffArgs a, MatdiffRecord* rec, int lw)
{
  const int lane = threadIdx.x & 63, LW = 1 << lw, LS = 64 >> lw, lj = lane & (LW - 1), li = lane >> lw;
  const long long nwaves = (long long)gridDim.x * MATDIFF_WAVES;
  const long long j = (long long)MATDIFF_VEC * lj;
  const int valid = (int)(a.mm - j < 0 ? 0 : (a.mm - j > MATDIFF_VEC ? MATDIFF_VEC : a.mm - j));
  const bool vec_r = (0 != a.vec_ref), vec_t = (0 != a.vec_tst);
  for (long long item = (long long)blockIdx.x * MATDIFF_WAVES + (threadIdx.x >> 6); item < a.batch; item += nwaves) {
    const T* const r = static_cast<const T*>(a.ref) + item * a.sr;
    const T* const t = (nullptr != a.tst ? static_cast<const T*>(a.tst) + item * a.st : nullptr);
    Sums s; sums_clear(s);
    double cs[3 * MATDIFF_VEC], nrm[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 3 * MATDIFF_VEC; ++k) cs[k] = 0;
    for (long long i0 = 0; i0 < a.nn; i0 += LS) {
      const long long i = i0 + li;
      double ls[3] = { 0, 0, 0 };
      if (i < a.nn && 0 < valid) quad<T>(s, cs, ls, r + i * a.ldr + j, nullptr != t ? t + i * a.ldt + j : nullptr, vec_r, vec_t, valid, i * a.mm + j);
      for (int o = 1; o < LW; o <<= 1) { ls[0] += __shfl_xor(ls[0], o, 64); ls[1] += __shfl_xor(ls[1], o, 64); ls[2] += __shfl_xor(ls[2], o, 64); }
#pragma unroll
      for (int q = 0; q < 3; ++q) if (nrm[q] < ls[q]) nrm[q] = ls[q];
    }
    for (int o = LW; o < 64; o <<= 1) { // the column sums over the groups of lines; the largest line sum of any group
#pragma unroll
      for (int k = 0; k < 3 * MATDIFF_VEC; ++k) cs[k] += __shfl_xor(cs[k], o, 64);
#pragma unroll
      for (int q = 0; q < 3; ++q) { const double x = __shfl_xor(nrm[q], o, 64); if (nrm[q] < x) nrm[q] = x; }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double x = 0;
#pragma unroll
      for (int k = 0; k < MATDIFF_VEC; ++k) if (x < cs[q * MATDIFF_VEC + k]) x = cs[q * MATDIFF_VEC + k];
      for (int o = 1; o < LW; o <<= 1) { const double y = __shfl_xor(x, o, 64); if (x < y) x = y; }
      nrm[3 + q] = x;
    }
    sums_wave(s);
    const long long size = a.mm * a.nn;
    const double avg_r = __ddiv_rn(s.l1r, (double)size), avg_t = __ddiv_rn(s.l1t, (double)size);
    double vr = 0, vt = 0;
    for (long long i = li; i < a.nn; i += LS) {
      if (0 < valid) quad_var<T>(vr, vt, avg_r, avg_t, r + i * a.ldr + j, nullptr != t ? t + i * a.ldt + j : nullptr, vec_r, vec_t, valid);
    }
    vr = wave_sum(vr); vt = wave_sum(vt);
    if (0 == lane) finalize(s, nrm, vr, vt, a.mm, size, a.item0 + item, rec + item);
  }
}

// ---- tiles of one large item ---------------------------------------------------------------------------------------------------
struct TileWs { // the workspace of one tiled call (doubles; see matdiff_tiled_workspace)
  unsigned long long* norm; // [6] bit patterns of the largest line sums (d, |r|, |t|), then of the largest column sums
  double* avg;              // [2]
  Sums* sums;               // [nwg]
  double* var;              // [nwg][2]
  double* line;             // [nn][nstrips][3]
  double* col;              // [nrows][mm][3]
};

__device__ __forceinline__ TileWs tile_ws(void* base, const MatdiffArgs& a, long long nstrips, long long nrows)
{
  TileWs w;
  double* p = static_cast<double*>(base);
  const long long nwg = nstrips * nrows;
  w.norm = reinterpret_cast<unsigned long long*>(p); p += 6;
  w.avg = p; p += 2;
  w.sums = reinterpret_cast<Sums*>(p); p += nwg * (long long)(sizeof(Sums) / sizeof(double));
  w.var = p; p += 2 * nwg;
  w.line = p; p += 3 * a.nn * nstrips;
  w.col = p;
  return w;
}

// work-group g: strip g % nstrips, tile row g / nstrips; wave w takes the lines w, w + 4, ... of the tile
template<typename T>
__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_tiles_kernel(MatdiffArgs a, void* wsbase, long long nstrips, long long nrows, int lines)
{
  __shared__ Sums wave_sums[MATDIFF_WAVES];
  __shared__ double wave_cols[MATDIFF_WAVES][3 * MATDIFF_VEC][64];
  const TileWs ws = tile_ws(wsbase, a, nstrips, nrows);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long strip = blockIdx.x % nstrips, row = blockIdx.x / nstrips;
  const long long j = strip * MATDIFF_STRIP + (long long)MATDIFF_VEC * lane;
  const int valid = (int)(a.mm - j < 0 ? 0 : (a.mm - j > MATDIFF_VEC ? MATDIFF_VEC : a.mm - j));
  const bool vec_r = (0 != a.vec_ref), vec_t = (0 != a.vec_tst);
  const T* const r = static_cast<const T*>(a.ref);
  const T* const t = static_cast<const T*>(a.tst);
  const long long i0 = row * lines, i1 = (i0 + lines < a.nn ? i0 + lines : a.nn);
  Sums s; sums_clear(s);
  double cs[3 * MATDIFF_VEC];
#pragma unroll
  for (int k = 0; k < 3 * MATDIFF_VEC; ++k) cs[k] = 0;
  for (long long i = i0 + wave; i < i1; i += MATDIFF_WAVES) { // (wave-uniform)
    double ls[3] = { 0, 0, 0 };
    if (0 < valid) quad<T>(s, cs, ls, r + i * a.ldr + j, nullptr != t ? t + i * a.ldt + j : nullptr, vec_r, vec_t, valid, i * a.mm + j);
    const double x = wave_sum3(ls[0], ls[1], ls[2]);
    if (lane < 3) ws.line[(i * nstrips + strip) * 3 + lane] = x;
  }
#pragma unroll
  for (int k = 0; k < 3 * MATDIFF_VEC; ++k) wave_cols[wave][k][lane] = cs[k];
  sums_block(s, wave_sums); // (its barriers also order the column sums)
  if (0 == threadIdx.x) ws.sums[blockIdx.x] = s;
  if (0 == wave && 0 < valid) {
#pragma unroll
    for (int k = 0; k < 3 * MATDIFF_VEC; ++k) {
      double x = cs[k];
#pragma unroll
      for (int w = 1; w < MATDIFF_WAVES; ++w) x += wave_cols[w][k][lane];
      if (k % MATDIFF_VEC < valid) ws.col[(row * a.mm + j + k % MATDIFF_VEC) * 3 + k / MATDIFF_VEC] = x;
    }
  }
}

// thread x < nn: line x over the strips; thread nn + x: column x over the tile rows. Sums of non-negative doubles: their bit
// patterns order as unsigned integers.
__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_norms_kernel(MatdiffArgs a, void* wsbase, long long nstrips, long long nrows)
{
  const TileWs ws = tile_ws(wsbase, a, nstrips, nrows);
  const long long total = a.nn + a.mm, step = (long long)gridDim.x * MATDIFF_THREADS;
  for (long long x = (long long)blockIdx.x * MATDIFF_THREADS + threadIdx.x; x < total; x += step) {
    double sum[3] = { 0, 0, 0 };
    if (x < a.nn) {
      const double* const p = ws.line + x * nstrips * 3;
      for (long long s = 0; s < nstrips; ++s) { sum[0] += p[3 * s]; sum[1] += p[3 * s + 1]; sum[2] += p[3 * s + 2]; }
    }
    else {
      const double* const p = ws.col + (x - a.nn) * 3;
      for (long long s = 0; s < nrows; ++s) { sum[0] += p[s * a.mm * 3]; sum[1] += p[s * a.mm * 3 + 1]; sum[2] += p[s * a.mm * 3 + 2]; }
    }
    unsigned long long* const out = ws.norm + (x < a.nn ? 0 : 3);
    for (int q = 0; q < 3; ++q) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(sum[q]);
      if (0 != bits) atomicMax(out + q, bits);
    }
  }
}

__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_mid_kernel(MatdiffArgs a, void* wsbase, long long nstrips, long long nrows)
{
  __shared__ Sums wave_sums[MATDIFF_WAVES];
  const TileWs ws = tile_ws(wsbase, a, nstrips, nrows);
  const long long nwg = nstrips * nrows;
  Sums s; sums_clear(s);
  for (long long g = threadIdx.x; g < nwg; g += MATDIFF_THREADS) sums_merge(s, ws.sums[g]);
  sums_block(s, wave_sums);
  if (0 == threadIdx.x) {
    const double size = (double)(a.mm * a.nn);
    ws.sums[0] = s; // (every record has been read: the barriers of sums_block lie in between)
    ws.avg[0] = __ddiv_rn(s.l1r, size); ws.avg[1] = __ddiv_rn(s.l1t, size);
  }
}

template<typename T>
__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_var_kernel(MatdiffArgs a, void* wsbase, long long nstrips, long long nrows, int lines)
{
  __shared__ double wave_var[MATDIFF_WAVES][2];
  const TileWs ws = tile_ws(wsbase, a, nstrips, nrows);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long strip = blockIdx.x % nstrips, row = blockIdx.x / nstrips;
  const long long j = strip * MATDIFF_STRIP + (long long)MATDIFF_VEC * lane;
  const int valid = (int)(a.mm - j < 0 ? 0 : (a.mm - j > MATDIFF_VEC ? MATDIFF_VEC : a.mm - j));
  const T* const r = static_cast<const T*>(a.ref);
  const T* const t = static_cast<const T*>(a.tst);
  const long long i0 = row * lines, i1 = (i0 + lines < a.nn ? i0 + lines : a.nn);
  const double avg_r = ws.avg[0], avg_t = ws.avg[1];
  double vr = 0, vt = 0;
  if (0 < valid) {
    for (long long i = i0 + wave; i < i1; i += MATDIFF_WAVES) {
      quad_var<T>(vr, vt, avg_r, avg_t, r + i * a.ldr + j, nullptr != t ? t + i * a.ldt + j : nullptr, 0 != a.vec_ref, 0 != a.vec_tst, valid);
    }
  }
  vr = wave_sum(vr); vt = wave_sum(vt);
  if (0 == lane) { wave_var[wave][0] = vr; wave_var[wave][1] = vt; }
  __syncthreads();
  if (0 == threadIdx.x) {
#pragma unroll
    for (int w = 1; w < MATDIFF_WAVES; ++w) { vr += wave_var[w][0]; vt += wave_var[w][1]; }
    ws.var[2 * (long long)blockIdx.x] = vr; ws.var[2 * (long long)blockIdx.x + 1] = vt;
  }
}

__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_close_kernel(MatdiffArgs a, void* wsbase, long long nstrips, long long nrows, MatdiffRecord* rec)
{
  __shared__ double wave_var[MATDIFF_WAVES][2];
  const TileWs ws = tile_ws(wsbase, a, nstrips, nrows);
  const long long nwg = nstrips * nrows;
  double vr = 0, vt = 0;
  for (long long g = threadIdx.x; g < nwg; g += MATDIFF_THREADS) { vr += ws.var[2 * g]; vt += ws.var[2 * g + 1]; }
  vr = wave_sum(vr); vt = wave_sum(vt);
  if (0 == (threadIdx.x & 63)) { wave_var[threadIdx.x >> 6][0] = vr; wave_var[threadIdx.x >> 6][1] = vt; }
  __syncthreads();
  if (0 == threadIdx.x) {
    double nrm[6];
    for (int w = 1; w < MATDIFF_WAVES; ++w) { vr += wave_var[w][0]; vt += wave_var[w][1]; }
    for (int q = 0; q < 6; ++q) nrm[q] = __longlong_as_double((long long)ws.norm[q]);
    finalize(ws.sums[0], nrm, vr, vt, a.mm, a.mm * a.nn, a.item0, rec);
  }
}

// ---- records of a batch ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void record_clear(MatdiffRecord& r)
{ // libxsmm_matdiff_clear: what libxsmm_matdiff_reduce starts from
  for (int i = 0; i < MATDIFF_FIELDS; ++i) r.f[i] = 0;
  r.f[MD_MIN_REF] = r.f[MD_MIN_TST] = pos_inf(); r.f[MD_MAX_REF] = r.f[MD_MAX_TST] = -pos_inf();
  r.m = r.n = -1; r.item = NONE; r.nan = 0;
}

// b into a, every field on its own (src/libxsmm_math.c:182-238); a tie of linf_abs goes to the lower item: the first one
__device__ __forceinline__ void record_merge(MatdiffRecord& a, const MatdiffRecord& b)
{
  const int larger[] = { MD_NORM1_ABS, MD_NORM1_REL, MD_NORMI_ABS, MD_NORMI_REL, MD_NORMF_REL, MD_LINF_REL, MD_L2_ABS, MD_L2_REL,
    MD_VAR_REF, MD_VAR_TST, MD_MAX_REF, MD_MAX_TST };
  if (0 != b.nan) {
    if (0 == a.nan || b.item < a.item) { a.nan = 1; a.m = b.m; a.n = b.n; a.item = b.item; }
    return;
  }
  if (0 != a.nan) return;
  if (a.f[MD_LINF_ABS] < b.f[MD_LINF_ABS] || (a.f[MD_LINF_ABS] == b.f[MD_LINF_ABS] && 0 <= b.m && b.item < a.item)) {
    a.f[MD_LINF_ABS] = b.f[MD_LINF_ABS]; a.m = b.m; a.n = b.n; a.item = b.item;
  }
#pragma unroll
  for (int i = 0; i < (int)(sizeof(larger) / sizeof(*larger)); ++i) if (a.f[larger[i]] < b.f[larger[i]]) a.f[larger[i]] = b.f[larger[i]];
  if (a.f[MD_MIN_REF] > b.f[MD_MIN_REF]) a.f[MD_MIN_REF] = b.f[MD_MIN_REF];
  if (a.f[MD_MIN_TST] > b.f[MD_MIN_TST]) a.f[MD_MIN_TST] = b.f[MD_MIN_TST];
  a.f[MD_L1_REF] += b.f[MD_L1_REF]; a.f[MD_L1_TST] += b.f[MD_L1_TST];
}

__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_reduce_kernel(const MatdiffRecord* in, long long count, MatdiffRecord* out)
{
  __shared__ MatdiffRecord tree[MATDIFF_THREADS];
  constexpr int PER = MATDIFF_REDUCE_CHUNK / MATDIFF_THREADS;
  const long long first = (long long)blockIdx.x * MATDIFF_REDUCE_CHUNK + (long long)threadIdx.x * PER;
  MatdiffRecord r; record_clear(r);
  for (int k = 0; k < PER; ++k) if (first + k < count) record_merge(r, in[first + k]);
  tree[threadIdx.x] = r;
  __syncthreads();
  for (int s = MATDIFF_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) record_merge(tree[threadIdx.x], tree[threadIdx.x + s]);
    __syncthreads();
  }
  if (0 == threadIdx.x) out[blockIdx.x] = tree[0];
}

// record k to out[k]; avg_size > 0: the averages are l1 / avg_size (the batch's info)
__global__ __launch_bounds__(MATDIFF_THREADS) void matdiff_emit_kernel(const MatdiffRecord* rec, long long count, libxsmm_matdiff_info* out, long long* item_out,
  int swap_norms, int swap_ref, double avg_size)
{
  const long long k = (long long)blockIdx.x * MATDIFF_THREADS + threadIdx.x;
  if (k >= count) return;
  const MatdiffRecord r = rec[k];
  libxsmm_matdiff_info o;
  if (0 != r.nan) { // the nine fields; the rest as libxsmm_matdiff_clear leaves it
    const double inf = pos_inf();
    o.norm1_abs = o.norm1_rel = o.normi_abs = o.normi_rel = o.normf_rel = o.linf_abs = o.linf_rel = o.l2_abs = o.l2_rel = inf;
    o.l1_ref = o.avg_ref = o.var_ref = o.l1_tst = o.avg_tst = o.var_tst = 0;
    o.min_ref = o.min_tst = inf; o.max_ref = o.max_tst = -inf;
  }
  else {
    o.norm1_abs = r.f[MD_NORM1_ABS]; o.norm1_rel = r.f[MD_NORM1_REL]; o.normi_abs = r.f[MD_NORMI_ABS]; o.normi_rel = r.f[MD_NORMI_REL];
    o.normf_rel = r.f[MD_NORMF_REL]; o.linf_abs = r.f[MD_LINF_ABS]; o.linf_rel = r.f[MD_LINF_REL]; o.l2_abs = r.f[MD_L2_ABS]; o.l2_rel = r.f[MD_L2_REL];
    o.l1_ref = r.f[MD_L1_REF]; o.min_ref = r.f[MD_MIN_REF]; o.max_ref = r.f[MD_MAX_REF]; o.avg_ref = r.f[MD_AVG_REF]; o.var_ref = r.f[MD_VAR_REF];
    o.l1_tst = r.f[MD_L1_TST]; o.min_tst = r.f[MD_MIN_TST]; o.max_tst = r.f[MD_MAX_TST]; o.avg_tst = r.f[MD_AVG_TST]; o.var_tst = r.f[MD_VAR_TST];
    if (0 < avg_size) { o.avg_ref = __ddiv_rn(o.l1_ref, avg_size); o.avg_tst = __ddiv_rn(o.l1_tst, avg_size); }
    if (0 != swap_norms) { // a vector was walked as one line: its lines are the reference's columns
      double x = o.norm1_abs; o.norm1_abs = o.normi_abs; o.normi_abs = x;
      x = o.norm1_rel; o.norm1_rel = o.normi_rel; o.normi_rel = x;
    }
  }
  o.m = (libxsmm_blasint)r.m; o.n = (libxsmm_blasint)r.n;
  if (0 != swap_ref) { // only tst was given (src/libxsmm_math.c:161-172)
    o.min_tst = o.min_ref; o.min_ref = 0; o.max_tst = o.max_ref; o.max_ref = 0;
    o.avg_tst = o.avg_ref; o.avg_ref = 0; o.var_tst = o.var_ref; o.var_ref = 0;
    o.l1_tst = o.l1_ref; o.l1_ref = 0;
  }
  out[k] = o;
  if (nullptr != item_out && 0 == k) *item_out = (0 <= r.m ? r.item : -1);
}

struct TilePlan { long long nstrips, nrows, nwg; int lines; };
TilePlan tile_plan(const MatdiffArgs& a)
{
  TilePlan p;
  p.nstrips = (a.mm + MATDIFF_STRIP - 1) / MATDIFF_STRIP;
  long long lines = (a.nn * p.nstrips + MATDIFF_MAX_BLOCKS - 1) / MATDIFF_MAX_BLOCKS;
  lines = (lines + MATDIFF_LINES - 1) / MATDIFF_LINES * MATDIFF_LINES;
  if (lines < MATDIFF_LINES) lines = MATDIFF_LINES;
  if (lines > (1 << 20)) lines = 1 << 20;
  p.lines = (int)lines;
  p.nrows = (a.nn + lines - 1) / lines;
  p.nwg = p.nstrips * p.nrows;
  return p;
}

template<typename T> int tiled_typed(const MatdiffArgs& a, void* ws, const TilePlan& p, MatdiffRecord* rec, hipStream_t st)
{
  const dim3 block(MATDIFF_THREADS), grid((unsigned)p.nwg), one(1);
  const long long lanes = a.nn + a.mm;
  const long long nb = (lanes + MATDIFF_THREADS - 1) / MATDIFF_THREADS;
  hipLaunchKernelGGL(matdiff_tiles_kernel<T>, grid, block, 0, st, a, ws, p.nstrips, p.nrows, p.lines);
  hipLaunchKernelGGL(matdiff_norms_kernel, dim3((unsigned)(nb > MATDIFF_MAX_BLOCKS ? MATDIFF_MAX_BLOCKS : nb)), block, 0, st, a, ws, p.nstrips, p.nrows);
  hipLaunchKernelGGL(matdiff_mid_kernel, one, block, 0, st, a, ws, p.nstrips, p.nrows);
  hipLaunchKernelGGL(matdiff_var_kernel<T>, grid, block, 0, st, a, ws, p.nstrips, p.nrows, p.lines);
  hipLaunchKernelGGL(matdiff_close_kernel, one, block, 0, st, a, ws, p.nstrips, p.nrows, rec);
  return (int)hipGetLastError();
}

template<typename T> int items_typed(const MatdiffArgs& a, MatdiffRecord* rec, hipStream_t st)
{
  int lw = 0;
  while (((long long)MATDIFF_VEC << lw) < a.mm) ++lw; // (mm <= MATDIFF_STRIP: lw <= 6)
  long long nb = (a.batch + MATDIFF_WAVES - 1) / MATDIFF_WAVES;
  if (nb > MATDIFF_MAX_BLOCKS) nb = MATDIFF_MAX_BLOCKS;
  hipLaunchKernelGGL(matdiff_items_kernel<T>, dim3((unsigned)nb), dim3(MATDIFF_THREADS), 0, st, a, rec, lw);
  return (int)hipGetLastError();
}

} // namespace

bool matdiff_small(long long mm, long long nn) { return mm <= MATDIFF_STRIP && mm * nn <= MATDIFF_ITEM_MAX; }

size_t matdiff_tiled_workspace(const MatdiffArgs& a)
{
  const TilePlan p = tile_plan(a);
  return sizeof(double) * (size_t)(8 + p.nwg * (long long)(sizeof(Sums) / sizeof(double)) + 2 * p.nwg + 3 * a.nn * p.nstrips + 3 * p.nrows * a.mm);
}

int launch_matdiff_items(const MatdiffArgs& a, MatdiffRecord* rec, void* stream)
{
  const hipStream_t st = (hipStream_t)stream;
  switch (a.datatype) {
    case LIBXSMM_DATATYPE_F64: return items_typed<double>(a, rec, st);
    case LIBXSMM_DATATYPE_F32: return items_typed<float>(a, rec, st);
    case LIBXSMM_DATATYPE_I32: return items_typed<int>(a, rec, st);
    case LIBXSMM_DATATYPE_I16: return items_typed<short>(a, rec, st);
    case LIBXSMM_DATATYPE_I8: return items_typed<signed char>(a, rec, st);
    default: return (int)hipErrorInvalidValue;
  }
}

int launch_matdiff_tiled(const MatdiffArgs& a, void* workspace, MatdiffRecord* rec, void* stream)
{
  const hipStream_t st = (hipStream_t)stream;
  const TilePlan p = tile_plan(a);
  if (p.nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(workspace, 0, 8 * sizeof(double), st); // the maxima and the averages
  if (hipSuccess != e) return (int)e;
  switch (a.datatype) {
    case LIBXSMM_DATATYPE_F64: return tiled_typed<double>(a, workspace, p, rec, st);
    case LIBXSMM_DATATYPE_F32: return tiled_typed<float>(a, workspace, p, rec, st);
    case LIBXSMM_DATATYPE_I32: return tiled_typed<int>(a, workspace, p, rec, st);
    case LIBXSMM_DATATYPE_I16: return tiled_typed<short>(a, workspace, p, rec, st);
    case LIBXSMM_DATATYPE_I8: return tiled_typed<signed char>(a, workspace, p, rec, st);
    default: return (int)hipErrorInvalidValue;
  }
}

long long matdiff_reduce_records(long long count) { return (count + MATDIFF_REDUCE_CHUNK - 1) / MATDIFF_REDUCE_CHUNK; }

int launch_matdiff_reduce(const MatdiffRecord* in, long long count, MatdiffRecord* out, void* stream)
{
  hipLaunchKernelGGL(matdiff_reduce_kernel, dim3((unsigned)matdiff_reduce_records(count)), dim3(MATDIFF_THREADS), 0, (hipStream_t)stream, in, count, out);
  return (int)hipGetLastError();
}

int launch_matdiff_emit(const MatdiffRecord* rec, long long count, libxsmm_matdiff_info* out, long long* item_out, int swap_norms, int swap_ref,
  double avg_size, void* stream)
{
  const long long nb = (count + MATDIFF_THREADS - 1) / MATDIFF_THREADS;
  hipLaunchKernelGGL(matdiff_emit_kernel, dim3((unsigned)nb), dim3(MATDIFF_THREADS), 0, (hipStream_t)stream, rec, count, out, item_out, swap_norms, swap_ref, avg_size);
  return (int)hipGetLastError();
}

} // namespace xsmm
