// smm_jit_geom.h -- DevAddr and the LDS geometry of the generated dense SMM kernels (csrc/xsmm_jit_smm.cpp), stated once: the
// host includes this file and the same text stands in front of every generated kernel (Makefile: SMM_JIT_GEOM_SOURCE). The
// kernels lay their LDS out by these functions and the host sizes the launch (waves per work-group, work-groups per CU, dynamic
// LDS bytes) by the same ones. Plain C++17 constexpr arithmetic on ints: no #include, no HIP keyword (hiprtc compiles this
// without a standard library). Sizes are in elements of the kernel's T unless a name says bytes; typesize is sizeof(T).
#ifndef XSMM_SMM_JIT_GEOM_H
#define XSMM_SMM_JIT_GEOM_H

// batch addressing, the first argument of every generated kernel (same structure and meaning as kernels/smm_common.cuh)
struct DevAddr {
  const char* a; const char* b; char* c;
  const char* ia; const char* ib; const char* ic;
  long long sa, sb, sc;
  int index_base, index_stride, mode;
  const int* flags; // device-side verdict on how C blocks repeat: [0] equal neighbours, [1] out-of-order repeats (or null)
};
static_assert(sizeof(DevAddr) == 96, "DevAddr is a kernel argument: host and device must agree on its layout");

namespace geom {
constexpr int LDS_STATIC = 65536; // bytes of static LDS a work-group may have
constexpr int round4(int elems) { return ((elems + 3) / 4) * 4; }

// ---- register-tiled wave and work-group forms (SMM_JIT_SHAPE) -------------------------------------------------------------
// row stride of B's image [n][kp]: chosen so that the column groups of one instruction fall into different banks
// (tn * typesize / 4 a multiple of 16 -- fp64, eight columns per lane -- has no such stride: an odd one then)
constexpr int kp(int typesize, int tn, int k)
{
  if (0 == (tn * (typesize / 4)) % 16) return k | 1;
  while (0 == (tn * k * (typesize / 4)) % 16) ++k;
  return k;
}
struct Tiled {
  int tgm, tgn, nq, tm, tn; // lanes along m and n of one item, columns of C a wave owns (work-group form), register tile of a lane
  int npad, kp;             // highest column index a lane may touch, plus one; row stride of B's image
  int as1, bs1, cs;         // images of A ([k][m]: lanes with equal ty read the same words, lanes with different tx adjacent ones) and
                            // B ([n][kp]; TRANS_B: [k][n]) of one item, padded by what lanes past the edge read; C of all `pack` items
  int wave_lds, wg_buf, wg_nbuf; // all a wave keeps (wave forms); an operand buffer of the work-group form, two if 64 KiB allow
};
// pack: items a wave handles at a time (the 64 lanes split into `pack` groups); xruns: 0 streaming form, 1 wave run form,
// 2 work-group form (4 waves share one product; a wave owns nq = ceil(n / 4) columns of C, its lanes are 16 along m x 4)
constexpr Tiled tiled(int typesize, int m, int n, int k, bool transb, int pack, int xruns)
{
  const bool wg = (2 == xruns);
  const int tgm = wg ? 16 : ((pack >= 4) ? ((pack >= 16) ? 2 : 4) : 8), tgn = wg ? 4 : 64 / (pack * tgm), nq = wg ? (n + 3) / 4 : 0;
  const int tm = (m + tgm - 1) / tgm, tn = ((wg ? nq : n) + tgn - 1) / tgn, npad = 3 * nq + tgn * tn, kps = kp(typesize, tn, k);
  const int as1 = round4(k * m + tgm * tm), bs1 = transb ? round4(k * n + npad) : round4(npad * kps);
  const int ab = pack * (as1 + bs1), cs = round4(pack * m * n);
  // wave run form: C is in LDS only while a run is opened or closed, when no operand image is alive -- its image lies over
  // theirs; a third less LDS per wave is a third more chains resident per CU
  const int wave_lds = (1 == xruns) ? ((ab > cs) ? ab : cs) : (ab + cs);
  return Tiled{ tgm, tgn, nq, tm, tn, npad, kps, as1, bs1, cs, wave_lds, ab, (2 * ab * typesize <= LDS_STATIC) ? 2 : 1 };
}

// ---- matrix-core kernels: K padded to a multiple of four, the depth of a v_mfma_*_16x16x4 step ----------------------------
constexpr int kp4(int k) { return 4 * ((k + 3) / 4); }

// ---- matrix-core wave form (SMM_JIT_MFMA_WAVE_BODY): a wave per item, m, n, k <= 64 --------------------------------------
// vec: elements per memory access -- a 16-byte chunk where the shape allows it (m a multiple of it, k of four; TRANS_B: n too), or 1
constexpr bool mfma_wave_served(int m, int n, int k, int vec, bool transb)
{
  return m >= 1 && n >= 1 && k >= 1 && m <= 64 && n <= 64 && k <= 64 && (1 == vec || (0 == m % vec && 0 == k % 4 && (!transb || 0 == n % vec)));
}
constexpr int mfma_rows(int m) { return (m <= 16) ? 16 : (m <= 48 ? 48 : 64); } // rows of a k-major image (64: swizzled, not padded)
// row stride of B's image [n][ksd]: an odd number of accesses, so that the rows of one fetch spread over the banks
constexpr int mfma_ksd(int k4, int vec) { return (((k4 + vec - 1) / vec) | 1) * vec; }
// column stride of C's image: such that the four column groups of a tile access fall into different banks
constexpr int mfma_csd(int typesize, int m, int vec) { while (!(8 == typesize ? (16 == m % 32) : (4 == m % 16 || 12 == m % 16))) m += vec; return m; }
struct MfmaWave {
  int ms, ns, ksd, csd;           // rows of A's image [k][ms] and of the TRANS_B image of B [k][ns]; strides of B's [n][ksd] and C's [n][csd]
  int c_elems, a_elems, b_elems;  // C's image shares the place of A's (never alive together)
  int lds_bytes;                  // both images and a word per lane for the writes of lanes outside C; 0: the shape is not served
};
constexpr MfmaWave mfma_wave(int typesize, int m, int n, int k, int vec, bool transb)
{
  if (!mfma_wave_served(m, n, k, vec, transb)) return MfmaWave{ 0, 0, 0, 0, 0, 0, 0, 0 };
  const int k4 = kp4(k), ms = mfma_rows(m), ns = mfma_rows(n), ksd = mfma_ksd(k4, vec), csd = mfma_csd(typesize, m, vec);
  const int c_elems = n * csd, a_elems = (c_elems > k4 * ms) ? c_elems : k4 * ms, b_elems = transb ? k4 * ns : n * ksd;
  return MfmaWave{ ms, ns, ksd, csd, c_elems, a_elems, b_elems, (a_elems + b_elems + 64) * typesize };
}
// ... the columns of C in two halves against one tight image of A ([k][m]); 16-byte chunks only
constexpr bool mfma_wave2_served(int typesize, int m, int n, int k)
{
  const int vec = 16 / typesize, nh = n / 2;
  return 0 == m % vec && 0 == k % 4 && m <= 64 && n <= 64 && k <= 64 && k >= 4 && 0 == (n & 1) && 0 == (k * nh) % vec && 0 == (m * nh) % vec;
}
struct MfmaWave2 { int a_elems, bh_elems, lds_bytes; }; // A; half of B ([nh][ksd]) or of C ([nh][m]) in one place; ... + a word per lane (0: not served)
constexpr MfmaWave2 mfma_wave2(int typesize, int m, int n, int k)
{
  if (!mfma_wave2_served(typesize, m, n, k)) return MfmaWave2{ 0, 0, 0 };
  const int nh = n / 2, ksd = mfma_ksd(kp4(k), 16 / typesize), bh = (nh * ksd > nh * m) ? nh * ksd : nh * m;
  return MfmaWave2{ k * m, bh, (k * m + bh + 64) * typesize };
}

// ---- matrix-core run and streaming forms (SMM_JIT_MFMA_RUNS_CONST): m, n <= 32; A never touches LDS ------------------------
// K goes through the registers and B's image in nch chunks of kc (a multiple of four) -- one chunk up to k = 64; beyond that only
// the streaming form (the run form keeps a whole product's fragments of A in flight), in chunks of at most 32: two chunk variants
// of fragments and address arithmetic alive at once cost registers.
// ksd, row stride of B's image [n][ksd]: fp64 fragments are fetched sixteen lanes (one k, sixteen n) at a time -- an odd stride spreads
// them over all bank pairs; fp32 fragments thirty-two lanes (two k) at a time -- a stride of 2 mod 4 keeps the two k apart as well
struct MfmaRuns { int nch, kc, ksd, wave_lds; }; // wave_lds: B's image, all a wave keeps
constexpr MfmaRuns mfma_runs(int typesize, int n, int k, bool stream)
{
  const int nch = (stream && k > 64) ? (k + 31) / 32 : 1, kc = 4 * (((k + nch - 1) / nch + 3) / 4), ksd = (8 == typesize) ? kc + 1 : kc + 2;
  return MfmaRuns{ nch, kc, ksd, round4(n * ksd) };
}
// LDS bytes of a wave; 0: not served. stream: the streaming form (every item owns its C), which takes k beyond 64 in chunks. In one
// chunk B's span in memory travels through registers, an element per lane and load: 40 loads at most
constexpr int mfma_runs_lds_bytes(int typesize, int m, int n, int k, int ldb, bool stream)
{
  if (m < 1 || n < 1 || k < 1 || m > 32 || n > 32 || k > (stream ? 256 : 64) || (4 != typesize && 8 != typesize)) return 0;
  const MfmaRuns g = mfma_runs(typesize, n, k, stream);
  return (1 == g.nch && (long long)(ldb < k ? k : ldb) * (n - 1) + k > 64 * 40) ? 0 : g.wave_lds * typesize;
}

// ---- work-group-per-item form (SMM_JIT_BIG_BODY): 256 threads (16 x 16) per item, K in chunks of kc through two LDS buffers --
// tm, tn: register tile of a thread; mp, np: m and n in whole tiles. Images of a chunk: A as [kk][mp], B as [kk][npp]: a thread's tm
// resp. tn operands of one k are contiguous (one or two 16-byte reads each). B arrives k-contiguous unless TRANS_B, so its LDS
// writes stride by a row; the 16-byte row padding keeps that at a 4-way bank conflict on the (16x rarer) writes while the reads
// stay aligned.
struct Big { int tm, tn, mp, np, npp, as, bs, buf; };
constexpr Big big(int typesize, int m, int n, int kc)
{
  const int tm = (m + 15) / 16, tn = (n + 15) / 16, mp = 16 * tm, np = 16 * tn, npp = np + 16 / typesize;
  return Big{ tm, tn, mp, np, npp, kc * mp, kc * npp, round4(kc * mp + kc * npp) };
}
} // namespace geom
#endif
