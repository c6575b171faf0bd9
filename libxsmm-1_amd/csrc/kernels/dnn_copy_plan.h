// kernels/dnn_copy_plan.h -- the geometry of libxsmm_dnn_copyin_tensor / _copyout_tensor on the GPU: what the
// launcher of kernels/dnn_copy.hip, the kernels themselves, libxsmm_amd_dnn_copy_plan and tools/dnn_copy_walk.cpp share.
// Nothing here needs HIP: the host includes it as it is, and the walk tool checks every offset it yields on the CPU.
//
// A tensor is `blocks` independent blocks. On the plain side (NCHW / KCRS) a block is J rows of a contiguous run of L elements,
// the rows `rowpitch` elements apart; on the blocked side it is one contiguous extent of J * L elements. The run position l
// decomposes as l = (a * Q + q) * S + s (a < A, q < Q, s < S), and the element (row j, l) lies at ((s * A + a) * J + j) * Q + q of
// the extent:
//   activations  [N][fmb][H][W][bfm][lpb] <-> [N][C][H][W]: J = bfm * lpb, L = S = H * W, A = Q = 1 (blocked = l * J + j)
//   filters      [ofmb][ifmb][R][S][bifm][bofm][lpb] <-> [K][C][R][S]: J = bofm, A = bifm, Q = lpb, S = R * S
// A work item is a tile of a block: the rows [j0, j0 + jn) times the run positions [l0, l0 + ln), held in LDS as [row][pitch].
// Runs are cut (l0 > 0) only where A == Q == 1; rows are cut where a whole block does not fit the LDS budget.
#ifndef XSMM_DNN_COPY_PLAN_H
#define XSMM_DNN_COPY_PLAN_H

#if defined(__HIPCC__)
#define DNN_COPY_HD __host__ __device__ __forceinline__
#else
#define DNN_COPY_HD inline
#endif

namespace xsmm {

constexpr int DNN_COPY_THREADS = 256;
constexpr int DNN_COPY_MAX_BLOCKS = 2048;     // 256 CUs x 8 work-groups: the rest is walked by the grid-stride loops
constexpr int DNN_COPY_LDS_BUDGET = 65536;    // bytes of LDS a tile may take, padding included
constexpr int DNN_COPY_TILE_BYTES = 16384;    // what a tile of a cut run aims at
constexpr int DNN_COPY_PIX = 64;              // run positions of a cut run come in multiples of this
constexpr int DNN_COPY_PAD_MAX = 8;           // the pitch of a row in LDS is its run rounded up, plus at most this many elements

enum { DNN_COPY_FLAT = 0, DNN_COPY_ACT = 1, DNN_COPY_FIL = 2 };

struct DnnCopyGeom {
  int form;               // DNN_COPY_FLAT: the same order on both sides (channel tensors, activations of one pixel)
  int ts;                 // bytes per element: 2 or 4
  int lds;                // 0: no tile fits the budget (or FLAT): element by element
  long long total;        // elements
  long long blocks, nb2;  // nb2: blocks that share their rows on the plain side (filters: ifmb)
  long long J, L, rowpitch;
  long long A, Q, S;
  long long jn, P;        // rows and run positions of a full tile
  long long jpasses, ltiles, items;
  int pitch;              // elements per row of a tile in LDS
  int grid;               // work-groups
  int lds_bytes;
};

struct DnnCopyTile {
  long long plain0;       // element offset of (j0, l0) on the plain side
  long long blocked0;     // element offset of the tile's first piece on the blocked side
  long long piece_step;   // from one piece to the next
  int j0, jn, l0, ln;
  int sa0;                // first (s * A + a) of the tile
  int npieces, plen;      // the tile on the blocked side: npieces contiguous pieces of plen elements
};

// ---- index arithmetic shared by the kernels and the host ----------------------------------------------------------------------
DNN_COPY_HD long long dnn_copy_plain_block(const DnnCopyGeom& g, long long blk)
{
  return (blk / g.nb2) * g.J * g.rowpitch + (blk % g.nb2) * g.L;
}

// where in its block's extent the element (row j, run position l) lies
DNN_COPY_HD long long dnn_copy_blocked_of(const DnnCopyGeom& g, long long j, long long l)
{
  const long long s = l % g.S, aq = l / g.S, q = aq % g.Q, a = aq / g.Q;
  return ((s * g.A + a) * g.J + j) * g.Q + q;
}

DNN_COPY_HD DnnCopyTile dnn_copy_tile(const DnnCopyGeom& g, long long item)
{
  DnnCopyTile t;
  const long long lt = item % g.ltiles; item /= g.ltiles;
  const long long jp = item % g.jpasses, blk = item / g.jpasses;
  t.j0 = (int)(jp * g.jn); t.l0 = (int)(lt * g.P);
  t.jn = (int)(g.J - t.j0 < g.jn ? g.J - t.j0 : g.jn);
  t.ln = (int)(g.L - t.l0 < g.P ? g.L - t.l0 : g.P);
  t.sa0 = t.l0; // (a cut run has A == Q == 1: s * A + a is l)
  t.plain0 = dnn_copy_plain_block(g, blk) + t.j0 * g.rowpitch + t.l0;
  t.blocked0 = blk * g.J * g.L + ((long long)t.sa0 * g.J + t.j0) * g.Q;
  const int nsa = (int)(t.ln / g.Q);
  if (t.jn == g.J) { t.npieces = 1; t.plen = (int)(nsa * g.J * g.Q); t.piece_step = 0; }
  else { t.npieces = nsa; t.plen = (int)(t.jn * g.Q); t.piece_step = g.J * g.Q; }
  return t;
}

// The place of one element of a tile on its blocked side, kept while a lane walks along a piece: sa counts (s * A + a) from the
// tile's first, jj the row from j0.
struct DnnCopyCursor { int sa, jj, q, a, s; };

DNN_COPY_HD DnnCopyCursor dnn_copy_cursor(const DnnCopyGeom& g, const DnnCopyTile& t, int piece, int e)
{
  DnnCopyCursor c;
  const int jq = t.jn * (int)g.Q;
  int rem = e;
  if (1 == t.npieces) { c.sa = e / jq; rem = e % jq; } else c.sa = piece;
  if (1 == g.Q) { c.jj = rem; c.q = 0; } else { c.jj = rem / (int)g.Q; c.q = rem % (int)g.Q; } // (uniform: a division less per access)
  const int sag = t.sa0 + c.sa;
  if (1 == g.A) { c.a = 0; c.s = sag; } else { c.a = sag % (int)g.A; c.s = sag / (int)g.A; }
  return c;
}

DNN_COPY_HD void dnn_copy_advance(const DnnCopyGeom& g, const DnnCopyTile& t, DnnCopyCursor& c)
{
  if (++c.q < (int)g.Q) return;
  c.q = 0;
  if (++c.jj < t.jn) return;
  c.jj = 0; ++c.sa;
  if (++c.a < (int)g.A) return;
  c.a = 0; ++c.s;
}

// the element's place in the tile's image in LDS ([row][pitch], the run as on the plain side)
DNN_COPY_HD int dnn_copy_lds_of(const DnnCopyGeom& g, const DnnCopyTile& t, const DnnCopyCursor& c)
{
  return c.jj * g.pitch + ((c.a * (int)g.Q + c.q) * (int)g.S + c.s - t.l0);
}

// The units a work-group moves per side of a tile, one per lane and trip: unit u of the rows' side is `cnt` elements from run
// position l0 + l of row j0 + jj; unit u of the permuted side is `cnt` elements from element e of a piece. v: elements per unit.
DNN_COPY_HD int dnn_copy_row_units(const DnnCopyTile& t, int v) { return t.jn * ((t.ln + v - 1) / v); }
DNN_COPY_HD void dnn_copy_row_unit(const DnnCopyTile& t, int v, int u, int* jj, int* l, int* cnt)
{
  const int upr = (t.ln + v - 1) / v;
  *jj = u / upr; *l = (u % upr) * v;
  *cnt = t.ln - *l < v ? t.ln - *l : v;
}
DNN_COPY_HD int dnn_copy_piece_units(const DnnCopyTile& t, int v) { return t.npieces * ((t.plen + v - 1) / v); }
DNN_COPY_HD void dnn_copy_piece_unit(const DnnCopyTile& t, int v, int u, int* piece, int* e, int* cnt)
{
  const int upp = (t.plen + v - 1) / v;
  *piece = u / upp; *e = (u % upp) * v;
  *cnt = t.plen - *e < v ? t.plen - *e : v;
}

// Elements per access of a side: 16 bytes' worth where every full unit of every tile begins on a multiple of 16 bytes, else 1.
inline bool dnn_copy_multiple16(long long elements, int ts) { return 0 == (elements * ts) % 16; }
inline int dnn_copy_plain_width(const DnnCopyGeom& g, bool base_aligned16)
{ // rows begin at multiples of the row pitch and of the run; tiles at multiples of DNN_COPY_PIX elements
  return (base_aligned16 && dnn_copy_multiple16(g.rowpitch, g.ts) && dnn_copy_multiple16(g.L, g.ts)) ? 16 / g.ts : 1;
}
inline int dnn_copy_blocked_width(const DnnCopyGeom& g, bool base_aligned16)
{ // blocks begin at multiples of J * L; the pieces of a cut block at multiples of jn * Q, J * Q apart
  return (base_aligned16 && dnn_copy_multiple16(g.J * g.L, g.ts)
    && (1 == g.jpasses || (dnn_copy_multiple16(g.jn * g.Q, g.ts) && dnn_copy_multiple16(g.J * g.Q, g.ts)))) ? 16 / g.ts : 1;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// How many of the 32 lanes of a half wave meet on one LDS bank (4-byte banks, 32 of them for 32-bit and narrower accesses) when
// lane x touches the element at lds(x): the largest number of different words on one bank.
template<typename F> inline int dnn_copy_bank_degree(int ts, F lds)
{
  int words[32], degree = 1;
  for (int x = 0; x < 32; ++x) words[x] = lds(x) * ts / 4;
  for (int x = 0; x < 32; ++x) {
    int n = 1;
    for (int y = 0; y < x; ++y) {
      if (words[y] % 32 != words[x] % 32 || words[y] == words[x]) continue;
      bool seen = false;
      for (int z = 0; z < y; ++z) seen = seen || words[z] == words[y];
      if (!seen) ++n;
    }
    if (n > degree) degree = n;
  }
  return degree;
}

// the conflict degrees of the first full tile's two sides for a pitch: the rows' side (lane x at unit x of the tile's rows, vec
// elements apart) and the permuted side (lane x at unit x of the first piece)
inline void dnn_copy_conflicts(DnnCopyGeom g, int pitch, int vec, int* rows_side, int* permuted_side)
{
  g.pitch = pitch;
  const DnnCopyTile t = dnn_copy_tile(g, 0);
  const int upr = (t.ln + vec - 1) / vec;
  *rows_side = *permuted_side = 1;
  for (int k = 0; k < vec; ++k) { // (a lane moves the elements of its unit one after the other)
    const int r = dnn_copy_bank_degree(g.ts, [&](int x) { return (x / upr % t.jn) * pitch + ((x % upr) * vec + k) % t.ln; });
    const int p = dnn_copy_bank_degree(g.ts, [&](int x) {
      return dnn_copy_lds_of(g, t, dnn_copy_cursor(g, t, 0, (int)(((long long)x * vec + k) % t.plen))); });
    if (r > *rows_side) *rows_side = r;
    if (p > *permuted_side) *permuted_side = p;
  }
}

// form ACT: d = { N, fmb, H, W, bfm, lpb }; FIL: d = { ofmb, ifmb, R, S, bifm, bofm, lpb }; FLAT: d[0] = elements
inline DnnCopyGeom dnn_copy_geom(int form, const unsigned int* d, int ts)
{
  DnnCopyGeom g;
  g.form = form; g.ts = ts; g.lds = 0; g.pitch = 0; g.lds_bytes = 0;
  g.blocks = 1; g.nb2 = 1; g.J = 1; g.A = 1; g.Q = 1; g.jn = 1; g.jpasses = 1; g.ltiles = 1;
  const int vec = 16 / ts;
  if (DNN_COPY_ACT == form) {
    g.blocks = (long long)d[0] * d[1]; g.J = (long long)d[4] * d[5]; g.L = (long long)d[2] * d[3];
    g.S = g.L; g.rowpitch = g.L;
    if (1 == g.L) g.form = DNN_COPY_FLAT; // (one pixel: channels are neighbours on both sides)
  }
  else if (DNN_COPY_FIL == form) {
    g.blocks = (long long)d[0] * d[1]; g.nb2 = d[1]; g.J = d[5]; g.A = d[4]; g.Q = d[6]; g.S = (long long)d[2] * d[3];
    g.L = g.A * g.Q * g.S; g.rowpitch = g.nb2 * g.L;
  }
  else { g.L = d[0]; g.S = g.L; g.rowpitch = g.L; }
  g.total = g.blocks * g.J * g.L;
  g.P = g.L;
  if (DNN_COPY_FLAT == g.form || 0 == g.total) {
    if (DNN_COPY_FLAT == g.form) { g.blocks = 1; g.nb2 = 1; g.J = 1; g.L = g.total; g.S = g.L; g.rowpitch = g.L; g.P = g.L; }
    g.jn = 0; g.items = (g.total + vec - 1) / vec; // (units of a vector, one per lane and trip)
    const long long wg = (g.items + DNN_COPY_THREADS - 1) / DNN_COPY_THREADS;
    g.grid = (int)(wg < 1 ? 1 : (wg > DNN_COPY_MAX_BLOCKS ? DNN_COPY_MAX_BLOCKS : wg));
    return g;
  }
  const long long budget = DNN_COPY_LDS_BUDGET / ts; // elements
  if (1 == g.A && 1 == g.Q) { // a run that may be cut: tiles of P run positions times (if they fit) all rows
    long long p = DNN_COPY_TILE_BYTES / (g.J * ts) / DNN_COPY_PIX * DNN_COPY_PIX;
    if (p < DNN_COPY_PIX) p = DNN_COPY_PIX;
    if (p < g.P) g.P = p;
  }
  const long long rowmax = g.P + DNN_COPY_PAD_MAX;
  if (rowmax <= budget) {
    g.lds = 1;
    g.jn = budget / rowmax < g.J ? budget / rowmax : g.J;
    // the pitch: the least conflicts on both sides of the first tile among the paddings allowed
    int best = -1;
    for (int pad = 0; pad <= DNN_COPY_PAD_MAX; ++pad) {
      int r, p;
      g.jpasses = (g.J + g.jn - 1) / g.jn; g.ltiles = (g.L + g.P - 1) / g.P; // (dnn_copy_tile reads them)
      dnn_copy_conflicts(g, (int)g.P + pad, vec, &r, &p);
      if (best < 0 || r + p < best) { best = r + p; g.pitch = (int)g.P + pad; }
    }
    g.lds_bytes = (int)((g.jn * g.pitch * ts + 15) / 16 * 16);
  }
  else { g.jn = 0; g.P = g.L; }
  if (0 != g.lds) {
    g.jpasses = (g.J + g.jn - 1) / g.jn; g.ltiles = (g.L + g.P - 1) / g.P;
    g.items = g.blocks * g.jpasses * g.ltiles;
  }
  else { g.jpasses = 1; g.ltiles = 1; g.items = (g.total + DNN_COPY_THREADS - 1) / DNN_COPY_THREADS; }
  g.grid = (int)(g.items < DNN_COPY_MAX_BLOCKS ? g.items : DNN_COPY_MAX_BLOCKS);
  return g;
}

} // namespace xsmm

#endif
