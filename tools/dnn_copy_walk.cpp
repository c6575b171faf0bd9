// tools/dnn_copy_walk.cpp -- walks the plan of the DNN tensor copy (libxsmm-1_amd/csrc/kernels/dnn_copy_plan.h) on the CPU.
//
// For every layout of the list below -- those of tests/test_dnn_copy_gpu.py and a few that force the other paths -- and for
// both access widths of either side, the program does what the work-groups of kernels/dnn_copy.hip do, with the same index
// functions: tile by tile, the units of the filling side into an image of the tile in LDS, then the units of the draining
// side out of it. The tensors and the image are heap blocks of exactly their size, so an offset out of range is an error of
// the address sanitizer; the program itself checks that every element of the image is written once per tile and read once,
// that every destination element is written once, and that the result equals the reference's loops
// (template/libxsmm_dnn_tensor_{buffer_copy_in_nchw,filter_copy_in_kcrs}.tpl.c), in both directions. It needs no device:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/dnn_copy_walk.cpp -o dnn_copy_walk && ./dnn_copy_walk
#include "../libxsmm-1_amd/csrc/kernels/dnn_copy_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace xsmm;

namespace {

struct Layout { const char* name; int form; unsigned int d[7]; int ts; };

const Layout LAYOUTS[] = {
  // activations { N, fmb, H, W, bfm, lpb }
  { "act conv N2 C24 7x9 (5x7 pad 1)", DNN_COPY_ACT, { 2, 3, 7, 9, 8, 1 }, 4 },
  { "act conv C3 7x9", DNN_COPY_ACT, { 2, 1, 7, 9, 3, 1 }, 4 },
  { "act 8x8", DNN_COPY_ACT, { 2, 1, 8, 8, 16, 1 }, 4 },
  { "act 5x13", DNN_COPY_ACT, { 2, 1, 5, 13, 16, 1 }, 4 },
  { "act fc l_5_32_48", DNN_COPY_ACT, { 5, 2, 1, 1, 16, 1 }, 4 },
  { "act fc lb_5_32_48 bf16", DNN_COPY_ACT, { 5, 2, 1, 1, 8, 2 }, 2 },
  { "act bf16 C32 6x6", DNN_COPY_ACT, { 2, 2, 6, 6, 8, 2 }, 2 },
  { "act 20x20 (two tiles of the run)", DNN_COPY_ACT, { 1, 2, 20, 20, 16, 1 }, 4 },
  { "act bf16 30x30 odd block", DNN_COPY_ACT, { 1, 1, 30, 30, 3, 1 }, 2 },
  { "act wide block (rows and run cut)", DNN_COPY_ACT, { 1, 1, 9, 9, 300, 1 }, 4 },
  // filters { ofmb, ifmb, R, S, bifm, bofm, lpb }
  { "fil C24 K40 3x3", DNN_COPY_FIL, { 5, 3, 3, 3, 8, 8, 1 }, 4 },
  { "fil C3 K16 7x7", DNN_COPY_FIL, { 1, 1, 7, 7, 3, 16, 1 }, 4 },
  { "fil C16 K18 1x1", DNN_COPY_FIL, { 9, 1, 1, 1, 16, 2, 1 }, 4 },
  { "fil C16 K16 11x11 (cut)", DNN_COPY_FIL, { 1, 1, 11, 11, 16, 16, 1 }, 4 },
  { "fil fc 48x32", DNN_COPY_FIL, { 3, 2, 1, 1, 16, 16, 1 }, 4 },
  { "fil fc bf16 48x32", DNN_COPY_FIL, { 3, 2, 1, 1, 8, 16, 2 }, 2 },
  { "fil fc 64x64 blocks", DNN_COPY_FIL, { 2, 2, 1, 1, 64, 64, 1 }, 4 },
  { "fil bf16 3x3 lpb 2", DNN_COPY_FIL, { 2, 2, 3, 3, 8, 16, 2 }, 2 },
  { "fil cut with odd rest", DNN_COPY_FIL, { 2, 1, 11, 11, 16, 19, 1 }, 4 },
  { "fil row beyond the budget (direct)", DNN_COPY_FIL, { 1, 2, 17, 17, 64, 2, 1 }, 4 },
  { "act past the grid clamp", DNN_COPY_ACT, { 1, 4135, 3, 3, 4, 1 }, 4 },
  { "fil past the grid clamp", DNN_COPY_FIL, { 827, 5, 1, 3, 3, 2, 1 }, 4 },
  { "fil direct past the grid clamp", DNN_COPY_FIL, { 1, 59, 17, 17, 63, 1, 1 }, 4 },
  // channel tensors { elements }
  { "bias K40", DNN_COPY_FLAT, { 40 }, 4 },
  { "bn C24", DNN_COPY_FLAT, { 24 }, 4 },
  { "bn bf16 C24 (odd tail)", DNN_COPY_FLAT, { 27 }, 2 },
};

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s: ", lay.name); printf(__VA_ARGS__); printf("\n"); return; } } while (0)

// the reference's loops: blocked offset -> plain offset
std::vector<long long> reference_map(const Layout& lay)
{
  const unsigned int* d = lay.d;
  std::vector<long long> map;
  if (DNN_COPY_ACT == lay.form) {
    const long long N = d[0], fmb = d[1], H = d[2], W = d[3], bfm = d[4], lpb = d[5], C = fmb * bfm * lpb;
    map.resize(N * C * H * W);
    for (long long i1 = 0; i1 < N; ++i1) for (long long i2 = 0; i2 < fmb; ++i2) for (long long i3 = 0; i3 < H; ++i3) for (long long i4 = 0; i4 < W; ++i4)
      for (long long i5 = 0; i5 < bfm; ++i5) for (long long i6 = 0; i6 < lpb; ++i6)
        map[((((i1 * fmb + i2) * H + i3) * W + i4) * bfm + i5) * lpb + i6] = ((i1 * C + (i2 * bfm * lpb + i5 * lpb + i6)) * H + i3) * W + i4;
  }
  else if (DNN_COPY_FIL == lay.form) {
    const long long ofmb = d[0], ifmb = d[1], R = d[2], S = d[3], bifm = d[4], bofm = d[5], lpb = d[6], C = ifmb * bifm * lpb;
    map.resize(ofmb * bofm * C * R * S);
    for (long long i1 = 0; i1 < ofmb; ++i1) for (long long i2 = 0; i2 < ifmb; ++i2) for (long long i3 = 0; i3 < R; ++i3) for (long long i4 = 0; i4 < S; ++i4)
      for (long long i5 = 0; i5 < bifm; ++i5) for (long long i6 = 0; i6 < bofm; ++i6) for (long long i7 = 0; i7 < lpb; ++i7)
        map[(((((i1 * ifmb + i2) * R + i3) * S + i4) * bifm + i5) * bofm + i6) * lpb + i7] = (((i1 * bofm + i6) * C + (i2 * bifm * lpb + i5 * lpb + i7)) * R + i3) * S + i4;
  }
  else {
    map.resize(d[0]);
    for (long long i = 0; i < (long long)d[0]; ++i) map[i] = i;
  }
  return map;
}

// one launch as the kernels run it; vp, vb: elements per unit of the plain and of the blocked side
void walk(const Layout& lay, const DnnCopyGeom& g, bool in, int vp, int vb)
{
  const std::vector<long long> map = reference_map(lay);
  const long long n = g.total;
  CHECK((long long)map.size() == n, "%lld elements, the plan says %lld", (long long)map.size(), n);
  CHECK(g.blocks * g.J * g.L == n, "blocks * rows * run");
  CHECK(g.grid >= 1 && g.grid <= DNN_COPY_MAX_BLOCKS, "grid %d", g.grid);
  long long* const plain = new long long[n];
  long long* const blocked = new long long[n];
  int* const hits = new int[n]();
  for (long long i = 0; i < n; ++i) { plain[i] = in ? i : -1; blocked[i] = in ? -1 : i; }
  long long* const dst = in ? blocked : plain;
  const long long* const src = in ? plain : blocked;
  if (DNN_COPY_FLAT == g.form) { // (dnn_copy_flat: units of 16 bytes, then the tail)
    const int V = 16 / g.ts;
    const long long units = n / V;
    CHECK(g.items == (n + V - 1) / V, "items");
    for (long long q = 0; q < units; ++q) for (int k = 0; k < V; ++k) { dst[q * V + k] = src[q * V + k]; ++hits[q * V + k]; }
    for (long long i = units * V; i < n; ++i) { dst[i] = src[i]; ++hits[i]; }
  }
  else if (0 == g.lds) { // (dnn_copy_direct)
    const long long per = g.J * g.L;
    for (long long i = 0; i < n; ++i) {
      const long long blk = i / per, r = i % per, j = r / g.L, l = r % g.L;
      const long long p = dnn_copy_plain_block(g, blk) + j * g.rowpitch + l, b = blk * per + dnn_copy_blocked_of(g, j, l);
      CHECK(0 <= p && p < n && 0 <= b && b < n, "direct offsets %lld %lld", p, b);
      if (in) { blocked[b] = plain[p]; ++hits[b]; } else { plain[p] = blocked[b]; ++hits[p]; }
    }
  }
  else {
    CHECK(1 <= g.jn && g.jn <= g.J && g.jn * g.P * g.ts <= DNN_COPY_LDS_BUDGET, "rows per pass");
    CHECK(g.lds_bytes <= DNN_COPY_LDS_BUDGET && 0 == g.lds_bytes % 16 && g.jn * g.pitch * g.ts <= g.lds_bytes, "LDS %d bytes", g.lds_bytes);
    CHECK(g.items == g.blocks * g.jpasses * g.ltiles, "items");
    const int slots = g.lds_bytes / g.ts;
    for (long long item = 0; item < g.items; ++item) {
      const DnnCopyTile t = dnn_copy_tile(g, item);
      long long* const tile = new long long[slots];
      int* const filled = new int[slots]();
      for (int phase = 0; phase < 2; ++phase) {
        const bool load = (0 == phase), rows = (in == load);
        if (rows) {
          for (int u = 0; u < dnn_copy_row_units(t, vp); ++u) {
            int jj, l, cnt;
            dnn_copy_row_unit(t, vp, u, &jj, &l, &cnt);
            const long long gp = t.plain0 + (long long)jj * g.rowpitch + l;
            if (cnt == 16 / g.ts && 1 < vp) CHECK(0 == (gp * g.ts) % 16, "plain unit at element %lld is not aligned", gp);
            for (int k = 0; k < cnt; ++k) {
              const int s = jj * g.pitch + l + k;
              if (load) { tile[s] = plain[gp + k]; ++filled[s]; } else { plain[gp + k] = tile[s]; ++hits[gp + k]; --filled[s]; }
            }
          }
        }
        else {
          for (int u = 0; u < dnn_copy_piece_units(t, vb); ++u) {
            int piece, e, cnt;
            dnn_copy_piece_unit(t, vb, u, &piece, &e, &cnt);
            const long long gp = t.blocked0 + piece * t.piece_step + e;
            if (cnt == 16 / g.ts && 1 < vb) CHECK(0 == (gp * g.ts) % 16, "blocked unit at element %lld is not aligned", gp);
            DnnCopyCursor c = dnn_copy_cursor(g, t, piece, e);
            for (int k = 0; k < cnt; ++k) {
              const int s = dnn_copy_lds_of(g, t, c);
              if (load) { tile[s] = blocked[gp + k]; ++filled[s]; } else { blocked[gp + k] = tile[s]; ++hits[gp + k]; --filled[s]; }
              dnn_copy_advance(g, t, c);
            }
          }
        }
        if (load) {
          long long once = 0;
          for (int s = 0; s < slots; ++s) { CHECK(filled[s] <= 1, "LDS element %d filled %d times", s, filled[s]); once += filled[s]; }
          CHECK(once == (long long)t.jn * t.ln, "a tile of %d x %d filled %lld elements", t.jn, t.ln, once);
        }
        else for (int s = 0; s < slots; ++s) CHECK(0 == filled[s], "LDS element %d drained %d times too few", s, filled[s]);
      }
      delete[] tile; delete[] filled;
    }
  }
  for (long long b = 0; b < n; ++b) {
    CHECK(1 == hits[b], "destination element %lld written %d times", b, hits[b]);
    if (in) CHECK(blocked[b] == map[b], "blocked %lld holds plain %lld, the reference takes %lld", b, blocked[b], map[b]);
    else CHECK(plain[map[b]] == b, "plain %lld holds blocked %lld, the reference takes %lld", map[b], plain[map[b]], b);
  }
  delete[] plain; delete[] blocked; delete[] hits;
}

} // namespace

int main()
{
  printf("%-36s form ts blocks rows run rows/pass run/tile pitch conflicts(rows,permuted) items grid lds\n", "layout");
  for (const Layout& lay : LAYOUTS) {
    const DnnCopyGeom g = dnn_copy_geom(lay.form, lay.d, lay.ts);
    int r = 0, p = 0;
    if (0 != g.lds) dnn_copy_conflicts(g, g.pitch, 16 / g.ts, &r, &p);
    printf("%-36s %d %d %lld %lld %lld %lld %lld %d (%d,%d) %lld %d %d\n", lay.name, g.form, g.ts, g.blocks, g.J, g.L, 0 != g.lds ? g.jn : 0, g.P, g.pitch, r, p,
      g.items, g.grid, g.lds_bytes);
    for (int dir = 0; dir < 2; ++dir) {
      walk(lay, g, 0 != dir, 1, 1); // bases that are not aligned: an element per access on both sides
      if (0 != g.lds) {
        const int vp = dnn_copy_plain_width(g, true), vb = dnn_copy_blocked_width(g, true);
        walk(lay, g, 0 != dir, vp, vb);
        walk(lay, g, 0 != dir, vp, 1);
        walk(lay, g, 0 != dir, 1, vb);
      }
    }
  }
  printf(0 == failures ? "dnn_copy_walk: every offset in range and hit once\n" : "dnn_copy_walk: %d FAILED\n", failures);
  return 0 == failures ? EXIT_SUCCESS : EXIT_FAILURE;
}
