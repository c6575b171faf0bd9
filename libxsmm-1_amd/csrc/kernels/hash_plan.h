// kernels/hash_plan.h -- the arithmetic of libxsmm_hash / libxsmm_memcmp on the GPU (kernels/hash.hip, xsmm_hash.cpp): everything
// that can be wrong without a device. No HIP header is needed: the host, the kernels and tools/hash_walk.cpp (which walks the
// partition on the CPU under the sanitizers) include this one file, so all three split a byte range the same way.
//
// The function (reference: src/libxsmm_hash.c, src/libxsmm_math.c:260-263) is CRC-32C in its reflected form: polynomial
// 0x82F63B78, the register starts at the seed, nothing is inverted. Bit 31 of a register is the coefficient of x^0, so one zero
// bit multiplies by x: c -> (c >> 1) ^ (c & 1 ? P : 0). With adv(c, n) = c * x^(8n) mod P (n zero bytes),
//   crc(s, A | B) = adv(crc(s, A), |B|) ^ crc(0, B)         and        crc(s, W) = crc(0, W ^ s) for |W| >= 4
// (s folded into the first four bytes). XOR is exact and has no order: any split of a range gives the reference's bits.
#ifndef XSMM_HASH_PLAN_H
#define XSMM_HASH_PLAN_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
# define XSMM_HASH_HD __host__ __device__
#else
# define XSMM_HASH_HD
#endif

namespace xsmm {

constexpr uint32_t HASH_POLY = 0x82F63B78u;
constexpr uint32_t HASH_ONE = 0x80000000u;        // x^0
constexpr int HASH_THREADS = 256;
constexpr int HASH_WAVES = HASH_THREADS / 64;
constexpr int HASH_WORD = 16;                     // bytes a lane loads at once
constexpr int HASH_PASS = 64 * HASH_WORD;         // bytes a wave takes per step: the distance between two words of a lane
constexpr int HASH_SPAN_MIN = 4 * HASH_PASS;      // the least a wave is given (its closing step costs about one pass)
constexpr int HASH_MAX_BLOCKS = 2048;             // 256 CUs x 8 work-groups, the cap of matdiff
constexpr int HASH_ITEM_MAX = 16 * HASH_PASS;     // bytes of an item that a single wave takes in the batch forms
constexpr int HASH_LANE_POWERS = 64;              // a lane ends at most 63 words before its wave does

// ---- GF(2) ---------------------------------------------------------------------------------------------------------------
XSMM_HASH_HD constexpr uint32_t hash_times_x(uint32_t c) { return (c >> 1) ^ (0 != (c & 1u) ? HASH_POLY : 0u); }

XSMM_HASH_HD constexpr uint32_t hash_zero_byte(uint32_t c)
{ // adv(c, 1) without a table
  for (int i = 0; i < 8; ++i) c = hash_times_x(c);
  return c;
}

XSMM_HASH_HD constexpr uint32_t hash_gfmul(uint32_t a, uint32_t b)
{ // a * b mod P: 32 steps whatever the operands are
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (0 != (a & (HASH_ONE >> i))) p ^= b;
    b = hash_times_x(b);
  }
  return p;
}

// t[k][b]: the register after byte b and k zero bytes, from 0 (slicing by four: t[0] is the reference's table, src/libxsmm_hash.c:313)
// adv[k][b]: (b << 8k) * x^(8 * HASH_PASS) -- adv(c, HASH_PASS) is the XOR of four entries, one per byte of c
struct HashTables { uint32_t t[4][256]; uint32_t adv[4][256]; };
// pow2[k] = x^(8 * 2^k); lane[j] = x^(8 * HASH_WORD * j)
struct HashPowers { uint32_t pow2[64]; uint32_t lane[HASH_LANE_POWERS]; };

constexpr HashPowers hash_powers()
{
  HashPowers r{};
  r.pow2[0] = hash_zero_byte(HASH_ONE);
  for (int k = 1; k < 64; ++k) r.pow2[k] = hash_gfmul(r.pow2[k - 1], r.pow2[k - 1]);
  r.lane[0] = HASH_ONE;
  for (int j = 1; j < HASH_LANE_POWERS; ++j) r.lane[j] = hash_gfmul(r.lane[j - 1], r.pow2[4]);
  return r;
}

constexpr HashTables hash_tables()
{
  HashTables r{};
  uint32_t pass = hash_zero_byte(HASH_ONE); // x^8, squared until it is x^(8 * HASH_PASS)
  for (int n = 1; n < HASH_PASS; n *= 2) pass = hash_gfmul(pass, pass);
  for (int b = 0; b < 256; ++b) {
    uint32_t c = (uint32_t)b;
    for (int k = 0; k < 4; ++k) { c = hash_zero_byte(c); r.t[k][b] = c; }
    for (int k = 0; k < 4; ++k) r.adv[k][b] = hash_gfmul((uint32_t)b << (8 * k), pass);
  }
  return r;
}

// x^(8n)
XSMM_HASH_HD inline uint32_t hash_xpow(const uint32_t* pow2 /* HashPowers::pow2 */, uint64_t n)
{
  uint32_t r = HASH_ONE;
  for (int k = 0; 0 != n; ++k, n >>= 1) if (0 != (n & 1u)) r = hash_gfmul(r, pow2[k]);
  return r;
}
XSMM_HASH_HD inline uint32_t hash_adv(const uint32_t* pow2, uint32_t c, uint64_t n) { return 0 != c ? hash_gfmul(c, hash_xpow(pow2, n)) : 0u; }

// ---- table steps (t: HashTables::t, adv: HashTables::adv, as flat arrays of 4 * 256) -----------------------------------------
XSMM_HASH_HD inline uint32_t hash_byte(const uint32_t* t, uint32_t c, unsigned int byte) { return t[(c ^ byte) & 0xffu] ^ (c >> 8); }
XSMM_HASH_HD inline uint32_t hash_dword(const uint32_t* t, uint32_t x)
{ // four bytes at once: x is the register XORed with the (little-endian) dword
  return t[768 + (x & 0xffu)] ^ t[512 + ((x >> 8) & 0xffu)] ^ t[256 + ((x >> 16) & 0xffu)] ^ t[x >> 24];
}
XSMM_HASH_HD inline uint32_t hash_word(const uint32_t* t, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3)
{ // crc(0, the 16 bytes)
  uint32_t x = hash_dword(t, d0);
  x = hash_dword(t, x ^ d1); x = hash_dword(t, x ^ d2);
  return hash_dword(t, x ^ d3);
}
XSMM_HASH_HD inline uint32_t hash_adv_pass(const uint32_t* adv, uint32_t c)
{ // adv(c, HASH_PASS)
  return adv[c & 0xffu] ^ adv[256 + ((c >> 8) & 0xffu)] ^ adv[512 + ((c >> 16) & 0xffu)] ^ adv[768 + (c >> 24)];
}

// ---- a byte range as a wave takes it ------------------------------------------------------------------------------------------
// head: the bytes up to the first address that is a multiple of 16 (all of a shorter range), words: whole 16-byte words,
// tail: what is left. Lane l takes the words l, l + 64, ...; head and tail go byte by byte.
struct HashParts { unsigned int head; uint64_t words; unsigned int tail; };
XSMM_HASH_HD inline HashParts hash_parts(uint64_t address, uint64_t bytes)
{
  HashParts p;
  const uint64_t to_aligned = (0 - address) & (uint64_t)(HASH_WORD - 1);
  p.head = (unsigned int)(bytes < to_aligned ? bytes : to_aligned);
  p.words = (bytes - p.head) / HASH_WORD;
  p.tail = (unsigned int)((bytes - p.head) % HASH_WORD);
  return p;
}
// the words between the last word of lane `lane` and the end of the words (the index into HashPowers::lane); -1: the lane has no word
XSMM_HASH_HD inline int hash_lane_rest(uint64_t words, int lane)
{
  if ((uint64_t)lane >= words) return -1;
  return (int)((words - 1 - (uint64_t)lane) % 64);
}

// ---- a large item: lines of line_bytes bytes, cut into units that waves take in turn ---------------------------------------
// Unit u is part u % per_line of line u / per_line. Part s of a line whose head is h covers [s ? h + s * span : 0, h + (s + 1) * span),
// the last part ends with the line: every part but the first starts at a multiple of 16, and a part may be empty. Wave w of
// grid * HASH_WAVES takes the units w, w + waves, ...
struct HashPlan { uint64_t span; long long per_line, units; int grid; };
XSMM_HASH_HD inline HashPlan hash_plan(uint64_t line_bytes, long long lines)
{
  HashPlan p;
  const uint64_t total = line_bytes * (uint64_t)lines, waves = (uint64_t)HASH_MAX_BLOCKS * HASH_WAVES;
  p.span = (total / waves + (0 != total % waves ? 1 : 0) + HASH_PASS - 1) / HASH_PASS * HASH_PASS;
  if (p.span < (uint64_t)HASH_SPAN_MIN) p.span = HASH_SPAN_MIN;
  p.per_line = (long long)((line_bytes + p.span - 1) / p.span);
  if (p.per_line < 1) p.per_line = 1;
  p.units = p.per_line * lines;
  const long long blocks = (p.units + HASH_WAVES - 1) / HASH_WAVES;
  p.grid = (int)(blocks < HASH_MAX_BLOCKS ? (blocks < 1 ? 1 : blocks) : HASH_MAX_BLOCKS);
  return p;
}
struct HashRange { uint64_t begin, end; };
XSMM_HASH_HD inline HashRange hash_unit(const HashPlan& p, uint64_t line_address, uint64_t line_bytes, long long part)
{
  HashRange r;
  const uint64_t head = hash_parts(line_address, line_bytes).head;
  const uint64_t b = head + (uint64_t)part * p.span, e = b + p.span;
  r.begin = (0 == part ? 0 : (b < line_bytes ? b : line_bytes));
  r.end = (part + 1 == p.per_line || e > line_bytes) ? line_bytes : e;
  return r;
}

// the batch forms: a wave per item up to here, larger items one after the other through the units
XSMM_HASH_HD inline bool hash_small(uint64_t line_bytes, long long lines) { return line_bytes * (uint64_t)lines <= (uint64_t)HASH_ITEM_MAX; }
inline int hash_items_grid(long long batch)
{
  const long long blocks = (batch + HASH_WAVES - 1) / HASH_WAVES;
  return (int)(blocks < HASH_MAX_BLOCKS ? (blocks < 1 ? 1 : blocks) : HASH_MAX_BLOCKS);
}

} // namespace xsmm

#endif
