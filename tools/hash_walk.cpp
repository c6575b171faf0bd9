// tools/hash_walk.cpp -- walks the partition of the GPU hash (libxsmm-1_amd/csrc/kernels/hash_plan.h) on the CPU.
//
// The program does what the waves of kernels/hash.hip do, with the same functions of hash_plan.h and in the same order, one
// lane after the other: the head of a range byte by byte, lane l over the words l, l + 64, ..., the lane's closing product, the
// XOR over the lanes, the tail; for a large item the units of hash_unit() dealt to the waves of the grid, each wave's value
// carried forward by the distance between its units, the partials of the work-groups and the closing step with the seed; for
// a small item line after line. Every read is counted per byte and the buffer is a heap block of exactly the item's extent,
// so a read outside is an error of the address sanitizer. Checked: every byte of every line is read exactly once, no byte of
// a gap is read, and the value equals the bytewise CRC -- for every size 0...5000 at every base offset 0...31, for sizes around
// each span and grid boundary, and for items of several lines. It needs no device:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/hash_walk.cpp -o hash_walk && ./hash_walk
#include "../libxsmm-1_amd/csrc/kernels/hash_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace xsmm;

namespace {

const HashTables TABLES = hash_tables();
const HashPowers POWERS = hash_powers();
const uint32_t* const T = &TABLES.t[0][0];
const uint32_t* const ADV = &TABLES.adv[0][0];

int failures = 0;

struct Buffer { // `extent` bytes whose address is `offset` past a multiple of 64, and a read counter per byte
  unsigned char* block; unsigned char* p; std::vector<unsigned char> reads; size_t extent;
  Buffer(size_t n, unsigned int offset, unsigned int seed) : reads(n, 0), extent(n)
  {
    block = static_cast<unsigned char*>(aligned_alloc(64, (n + offset + 63) / 64 * 64 + 64));
    p = block + offset; // (a read outside the item indexes outside `reads`, which has exactly the item's size: the sanitizer's)
    uint32_t x = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; p[i] = (unsigned char)(x >> 24); }
  }
  ~Buffer() { free(block); }
  unsigned int byte(const unsigned char* q) { ++reads[(size_t)(q - p)]; return *q; }
  uint32_t dword(const unsigned char* q) { uint32_t v; for (int k = 0; k < 4; ++k) ++reads[(size_t)(q - p) + k]; memcpy(&v, q, 4); return v; }
};

uint32_t bytewise(const unsigned char* p, size_t n, uint32_t c)
{
  for (size_t i = 0; i < n; ++i) c = hash_byte(T, c, p[i]); // (main() holds the table against the bit-by-bit form first)
  return c;
}

// wave_hash of kernels/hash.hip
uint32_t wave_hash(Buffer& buf, const unsigned char* p, uint64_t n, uint32_t init)
{
  const HashParts parts = hash_parts(reinterpret_cast<uint64_t>(p), n);
  uint32_t v = init;
  for (unsigned int k = 0; k < parts.head; ++k) v = hash_byte(T, v, buf.byte(p + k));
  if (0 != parts.words) {
    const unsigned char* const w = p + parts.head;
    uint32_t sum = 0;
    for (int lane = 0; lane < 64; ++lane) {
      uint32_t state = 0;
      uint64_t i = (uint64_t)lane;
      if (i < parts.words) {
        const unsigned char* const q = w + i * HASH_WORD;
        const uint32_t d0 = buf.dword(q) ^ (0 == lane ? v : 0u);
        state = hash_word(T, d0, buf.dword(q + 4), buf.dword(q + 8), buf.dword(q + 12));
        i += 64;
      }
      for (; i < parts.words; i += 64) { // (the kernel takes four of these steps per trip while it can)
        const unsigned char* const q = w + i * HASH_WORD;
        state = hash_adv_pass(ADV, state) ^ hash_word(T, buf.dword(q), buf.dword(q + 4), buf.dword(q + 8), buf.dword(q + 12));
      }
      const int rest = hash_lane_rest(parts.words, lane);
      if (rest >= HASH_LANE_POWERS) { ++failures; printf("FAILED: lane rest %d\n", rest); return 0; }
      sum ^= (0 <= rest ? hash_gfmul(state, POWERS.lane[rest]) : 0u);
    }
    v = sum;
  }
  const unsigned char* const tail = p + parts.head + parts.words * HASH_WORD;
  for (unsigned int k = 0; k < parts.tail; ++k) v = hash_byte(T, v, buf.byte(tail + k));
  return v;
}

// hash_items of kernels/hash.hip for one item
uint32_t walk_item(Buffer& buf, uint64_t line_bytes, long long lines, long long ld, uint32_t seed)
{
  uint32_t v = seed;
  for (long long line = 0; line < lines; ++line) v = wave_hash(buf, buf.p + line * ld, line_bytes, v);
  return v;
}

// hash_units and hash_close of kernels/hash.hip
uint32_t walk_units(Buffer& buf, uint64_t line_bytes, long long lines, long long ld, uint32_t seed)
{
  const HashPlan plan = hash_plan(line_bytes, lines);
  if (plan.grid < 1 || plan.grid > HASH_MAX_BLOCKS || 0 != plan.span % HASH_PASS) { ++failures; printf("FAILED: plan\n"); return 0; }
  const long long waves = (long long)plan.grid * HASH_WAVES;
  uint32_t total = 0;
  for (long long w = 0; w < waves; ++w) { // (the XOR of the waves of a work-group, then of the work-groups' partials)
    uint32_t acc = 0, mult = HASH_ONE;
    uint64_t acc_end = 0, mult_gap = 0;
    for (long long u = w; u < plan.units; u += waves) {
      const long long line = u / plan.per_line, part = u % plan.per_line;
      const unsigned char* const la = buf.p + line * ld;
      const HashRange r = hash_unit(plan, reinterpret_cast<uint64_t>(la), line_bytes, part);
      if (r.begin > r.end || r.end > line_bytes || (0 != part && r.begin < r.end && 0 != reinterpret_cast<uint64_t>(la + r.begin) % HASH_WORD)) {
        ++failures; printf("FAILED: unit %lld of %llu x %lld\n", u, (unsigned long long)line_bytes, lines); return 0;
      }
      const uint64_t end = (uint64_t)line * line_bytes + r.end;
      if (0 != acc) {
        if (end - acc_end != mult_gap) { mult_gap = end - acc_end; mult = hash_xpow(POWERS.pow2, mult_gap); }
        acc = hash_gfmul(acc, mult);
      }
      acc ^= wave_hash(buf, la + r.begin, r.end - r.begin, 0u);
      acc_end = end;
    }
    total ^= hash_adv(POWERS.pow2, acc, line_bytes * (uint64_t)lines - acc_end);
  }
  return total ^ hash_adv(POWERS.pow2, seed, line_bytes * (uint64_t)lines);
}

void check(uint64_t line_bytes, long long lines, long long ld, unsigned int offset, uint32_t seed)
{
  const size_t extent = (0 < lines && 0 < line_bytes ? (size_t)(lines - 1) * (size_t)ld + line_bytes : 0);
  for (int form = 0; form < 2; ++form) {
    if (0 == form && !hash_small(line_bytes, lines) && 1 < lines) continue; // (a large item of several lines goes by units only)
    Buffer buf(extent, offset, (unsigned int)(line_bytes * 31 + offset + lines));
    uint32_t want = seed;
    for (long long line = 0; line < lines; ++line) want = bytewise(buf.p + line * ld, line_bytes, want);
    const uint32_t got = (0 == form ? walk_item(buf, line_bytes, lines, ld, seed) : walk_units(buf, line_bytes, lines, ld, seed));
    if (got != want) {
      ++failures;
      printf("FAILED: %s, %llu bytes x %lld lines, ld %lld, offset %u: %08x, expected %08x\n", 0 == form ? "item" : "units",
        (unsigned long long)line_bytes, lines, ld, offset, got, want);
    }
    for (size_t i = 0; i < extent; ++i) {
      const unsigned char expected = ((uint64_t)(i % (size_t)(0 != ld ? ld : 1)) < line_bytes || 1 >= lines) ? 1 : 0;
      if (buf.reads[i] != expected) {
        ++failures;
        printf("FAILED: %s, %llu bytes x %lld lines, ld %lld, offset %u: byte %llu read %d times\n", 0 == form ? "item" : "units",
          (unsigned long long)line_bytes, lines, ld, offset, (unsigned long long)i, (int)buf.reads[i]);
        break;
      }
    }
  }
}

} // namespace

int main()
{
  // the check value of CRC-32C and the identities the kernels rest on
  if (0x1CF96D7Cu != bytewise(reinterpret_cast<const unsigned char*>("123456789"), 9, 0xFFFFFFFFu)) { ++failures; printf("FAILED: check value\n"); }
  for (uint32_t b = 0; b < 256; ++b) if (TABLES.t[0][b] != hash_zero_byte(b)) { ++failures; printf("FAILED: table entry %u\n", b); }
  if (0xF26B8303u != TABLES.t[0][1] || 0xE13B70F7u != TABLES.t[0][2]) { ++failures; printf("FAILED: table\n"); }
  for (uint32_t c : { 1u, 0x80000000u, 0xdeadbeefu }) {
    uint32_t z = c;
    for (int k = 0; k < HASH_PASS; ++k) z = hash_zero_byte(z);
    if (z != hash_adv_pass(ADV, c) || z != hash_adv(POWERS.pow2, c, HASH_PASS)) { ++failures; printf("FAILED: advance of %08x\n", c); }
  }
  const uint32_t seeds[] = { 0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0x9e3779b9u };
  long long cases = 0;
  for (unsigned int offset = 0; offset < 32; ++offset) {
    for (uint64_t size = 0; size <= 5000; ++size, ++cases) check(size, 1, 0, offset, seeds[(size + offset) % 5]);
  }
  // around the span of a wave, of a work-group, and the sizes that fill the grid once and twice (past that the span grows)
  const uint64_t fill = (uint64_t)HASH_MAX_BLOCKS * HASH_WAVES * HASH_SPAN_MIN;
  const uint64_t edges[] = { HASH_ITEM_MAX, HASH_SPAN_MIN * HASH_WAVES, 2 * HASH_SPAN_MIN * HASH_WAVES, 64 * HASH_SPAN_MIN + HASH_PASS, fill, 2 * fill };
  for (const uint64_t edge : edges) {
    for (int d = -1; d <= 1; ++d) {
      const unsigned int offsets[] = { 0, 1, 7, 15 };
      if (edge < fill) { for (int o = 0; o < 4; ++o, ++cases) check(edge + d, 1, 0, offsets[o], seeds[(d + 1 + o) % 5]); }
      else { check(edge + d, 1, 0, offsets[d + 2], seeds[d + 2]); ++cases; } // (tens of MiB each: one offset per size)
    }
  }
  // several lines: gaps that are never read, heads that change from line to line, small and large items
  const long long shapes[][3] = { { 1, 5, 3 }, { 5, 7, 5 }, { 16, 4, 16 }, { 16, 4, 19 }, { 100, 33, 101 }, { 1024, 16, 1024 }, { 1025, 15, 1031 },
    { 5000, 3, 5003 }, { 5000, 4, 5003 }, { 40000, 5, 40009 }, { 4097, 37, 4111 }, { 33, 3000, 35 } };
  for (const auto& s : shapes) for (unsigned int offset : { 0u, 3u, 15u }) { check((uint64_t)s[0], s[1], s[2], offset, seeds[offset % 5]); ++cases; }
  printf("%lld cases, %d failures\n", cases, failures);
  return 0 == failures ? 0 : 1;
}
