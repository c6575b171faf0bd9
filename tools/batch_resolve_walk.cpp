// tools/batch_resolve_walk.cpp -- walks the address arithmetic of a batch call (libxsmm-1_amd/csrc/xsmm_batch.hpp) on the CPU.
//
// Pointer steps, task slices, index ranges, address hulls, gathered pointer arrays and the slots of staged C matrices, each
// over the cases a batch front end meets -- a batch of one, more tasks than items, index_base 1, a wide stride, a repeated C
// first / last / only, offsets past 2^31 elements -- and each checked against a naive restatement. Index and pointer arrays
// are heap blocks of exactly their size, so a read out of range is an error of the address sanitizer, and an offset that
// leaves 64 bits (or passes through 32) one of the undefined-behaviour sanitizer or of the comparison. It needs no device:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/batch_resolve_walk.cpp -o batch_resolve_walk && ./batch_resolve_walk
#include "../libxsmm-1_amd/csrc/xsmm_batch.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace xsmm;

namespace {

int failures = 0;
#define CHECK(COND) do { if (!(COND)) { ++failures; fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #COND); } } while (0)

unsigned long long lcg_state = 12345;
unsigned int lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned int)(lcg_state >> 33); }

// an index array of n entries, `stride` bytes apart, in a block of exactly (n - 1) * stride + sizeof(int) bytes
struct Indexes {
  char* raw; int stride; long long n;
  Indexes(const std::vector<int>& values, int stride_) : stride(stride_), n((long long)values.size()) {
    raw = static_cast<char*>(malloc((size_t)(n - 1) * stride + sizeof(int)));
    for (long long i = 0; i < n; ++i) memcpy(raw + i * stride, &values[(size_t)i], sizeof(int));
  }
  ~Indexes() { free(raw); }
  const int* data() const { return reinterpret_cast<const int*>(raw); }
};

void walk_steps()
{
  const int tight = (int)sizeof(void*), wide = 3 * (int)sizeof(void*);
  CHECK(0 == pointer_step(nullptr, 0) && 0 == pointer_step(nullptr, 1));
  CHECK(8 == pointer_step(&tight, 0) && 0 == pointer_step(&tight, 1)); // (the reference's correction: stride - index_base * sizeof(void*))
  CHECK(24 == pointer_step(&wide, 0) && 16 == pointer_step(&wide, 1));
  const int top = 2147483647;
  CHECK(2147483647ll - 8 == pointer_step(&top, 1));
  CHECK(1 == pointer_count(0, 7) && 7 == pointer_count(24, 7) && 1 == pointer_count(8, 1));
  CHECK(0 == tight_step(0) && 8 == tight_step(24) && 8 == tight_step(8));
  CHECK(5 == batch_size(5) && 5 == batch_size(-5) && 2147483648ll == batch_size(-2147483648ll));
  CHECK(c_verdict_needed(false, 7) && c_verdict_needed(false, 2));
  CHECK(!c_verdict_needed(true, 7) && !c_verdict_needed(false, -7) && !c_verdict_needed(false, 1) && !c_verdict_needed(false, 0));
  const LeadingDims nn = default_lds(false, false, 5, 4, 3), tn = default_lds(true, false, 5, 4, 3), nt = default_lds(false, true, 5, 4, 3);
  CHECK(5 == nn.a && 3 == nn.b && 5 == nn.c);
  CHECK(3 == tn.a && 3 == tn.b && 5 == tn.c);
  CHECK(5 == nt.a && 4 == nt.b && 5 == nt.c);
}

// every item belongs to exactly one task, in order, and no task but the last non-empty one is short
void walk_slices()
{
  const long long sizes[] = { 0, 1, 2, 7, 23, 64, 1000, 2147483647ll };
  const int tasks[] = { 1, 2, 3, 7, 8, 64, 1000 };
  for (const long long size : sizes) for (const int ntasks : tasks) {
    const long long tasksize = (size + ntasks - 1) / ntasks; // the reference's formula (src/libxsmm_gemm.c:1315-1324)
    long long next = 0;
    for (int tid = 0; tid < ntasks; ++tid) {
      const TaskSlice s = task_slice(size, tid, ntasks);
      CHECK(s.begin == (long long)tid * tasksize);
      if (s.begin < s.end) { CHECK(s.begin == next && s.end <= size && s.end - s.begin <= tasksize); next = s.end; }
      else CHECK(next == size); // empty slices only once the batch is used up (ntasks larger than the batch)
    }
    CHECK(next == size);
  }
  const TaskSlice one = task_slice(1, 2, 3); // batch 1, three tasks: the first takes it, the others nothing
  CHECK(one.end <= one.begin);
}

void walk_indexes()
{
  const int strides[] = { 4, 8, 12 };
  const int bases[] = { 0, 1 };
  const long long counts[] = { 1, 2, 7, 23, 100 };
  for (const int stride : strides) for (const int base : bases) for (const long long n : counts) for (int big = 0; big < 2; ++big) {
    std::vector<int> values((size_t)n);
    for (int& v : values) v = base + (int)(0 != big ? (2147483647u - 64u + lcg() % 64u) : lcg() % 100000u);
    if (0 != big) values[0] = base; // a range that spans (nearly) all of 31 bits
    const Indexes idx(values, stride);
    long long lo = values[0] - (long long)base, hi = lo;
    for (const int v : values) { const long long e = (long long)v - base; if (e < lo) lo = e; if (e > hi) hi = e; }
    const IndexRange r = index_range(idx.data(), stride, base, n);
    CHECK(r.lo == lo && r.hi == hi && 0 <= r.lo);
    for (long long b = 0; b < n; b += (n + 2) / 3) { // the array from a task's first item on
      const int* const at = index_at(idx.data(), b, stride);
      CHECK(*at == values[(size_t)b]);
      const IndexRange rest = index_range(at, stride, base, n - b);
      long long rlo = values[(size_t)b] - (long long)base, rhi = rlo;
      for (long long i = b; i < n; ++i) { const long long e = (long long)values[(size_t)i] - base; if (e < rlo) rlo = e; if (e > rhi) rhi = e; }
      CHECK(rest.lo == rlo && rest.hi == rhi);
    }
    // the hull in bytes: fp64 elements past 2^31 elements are past 2^34 bytes
    const unsigned long long basep = 0x7f0000000000ull; const size_t span = 22 * 23 + 23;
    unsigned long long hull[2];
    hull_of_indexes(hull, reinterpret_cast<const void*>(basep), idx.data(), stride, base, n, 8, span);
    CHECK(hull[0] == basep + (unsigned long long)lo * 8 && hull[1] == basep + (unsigned long long)hi * 8 + span * 8);
    if (0 != big && 1 < n) CHECK(hull[1] - hull[0] > (1ull << 33));
  }
  CHECK(nullptr == index_at(nullptr, 5, 4));
  const IndexRange none = index_range(nullptr, 4, 1, 7); // no index array: every item uses the base itself
  CHECK(0 == none.lo && 0 == none.hi);
  unsigned long long hull[2];
  hull_of_indexes(hull, reinterpret_cast<const void*>(4096), nullptr, 4, 1, 7, 4, 60);
  CHECK(4096 == hull[0] && 4096 + 240 == hull[1]);
}

void walk_pointers()
{
  const long long counts[] = { 1, 2, 7, 23 };
  const int strides[] = { 8, 24 }; // tight, wide
  const int bases[] = { 0, 1 };
  for (const long long n : counts) for (const int stride : strides) for (const int base : bases) {
    const long long step = pointer_step(&stride, base);
    if (0 == step && 1 < n) continue; // (stride 8, index_base 1: one operand for the whole batch -- below)
    // a stepped array in a block of exactly its size; matrices up to 2^40 bytes apart (offsets past 2^31 elements)
    char* const raw = static_cast<char*>(malloc((size_t)(n - 1) * (size_t)step + sizeof(void*)));
    std::vector<void*> want((size_t)n);
    for (long long i = 0; i < n; ++i) {
      want[(size_t)i] = reinterpret_cast<void*>(0x10000ull + ((unsigned long long)lcg() << 8));
      memcpy(raw + i * step, &want[(size_t)i], sizeof(void*));
    }
    std::vector<void*> tight(pointer_count(step, n));
    gather_pointers(tight, raw, step);
    CHECK(tight == want);
    unsigned long long lo = ~0ull, hi = 0;
    for (void* const p : want) { const unsigned long long q = reinterpret_cast<uintptr_t>(p); if (q < lo) lo = q; if (q > hi) hi = q; }
    unsigned long long hull[2];
    hull_of_pointers(hull, tight.data(), tight.size(), 4, 23 * 23);
    CHECK(hull[0] == lo && hull[1] == hi + 23 * 23 * 4);
    free(raw);
  }
  void* const one = reinterpret_cast<void*>(0x123400);
  std::vector<void*> tight(pointer_count(0, 7)); // step 0: a single pointer, whatever the batch
  gather_pointers(tight, &one, 0);
  CHECK(1 == tight.size() && one == tight[0]);
}

// naive: the slot of a matrix is the number of distinct matrices seen before its first use
void walk_unique_slots()
{
  auto P = [](int i) { return reinterpret_cast<void*>((uintptr_t)0x1000 * (uintptr_t)(i + 1)); };
  const std::vector<std::vector<int>> cases = {
    { 0 },                          // batch 1
    { 0, 0, 0, 1, 2, 3, 4 },        // a repeated C first
    { 0, 1, 2, 3, 4, 4, 4 },        // ... last
    { 5, 5, 5, 5, 5, 5, 5 },        // only a repeated C
    { 0, 0, 1, 1, 1, 2, 2 },        // consecutive runs
    { 0, 1, 0, 2, 1, 0, 3 },        // out of order: the map
    { 3, 3, 1, 3, 3, 1, 1 } };
  for (const std::vector<int>& ids : cases) {
    std::vector<void*> c; for (const int id : ids) c.push_back(P(id));
    std::vector<void*> uniq, want_uniq; std::vector<size_t> slot_of(c.size()), want_slot;
    unique_slots(c, uniq, slot_of);
    for (void* const p : c) {
      size_t j = 0;
      while (j < want_uniq.size() && want_uniq[j] != p) ++j;
      if (j == want_uniq.size()) want_uniq.push_back(p);
      want_slot.push_back(j);
    }
    CHECK(uniq == want_uniq && slot_of == want_slot);
  }
}

// "one segment" against "no pair meets" on small random tables, and the segments against a restatement
void walk_segments()
{
  auto meet = [](const unsigned long long* x, const unsigned long long* y) { return x[0] < y[1] && y[0] < x[1]; };
  for (int trial = 0; trial < 2000; ++trial) {
    const int n = 1 + (int)(lcg() % 8);
    const unsigned int space = (0 == trial % 3 ? 600u : (1 == trial % 3 ? 3000u : 40000u));
    std::vector<unsigned long long> hulls(6 * (size_t)n);
    for (size_t i = 0; i < hulls.size(); i += 2) { hulls[i] = 0xFFFF800000000000ull * (lcg() % 2) + lcg() % space; hulls[i + 1] = hulls[i] + 1 + lcg() % 120; }
    bool none = true;
    for (int x = 0; x < n; ++x) for (int y = 0; y < n; ++y) {
      const unsigned long long* const hx = hulls.data() + 6 * x, * const hy = hulls.data() + 6 * y;
      if (x != y && (meet(hx + 4, hy + 0) || meet(hx + 4, hy + 2) || (x < y && meet(hx + 4, hy + 4)))) none = false;
    }
    std::vector<int> segment((size_t)n, -1);
    const int segments = merge_segments(n, hulls.data(), segment.data());
    CHECK((1 == segments) == none);
    CHECK(0 == segment[0] && segments - 1 == segment[(size_t)n - 1]);
    for (int i = 1; i < n; ++i) CHECK(segment[(size_t)i] == segment[(size_t)i - 1] || segment[(size_t)i] == segment[(size_t)i - 1] + 1);
  }
  CHECK(0 == merge_segments(0, nullptr, nullptr));
}

} // namespace

int main()
{
  walk_steps();
  walk_slices();
  walk_indexes();
  walk_pointers();
  walk_unique_slots();
  walk_segments();
  if (0 != failures) { fprintf(stderr, "batch_resolve_walk: %d checks FAILED\n", failures); return EXIT_FAILURE; }
  printf("batch_resolve_walk: steps, slices, index ranges, hulls, gathered arrays, C slots and segments agree with their restatements\n");
  return EXIT_SUCCESS;
}
