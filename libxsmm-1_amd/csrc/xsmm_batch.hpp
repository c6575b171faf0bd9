// xsmm_batch.hpp -- the address arithmetic of a batch call, each rule once: what the entry points, the recorders and the thunks
// (xsmm_gemm.cpp, xsmm_batch.cpp, xsmm_batch_record.cpp, xsmm_call.cpp) work out before anything is staged or launched. Pure
// host code without a HIP header: tools/batch_resolve_walk.cpp walks it under the sanitizers. Every offset is 64-bit.
#ifndef XSMM_BATCH_HPP
#define XSMM_BATCH_HPP

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace xsmm {

// Arrays of pointers: *stride is the byte distance between consecutive pointers (reference src/libxsmm_gemm.c:1426-1428,
// including its index_base*sizeof(void*) correction); NULL: one operand for the whole batch.
inline long long pointer_step(const int* stride, int index_base) { return nullptr != stride ? ((long long)*stride - (long long)index_base * (long long)sizeof(void*)) : 0; }
inline size_t pointer_count(long long step, long long n) { return 0 != step ? (size_t)n : 1; } // pointers such an array holds
inline long long tight_step(long long step) { return 0 != step ? (long long)sizeof(void*) : 0; } // the step of its gathered form

// the pointers of a stepped array as a tight one: tight arrives with pointer_count(step, n) entries
template<typename P> void gather_pointers(std::vector<P>& tight, const void* array, long long step)
{
  for (size_t i = 0; i < tight.size(); ++i) tight[i] = *reinterpret_cast<const P*>(static_cast<const char*>(array) + step * (long long)i);
}

// Task `tid` of `ntasks` owns the items [begin, end) of the batch (reference src/libxsmm_gemm.c:1315-1324); end <= begin: none.
struct TaskSlice { long long begin, end; };
inline TaskSlice task_slice(long long size, int tid, int ntasks)
{
  const long long tasksize = (size + ntasks - 1) / ntasks;
  const long long begin = (long long)tid * tasksize, span = begin + tasksize;
  return TaskSlice{ begin, span < size ? span : size };
}
inline long long batch_size(long long signed_size) { return signed_size < 0 ? -signed_size : signed_size; } // (negative: nothing is shared)

// the leading dimensions BLAS assumes where the caller passes none
struct LeadingDims { long long a, b, c; };
inline LeadingDims default_lds(bool trans_a, bool trans_b, long long m, long long n, long long k) { return LeadingDims{ trans_a ? k : m, trans_b ? n : k, m }; }

// How the C blocks of a batch repeat must be found out (on the device) unless nobody cares: beta == 0, the caller's promise of
// a negative size, a single item. (One C for the whole batch is found out there as well: all neighbours equal.)
inline bool c_verdict_needed(bool beta0, long long signed_size) { return !(beta0 || signed_size < 0 || batch_size(signed_size) < 2); }

// an index array from item `begin` on (NULL stays NULL: every item uses the base itself)
inline const int* index_at(const int* idx, long long begin, int index_stride) { return nullptr != idx ? reinterpret_cast<const int*>(reinterpret_cast<const char*>(idx) + begin * index_stride) : nullptr; }

struct IndexRange { long long lo, hi; }; // element index range [lo, hi] used by an index array
inline IndexRange index_range(const int* idx, int index_stride, int index_base, long long n)
{
  IndexRange r = { 0, 0 };
  if (nullptr == idx || 0 == n) return r;
  r.lo = r.hi = (long long)(*idx) - index_base;
  for (long long i = 1; i < n; ++i) {
    const long long v = (long long)(*index_at(idx, i, index_stride)) - index_base;
    if (v < r.lo) r.lo = v;
    if (v > r.hi) r.hi = v;
  }
  return r;
}

// Address hulls {lo, hi} of one operand of a call, byte addresses, half-open; span: elements one operand touches.
inline void hull_of_indexes(unsigned long long* out, const void* base, const int* idx, int index_stride, int index_base, long long n, int typesize, size_t span)
{ // (a NULL index array: every item uses the base itself, see resolve() in kernels/smm_common.cuh)
  const IndexRange r = index_range(idx, index_stride, index_base, n);
  const unsigned long long p = reinterpret_cast<uintptr_t>(base);
  out[0] = p + (unsigned long long)(r.lo * typesize);
  out[1] = p + (unsigned long long)(r.hi * typesize) + (unsigned long long)span * typesize;
}

inline void hull_of_pointers(unsigned long long* out, const void* const* ptrs, size_t n, int typesize, size_t span)
{
  unsigned long long lo = reinterpret_cast<uintptr_t>(ptrs[0]), hi = lo;
  for (size_t i = 1; i < n; ++i) { const unsigned long long q = reinterpret_cast<uintptr_t>(ptrs[i]); if (q < lo) lo = q; if (q > hi) hi = q; }
  out[0] = lo; out[1] = hi + (unsigned long long)span * typesize;
}

// When calls may run side by side, for the calls recorded inside a bracket and for the groups of ?gemm_batch alike: a call's
// C must not meet another member's A, B or C. Calls leave in segments: consecutive calls that may run side by side. A call
// that conflicts with a member of the open segment opens a new one -- it then runs behind all of them, in call order. ("One
// segment" says the same as "no pair of calls meets".)
// hulls: {a_lo, a_hi, b_lo, b_hi, c_lo, c_hi} per call, byte addresses, half-open. segment_of[i] receives the segment of call i
// (0, 1, ...; non-decreasing); returns the number of segments.
inline int merge_segments(int n, const unsigned long long* hulls, int* segment_of)
{
  auto meet = [](const unsigned long long* x, const unsigned long long* y) { return x[0] < y[1] && y[0] < x[1]; }; // half-open ranges
  int first = 0, segment = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned long long* const hi = hulls + 6 * (size_t)i;
    for (int j = first; j < i; ++j) {
      const unsigned long long* const hj = hulls + 6 * (size_t)j;
      if (meet(hi + 4, hj + 0) || meet(hi + 4, hj + 2) || meet(hi + 4, hj + 4) || meet(hj + 4, hi + 0) || meet(hj + 4, hi + 2)) {
        first = i; ++segment;
        break;
      }
    }
    segment_of[i] = segment;
  }
  return 0 < n ? segment + 1 : 0;
}

// Host C matrices that are staged: distinct matrices get distinct device copies, repeated pointers share one. uniq receives the
// distinct pointers in order of first use, slot_of[i] (one entry per item on arrival) the position of item i's matrix among them.
inline void unique_slots(const std::vector<void*>& c, std::vector<void*>& uniq, std::vector<size_t>& slot_of)
{
  std::unordered_map<void*, size_t> seen; seen.reserve(c.size());
  for (size_t i = 0; i < c.size(); ++i) {
    size_t j;
    if (!uniq.empty() && uniq.back() == c[i]) j = uniq.size() - 1; // consecutive duplicates are the common case (CP2K stacks)
    else {
      const auto it = seen.find(c[i]);
      if (it != seen.end()) j = it->second; else { j = uniq.size(); uniq.push_back(c[i]); seen.emplace(c[i], j); }
    }
    slot_of[i] = j;
  }
}

} // namespace xsmm

#endif
