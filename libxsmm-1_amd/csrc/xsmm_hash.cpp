// xsmm_hash.cpp -- libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n (include/libxsmm.h) and their extensions
// libxsmm_amd_hash_async / _hash_batch / _memcmp_async / _memcmp_batch (include/libxsmm_amd.h).
//
// Reference: src/libxsmm_math.c:260-263 with src/libxsmm_hash.c (CRC-32C, the register starts at the seed, nothing inverted),
// src/libxsmm_diff.c:131-146, src/libxsmm_diff.h:76-98. The definition is restated in kernels/hash_plan.h and DESIGN.md 8u.
// Operands that are all host memory (pageable, pinned or managed) take the loops of this file: nothing is launched. A call with
// an operand in plain device memory runs the kernels of kernels/hash.hip on the calling thread's stream. This file checks the
// arguments (before any device probe: a wrong call is quiet and writes nothing on any machine), stages pageable operands as the
// other entry points do, and decides who waits: a result in plain host memory is complete on return, a result in memory the
// GPU reaches is written by the last kernel and nobody waits.
#include "xsmm_internal.hpp"
#include "kernels/hash_plan.h"
#include "../../include/libxsmm_amd.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

namespace {

void complain(int* flag, const char* what, const char* msg)
{ // library code is expected to be mute: one line per entry point, only if asked for
  if (0 != libxsmm_verbosity && once(flag)) fprintf(stderr, "LIBXSMM ERROR: %s: %s\n", what, msg);
}

int report(int e, const char* name)
{
  if (0 == e) { note_launch(name); return EXIT_SUCCESS; }
  fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
  return EXIT_FAILURE;
}

// ---- host loops ------------------------------------------------------------------------------------------------------------
unsigned int host_hash(const void* data, size_t size, unsigned int seed)
{
  static const HashTables tables = hash_tables();
  const uint32_t* const t = &tables.t[0][0];
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t c = seed;
  for (; 4 <= size; size -= 4, p += 4) { // slicing by four; the value does not depend on how the bytes are chunked
    const uint32_t x = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    c = hash_dword(t, x);
  }
  for (; 0 < size; --size, ++p) c = hash_byte(t, c, *p);
  return c;
}

unsigned int host_diff_n(const unsigned char* a, const unsigned char* bn, unsigned int size, unsigned int stride, unsigned int hint, unsigned int n)
{
  for (unsigned int k = 0; k < n; ++k) { // hint, hint + 1, ..., n - 1, 0, ..., hint - 1
    const unsigned int i = (unsigned int)(((unsigned long long)hint + k) % n);
    if (0 == memcmp(a, bn + (size_t)i * stride, size)) return i;
  }
  return n;
}

// ---- device path -------------------------------------------------------------------------------------------------------------
// `value` into count results of any kind of memory (a call with nothing to read)
int write_neutral(unsigned int* out, long long count, unsigned int value)
{
  const int kind = pointer_kind(out);
  for (long long i = 0; i < count; ++i) {
    if (1 == kind) { if (0 != h2d(out + i, &value, sizeof(value))) { (void)hipGetLastError(); return EXIT_FAILURE; } }
    else out[i] = value;
  }
  if (1 == kind && 0 < count && 0 != stream_sync()) return EXIT_FAILURE; // (the copies read a local)
  return EXIT_SUCCESS;
}

int write_first(long long* out, long long value)
{
  if (nullptr == out) return EXIT_SUCCESS;
  if (1 == pointer_kind(out)) return (0 == h2d(out, &value, sizeof(value)) && 0 == stream_sync()) ? EXIT_SUCCESS : EXIT_FAILURE;
  *out = value;
  return EXIT_SUCCESS;
}

enum Form { FORM_SYNC = 0 /* the reference's functions */, FORM_ASYNC = 1, FORM_BATCH = 2 };

int hash_run(Form form, bool compare, unsigned int* results, long long* first_diff, const void* a, const void* b, size_t line_bytes,
  long long lines, long long lda, long long ldb, long long stride_a, long long stride_b, long long batch, unsigned int seed, const char* what, int* flag)
{
  if (nullptr == results) { complain(flag, what, "the result cannot be NULL!"); return EXIT_FAILURE; }
  if (lines < 0 || batch < 0 || stride_a < 0 || stride_b < 0) { complain(flag, what, "counts and strides cannot be negative!"); return EXIT_FAILURE; }
  if (1 < lines && (lda < 0 || (size_t)lda < line_bytes || (compare && (ldb < 0 || (size_t)ldb < line_bytes)))) {
    complain(flag, what, "a line cannot exceed the leading dimension!"); return EXIT_FAILURE;
  }
  if (0 != line_bytes && 0 < lines && (size_t)lines > ((size_t)-1 >> 1) / line_bytes) { complain(flag, what, "the item is too large!"); return EXIT_FAILURE; }
  const bool empty = (0 == line_bytes || 0 == lines || 0 == batch);
  if (!empty && (nullptr == a || (compare && nullptr == b))) { complain(flag, what, "an operand cannot be NULL!"); return EXIT_FAILURE; }
  if (empty) { // nothing to read: the seed or "equal" per item, nothing is launched
    if (EXIT_SUCCESS != write_first(first_diff, -1)) return EXIT_FAILURE;
    return write_neutral(results, FORM_BATCH == form ? batch : 1, compare ? 0u : seed);
  }
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  const int kind_results = pointer_kind(results), kind_first = pointer_kind(first_diff);
  if (FORM_ASYNC == form && 0 == (kind_results & 1)) { complain(flag, what, "the result must be memory the GPU reaches!"); return EXIT_FAILURE; }

  HashArgs args; memset(&args, 0, sizeof(args));
  args.a = a; args.b = b; args.line_bytes = line_bytes; args.lines = lines; args.lda = (1 < lines ? lda : 0); args.ldb = (1 < lines ? ldb : 0);
  args.stride_a = stride_a; args.stride_b = stride_b; args.batch = batch; args.seed = seed; args.compare = compare ? 1 : 0;

  // operands the GPU does not reach are staged
  const size_t ext_a = (size_t)(batch - 1) * (size_t)stride_a + (size_t)(lines - 1) * (size_t)args.lda + line_bytes;
  const size_t ext_b = (size_t)(batch - 1) * (size_t)stride_b + (size_t)(lines - 1) * (size_t)args.ldb + line_bytes;
  if (0 == (pointer_kind(a) & 1)) {
    void* const p = scratch(0, ext_a);
    if (nullptr == p || 0 != h2d(p, a, ext_a)) return EXIT_FAILURE;
    args.a = p;
  }
  if (compare && 0 == (pointer_kind(b) & 1)) {
    void* const p = scratch(1, ext_b);
    if (nullptr == p || 0 != h2d(p, b, ext_b)) return EXIT_FAILURE;
    args.b = p;
  }

  // the workspace: [the lowest differing item][the partials of a large item][staged results][staged first_diff]
  const bool stage_results = (0 == (kind_results & 1)), stage_first = (nullptr != first_diff && 0 == (kind_first & 1));
  const size_t head = sizeof(long long) + sizeof(unsigned int) * HASH_MAX_BLOCKS, nres = (size_t)(FORM_BATCH == form ? batch : 1);
  char* const ws = static_cast<char*>(scratch(8, head + (stage_results ? sizeof(unsigned int) * nres : 0) + sizeof(long long)));
  if (nullptr == ws) return EXIT_FAILURE;
  long long* const ws_first = reinterpret_cast<long long*>(ws);
  unsigned int* const partial = reinterpret_cast<unsigned int*>(ws + sizeof(long long));
  unsigned int* const d_results = stage_results ? reinterpret_cast<unsigned int*>(ws + head) : results;
  long long* const d_first = stage_first ? reinterpret_cast<long long*>(ws + head + (stage_results ? sizeof(unsigned int) * nres : 0)) : first_diff;

  int rc = EXIT_SUCCESS;
  if (nullptr != first_diff) rc = (0 == launch_hash_first(ws_first, nullptr, true, stream)) ? EXIT_SUCCESS : EXIT_FAILURE;
  if (EXIT_SUCCESS != rc) return rc;
  if (FORM_BATCH == form && hash_small(line_bytes, lines)) {
    rc = report(launch_hash_items(args, d_results, nullptr != first_diff ? ws_first : nullptr, stream), compare ? "memcmp_items" : "hash_items");
  }
  else {
    HashArgs one = args; one.batch = 1;
    for (long long i = 0; i < batch && EXIT_SUCCESS == rc; ++i) { // large items one after the other: each fills the chip
      one.a = static_cast<const char*>(args.a) + (size_t)i * (size_t)stride_a;
      one.b = (compare ? static_cast<const char*>(args.b) + (size_t)i * (size_t)stride_b : nullptr);
      one.item0 = i;
      rc = report(launch_hash_units(one, partial, d_results + i, nullptr != first_diff ? ws_first : nullptr, stream), compare ? "memcmp_units" : "hash_units");
    }
  }
  if (EXIT_SUCCESS == rc && nullptr != first_diff) rc = report(launch_hash_first(ws_first, d_first, false, stream), "hash_first");
  if (EXIT_SUCCESS != rc) return rc;

  if (stage_results || stage_first) { // one copy per staged result, then one wait
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (stage_results) e = hipMemcpyAsync(results, d_results, sizeof(unsigned int) * nres, hipMemcpyDefault, st);
    if (hipSuccess == e && stage_first) e = hipMemcpyAsync(first_diff, d_first, sizeof(*first_diff), hipMemcpyDefault, st);
    if (hipSuccess == e) e = hipStreamSynchronize(st);
    if (hipSuccess != e) { (void)hipGetLastError(); return EXIT_FAILURE; }
  }
  return EXIT_SUCCESS;
}

bool on_device(const void* p) { return 1 == pointer_kind(p); } // plain device memory (false without a device)

} // namespace

// ---- the reference's functions -------------------------------------------------------------------------------------------------
LIBXSMM_API unsigned int libxsmm_hash(const void* data, unsigned int size, unsigned int seed)
{
  static int error_once = 0;
  if (0 == size) return seed;
  if (nullptr == data) { complain(&error_once, "libxsmm_hash", "data cannot be NULL!"); return seed; }
  if (!on_device(data)) return host_hash(data, size, seed);
  unsigned int result = seed;
  if (EXIT_SUCCESS != hash_run(FORM_SYNC, false, &result, nullptr, data, nullptr, size, 1, 0, 0, 0, 0, 1, seed, "libxsmm_hash", &error_once)) return seed;
  return result;
}

LIBXSMM_API int libxsmm_memcmp(const void* a, const void* b, size_t size)
{
  static int error_once = 0;
  if (0 == size) return 0;
  if (nullptr == a || nullptr == b) { complain(&error_once, "libxsmm_memcmp", "an operand cannot be NULL!"); return 0; }
  if (!on_device(a) && !on_device(b)) return 0 != memcmp(a, b, size) ? 1 : 0;
  unsigned int result = 0;
  if (EXIT_SUCCESS != hash_run(FORM_SYNC, true, &result, nullptr, a, b, size, 1, 0, 0, 0, 0, 1, 0, "libxsmm_memcmp", &error_once)) return 0;
  return (int)result;
}

LIBXSMM_API unsigned char libxsmm_diff(const void* a, const void* b, unsigned char size)
{
  static int error_once = 0;
  if (0 == size) return 0;
  if (nullptr == a || nullptr == b) { complain(&error_once, "libxsmm_diff", "an operand cannot be NULL!"); return 0; }
  if (!on_device(a) && !on_device(b)) return 0 != memcmp(a, b, size) ? 1 : 0;
  unsigned int result = 0;
  if (EXIT_SUCCESS != hash_run(FORM_SYNC, true, &result, nullptr, a, b, size, 1, 0, 0, 0, 0, 1, 0, "libxsmm_diff", &error_once)) return 0;
  return (unsigned char)result;
}

LIBXSMM_API unsigned int libxsmm_diff_n(const void* a, const void* bn, unsigned char size, unsigned char stride, unsigned int hint, unsigned int n)
{
  static int error_once = 0;
  if (0 == n) return 0;
  hint %= n; // (the reference reads out of bounds for hint >= n)
  if (0 == size) return hint; // nothing differs: the first item visited
  if (nullptr == a || nullptr == bn) { complain(&error_once, "libxsmm_diff_n", "an operand cannot be NULL!"); return 0; }
  if (!on_device(a) && !on_device(bn)) return host_diff_n(static_cast<const unsigned char*>(a), static_cast<const unsigned char*>(bn), size, stride, hint, n);
  if (!device_ready()) { fail_no_device("libxsmm_diff_n"); return 0; }
  void* const stream = device().stream;
  DiffKey key; memset(&key, 0, sizeof(key));
  const void* d_a = a;
  if (0 == (pointer_kind(a) & 1)) { memcpy(key.b, a, size); d_a = nullptr; }
  const void* d_bn = bn;
  if (0 == (pointer_kind(bn) & 1)) {
    const size_t ext = (size_t)(n - 1) * stride + size;
    void* const p = scratch(1, ext);
    if (nullptr == p || 0 != h2d(p, bn, ext)) return 0;
    d_bn = p;
  }
  unsigned int* const best = static_cast<unsigned int*>(scratch(8, sizeof(long long)));
  unsigned int r = 0xffffffffu;
  if (nullptr == best || EXIT_SUCCESS != report(launch_diff_n(key, d_a, d_bn, size, stride, hint, n, best, stream), "diff_n") || 0 != d2h(&r, best, sizeof(r))) {
    (void)hipGetLastError();
    return 0;
  }
  return 0xffffffffu == r ? n : (unsigned int)(((unsigned long long)r + hint) % n);
}

// ---- extensions ----------------------------------------------------------------------------------------------------------------
LIBXSMM_API int libxsmm_amd_hash_async(unsigned int* result, const void* data, size_t size, unsigned int seed)
{
  static int error_once = 0;
  return hash_run(FORM_ASYNC, false, result, nullptr, data, nullptr, size, 1, 0, 0, 0, 0, 1, seed, "libxsmm_amd_hash_async", &error_once);
}

LIBXSMM_API int libxsmm_amd_hash_batch(unsigned int* results, const void* data, size_t line_bytes, long long lines, long long ld, long long stride,
  long long batch, unsigned int seed)
{
  static int error_once = 0;
  return hash_run(FORM_BATCH, false, results, nullptr, data, nullptr, line_bytes, lines, ld, 0, stride, 0, batch, seed, "libxsmm_amd_hash_batch", &error_once);
}

LIBXSMM_API int libxsmm_amd_memcmp_async(int* result, const void* a, const void* b, size_t size)
{
  static int error_once = 0;
  return hash_run(FORM_ASYNC, true, reinterpret_cast<unsigned int*>(result), nullptr, a, b, size, 1, 0, 0, 0, 0, 1, 0, "libxsmm_amd_memcmp_async", &error_once);
}

LIBXSMM_API int libxsmm_amd_memcmp_batch(int* results, long long* first_diff, const void* a, const void* b, size_t line_bytes, long long lines,
  long long lda, long long ldb, long long stride_a, long long stride_b, long long batch)
{
  static int error_once = 0;
  return hash_run(FORM_BATCH, true, reinterpret_cast<unsigned int*>(results), first_diff, a, b, line_bytes, lines, lda, ldb, stride_a, stride_b, batch, 0,
    "libxsmm_amd_memcmp_batch", &error_once);
}
