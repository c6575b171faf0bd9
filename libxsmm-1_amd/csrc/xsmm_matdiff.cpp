// xsmm_matdiff.cpp -- libxsmm_matdiff for operands in device memory, libxsmm_amd_matdiff_async and libxsmm_amd_matdiff_batch
// (include/libxsmm_amd.h).
//
// Reference: src/libxsmm_math.c:48-238 with src/template/libxsmm_matdiff.tpl.c -- one CPU thread walks both matrices twice.
// Here the walks are kernels of kernels/matdiff.hip queued back to back on the calling thread's stream: the
// second pass takes the averages from device memory, so no host round trip sits between them. This file checks the arguments
// (before any device probe: a wrong call is quiet and writes nothing on any machine), stages pageable operands as the other
// entry points do, and decides who waits: a result in plain host memory is complete on return, a result in memory the GPU
// reaches is written by the last kernel and nobody waits. libxsmm_matdiff itself (xsmm_util.cpp) comes here only if an operand
// is plain device memory; two host operands take the host loop as before.
#include "xsmm_internal.hpp"
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

size_t type_size(int datatype)
{
  switch (datatype) {
    case LIBXSMM_DATATYPE_F64: return 8;
    case LIBXSMM_DATATYPE_F32: case LIBXSMM_DATATYPE_I32: return 4;
    case LIBXSMM_DATATYPE_I16: return 2;
    case LIBXSMM_DATATYPE_I8: return 1;
    default: return 0;
  }
}

// one load per four elements: 16 bytes (fp64: two of them), 8 bytes of i16, 4 bytes of i8
bool vector_loads(const void* p, size_t ts, long long ld, long long stride)
{
  const long long unit = (8 == ts ? 2 : 4);
  return 0 == reinterpret_cast<uintptr_t>(p) % (size_t)(unit * ts) && 0 == ld % unit && 0 == stride % unit;
}

// cleared infos into memory of any kind (a call with nothing to compare)
int write_cleared(libxsmm_matdiff_info* out, long long count)
{
  libxsmm_matdiff_info c;
  libxsmm_matdiff_clear(&c);
  const int kind = pointer_kind(out);
  for (long long i = 0; i < count; ++i) {
    if (1 == kind) { if (0 != h2d(out + i, &c, sizeof(c))) { (void)hipGetLastError(); return EXIT_FAILURE; } }
    else out[i] = c;
  }
  return EXIT_SUCCESS;
}

enum Form { FORM_SYNC = 0 /* libxsmm_matdiff */, FORM_ASYNC = 1, FORM_BATCH = 2 };

int matdiff_run(Form form, libxsmm_matdiff_info* info, libxsmm_matdiff_info* items, long long* item, libxsmm_datatype datatype,
  libxsmm_blasint m, libxsmm_blasint n, const void* ref, const void* tst, const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst,
  long long stride_ref, long long stride_tst, long long batch, const char* what, int* flag)
{
  int swap_ref = 0;
  // (src/libxsmm_math.c:53-54 swaps the operands, not the pitches: a lone operand is walked by ldref, and here by stride_ref)
  if (nullptr == ref && nullptr != tst) { ref = tst; tst = nullptr; swap_ref = 1; }
  const size_t ts = type_size((int)datatype);
  if (nullptr == info || nullptr == ref) { complain(flag, what, "info and an operand cannot be NULL!"); return EXIT_FAILURE; }
  if (0 == ts) { complain(flag, what, "unsupported data-type requested!"); return EXIT_FAILURE; }
  if (m < 0 || n < 0 || batch < 0 || stride_ref < 0 || stride_tst < 0) { complain(flag, what, "sizes and strides cannot be negative!"); return EXIT_FAILURE; }
  const long long ldr = (nullptr != ldref ? *ldref : m), ldt = (nullptr != ldtst ? *ldtst : m);
  if (m > ldr || m > ldt) { complain(flag, what, "m cannot exceed the leading dimensions!"); return EXIT_FAILURE; }
  if (0 == m || 0 == n || 0 == batch) { // nothing to compare: cleared results, nothing is launched
    if (FORM_BATCH == form) {
      if (nullptr != item) { const long long none = -1; if (1 == pointer_kind(item)) { if (0 != h2d(item, &none, sizeof(none))) return EXIT_FAILURE; } else *item = none; }
      if (nullptr != items && EXIT_SUCCESS != write_cleared(items, batch)) return EXIT_FAILURE;
    }
    return write_cleared(info, 1);
  }
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  const int kind_info = pointer_kind(info), kind_items = pointer_kind(items), kind_item = pointer_kind(item);
  if (FORM_ASYNC == form && 0 == (kind_info & 1)) { complain(flag, what, "info must be memory the GPU reaches!"); return EXIT_FAILURE; }

  MatdiffArgs a; memset(&a, 0, sizeof(a));
  a.datatype = (int)datatype; a.batch = batch; a.sr = stride_ref; a.st = stride_tst;
  int swap_norms = 0;
  if (1 == n) { a.mm = m; a.nn = 1; a.ldr = a.ldt = m; swap_norms = 1; } // a vector: one contiguous line
  else { a.mm = m; a.nn = n; a.ldr = ldr; a.ldt = ldt; }
  const long long size = a.mm * a.nn;

  // operands the GPU does not reach are staged
  const size_t ext_r = ((size_t)(batch - 1) * (size_t)a.sr + (size_t)(a.nn - 1) * (size_t)a.ldr + (size_t)a.mm) * ts;
  const size_t ext_t = ((size_t)(batch - 1) * (size_t)a.st + (size_t)(a.nn - 1) * (size_t)a.ldt + (size_t)a.mm) * ts;
  a.ref = ref; a.tst = tst;
  if (0 == (pointer_kind(ref) & 1)) {
    void* const p = scratch(0, ext_r);
    if (nullptr == p || 0 != h2d(p, ref, ext_r)) return EXIT_FAILURE;
    a.ref = p;
  }
  if (nullptr != tst && 0 == (pointer_kind(tst) & 1)) {
    void* const p = scratch(1, ext_t);
    if (nullptr == p || 0 != h2d(p, tst, ext_t)) return EXIT_FAILURE;
    a.tst = p;
  }
  a.vec_ref = vector_loads(a.ref, ts, a.ldr, a.sr) ? 1 : 0;
  a.vec_tst = (nullptr != a.tst && vector_loads(a.tst, ts, a.ldt, a.st)) ? 1 : 0;

  // the workspace: the items' records, two rows of records for the levels of the reduction, the partials of a tiled item
  const bool small = matdiff_small(a.mm, a.nn);
  const long long level1 = matdiff_reduce_records(batch), level2 = matdiff_reduce_records(level1);
  MatdiffArgs one = a; one.batch = 1;
  const size_t ws_tiled = small ? 0 : matdiff_tiled_workspace(one);
  const size_t nrec = (size_t)(batch + level1 + level2);
  char* const ws = static_cast<char*>(scratch(6, nrec * sizeof(MatdiffRecord) + ws_tiled));
  if (nullptr == ws) return EXIT_FAILURE;
  MatdiffRecord* const rec = reinterpret_cast<MatdiffRecord*>(ws);
  MatdiffRecord* level[2] = { rec + batch, rec + batch + level1 };
  void* const tiled = ws + nrec * sizeof(MatdiffRecord);

  // results that the GPU does not reach are staged: [info][items][item]
  const bool stage_info = (0 == (kind_info & 1)), stage_items = (nullptr != items && 0 == (kind_items & 1)), stage_item = (nullptr != item && 0 == (kind_item & 1));
  char* staged = nullptr;
  if (stage_info || stage_items || stage_item) {
    staged = static_cast<char*>(scratch(2, sizeof(libxsmm_matdiff_info) * (size_t)(1 + batch) + sizeof(long long)));
    if (nullptr == staged) return EXIT_FAILURE;
  }
  libxsmm_matdiff_info* const d_info = stage_info ? reinterpret_cast<libxsmm_matdiff_info*>(staged) : info;
  libxsmm_matdiff_info* const d_items = stage_items ? reinterpret_cast<libxsmm_matdiff_info*>(staged) + 1 : items;
  long long* const d_item = stage_item ? reinterpret_cast<long long*>(staged + sizeof(libxsmm_matdiff_info) * (size_t)(1 + batch)) : item;

  int rc;
  if (small) rc = report(launch_matdiff_items(a, rec, stream), "matdiff_items");
  else {
    rc = EXIT_SUCCESS;
    for (long long i = 0; i < batch && EXIT_SUCCESS == rc; ++i) { // large items one after the other: each fills the chip
      one.ref = static_cast<const char*>(a.ref) + (size_t)i * (size_t)a.sr * ts;
      one.tst = (nullptr != a.tst ? static_cast<const char*>(a.tst) + (size_t)i * (size_t)a.st * ts : nullptr);
      one.item0 = i;
      rc = report(launch_matdiff_tiled(one, tiled, rec + i, stream), "matdiff_tiles");
    }
  }
  if (EXIT_SUCCESS != rc) return rc;
  if (FORM_BATCH != form) rc = report(launch_matdiff_emit(rec, 1, d_info, nullptr, swap_norms, swap_ref, 0.0, stream), "matdiff_emit");
  else {
    if (nullptr != items) rc = report(launch_matdiff_emit(rec, batch, d_items, nullptr, swap_norms, swap_ref, 0.0, stream), "matdiff_emit");
    const MatdiffRecord* in = rec;
    long long count = batch;
    for (int l = 0; EXIT_SUCCESS == rc; l ^= 1) { // 1024 records to one per level (a batch of one as well: the reduction starts from a cleared info)
      rc = report(launch_matdiff_reduce(in, count, level[l], stream), "matdiff_reduce");
      in = level[l]; count = matdiff_reduce_records(count);
      if (1 == count) break;
    }
    if (EXIT_SUCCESS == rc) rc = report(launch_matdiff_emit(in, 1, d_info, d_item, swap_norms, swap_ref, (double)size * (double)batch, stream), "matdiff_emit");
  }
  if (EXIT_SUCCESS != rc) return rc;

  if (nullptr != staged) { // one copy per staged result, then one wait
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (stage_info) e = hipMemcpyAsync(info, d_info, sizeof(*info), hipMemcpyDefault, st);
    if (hipSuccess == e && stage_items) e = hipMemcpyAsync(items, d_items, sizeof(*items) * (size_t)batch, hipMemcpyDefault, st);
    if (hipSuccess == e && stage_item) e = hipMemcpyAsync(item, d_item, sizeof(*item), hipMemcpyDefault, st);
    if (hipSuccess == e) e = hipStreamSynchronize(st);
    if (hipSuccess != e) { (void)hipGetLastError(); return EXIT_FAILURE; }
  }
  else if (FORM_SYNC == form) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

} // namespace

namespace xsmm {

bool matdiff_route(libxsmm_matdiff_info* info, libxsmm_datatype datatype, libxsmm_blasint m, libxsmm_blasint n, const void* ref, const void* tst,
  const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst, int* rc)
{
  static int error_once = 0;
  if (1 != pointer_kind(ref) && 1 != pointer_kind(tst)) return false; // (0 without a device)
  *rc = matdiff_run(FORM_SYNC, info, nullptr, nullptr, datatype, m, n, ref, tst, ldref, ldtst, 0, 0, 1, "libxsmm_matdiff", &error_once);
  return true;
}

} // namespace xsmm

LIBXSMM_API int libxsmm_amd_matdiff_async(libxsmm_matdiff_info* info, libxsmm_datatype datatype, libxsmm_blasint m, libxsmm_blasint n,
  const void* ref, const void* tst, const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst)
{
  static int error_once = 0;
  return matdiff_run(FORM_ASYNC, info, nullptr, nullptr, datatype, m, n, ref, tst, ldref, ldtst, 0, 0, 1, "libxsmm_amd_matdiff_async", &error_once);
}

LIBXSMM_API int libxsmm_amd_matdiff_batch(libxsmm_matdiff_info* info, libxsmm_matdiff_info* items, long long* item, libxsmm_datatype datatype,
  libxsmm_blasint m, libxsmm_blasint n, const void* ref, const void* tst, const libxsmm_blasint* ldref, const libxsmm_blasint* ldtst,
  long long stride_ref, long long stride_tst, long long batch)
{
  static int error_once = 0;
  return matdiff_run(FORM_BATCH, info, items, item, datatype, m, n, ref, tst, ldref, ldtst, stride_ref, stride_tst, batch, "libxsmm_amd_matdiff_batch", &error_once);
}
