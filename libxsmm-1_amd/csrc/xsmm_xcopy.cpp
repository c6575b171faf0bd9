// xsmm_xcopy.cpp -- matrix copy and transposition: libxsmm_matcopy / otrans / itrans with their _thread and _omp forms, the
// dispatched mcopy / trans kernels, and the stack forms libxsmm_amd_{matcopy,otrans}_batch[_ptr].
//
// Reference: src/libxsmm_xcopy.c (argument checks :174-177, :295-298, :386-421; task split :244-275), the descriptors of
// src/libxsmm_main.h:171-190 with their initialisers (src/libxsmm_generator.c:339-381) and libxsmm_dispatch_mcopy / _trans
// (src/template/libxsmm.h:259-263). There the work is CPU loops over tiles plus JIT-generated AVX kernels for a tile; here it
// is the kernels of kernels/xcopy.hip. This file checks the arguments (before any device probe: a wrong call
// is quiet and writes nothing on any machine), picks the unit the data moves in -- the largest power of two up to 16 bytes
// that divides the typesize and every address involved -- and the path, and applies the memory rules of the other entry
// points: memory the GPU reaches is processed in place, host-visible memory is complete on return, pageable memory is staged.
#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

using namespace xsmm;

// the reference's descriptor layouts (src/libxsmm_main.h:171-190)
#pragma pack(push, 1)
struct libxsmm_mcopy_descriptor { unsigned int m, n, ldi, ldo; unsigned char typesize, unroll_level, prefetch, flags; };
struct libxsmm_trans_descriptor { unsigned int m, n, ldo; unsigned char typesize; };
#pragma pack(pop)
static_assert(sizeof(libxsmm_mcopy_descriptor) == 20 && sizeof(libxsmm_trans_descriptor) == 13, "xcopy descriptors");

namespace {

constexpr int OP_COPY = 0, OP_TRANS = 1, OP_ITRANS = 2;
constexpr size_t STACK_LDS_MAX = 64 * 1024;    // an item's image must fit the LDS a work-group can have
constexpr size_t STACK_LDS_CHUNK = 16 * 1024;  // items per chunk: as many as fit this (eight and more work-groups per CU)

void complain(int* flag, const char* msg)
{ // library code is expected to be mute: one line per process, only if asked for
  if (0 != libxsmm_verbosity && once(flag)) fprintf(stderr, "LIBXSMM ERROR: %s\n", msg);
}

int unit_of(unsigned ts, uintptr_t address_bits)
{
  int u = 16;
  while (u > 1 && (0 != ts % (unsigned)u || 0 != (address_bits & (uintptr_t)(u - 1)))) u >>= 1;
  return u;
}
uintptr_t bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }
bool mult16(const void* p, long long pitch_bytes) { return 0 == ((bits(p) | (uintptr_t)pitch_bytes) & 15); }

int report(int e, const char* name)
{
  note_launch(name);
  if (0 == e) return EXIT_SUCCESS;
  fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
  return EXIT_FAILURE;
}

// ---- operands the GPU reaches ------------------------------------------------------------------------------------------
int dev_copy(void* out, const void* in, long long rowbytes, long long ncols, long long pin, long long pout, void* stream)
{
  if (pout == rowbytes && (nullptr == in || pin == rowbytes)) { rowbytes *= ncols; ncols = 1; } // one run of bytes
  uintptr_t b = bits(out) | bits(in);
  if (1 < ncols) b |= (uintptr_t)pout | (nullptr != in ? (uintptr_t)pin : 0);
  return report(launch_xcopy_copy(unit_of(16, b), in, out, rowbytes, ncols, pin, pout, stream), nullptr != in ? "xcopy_copy" : "xcopy_zero");
}

// the plan of a stack transposition: through LDS where an item's image fits, without it otherwise
int dev_stack_trans(StackMove a, int unit, bool inplace, void* stream)
{
  const int mP = a.m * a.P;
  int mp = mP;
  if (4 <= unit) mp |= 1;                          // an odd number of units per column (kernels/xcopy.hip: banks)
  else if (2 == unit) { while (2 != mp % 4) ++mp; }  // ... (pitch in bytes) / 4 odd
  else { while (4 != mp % 8) ++mp; }
  const size_t item_bytes = (size_t)a.n * mp * unit;
  const char* name = "";
  a.mp = mp; a.G = 0;
  if (item_bytes <= STACK_LDS_MAX) {
    long long g = (long long)(STACK_LDS_CHUNK / item_bytes);
    if (g < 1) g = 1;
    if (g > a.batch) g = a.batch;
    a.G = (int)g;
    return report(launch_xcopy_stack(unit, a, XCOPY_STACK_TRANS, stream, &name), "xcopy_stack_trans");
  }
  const int e = launch_xcopy_stack(unit, a, inplace ? XCOPY_STACK_SWAP : XCOPY_STACK_TRANS, stream, &name);
  return report(e, name);
}

int dev_otrans(void* out, const void* in, unsigned ts, int m, int n, long long ldi, long long ldo, void* stream)
{
  const int unit = unit_of(ts, bits(out) | bits(in));
  if ((unsigned)unit == ts) {
    return report(launch_xcopy_trans(unit, in, out, m, n, ldi, ldo, mult16(in, ldi * ts), mult16(out, ldo * ts), stream), "xcopy_trans_tile");
  }
  StackMove a; memset(&a, 0, sizeof(a));
  a.P = (int)ts / unit; a.in = in; a.out = out; a.ldi = ldi * a.P; a.ldo = ldo * a.P; a.m = m; a.n = n; a.batch = 1;
  return dev_stack_trans(a, unit, false, stream);
}

int dev_itrans(void* inout, unsigned ts, int n, long long ld, void* stream)
{
  const int unit = unit_of(ts, bits(inout));
  if ((unsigned)unit == ts) return report(launch_xcopy_itrans(unit, inout, n, ld, mult16(inout, ld * ts), stream), "xcopy_itrans_tile");
  StackMove a; memset(&a, 0, sizeof(a));
  a.P = (int)ts / unit; a.in = inout; a.out = inout; a.ldi = a.ldo = ld * a.P; a.m = a.n = n; a.batch = 1;
  return dev_stack_trans(a, unit, true, stream);
}

// ---- one matrix, any memory ----------------------------------------------------------------------------------------------
// op: OP_COPY (in == nullptr: zeros), OP_TRANS, OP_ITRANS (in is ignored, ldi == ldo). The arguments are valid and not empty.
int run2d(int op, void* out, const void* in, unsigned ts, int m, int n, long long ldi, long long ldo, const char* what)
{
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  const hipStream_t st = (hipStream_t)stream;
  const int rows_out = (OP_TRANS == op ? n : m), cols_out = (OP_TRANS == op ? m : n); // as the destination is stored
  const int kind_out = pointer_kind(out), kind_in = (nullptr != in && OP_ITRANS != op) ? pointer_kind(in) : 1;
  const bool stage_out = (0 == (kind_out & 1)), stage_in = (0 == (kind_in & 1));
  const bool visible = (0 != (kind_out & 2)) || (0 != (kind_in & 2));
  const size_t tight = (size_t)rows_out * ts; // bytes of a column of the destination
  void* dout = out; const void* din = (OP_ITRANS == op ? nullptr : in);
  long long dldo = ldo;
  if (stage_in) { // the span of the input as it lies
    const size_t nbytes = ((size_t)(n - 1) * ldi + m) * ts;
    void* const p = scratch(0, nbytes);
    if (nullptr == p || 0 != h2d(p, in, nbytes)) return EXIT_FAILURE;
    din = p;
  }
  if (stage_out) { // a tight image of the destination; only the valid part travels (back), the padding keeps its bytes
    dout = scratch(1, tight * cols_out);
    if (nullptr == dout) return EXIT_FAILURE;
    dldo = rows_out;
    if (OP_ITRANS == op && hipSuccess != hipMemcpy2DAsync(dout, tight, out, (size_t)ldo * ts, tight, cols_out, hipMemcpyHostToDevice, st)) {
      (void)hipGetLastError(); return EXIT_FAILURE;
    }
  }
  int rc;
  if (OP_COPY == op) rc = dev_copy(dout, din, (long long)m * ts, n, ldi * ts, dldo * ts, stream);
  else if (OP_TRANS == op) rc = dev_otrans(dout, din, ts, m, n, ldi, dldo, stream);
  else rc = dev_itrans(dout, ts, n, dldo, stream);
  if (EXIT_SUCCESS != rc) return rc;
  if (stage_out) {
    if (hipSuccess != hipMemcpy2DAsync(out, (size_t)ldo * ts, dout, tight, tight, cols_out, hipMemcpyDeviceToHost, st)) { (void)hipGetLastError(); return EXIT_FAILURE; }
    return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  if (stage_in || visible) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

// ---- the reference's entry points ------------------------------------------------------------------------------------
void itrans_checked(void* inout, unsigned ts, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint ld, int* flag)
{ // src/libxsmm_xcopy.c:381-423 (plus: an extent beyond ld would make columns overlap)
  if (nullptr == inout) { complain(flag, "the transpose input/output cannot be NULL!"); return; }
  if (m != n) { complain(flag, "in-place transpose is not fully implemented!"); return; }
  if (0 == ts || 255 < ts || m < 0 || m > ld) { complain(flag, "the type-size or the leading dimension of the in-place transpose is invalid!"); return; }
  if (2 > m) return; // nothing moves
  (void)run2d(OP_ITRANS, inout, nullptr, ts, m, n, ld, ld, "libxsmm_itrans");
}

void matcopy_checked(void* out, const void* in, unsigned ts, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo,
  int tid, int nthreads, int* flag)
{ // src/libxsmm_xcopy.c:169-233
  if (0 < ts && ts <= 255 && m <= ldi && m <= ldo && out != in && ((nullptr != out && 0 < m && 0 < n) || (0 == m && 0 == n)) && 0 <= tid && tid < nthreads) {
    if (0 < m && 0 < n) { // task tid: its range of the columns
      const long long n0 = (long long)n * tid / nthreads, n1 = (long long)n * (tid + 1) / nthreads;
      if (n0 < n1) {
        (void)run2d(OP_COPY, static_cast<char*>(out) + (size_t)n0 * ldo * ts, nullptr != in ? static_cast<const char*>(in) + (size_t)n0 * ldi * ts : nullptr,
          ts, m, (int)(n1 - n0), ldi, ldo, "libxsmm_matcopy");
      }
    }
  }
  else if (0 > tid || tid >= nthreads) complain(flag, "the matrix-copy thread-id or number of threads is incorrect!");
  else if (nullptr == out) complain(flag, "the matrix-copy input and/or output is NULL!");
  else if (out == in) complain(flag, "output and input of the matrix-copy must be different!");
  else if (0 == ts || 255 < ts) complain(flag, "the type-size of the matrix-copy is zero or too large!");
  else if (0 >= m || 0 >= n) complain(flag, "the matrix extent(s) of the matrix-copy is/are zero or negative!");
  else complain(flag, "the leading dimension(s) of the matrix-copy is/are too small!");
}

void otrans_checked(void* out, const void* in, unsigned ts, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo,
  int tid, int nthreads, int* flag)
{ // src/libxsmm_xcopy.c:289-371
  if (0 < ts && ts <= 255 && m <= ldi && n <= ldo && ((nullptr != out && nullptr != in && 0 < m && 0 < n) || (0 == m && 0 == n)) && 0 <= tid && tid < nthreads) {
    if (0 < m && 0 < n) {
      if (out != in) { // task tid: its range of the rows of the input, which are the columns of the output
        const long long m0 = (long long)m * tid / nthreads, m1 = (long long)m * (tid + 1) / nthreads;
        if (m0 < m1) {
          (void)run2d(OP_TRANS, static_cast<char*>(out) + (size_t)m0 * ldo * ts, static_cast<const char*>(in) + (size_t)m0 * ts,
            ts, (int)(m1 - m0), n, ldi, ldo, "libxsmm_otrans");
        }
      }
      else if (ldi == ldo) { if (0 == tid) itrans_checked(out, ts, m, n, ldi, flag); } // (in place there are no independent shares: the first task does it)
      else complain(flag, "output and input of the transpose must be different!");
    }
  }
  else if (0 > tid || tid >= nthreads) complain(flag, "the transpose thread-id or number of threads is incorrect!");
  else if (nullptr == out || nullptr == in) complain(flag, "the transpose input and/or output is NULL!");
  else if (out == in) complain(flag, "output and input of the transpose must be different!");
  else if (0 == ts || 255 < ts) complain(flag, "the type-size of the transpose is zero or too large!");
  else if (0 >= m || 0 >= n) complain(flag, "the matrix extent(s) of the transpose is/are zero or negative!");
  else complain(flag, "the leading dimension(s) of the transpose is/are too small!");
}

Kernel* make_xcopy(int kind, unsigned ts, unsigned m, unsigned n, unsigned ldi, unsigned ldo, unsigned flags, unsigned prefetch)
{
  Kernel* const k = new Kernel();
  memset(&k->desc, 0, sizeof(k->desc));
  k->kclass = KC_XCOPY; k->registered = true; k->thunk = nullptr;
  k->xkind = kind; k->xtypesize = ts; k->xm = m; k->xn = n; k->xldi = ldi; k->xldo = ldo; k->xflags = flags; k->xprefetch = prefetch;
  return k;
}

Kernel* make_mcopy(const void* desc)
{
  const auto* const d = static_cast<const libxsmm_mcopy_descriptor*>(desc);
  const bool zero = (0 != (d->flags & LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE));
  if (0 == d->typesize || 0 == d->m || 0 == d->n || d->m > 0x7fffffffu || d->n > 0x7fffffffu || d->ldo < d->m || d->ldo > 0x7fffffffu
    || (!zero && (d->ldi < d->m || d->ldi > 0x7fffffffu))) return nullptr;
  return make_xcopy(LIBXSMM_KERNEL_KIND_MCOPY, d->typesize, d->m, d->n, d->ldi, d->ldo, d->flags, d->prefetch);
}

Kernel* make_trans(const void* desc)
{
  const auto* const d = static_cast<const libxsmm_trans_descriptor*>(desc);
  if (0 == d->typesize || 0 == d->m || 0 == d->n || d->m > 0x7fffffffu || d->n > 0x7fffffffu || d->ldo < d->n || d->ldo > 0x7fffffffu) return nullptr;
  return make_xcopy(LIBXSMM_KERNEL_KIND_TRANS, d->typesize, d->m, d->n, 0, d->ldo, 0, 0);
}

// ---- stacks ----------------------------------------------------------------------------------------------------------
int batch_move(int op, void* out, const void* in, unsigned ts, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo,
  long long sin, long long sout, long long batch, int ptrs, const char* what)
{
  // (everything that can be wrong with the call is found before the device is asked for)
  if (0 == ts || 255 < ts || m < 0 || n < 0 || batch < 0) return EXIT_FAILURE;
  const int rows_out = (OP_TRANS == op ? n : m), cols_out = (OP_TRANS == op ? m : n);
  if (rows_out > ldo || ((nullptr != in || OP_TRANS == op) && m > ldi)) return EXIT_FAILURE;
  if (0 == batch || 0 == m || 0 == n) return EXIT_SUCCESS;
  if (nullptr == out || (OP_TRANS == op && nullptr == in)) return EXIT_FAILURE;
  const long long ext_out = (long long)(cols_out - 1) * ldo + rows_out, ext_in = (long long)(n - 1) * ldi + m;
  bool inplace = false;
  if (out == in) { // only the transposition of square items onto themselves
    if (OP_TRANS != op || m != n || ldi != ldo || (0 == ptrs && sin != sout)) return EXIT_FAILURE;
    inplace = true;
  }
  if (0 == ptrs && (sout < ext_out || (nullptr != in && sin < 0))) return EXIT_FAILURE; // items of out would overlap
  if (batch > (1LL << 40)) return EXIT_FAILURE;
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls)

  const void* din = in; void* dout = out;
  uintptr_t align = 0;
  bool sync = false, staged_out = false, uploaded = false;
  size_t out_bytes = 0;
  if (0 != ptrs) { // arrays of pointers: host arrays travel through the upload ring; the items must be memory the GPU reaches
    const size_t nbytes = (size_t)batch * sizeof(void*);
    const void* const arr[2] = { out, in };
    const void* dev[2] = { out, in };
    for (int i = 0; i < 2; ++i) {
      if (nullptr == arr[i] || (1 == i && inplace)) continue;
      if (0 != (pointer_kind(arr[i]) & 1)) continue; // (alignment of the items: the documented one)
      const void* const* const p = static_cast<const void* const*>(arr[i]);
      for (long long g = 0; g < batch; ++g) { if (nullptr == p[g]) return EXIT_FAILURE; align |= bits(p[g]); }
      if (0 == (pointer_kind(p[0]) & 1) || 0 == (pointer_kind(p[batch - 1]) & 1)) return EXIT_FAILURE;
      dev[i] = index_upload(arr[i], nbytes);
      if (nullptr == dev[i]) return EXIT_FAILURE;
      uploaded = true;
    }
    dout = const_cast<void*>(dev[0]); din = inplace ? dev[0] : dev[1];
  }
  else { // strided: pageable host memory through device copies of the spans as they lie (what is between the items travels along)
    align = bits(out) | bits(in);
    const int kind_out = pointer_kind(out), kind_in = (nullptr != in ? pointer_kind(in) : 1);
    sync = (0 != (kind_out & 2)) || (0 != (kind_in & 2));
    if (0 == (kind_out & 1)) {
      out_bytes = ((size_t)(batch - 1) * sout + ext_out) * ts;
      dout = scratch(1, out_bytes);
      if (nullptr == dout || 0 != h2d(dout, out, out_bytes)) return EXIT_FAILURE;
      staged_out = true;
      if (inplace) din = dout;
    }
    if (nullptr != in && !inplace && 0 == (kind_in & 1)) {
      const size_t nbytes = ((size_t)(batch - 1) * sin + ext_in) * ts;
      void* const p = scratch(0, nbytes);
      if (nullptr == p || 0 != h2d(p, in, nbytes)) return EXIT_FAILURE;
      din = p; sync = true;
    }
    align = (align & 15) | bits(dout) | bits(din);
  }

  int rc;
  if (OP_COPY == op && 0 == ptrs && ldo == m && (nullptr == in || ldi == m)) { // tight items: rows of m * n elements
    rc = dev_copy(dout, din, (long long)m * n * ts, batch, sin * ts, sout * ts, stream);
  }
  else {
    const int unit = unit_of(ts, align);
    StackMove a; memset(&a, 0, sizeof(a));
    a.P = (int)ts / unit; a.in = din; a.out = dout; a.sin = sin * a.P; a.sout = sout * a.P; a.ldi = (long long)ldi * a.P; a.ldo = (long long)ldo * a.P;
    a.m = m; a.n = n; a.batch = batch; a.ptrs = ptrs;
    if (OP_TRANS == op) rc = dev_stack_trans(a, unit, inplace, stream);
    else {
      const char* name = "";
      const int e = launch_xcopy_stack(unit, a, XCOPY_STACK_COPY, stream, &name);
      rc = report(e, nullptr != in ? name : "xcopy_generic_zero");
    }
  }
  if (uploaded) index_upload_commit();
  if (EXIT_SUCCESS != rc) return rc;
  if (staged_out) return 0 == d2h(out, dout, out_bytes) ? EXIT_SUCCESS : EXIT_FAILURE;
  if (sync) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

} // namespace

namespace xsmm {

void xcopy_call(Kernel* k, const void* in, const void* ldi, void* out, const void* ldo)
{
  (void)ldo; // (the descriptor's)
  if (nullptr == k || nullptr == out) return;
  if (LIBXSMM_KERNEL_KIND_TRANS == k->xkind) {
    const unsigned li = (nullptr != ldi ? *static_cast<const unsigned*>(ldi) : k->xm);
    if (nullptr == in || li < k->xm || li > 0x7fffffffu) return;
    if (out != in) (void)run2d(OP_TRANS, out, in, k->xtypesize, (int)k->xm, (int)k->xn, li, k->xldo, "a dispatched transpose kernel");
    else if (li == k->xldo && k->xm == k->xn && 1 < k->xm) (void)run2d(OP_ITRANS, out, nullptr, k->xtypesize, (int)k->xm, (int)k->xn, li, li, "a dispatched transpose kernel");
  }
  else {
    const bool zero = (0 != (k->xflags & LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE));
    if ((!zero && nullptr == in) || out == in) return;
    (void)run2d(OP_COPY, out, zero ? nullptr : in, k->xtypesize, (int)k->xm, (int)k->xn, k->xldi, k->xldo, "a dispatched matcopy kernel");
  }
}

} // namespace xsmm

LIBXSMM_API libxsmm_trans_descriptor* libxsmm_trans_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, unsigned int m,
  unsigned int n, unsigned int ldo)
{ // src/libxsmm_generator.c:339-353
  if (nullptr == blob) return nullptr;
  memset(blob, 0, sizeof(*blob));
  libxsmm_trans_descriptor* const d = reinterpret_cast<libxsmm_trans_descriptor*>(blob->data);
  d->typesize = (unsigned char)typesize; d->ldo = ldo; d->m = m; d->n = n;
  return d;
}

LIBXSMM_API libxsmm_mcopy_descriptor* libxsmm_mcopy_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, unsigned int m,
  unsigned int n, unsigned int ldo, unsigned int ldi, int flags, int prefetch, const int* unroll)
{ // src/libxsmm_generator.c:356-381: only multiples of four bytes, normalised to typesize 4
  if (nullptr == blob || 0 != (typesize % 4)) return nullptr;
  const unsigned int typescale = typesize / 4;
  memset(blob, 0, sizeof(*blob));
  libxsmm_mcopy_descriptor* const d = reinterpret_cast<libxsmm_mcopy_descriptor*>(blob->data);
  d->unroll_level = (unsigned char)((nullptr == unroll || 0 >= *unroll) ? 2 : (*unroll < 64 ? *unroll : 64));
  d->typesize = 4; d->prefetch = (unsigned char)prefetch; d->flags = (unsigned char)flags;
  d->ldi = ldi * typescale; d->ldo = ldo * typescale; d->m = m * typescale; d->n = n;
  return d;
}

LIBXSMM_API libxsmm_xmcopyfunction libxsmm_dispatch_mcopy(const libxsmm_mcopy_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_xmcopyfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_MCOPY, make_mcopy));
}

LIBXSMM_API libxsmm_xtransfunction libxsmm_dispatch_trans(const libxsmm_trans_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_xtransfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_TRANS, make_trans));
}

LIBXSMM_API void libxsmm_matcopy(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, const int* prefetch)
{
  static int error_once = 0;
  (void)prefetch;
  matcopy_checked(out, in, typesize, m, n, ldi, ldo, 0, 1, &error_once);
}

LIBXSMM_API void libxsmm_matcopy_thread(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, const int* prefetch, int tid, int nthreads)
{
  static int error_once = 0;
  (void)prefetch;
  matcopy_checked(out, in, typesize, m, n, ldi, ldo, tid, nthreads, &error_once);
}

LIBXSMM_APIEXT void libxsmm_matcopy_omp(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, const int* prefetch)
{ // (the reference spreads tiles over OpenMP threads; one launch covers the matrix here)
  static int error_once = 0;
  (void)prefetch;
  matcopy_checked(out, in, typesize, m, n, ldi, ldo, 0, 1, &error_once);
}

LIBXSMM_API void libxsmm_otrans(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo)
{
  static int error_once = 0;
  otrans_checked(out, in, typesize, m, n, ldi, ldo, 0, 1, &error_once);
}

LIBXSMM_API void libxsmm_otrans_thread(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, int tid, int nthreads)
{
  static int error_once = 0;
  otrans_checked(out, in, typesize, m, n, ldi, ldo, tid, nthreads, &error_once);
}

LIBXSMM_APIEXT void libxsmm_otrans_omp(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo)
{
  static int error_once = 0;
  otrans_checked(out, in, typesize, m, n, ldi, ldo, 0, 1, &error_once);
}

LIBXSMM_API void libxsmm_itrans(void* inout, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint ld)
{
  static int error_once = 0;
  itrans_checked(inout, typesize, m, n, ld, &error_once);
}

LIBXSMM_API int libxsmm_amd_matcopy_batch(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, long long stride_in, long long stride_out, long long batch)
{
  return batch_move(OP_COPY, out, in, typesize, m, n, ldi, ldo, stride_in, stride_out, batch, 0, "libxsmm_amd_matcopy_batch");
}

LIBXSMM_API int libxsmm_amd_otrans_batch(void* out, const void* in, unsigned int typesize, libxsmm_blasint m, libxsmm_blasint n,
  libxsmm_blasint ldi, libxsmm_blasint ldo, long long stride_in, long long stride_out, long long batch)
{
  return batch_move(OP_TRANS, out, in, typesize, m, n, ldi, ldo, stride_in, stride_out, batch, 0, "libxsmm_amd_otrans_batch");
}

LIBXSMM_API int libxsmm_amd_matcopy_batch_ptr(void* const out[], const void* const in[], unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo, long long batch)
{
  return batch_move(OP_COPY, const_cast<void**>(out), in, typesize, m, n, ldi, ldo, 0, 0, batch, 1, "libxsmm_amd_matcopy_batch_ptr");
}

LIBXSMM_API int libxsmm_amd_otrans_batch_ptr(void* const out[], const void* const in[], unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint ldi, libxsmm_blasint ldo, long long batch)
{
  return batch_move(OP_TRANS, const_cast<void**>(out), in, typesize, m, n, ldi, ldo, 0, 0, batch, 1, "libxsmm_amd_otrans_batch_ptr");
}
