// xsmm_packed.cpp -- the packed ("compact") kernels: pgemm, getrf, trmm, trsm over packs of VLEN interleaved matrices.
//
// Reference: libxsmm_dispatch_{pgemm,getrf,trmm,trsm} (src/template/libxsmm.h:265-275), the descriptor initialisers
// (src/libxsmm_generator.c:383-505) and the packed descriptor structs (src/libxsmm_main.h:193-226); its kernels are AVX
// code in which a vector register holds one element of VLEN matrices. Here a lane owns a matrix: the kernel text is
// generated per descriptor (every dimension, flag and alpha a constant of the text, so the substitution / elimination
// loops unroll completely) and compiled with hiprtc like the other specialised kernels (xsmm_jit.cpp).
//
// Two forms of one text (packed kernels):
//   form 1  a work-group moves the operands of G packs between global memory and LDS in 16-byte pieces per lane (a
//           pack's lines are contiguous), then lane (g, v) works on matrix v of pack g out of LDS; the triangle / A /
//           the LU matrix is kept in registers where it fits (RESIDENT), otherwise read from LDS where it is used;
//   form 2  every lane works on its matrix where it lies in global memory (shapes whose packs do not fit the LDS
//           budget, operands that are not 16-byte aligned).
// Both forms run the same statements in the same order on every matrix: the results do not depend on the form, the
// batch size or the entry point. Arithmetic: fma chains; non-unit trsm and getrf multiply by the rounded reciprocal
// of the pivot.
#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"

#include <cstring>
#include <mutex>
#include <string>

using namespace xsmm;

// the reference's packed descriptor layouts (src/libxsmm_main.h:193-226)
#pragma pack(push, 1)
struct libxsmm_pgemm_descriptor { unsigned int m, n, k, lda, ldb, ldc; unsigned char typesize, layout; char transa, transb, alpha_val; };
struct libxsmm_getrf_descriptor { unsigned int m, n, lda; unsigned char typesize, layout; };
struct libxsmm_trmm_descriptor { union { double d; float s; } alpha; unsigned int m, n, lda, ldb; unsigned char typesize, layout; char diag, side, uplo, transa; };
struct libxsmm_trsm_descriptor { union { double d; float s; } alpha; unsigned int m, n, lda, ldb; unsigned char typesize, layout; char diag, side, uplo, transa; };
#pragma pack(pop)
static_assert(sizeof(libxsmm_pgemm_descriptor) == 29 && sizeof(libxsmm_getrf_descriptor) == 14, "packed descriptors");
static_assert(sizeof(libxsmm_trmm_descriptor) == 30 && sizeof(libxsmm_trsm_descriptor) == 30, "packed descriptors");

namespace xsmm { extern const char* const PACKED_BODY; } // kernels/packed_jit.inc as text (Makefile, TEXTS)

namespace {

constexpr int PK_MAXDIM = 32, PK_MAXLD = 4096;
constexpr int PK_LDS_BUDGET = 48 * 1024;  // bytes of LDS a work-group of form 1 may take (three of them fit a CU)
constexpr int PK_RESIDENT_DWORDS = 128;   // registers the resident operand may take

struct OpGeom {       // one operand as it is stored
  bool used = false;
  int rows = 0, cols = 0, ld = 0;
  int cd = 0, nl = 0; // contiguous extent of a line (elements of one matrix), number of lines
  size_t ps = 0;      // elements from one pack to the next
  size_t extent = 0;  // elements a pack spans
  int ls = 0;         // elements of a pack's image in LDS (padded: the images of neighbouring packs start 64 bytes apart modulo 256)
};

struct PSpec {
  int kind = 0;       // LIBXSMM_KERNEL_KIND_PGEMM ... TRSM
  int ts = 0, vlen = 0, rowmajor = 0;
  int m = 0, n = 0, k = 0;
  int transa = 0, transb = 0, side_r = 0, upper = 0, unit = 0;
  int alpha_kind = 0; // 0: 1, 1: -1, 2: alpha
  double alpha = 1.0;
  OpGeom op[3];       // A, B, C as the kernel is called
  int written = 0;    // the operand that is written
  int resident = 0, G = 0, threads = 0;
};

struct Packed {       // payload of a KC_PACKED kernel
  PSpec spec;
  std::mutex lock;
  JitKernel* jit[3][2] = { { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr } }; // by form and RESIDENT
  bool failed[3][2] = { { false, false }, { false, false }, { false, false } };
};

bool is_char(char c, char a, char b) { return a == c || b == c || (a | 0x20) == c || (b | 0x20) == c; }
bool upper_of(char c, char u) { return u == c || (u | 0x20) == c; }

void set_op(PSpec& s, int i, int rows, int cols, int ld)
{
  OpGeom& o = s.op[i];
  o.used = true; o.rows = rows; o.cols = cols; o.ld = ld;
  o.cd = (0 != s.rowmajor ? cols : rows); o.nl = (0 != s.rowmajor ? rows : cols);
  o.ps = (size_t)ld * o.nl * s.vlen;
  o.extent = ((size_t)(o.nl - 1) * ld + o.cd) * s.vlen;
  size_t bytes = (size_t)o.cd * o.nl * s.vlen * s.ts; // a multiple of 64
  while (64 != bytes % 256) bytes += 64;
  o.ls = (int)(bytes / s.ts);
}

bool dims_ok(int rows, int cols, int ld, int rowmajor)
{
  return 1 <= rows && rows <= PK_MAXDIM && 1 <= cols && cols <= PK_MAXDIM && (0 != rowmajor ? cols : rows) <= ld && ld <= PK_MAXLD;
}

void finish(PSpec& s)
{
  size_t resident_elems = 0, lds_bytes = 0;
  const int nt = (0 != s.side_r ? s.n : s.m);
  switch (s.kind) {
    case LIBXSMM_KERNEL_KIND_PGEMM: resident_elems = (size_t)s.m * s.k; s.written = 2; break;
    case LIBXSMM_KERNEL_KIND_GETRF: resident_elems = (size_t)s.m * s.n; s.written = 0; break;
    default: resident_elems = (size_t)nt * (nt + 1) / 2; s.written = 1; break;
  }
  s.resident = (resident_elems * (s.ts / 4) <= (size_t)PK_RESIDENT_DWORDS) ? 1 : 0;
  for (const OpGeom& o : s.op) if (o.used) lds_bytes += (size_t)o.ls * s.ts;
  const int gmax = 256 / s.vlen;
  s.G = (int)(PK_LDS_BUDGET / lds_bytes);
  if (s.G > gmax) s.G = gmax;
  s.threads = 256; // (the whole work-group moves the packs; lanes 0 ... G * VLEN - 1 then work on them)
}

// descriptor -> specification; false: outside the supported domain
bool spec_of(const void* desc, int kind, PSpec& s)
{
  if (nullptr == desc) return false;
  s = PSpec(); s.kind = kind;
  unsigned typesize = 0, layout = 0;
  switch (kind) {
    case LIBXSMM_KERNEL_KIND_PGEMM: { const auto* d = static_cast<const libxsmm_pgemm_descriptor*>(desc); typesize = d->typesize; layout = d->layout; } break;
    case LIBXSMM_KERNEL_KIND_GETRF: { const auto* d = static_cast<const libxsmm_getrf_descriptor*>(desc); typesize = d->typesize; layout = d->layout; } break;
    case LIBXSMM_KERNEL_KIND_TRMM: { const auto* d = static_cast<const libxsmm_trmm_descriptor*>(desc); typesize = d->typesize; layout = d->layout; } break;
    case LIBXSMM_KERNEL_KIND_TRSM: { const auto* d = static_cast<const libxsmm_trsm_descriptor*>(desc); typesize = d->typesize; layout = d->layout; } break;
    default: return false;
  }
  if ((4 != typesize && 8 != typesize) || (101 != layout && 102 != layout)) return false;
  s.ts = (int)typesize; s.vlen = libxsmm_amd_packed_width(typesize); s.rowmajor = (101 == layout) ? 1 : 0;
  auto dim = [](unsigned v) { return v > 1000000u ? -1 : (int)v; };
  if (LIBXSMM_KERNEL_KIND_PGEMM == kind) {
    const auto* d = static_cast<const libxsmm_pgemm_descriptor*>(desc);
    if (!is_char(d->transa, 'N', 'T') || !is_char(d->transb, 'N', 'T') || (0 != d->alpha_val && 1 != d->alpha_val)) return false;
    s.m = dim(d->m); s.n = dim(d->n); s.k = dim(d->k);
    s.transa = upper_of(d->transa, 'T'); s.transb = upper_of(d->transb, 'T'); s.alpha_kind = d->alpha_val;
    s.alpha = (0 == d->alpha_val ? 1.0 : -1.0);
    const int ar = s.transa ? s.k : s.m, ac = s.transa ? s.m : s.k, br = s.transb ? s.n : s.k, bc = s.transb ? s.k : s.n;
    if (!dims_ok(ar, ac, dim(d->lda), s.rowmajor) || !dims_ok(br, bc, dim(d->ldb), s.rowmajor) || !dims_ok(s.m, s.n, dim(d->ldc), s.rowmajor)) return false;
    set_op(s, 0, ar, ac, (int)d->lda); set_op(s, 1, br, bc, (int)d->ldb); set_op(s, 2, s.m, s.n, (int)d->ldc);
  }
  else if (LIBXSMM_KERNEL_KIND_GETRF == kind) {
    const auto* d = static_cast<const libxsmm_getrf_descriptor*>(desc);
    s.m = dim(d->m); s.n = dim(d->n);
    if (!dims_ok(s.m, s.n, dim(d->lda), s.rowmajor)) return false;
    set_op(s, 0, s.m, s.n, (int)d->lda);
  }
  else { // trmm and trsm share their layout
    const auto* d = static_cast<const libxsmm_trsm_descriptor*>(desc);
    if (!is_char(d->transa, 'N', 'T') || !is_char(d->side, 'L', 'R') || !is_char(d->uplo, 'L', 'U') || !is_char(d->diag, 'N', 'U')) return false;
    s.m = dim(d->m); s.n = dim(d->n);
    s.transa = upper_of(d->transa, 'T'); s.side_r = upper_of(d->side, 'R'); s.upper = upper_of(d->uplo, 'U'); s.unit = upper_of(d->diag, 'U');
    s.alpha = (8 == typesize ? d->alpha.d : (double)d->alpha.s);
    if (!(s.alpha == s.alpha) || s.alpha - s.alpha != 0.0) return false; // NaN, infinity
    s.alpha_kind = (1.0 == s.alpha ? 0 : (-1.0 == s.alpha ? 1 : 2));
    const int nt = (0 != s.side_r ? s.n : s.m);
    if (!dims_ok(s.m, s.n, dim(d->ldb), s.rowmajor) || !dims_ok(nt, nt, dim(d->lda), s.rowmajor)) return false;
    set_op(s, 0, nt, nt, (int)d->lda); set_op(s, 1, s.m, s.n, (int)d->ldb);
  }
  finish(s);
  return true;
}

// LIBXSMM_AMD_PACKED_FORM (read at every use: the tests switch it): 0 / unset: by shape
int form_env()
{
  const char* const e = getenv("LIBXSMM_AMD_PACKED_FORM");
  const int f = (nullptr == e || 0 == *e) ? 0 : atoi(e);
  return (1 == f || 2 == f) ? f : 0;
}

// LIBXSMM_AMD_PACKED_RESIDENT=0 (developer knob, read at every use): no operand in registers, also where it would fit -- the
// loops that large shapes run, on any shape (the tests compare the two bit for bit)
int resident_of(const PSpec& s)
{
  const char* const e = getenv("LIBXSMM_AMD_PACKED_RESIDENT");
  return (0 != s.resident && (nullptr == e || 0 == *e || 0 != atoi(e))) ? 1 : 0;
}

// The form a launch takes. Form 1 needs at least one pack's operands within the LDS budget and 16-byte aligned operands. By
// measurement (profiles/packed_bench.txt): with a lane per matrix the loads of form 2 are independent and all in
// flight at once, and it is the faster form wherever the operands are read once -- every register-resident shape of pgemm, trmm
// and trsm (65-75 % of the 8 TB/s peak against 52-65 %), and their larger shapes too. Form 1 wins where the lane works on its
// matrix in place over and over, getrf from 8 x 8 on (16 x 16: 2 x), since LDS then takes the traffic global memory would.
int form_of(const PSpec& s, bool aligned16)
{
  if (s.G < 1 || !aligned16) return 2;
  const int f = form_env();
  if (0 != f) return f;
  return (LIBXSMM_KERNEL_KIND_GETRF == s.kind && (size_t)s.m * s.n >= 64) ? 1 : 2;
}

// the #define block of a descriptor in front of the one text of all packed kernels (kernels/packed_jit.inc)
std::string gen_source(const PSpec& s, int form, int resident)
{
  char buf[2048];
  std::string src = "// packed kernel specialised per descriptor (xsmm_packed.cpp)\n";
  snprintf(buf, sizeof(buf),
    "typedef %s T;\n#define XFMA %s\n#define VLEN %d\n#define KIND %d\n#define FORM %d\n#define RESIDENT %d\n#define G %d\n#define THREADS %d\n"
    "#define ROWMAJOR %d\n#define M_ %d\n#define N_ %d\n#define K_ %d\n#define TRANSA %d\n#define TRANSB %d\n#define SIDE_R %d\n"
    "#define UPPER %d\n#define UNITDIAG %d\n#define ALPHA_KIND %d\n#define ALPHA_VAL ((T)%a)\n#define WRITTEN %d\n",
    8 == s.ts ? "double" : "float", 8 == s.ts ? "__builtin_fma" : "__builtin_fmaf", s.vlen, s.kind, form, resident, 1 == form ? s.G : 1, 1 == form ? s.threads : 256,
    s.rowmajor, s.m, s.n, s.k, s.transa, s.transb, s.side_r, s.upper, s.unit, s.alpha_kind, s.alpha, s.written);
  src += buf;
  static const char* const names[3] = { "A", "B", "C" };
  for (int i = 0; i < 3; ++i) {
    const OpGeom& o = s.op[i];
    // X_S: the distance of two lines where the lane works (LDS image: tight; global memory: the leading dimension)
    snprintf(buf, sizeof(buf), "#define %s_USED %d\n#define %s_CD %d\n#define %s_NL %d\n#define %s_LD %d\n#define %s_LS %d\n#define %s_S %d\n",
      names[i], o.used ? 1 : 0, names[i], o.used ? o.cd : 1, names[i], o.used ? o.nl : 1, names[i], o.used ? o.ld : 1,
      names[i], (o.used && 1 == form) ? o.ls : 0, names[i], o.used ? (1 == form ? o.cd : o.ld) : 1);
    src += buf;
  }
  src += PACKED_BODY;
  return src;
}

const char* launch_name(const PSpec& s, int form, bool burst)
{
  static const char* const names[4][2][2][2] = {
    { { { "packed_pgemm_f32_lds", "packed_pgemm_f32_lds_deferred" }, { "packed_pgemm_f32_direct", "packed_pgemm_f32_direct_deferred" } },
      { { "packed_pgemm_f64_lds", "packed_pgemm_f64_lds_deferred" }, { "packed_pgemm_f64_direct", "packed_pgemm_f64_direct_deferred" } } },
    { { { "packed_getrf_f32_lds", "packed_getrf_f32_lds_deferred" }, { "packed_getrf_f32_direct", "packed_getrf_f32_direct_deferred" } },
      { { "packed_getrf_f64_lds", "packed_getrf_f64_lds_deferred" }, { "packed_getrf_f64_direct", "packed_getrf_f64_direct_deferred" } } },
    { { { "packed_trmm_f32_lds", "packed_trmm_f32_lds_deferred" }, { "packed_trmm_f32_direct", "packed_trmm_f32_direct_deferred" } },
      { { "packed_trmm_f64_lds", "packed_trmm_f64_lds_deferred" }, { "packed_trmm_f64_direct", "packed_trmm_f64_direct_deferred" } } },
    { { { "packed_trsm_f32_lds", "packed_trsm_f32_lds_deferred" }, { "packed_trsm_f32_direct", "packed_trsm_f32_direct_deferred" } },
      { { "packed_trsm_f64_lds", "packed_trsm_f64_lds_deferred" }, { "packed_trsm_f64_direct", "packed_trsm_f64_direct_deferred" } } } };
  return names[s.kind - LIBXSMM_KERNEL_KIND_PGEMM][8 == s.ts ? 1 : 0][2 == form ? 1 : 0][burst ? 1 : 0];
}

JitKernel* kernel_of(Packed& p, int form)
{
  std::lock_guard<std::mutex> guard(p.lock);
  const int res = resident_of(p.spec);
  if (nullptr == p.jit[form][res] && !p.failed[form][res]) {
    std::string log;
    p.jit[form][res] = jit_compile(gen_source(p.spec, form, res), "xsmm_packed_op", &log);
    if (nullptr == p.jit[form][res]) {
      p.failed[form][res] = true;
      fprintf(stderr, "LIBXSMM-AMD ERROR: packed kernel did not compile (%s)\n", log.c_str());
    }
  }
  return p.jit[form][res];
}

// one launch over npacks packs (ring == nullptr: operands back to back from a, b, c)
int launch(Packed& p, int form, const void* a, const void* b, void* c, long long npacks, const unsigned long long* count, const void* ring,
           void* stream, const char** name)
{
  const PSpec& s = p.spec;
  *name = launch_name(s, form, nullptr != ring);
  JitKernel* const k = kernel_of(p, form);
  if (nullptr == k) return -1; // a missing kernel is an error, there is no other path
  // (the grid is never clamped: a launch beyond 2^31 - 1 blocks is refused below. The form-1 kernel has a grid-stride loop over groups of G
  // packs, but with one block per group it takes exactly one trip; form 2 has a lane per matrix and no loop)
  const long long blocks = (1 == form) ? (npacks + s.G - 1) / s.G : (npacks * s.vlen + 255) / 256;
  if (blocks < 1 || blocks > 0x7fffffffLL) return -1;
  void* args[] = { (void*)&a, (void*)&b, (void*)&c, (void*)&npacks, (void*)&count, (void*)&ring };
  return jit_launch_args(k, (unsigned)blocks, (unsigned)(1 == form ? s.threads : 256), args, stream);
}

bool aligned16(const PSpec& s, const void* a, const void* b, const void* c)
{
  const void* const p[3] = { a, b, c };
  uintptr_t bits = 0;
  for (int i = 0; i < 3; ++i) if (s.op[i].used) bits |= reinterpret_cast<uintptr_t>(p[i]);
  return 0 == (bits & 15);
}

int execute(Kernel* k, const void* a, const void* b, void* c, long long npacks, const char* what)
{
  Packed* const p = (nullptr != k && KC_PACKED == k->kclass) ? static_cast<Packed*>(k->packed) : nullptr;
  if (nullptr == p || npacks < 0) return EXIT_FAILURE;
  const PSpec& s = p->spec;
  const void* src[3] = { a, b, c };
  for (int i = 0; i < 3; ++i) if (s.op[i].used && nullptr == src[i]) return EXIT_FAILURE;
  if (0 == npacks) return EXIT_SUCCESS;
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* dev[3] = { nullptr, nullptr, nullptr };
  size_t bytes[3] = { 0, 0, 0 };
  bool staged[3] = { false, false, false }, visible = false;
  for (int i = 0; i < 3; ++i) {
    if (!s.op[i].used) continue;
    bytes[i] = ((size_t)(npacks - 1) * s.op[i].ps + s.op[i].extent) * s.ts;
    const int kind = pointer_kind(src[i]);
    if (0 != (kind & 1)) { dev[i] = const_cast<void*>(src[i]); visible = visible || 0 != (kind & 2); }
    else { // the CPU's memory: through a device copy
      dev[i] = scratch(3 + i, bytes[i]);
      if (nullptr == dev[i] || 0 != h2d(dev[i], src[i], bytes[i])) return EXIT_FAILURE;
      staged[i] = true;
    }
  }
  const char* name = "";
  const int e = launch(*p, form_of(s, aligned16(s, dev[0], dev[1], dev[2])), dev[0], dev[1], dev[2], npacks, nullptr, nullptr, device().stream, &name);
  note_launch(name);
  if (0 != e) { fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e); return EXIT_FAILURE; }
  if (staged[s.written]) return 0 == d2h(const_cast<void*>(src[s.written]), dev[s.written], bytes[s.written]) ? EXIT_SUCCESS : EXIT_FAILURE;
  if (staged[0] || staged[1] || staged[2] || visible) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

Kernel* make_kernel(const void* desc, int kind)
{
  PSpec s;
  if (!spec_of(desc, kind, s)) return nullptr;
  Packed* const p = new Packed();
  p->spec = s;
  Kernel* const k = new Kernel();
  memset(&k->desc, 0, sizeof(k->desc));
  k->kclass = KC_PACKED; k->registered = true; k->thunk = nullptr; k->packed = p;
  return k;
}
Kernel* make_pgemm(const void* d) { return make_kernel(d, LIBXSMM_KERNEL_KIND_PGEMM); }
Kernel* make_getrf(const void* d) { return make_kernel(d, LIBXSMM_KERNEL_KIND_GETRF); }
Kernel* make_trmm(const void* d) { return make_kernel(d, LIBXSMM_KERNEL_KIND_TRMM); }
Kernel* make_trsm(const void* d) { return make_kernel(d, LIBXSMM_KERNEL_KIND_TRSM); }

template<typename D> D* tr_init(libxsmm_descriptor_blob* blob, unsigned typesize, libxsmm_blasint m, libxsmm_blasint n, libxsmm_blasint lda,
  libxsmm_blasint ldb, const void* alpha, char transa, char diag, char side, char uplo, int layout)
{ // src/libxsmm_generator.c:383-446 (dimensions in full instead of modulo 256)
  if (nullptr == blob) return nullptr;
  memset(blob, 0, sizeof(*blob));
  D* const d = reinterpret_cast<D*>(blob->data);
  d->typesize = (unsigned char)typesize; d->layout = (unsigned char)layout;
  d->m = (unsigned)m; d->n = (unsigned)n; d->lda = (unsigned)lda; d->ldb = (unsigned)ldb;
  d->transa = transa; d->diag = diag; d->side = side; d->uplo = uplo;
  if (4 == typesize) d->alpha.s = (nullptr != alpha ? *static_cast<const float*>(alpha) : (float)LIBXSMM_ALPHA);
  else if (8 == typesize) d->alpha.d = (nullptr != alpha ? *static_cast<const double*>(alpha) : (double)LIBXSMM_ALPHA);
  return d;
}

} // namespace

namespace xsmm {

void packed_destroy(void* packed)
{
  Packed* const p = static_cast<Packed*>(packed);
  if (nullptr == p) return;
  for (auto& byform : p->jit) for (JitKernel* j : byform) if (nullptr != j) jit_release(j);
  delete p;
}

int packed_kind(const Kernel* k) { return (nullptr != k && nullptr != k->packed) ? static_cast<const Packed*>(k->packed)->spec.kind : LIBXSMM_KERNEL_KIND_INVALID; }

void packed_call(Kernel* k, const void* a, const void* b, void* c)
{
  if (defer_call(k, a, b, c)) return; // device operands inside the bracket: recorded, one launch for the burst (xsmm_defer.cpp)
  (void)execute(k, a, b, c, 1, "a dispatched packed kernel");
}

bool packed_operands(const Kernel* k, const void* a, const void* b, void* c, PackedOps* ops)
{
  const Packed* const p = (nullptr != k) ? static_cast<const Packed*>(k->packed) : nullptr;
  if (nullptr == p || nullptr == ops) return false;
  const PSpec& s = p->spec;
  const void* src[3] = { a, b, c };
  for (int i = 0; i < 3; ++i) if (s.op[i].used && nullptr == src[i]) return false;
  if (!aligned16(s, a, b, c)) return false; // (the burst's kernel is compiled once, for the form aligned operands take)
  ops->wr = const_cast<void*>(src[s.written]); ops->wr_bytes = s.op[s.written].extent * s.ts;
  int n = 0;
  for (int i = 0; i < 3; ++i) if (s.op[i].used && i != s.written) { ops->rd[n] = src[i]; ops->rd_bytes[n] = s.op[i].extent * s.ts; ++n; }
  for (; n < 2; ++n) { ops->rd[n] = ops->wr; ops->rd_bytes[n] = 0; }
  return true;
}

int packed_launch_burst(Kernel* k, const void* ring, const unsigned long long* count, int capacity, void* stream, const char** name)
{
  Packed* const p = (nullptr != k) ? static_cast<Packed*>(k->packed) : nullptr;
  if (nullptr == p) return -1;
  return launch(*p, form_of(p->spec, true), nullptr, nullptr, nullptr, capacity, count, ring, stream, name);
}

} // namespace xsmm

LIBXSMM_API int libxsmm_amd_packed_width(unsigned int typesize) { return 8 == typesize ? 8 : (4 == typesize ? 16 : 0); }

LIBXSMM_API libxsmm_trsm_descriptor* libxsmm_trsm_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint lda, libxsmm_blasint ldb, const void* alpha, char transa, char diag, char side, char uplo, int layout)
{
  return tr_init<libxsmm_trsm_descriptor>(blob, typesize, m, n, lda, ldb, alpha, transa, diag, side, uplo, layout);
}

LIBXSMM_API libxsmm_trmm_descriptor* libxsmm_trmm_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint lda, libxsmm_blasint ldb, const void* alpha, char transa, char diag, char side, char uplo, int layout)
{
  return tr_init<libxsmm_trmm_descriptor>(blob, typesize, m, n, lda, ldb, alpha, transa, diag, side, uplo, layout);
}

LIBXSMM_API libxsmm_pgemm_descriptor* libxsmm_pgemm_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint k, libxsmm_blasint lda, libxsmm_blasint ldb, libxsmm_blasint ldc, const void* alpha, char transa,
  char transb, int layout)
{ // src/libxsmm_generator.c:449-487; an alpha other than 1 or -1 ends the process there, here the result is NULL
  if (nullptr == blob) return nullptr;
  const double al = (nullptr == alpha ? 1.0 : (4 == typesize ? (double)*static_cast<const float*>(alpha) : *static_cast<const double*>(alpha)));
  if (1.0 != al && -1.0 != al) return nullptr;
  memset(blob, 0, sizeof(*blob));
  libxsmm_pgemm_descriptor* const d = reinterpret_cast<libxsmm_pgemm_descriptor*>(blob->data);
  d->typesize = (unsigned char)typesize; d->layout = (unsigned char)layout;
  d->m = (unsigned)m; d->n = (unsigned)n; d->k = (unsigned)k; d->lda = (unsigned)lda; d->ldb = (unsigned)ldb; d->ldc = (unsigned)ldc;
  d->transa = transa; d->transb = transb; d->alpha_val = (1.0 == al ? 0 : 1);
  return d;
}

LIBXSMM_API libxsmm_getrf_descriptor* libxsmm_getrf_descriptor_init(libxsmm_descriptor_blob* blob, unsigned int typesize, libxsmm_blasint m,
  libxsmm_blasint n, libxsmm_blasint lda, int layout)
{ // src/libxsmm_generator.c:490-505
  if (nullptr == blob) return nullptr;
  memset(blob, 0, sizeof(*blob));
  libxsmm_getrf_descriptor* const d = reinterpret_cast<libxsmm_getrf_descriptor*>(blob->data);
  d->typesize = (unsigned char)typesize; d->layout = (unsigned char)layout;
  d->m = (unsigned)m; d->n = (unsigned)n; d->lda = (unsigned)lda;
  return d;
}

// src/libxsmm_main.c (libxsmm_dispatch_pgemm ... libxsmm_dispatch_trsm): NULL for a NULL or unsupported descriptor
LIBXSMM_API libxsmm_pgemm_xfunction libxsmm_dispatch_pgemm(const libxsmm_pgemm_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_pgemm_xfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_PGEMM, make_pgemm));
}
LIBXSMM_API libxsmm_getrf_xfunction libxsmm_dispatch_getrf(const libxsmm_getrf_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_getrf_xfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_GETRF, make_getrf));
}
LIBXSMM_API libxsmm_trmm_xfunction libxsmm_dispatch_trmm(const libxsmm_trmm_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_trmm_xfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_TRMM, make_trmm));
}
LIBXSMM_API libxsmm_trsm_xfunction libxsmm_dispatch_trsm(const libxsmm_trsm_descriptor* descriptor)
{
  return reinterpret_cast<libxsmm_trsm_xfunction>(registry_dispatch(descriptor, sizeof(*descriptor), LIBXSMM_KERNEL_KIND_TRSM, make_trsm));
}

LIBXSMM_API int libxsmm_amd_packed_execute_batch(const void* kernel, const void* a, const void* b, void* c, long long npacks)
{
  Kernel* const k = kernel_from_pointer(kernel);
  if (nullptr == k || KC_PACKED != k->kclass) return EXIT_FAILURE;
  return execute(k, a, b, c, npacks, "libxsmm_amd_packed_execute_batch");
}

LIBXSMM_API int libxsmm_amd_packed_kernel_source(const void* descriptor, int kind, char* buffer, size_t buffer_size, int compile)
{
  PSpec s;
  if (!spec_of(descriptor, kind, s)) return -1;
  const std::string src = gen_source(s, form_of(s, true), resident_of(s));
  if (nullptr != buffer && 0 < buffer_size) {
    const size_t n = (src.size() < buffer_size - 1 ? src.size() : buffer_size - 1);
    memcpy(buffer, src.data(), n); buffer[n] = 0;
  }
  if (0 != compile) {
    std::string log;
    const int rc = jit_check_source(src, &log);
    if (0 != rc && 0 != libxsmm_verbosity) fprintf(stderr, "LIBXSMM-AMD: hiprtc: %s\n", log.c_str());
    return rc;
  }
  return (int)src.size();
}
