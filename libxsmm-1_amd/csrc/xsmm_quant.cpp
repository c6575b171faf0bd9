// xsmm_quant.cpp -- the producers of 16-bit GEMM inputs: libxsmm_dnn_quantize / _act / _fil, libxsmm_dnn_dequantize and the
// fp32 <-> bf16 converters (include/libxsmm_dnn.h), with the stream-ordered forms libxsmm_amd_dnn_quantize*_async.
//
// Reference: src/libxsmm_dnn.c:2394-2907 -- CPU loops (OpenMP) over the tensor: one pass for the largest magnitude, one
// that maps every element. Here both passes are kernels of kernels/quant.hip queued back to back: the second
// reads the maximum the first left in a device word, so no host round trip sits between them. This file checks the arguments
// (before any device probe: a wrong call is quiet and writes nothing on any machine) and applies the memory rules of the other
// entry points: memory the GPU reaches is processed in place, host-visible memory is complete on return, pageable memory is
// staged. The reference forms return the scaling factor through a host byte, which costs one wait per call; the _async forms
// leave it in a byte the GPU reaches and do not wait.
#include "xsmm_internal.hpp"
#include "../../include/libxsmm_amd.h"
#include "../../include/libxsmm_dnn.h"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstring>

using namespace xsmm;

namespace {

std::atomic<unsigned int> g_seed(0); // 0: a seed per call from libxsmm_timer_tick, as the reference does

void complain(int* flag, const char* what, const char* msg)
{ // library code is expected to be mute: one line per entry point, only if asked for
  if (0 != libxsmm_verbosity && once(flag)) fprintf(stderr, "LIBXSMM ERROR: %s: %s\n", what, msg);
}

// a * b * c * d elements; false beyond 2^62 (nothing of that size is addressable)
bool count_elements(unsigned int a, unsigned int b, unsigned int c, unsigned int d, unsigned long long* total)
{
  const unsigned long long ab = (unsigned long long)a * b, cd = (unsigned long long)c * d;
  if (0 != cd && ab > (1ULL << 62) / cd) return false;
  *total = ab * cd;
  return true;
}

bool tiled_enabled()
{ // LIBXSMM_AMD_QUANT_TILED=0 forces the generic form of libxsmm_dnn_quantize_act (read per call: a benchmark compares both)
  const char* const e = getenv("LIBXSMM_AMD_QUANT_TILED");
  return nullptr == e || 0 != atoi(e);
}

// ---- operands in any memory --------------------------------------------------------------------------------------------
struct Staged {
  const void* din; void* dout;  // what the kernels see
  void* out; size_t out_bytes;  // the caller's output, if it was staged
  bool wait;                    // an operand is host-visible or was staged: complete on return
};

bool stage(Staged* s, const void* in, size_t in_bytes, void* out, size_t out_bytes)
{
  const int kind_in = pointer_kind(in), kind_out = pointer_kind(out);
  s->din = in; s->dout = out; s->out = nullptr; s->out_bytes = out_bytes;
  s->wait = (0 != ((kind_in | kind_out) & 2));
  if (0 == (kind_in & 1)) {
    void* const p = scratch(0, in_bytes);
    if (nullptr == p || 0 != h2d(p, in, in_bytes)) return false;
    s->din = p; s->wait = true;
  }
  if (0 == (kind_out & 1)) { // (every element of the output is written: nothing travels to the device first)
    s->dout = scratch(1, out_bytes);
    if (nullptr == s->dout) return false;
    s->out = out; s->wait = true;
  }
  return true;
}

int finish(const Staged& s)
{
  if (nullptr != s.out) return 0 == d2h(s.out, s.dout, s.out_bytes) ? EXIT_SUCCESS : EXIT_FAILURE;
  if (s.wait) return 0 == stream_sync() ? EXIT_SUCCESS : EXIT_FAILURE;
  return EXIT_SUCCESS;
}

int report(int e, const char* name)
{
  if (0 == e) { note_launch(name); return EXIT_SUCCESS; } // (last_kernel names what was queued, never a launch that failed)
  fprintf(stderr, "LIBXSMM-AMD ERROR: kernel launch failed (%s, hip error %d)\n", name, e);
  return EXIT_FAILURE;
}

// ---- quantisation ----------------------------------------------------------------------------------------------------------
struct QuantCall {
  const float* in; short* out; unsigned char* scf;
  long long total;
  unsigned char add_shift; int mode; // QuantMode
  int layout;                        // 0: flat, 1: act, 2: fil
  QuantLayout g;
};

// The arguments are valid and the tensor is not empty. async: scf is a byte the GPU reaches and nothing waits for the stream
// (unless in / out are host memory); otherwise the byte travels through a device word and one read-back.
int quantize_run(const QuantCall& q, bool async, const char* what, int* flag)
{
  if (!device_ready()) { fail_no_device(what); return EXIT_FAILURE; }
  void* const stream = device().stream; // (seals an open burst of deferred calls: everything stays in call order)
  if (async && 0 == (pointer_kind(q.scf) & 1)) { complain(flag, what, "scf must be memory the GPU reaches!"); return EXIT_FAILURE; }
  int* const slot = flag_slot(); // [0]: the maximum; [1]: the scf byte of the reference forms
  if (nullptr == slot) return EXIT_FAILURE;
  Staged s;
  if (!stage(&s, q.in, (size_t)q.total * sizeof(float), q.out, (size_t)q.total * sizeof(short))) { flag_slot_commit(); return EXIT_FAILURE; }
  const float* const din = static_cast<const float*>(s.din);
  short* const dout = static_cast<short*>(s.dout);
  QuantHead h;
  h.mode = q.mode; h.add_shift = q.add_shift; h.seed = 0;
  h.maxword = reinterpret_cast<const unsigned*>(slot);
  h.scf = async ? q.scf : reinterpret_cast<unsigned char*>(slot + 1);
  if (QUANT_STOCH == q.mode) { // :2564-2566
    h.seed = g_seed.load(std::memory_order_relaxed);
    if (0 == h.seed) h.seed = (unsigned int)(libxsmm_timer_tick() % 0xffffffffu);
  }
  int rc = report(launch_quant_absmax(din, q.total, reinterpret_cast<unsigned*>(slot), stream), "quant_absmax");
  if (EXIT_SUCCESS == rc) {
    const unsigned CB = q.g.cb16 * q.g.lp;
    if (0 == q.layout || (1 == q.layout && q.g.cb32 == CB)) { // identical blockings: the same order on both sides
      rc = report(launch_quant_flat(din, dout, q.total, h, stream), "quant_flat");
    }
    else if (1 == q.layout && 1 == q.g.cb32 && 0 == CB % 2 && 0 == reinterpret_cast<uintptr_t>(dout) % 4 && tiled_enabled()) {
      rc = report(launch_quant_act_tiled(din, dout, q.total / ((long long)CB * q.g.H * q.g.W), (int)CB, (long long)q.g.H * q.g.W, h, stream), "quant_act_tiled");
    }
    else rc = report(launch_quant_layout(din, dout, q.g, h, stream), 1 == q.layout ? "quant_act" : "quant_fil");
  }
  flag_slot_commit();
  if (EXIT_SUCCESS != rc) return rc;
  if (!async) { // the host byte of the reference's signature: one wait per call
    if (nullptr != s.out && hipSuccess != hipMemcpyAsync(s.out, s.dout, s.out_bytes, hipMemcpyDefault, (hipStream_t)stream)) { (void)hipGetLastError(); return EXIT_FAILURE; }
    return 0 == d2h(q.scf, h.scf, 1) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  return finish(s);
}

bool mode_of(int round_mode, int* mode)
{
  if (round_mode < LIBXSMM_DNN_QUANT_NO_ROUND || round_mode > LIBXSMM_DNN_QUANT_FPHW_ROUND) return false;
  *mode = round_mode - LIBXSMM_DNN_QUANT_NO_ROUND;
  return true;
}

int quantize_flat(float* in, short* out, int length, unsigned char add_shift, unsigned char* scf, int round_mode, bool async, const char* what, int* flag)
{
  QuantCall q; memset(&q, 0, sizeof(q));
  if (nullptr == in || nullptr == out || nullptr == scf) { complain(flag, what, "in, out and scf cannot be NULL!"); return EXIT_FAILURE; }
  if (!mode_of(round_mode, &q.mode)) { complain(flag, what, "unknown round_mode!"); return EXIT_FAILURE; }
  if (length <= 0) return EXIT_SUCCESS; // (the reference would read in[0])
  q.in = in; q.out = out; q.scf = scf; q.total = length; q.add_shift = add_shift; q.layout = 0;
  return quantize_run(q, async, what, flag);
}

int quantize_act(float* in, short* out, unsigned int N, unsigned int C, unsigned int H, unsigned int W, unsigned int cblk_f32, unsigned int cblk_i16,
  unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode, bool async, const char* what, int* flag)
{
  QuantCall q; memset(&q, 0, sizeof(q));
  if (nullptr == in || nullptr == out || nullptr == scf) { complain(flag, what, "in, out and scf cannot be NULL!"); return EXIT_FAILURE; }
  if (!mode_of(round_mode, &q.mode)) { complain(flag, what, "unknown round_mode!"); return EXIT_FAILURE; }
  const unsigned long long CB = (unsigned long long)cblk_i16 * lp_blk;
  if (0 == cblk_f32 || 0 == CB || CB > 0x7fffffffu || 0 != C % cblk_f32 || 0 != C % CB) { // (:2587-2588 asserts)
    complain(flag, what, "C must be a multiple of cblk_f32 and of cblk_i16 * lp_blk!"); return EXIT_FAILURE;
  }
  unsigned long long total = 0;
  if (!count_elements(N, C, H, W, &total)) { complain(flag, what, "the tensor is too large!"); return EXIT_FAILURE; }
  if (0 == total) return EXIT_SUCCESS;
  q.in = in; q.out = out; q.scf = scf; q.total = (long long)total; q.add_shift = add_shift; q.layout = 1;
  q.g.C = C; q.g.H = H; q.g.W = W; q.g.cb32 = cblk_f32; q.g.cb16 = cblk_i16; q.g.lp = lp_blk; q.g.cblk = (unsigned)(C / CB);
  q.g.kb32 = q.g.kb16 = 1; q.g.fil = 0; q.g.total = q.total;
  return quantize_run(q, async, what, flag);
}

int quantize_fil(float* in, short* out, unsigned int K, unsigned int C, unsigned int R, unsigned int S, unsigned int cblk_f32, unsigned int cblk_i16,
  unsigned int kblk_f32, unsigned int kblk_i16, unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode, bool async,
  const char* what, int* flag)
{
  QuantCall q; memset(&q, 0, sizeof(q));
  if (nullptr == in || nullptr == out || nullptr == scf) { complain(flag, what, "in, out and scf cannot be NULL!"); return EXIT_FAILURE; }
  if (!mode_of(round_mode, &q.mode)) { complain(flag, what, "unknown round_mode!"); return EXIT_FAILURE; }
  const unsigned long long CB = (unsigned long long)cblk_i16 * lp_blk;
  if (0 == cblk_f32 || 0 == CB || CB > 0x7fffffffu || 0 == kblk_f32 || 0 == kblk_i16 || 0 != C % cblk_f32 || 0 != C % CB
    || 0 != K % kblk_f32 || 0 != K % kblk_i16 || 0 != lp_blk % 2) { // (:2690-2694 asserts)
    complain(flag, what, "C must be a multiple of cblk_f32 and of cblk_i16 * lp_blk, K of kblk_f32 and of kblk_i16, and lp_blk even!"); return EXIT_FAILURE;
  }
  unsigned long long total = 0;
  if (!count_elements(K, C, R, S, &total)) { complain(flag, what, "the tensor is too large!"); return EXIT_FAILURE; }
  if (0 == total) return EXIT_SUCCESS;
  q.in = in; q.out = out; q.scf = scf; q.total = (long long)total; q.add_shift = add_shift; q.layout = 2;
  q.g.C = C; q.g.H = R; q.g.W = S; q.g.cb32 = cblk_f32; q.g.cb16 = cblk_i16; q.g.lp = lp_blk; q.g.cblk = (unsigned)(C / CB);
  q.g.kb32 = kblk_f32; q.g.kb16 = kblk_i16; q.g.fil = 1; q.g.total = q.total;
  return quantize_run(q, async, what, flag);
}

// ---- element-wise maps -------------------------------------------------------------------------------------------------------
// op: 0 dequantise, 1 ... 3 fp32 -> bf16 (truncate, nearest-away, nearest-even), 4 bf16 -> fp32; the arguments are valid, n > 0
void map_run(int op, const void* in, void* out, long long n, float scale, const char* what)
{
  static const char* const names[] = { "dequant_flat", "bf16_truncate", "bf16_rnaz", "bf16_rne", "bf16_widen" };
  if (!device_ready()) { fail_no_device(what); return; }
  void* const stream = device().stream; // (seals an open burst of deferred calls)
  const bool widen = (0 == op || 4 == op); // 2 bytes in, 4 out
  Staged s;
  if (!stage(&s, in, (size_t)n * (widen ? 2 : 4), out, (size_t)n * (widen ? 4 : 2))) return;
  int e;
  if (0 == op) e = launch_dequant_flat(static_cast<const short*>(s.din), static_cast<float*>(s.dout), n, scale, stream);
  else if (4 == op) e = launch_bf16_widen(static_cast<const unsigned short*>(s.din), static_cast<float*>(s.dout), n, stream);
  else e = launch_bf16_narrow(op - 1, static_cast<const float*>(s.din), static_cast<unsigned short*>(s.dout), n, stream);
  if (EXIT_SUCCESS == report(e, names[op])) (void)finish(s);
}

} // namespace

// ---- include/libxsmm_math.h of the reference (src/libxsmm_math.c:462-520) -------------------------------------------------
LIBXSMM_API float libxsmm_sexp2_u8(unsigned char x)
{
  union { int i; float s; } result;
  if (128 > x) { // 2^32 multiplied up, then the rest: every factor and product is a power of two
    result.s = 1.f;
    for (int i = 0; i < (x >> 5); ++i) result.s *= 4294967296.f;
    result.s *= (float)(1U << (x & 31));
  }
  else result.i = 0x7F800000;
  return result.s;
}

LIBXSMM_API float libxsmm_sexp2_i8(signed char x)
{
  union { int i; float s; } result;
  if (-128 != x) {
    result.s = libxsmm_sexp2_u8((unsigned char)(0 > x ? -x : x));
    if (0 > x) result.s = 1.f / result.s; // (2^-127 is the denormal)
  }
  else result.i = 0x200000; // :510
  return result.s;
}

LIBXSMM_API float libxsmm_sexp2_i8i(int x) { return libxsmm_sexp2_i8((signed char)x); }

// ---- include/libxsmm_dnn.h --------------------------------------------------------------------------------------------------
LIBXSMM_API void libxsmm_dnn_quantize(float* in_buffer, short* out_buffer, int length, unsigned char add_shift, unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  (void)quantize_flat(in_buffer, out_buffer, length, add_shift, scf, round_mode, false, "libxsmm_dnn_quantize", &error_once);
}

LIBXSMM_API void libxsmm_dnn_quantize_act(float* in_buffer, short* out_buffer, unsigned int N, unsigned int C, unsigned int H, unsigned int W,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  (void)quantize_act(in_buffer, out_buffer, N, C, H, W, cblk_f32, cblk_i16, lp_blk, add_shift, scf, round_mode, false, "libxsmm_dnn_quantize_act", &error_once);
}

LIBXSMM_API void libxsmm_dnn_quantize_fil(float* in_buffer, short* out_buffer, unsigned int K, unsigned int C, unsigned int R, unsigned int S,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int kblk_f32, unsigned int kblk_i16, unsigned int lp_blk, unsigned char add_shift,
  unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  (void)quantize_fil(in_buffer, out_buffer, K, C, R, S, cblk_f32, cblk_i16, kblk_f32, kblk_i16, lp_blk, add_shift, scf, round_mode, false,
    "libxsmm_dnn_quantize_fil", &error_once);
}

LIBXSMM_API int libxsmm_amd_dnn_quantize_async(float* in_buffer, short* out_buffer, int length, unsigned char add_shift, unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  return quantize_flat(in_buffer, out_buffer, length, add_shift, scf, round_mode, true, "libxsmm_amd_dnn_quantize_async", &error_once);
}

LIBXSMM_API int libxsmm_amd_dnn_quantize_act_async(float* in_buffer, short* out_buffer, unsigned int N, unsigned int C, unsigned int H, unsigned int W,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int lp_blk, unsigned char add_shift, unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  return quantize_act(in_buffer, out_buffer, N, C, H, W, cblk_f32, cblk_i16, lp_blk, add_shift, scf, round_mode, true, "libxsmm_amd_dnn_quantize_act_async", &error_once);
}

LIBXSMM_API int libxsmm_amd_dnn_quantize_fil_async(float* in_buffer, short* out_buffer, unsigned int K, unsigned int C, unsigned int R, unsigned int S,
  unsigned int cblk_f32, unsigned int cblk_i16, unsigned int kblk_f32, unsigned int kblk_i16, unsigned int lp_blk, unsigned char add_shift,
  unsigned char* scf, int round_mode)
{
  static int error_once = 0;
  return quantize_fil(in_buffer, out_buffer, K, C, R, S, cblk_f32, cblk_i16, kblk_f32, kblk_i16, lp_blk, add_shift, scf, round_mode, true,
    "libxsmm_amd_dnn_quantize_fil_async", &error_once);
}

LIBXSMM_API void libxsmm_amd_dnn_quantize_set_seed(unsigned int seed) { g_seed.store(seed, std::memory_order_relaxed); }

LIBXSMM_API void libxsmm_dnn_dequantize(short* in_buffer, float* out_buffer, int length, unsigned char scf)
{ // :2813-2823
  static int error_once = 0;
  if (nullptr == in_buffer || nullptr == out_buffer) { complain(&error_once, "libxsmm_dnn_dequantize", "in and out cannot be NULL!"); return; }
  if (length <= 0) return;
  map_run(0, in_buffer, out_buffer, length, libxsmm_sexp2_i8((signed char)(-(int)scf)), "libxsmm_dnn_dequantize");
}

LIBXSMM_API void libxsmm_truncate_convert_f32_bf16(const float* in, libxsmm_bfloat16* out, unsigned int length)
{ // :2826-2836
  static int error_once = 0;
  if (nullptr == in || nullptr == out) { complain(&error_once, "libxsmm_truncate_convert_f32_bf16", "in and out cannot be NULL!"); return; }
  if (0 != length) map_run(1, in, out, length, 0.f, "libxsmm_truncate_convert_f32_bf16");
}

LIBXSMM_API void libxsmm_rnaz_convert_fp32_bfp16(const float* in, libxsmm_bfloat16* out, unsigned int len)
{ // :2839-2864
  static int error_once = 0;
  if (nullptr == in || nullptr == out) { complain(&error_once, "libxsmm_rnaz_convert_fp32_bfp16", "in and out cannot be NULL!"); return; }
  if (0 != len) map_run(2, in, out, len, 0.f, "libxsmm_rnaz_convert_fp32_bfp16");
}

LIBXSMM_API void libxsmm_rne_convert_fp32_bfp16(const float* in, libxsmm_bfloat16* out, unsigned int len)
{ // :2867-2893
  static int error_once = 0;
  if (nullptr == in || nullptr == out) { complain(&error_once, "libxsmm_rne_convert_fp32_bfp16", "in and out cannot be NULL!"); return; }
  if (0 != len) map_run(3, in, out, len, 0.f, "libxsmm_rne_convert_fp32_bfp16");
}

LIBXSMM_API void libxsmm_convert_bf16_f32(const libxsmm_bfloat16* in, float* out, unsigned int length)
{ // :2896-2907
  static int error_once = 0;
  if (nullptr == in || nullptr == out) { complain(&error_once, "libxsmm_convert_bf16_f32", "in and out cannot be NULL!"); return; }
  if (0 != length) map_run(4, in, out, length, 0.f, "libxsmm_convert_bf16_f32");
}
