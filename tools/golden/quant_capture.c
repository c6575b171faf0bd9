/* quant_capture.c -- drives an unmodified build of the reference library through its public quantisation and bf16 conversion
 * functions and writes what they return as raw binary, for tools/golden/quant_capture.py to pack into tests/golden/quant_*.npz.
 * Build it against the reference (make BLAS=0 FORTRAN=0 STATIC=1 ECFLAGS=-fcommon), not against this library:
 *   gcc -O1 -I<reference>/include quant_capture.c <reference>/lib/libxsmm.a -lm -lpthread -ldl -lrt -o quant_capture
 * Usage: quant_capture flat  mode add_shift n in out                 out: n shorts, then the scf byte
 *        quant_capture act   mode add_shift N C H W cb32 cb16 lp in out
 *        quant_capture fil   mode add_shift K C R S cb32 cb16 kb32 kb16 lp in out
 *        quant_capture deq   scf n in out                            in: n shorts; out: n floats
 *        quant_capture bf16  which n in out                          which: 0 truncate, 1 rnaz, 2 rne (floats in), 3 widen (bf16 in)
 *        quant_capture sexp2 out                                     256 floats each of sexp2_u8, sexp2_i8, sexp2_i8i(-128 ... 127)
 *        quant_capture consts                                        NAME=value lines on stdout */
#include <libxsmm.h>
#include <libxsmm_dnn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void* slurp(const char* path, size_t bytes)
{
  void* p = malloc(bytes + 64);
  FILE* f = fopen(path, "rb");
  if (NULL == p || NULL == f || bytes != fread(p, 1, bytes, f)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
  return p;
}

static void dump(const char* path, const void* p, size_t bytes, const unsigned char* scf)
{
  FILE* f = fopen(path, "wb");
  if (NULL == f || bytes != fwrite(p, 1, bytes, f) || (NULL != scf && 1 != fwrite(scf, 1, 1, f))) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char* argv[])
{
  const char* const what = (1 < argc ? argv[1] : "");
  unsigned char scf = 0;
  libxsmm_init();
  if (0 == strcmp(what, "flat") && 7 == argc) {
    const int mode = atoi(argv[2]), shift = atoi(argv[3]), n = atoi(argv[4]);
    float* in = (float*)slurp(argv[5], sizeof(float) * n);
    short* out = (short*)calloc(n + 32, sizeof(short));
    libxsmm_dnn_quantize(in, out, n, (unsigned char)shift, &scf, mode);
    dump(argv[6], out, sizeof(short) * n, &scf);
  }
  else if (0 == strcmp(what, "act") && 13 == argc) {
    unsigned int d[7]; int i; size_t n;
    for (i = 0; i < 7; ++i) d[i] = (unsigned int)atoi(argv[4 + i]);
    n = (size_t)d[0] * d[1] * d[2] * d[3];
    { float* in = (float*)slurp(argv[11], sizeof(float) * n);
      short* out = (short*)calloc(n + 32, sizeof(short));
      libxsmm_dnn_quantize_act(in, out, d[0], d[1], d[2], d[3], d[4], d[5], d[6], (unsigned char)atoi(argv[3]), &scf, atoi(argv[2]));
      dump(argv[12], out, sizeof(short) * n, &scf); }
  }
  else if (0 == strcmp(what, "fil") && 15 == argc) {
    unsigned int d[9]; int i; size_t n;
    for (i = 0; i < 9; ++i) d[i] = (unsigned int)atoi(argv[4 + i]);
    n = (size_t)d[0] * d[1] * d[2] * d[3];
    { float* in = (float*)slurp(argv[13], sizeof(float) * n);
      short* out = (short*)calloc(n + 32, sizeof(short));
      libxsmm_dnn_quantize_fil(in, out, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], (unsigned char)atoi(argv[3]), &scf, atoi(argv[2]));
      dump(argv[14], out, sizeof(short) * n, &scf); }
  }
  else if (0 == strcmp(what, "deq") && 6 == argc) {
    const int n = atoi(argv[3]);
    short* in = (short*)slurp(argv[4], sizeof(short) * n);
    float* out = (float*)calloc(n + 16, sizeof(float));
    libxsmm_dnn_dequantize(in, out, n, (unsigned char)atoi(argv[2]));
    dump(argv[5], out, sizeof(float) * n, NULL);
  }
  else if (0 == strcmp(what, "bf16") && 6 == argc) {
    const int which = atoi(argv[2]); const unsigned int n = (unsigned int)atoi(argv[3]);
    if (3 == which) {
      libxsmm_bfloat16* in = (libxsmm_bfloat16*)slurp(argv[4], sizeof(libxsmm_bfloat16) * n);
      float* out = (float*)calloc(n + 16, sizeof(float));
      libxsmm_convert_bf16_f32(in, out, n);
      dump(argv[5], out, sizeof(float) * n, NULL);
    }
    else {
      float* in = (float*)slurp(argv[4], sizeof(float) * n);
      libxsmm_bfloat16* out = (libxsmm_bfloat16*)calloc(n + 32, sizeof(libxsmm_bfloat16));
      if (0 == which) libxsmm_truncate_convert_f32_bf16(in, out, n);
      else if (1 == which) libxsmm_rnaz_convert_fp32_bfp16(in, out, n);
      else libxsmm_rne_convert_fp32_bfp16(in, out, n);
      dump(argv[5], out, sizeof(libxsmm_bfloat16) * n, NULL);
    }
  }
  else if (0 == strcmp(what, "sexp2") && 3 == argc) {
    float out[3 * 256]; int i;
    for (i = 0; i < 256; ++i) {
      out[i] = libxsmm_sexp2_u8((unsigned char)i);
      out[256 + i] = libxsmm_sexp2_i8((signed char)(i - 128));
      out[512 + i] = libxsmm_sexp2_i8i(i - 128);
    }
    dump(argv[2], out, sizeof(out), NULL);
  }
  else if (0 == strcmp(what, "consts")) {
    union { float f; unsigned int u; } res;
    res.f = LIXSMMM_DNN_RES_DFP16;
#define SHOW(NAME) printf(#NAME "=%lu\n", (unsigned long)(NAME))
    SHOW(LIBXSNN_DNN_MASK_SIGN_F32); SHOW(LIBXSMM_DNN_MASK_EXP_F32); SHOW(LIBXSMM_DNN_MASK_MANT_F32); SHOW(LIBXSMM_DNN_MASK_ABS_F32);
    SHOW(LIBXSMM_DNN_MASK_FULL_F32); SHOW(LIBXSMM_DNN_MANT_SZ_F32); SHOW(LIBXSMM_DNN_SZ_F32); SHOW(LIBXSMM_DNN_MANT_DFP16);
    SHOW(LIBXSMM_DNN_QUANT_NO_ROUND); SHOW(LIBXSMM_DNN_QUANT_BIAS_ROUND); SHOW(LIBXSMM_DNN_QUANT_STOCH_ROUND);
    SHOW(LIBXSMM_DNN_QUANT_NEAREST_ROUND); SHOW(LIBXSMM_DNN_QUANT_FPHW_ROUND);
    printf("LIXSMMM_DNN_RES_DFP16_BITS=%lu\n", (unsigned long)res.u);
  }
  else { fprintf(stderr, "usage: see the head of quant_capture.c\n"); return 1; }
  libxsmm_finalize();
  return 0;
}
