/* libxsmm_math.h -- the reference splits its interface over several headers; nearly everything of its include/libxsmm_math.h
 * that this engine provides (matdiff, hash, memcmp, diff, diff_n, isqrt, icbrt, sexp2, shuffle) is declared in libxsmm.h, which includes this header as the
 * reference's does. Declared here are the exact powers of two that the quantisation scale factors of libxsmm_dnn.h are
 * defined through (reference: include/libxsmm_math.h:135-144, src/libxsmm_math.c:462-520). They are host functions. */
#ifndef LIBXSMM_MATH_H_COMPAT
#define LIBXSMM_MATH_H_COMPAT
#include "libxsmm.h"

LIBXSMM_API float libxsmm_sexp2_u8(unsigned char x);  /* :135 2^x exactly; +Inf from 128 on */
LIBXSMM_API float libxsmm_sexp2_i8(signed char x);    /* :141 2^x exactly (2^-127 is a denormal); -128 gives the bits 0x200000 */
LIBXSMM_API float libxsmm_sexp2_i8i(int x);           /* :144 libxsmm_sexp2_i8((signed char)x) */

#endif
