"""The arithmetic contract of include/libxsmm_dnn.h restated in numpy, with integer operations on the bits (view(np.uint32)):
the gold of tests/test_quant_gpu.py on a machine where the reference does not exist, itself checked bit for bit against the
reference's own outputs (tests/golden/quant_*.npz) by tests/test_quant_cpu.py.

Reference: src/libxsmm_dnn.c:2394-2907 (quantize / _act / _fil, dequantize, bf16 converters), src/libxsmm_math.c:462-520."""
import os

import numpy as np

NO_ROUND, BIAS_ROUND, STOCH_ROUND, NEAREST_ROUND, FPHW_ROUND = 80000, 80001, 80002, 80003, 80004
DETERMINISTIC = (NO_ROUND, BIAS_ROUND, NEAREST_ROUND, FPHW_ROUND)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CONSTANTS = {  # include/libxsmm_dnn.h:340-357 of the reference, misspellings included
    "LIBXSNN_DNN_MASK_SIGN_F32": 0x80000000, "LIBXSMM_DNN_MASK_EXP_F32": 0x7f800000, "LIBXSMM_DNN_MASK_MANT_F32": 0x007fffff,
    "LIBXSMM_DNN_MASK_ABS_F32": 0x7fffffff, "LIBXSMM_DNN_MASK_FULL_F32": 0xffffffff, "LIBXSMM_DNN_MANT_SZ_F32": 23,
    "LIBXSMM_DNN_SZ_F32": 32, "LIBXSMM_DNN_MANT_DFP16": 15,
    "LIBXSMM_DNN_QUANT_NO_ROUND": 80000, "LIBXSMM_DNN_QUANT_BIAS_ROUND": 80001, "LIBXSMM_DNN_QUANT_STOCH_ROUND": 80002,
    "LIBXSMM_DNN_QUANT_NEAREST_ROUND": 80003, "LIBXSMM_DNN_QUANT_FPHW_ROUND": 80004,
}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def sexp2_u8(x):
    """libxsmm_sexp2_u8: 2^x for x < 128, +Inf otherwise"""
    x = int(x) & 0xff
    return np.float32(np.inf) if x >= 128 else from_bits(np.uint32((x + 127) << 23))[0]


def sexp2_i8(x):
    """libxsmm_sexp2_i8 of a signed char: 2^x; 2^-127 is the denormal 0x400000, -128 gives the bits 0x200000"""
    x = ((int(x) + 128) & 0xff) - 128
    if x == -128:
        return from_bits(np.uint32(0x200000))[0]
    if x == -127:
        return from_bits(np.uint32(0x400000))[0]
    return from_bits(np.uint32((x + 127) << 23))[0]


def absmax_bits(x):
    """the largest (bits & 0x7fffffff): the bits of the largest fabsf for finite inputs, whatever the order"""
    return int((bits(x).ravel() & np.uint32(0x7fffffff)).max())


def frexp_exponent(b):
    """the exponent frexpf gives for the non-negative finite float with bits b"""
    e = b >> 23
    if e:
        return e - 126
    return 0 if b == 0 else (b.bit_length() - 1) - 148


def no_scf_parts(x, max_exp, add_shift, mode, p=None):
    """libxsmm_internal_quantize_scalar_no_scf over an array: (result as uint16, q of the stochastic formula as float32)"""
    ui = bits(x).ravel().astype(np.int64)
    exp_off = (max_exp - ((ui & 0x7fffffff) >> 23)) & 0xff
    mant = 0x800000 | (ui & 0x007fffff)
    rhs = np.minimum((24 - 15 + exp_off + (add_shift & 0xff)) & 0xff, 24)
    q = mant >> rhs
    neg = ((ui >> 31) != 0) & (q > 0)
    q = np.where(neg, (~q + 1) & 0xffffffff, q)
    stoch_q = None
    if mode == BIAS_ROUND:  # (a shift count below zero: the x86 shift takes the count modulo 32)
        inc = (mant & ((3 << ((rhs - 2) & 31)) & 0x7fffffff)) > 0
    elif mode == NEAREST_ROUND:
        inc = ((mant & ((1 << ((rhs - 1) & 31)) & 0x7fffffff)) > 0) & (rhs > 1)
    elif mode == STOCH_ROUND:
        fvalue = from_bits(((ui & ((0xffffffff << rhs) & 0xffffffff))).astype(np.uint32))
        xin = from_bits(ui.astype(np.uint32))
        with np.errstate(all="ignore"):
            stoch_q = ((xin - fvalue).astype(np.float32) / np.float32(2.0 ** -15)).astype(np.float32)
        inc = np.zeros(ui.shape, dtype=bool) if p is None else ((np.asarray(p, dtype=np.float32) + stoch_q).astype(np.float32) > np.float32(0.5))
    else:
        inc = np.zeros(ui.shape, dtype=bool)
    q = np.where(inc, q + 1, q)
    q = np.where((ui & 0x7fffffff) == 0, 0, q)  # LIBXSMM_FEQ(input, 0)
    return (q & 0xffff).astype(np.uint16), stoch_q


def quantize(x, add_shift, mode, p=None):
    """libxsmm_dnn_quantize on a flat array: (int16 array, scf byte). STOCH_ROUND: p holds the draws (None: never increments)."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    mb = absmax_bits(x)
    if mode == FPHW_ROUND:
        maxexp = frexp_exponent(mb) - (15 - add_shift)
        scfq = sexp2_i8(-maxexp)
        with np.errstate(all="ignore"):
            v = (x * scfq).astype(np.float32)
            t = np.trunc(v)
            t = np.where(np.abs(v - t) >= np.float32(0.5), t + np.copysign(np.float32(1), v), t).astype(np.float32)
            ok = np.abs(t) < np.float32(2147483648.0)  # cvttss2si: out of range (and NaN) gives 0x80000000
            q = np.where(ok, np.where(ok, t, 0).astype(np.int64), -0x80000000)
        return (q & 0xffff).astype(np.uint16).view(np.int16), (-maxexp) & 0xff
    max_exp = (mb >> 23) & 0xff
    q, _ = no_scf_parts(x, max_exp, add_shift, mode, p)
    return q.view(np.int16), (14 - add_shift - (max_exp - 127)) & 0xff


def act_source(N, C, H, W, cb32, cb16, lp):
    """flat source index of every element of the output of libxsmm_dnn_quantize_act, in output order (:2616-2628)"""
    cblk = C // (cb16 * lp)
    i1, i2, i3, i4, i5, i6 = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in (N, cblk, H, W, cb16, lp)), indexing="ij")
    c = i2 * cb16 * lp + i5 * lp + i6
    fi2, fi5 = c // cb32, c % cb32
    return (((((i1 * (C // cb32) + fi2) * H + i3) * W + i4) * cb32) + fi5).ravel()


def fil_source(K, C, R, S, cb32, cb16, kb32, kb16, lp):
    """the same for libxsmm_dnn_quantize_fil (:2741-2755)"""
    cblk, kblk = C // (cb16 * lp), K // kb16
    i1, i2, i3, i4, i5, i6, i7 = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in (kblk, cblk, R, S, cb16, kb16, lp)), indexing="ij")
    k = i1 * kb16 + i6
    fi1, fi6 = k // kb32, k % kb32
    c = i2 * cb16 * lp + i5 * lp + i7
    fi2, fi5 = c // cb32, c % cb32
    return ((((((fi1 * (C // cb32) + fi2) * R + i3) * S + i4) * cb32 + fi5) * kb32) + fi6).ravel()


def quantize_act(x, shape, add_shift, mode):
    q, scf = quantize(np.ascontiguousarray(x, dtype=np.float32).ravel()[act_source(*shape)], add_shift, mode)
    return q, scf


def quantize_fil(x, shape, add_shift, mode):
    q, scf = quantize(np.ascontiguousarray(x, dtype=np.float32).ravel()[fil_source(*shape)], add_shift, mode)
    return q, scf


def dequantize(q, scf):
    with np.errstate(all="ignore"):
        return (np.asarray(q, dtype=np.int16).astype(np.float32) * sexp2_i8(-int(scf))).astype(np.float32)


def bf16_truncate(x):
    return (bits(x) >> 16).astype(np.uint16)


def _unrounded(u):
    return (u & 0x7f800000) == 0x7f800000  # NaN and Inf are only shifted


def bf16_rnaz(x):
    u = bits(x).astype(np.int64)
    return ((np.where(_unrounded(u), u, u + 0x8000) >> 16) & 0xffff).astype(np.uint16)


def bf16_rne(x):
    u = bits(x).astype(np.int64)
    return ((np.where(_unrounded(u), u, u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_widen(h):
    return from_bits(np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16)


# ---- the cases tests/golden/quant_*.npz hold and tests/test_quant_gpu.py runs ---------------------------------------------
# (the last two act cases reach the rest of the tiled kernel: 72 channels per block are two chunks, 64 and 8 wide, and
# 6 channels per block are 3 pairs, no power of two -- the LDS pitch of 65 -- over two tiles of pixels)
ACT_CASES = [(2, 16, 3, 5, 1, 8, 2), (1, 32, 2, 70, 1, 8, 2), (2, 32, 3, 4, 16, 8, 2), (1, 32, 2, 3, 4, 16, 2), (3, 8, 1, 1, 1, 2, 2),
             (1, 144, 2, 5, 1, 36, 2), (1, 12, 2, 35, 1, 3, 2)]
FIL_CASES = [(16, 16, 3, 3, 1, 8, 1, 16, 2), (32, 16, 1, 1, 16, 8, 16, 16, 2), (4, 8, 2, 1, 2, 2, 4, 2, 2)]
FLAT_GOLDEN_LENGTHS = (1, 5, 1023)
DEQUANT_SCF = (0, 12, 14, 141)

BF16_SPECIALS = np.array([
    0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00018000, 0x00007fff, 0x00008001,  # zeros, denormals, ties
    0x3f800000, 0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0xbf808000, 0xbf818000, 0x3f80ffff, 0x7f7fffff, 0xff7fffff,
    0x7f7f8000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7f80ffff, 0x7f808000, 0x7fffffff,
], dtype=np.uint32)


def golden_input(seed, n, scale=1.0):
    """the inputs of the golden captures: seeded, so that a capture and its check agree on them without storing twice"""
    rng = np.random.default_rng(seed)
    x = ((rng.random(n) - 0.5) * 2.0 * scale).astype(np.float32)
    x[rng.random(n) < 0.05] = 0.0
    return x


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name))


GOLDEN_MODES = {"no": NO_ROUND, "bias": BIAS_ROUND, "nearest": NEAREST_ROUND, "fphw": FPHW_ROUND}


def golden_layout(g, name, shift, ci):
    """(reference output, scf byte) of case ci in quant_act.npz / quant_fil.npz. NO_ROUND is stored as it is; the other modes
    differ from it by at most one (the same scale, another rounding) and are stored as that difference, which packs small."""
    out = g["out_no_%d_%d" % (shift, ci)]
    if name != "no":
        out = (out.view(np.uint16) + g["delta_%s_%d_%d" % (name, shift, ci)].astype(np.int16).view(np.uint16)).view(np.int16)
    return out, int(g["scf_%s_%d_%d" % (name, shift, ci)])
