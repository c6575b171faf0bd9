"""The pooling layer restated in numpy: handle rules, datalayouts, scratch formula, the statuses of execute_st, the split over
logical threads, seeded inputs, and the arithmetic contract of include/libxsmm_dnn_pooling.h (FWD and BWD, MAX and AVG, fp32
and bf16) as plain array code. Shared by tests/test_pool_cpu.py, tests/test_pool_gpu.py and tools/golden/pool_capture.py; the
reference's own answers are in tests/golden/pool.npz and tests/test_pool_cpu.py holds this file against them bit for bit."""
import functools
import os
import zlib

import numpy as np

from dnn_common import *  # noqa: F401,F403 (re-exported: the tests reach every shared name through this module)
from dnn_common import FmHandle, fma

MAX, AVG = 1, 2
MASK = 31
BINDABLE = (REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, MASK)
LAYOUT_TYPES = BINDABLE + (GEN_IN, GEN_OUT, REG_FIL)  # the layouts the capture asks for (the last one is no pooling tensor)
ERR_UNSUPPORTED_POOLING = 100033

FLT_MAX = np.float32(3.4028234663852886e38)
SENTINEL = -1  # what the mask is pre-filled with: FWD leaves it where no input exceeded -FLT_MAX

DESC_FIELDS = ("N", "C", "H", "W", "R", "S", "u", "v", "pad_h", "pad_w", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out", "threads",
               "datatype_in", "datatype_out", "datatype_mask", "buffer_format", "pooling_type")


def desc(H, W, R, S, u, v, pad_h=0, pad_w=0, pin=(0, 0), pout=(0, 0), N=2, C=32, pool=MAX, dt=F32, dt_out=None, dt_mask=I32, fmt=FMT_LIBXSMM, threads=1):
    return dict(N=N, C=C, H=H, W=W, R=R, S=S, u=u, v=v, pad_h=pad_h, pad_w=pad_w, pad_h_in=pin[0], pad_w_in=pin[1], pad_h_out=pout[0],
                pad_w_out=pout[1], threads=threads, datatype_in=dt, datatype_out=dt if dt_out is None else dt_out, datatype_mask=dt_mask,
                buffer_format=fmt, pooling_type=pool)


# the shapes of tests/test_pool_gpu.py: the smallest at which each mistake shows (N = 2, C = 32: two channel blocks, four items)
SHAPES = {
    "a": dict(H=7, W=7, R=3, S=3, u=2, v=2, pad_h=1, pad_w=1),                                  # overlap, logical padding on all four edges
    "b": dict(H=9, W=11, R=2, S=3, u=2, v=1, pad_h=0, pad_w=1, pin=(1, 2), pout=(2, 1)),        # H/W, R/S, u/v swapped; padded strides
    "c": dict(H=8, W=8, R=2, S=2, u=2, v=2),                                                    # no overlap
    "d": dict(H=8, W=8, R=3, S=3, u=2, v=2),                                                    # the floor leaves row / column 7 uncovered
    "e": dict(H=9, W=9, R=2, S=2, u=3, v=3),                                                    # stride above kernel: holes inside
    "f": dict(H=7, W=7, R=7, S=7, u=1, v=1),                                                    # global pooling
    "g": dict(H=6, W=6, R=3, S=3, u=1, v=1, pad_h=1, pad_w=1),                                  # nine covering outputs per input
    "h": dict(H=33, W=33, R=3, S=3, u=2, v=2, pad_h=1, pad_w=1),                                # 17 x 17 outputs: more than one tile
}


def compute_cases():
    """name -> desc; the name ends in the kind of input: n random normals, t a 7-value alphabet (ties in most windows)"""
    out = {}
    for s, shape in SHAPES.items():
        for pool, pname in ((MAX, "max"), (AVG, "avg")):
            for dt, dname in ((F32, "f32"), (BF16, "bf16")):
                for kind in ("n", "t"):
                    out["%s_%s_%s_%s" % (s, pname, dname, kind)] = desc(pool=pool, dt=dt, **shape)
    out["c24_max_f32_n"] = desc(C=24, **SHAPES["a"])   # the remainder of 8 channels is dropped silently: one block
    out["c24_avg_bf16_n"] = desc(C=24, pool=AVG, dt=BF16, **SHAPES["a"])
    return out


COMPUTE_CASES = compute_cases()
# windows that are all NaN / all -FLT_MAX (bf16: -Inf, as -FLT_MAX is no bf16 number): FWD only, the mask keeps its sentinel there
SPECIAL_CASES = {"nanwin_f32": desc(**SHAPES["c"]), "nanwin_bf16": desc(dt=BF16, **SHAPES["c"])}
# what the capture stores of the compute cases: all of them would exceed the size aimed at, and the alphabet kind (ties) says
# nothing about AVG, or about the 16-bit MAX, that the normals and the fp32 MAX do not
GOLDEN_CASES = [n for n in COMPUTE_CASES if n.endswith("_n") or "_max_f32_" in n]
STATUS_CASES = {
    "e_f32_bf16": desc(dt=F32, dt_out=BF16, **SHAPES["c"]), "e_bf16_f32": desc(dt=BF16, dt_out=F32, **SHAPES["c"]),
    "e_c8": desc(C=8, **SHAPES["c"]), "e_nhwc": desc(fmt=FMT_NHWC, **SHAPES["c"]), "e_nhwc_bf16": desc(fmt=FMT_NHWC, dt=BF16, dt_mask=I16, **SHAPES["c"]),
    "e_nchw": desc(fmt=FMT_NCHW, **SHAPES["c"]),
    "e_fmt3": desc(fmt=FMT_LIBXSMM | FMT_NHWC, pool=AVG, **SHAPES["c"]), "e_pool3": desc(pool=3, **SHAPES["c"]), "e_avg_nomask": desc(pool=AVG, **SHAPES["c"]),
    "e_unbound_regin": desc(pool=AVG, **SHAPES["c"]), "e_unbound_regout": desc(pool=AVG, **SHAPES["c"]), "e_unbound_gradin": desc(pool=AVG, **SHAPES["c"]),
    "e_unbound_gradout": desc(pool=AVG, **SHAPES["c"]), "e_unbound_mask": desc(**SHAPES["c"]), "e_mask_i16": desc(dt_mask=I16, **SHAPES["c"]),
}
UNBOUND = {"e_avg_nomask": (MASK,), "e_unbound_regin": (REG_IN,), "e_unbound_regout": (REG_OUT,), "e_unbound_gradin": (GRAD_IN,),
           "e_unbound_gradout": (GRAD_OUT,), "e_unbound_mask": (MASK,)}
# cases the reference must not execute: it writes C-wide pixels into an output layout of zero elements (C = 8) and 32-bit
# indices into a 16-bit mask
NO_RUN = ("e_c8", "e_mask_i16")


def all_cases():
    out = dict(COMPUTE_CASES)
    out.update(SPECIAL_CASES)
    out.update(STATUS_CASES)
    return out


def captured_cases():
    out = {n: COMPUTE_CASES[n] for n in GOLDEN_CASES}
    out.update(SPECIAL_CASES)
    out.update(STATUS_CASES)
    return out


def _cdiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- handle rules (src/libxsmm_dnn_pooling.c:44-95, src/libxsmm_dnn_setup.c:197-252) -------------------------------------------
class Handle(FmHandle):
    def __init__(self, d):
        super().__init__(d)
        if self.status != SUCCESS:
            return
        self.set_output(_cdiv(d["H"] + 2 * d["pad_h"] - d["R"], d["u"]) + 1, _cdiv(d["W"] + 2 * d["pad_w"] - d["S"], d["v"]) + 1)
        self.scratch_size = 4 * (d["H"] + 2 * max(d["pad_h_in"], d["pad_h_out"])) * (d["W"] + 2 * max(d["pad_w_in"], d["pad_w_out"])) \
            * max(self.ofmblock, self.ifmblock) * d["threads"]
        self.ok = True

    def layout(self, t):
        """(status, None) or (0, dict) as libxsmm_dnn_pooling_create_tensor_datalayout (:114-291)"""
        d = self.d
        inp, out, fmt = t in (REG_IN, GRAD_IN, GEN_IN), t in (REG_OUT, GRAD_OUT, GEN_OUT), d["buffer_format"]
        if inp or out:
            return self.activation_layout(inp)
        if t != MASK:
            return ERR_UNKNOWN_TENSOR_TYPE, None
        if fmt & FMT_LIBXSMM:  # always five dimensions over (ofw, ofh), without physical padding
            return made((DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), (self.ofmblock, self.ofw, self.ofh, self.blocksofm, d["N"]), d["datatype_mask"], fmt)
        if fmt & FMT_NHWC:     # (the reference sets the mask's datatype to datatype_in and then has no sizes for it)
            return ERR_UNKNOWN_TENSOR_TYPE, None
        return ERR_INVALID_FORMAT_GENERAL, None

    def execute_status(self, kind, bound, ltid=0):
        """what execute_st returns before anything is computed (bound: the tensor types that are bound). Up to
        ERR_UNSUPPORTED_POOLING the reference's order; the last four checks are this engine's own (the last of them: sizes below
        1, among them an output plane that the floor of a window larger than the padded plane leaves empty)."""
        d = self.d
        if kind not in (FWD, BWD):
            return ERR_INVALID_KIND
        if d["buffer_format"] != FMT_LIBXSMM:
            return ERR_INVALID_FORMAT_FUSEDBN
        need = (REG_IN, REG_OUT) if kind == FWD else (GRAD_IN, GRAD_OUT)
        if any(t not in bound for t in need) or (d["pooling_type"] == MAX and MASK not in bound):
            return ERR_DATA_NOT_BOUND
        if d["pooling_type"] not in (MAX, AVG):
            return ERR_UNSUPPORTED_POOLING
        if ltid < 0 or d["threads"] < 1:
            return ERR_GENERAL
        if d["pooling_type"] == MAX and d["datatype_mask"] != I32:
            return ERR_UNSUPPORTED_DATATYPE
        if not self.runnable():
            return ERR_GENERAL
        if min(d["N"], d["H"], d["W"], d["R"], d["S"], d["u"], d["v"], self.ofh, self.ofw) < 1 \
                or min(d["pad_h"], d["pad_w"], d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]) < 0 \
                or d["H"] * d["W"] >= 1 << 27 or self.ofh * self.ofw >= 1 << 27:
            return ERR_GENERAL
        return SUCCESS

    def mask_shape(self):
        return (self.work(), self.ofh, self.ofw, 16)


# ---- inputs: seeded, in the tensors' own layout (physical padding included: it is never read) -----------------------------------
def inputs(name, d):
    """(x, dout): the whole REGULAR_INPUT and GRADIENT_OUTPUT tensors, [item][row][column][16] in the element type"""
    h = Handle(d)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.endswith("_t"):
        x = rng.integers(-3, 4, size=h.in_shape()).astype(np.float32)
        dout = rng.integers(-3, 4, size=h.out_shape()).astype(np.float32)
    else:
        x = rng.standard_normal(h.in_shape()).astype(np.float32)
        dout = rng.standard_normal(h.out_shape()).astype(np.float32)
    if name.startswith("nanwin"):
        lowest = -FLT_MAX if h.f32 else np.float32(-np.inf)
        x[0, 0:2, 0:2, :] = np.nan          # item 0, output (0, 0): a NaN never wins
        x[1, 2:4, 4:6, :] = lowest          # item 1, output (1, 2): nothing exceeds -FLT_MAX
        x[3, 6:8, 0:2, 3] = np.nan          # item 3, output (3, 0): one channel lane only
    if not h.f32:
        x, dout = truncate(x), truncate(dout)
    return x, dout


# ---- the arithmetic contract ---------------------------------------------------------------------------------------------------------
WRONG = ("ge", "clipped count", "pads swapped", "strides swapped", "mask on padded plane")  # what forward(wrong=...) can get wrong on purpose


def _windows(h, wrong=None):
    """per (kh, kw): the outputs whose window position lies inside the plane, and the input coordinates it reads"""
    d = h.d
    u, v, pad_h, pad_w = d["u"], d["v"], d["pad_h"], d["pad_w"]
    if wrong == "pads swapped":
        pad_h, pad_w = pad_w, pad_h
    if wrong == "strides swapped":
        u, v = v, u
    for kh in range(d["R"]):
        hi = np.arange(h.ofh) * u - pad_h + kh
        hv = np.nonzero((hi >= 0) & (hi < d["H"]))[0]
        for kw in range(d["S"]):
            wi = np.arange(h.ofw) * v - pad_w + kw
            wv = np.nonzero((wi >= 0) & (wi < d["W"]))[0]
            if hv.size and wv.size:
                yield hv, wv, hi[hv], wi[wv]


def forward(h, x, out, mask=None, wrong=None):
    """FWD into the pre-filled destinations out (element type) and mask (int32, MAX only), in place: the interior of out and
    the mask elements whose output found an input above -FLT_MAX are written, nothing else. wrong: one of WRONG, a mistake made
    on purpose (for tests/test_pool_sweep_cpu.py, which shows that its float64 comparison rejects each of them)."""
    d = h.d
    iph, ipw, oph, opw = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]
    xin = as_f32(h, x)[:, iph:iph + d["H"], ipw:ipw + d["W"], :]
    lanes = np.arange(16, dtype=np.int32)
    work = h.work()
    if d["pooling_type"] == MAX:
        cur = np.full((work, h.ofh, h.ofw, 16), -FLT_MAX, dtype=np.float32)
        idx = np.full((work, h.ofh, h.ofw, 16), SENTINEL, dtype=np.int32)
        for hv, wv, hi, wi in _windows(h, wrong):  # kh ascending, then kw ascending; a strict > replaces: the first maximum wins, a NaN never
            v = xin[:, hi[:, None], wi[None, :], :]
            here = ((hi[:, None] * d["W"] + wi[None, :]) * 16).astype(np.int32)[None, :, :, None] + lanes
            if wrong == "mask on padded plane":
                here = (((hi[:, None] + iph) * h.ifwp + wi[None, :] + ipw) * 16).astype(np.int32)[None, :, :, None] + lanes
            c, i = cur[:, hv[:, None], wv[None, :], :], idx[:, hv[:, None], wv[None, :], :]
            won = v >= c if wrong == "ge" else v > c
            cur[:, hv[:, None], wv[None, :], :] = np.where(won, v, c)
            idx[:, hv[:, None], wv[None, :], :] = np.where(won, here, i)
        np.copyto(mask, idx, where=idx != SENTINEL)
        res = cur
    else:
        acc = np.zeros((work, h.ofh, h.ofw, 16), dtype=np.float32)
        count = np.zeros((1, h.ofh, h.ofw, 1), dtype=np.float32)
        for hv, wv, hi, wi in _windows(h, wrong):
            acc[:, hv[:, None], wv[None, :], :] = acc[:, hv[:, None], wv[None, :], :] + xin[:, hi[:, None], wi[None, :], :]
            count[:, hv[:, None], wv[None, :], :] += 1
        recp = np.float32(1.0) / (np.float32(d["R"]) * np.float32(d["S"]))
        res = acc * (np.float32(1.0) / np.maximum(count, 1) if wrong == "clipped count" else recp)
    out[:, oph:oph + h.ofh, opw:opw + h.ofw, :] = stored(h, res)


def backward(h, dout, mask, din, fused=False):
    """BWD into the interior of the pre-filled din (element type), in place. Per input element the contributions arrive with ho
    ascending, then wo ascending -- the order of the reference's scatter and of the engine's gather -- from +0.0.
    AVG: acc + dout * recp as a separate multiply and add (fused=True: the form the reference does not have; for the test that
    tells them apart). MAX trusts only masks FWD could have written: inside the output's window, in the element's own lane."""
    d = h.d
    iph, ipw, oph, opw = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]
    H, W, work = d["H"], d["W"], h.work()
    g = as_f32(h, dout)[:, oph:oph + h.ofh, opw:opw + h.ofw, :]
    acc = np.zeros((work, H, W, 16), dtype=np.float32)
    recp = np.float32(1.0) / (np.float32(d["R"]) * np.float32(d["S"]))
    lanes = np.arange(16, dtype=np.int64)
    flat = acc.reshape(work, H * W * 16)
    for ho in range(h.ofh):
        h0 = ho * d["u"] - d["pad_h"]
        for wo in range(h.ofw):
            w0 = wo * d["v"] - d["pad_w"]
            if d["pooling_type"] == MAX:
                m = mask[:, ho, wo, :].astype(np.int64)
                mh, mw = (m // 16) // W, (m // 16) % W
                ok = (m >= 0) & (m < H * W * 16) & (m % 16 == lanes) & (mh >= h0) & (mh < h0 + d["R"]) & (mw >= w0) & (mw < w0 + d["S"])
                ii, ll = np.nonzero(ok)
                flat[ii, m[ii, ll]] = flat[ii, m[ii, ll]] + g[ii, ho, wo, ll]  # (one element per lane: no index repeats)
            else:
                a0, a1, b0, b1 = max(h0, 0), min(h0 + d["R"], H), max(w0, 0), min(w0 + d["S"], W)
                if a0 < a1 and b0 < b1:
                    t = g[:, ho, wo, :][:, None, None, :]
                    part = acc[:, a0:a1, b0:b1, :]
                    acc[:, a0:a1, b0:b1, :] = fma(np.broadcast_to(t, part.shape), recp, part) if fused else part + t * recp
    din[:, iph:iph + H, ipw:ipw + W, :] = stored(h, acc)


def expected(name, d, fused=False):
    """dict of the tensors of a case after FWD and BWD on destinations pre-filled with ones bits (NaN / 0xffff) and a mask
    pre-filled with SENTINEL: x, dout, out, mask (MAX), din (None where BWD must not run on the reference: sentinels left)"""
    h = Handle(d)
    x, dout = inputs(name, d)
    fill = np.float32(np.nan) if h.f32 else np.uint16(0xffff)
    out = np.full(h.out_shape(), fill, dtype=elem_dtype(h))
    din = np.full(h.in_shape(), fill, dtype=elem_dtype(h))
    if h.f32:  # (the capture fills with 0xff bytes: that NaN's bits)
        out.view(np.uint32)[...] = 0xffffffff
        din.view(np.uint32)[...] = 0xffffffff
    mask = np.full(h.mask_shape(), SENTINEL, dtype=np.int32) if d["pooling_type"] == MAX else None
    forward(h, x, out, mask)
    backward(h, dout, mask, din, fused)
    return dict(x=x, dout=dout, out=out, mask=mask, din=din)


def load_golden():
    return np.load(os.path.join(GOLDEN, "pool.npz"))


# ---- the seeded sweep: descriptors nobody picked --------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 2, 48
SWEEP_CHANNELS = (16, 24, 32, 48, 64, 80)
U24, BF16_CUT = 2.0 ** -24, 2.0 ** -7  # the unit roundoff of fp32; what a truncation to bf16 takes off at most, relative


def gamma(n):
    """n roundings of relative size 2^-24 each, compounded: (1 + 2^-24)^n - 1 <= n * 2^-24 / (1 - n * 2^-24)"""
    n = np.asarray(n, dtype=np.float64)
    return n * U24 / (1 - n * U24)


def _draw(rng):
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    H, W = (pick(17, 40), pick(17, 40)) if pick(0, 7) == 0 else (pick(1, 12), pick(1, 12))
    R, S, u, v = pick(1, 4), pick(1, 4), pick(1, 4), pick(1, 4)
    pad_h, pad_w = pick(0, 3), pick(0, 3)
    pin, pout = (pick(0, 2), pick(0, 2)), (pick(0, 2), pick(0, 2))
    return desc(H, W, R, S, u, v, pad_h, pad_w, pin, pout, N=pick(1, 5), C=SWEEP_CHANNELS[pick(0, 5)], pool=(MAX, AVG)[pick(0, 1)],
                dt=(F32, BF16)[pick(0, 1)], threads=pick(1, 5))


def window_counts(h):
    """[ofh][ofw]: the number of input elements inside each output's window (R * S where nothing clips it, 0 where it lies wholly
    in the padding)"""
    d = h.d
    rows = [max(0, min(ho * d["u"] - d["pad_h"] + d["R"], d["H"]) - max(ho * d["u"] - d["pad_h"], 0)) for ho in range(h.ofh)]
    cols = [max(0, min(wo * d["v"] - d["pad_w"] + d["S"], d["W"]) - max(wo * d["v"] - d["pad_w"], 0)) for wo in range(h.ofw)]
    return np.outer(rows, cols)


def sweep_cases_from(seed):
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < SWEEP_CASES:
        d = _draw(rng)
        h = Handle(d)
        bound = BINDABLE if d["pooling_type"] == MAX else BINDABLE[:4]
        if h.status != SUCCESS or SUCCESS != h.execute_status(FWD, bound) or SUCCESS != h.execute_status(BWD, bound):
            continue
        if not window_counts(h).any():  # no window holds an input element: it would test nothing
            continue
        out["sweep_%02d" % len(out)] = d
    return out


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """name -> desc: SWEEP_CASES descriptors drawn from SWEEP_SEED. A draw that create or execute_status refuses (an output plane
    below 1 x 1) is left out, one in which no window holds an input element is drawn again. tests/test_pool_sweep_cpu.py counts
    what the set holds; the seed is the first from 0 up that passes that census."""
    return sweep_cases_from(SWEEP_SEED)


@functools.lru_cache(maxsize=None)
def sweep_expected(name):
    """expected() of a sweep case (computed once, shared: read only)"""
    t = expected(name, sweep_cases()[name])
    for a in t.values():
        if a is not None:
            a.setflags(write=False)
    return t


def contract64(h, t):
    """key -> (value, bound, compared) for out, mask (MAX) and din: the layer's contract (include/libxsmm_dnn_pooling.h, DESIGN.md
    8h) in float64, window by window, written from that text and not from forward / backward above. Interior elements only,
    [item][row][column][16]. compared is all True: pooling has no decision that rounding can flip (a tie falls alike on both sides).

    MAX FWD   the maximum of the window's elements inside the plane; the first one in row order, then column order, wins (numpy's
              argmax). bound 0: no rounding is involved, and a bf16 maximum is a bf16 number. A window without an element gives
              -FLT_MAX as the element type stores it (bf16: cut to 0xff7f) and leaves the mask's sentinel.
    AVG FWD   (sum of those elements) / (R * S), whatever the clipping. n elements cost n - 1 adds, the reciprocal is rounded
              once and multiplied once: gamma(n + 1) * sum|x| / (R * S).
    MAX BWD   an input element receives the dout of every output whose mask names it: t terms, t - 1 roundings (the first add
              to +0.0 is exact): gamma(t - 1) * sum|dout|.
    AVG BWD   it receives dout * (1 / (R * S)) from every output whose window covers it: the reciprocal, the product and t - 1
              adds: gamma(t + 1) * sum|dout| / (R * S).
    A bf16 store cuts off below 2^-7 * |what was computed| <= 2^-7 * (|value| + bound), added to the bound.
    An input element no term reaches is +0.0: value 0, bound 0."""
    d = h.d
    H, W, R, S, u, v = d["H"], d["W"], d["R"], d["S"], d["u"], d["v"]
    iph, ipw, oph, opw = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]
    is_max = d["pooling_type"] == MAX
    x = as_f32(h, t["x"]).astype(np.float64)[:, iph:iph + H, ipw:ipw + W, :]
    g = as_f32(h, t["dout"]).astype(np.float64)[:, oph:oph + h.ofh, opw:opw + h.ofw, :]
    work = h.work()
    items, lanes = np.arange(work)[:, None], np.arange(16)[None, :]
    out, out_bound = np.zeros((work, h.ofh, h.ofw, 16)), np.zeros((work, h.ofh, h.ofw, 16))
    mask = np.full((work, h.ofh, h.ofw, 16), SENTINEL, dtype=np.int64)
    din, din_abs, din_terms = np.zeros((work, H, W, 16)), np.zeros((work, H, W, 16)), np.zeros((work, H, W, 16), dtype=np.int64)
    lowest = float(-FLT_MAX) if h.f32 else float(widen(truncate(np.array([-FLT_MAX])))[0])
    for ho in range(h.ofh):
        a0, a1 = max(ho * u - d["pad_h"], 0), min(ho * u - d["pad_h"] + R, H)
        for wo in range(h.ofw):
            b0, b1 = max(wo * v - d["pad_w"], 0), min(wo * v - d["pad_w"] + S, W)
            if a0 >= a1 or b0 >= b1:
                out[:, ho, wo, :] = lowest if is_max else 0.0
                continue
            win = x[:, a0:a1, b0:b1, :].reshape(work, -1, 16)
            n = win.shape[1]
            if is_max:
                k = win.argmax(axis=1)
                out[:, ho, wo, :] = np.take_along_axis(win, k[:, None, :], axis=1)[:, 0, :]
                row, col = a0 + k // (b1 - b0), b0 + k % (b1 - b0)
                mask[:, ho, wo, :] = (row * W + col) * 16 + lanes
                np.add.at(din, (items, row, col, lanes), g[:, ho, wo, :])
                np.add.at(din_abs, (items, row, col, lanes), np.abs(g[:, ho, wo, :]))
                np.add.at(din_terms, (items, row, col, lanes), 1)
            else:
                out[:, ho, wo, :] = win.sum(axis=1) / (R * S)
                out_bound[:, ho, wo, :] = gamma(n + 1) * np.abs(win).sum(axis=1) / (R * S)
                din[:, a0:a1, b0:b1, :] += (g[:, ho, wo, :] / (R * S))[:, None, None, :]
                din_abs[:, a0:a1, b0:b1, :] += (np.abs(g[:, ho, wo, :]) / (R * S))[:, None, None, :]
                din_terms[:, a0:a1, b0:b1, :] += 1
    din_bound = np.where(din_terms > 0, gamma(np.maximum(din_terms + (-1 if is_max else 1), 0)) * din_abs, 0.0)
    if not h.f32:
        din_bound = din_bound + BF16_CUT * (np.abs(din) + din_bound)
        if not is_max:
            out_bound = out_bound + BF16_CUT * (np.abs(out) + out_bound)
    yes = np.ones(out.shape, dtype=bool)
    res = {"out": (out, out_bound, yes), "din": (din, din_bound, np.ones(din.shape, dtype=bool)), "unreached": din_terms == 0}
    if is_max:
        res["mask"] = (mask, np.zeros(mask.shape), yes)
    return res


def interior(h, key, a):
    """the elements of a tensor of expected() that contract64 computes, in its index order"""
    d = h.d
    if key == "out":
        return as_f32(h, a)[:, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :]
    if key == "din":
        return as_f32(h, a)[:, d["pad_h_in"]:d["pad_h_in"] + d["H"], d["pad_w_in"]:d["pad_w_in"] + d["W"], :]
    return a
