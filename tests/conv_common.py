"""The convolution layer restated in numpy: handle rules, datalayouts, scratch formulas, the statuses of the API, the split over
logical threads, seeded inputs, and the three generic templates of the reference (src/template/libxsmm_dnn_convolve_st_{fwd,bwd,
upd}_custom_custom_generic.tpl.c) loop for loop, every SMM call of theirs being one call of the CPU oracle's SMM (tests/
oracle_binding.py: one fmaf per term, k ascending -- or a separate multiply and add, which is how
test_fused_or_separate_is_decided_by_the_capture tells the two apart). Shared by tests/test_conv_cpu.py, tests/test_conv_gpu.py and
tools/golden/conv_capture.py; the reference's own answers are in tests/golden/conv.npz and tests/test_conv_cpu.py holds this file
against them bit for bit."""
import functools
import zlib

import numpy as np

import oracle_binding as orc
from dnn_common import *  # noqa: F401,F403 (re-exported: the tests reach every shared name through this module)
from dnn_common import share

REG_FIL_TR, GRAD_FIL, GEN_FIL, REG_BIAS, GRAD_BIAS, GEN_BIAS, POOL_MASK = 11, 12, 13, 14, 15, 16, 31
DIM_K, DIM_R, DIM_S = 4, 5, 6
BINDABLE = (REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, REG_FIL, GRAD_FIL, REG_FIL_TR, REG_BIAS, GRAD_BIAS)
LAYOUT_TYPES = BINDABLE + (GEN_IN, GEN_OUT, GEN_FIL, GEN_BIAS, POOL_MASK)  # the layouts the capture asks for (the last one is no conv tensor)
FMT_RSCK, FMT_KCRS = 8, 16
ALGO_AUTO, ALGO_DIRECT = 0, 1
OVERWRITE, NO_FILTER_TRANSPOSE = 1, 8
FUSE_BIAS, FUSE_RELU_FWD, FUSE_RELU_BWD, FUSE_RELU = 1, 2, 4, 6
WARN_FALLBACK = 90000
ERR_INVALID_TENSOR, ERR_INVALID_FORMAT_NCHW, ERR_INVALID_FORMAT_CONVOLVE, ERR_INVALID_FORMAT_KCRS = 100007, 100011, 100014, 100015
ERR_INVALID_ALGO, ERR_INVALID_PADDING, ERR_FUSION = 100022, 100023, 100031

DESC_FIELDS = ("N", "C", "H", "W", "K", "R", "S", "u", "v", "pad_h", "pad_w", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out", "threads",
               "datatype_in", "datatype_out", "buffer_format", "filter_format", "algo", "options", "fuse_ops")
OUTPUTS = ("out", "din", "dw", "wtr")


def desc(H, W, R, S, u=1, v=1, pad=(0, 0), pin=None, pout=(0, 0), N=2, C=16, K=16, threads=1, dt=F32, dt_out=None, fmt=FMT_LIBXSMM, ffmt=FMT_LIBXSMM,
         algo=ALGO_DIRECT, options=OVERWRITE, fuse=0):
    """pin None: physical padding (pad_*_in = pad_*)"""
    pin = pad if pin is None else pin
    return dict(N=N, C=C, H=H, W=W, K=K, R=R, S=S, u=u, v=v, pad_h=pad[0], pad_w=pad[1], pad_h_in=pin[0], pad_w_in=pin[1], pad_h_out=pout[0],
                pad_w_out=pout[1], threads=threads, datatype_in=dt, datatype_out=dt if dt_out is None else dt_out, buffer_format=fmt,
                filter_format=ffmt, algo=algo, options=options, fuse_ops=fuse)


LOGICAL = (0, 0)
BASE = dict(H=5, W=4, R=3, S=3, pad=(1, 1), pin=LOGICAL)  # the shape of the fuse / overwrite matrix and of the status cases


def compute_cases():
    """name -> desc: the smallest shapes at which each path of the kernels and each branch of the templates is taken"""
    out = {
        # kernel, stride and padding
        "k1x1": desc(5, 6, 1, 1, C=32, K=32),
        "k3x3_phys": desc(6, 5, 3, 3, pad=(1, 1), C=32, K=32),
        "k3x3_log": desc(6, 5, 3, 3, pad=(1, 1), pin=LOGICAL, C=32, K=32),
        "k3x3_s2_phys": desc(7, 8, 3, 3, 2, 2, pad=(1, 1)),                    # UPD: one chain per image, physical branch
        "k3x3_s2_log": desc(7, 8, 3, 3, 2, 2, pad=(1, 1), pin=LOGICAL),        # ... and the branch through the padded copy
        "k3x2_s12_log_acc": desc(6, 7, 3, 2, 1, 2, pad=(1, 0), pin=LOGICAL, options=0),  # u != v, R != S, padding in one direction only
        "k1x1_s2": desc(5, 7, 1, 1, 2, 2),                                      # BWD: pixels no term reaches; UPD: the ifhp/u loops
        "k1x1_s2_acc": desc(5, 7, 1, 1, 2, 2, options=0),                       # ... which keep their start value
        "k1x1_s2_pad": desc(6, 5, 1, 1, 2, 2, pad=(1, 1)),                      # 1x1 with a physical rim: UPD's GEMM form with a stride
        "outpad": desc(6, 5, 3, 3, pad=(1, 1), pout=(1, 2)),
        "outpad_acc": desc(6, 5, 3, 3, pad=(1, 1), pout=(1, 2), options=0),
        # block sizes
        "b_c3_7x7": desc(10, 9, 7, 7, 2, 2, pad=(3, 3), pin=LOGICAL, C=3, K=16),  # reduction length 147
        "b_c24_k40": desc(4, 5, 3, 3, pad=(1, 1), C=24, K=40),
        "b_c5_k7": desc(4, 5, 3, 3, pad=(1, 1), pin=LOGICAL, C=5, K=7),
        "b_k18": desc(4, 5, 1, 1, C=16, K=18),
        "b_c1_k1": desc(4, 5, 3, 3, pad=(1, 1), C=1, K=1),
        # the filter read through REGULAR_FILTER_TRANS in BWD
        "notrans": desc(6, 5, 3, 3, pad=(1, 1), C=32, K=24, options=OVERWRITE | NO_FILTER_TRANSPOSE),
        # rim contents: a physical rim filled with ones
        "rim_ones": desc(5, 4, 3, 3, pad=(1, 1)),
        # one case per side of the 128-tile of FWD that crosses it with a remainder (and of the 64-tile)
        "t_13x11": desc(13, 11, 3, 3, pad=(1, 1)),
        "t_k144": desc(4, 4, 1, 1, K=144),
        "t_n5": desc(6, 6, 3, 3, pad=(1, 1), pin=LOGICAL, N=5),
        # special values: a filter Inf and an input NaN at a border; products that underflow to -0.0
        "special_infnan_phys": desc(5, 4, 3, 3, pad=(1, 1)),
        "special_infnan_log": desc(5, 4, 3, 3, pad=(1, 1), pin=LOGICAL),
        "special_negzero_phys": desc(5, 4, 3, 3, pad=(1, 1)),
        "special_negzero_log": desc(5, 4, 3, 3, pad=(1, 1), pin=LOGICAL),
        "special_negzero_s2": desc(5, 4, 3, 3, 2, 2, pad=(1, 1), pin=LOGICAL),
    }
    for fuse in (0, 1, 2, 4, 6, 7):  # every fuse value with and without OPTION_OVERWRITE, all three passes
        for ow in (0, 1):
            out["f%d_o%d" % (fuse, ow)] = desc(fuse=fuse, options=ow, **BASE)
    return out


COMPUTE_CASES = compute_cases()
# every row of the "kept" list: the statuses of create in their order, of the bindings, of the scratch and of the passes
STATUS_CASES = {
    "e_nchw": desc(fmt=FMT_NCHW, **BASE), "e_kcrs": desc(fmt=FMT_KCRS, **BASE), "e_algo": desc(algo=2, **BASE),
    "e_nchw_kcrs_algo": desc(fmt=FMT_NCHW | FMT_KCRS, algo=2, **BASE), "e_kcrs_algo": desc(fmt=FMT_KCRS, algo=2, **BASE),
    "e_auto": desc(algo=ALGO_AUTO, **BASE),
    "e_unbound_regin": desc(**BASE), "e_unbound_regout": desc(**BASE), "e_unbound_regfil": desc(**BASE), "e_unbound_gradin": desc(**BASE),
    "e_unbound_gradout": desc(**BASE), "e_unbound_gradfil": desc(**BASE), "e_unbound_filtr": desc(**BASE), "e_noscratch": desc(**BASE),
}
UNBOUND = {"e_unbound_regin": (REG_IN,), "e_unbound_regout": (REG_OUT,), "e_unbound_regfil": (REG_FIL,), "e_unbound_gradin": (GRAD_IN,),
           "e_unbound_gradout": (GRAD_OUT,), "e_unbound_gradfil": (GRAD_FIL,), "e_unbound_filtr": (REG_FIL_TR,)}
NO_SCRATCH = ("e_noscratch",)
# what the reference cannot or must not run; its status at create is still captured: name -> (desc, why, the reference's create status)
NO_RUN = {
    "o_bf16": (desc(dt=BF16, **BASE), "ours alone: only F32 / F32 computes in the reference's generic path (the BF16 branch is inside #if 0)", SUCCESS),
    "o_f32_bf16": (desc(dt=F32, dt_out=BF16, **BASE), "ours alone: no such pair", SUCCESS),
    "o_nhwc": (desc(fmt=FMT_NHWC, **BASE), "ours alone: NHWC buffers are a later pull request", SUCCESS),
    "o_rsck": (desc(ffmt=FMT_RSCK, **BASE), "ours alone: RSCK filters are a later pull request", SUCCESS),
    "o_filter_kcrs": (desc(ffmt=FMT_KCRS, **BASE), "the reference tests KCRS on buffer_format only and would run into its format switch", SUCCESS),
    "o_pad_mixed": (desc(5, 4, 3, 3, pad=(1, 1), pin=(1, 0)), "ours alone: the reference reads the input without its offset", SUCCESS),
    "o_pad_other": (desc(5, 4, 3, 3, pad=(1, 1), pin=(2, 2)), "ours alone: the reference reads the input without its offset", SUCCESS),
    "o_fuse8": (desc(fuse=8, **BASE), "ours alone: the generic path ignores the batch-stats fusion silently", SUCCESS),
    "o_fuse128": (desc(fuse=128 | 1, **BASE), "ours alone: the generic path ignores the batch-norm fusion silently", SUCCESS),
    "o_n0": (desc(N=0, **BASE), "ours alone: nothing to do, and a layout of zero elements", SUCCESS),
    "o_negpad": (desc(5, 4, 1, 1, pad=(-1, 0), pin=(-1, 0)), "ours alone: the reference would index before its buffers", SUCCESS),
    "o_ofh0": (desc(1, 4, 3, 3), "ours alone: ofh = -1, loops that never run and layouts with a wrapped size", SUCCESS),
    "o_huge": (desc(64, 64, 3, 3, pad=(1, 1), N=1024, C=1024, K=16), "ours alone: 2^32 elements wrap the reference's unsigned sizes", SUCCESS),
    "o_threads3": (desc(threads=3, **BASE), "the reference's BWD waits at a barrier for three threads; only statuses, layouts and scratch sizes are captured", SUCCESS),
}
CREATE_ONLY = tuple(n for n in NO_RUN if n != "o_threads3")  # nothing but create is called: sizes and layouts would be garbage


def all_cases():
    out = dict(COMPUTE_CASES)
    out.update(STATUS_CASES)
    out.update({n: v[0] for n, v in NO_RUN.items()})
    return out


def captured_cases():
    return all_cases()


def _cdiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def block_of(n):
    """libxsmm_dnn_setup_generic: n below 16 is its own block, else the largest power of two up to 16 that divides n"""
    if n < 16:
        return n
    return max(t for t in (1, 2, 4, 8, 16) if n % t == 0)


def up64(n):
    return (n + 63) // 64 * 64


def ref_create_status(d):
    """what the reference's create answers (src/libxsmm_dnn.c:191-308 with the generic setup): three checks, in this order"""
    if d["buffer_format"] & FMT_NCHW:
        return ERR_INVALID_FORMAT_NCHW
    if d["buffer_format"] & FMT_KCRS:
        return ERR_INVALID_FORMAT_KCRS
    if d["algo"] not in (ALGO_AUTO, ALGO_DIRECT):
        return ERR_INVALID_ALGO
    return SUCCESS


# ---- handle rules (include/libxsmm_dnn_convolution.h) ---------------------------------------------------------------------------
class Handle:
    def __init__(self, d):
        self.d = d
        self.ok = False
        self.status = self._create_status()
        if self.status != SUCCESS:
            return
        self.ok = True
        self.ifmblock, self.ofmblock = block_of(d["C"]), block_of(d["K"])
        self.blocksifm, self.blocksofm = d["C"] // self.ifmblock, d["K"] // self.ofmblock
        self.ofh = _cdiv(d["H"] + 2 * d["pad_h"] - d["R"], d["u"]) + 1
        self.ofw = _cdiv(d["W"] + 2 * d["pad_w"] - d["S"], d["v"]) + 1
        self.ifhp, self.ifwp = d["H"] + 2 * d["pad_h_in"], d["W"] + 2 * d["pad_w_in"]
        self.ofhp, self.ofwp = self.ofh + 2 * d["pad_h_out"], self.ofw + 2 * d["pad_w_out"]
        self.hp, self.wp = d["H"] + 2 * d["pad_h"], d["W"] + 2 * d["pad_w"]  # the padded plane the templates work on
        self.physical = d["pad_h"] == d["pad_h_in"] and d["pad_w"] == d["pad_w_in"]
        self.overwrite = bool(d["options"] & OVERWRITE)
        th = d["threads"]
        self.s1 = 4 * d["C"] * d["K"] * d["R"] * d["S"]
        self.s5 = up64(4 * self.hp * self.wp * self.ifmblock) * th
        self.s6 = max(up64(4 * max(self.ofmblock * self.ofw * self.ofh, self.ifmblock * d["W"] * d["H"])) * th, up64(4 * self.ofhp * self.ofwp * self.ofmblock) * th)
        self.s7 = up64(4 * d["R"] * d["S"] * self.ifmblock * self.ofmblock) * th

    def _create_status(self):
        d = self.d
        st = ref_create_status(d)
        if st != SUCCESS:
            return st
        if (d["datatype_in"], d["datatype_out"]) != (F32, F32):
            return ERR_UNSUPPORTED_DATATYPE
        if d["buffer_format"] != FMT_LIBXSMM or d["filter_format"] != FMT_LIBXSMM:
            return ERR_INVALID_FORMAT_CONVOLVE
        if min(d[k] for k in ("N", "C", "H", "W", "K", "R", "S", "u", "v", "threads")) < 1 or min(d[k] for k in DESC_FIELDS[9:15]) < 0:
            return ERR_GENERAL
        if (d["pad_h_in"], d["pad_w_in"]) not in ((d["pad_h"], d["pad_w"]), (0, 0)):
            return ERR_INVALID_PADDING
        if d["fuse_ops"] & ~(FUSE_BIAS | FUSE_RELU):
            return ERR_FUSION
        hp, wp = d["H"] + 2 * d["pad_h"], d["W"] + 2 * d["pad_w"]
        if hp < d["R"] or wp < d["S"]:
            return ERR_GENERAL
        ofhp = (hp - d["R"]) // d["u"] + 1 + 2 * d["pad_h_out"]
        ofwp = (wp - d["S"]) // d["v"] + 1 + 2 * d["pad_w_out"]
        ifhp, ifwp = d["H"] + 2 * d["pad_h_in"], d["W"] + 2 * d["pad_w_in"]
        sizes = (d["N"] * d["C"] * ifhp * ifwp, d["N"] * d["C"] * hp * wp, d["N"] * d["K"] * ofhp * ofwp, d["C"] * d["K"] * d["R"] * d["S"])
        return ERR_GENERAL if max(sizes) >= 2 ** 31 else SUCCESS

    def scratch(self, kind):
        """(size, status) of libxsmm_dnn_get_scratch_size (src/libxsmm_dnn.c:1720-1808 in the generic path)"""
        s1, s3, s5, s6, s7 = self.s1 + 64, 64, self.s5 + 64, self.s6 + 64, self.s7 + 64
        sizes = {FWD: s5 + s6 + s7, BWD: s1 + s5 + s7, UPD: s3 + s5 + s6 + s7, ALL: s1 + s3 + s5 + s6 + s7}
        return (sizes[kind], SUCCESS) if kind in sizes else (0, ERR_INVALID_KIND)

    def layout(self, t):
        """(status, None) or (0, dict) as libxsmm_dnn_create_tensor_datalayout (src/libxsmm_dnn.c:363-997), F32 in custom format 1"""
        d = self.d
        if t in (REG_IN, GRAD_IN, GEN_IN):
            return made((DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), (self.ifmblock, self.ifwp, self.ifhp, self.blocksifm, d["N"]), F32, d["buffer_format"], 9)
        if t in (REG_OUT, GRAD_OUT, GEN_OUT):
            return made((DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), (self.ofmblock, self.ofwp, self.ofhp, self.blocksofm, d["N"]), F32, d["buffer_format"], 9)
        if t in (REG_FIL, GRAD_FIL, GEN_FIL):
            return made((DIM_K, DIM_C, DIM_S, DIM_R, DIM_C, DIM_K), (self.ofmblock, self.ifmblock, d["S"], d["R"], self.blocksifm, self.blocksofm), F32,
                        d["filter_format"], GEN_FIL)
        if t == REG_FIL_TR:
            return made((DIM_C, DIM_K, DIM_S, DIM_R, DIM_K, DIM_C), (self.ifmblock, self.ofmblock, d["S"], d["R"], self.blocksofm, self.blocksifm), F32,
                        d["filter_format"], REG_FIL_TR)
        if t in (REG_BIAS, GRAD_BIAS, GEN_BIAS):
            return made((DIM_C, DIM_C), (self.ofmblock, self.blocksofm), F32, d["buffer_format"], 26)
        return ERR_UNKNOWN_TENSOR_TYPE, None

    def work(self, kind):
        return {FWD: self.d["N"] * self.blocksofm, BWD: self.d["N"] * self.blocksifm, UPD: self.blocksifm * self.blocksofm}[kind]

    def share(self, kind, ltid):
        return share(self.work(kind), self.d["threads"], ltid)

    def execute_status(self, kind, bound, scratch_bwd=True, scratch_upd=True, ltid=0):
        """what execute_st returns before anything is computed (bound: the tensor types that are bound). Up to the first
        ERR_DATA_NOT_BOUND the reference's; the rest is this engine's own."""
        if kind not in (FWD, BWD, UPD):
            return ERR_INVALID_KIND
        need = {FWD: (REG_IN, REG_OUT, REG_FIL), BWD: (GRAD_IN, GRAD_OUT, REG_FIL), UPD: (REG_IN, GRAD_OUT, GRAD_FIL)}[kind]
        if any(t not in bound for t in need) or (kind == BWD and not scratch_bwd) or (kind == UPD and not scratch_upd):
            return ERR_DATA_NOT_BOUND
        if kind == FWD and self.d["fuse_ops"] & FUSE_BIAS and REG_BIAS not in bound:
            return ERR_DATA_NOT_BOUND
        if kind == BWD and self.d["options"] & NO_FILTER_TRANSPOSE and REG_FIL_TR not in bound:
            return ERR_DATA_NOT_BOUND
        return ERR_GENERAL if ltid < 0 else SUCCESS

    def upd_per_image(self):
        """the upd template :91-92: False is the GEMM form"""
        d = self.d
        return not ((d["R"] == 1 and d["S"] == 1 and self.physical) or (d["u"] == 1 and d["v"] == 1))

    # shapes of the tensors as arrays
    def in_shape(self):
        return (self.d["N"], self.blocksifm, self.ifhp, self.ifwp, self.ifmblock)

    def out_shape(self):
        return (self.d["N"], self.blocksofm, self.ofhp, self.ofwp, self.ofmblock)

    def fil_shape(self):
        return (self.blocksofm, self.blocksifm, self.d["R"], self.d["S"], self.ifmblock, self.ofmblock)

    def filtr_shape(self):
        return (self.blocksifm, self.blocksofm, self.d["R"], self.d["S"], self.ofmblock, self.ifmblock)

    def bias_shape(self):
        return (self.blocksofm, self.ofmblock)


# ---- inputs: seeded, in the tensors' own layout ----------------------------------------------------------------------------------
POISON = np.frombuffer(b"\xff\xff\xff\xff", dtype=np.float32)[0]  # what a destination that is overwritten starts from


def inputs(name, d):
    """dict of x, w, dout, bias (the whole tensors, physical padding included) and out0, din0, dw0: what the destinations hold before
    a pass -- seeded values where the pass accumulates, ones bits where it overwrites (FWD: also with a bias)"""
    h = Handle(d)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = lambda shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    t = dict(x=n(h.in_shape()), w=n(h.fil_shape()), dout=n(h.out_shape()), bias=n(h.bias_shape()), out0=n(h.out_shape()), din0=n(h.in_shape()),
             dw0=n(h.fil_shape()))
    ph, pw = d["pad_h_in"], d["pad_w_in"]
    if name == "rim_ones":
        inner = t["x"][:, :, ph:ph + d["H"], pw:pw + d["W"], :].copy()
        t["x"][...] = 1
        t["x"][:, :, ph:ph + d["H"], pw:pw + d["W"], :] = inner
    if name.startswith("special_infnan"):
        t["w"][0, 0, 0, 0, 1, 2] = np.inf            # the filter's corner: it meets the rim at every border output
        t["w"][0, 0, 2, 1, 0, 3] = -np.inf
        t["x"][0, 0, ph, pw, 1] = np.nan             # the first pixel of the interior
        t["x"][1, 0, ph + d["H"] - 1, pw + d["W"] - 1, 0] = np.inf
        t["dout"][0, 0, d["pad_h_out"], d["pad_w_out"], 2] = np.nan
        t["dout"][1, 0, d["pad_h_out"] + h.ofh - 1, d["pad_w_out"] + h.ofw - 1, 3] = np.inf
    if name.startswith("special_negzero"):           # every product underflows to -0.0
        t["x"][...] = np.float32(1e-30)
        t["dout"][...] = np.float32(1e-30)
        t["w"][...] = np.float32(-1e-30)
    if h.overwrite:
        t["din0"][...] = POISON
        t["dw0"][...] = POISON
    if h.overwrite or d["fuse_ops"] & FUSE_BIAS:
        t["out0"][...] = POISON
    return t


# ---- the three templates, loop for loop ----------------------------------------------------------------------------------------------
def _smm(arith, m, n, k, lda, ldb, ldc, a, b, c):
    orc.smm(arith, 0, m, n, k, lda, ldb, ldc, a, b, c)


def trans_filter(h, w):
    """libxsmm_dnn_trans_reg_filter (src/libxsmm_dnn.c:1571-1604) and the transposition at the head of the bwd template"""
    w = np.asarray(w, dtype=np.float32).reshape(h.fil_shape())
    return np.ascontiguousarray(w[:, :, ::-1, ::-1, :, :].transpose(1, 0, 2, 3, 5, 4))


def fwd(h, x, w, out0, bias, ltid=0, arith=orc.FMA):
    """the output tensor after FWD of logical thread ltid on out0 (fwd template :32-152)"""
    d = h.d
    R, S, u, v, ib, ob = d["R"], d["S"], d["u"], d["v"], h.ifmblock, h.ofmblock
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    out = np.array(out0, dtype=np.float32).reshape(h.out_shape())
    flat = out.reshape(-1)
    xs = h.in_shape()
    padded = np.zeros((h.hp, h.wp, ib), dtype=np.float32)
    b0, b1 = h.share(FWD, ltid)
    for item in range(b0, b1):
        img, ofm1 = divmod(item, h.blocksofm)
        inner = out[img, ofm1, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :]
        if d["fuse_ops"] & FUSE_BIAS:
            inner[...] = np.asarray(bias, dtype=np.float32).reshape(h.bias_shape())[ofm1]
        for ifm1 in range(h.blocksifm):
            if ifm1 == 0 and h.overwrite and not d["fuse_ops"] & FUSE_BIAS:
                inner[...] = 0
            if h.physical:
                src, src_w, base = x, h.ifwp, (img * h.blocksifm + ifm1) * h.ifhp * h.ifwp * ib
            else:
                padded[d["pad_h"]:d["pad_h"] + d["H"], d["pad_w"]:d["pad_w"] + d["W"], :] = x.reshape(xs)[img, ifm1]
                src, src_w, base = padded.reshape(-1), h.wp, 0
            for oj in range(h.ofh):
                c = flat[(((img * h.blocksofm + ofm1) * h.ofhp + d["pad_h_out"] + oj) * h.ofwp + d["pad_w_out"]) * ob:]
                for kj in range(R):
                    for ki in range(S):
                        a = w[(((ofm1 * h.blocksifm + ifm1) * R + kj) * S + ki) * ib * ob:]
                        b = src[base + ((oj * u + kj) * src_w + ki) * ib:]
                        _smm(arith, ob, h.ofw, ib, ob, v * ib, ob, a, b, c)
        if d["fuse_ops"] & FUSE_RELU:
            inner[...] = np.where(inner < 0, np.float32(0), inner)
    return out


def bwd(h, dout, w, din0, ltid=0, arith=orc.FMA):
    """the dinput tensor after BWD of logical thread ltid on din0 (bwd template :32-197); the filter is read through its
    transposed copy, as there"""
    d = h.d
    R, S, u, v, ib, ob = d["R"], d["S"], d["u"], d["v"], h.ifmblock, h.ofmblock
    dout = np.ascontiguousarray(dout, dtype=np.float32).reshape(-1)
    wt = trans_filter(h, w).reshape(-1)
    din = np.array(din0, dtype=np.float32).reshape(h.in_shape())
    flat = din.reshape(-1)
    padded = np.zeros((h.hp, h.wp, ib), dtype=np.float32)
    b0, b1 = h.share(BWD, ltid)
    for item in range(b0, b1):
        img, ifm1 = divmod(item, h.blocksifm)
        if h.physical:
            if h.overwrite:
                din[img, ifm1] = 0
            dst, dst_w, base = flat, h.ifwp, (img * h.blocksifm + ifm1) * h.ifhp * h.ifwp * ib
        else:
            if h.overwrite:
                padded[...] = 0
            else:
                padded[d["pad_h"]:d["pad_h"] + d["H"], d["pad_w"]:d["pad_w"] + d["W"], :] = din[img, ifm1]
            dst, dst_w, base = padded.reshape(-1), h.wp, 0
        for ofm1 in range(h.blocksofm):
            for oj in range(h.ofh):
                b = dout[(((img * h.blocksofm + ofm1) * h.ofhp + d["pad_h_out"] + oj) * h.ofwp + d["pad_w_out"]) * ob:]
                for kj in range(R):
                    for ki in range(S):
                        a = wt[(((ifm1 * h.blocksofm + ofm1) * R + R - 1 - kj) * S + S - 1 - ki) * ob * ib:]
                        c = dst[base + ((oj * u + kj) * dst_w + ki) * ib:]
                        _smm(arith, ib, h.ofw, ob, ib, ob, v * ib, a, b, c)
        if h.physical:
            ph, pw = d["pad_h_in"], d["pad_w_in"]
            if ph > 0 or pw > 0:
                inner = din[img, ifm1, ph:ph + d["H"], pw:pw + d["W"], :].copy()
                din[img, ifm1] = 0
                din[img, ifm1, ph:ph + d["H"], pw:pw + d["W"], :] = inner
        else:
            din[img, ifm1] = padded[d["pad_h"]:d["pad_h"] + d["H"], d["pad_w"]:d["pad_w"] + d["W"], :]
    return din


def upd(h, x, dout, dw0, ltid=0, arith=orc.FMA):
    """the dfilter tensor after UPD of logical thread ltid on dw0 (upd template :32-205)"""
    d = h.d
    R, S, u, v, ib, ob = d["R"], d["S"], d["u"], d["v"], h.ifmblock, h.ofmblock
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(h.in_shape())
    xflat = x.reshape(-1)
    dout = np.ascontiguousarray(dout, dtype=np.float32).reshape(h.out_shape())
    dflat = dout.reshape(-1)
    dw = np.array(dw0, dtype=np.float32).reshape(h.fil_shape())
    wflat = dw.reshape(-1)
    input_scratch = np.zeros(h.hp * h.wp * ib, dtype=np.float32)  # (zeroed once per call, as there)
    input_trans = input_scratch.reshape(h.hp, ib, h.wp)
    input_padded = input_scratch.reshape(h.hp, h.wp, ib)
    output_trans = np.zeros((h.ofhp, ob, h.ofwp), dtype=np.float32)
    local = np.zeros((R, S, ob, ib), dtype=np.float32)
    po_h, po_w = d["pad_h_out"], d["pad_w_out"]
    b0, b1 = h.share(UPD, ltid)
    for item in range(b0, b1):
        ofm1, ifm1 = divmod(item, h.blocksifm)
        if h.overwrite:
            dw[ofm1, ifm1] = 0
        for img in range(d["N"]):
            if not h.upd_per_image():
                if h.physical:
                    nr, nc = h.ifhp // u, h.ifwp // v
                    input_trans[:nr, :, :nc] = x[img, ifm1, 0:nr * u:u, 0:nc * v:v, :].transpose(0, 2, 1)
                else:
                    nr, nc = d["H"] // u, d["W"] // v
                    input_trans[d["pad_h"]:d["pad_h"] + nr, :, d["pad_w"]:d["pad_w"] + nc] = x[img, ifm1, 0:nr * u:u, 0:nc * v:v, :].transpose(0, 2, 1)
                for oj in range(h.ofh):
                    a = dflat[(((img * h.blocksofm + ofm1) * h.ofhp + po_h + oj) * h.ofwp + po_w) * ob:]
                    for kj in range(R):
                        for ki in range(S):
                            b = input_scratch[(oj + kj) * ib * h.wp + ki:]
                            c = wflat[(((ofm1 * h.blocksifm + ifm1) * R + kj) * S + ki) * ib * ob:]
                            _smm(arith, ob, ib, h.ofw, ob, h.wp, ob, a, b, c)
                continue
            local[...] = 0
            lflat = local.reshape(-1)
            if h.physical:
                output_trans[...] = dout[img, ofm1].transpose(0, 2, 1)
                src, src_w, base, oh, ow = xflat, h.ifwp, (img * h.blocksifm + ifm1) * h.ifhp * h.ifwp * ib, po_h, po_w
            else:
                input_padded[d["pad_h"]:d["pad_h"] + d["H"], d["pad_w"]:d["pad_w"] + d["W"], :] = x[img, ifm1]
                output_trans[:h.ofh, :, :h.ofw] = dout[img, ofm1, po_h:po_h + h.ofh, po_w:po_w + h.ofw, :].transpose(0, 2, 1)
                src, src_w, base, oh, ow = input_scratch, h.wp, 0, 0, 0
            oflat = output_trans.reshape(-1)
            for oj in range(h.ofh):
                for kj in range(R):
                    for ki in range(S):
                        a = src[base + ((oj * u + kj) * src_w + ki) * ib:]
                        b = oflat[(oj + oh) * ob * h.ofwp + ow:]
                        c = lflat[(kj * S + ki) * ob * ib:]
                        _smm(arith, ib, ob, h.ofw, v * ib, h.ofwp, ib, a, b, c)
            dw[ofm1, ifm1] += local.transpose(0, 1, 3, 2)
    return dw


@functools.lru_cache(maxsize=None)
def expected(name, arith=orc.FMA):
    """dict of the inputs of a compute case and of out, din, dw, wtr after the passes with threads = 1 (computed once, shared: read only)"""
    d = COMPUTE_CASES[name]
    return _with_outputs(Handle(d), inputs(name, d), arith)


def _with_outputs(h, t, arith):
    """t with out, din, dw and wtr after the passes, the shares of the logical threads in turn (read only)"""
    t["out"], t["din"], t["dw"] = t["out0"], t["din0"], t["dw0"]
    for ltid in range(h.d["threads"]):
        t["out"] = fwd(h, t["x"], t["w"], t["out"], t["bias"], ltid, arith)
        t["din"] = bwd(h, t["dout"], t["w"], t["din"], ltid, arith)
        t["dw"] = upd(h, t["x"], t["dout"], t["dw"], ltid, arith)
    t["wtr"] = trans_filter(h, t["w"])
    for a in t.values():
        a.setflags(write=False)
    return t


# ---- the seeded sweep: descriptors nobody picked --------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 1, 48
SWEEP_FEATURES = (1, 3, 5, 8, 16, 17, 18, 24, 32, 40, 144)
RELU_NEAR_ZERO = 0.02  # the share of a case's outputs that the float64 comparison may leave out because the ReLU's argument is within the bound of 0


def _draw(rng):
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    H, W, R, S, u, v = pick(1, 9), pick(1, 9), pick(1, 4), pick(1, 4), pick(1, 3), pick(1, 3)
    pad = (pick(0, 2), pick(0, 2))
    pin = pad if pick(0, 1) else LOGICAL
    pout = (pick(0, 2), pick(0, 2))
    N, C, K = pick(1, 3), SWEEP_FEATURES[pick(0, 10)], SWEEP_FEATURES[pick(0, 10)]
    options = (0, OVERWRITE, NO_FILTER_TRANSPOSE, OVERWRITE | NO_FILTER_TRANSPOSE)[pick(0, 3)]
    return desc(H, W, R, S, u, v, pad=pad, pin=pin, pout=pout, N=N, C=C, K=K, threads=pick(1, 3), options=options, fuse=pick(0, 7))


def contract64(h, t):
    """key -> (value, bound, compared) for out, din and dw: naive64 with the chain's start value added where the pass accumulates
    or has a bias, UPD's GEMM form as the reference has it, the ReLU applied in float64, and the bound terms * 2^-24 * (sum|a * b| +
    |start|) of an fp32 chain (derived, as the guard of tools/golden/conv_capture.py). compared: False where the ReLU's argument
    lies within the bound of 0, so that the two sides may be on either side of it. "unreached": the elements of dinput no term
    reaches, which keep their start bits (overwrite: +0.0)."""
    d = h.d
    want, terms = naive64(h, t, gemm_form_copy=True)
    res = {}
    start = {"out": interior(h, "out", t["out0"]).astype(np.float64), "din": interior(h, "din", t["din0"]).astype(np.float64),
             "dw": interior(h, "dw", t["dw0"]).astype(np.float64)}
    if d["fuse_ops"] & FUSE_BIAS:
        start["out"] = np.broadcast_to(np.asarray(t["bias"], dtype=np.float64).reshape(1, d["K"], 1, 1), start["out"].shape)
    elif h.overwrite:
        start["out"] = np.zeros_like(start["out"])
    if h.overwrite:
        start["din"], start["dw"] = np.zeros_like(start["din"]), np.zeros_like(start["dw"])
    for key in ("out", "din", "dw"):
        value, weight = want[key]
        value, bound = value + start[key], terms[key] * 2.0 ** -24 * (weight + np.abs(start[key]))
        compared = np.ones(value.shape, dtype=bool)
        if key == "out" and d["fuse_ops"] & FUSE_RELU:
            compared = np.abs(value) > bound
            value = np.maximum(value, 0)
        res[key] = (value, bound, compared)
    res["unreached"] = want["din_terms"] == 0
    return res


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """name -> desc: SWEEP_CASES descriptors drawn from SWEEP_SEED, those that create refuses left out, and those (none so far)
    whose ReLU leaves more than RELU_NEAR_ZERO of the outputs uncompared replaced by the next draw. tests/test_conv_sweep_cpu.py
    counts what the set holds; the seed is the first from 0 up that passes that census."""
    rng = np.random.default_rng(SWEEP_SEED)
    out = {}
    while len(out) < SWEEP_CASES:
        d = _draw(rng)
        h = Handle(d)
        if h.status != SUCCESS:
            continue
        name = "sweep_%02d" % len(out)
        if d["fuse_ops"] & FUSE_RELU and np.mean(~contract64(h, inputs(name, d))["out"][2]) >= RELU_NEAR_ZERO:
            continue
        out[name] = d
    return out


@functools.lru_cache(maxsize=None)
def sweep_expected(name):
    """expected() of a sweep case: the shares of its logical threads in turn"""
    d = sweep_cases()[name]
    return _with_outputs(Handle(d), inputs(name, d), orc.FMA)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def same_bits(got, want, nan_class=False):
    """bitwise equality. nan_class (the special_* cases on the GPU only): an element that is NaN in both counts as equal whatever
    its sign and payload -- x86 answers 0 * Inf with the negative default NaN 0xffc00000, gfx950 with 0x7fc00000"""
    g, w = bits(got), bits(want)
    if g.shape != w.shape:
        return False
    if not nan_class:
        return bool(np.array_equal(g, w))
    both = np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))
    return bool(np.array_equal(g[~both], w[~both]))


def naive64(h, t, gemm_form_copy=False):
    """(out, din, dw) of a plain float64 convolution of the inputs t with the chains' start values, and per element the number of
    terms and the sum of |a * b|: the guard of tools/golden/conv_capture.py. Interior elements only ([N][C or K][rows][columns]).
    "din_terms" counts the terms that reach an element of dinput. gemm_form_copy: UPD as the reference's GEMM form computes it
    where that is no plain convolution (upd template :95-103): with a physical padding it reads a copy of the input
    that holds rows below ifhp / u * u and columns below ifwp / v * v only, the rest is +0.0 (a stride above 1 means a 1 x 1 window
    there, so ifhp % u rows at the bottom and ifwp % v columns at the right drop out of dW)."""
    d = h.d
    N, C, K, R, S, u, v = d["N"], d["C"], d["K"], d["R"], d["S"], d["u"], d["v"]
    ph, pw, qh, qw = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]
    plain = lambda a, p, q, rows, cols: a.astype(np.float64)[:, :, p:p + rows, q:q + cols, :].transpose(0, 1, 4, 2, 3).reshape(N, -1, rows, cols)  # noqa: E731
    x = np.zeros((N, C, h.hp, h.wp))
    x[:, :, d["pad_h"]:d["pad_h"] + d["H"], d["pad_w"]:d["pad_w"] + d["W"]] = plain(t["x"], ph, pw, d["H"], d["W"])
    if h.physical:  # (the rim is read as it is)
        x = plain(t["x"], 0, 0, h.ifhp, h.ifwp)
    dout = plain(t["dout"], qh, qw, h.ofh, h.ofw)
    w = t["w"].astype(np.float64).transpose(0, 5, 1, 4, 2, 3).reshape(K, C, R, S)
    out, out_abs = np.zeros((N, K, h.ofh, h.ofw)), np.zeros((N, K, h.ofh, h.ofw))
    din, din_abs = np.zeros((N, C, h.hp, h.wp)), np.zeros((N, C, h.hp, h.wp))
    dw, dw_abs = np.zeros((K, C, R, S)), np.zeros((K, C, R, S))
    din_terms = np.zeros((N, C, h.hp, h.wp), dtype=np.int64)
    x_upd = x
    if gemm_form_copy and h.physical and not h.upd_per_image():
        x_upd = x.copy()
        x_upd[:, :, h.ifhp // u * u:, :] = 0
        x_upd[:, :, :, h.ifwp // v * v:] = 0
    for kj in range(R):
        for ki in range(S):
            xs = x[:, :, kj:kj + (h.ofh - 1) * u + 1:u, ki:ki + (h.ofw - 1) * v + 1:v]
            out += np.einsum("nchw,kc->nkhw", xs, w[:, :, kj, ki])
            out_abs += np.einsum("nchw,kc->nkhw", np.abs(xs), np.abs(w[:, :, kj, ki]))
            din[:, :, kj:kj + (h.ofh - 1) * u + 1:u, ki:ki + (h.ofw - 1) * v + 1:v] += np.einsum("nkhw,kc->nchw", dout, w[:, :, kj, ki])
            din_abs[:, :, kj:kj + (h.ofh - 1) * u + 1:u, ki:ki + (h.ofw - 1) * v + 1:v] += np.einsum("nkhw,kc->nchw", np.abs(dout), np.abs(w[:, :, kj, ki]))
            din_terms[:, :, kj:kj + (h.ofh - 1) * u + 1:u, ki:ki + (h.ofw - 1) * v + 1:v] += K
            xs = x_upd[:, :, kj:kj + (h.ofh - 1) * u + 1:u, ki:ki + (h.ofw - 1) * v + 1:v]
            dw[:, :, kj, ki] = np.einsum("nkhw,nchw->kc", dout, xs)
            dw_abs[:, :, kj, ki] = np.einsum("nkhw,nchw->kc", np.abs(dout), np.abs(xs))
    cut = (slice(None), slice(None), slice(d["pad_h"], d["pad_h"] + d["H"]), slice(d["pad_w"], d["pad_w"] + d["W"]))
    terms = dict(out=C * R * S, din=K * R * S, dw=N * h.ofh * h.ofw)
    return dict(out=(out, out_abs), din=(din[cut], din_abs[cut]), dw=(dw, dw_abs), din_terms=din_terms[cut]), terms


def interior(h, key, a):
    """the elements of a captured tensor that naive64 computes, in its index order"""
    d = h.d
    a = np.asarray(a, dtype=np.float32)
    if key == "out":
        a = a.reshape(h.out_shape())[:, :, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :]
        return a.transpose(0, 1, 4, 2, 3).reshape(d["N"], d["K"], h.ofh, h.ofw)
    if key == "din":
        a = a.reshape(h.in_shape())[:, :, d["pad_h_in"]:d["pad_h_in"] + d["H"], d["pad_w_in"]:d["pad_w_in"] + d["W"], :]
        return a.transpose(0, 1, 4, 2, 3).reshape(d["N"], d["C"], d["H"], d["W"])
    return a.reshape(h.fil_shape()).transpose(0, 5, 1, 4, 2, 3).reshape(d["K"], d["C"], d["R"], d["S"])


def load_golden():
    import os
    with np.load(os.path.join(GOLDEN, "conv.npz")) as z:
        return {k: z[k] for k in z.files}
