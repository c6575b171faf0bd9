"""The fused batch-norm layer restated in numpy: handle rules, datalayouts, scratch formula, the statuses of execute_st, the split
over logical threads, seeded inputs, and the arithmetic contract of include/libxsmm_dnn_fusedbatchnorm.h (FWD and BWD, the eight
fuse combinations, fp32 and bf16) as plain array code. Shared by tests/test_bn_cpu.py, tests/test_bn_gpu.py and
tools/golden/bn_capture.py; the reference's own answers are in tests/golden/bn.npz and tests/test_bn_cpu.py holds this file
against them bit for bit."""
import functools
import os
import zlib

import numpy as np

from dnn_common import *  # noqa: F401,F403 (re-exported: the tests reach every shared name through this module)
from dnn_common import FmHandle, fma

OPS_BN, OPS_BNSCALE, OPS_ELTWISE, OPS_RELU = 1, 2, 4, 8
FUSE_COMBINATIONS = (1, 2, 5, 6, 9, 10, 13, 14)
REG_ADD, GRAD_ADD = 1, 4
REG_BETA, GRAD_BETA, GEN_BETA, REG_GAMMA, GRAD_GAMMA, GEN_GAMMA, MEAN, RSTD, VAR, CHANNEL_SCALAR = 17, 18, 19, 20, 21, 22, 23, 24, 25, 26
BINDABLE = (REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, REG_ADD, GRAD_ADD, REG_BETA, GRAD_BETA, REG_GAMMA, GRAD_GAMMA, MEAN, RSTD, VAR)
LAYOUT_TYPES = BINDABLE + (GEN_IN, GEN_OUT, GEN_BETA, GEN_GAMMA, REG_FIL)  # the layouts the capture asks for (the last one is no batch-norm tensor)
ERR_FUSEBN_UNSUPPORTED_ORDER, ERR_FUSEBN_UNSUPPORTED_FUSION = 100030, 100031

DESC_FIELDS = ("N", "C", "H", "W", "u", "v", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out", "threads", "datatype_in", "datatype_out",
               "datatype_stats", "buffer_format", "fuse_order", "fuse_ops")
# the tensors of a case: key -> tensor type. Inputs are seeded; the rest are destinations (pre-filled with ones bits).
KEYS = {"x": REG_IN, "add": REG_ADD, "dout": GRAD_OUT, "gamma": REG_GAMMA, "beta": REG_BETA, "mean": MEAN, "rstd": RSTD, "var": VAR, "out": REG_OUT,
        "din": GRAD_IN, "dadd": GRAD_ADD, "dgamma": GRAD_GAMMA, "dbeta": GRAD_BETA}
CHUNK = 128  # pixels the partial-sum kernel adds between two barriers (kernels/bn.hip: CH)


def desc(H, W, N=2, C=16, u=1, v=1, pin=(0, 0), pout=(0, 0), ops=OPS_BN, dt=F32, dt_out=None, dt_stats=F32, fmt=FMT_LIBXSMM, order=0, threads=1):
    return dict(N=N, C=C, H=H, W=W, u=u, v=v, pad_h_in=pin[0], pad_w_in=pin[1], pad_h_out=pout[0], pad_w_out=pout[1], threads=threads, datatype_in=dt,
                datatype_out=dt if dt_out is None else dt_out, datatype_stats=dt_stats, buffer_format=fmt, fuse_order=order, fuse_ops=ops)


def compute_cases():
    """name -> desc: the smallest shapes at which something can go wrong. The name ends in the element type and, after it, the
    kind of input: n random normals, t a 7-value alphabet with 0 and -0.0, c one constant channel."""
    out = {}
    for dt, dname in ((F32, "f32"), (BF16, "bf16")):
        for ops in FUSE_COMBINATIONS:                     # 1: every fuse combination, two blocks, 15 pixels
            out["fuse%d_%s_n" % (ops, dname)] = desc(5, 3, C=32, ops=ops, dt=dt)
        out["pad_%s_n" % dname] = desc(6, 4, N=3, pin=(1, 2), pout=(2, 1), ops=13, dt=dt)       # 2: rows are not contiguous
        out["stride_bn_%s_n" % dname] = desc(6, 4, u=2, v=2, ops=9, dt=dt)                      # 3: statistics over all pixels, the rest strided
        out["stride_scale_%s_n" % dname] = desc(6, 4, u=2, v=2, ops=6, dt=dt)
        out["one_%s_n" % dname] = desc(1, 1, N=1, ops=1, dt=dt)                                 # 4: var is 0 or noise, rstd comes from the epsilon
        out["chunk_%s_n" % dname] = desc(29, 29, ops=13, dt=dt)                                 # 5: 841 pixels = 6 chunks of 128 and 73 more
        out["images_%s_n" % dname] = desc(4, 4, N=5, C=48, ops=1, dt=dt)                        # 6: five terms in image order, three blocks
        out["c24_%s_n" % dname] = desc(5, 3, C=24, ops=9, dt=dt)                                # 7: the remainder of 8 channels is lost
        out["const_%s_c" % dname] = desc(5, 3, ops=1, dt=dt)                                    # 9: a constant channel: var may round below zero
    out["zeros_f32_t"] = desc(5, 3, ops=9)                                                      # 8: exact zeros and -0.0 reach the output
    return out


COMPUTE_CASES = compute_cases()
assert 29 * 29 > CHUNK and 29 * 29 % CHUNK != 0
# 10: a NaN and an Inf in one channel each; FWD only
SPECIAL_CASES = {"nonfinite_f32": desc(5, 3, ops=9), "nonfinite_bf16": desc(5, 3, ops=9, dt=BF16)}
_S = dict(H=6, W=4)
STATUS_CASES = {
    "e_f32_bf16": desc(dt=F32, dt_out=BF16, **_S), "e_bf16_f32": desc(dt=BF16, dt_out=F32, **_S), "e_c8": desc(C=8, **_S),
    "e_nhwc": desc(fmt=FMT_NHWC, **_S), "e_nhwc_bf16": desc(fmt=FMT_NHWC, dt=BF16, **_S), "e_nchw": desc(fmt=FMT_NCHW, **_S),
    "e_fmt3": desc(fmt=FMT_LIBXSMM | FMT_NHWC, **_S), "e_stats_bf16": desc(dt_stats=BF16, **_S), "e_stats_nhwc": desc(dt_stats=BF16, fmt=FMT_NHWC, **_S),
    "e_order1": desc(order=1, **_S), "e_ops0": desc(ops=0, **_S), "e_ops3": desc(ops=3, **_S), "e_ops4": desc(ops=4, **_S), "e_ops7": desc(ops=7, **_S),
    "e_ops12": desc(ops=12, **_S), "e_ops17": desc(ops=17, **_S),
    "e_un_regin": desc(ops=13, **_S), "e_un_regout": desc(ops=5, **_S), "e_un_regout_relu": desc(ops=13, **_S), "e_un_beta": desc(ops=13, **_S),
    "e_un_gamma": desc(ops=13, **_S), "e_un_mean": desc(ops=14, **_S), "e_un_rstd": desc(ops=14, **_S), "e_un_var": desc(ops=2, **_S),
    "e_un_regadd": desc(ops=5, **_S), "e_un_regadd_noelt": desc(ops=9, **_S), "e_un_gradin": desc(ops=13, **_S), "e_un_gradout": desc(ops=13, **_S),
    "e_un_gradbeta": desc(ops=2, **_S), "e_un_gradgamma": desc(ops=2, **_S), "e_un_gradadd": desc(ops=6, **_S), "e_un_gradadd_noelt": desc(ops=10, **_S),
    "e_un_order": desc(ops=13, order=1, **_S),   # an unbound tensor is found before the fuse order
}
UNBOUND = {"e_un_regin": (REG_IN,), "e_un_regout": (REG_OUT,), "e_un_regout_relu": (REG_OUT,), "e_un_beta": (REG_BETA,), "e_un_gamma": (REG_GAMMA,),
           "e_un_mean": (MEAN,), "e_un_rstd": (RSTD,), "e_un_var": (VAR,), "e_un_regadd": (REG_ADD,), "e_un_regadd_noelt": (REG_ADD,),
           "e_un_gradin": (GRAD_IN,), "e_un_gradout": (GRAD_OUT,), "e_un_gradbeta": (GRAD_BETA,), "e_un_gradgamma": (GRAD_GAMMA,),
           "e_un_gradadd": (GRAD_ADD,), "e_un_gradadd_noelt": (GRAD_ADD,), "e_un_order": (REG_IN,)}
# the case the reference must not execute: it writes C-wide pixels into an output layout of zero elements
NO_RUN = ("e_c8",)


def captured_cases():
    out = dict(COMPUTE_CASES)
    out.update(SPECIAL_CASES)
    out.update(STATUS_CASES)
    return out


# ---- handle rules (src/libxsmm_dnn_fusedbatchnorm.c:45-89, src/libxsmm_dnn_setup.c:197-252) ----------------------------------------
class Handle(FmHandle):
    def __init__(self, d):
        super().__init__(d)
        if self.status != SUCCESS:
            return
        self.set_output(d["H"] // d["u"], d["W"] // d["v"])
        self.scratch_size = 4 * 2 * d["C"] * d["N"]
        self.ok = True

    def layout(self, t):
        """(status, None) or (0, dict) as libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout (:108-314)"""
        d = self.d
        inp, out = t in (REG_IN, GRAD_IN, GEN_IN, REG_ADD, GRAD_ADD), t in (REG_OUT, GRAD_OUT, GEN_OUT)
        chan = t in (REG_BETA, GRAD_BETA, GEN_BETA, REG_GAMMA, GRAD_GAMMA, GEN_GAMMA, MEAN, RSTD, VAR)
        fmt = d["buffer_format"]
        if inp or out:
            return self.activation_layout(inp)
        if chan:
            if not fmt & (FMT_LIBXSMM | FMT_NHWC):
                return ERR_INVALID_FORMAT_GENERAL, None
            if d["datatype_stats"] != F32:
                return ERR_UNSUPPORTED_DATATYPE, None
            if fmt & FMT_LIBXSMM:
                return made((DIM_C, DIM_C), (self.ifmblock * self.fm_lp_block, self.blocksifm), F32, fmt, CHANNEL_SCALAR)
            return made((DIM_C,), (d["C"],), F32, fmt, CHANNEL_SCALAR)
        return ERR_UNKNOWN_TENSOR_TYPE, None

    def needed(self, kind):
        ops = self.d["fuse_ops"]
        if kind == FWD:
            need = [REG_IN, REG_OUT, REG_BETA, REG_GAMMA, MEAN, RSTD, VAR] + ([REG_ADD] if ops & OPS_ELTWISE else [])
        else:
            need = [REG_IN, REG_GAMMA, GRAD_IN, GRAD_OUT, GRAD_BETA, GRAD_GAMMA, MEAN, RSTD] + ([GRAD_ADD] if ops & OPS_ELTWISE else []) \
                + ([REG_OUT] if ops & OPS_RELU else [])
        return need

    def execute_status(self, kind, bound, ltid=0):
        """what execute_st returns before anything is computed (bound: the tensor types that are bound). Up to
        ERR_FUSEBN_UNSUPPORTED_FUSION the reference's order (with a scratch bound there); the rest is this engine's own."""
        d = self.d
        if kind not in (FWD, BWD):
            return ERR_INVALID_KIND
        if d["buffer_format"] != FMT_LIBXSMM:
            return ERR_INVALID_FORMAT_FUSEDBN
        if any(t not in bound for t in self.needed(kind)):
            return ERR_DATA_NOT_BOUND
        if d["fuse_order"] != 0:
            return ERR_FUSEBN_UNSUPPORTED_ORDER
        if d["fuse_ops"] not in FUSE_COMBINATIONS:
            return ERR_FUSEBN_UNSUPPORTED_FUSION
        if ltid < 0 or d["threads"] < 1:
            return ERR_GENERAL
        if not self.runnable():
            return ERR_GENERAL
        if min(d["N"], d["H"], d["W"], d["u"], d["v"]) < 1 or min(d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]) < 0 \
                or d["H"] % d["u"] or d["W"] % d["v"] or d["H"] * d["W"] >= 1 << 27:
            return ERR_GENERAL
        return SUCCESS

    # [block][16]
    def chan_shape(self):
        return (self.blocksifm, 16)

    def shape(self, key):
        if key in ("x", "add", "din", "dadd"):
            return self.in_shape()
        return self.out_shape() if key in ("out", "dout") else self.chan_shape()


ALPHABET = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0], dtype=np.float32)


# ---- inputs: seeded, in the tensors' own layout (physical padding included: it is never read) -----------------------------------
def inputs(name, d):
    """dict of the seeded tensors of a case: x, add, dout in the element type; gamma, beta in fp32; with BNSCALE the statistics
    (mean, rstd) and, for BWD, dgamma and dbeta, which the passes then only read"""
    h = Handle(d)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    t = {}
    if name.endswith("_t"):
        t["x"], t["add"], t["dout"] = (ALPHABET[rng.integers(0, 7, size=s)] for s in (h.in_shape(), h.in_shape(), h.out_shape()))
        t["gamma"] = ALPHABET[rng.integers(0, 7, size=h.chan_shape())]
        t["beta"] = ALPHABET[rng.integers(0, 7, size=h.chan_shape())]
        t["x"][..., 5] = -0.0                        # mean +0.0, x - mean = -0.0, times gamma = 1 and plus beta = -0.0: the output is -0.0
        t["gamma"][:, 5], t["beta"][:, 5] = 1.0, -0.0
    else:
        t["x"], t["add"], t["dout"] = (rng.standard_normal(s).astype(np.float32) for s in (h.in_shape(), h.in_shape(), h.out_shape()))
        t["x"] = (t["x"] * np.float32(1.5) + np.float32(0.75)).astype(np.float32)
        t["gamma"] = (rng.standard_normal(h.chan_shape()) + 1.0).astype(np.float32)
        t["beta"] = rng.standard_normal(h.chan_shape()).astype(np.float32)
    if name.endswith("_c"):
        t["x"][..., 3] = np.float32(0.1)             # a constant that is no sum of few powers of two
        t["x"][..., 9] = np.float32(1.0e4) / 3
    if name.startswith("nonfinite"):
        t["x"][0, 1, 1, 2] = np.nan
        t["x"][1, 3, 2, 7] = np.inf
    if d["fuse_ops"] & OPS_BNSCALE:
        t["mean"] = (rng.standard_normal(h.chan_shape()) * 0.25 + 0.75).astype(np.float32)
        t["rstd"] = (np.abs(rng.standard_normal(h.chan_shape())) + 0.5).astype(np.float32)
        t["dgamma"] = rng.standard_normal(h.chan_shape()).astype(np.float32)
        t["dbeta"] = rng.standard_normal(h.chan_shape()).astype(np.float32)
    if not h.f32:
        for key in ("x", "add", "dout"):
            t[key] = truncate(t[key])
    return {k: np.ascontiguousarray(v) for k, v in t.items()}


# ---- the arithmetic contract -------------------------------------------------------------------------------------------------------
def _nhw(d):
    nhw = np.float32(d["N"] * d["H"] * d["W"])
    return nhw, np.float32(1.0) / nhw


def _by_block(h, a):
    """[block][16] channel values as [item][1][1][16]"""
    return np.tile(a, (h.d["N"], 1))[:, None, None, :]


WRONG = ("statistics over the strided pixels", "nhw as the strided count", "block off by one under the wrap", "add at output coordinates",
         "relu in bwd by dout")  # what forward / backward (wrong=...) can get wrong on purpose


def touched_blocks(h, ltid, wrong=None):
    """the channel blocks of the items of logical thread ltid's share: the share computes the statistics of these, over all images.
    wrong: as the engine derives them (a run from b0 % blocks on that may wrap, or all blocks once the share is as long as an
    image), with the block after the wrap off by one"""
    b0, b1 = h.share(ltid)
    blocks = h.blocksifm
    if wrong != "block off by one under the wrap":
        return sorted({item % blocks for item in range(b0, b1)})
    if b1 - b0 >= blocks:
        return list(range(blocks))
    return [fm if fm < blocks else (fm + 1) % blocks for fm in (b0 % blocks + j for j in range(b1 - b0))]


def _share(h, ltid, wrong):
    """(the items [b0, b1) a pass applies to, the channel blocks whose statistics it computes); ltid None: everything"""
    if ltid is None:
        return (0, h.work()), list(range(h.blocksifm))
    return h.share(ltid), touched_blocks(h, ltid, wrong)


def forward(h, t, fused=False, ltid=None, wrong=None):
    """FWD on the dict of tensors t, in place: the interior of out is written and, with OPS_BN, mean, rstd and var.
    fused=True: sumsq += x * x and ... * rstd + beta as one rounding each (the form the reference's build does not have; for the
    test that tells them apart). ltid: the share of that logical thread only -- out of its items, and the statistics of the
    channel blocks those items belong to (over all images; the bits are those of one thread). wrong: one of WRONG, a mistake made
    on purpose (for tests/test_bn_sweep_cpu.py, which shows that its float64 comparison rejects each of them)."""
    d = h.d
    ops = d["fuse_ops"]
    iph, ipw, oph, opw, H, W = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"], d["H"], d["W"]
    xin = as_f32(h, t["x"])[:, iph:iph + H, ipw:ipw + W, :]
    nhw, recp = _nhw(d)
    (b0, b1), blocks = _share(h, ltid, wrong)
    with np.errstate(all="ignore"):
        if ops & OPS_BN and blocks:
            over = xin[:, ::d["u"], ::d["v"], :] if wrong == "statistics over the strided pixels" else xin
            s = np.zeros((h.work(), 16), dtype=np.float32)
            sq = np.zeros((h.work(), 16), dtype=np.float32)
            for hi in range(over.shape[1]):           # every pixel, hi ascending, then wi ascending
                for wi in range(over.shape[2]):
                    v = over[:, hi, wi, :]
                    s = s + v
                    sq = fma(v, v, sq) if fused else sq + v * v
            s, sq = s.reshape(d["N"], h.blocksifm, 16), sq.reshape(d["N"], h.blocksifm, 16)
            ts = np.zeros(h.chan_shape(), dtype=np.float32)
            tq = np.zeros(h.chan_shape(), dtype=np.float32)
            for img in range(d["N"]):     # the images in order
                ts = ts + s[img]
                tq = tq + sq[img]
            mean = recp * ts
            var = recp * tq - mean * mean
            rstd = (1.0 / np.sqrt(var.astype(np.float64) + np.float64(np.float32(1e-7)))).astype(np.float32)
            t["mean"][blocks], t["rstd"][blocks], t["var"][blocks] = mean[blocks], rstd[blocks], var[blocks]
        xs = xin[:, ::d["u"], ::d["v"], :]
        gamma, beta, mean, rstd = (_by_block(h, t[k]) for k in ("gamma", "beta", "mean", "rstd"))
        part = gamma * (xs - mean)
        o = fma(part, rstd, beta) if fused else part * rstd + beta
        if ops & OPS_ELTWISE:
            if wrong == "add at output coordinates":
                o = o + as_f32(h, t["add"])[:, iph:iph + h.ofh, ipw:ipw + h.ofw, :]
            else:
                o = o + as_f32(h, t["add"])[:, iph:iph + H:d["u"], ipw:ipw + W:d["v"], :]
        if ops & OPS_RELU:
            o = np.where(o < np.float32(0.0), np.float32(0.0), o)
    t["out"][b0:b1, oph:oph + h.ofh, opw:opw + h.ofw, :] = stored(h, o)[b0:b1]


def backward(h, t, ltid=None, wrong=None):
    """BWD on the dict of tensors t, in place: the strided pixels of din and, with OPS_BN, dgamma, dbeta, the RELU select
    stored back into dout and the strided pixels of dadd. ltid: the share of that logical thread only -- din of its items; dgamma
    and dbeta of the channel blocks those items belong to, and the select and dadd of those blocks' items in all images. wrong:
    as in forward."""
    d = h.d
    ops = d["fuse_ops"]
    iph, ipw, oph, opw, H, W, u, v = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"], d["H"], d["W"], d["u"], d["v"]
    xs = as_f32(h, t["x"])[:, iph:iph + H:u, ipw:ipw + W:v, :]
    nhw, recp = _nhw(d)
    if wrong == "nhw as the strided count":
        nhw = np.float32(d["N"] * h.ofh * h.ofw)
        recp = np.float32(1.0) / nhw
    (b0, b1), blocks = _share(h, ltid, wrong)
    gamma, mean, rstd = (_by_block(h, t[k]) for k in ("gamma", "mean", "rstd"))
    inner = (slice(None), slice(oph, oph + h.ofh), slice(opw, opw + h.ofw), slice(None))
    strided = (slice(None), slice(iph, iph + H, u), slice(ipw, ipw + W, v), slice(None))
    with np.errstate(all="ignore"):
        if ops & OPS_BN and blocks:
            mine = np.isin(np.arange(h.work()) % h.blocksifm, blocks)[:, None, None, None]  # the items of the touched blocks
            if ops & OPS_RELU:   # (a -0.0 output counts as zero; the element's bits are kept otherwise)
                zero = as_f32(h, t["out"])[inner] == np.float32(0.0)
                if wrong == "relu in bwd by dout":
                    zero = as_f32(h, t["dout"])[inner] <= np.float32(0.0)
                t["dout"][inner] = np.where(zero & mine, np.zeros((), dtype=t["dout"].dtype), t["dout"][inner])
            if ops & OPS_ELTWISE:
                t["dadd"][strided] = np.where(mine, t["dout"][inner], t["dadd"][strided])
            g = as_f32(h, t["dout"])[inner]
            dg = np.zeros((h.work(), 16), dtype=np.float32)
            db = np.zeros((h.work(), 16), dtype=np.float32)
            m2, r2 = mean[:, 0, 0, :], rstd[:, 0, 0, :]
            for ho in range(h.ofh):
                for wo in range(h.ofw):
                    dg = dg + (xs[:, ho, wo, :] - m2) * g[:, ho, wo, :] * r2
                    db = db + g[:, ho, wo, :]
            dg, db = dg.reshape(d["N"], h.blocksifm, 16), db.reshape(d["N"], h.blocksifm, 16)
            tg = np.zeros(h.chan_shape(), dtype=np.float32)
            tb = np.zeros(h.chan_shape(), dtype=np.float32)
            for img in range(d["N"]):
                tg = tg + dg[img]
                tb = tb + db[img]
            t["dgamma"][blocks], t["dbeta"][blocks] = tg[blocks], tb[blocks]
        g = as_f32(h, t["dout"])[inner]
        dgamma, dbeta = _by_block(h, t["dgamma"]), _by_block(h, t["dbeta"])
        din = gamma * rstd * recp * (nhw * g - (dbeta + (xs - mean) * dgamma * rstd))
    t["din"][strided][b0:b1] = stored(h, din)[b0:b1]


def filled(shape, dtype):
    a = np.zeros(shape, dtype=dtype)
    a.view(np.uint8)[...] = 0xff
    return a


def expected(name, d, fused=False, bwd=True):
    """dict of all thirteen tensors of a case after FWD and BWD on destinations pre-filled with ones bits (NaN / 0xffff);
    dout_in: doutput as it was seeded (BWD with RELU rewrites dout); seeded: the keys of the seeded tensors. bwd=False: FWD only."""
    h = Handle(d)
    t = inputs(name, d)
    seeded = tuple(t)
    for key in KEYS:
        if key not in t:
            t[key] = filled(h.shape(key), elem_dtype(h) if key in ("out", "din", "dadd") else np.float32)
    t["dout_in"] = t["dout"].copy()
    t["seeded"] = seeded
    forward(h, t, fused)
    if bwd:
        backward(h, t)
    return t


def inputs_of(t, d=None):
    """the seeded tensors of expected()'s dict as they were before the passes"""
    return {k: (t["dout_in"] if k == "dout" else t[k]) for k in t["seeded"]}


def written(d, kind):
    """the keys of the tensors a pass writes"""
    ops = d["fuse_ops"]
    if kind == FWD:
        return ["out"] + (["mean", "rstd", "var"] if ops & OPS_BN else [])
    if not ops & OPS_BN:
        return ["din"]
    return ["din", "dgamma", "dbeta"] + (["dout"] if ops & OPS_RELU else []) + (["dadd"] if ops & OPS_ELTWISE else [])


def load_golden():
    return np.load(os.path.join(GOLDEN, "bn.npz"))


# ---- the seeded sweep: descriptors nobody picked --------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 11, 40
SWEEP_CHANNELS = (16, 24, 32, 48, 64, 80)
RELU_NEAR_ZERO = 0.01  # the share of a case's outputs that the float64 comparison may leave out because the ReLU's argument is within its bound of 0
U24, BF16_CUT = 2.0 ** -24, 2.0 ** -7  # the unit roundoff of fp32; what a truncation to bf16 takes off at most, relative


def _draw(rng):
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    u, v = pick(1, 3), pick(1, 3)
    H, W = (u * pick(10, 14), v * pick(10, 14)) if pick(0, 7) == 0 else (u * pick(1, 6), v * pick(1, 6))
    pin, pout = (pick(0, 2), pick(0, 2)), (pick(0, 2), pick(0, 2))
    return desc(H, W, N=pick(1, 5), C=SWEEP_CHANNELS[pick(0, 5)], u=u, v=v, pin=pin, pout=pout, ops=FUSE_COMBINATIONS[pick(0, 7)],
                dt=(F32, BF16)[pick(0, 1)], threads=pick(1, 5))


def sweep_start(name, d):
    """the tensors of a case before the passes: seeded inputs, destinations of ones bits"""
    h = Handle(d)
    t = inputs(name, d)
    seeded = tuple(t)
    for key in KEYS:
        if key not in t:
            t[key] = filled(h.shape(key), elem_dtype(h) if key in ("out", "din", "dadd") else np.float32)
    t["dout_in"] = t["dout"].copy()
    t["seeded"] = seeded
    return t


def sweep_cases_from(seed):
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < SWEEP_CASES:
        d = _draw(rng)
        h = Handle(d)
        if h.status != SUCCESS or SUCCESS != h.execute_status(FWD, BINDABLE) or SUCCESS != h.execute_status(BWD, BINDABLE):
            continue
        name = "sweep_%02d" % len(out)
        want = contract64(h, sweep_start(name, d))
        if not all(np.all(np.isfinite(bound)) for _, bound, _ in want.values()) or np.mean(~want["out"][2]) >= RELU_NEAR_ZERO:
            continue
        out[name] = d
    return out


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """name -> desc: SWEEP_CASES descriptors drawn from SWEEP_SEED. A draw that create or execute_status refuses is left out; one
    whose ReLU leaves RELU_NEAR_ZERO or more of the outputs uncompared, or whose derived bound is not finite (a variance that its own
    bound cannot tell from -epsilon), is replaced by the next draw. tests/test_bn_sweep_cpu.py counts what the set holds; the seed is
    the first from 0 up that passes that census."""
    return sweep_cases_from(SWEEP_SEED)


@functools.lru_cache(maxsize=None)
def sweep_expected(name):
    """all thirteen tensors of a sweep case after FWD and BWD, each pass as the shares of its logical threads in reverse order, with
    dout_in and seeded as expected() has them (computed once, shared: read only)"""
    d = sweep_cases()[name]
    h = Handle(d)
    t = sweep_start(name, d)
    for ltid in reversed(range(d["threads"])):
        forward(h, t, ltid=ltid)
    for ltid in reversed(range(d["threads"])):
        backward(h, t, ltid=ltid)
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def gamma_n(n):
    """n roundings of relative size 2^-24 each, compounded: (1 + 2^-24)^n - 1 <= n * 2^-24 / (1 - n * 2^-24)"""
    n = np.asarray(n, dtype=np.float64)
    return n * U24 / (1 - n * U24)


# An fp32 operation on operands known to within ea and eb: the exact operation moves by what the operands are off, and the rounding of
# the computed result, which lies within that of the exact one, adds 2^-24 of its magnitude. Nothing here is first order only.
def _rounded(v, e):
    return e + U24 * (np.abs(v) + e)


def _add64(a, ea, b, eb):
    return a + b, _rounded(a + b, ea + eb)


def _sub64(a, ea, b, eb):
    return a - b, _rounded(a - b, ea + eb)


def _mul64(a, ea, b, eb):
    return a * b, _rounded(a * b, np.abs(a) * eb + np.abs(b) * ea + ea * eb)


def _sum64(v, e, axes, roundings):
    """an fp32 sum of terms known to within e, none of which passes through more than `roundings` rounded additions"""
    return v.sum(axis=axes), e.sum(axis=axes) + gamma_n(roundings) * (np.abs(v).sum(axis=axes) + e.sum(axis=axes))


def contract64(h, t):
    """key -> (value, bound, compared) for every tensor the two passes write: the layer's contract (include/
    libxsmm_dnn_fusedbatchnorm.h) in float64, written from that text and not from forward / backward above. out,
    dout: interior; din, dadd: the strided pixels; all as [item][ofh][ofw][16]; the channel tensors as [block][16].

    What differs from a textbook batch-norm and is part of the contract:
      * the statistics run over ALL N * H * W pixels, even with a stride; out, din, dadd, dgamma and dbeta cover the strided pixels;
      * din is scaled with the full nhw = N * H * W, not with the number of strided pixels;
      * var = sumsq / nhw - mean^2 (biased), rstd = 1 / sqrt(var + (double)1e-7f);
      * ReLU in BWD is decided by out == 0 (here: by the float64 argument being <= 0), and the selected dout is stored back;
      * with BNSCALE mean, rstd, dgamma and dbeta are given: BWD writes din alone, from dout as it is (no select, no dadd);
      * of C = 24 only the first block of 16 channels exists.

    Bounds: every fp32 operation is followed through as (value, error) by the rules above (_add64, _sub64, _mul64, _sum64), in the
    order kernels/bn.hip documents. sum and sumsq: chains of H * W terms per image from +0.0, then N images from +0.0, so a term
    meets at most H * W + N - 2 roundings (0 + v is exact). mean = fl(recp * sum) with recp = fl(1 / nhw) (nhw < 2^24 is exact).
    var = fl(fl(recp * sumsq) - fl(mean * mean)): the error of either product enters whole, which is the cancellation. rstd: the
    interval var +- e_var is carried through 1 / sqrt(. + eps), plus the final rounding to fp32 (the double arithmetic's 2^-52
    is added as 2^-50). Apply: ((gamma * (x - mean)) * rstd) + beta (+ add). dgamma, dbeta: sums of ((x - mean) * dout) * rstd and
    dout over ofh * ofw + N - 2 roundings. din: ((gamma * rstd) * recp) * (nhw * dout - (dbeta + ((x - mean) * dgamma) * rstd)).
    A bf16 store cuts off below 2^-7 * (|value| + bound), added last.
    compared: False where the float64 ReLU argument lies within its bound of 0, so that the two sides may fall on either side of
    it: in out, and with OPS_BN in dout, dadd and din of the same element; its whole term |dout| and |((x - mean) * dout) * rstd|
    joins the bound of its channel's dbeta and dgamma, and through them that of din."""
    d = h.d
    ops, N, blocks, H, W, u, v = d["fuse_ops"], d["N"], h.blocksifm, d["H"], d["W"], d["u"], d["v"]
    iph, ipw, oph, opw = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"]
    stats, relu, elt = bool(ops & OPS_BN), bool(ops & OPS_RELU), bool(ops & OPS_ELTWISE)
    f64 = lambda a: as_f32(h, a).astype(np.float64)  # noqa: E731
    per_chan = lambda a: a.reshape((N, blocks) + a.shape[1:])  # noqa: E731 ([image][block][row][column][16])
    by_item = lambda a: np.tile(a, (N, 1))[:, None, None, :]  # noqa: E731
    x_all = f64(t["x"])[:, iph:iph + H, ipw:ipw + W, :]
    xs = x_all[:, ::u, ::v, :]
    nhw = float(N * H * W)
    recp, e_recp = 1.0 / nhw, U24 / nhw
    res = {}
    if stats:
        X = per_chan(x_all)
        total, e_total = _sum64(X, np.zeros_like(X), (0, 2, 3), max(H * W + N - 2, 0))
        mean, e_mean = _mul64(recp, e_recp, total, e_total)
        sq, e_sq = _mul64(X, 0.0, X, 0.0)
        sumsq, e_sumsq = _sum64(sq, e_sq, (0, 2, 3), max(H * W + N - 2, 0))
        first, e_first = _mul64(recp, e_recp, sumsq, e_sumsq)
        second, e_second = _mul64(mean, e_mean, mean, e_mean)
        var, e_var = _sub64(first, e_first, second, e_second)
        eps = float(np.float32(1e-7))
        rstd = 1.0 / np.sqrt(var + eps)
        with np.errstate(all="ignore"):
            low = var - e_var + eps
            e_rstd = np.where(low > 0, np.maximum(1.0 / np.sqrt(np.where(low > 0, low, 1.0)) - rstd, rstd - 1.0 / np.sqrt(var + e_var + eps)), np.inf)
        e_rstd = _rounded(rstd, e_rstd + 2.0 ** -50 * rstd)
        yes = np.ones(mean.shape, dtype=bool)
        res["mean"], res["var"], res["rstd"] = (mean, e_mean, yes), (var, e_var, yes), (rstd, e_rstd, yes)
    else:
        mean, rstd = t["mean"].astype(np.float64), t["rstd"].astype(np.float64)
        e_mean, e_rstd = np.zeros_like(mean), np.zeros_like(rstd)
    gam, beta = t["gamma"].astype(np.float64), t["beta"].astype(np.float64)
    cut = (lambda a, e: e) if h.f32 else (lambda a, e: e + BF16_CUT * (np.abs(a) + e))
    # FWD apply
    centred, e_centred = _sub64(xs, 0.0, by_item(mean), by_item(e_mean))
    o, e = _mul64(by_item(gam), 0.0, centred, e_centred)
    o, e = _mul64(o, e, by_item(rstd), by_item(e_rstd))
    o, e = _add64(o, e, by_item(beta), 0.0)
    if elt:
        o, e = _add64(o, e, f64(t["add"])[:, iph:iph + H:u, ipw:ipw + W:v, :], 0.0)
    compared = np.abs(o) > e if relu else np.ones(o.shape, dtype=bool)
    positive = o > 0
    if relu:
        o = np.maximum(o, 0.0)
    res["out"] = (o, cut(o, e), compared)
    # BWD
    raw = f64(t["dout"])[:, oph:oph + h.ofh, opw:opw + h.ofw, :]
    g, settled = raw, np.ones(raw.shape, dtype=bool)
    if stats:
        if relu:
            g, settled = np.where(positive, raw, 0.0), compared
            res["dout"] = (g, np.zeros_like(g), settled)
        if elt:
            res["dadd"] = (g, np.zeros_like(g), settled)
        term, e_term = _mul64(centred, e_centred, raw, 0.0)
        term, e_term = _mul64(term, e_term, by_item(rstd), by_item(e_rstd))
        kept = positive if relu else np.ones(raw.shape, dtype=bool)
        roundings = max(h.ofh * h.ofw + N - 2, 0)
        dgamma, e_dgamma = _sum64(per_chan(np.where(kept, term, 0.0)), per_chan(np.where(kept, e_term, 0.0)), (0, 2, 3), roundings)
        dbeta, e_dbeta = _sum64(per_chan(g), np.zeros_like(per_chan(g)), (0, 2, 3), roundings)
        e_dgamma = e_dgamma + per_chan(np.where(settled, 0.0, np.abs(term) + e_term)).sum(axis=(0, 2, 3))
        e_dbeta = e_dbeta + per_chan(np.where(settled, 0.0, np.abs(raw))).sum(axis=(0, 2, 3))
        yes = np.ones(dgamma.shape, dtype=bool)
        res["dgamma"], res["dbeta"] = (dgamma, e_dgamma, yes), (dbeta, e_dbeta, yes)
    else:
        dgamma, dbeta = t["dgamma"].astype(np.float64), t["dbeta"].astype(np.float64)
        e_dgamma, e_dbeta = np.zeros_like(dgamma), np.zeros_like(dbeta)
    scale, e_scale = _mul64(by_item(gam), 0.0, by_item(rstd), by_item(e_rstd))
    scale, e_scale = _mul64(scale, e_scale, recp, e_recp)
    lead, e_lead = _mul64(nhw, 0.0, g, 0.0)
    part, e_part = _mul64(centred, e_centred, by_item(dgamma), by_item(e_dgamma))
    part, e_part = _mul64(part, e_part, by_item(rstd), by_item(e_rstd))
    part, e_part = _add64(by_item(dbeta), by_item(e_dbeta), part, e_part)
    inner, e_inner = _sub64(lead, e_lead, part, e_part)
    din, e_din = _mul64(scale, e_scale, inner, e_inner)
    res["din"] = (din, cut(din, e_din), settled)
    return res


def interior(h, key, a):
    """the elements of a tensor of sweep_expected() that contract64 computes, in its index order"""
    d = h.d
    if key in ("out", "dout"):
        return as_f32(h, a)[:, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :]
    if key in ("din", "dadd"):
        return as_f32(h, a)[:, d["pad_h_in"]:d["pad_h_in"] + d["H"]:d["u"], d["pad_w_in"]:d["pad_w_in"] + d["W"]:d["v"], :]
    return a
