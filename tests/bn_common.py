"""The fused batch-norm layer restated in numpy: handle rules, datalayouts, scratch formula, the statuses of execute_st, the split
over logical threads, seeded inputs, and the arithmetic contract of include/libxsmm_dnn_fusedbatchnorm.h (FWD and BWD, the eight
fuse combinations, fp32 and bf16) as plain array code. Shared by tests/test_bn_cpu.py, tests/test_bn_gpu.py and
tools/golden/bn_capture.py; the reference's own answers are in tests/golden/bn.npz and tests/test_bn_cpu.py holds this file
against them bit for bit."""
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


def forward(h, t, fused=False):
    """FWD on the dict of tensors t, in place: the interior of out is written and, with OPS_BN, mean, rstd and var.
    fused=True: sumsq += x * x and ... * rstd + beta as one rounding each (the form the reference's build does not have; for the
    test that tells them apart)."""
    d = h.d
    ops = d["fuse_ops"]
    iph, ipw, oph, opw, H, W = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"], d["H"], d["W"]
    xin = as_f32(h, t["x"])[:, iph:iph + H, ipw:ipw + W, :]
    nhw, recp = _nhw(d)
    with np.errstate(all="ignore"):
        if ops & OPS_BN:
            s = np.zeros((h.work(), 16), dtype=np.float32)
            sq = np.zeros((h.work(), 16), dtype=np.float32)
            for hi in range(H):           # every pixel, hi ascending, then wi ascending
                for wi in range(W):
                    v = xin[:, hi, wi, :]
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
            t["mean"][...], t["rstd"][...], t["var"][...] = mean, rstd, var
        xs = xin[:, ::d["u"], ::d["v"], :]
        gamma, beta, mean, rstd = (_by_block(h, t[k]) for k in ("gamma", "beta", "mean", "rstd"))
        part = gamma * (xs - mean)
        o = fma(part, rstd, beta) if fused else part * rstd + beta
        if ops & OPS_ELTWISE:
            o = o + as_f32(h, t["add"])[:, iph:iph + H:d["u"], ipw:ipw + W:d["v"], :]
        if ops & OPS_RELU:
            o = np.where(o < np.float32(0.0), np.float32(0.0), o)
    t["out"][:, oph:oph + h.ofh, opw:opw + h.ofw, :] = stored(h, o)


def backward(h, t):
    """BWD on the dict of tensors t, in place: the strided pixels of din and, with OPS_BN, dgamma, dbeta, the RELU select
    stored back into dout and the strided pixels of dadd"""
    d = h.d
    ops = d["fuse_ops"]
    iph, ipw, oph, opw, H, W, u, v = d["pad_h_in"], d["pad_w_in"], d["pad_h_out"], d["pad_w_out"], d["H"], d["W"], d["u"], d["v"]
    xs = as_f32(h, t["x"])[:, iph:iph + H:u, ipw:ipw + W:v, :]
    nhw, recp = _nhw(d)
    gamma, mean, rstd = (_by_block(h, t[k]) for k in ("gamma", "mean", "rstd"))
    inner = (slice(None), slice(oph, oph + h.ofh), slice(opw, opw + h.ofw), slice(None))
    strided = (slice(None), slice(iph, iph + H, u), slice(ipw, ipw + W, v), slice(None))
    with np.errstate(all="ignore"):
        if ops & OPS_BN:
            if ops & OPS_RELU:   # (a -0.0 output counts as zero; the element's bits are kept otherwise)
                zero = as_f32(h, t["out"])[inner] == np.float32(0.0)
                t["dout"][inner] = np.where(zero, np.zeros((), dtype=t["dout"].dtype), t["dout"][inner])
            if ops & OPS_ELTWISE:
                t["dadd"][strided] = t["dout"][inner]
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
            t["dgamma"][...], t["dbeta"][...] = tg, tb
        g = as_f32(h, t["dout"])[inner]
        dgamma, dbeta = _by_block(h, t["dgamma"]), _by_block(h, t["dbeta"])
        din = gamma * rstd * recp * (nhw * g - (dbeta + (xs - mean) * dgamma * rstd))
    t["din"][strided] = stored(h, din)


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
