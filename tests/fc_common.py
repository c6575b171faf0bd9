"""The fully-connected layer restated in numpy: handle rules, datalayouts, scratch formula, blocking and de-blocking, the split
over logical threads, and the expected outputs, which come from the CPU oracle (one orc.smm per pass over the whole reduction
length, fma, beta = 0, on the de-blocked plain matrices). Shared by tests/test_fc_cpu.py, tests/test_fc_gpu.py and
tools/golden/fc_capture.py; the reference's own answers are in tests/golden/fc.npz."""
import functools
import os

import numpy as np

import oracle_binding as orc
import quant_common as qc
from dnn_common import *  # noqa: F401,F403 (re-exported: the tests reach every shared name through this module)
from dnn_common import share

FMT_RSCK, FMT_KCRS, FMT_CKPACKED, FMT_NCPACKED = 8, 16, 64, 128
GRAD_FIL = 12
TENSOR_TYPES = (REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, REG_FIL, GRAD_FIL)
DIM_K, DIM_R, DIM_S = 4, 5, 6
TENSOR_FILTER = 13  # LIBXSMM_DNN_FILTER: what a filter layout's tensor_type says

WARN_N, WARN_C, WARN_K = 90004, 90005, 90006
ERR_CREATE_HANDLE, ERR_UNSUPPORTED_DST_FORMAT, ERR_UNSUPPORTED_SRC_FORMAT, ERR_FUSION, ERR_INVALID_FORMAT_FC = 100001, 100012, 100013, 100031, 100034


def desc(N, C, K, fmt="L", dt="f32", bn=0, bk=0, bc=0, threads=1, fuse=0):
    dts = {"f32": (F32, F32), "bf16": (BF16, F32), "bf16bf16": (BF16, BF16), "f32bf16": (F32, BF16)}[dt]
    fmts = {"L": (FMT_LIBXSMM, FMT_LIBXSMM), "B": (FMT_NCPACKED, FMT_CKPACKED), "nhwc": (FMT_NHWC, FMT_RSCK)}[fmt]
    return dict(N=N, C=C, K=K, bn=bn, bk=bk, bc=bc, threads=threads, datatype_in=dts[0], datatype_out=dts[1], buffer_format=fmts[0],
                filter_format=fmts[1], fuse_ops=fuse)


DESC_FIELDS = ("N", "C", "K", "bn", "bk", "bc", "threads", "datatype_in", "datatype_out", "buffer_format", "filter_format", "fuse_ops")

# the cases of tests/golden/fc.npz; "run": the passes are executed and their outputs stored; "bind": tensor types that are bound
COMPUTE_CASES = {
    "l_5_32_48": desc(5, 32, 48), "l_33_16_1000": desc(33, 16, 1000), "l_70_48_80": desc(70, 48, 80), "l_130_32_144": desc(130, 32, 144),
    "b_6_15_14": desc(6, 15, 14, "B", bn=3, bc=5, bk=7), "b_7_10_9": desc(7, 10, 9, "B", bn=4, bc=4, bk=2),
    "b_64_64_96": desc(64, 64, 96, "B", bn=32, bc=32, bk=32),
    "lb_5_32_48": desc(5, 32, 48, dt="bf16"), "lb_33_16_1000": desc(33, 16, 1000, dt="bf16"),
}
STATUS_CASES = {
    "e_c24": desc(5, 24, 16), "e_bf16bf16": desc(5, 32, 48, dt="bf16bf16"), "e_f32bf16": desc(5, 32, 48, dt="f32bf16"),
    "e_nhwc": desc(5, 32, 48, "nhwc"), "e_unbound": desc(5, 32, 48), "e_fuse": desc(5, 32, 48, fuse=1), "e_b_bf16": desc(6, 15, 14, "B", "bf16", bn=3, bc=5, bk=7),
    "w_n": desc(7, 8, 6, "B", bn=4, bc=4, bk=2), "w_c": desc(8, 10, 6, "B", bn=4, bc=4, bk=2), "w_k": desc(8, 8, 9, "B", bn=4, bc=4, bk=2),
}
UNBOUND = {"e_unbound": (REG_IN,)}  # tensor types left unbound


def all_cases():
    out = dict(COMPUTE_CASES)
    out.update(STATUS_CASES)
    return out


# ---- handle rules (src/libxsmm_dnn_fullyconnected.c:46-136) ---------------------------------------------------------------------
WRONG = ("block factors swapped", "non-dividing block kept")  # what Handle(wrong=...) can get wrong on purpose


class Handle:
    def __init__(self, d, wrong=None):
        """wrong: one of WRONG, a mistake made on purpose (for tests/test_fc_sweep_cpu.py, which shows that its float64 comparison
        rejects each of them)"""
        self.d = d
        self.status = SUCCESS
        self.ok = False
        pair = (d["datatype_in"], d["datatype_out"])
        if pair not in ((BF16, BF16), (F32, F32), (BF16, F32)):
            self.status = ERR_UNSUPPORTED_DATATYPE
            return
        self.f32, self.mixed, self.lowp = pair == (F32, F32), pair == (BF16, F32), pair == (BF16, BF16)
        self.packed = d["buffer_format"] == FMT_NCPACKED and d["filter_format"] == FMT_CKPACKED
        self.custom = d["buffer_format"] == FMT_LIBXSMM and d["filter_format"] == FMT_LIBXSMM
        N, C, K = d["N"], d["C"], d["K"]
        self.bn = self.bc = self.bk = 0
        self.ifmblock = self.ofmblock = self.fm_lp_block = self.blocksifm = self.blocksofm = 0
        if self.packed:
            self.bn, self.bc, self.bk = d["bn"], d["bc"], d["bk"]
            if wrong == "block factors swapped":
                self.bc, self.bk = self.bk, self.bc
            # (a block of zero or below divides nothing: the reference would trap on the modulo, this engine falls back as for any misfit)
            if (self.bn <= 0 or N % self.bn) and wrong != "non-dividing block kept":
                self.bn, self.status = N, WARN_N
            if (self.bc <= 0 or C % self.bc) and wrong != "non-dividing block kept":
                self.bc, self.status = C, WARN_C
            if (self.bk <= 0 or K % self.bk) and wrong != "non-dividing block kept":
                self.bk, self.status = K, WARN_K
        else:
            if C % 16 == 0 and K % 16 == 0:
                self.ifmblock, self.fm_lp_block = (8, 2) if self.lowp else (16, 1)
                self.ofmblock = 16
            elif C % 16 == 0 and K == 1000:
                self.ifmblock, self.fm_lp_block, self.ofmblock = 16, 1, 10
            else:
                self.status = ERR_CREATE_HANDLE
                return
            self.blocksifm = C // (self.ifmblock * self.fm_lp_block if self.lowp else self.ifmblock)
            self.blocksofm = K // self.ofmblock
        if self.mixed:
            self.scratch_size = 4 * (C * N + C * K)
        else:
            self.scratch_size = 4 * max((C + K) * N, C * K)
        self.ok = True

    def scratch(self):
        return self.scratch_size + 64

    def layout(self, t):
        """(status, None) or (0, dict) as libxsmm_dnn_fullyconnected_create_tensor_datalayout (:155-492)"""
        d = self.d
        N, C, K = d["N"], d["C"], d["K"]
        inp, out, fil = t in (REG_IN, GRAD_IN), t in (REG_OUT, GRAD_OUT), t in (REG_FIL, GRAD_FIL)

        if inp or out:
            fmt = d["buffer_format"]
            if fmt & FMT_LIBXSMM:
                act5 = (DIM_C, DIM_W, DIM_H, DIM_C, DIM_N)
                if self.f32 or (self.mixed and out):
                    sizes = (self.ifmblock, 1, 1, self.blocksifm, N) if inp else (self.ofmblock, 1, 1, self.blocksofm, N)
                    return made(act5, sizes, F32 if self.f32 else d["datatype_out"], fmt)
                if self.mixed:
                    return made((DIM_C, DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), (self.fm_lp_block, self.ifmblock, 1, 1, self.blocksifm, N), d["datatype_in"], fmt)
                return ERR_UNSUPPORTED_DATATYPE, None
            if fmt & FMT_NHWC:
                return made((DIM_C, DIM_W, DIM_H, DIM_N), (C, 1, 1, N), d["datatype_in"], fmt)
            if fmt & FMT_NCPACKED:
                if not self.f32:
                    return ERR_UNSUPPORTED_DATATYPE, None
                if inp:
                    return made((DIM_C, DIM_N, DIM_C, DIM_N), (self.bc, self.bn, C // self.bc, N // self.bn), F32, fmt)
                return made((DIM_K, DIM_N, DIM_K, DIM_N), (self.bk, self.bn, K // self.bk, N // self.bn), F32, fmt)
            return ERR_INVALID_FORMAT_GENERAL, None
        if fil:
            fmt = d["filter_format"]
            if fmt & FMT_LIBXSMM:
                if self.f32:
                    return made((DIM_K, DIM_C, DIM_S, DIM_R, DIM_C, DIM_K), (self.ofmblock, self.ifmblock, 1, 1, self.blocksifm, self.blocksofm), d["datatype_in"], fmt, TENSOR_FILTER)
                return made((DIM_C, DIM_K, DIM_C, DIM_S, DIM_R, DIM_C, DIM_K), (self.fm_lp_block, self.ofmblock, self.ifmblock, 1, 1, self.blocksifm, self.blocksofm),
                            BF16, fmt, TENSOR_FILTER)
            if fmt & FMT_RSCK:
                return made((DIM_K, DIM_C, DIM_S, DIM_R), (self.ofmblock * self.blocksofm, self.ifmblock * self.blocksifm, 1, 1), d["datatype_in"], fmt, TENSOR_FILTER)
            if fmt & FMT_CKPACKED:
                if not self.f32:
                    return ERR_UNSUPPORTED_DATATYPE, None
                return made((DIM_K, DIM_C, DIM_C, DIM_K), (self.bk, self.bc, C // self.bc, K // self.bk), F32, fmt, TENSOR_FILTER)
            return ERR_INVALID_FORMAT_GENERAL, None
        return ERR_UNKNOWN_TENSOR_TYPE, None

    def execute_status(self, kind, bound, scratch_bound=True):
        """what execute_st returns before anything is computed (bound: the tensor types that are bound)"""
        if kind not in (FWD, BWD, UPD):
            return ERR_INVALID_KIND
        if not (self.custom or self.packed):
            return ERR_INVALID_FORMAT_FC
        need = {FWD: (REG_FIL, REG_IN, REG_OUT), BWD: (REG_FIL, GRAD_OUT, GRAD_IN), UPD: (GRAD_OUT, REG_IN, GRAD_FIL)}[kind]
        if any(t not in bound for t in need) or (kind != FWD and not scratch_bound):
            return ERR_DATA_NOT_BOUND
        if not (self.f32 or (self.mixed and self.custom)):
            return ERR_UNSUPPORTED_DATATYPE
        if self.d["fuse_ops"]:
            return ERR_FUSION
        return SUCCESS

    # block sizes of n, c, k as the executed formats use them
    def blocks(self):
        if self.packed:
            return self.bn, self.bc, self.bk
        return 1, self.ifmblock * self.fm_lp_block, self.ofmblock

    def work(self, kind):
        bn, bc, bk = self.blocks()
        N, C, K = self.d["N"], self.d["C"], self.d["K"]
        if self.packed:
            return {FWD: (K // bk) * (N // bn), BWD: (C // bc) * (N // bn), UPD: (C // bc) * (K // bk)}[kind]
        return {FWD: K // bk, BWD: C // bc, UPD: (C // bc) * (K // bk)}[kind]

    def share(self, kind, ltid):
        return share(self.work(kind), self.d["threads"], ltid)


# ---- blocking: plain [N][C], [N][K], [K][C] <-> the tensors' layouts ---------------------------------------------------------------
def block_act(h, a, feat):
    """a: plain [N][F]; feat 'c' or 'k'"""
    bn, bc, bk = h.blocks()
    b = bc if feat == "c" else bk
    N, F = a.shape
    if h.packed:
        return np.ascontiguousarray(a.reshape(N // bn, bn, F // b, b).transpose(0, 2, 1, 3)).reshape(-1)
    return np.ascontiguousarray(a).reshape(-1)


def unblock_act(h, flat, feat):
    bn, bc, bk = h.blocks()
    N, F = h.d["N"], h.d["C"] if feat == "c" else h.d["K"]
    b = bc if feat == "c" else bk
    if h.packed:
        return np.ascontiguousarray(flat.reshape(N // bn, F // b, bn, b).transpose(0, 2, 1, 3)).reshape(N, F)
    return flat.reshape(N, F).copy()


def block_fil(h, w):
    """w: plain [K][C] -> [K/bk][C/bc][bc][bk]"""
    _, bc, bk = h.blocks()
    K, C = w.shape
    return np.ascontiguousarray(w.reshape(K // bk, bk, C // bc, bc).transpose(0, 2, 3, 1)).reshape(-1)


def unblock_fil(h, flat):
    _, bc, bk = h.blocks()
    K, C = h.d["K"], h.d["C"]
    return np.ascontiguousarray(flat.reshape(K // bk, C // bc, bc, bk).transpose(0, 3, 1, 2)).reshape(K, C)


# ---- inputs: seeded, bf16-representable (so that the 16-bit and the fp32 cases share them and the stored files stay small) ----------
def bf16_values(rng, shape):
    x = (rng.random(shape) - 0.5).astype(np.float32) * 2
    return qc.bf16_widen(qc.bf16_rne(x)).reshape(shape)


def plain_inputs(name, d):
    """(x [N][C], w [K][C], dy [N][K]) as fp32 arrays whose values are bf16 numbers; the 16-bit cases carry exact ties"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    rng = np.random.default_rng(seed)
    N, C, K = d["N"], d["C"], d["K"]
    x, w, dy = bf16_values(rng, (N, C)), bf16_values(rng, (K, C)), bf16_values(rng, (N, K))
    if d["datatype_in"] == BF16 and N >= 3 and K >= 3 and C >= 4:
        t = np.float32(2.0 ** -8)
        # dx[1][0] = 1 + 2^-8 and dx[1][1] = 1 + 3 * 2^-8: halfway between two bf16 numbers (ties to even: down, up)
        dy[1, :] = 0
        dy[1, 0] = dy[1, 1] = 1
        w[0, 0], w[1, 0], w[0, 1], w[1, 1] = 1, t, 1, 3 * t
        # dw[2][3] = 1 + 2^-8
        dy[:, 2] = 0
        dy[0, 2], dy[2, 2] = 1, t
        x[0, 3] = x[2, 3] = 1
    return x, w, dy


def expected(h, x, w, dy):
    """plain (y [N][K], dx [N][C], dw [K][C]) from the oracle: fma chains over the whole reduction length, beta = 0. The 16-bit
    case rounds dx and dw to bf16 (returned as uint16)."""
    N, C, K = h.d["N"], h.d["C"], h.d["K"]
    flags = orc.FLAG_BETA_0
    # column-major m x n x k: y^T (K x N) = w^T... every matrix below is handed over as the flat column-major image the oracle wants
    y = np.full(N * K, np.nan, dtype=np.float32)      # y as K x N column-major == [N][K] row-major
    a = np.ascontiguousarray(w.T).reshape(-1)         # A: K x C column-major: A(k, c) at k + K * c == w.T [C][K] row-major
    orc.smm(orc.FMA, flags, K, N, C, K, C, K, a, np.ascontiguousarray(x).reshape(-1), y)
    dx = np.full(N * C, np.nan, dtype=np.float32)     # dx as C x N column-major; A(c, k) at c + C * k == w [K][C] row-major
    orc.smm(orc.FMA, flags, C, N, K, C, K, C, np.ascontiguousarray(w).reshape(-1), np.ascontiguousarray(dy).reshape(-1), dx)
    dw = np.full(K * C, np.nan, dtype=np.float32)     # dw as K x C column-major (== dw.T row-major); A(k, n) = dy [N][K] row-major; B(n, c) at n + N * c
    orc.smm(orc.FMA, flags, K, C, N, K, N, K, np.ascontiguousarray(dy).reshape(-1), np.ascontiguousarray(x.T).reshape(-1), dw)
    y, dx, dw = y.reshape(N, K), dx.reshape(N, C), np.ascontiguousarray(dw.reshape(C, K).T)
    if h.mixed:
        return y, qc.bf16_rne(dx).reshape(N, C), qc.bf16_rne(dw).reshape(K, C)
    return y, dx, dw


def tensors(h, x, w, dy):
    """the six tensors' contents in their own layouts and element types (outputs: the expectation)"""
    y, dx, dw = expected(h, x, w, dy)
    lo = (lambda a: qc.bf16_rne(a).reshape(a.shape)) if h.mixed else (lambda a: a)  # (exact: the values are bf16 numbers)
    return {REG_IN: block_act(h, lo(x), "c"), REG_FIL: block_fil(h, lo(w)), GRAD_OUT: block_act(h, dy, "k"),
            REG_OUT: block_act(h, y, "k"), GRAD_IN: block_act(h, dx, "c"), GRAD_FIL: block_fil(h, dw)}


def dtype_of(h, t):
    return np.uint16 if (h.mixed and t in (REG_IN, GRAD_IN, REG_FIL, GRAD_FIL)) else np.float32


def load_golden():
    return np.load(os.path.join(GOLDEN, "fc.npz"))


# ---- the seeded sweep: descriptors nobody picked --------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 10, 32
SWEEP_C, SWEEP_K = (16, 32, 48, 64), (16, 32, 48, 80, 1000)
U24, BF16_RNE = 2.0 ** -24, 2.0 ** -8  # the unit roundoff of fp32; that of a round-to-nearest-even store to bf16 (8 significant bits: half of a spacing of 2^-7)


def _draw(rng, packed):
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    N = pick(65, 150) if pick(0, 5) == 0 else pick(1, 40)
    if packed:
        C, K = pick(1, 80), pick(1, 80)
        blk = lambda n: int(rng.choice([0, 1, n] + [q for q in range(2, n + 1) if n % q == 0] + [n + 1, 7]))  # noqa: E731 (as rnn_common.sweep_cases)
        return desc(N, C, K, "B", bn=blk(N), bc=blk(C), bk=blk(K), threads=pick(1, 5))
    return desc(N, SWEEP_C[pick(0, 3)], SWEEP_K[pick(0, 4)], "L", dt=("f32", "bf16")[pick(0, 1)], threads=pick(1, 5))


def sweep_cases_from(seed):
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < SWEEP_CASES:
        d = _draw(rng, len(out) % 2 == 0)   # the packed format and the custom one in turn
        h = Handle(d)
        if not h.ok or any(SUCCESS != h.execute_status(kind, TENSOR_TYPES) for kind in (FWD, BWD, UPD)):
            continue                        # (a handle that answers WARN_* is kept and runs)
        out["sweep_%02d" % len(out)] = d
    return out


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """name -> desc: SWEEP_CASES descriptors drawn from SWEEP_SEED, half in the packed format in fp32 with block factors drawn from
    divisors and non-divisors (0 among them), half in the custom format in fp32 or bf16-in / fp32-out. A draw that create or
    execute_status refuses is left out. tests/test_fc_sweep_cpu.py counts what the set holds; the seed is the first from 0 up that
    passes that census."""
    return sweep_cases_from(SWEEP_SEED)


@functools.lru_cache(maxsize=None)
def sweep_expected(name):
    """(handle restatement, plain inputs, the six tensors' expected contents) of a sweep case (computed once, shared: read only)"""
    d = sweep_cases()[name]
    h = Handle(d)
    x, w, dy = plain_inputs(name, d)
    want = tensors(h, x, w, dy)
    for a in (x, w, dy) + tuple(want.values()):
        a.setflags(write=False)
    return h, (x, w, dy), want


def contract64(d, x, w, dy):
    """key -> (value, bound, compared) for y [N][K], dx [N][C] and dw [K][C]: the layer's contract (include/
    libxsmm_dnn_fullyconnected.h) as three float64 matrix products of the plain operands, y = x w^T, dx = dy w,
    dw = dy^T x. Bounds: each element is a chain of n fused multiply-adds from +0.0 over the whole reduction length (n = C, K, N),
    n roundings of relative size 2^-24 compounded: n * 2^-24 / (1 - n * 2^-24) * sum|a * b|. With bf16 inputs the products are
    exact in fp32 and the bound still holds; dx and dw are then stored to bf16 by round-to-nearest-even, half a unit of its 8
    significant bits: 2^-8 * (|value| + bound) more. compared is all True: the layer has no decision."""
    gam = lambda n: n * U24 / (1 - n * U24)  # noqa: E731
    x, w, dy = (np.asarray(a, dtype=np.float64) for a in (x, w, dy))
    res = {"y": (x @ w.T, gam(d["C"]) * (np.abs(x) @ np.abs(w).T)), "dx": (dy @ w, gam(d["K"]) * (np.abs(dy) @ np.abs(w))),
           "dw": (dy.T @ x, gam(d["N"]) * (np.abs(dy).T @ np.abs(x)))}
    if d["datatype_in"] == BF16:
        for key in ("dx", "dw"):
            value, bound = res[key]
            res[key] = (value, bound + BF16_RNE * (np.abs(value) + bound))
    return {key: (value, bound, np.ones(value.shape, dtype=bool)) for key, (value, bound) in res.items()}
