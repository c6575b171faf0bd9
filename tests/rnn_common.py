"""The RNN cell layer restated for the tests (include/libxsmm_dnn_rnncell.h): the handle rules, layouts and sizes of
src/libxsmm_dnn_rnncell.c, and the forward pass of the three generic templates
src/template/libxsmm_dnn_rnncell_st_{rnn,lstm,gru}_fwd_nc_ck_generic.tpl.c loop for loop -- every SMM or batch-reduce SMM call of a
template is a call of the CPU oracle's SMM (tests/oracle_binding.py), the filters are reformatted into blocks first as the templates
do, and the elementwise loops of src/libxsmm_dnn_elementwise.c are evaluated element by element with the platform libm
(math.exp, math.tanh). tests/test_rnn_cpu.py holds all of it against the reference's captured outputs (tests/golden/rnn.npz,
written by tools/golden/rnn_capture.py)."""
import functools
import math
import zlib

import numpy as np

import oracle_binding as orc
from dnn_common import (GOLDEN, F32, BF16, FWD, BWD, UPD, BWDUPD, ALL, SUCCESS, ERR_GENERAL, ERR_UNSUPPORTED_DATATYPE, ERR_INVALID_HANDLE,  # noqa: F401
                        ERR_DATA_NOT_BOUND, ERR_MISMATCH_TENSOR, ERR_INVALID_HANDLE_TENSOR, ERR_INVALID_KIND, ERR_INVALID_FORMAT_GENERAL,
                        ERR_SCRATCH_NOT_ALLOCED, ERR_UNKNOWN_TENSOR_TYPE, made, layout_size, share, fma, crc, check_mixed_residency)

FMT_CK, FMT_CKPACKED, FMT_NCPACKED, FMT_NC = 32, 64, 128, 256
RELU, SIGMOID, TANH, LSTM, GRU = 0, 1, 2, 3, 4
CELL_NAMES = {RELU: "relu", SIGMOID: "sigmoid", TANH: "tanh", LSTM: "lstm", GRU: "gru"}
WARN_N, WARN_C, WARN_K = 90001, 90002, 90003
ERR_TIME_STEPS_TOO_SMALL, ERR_INVALID_RNN_TYPE, ERR_RNN_INVALID_SEQ_LEN = 100027, 100035, 100036
DIM_N, DIM_C, DIM_K, DIM_T, DIM_X = 0, 3, 4, 7, 8
TT_ACTIVATION, TT_FILTER, TT_CHANNEL_SCALAR = 9, 13, 26
# the 23 tensor types in the order of the enumeration (LIBXSMM_DNN_RNN_REGULAR_INPUT = 33)
(X, CSP, HP, W, R, WT, RT, B, CS, H, DX, DCSP, DHP, DW, DR, DB, DCS, DH, GI, GF, GO, GCI, GCO) = range(33, 56)
RNN_TYPES = tuple(range(33, 56))
DESC_FIELDS = ("N", "C", "K", "max_T", "cell", "bn", "bc", "bk", "threads", "datatype_in", "datatype_out", "buffer_format", "filter_format")
OUTPUTS = ("h", "cs", "i", "f", "o", "ci", "co", "z")
OUT_TYPE = {"h": H, "cs": CS, "i": GI, "f": GF, "o": GO, "ci": GCI, "co": GCO}
INPUTS = ("x", "hp", "csp", "w", "r", "b")
IN_TYPE = {"x": X, "hp": HP, "csp": CSP, "w": W, "r": R, "b": B}


def desc(N, C, K, max_T, cell, bn=0, bc=0, bk=0, threads=1, dt=F32, dt_out=None, bfmt=FMT_NC, ffmt=FMT_CK, seq=-1, forget_bias=None, seed=0):
    return dict(N=N, C=C, K=K, max_T=max_T, cell=cell, bn=bn, bc=bc, bk=bk, threads=threads, datatype_in=dt,
                datatype_out=dt if dt_out is None else dt_out, buffer_format=bfmt, filter_format=ffmt, seq=seq, forget_bias=forget_bias, seed=seed)


def gates(cell):
    return 4 if cell == LSTM else (3 if cell == GRU else 1)


def written(cell):
    """the tensors FWD of a cell writes"""
    return {LSTM: ("h", "cs", "i", "f", "o", "ci", "co"), GRU: ("h", "i", "f", "o", "ci")}.get(cell, ("h", "z"))


def read(cell):
    return {LSTM: ("x", "hp", "csp", "w", "r", "b")}.get(cell, ("x", "hp", "w", "r", "b"))


# ---- the handle (src/libxsmm_dnn_rnncell.c) ------------------------------------------------------------------------------------------
class Handle:
    def __init__(self, d, hsw=True):
        """hsw: the reference's answer below AVX-512, which is also this engine's (BF16 is refused)"""
        self.d, self.ok = d, False
        if d["datatype_in"] != d["datatype_out"] or d["datatype_in"] not in (F32, BF16):
            self.status = ERR_UNSUPPORTED_DATATYPE
            return
        if d["datatype_in"] == BF16:
            self.status = ERR_UNSUPPORTED_DATATYPE
            return
        if d["max_T"] < 1:
            self.status = ERR_TIME_STEPS_TOO_SMALL
            return
        self.ok, self.status = True, SUCCESS
        self.T = d["max_T"] if d["seq"] < 0 else d["seq"]
        self.bn, self.bc, self.bk = (64 if d[k] == 0 else d[k] for k in ("bn", "bc", "bk"))
        if d["N"] % self.bn:
            self.bn, self.status = d["N"], WARN_N
        if d["C"] % self.bc:
            self.bc, self.status = d["C"], WARN_C
        if d["K"] % self.bk:
            self.bk, self.status = d["K"], WARN_K
        self.G = gates(d["cell"])

    def layout(self, t):
        d = self.d
        N, C, K, T, G = d["N"], d["C"], d["K"], d["max_T"], self.G
        bfmt, ffmt = d["buffer_format"], d["filter_format"]
        state = t in (CSP, DCSP, HP, DHP, CS, DCS, H, DH, GI, GF, GO, GCI, GCO)
        if t in (X, DX) or state:
            dim, f, blk = (DIM_C, C, self.bc) if not state else (DIM_K, K, self.bk)
            if bfmt & FMT_NCPACKED:
                st, l = made((dim, DIM_N, dim, DIM_N, DIM_T), (blk, self.bn, f // blk, N // self.bn, T), F32, bfmt, TT_ACTIVATION)
            elif bfmt & FMT_NC:
                st, l = made((dim, DIM_N, DIM_T), (f, N, T), F32, bfmt, TT_ACTIVATION)
            else:
                return ERR_INVALID_FORMAT_GENERAL, None
        elif t in (W, DW, R, DR, WT, RT):
            trans, weight = t in (WT, RT), t in (W, DW, WT)
            dr, red, bred = (DIM_C, C, self.bc) if weight else (DIM_K, K, self.bk)
            if ffmt & FMT_CKPACKED:
                types = (dr, DIM_K, DIM_K, dr) if trans else (DIM_K, dr, dr, DIM_K)
                sizes = (bred, self.bk, K // self.bk, red // bred) if trans else (self.bk, bred, red // bred, K // self.bk)
                if G > 1:
                    types, sizes = types + (DIM_X,), sizes + (G,)
                st, l = made(types, sizes, F32, ffmt, TT_FILTER)
            elif ffmt & FMT_CK:
                st, l = made((dr, DIM_K) if trans else (DIM_K, dr), (red, G * K) if trans else (G * K, red), F32, ffmt, TT_FILTER)
            else:
                return ERR_INVALID_FORMAT_GENERAL, None
        elif t in (B, DB):
            if not bfmt & (FMT_NC | FMT_NCPACKED):
                return ERR_INVALID_FORMAT_GENERAL, None
            st, l = made((DIM_K,), (G * K,), F32, bfmt, TT_CHANNEL_SCALAR)
        else:
            return ERR_UNKNOWN_TENSOR_TYPE, None
        l["custom_format"] = 0
        return st, l

    def simple(self):
        return self.d["cell"] in (RELU, SIGMOID, TANH)

    def scratch_size(self, kind):
        """(size, status)"""
        d = self.d
        C, K, N, T, G = d["C"], d["K"], d["N"], d["max_T"], self.G
        if d["cell"] not in CELLS:
            return 0, ERR_INVALID_RNN_TYPE
        if kind not in (FWD, BWD, UPD, BWDUPD, ALL):
            return 0, ERR_INVALID_KIND
        if self.simple():
            if kind == FWD:
                return 0, SUCCESS
            return (C * K * 4 + 64) + (K * K * 4 + 64) + (C * N * 4 + 64) + (K * N * 4 + 64) + (K * N * 4 * T + 64), SUCCESS
        size = (C * K * 4 * G + G * 64) + (K * K * 4 * G + G * 64)
        if kind != FWD:
            size += (C * K * 4 * G + G * 64) + (K * K * 4 * G + G * 64) + (C * N * 4 + 64) + 12 * (K * N * 4 + 64)
        return size, SUCCESS

    def internalstate_size(self, kind):
        d = self.d
        if d["cell"] not in CELLS:
            return 0, ERR_INVALID_RNN_TYPE
        if kind not in (FWD, BWD, UPD, BWDUPD, ALL):
            return 0, ERR_INVALID_KIND
        return (d["K"] * d["N"] * 4 * d["max_T"] + 64 if self.simple() else 0), SUCCESS

    def bind_scratch(self, kind, null):
        if self.d["cell"] not in CELLS:
            return ERR_INVALID_RNN_TYPE
        if kind not in (FWD, BWD, UPD, BWDUPD, ALL):
            return ERR_INVALID_KIND
        if self.simple() and kind == FWD:
            return SUCCESS
        return ERR_SCRATCH_NOT_ALLOCED if null else SUCCESS

    def release(self, kind):
        if self.d["cell"] not in CELLS:
            return ERR_INVALID_RNN_TYPE
        return SUCCESS if kind in (FWD, BWD, UPD, BWDUPD, ALL) else ERR_INVALID_KIND

    def bind_internalstate(self, kind, null):
        if self.d["cell"] not in CELLS:
            return ERR_INVALID_RNN_TYPE
        if self.simple() and null:
            return ERR_SCRATCH_NOT_ALLOCED
        return self.release(kind)

    def shape(self, key):
        d = self.d
        N, C, K, T, G = d["N"], d["C"], d["K"], d["max_T"], self.G
        return {"x": (T, N, C), "w": (C, G * K), "r": (K, G * K), "b": (G * K,)}.get(key, (T, N, K))

    def shares(self):
        """the rows of the minibatch each logical thread owns"""
        blocks = self.d["N"] // self.bn
        return [tuple(self.bn * b for b in share(blocks, self.d["threads"], t)) for t in range(self.d["threads"])]


# ---- the reduction blocking and the chain order ------------------------------------------------------------------------------------------
def blocking_factor(C, K, cblocks, kblocks):
    bf = 1
    if 1024 < C <= 2048 or 1024 < K <= 2048:
        bf = 8
        while cblocks % bf or kblocks % bf:
            bf -= 1
    if C > 2048 or K > 2048:
        bf = 16
        while cblocks % bf or kblocks % bf:
            bf -= 1
    if C == 2048 and K == 1024:
        bf = 2
    return bf


# ---- elementwise (src/libxsmm_dnn_elementwise.c), element by element with the platform libm ---------------------------------------------
def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def sigmoid(a, log=None):
    """1.0f / (1.0f + (float)exp((double)-x))"""
    flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if log is not None:
        log.extend(("exp", -float(v)) for v in flat)
    with np.errstate(all="ignore"):
        e = np.array([_exp(-float(v)) for v in flat], dtype=np.float64).astype(np.float32)
        return (np.float32(1) / (np.float32(1) + e)).reshape(np.shape(a))


def tanh(a, log=None):
    flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if log is not None:
        log.extend(("tanh", float(v)) for v in flat)
    with np.errstate(all="ignore"):
        return np.array([math.tanh(float(v)) for v in flat], dtype=np.float64).astype(np.float32).reshape(np.shape(a))


def relu(a):
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(a < 0, np.float32(0), a)


def _first_nan(a, b, res):
    """where both operands are NaN the result is the first one, as the scalar x86 instruction has it (numpy's own choice depends on
    whether its vector loop or its scalar loop runs, that is on the shape; the signs of the NaNs of special_* are in the capture)"""
    return np.where(np.isnan(a) & np.isnan(b), a, res)


def mul(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        return _first_nan(a, b, a * b)


def fma_ld(a, b, c, fused):
    """dst += src0 * src1: a multiply and an add (what the capture shows), or one fused operation"""
    with np.errstate(all="ignore"):
        if fused:
            return fma(a, b, c)
        c, p = np.asarray(c, dtype=np.float32), mul(a, b)
        return _first_nan(c, p, c + p)


def filled(shape):
    return np.full(shape, 0xffffffff, dtype=np.uint32).view(np.float32)


# ---- the templates ---------------------------------------------------------------------------------------------------------------
def _blocked(m, G, K, red, bred, bk):
    """the upfront reformatting of w or r ([red][G * K]) into one [K/bk][red/bred][bred][bk] array per gate"""
    return [np.ascontiguousarray(m[:, q * K:(q + 1) * K].reshape(red // bred, bred, K // bk, bk).transpose(2, 0, 1, 3)) for q in range(G)]


def _reduce(h, blocked, ikb, first, count, src, col0, ld, dst, red_blk):
    """one batch-reduce call: dst block += sum over `count` blocks from `first` of blocked[ikb][block] * src rows"""
    if count <= 0:
        return
    a_list = [blocked[ikb, first + q].reshape(-1) for q in range(count)]
    b_list = [src[col0 + (first + q) * red_blk:] for q in range(count)]
    orc.smm_reduce(orc.FMA, 0, h.bk, h.bn, red_blk, h.bk, ld, h.d["K"], a_list, b_list, dst)


def forward(h, t, fused=False, log=None):
    """the tensors after FWD with threads = 1: what the pass writes (written(cell)), steps >= T left as 0xff bytes. log collects every
    transcendental evaluated as ("exp" or "tanh", argument)."""
    d = h.d
    N, C, K, maxT, T, cell, G = d["N"], d["C"], d["K"], d["max_T"], h.T, d["cell"], h.G
    bn, bc, bk = h.bn, h.bc, h.bk
    out = {key: filled((maxT, N, K)) for key in written(cell)}
    x, hp, w, r, b = t["x"].reshape(maxT, -1), t["hp"][0].reshape(-1), t["w"], t["r"], t["b"]  # (hp and csp are laid out for max_T steps; step 0 counts)
    hflat = out["h"].reshape(maxT, -1)
    hsrc = lambda j: hp if j == 0 else hflat[j - 1]  # noqa: E731
    work = (N // bn) * (K // bk)
    if h.simple():
        z = out["z"].reshape(maxT, -1)
        wf, rf = w.reshape(-1), r.reshape(-1)
        for j in range(T):
            for inik in range(work):
                n0, k0 = (inik // (K // bk)) * bn, (inik % (K // bk)) * bk
                zv = out["z"][j, n0:n0 + bn, k0:k0 + bk]
                zv[...] = b[k0:k0 + bk]
                dst = z[j][n0 * K + k0:]
                for ic in range(0, C, bc):
                    orc.smm(orc.FMA, 0, bk, bn, bc, K, C, K, wf[ic * K + k0:], x[j][n0 * C + ic:], dst)
                for ic in range(0, K, bk):
                    orc.smm(orc.FMA, 0, bk, bn, bk, K, K, K, rf[ic * K + k0:], hsrc(j)[n0 * K + ic:], dst)
                out["h"][j, n0:n0 + bn, k0:k0 + bk] = relu(zv) if cell == RELU else (sigmoid(zv, log) if cell == SIGMOID else tanh(zv, log))
        return out
    cblocks, kblocks = C // bc, K // bk
    bf = blocking_factor(C, K, cblocks, kblocks)
    cbb, kbb = cblocks // bf, kblocks // bf
    wb, rb = _blocked(w, G, K, C, bc, bk), _blocked(r, G, K, K, bk, bk)
    flat = {key: out[key].reshape(maxT, -1) for key in out}
    blocks = [((inik % (N // bn)) * bn, inik // (N // bn)) for inik in range(work)]
    view = lambda key, j, n0, k0: out[key][j, n0:n0 + bn, k0:k0 + bk]  # noqa: E731

    def init(key, q, j, n0, k0, extra=None):
        v = b[q * K + k0:q * K + k0 + bk]
        view(key, j, n0, k0)[...] = v if extra is None else v + np.float32(extra)

    def wx(key, q, j, cb, n0, ikb):
        _reduce(h, wb[q], ikb, cb * cbb, cbb, x[j], n0 * C, C, flat[key][j][n0 * K + ikb * bk:], bc)

    def rh(key, q, j, cb, n0, ikb, src):
        _reduce(h, rb[q], ikb, cb * kbb, kbb, src, n0 * K, K, flat[key][j][n0 * K + ikb * bk:], bk)

    if cell == LSTM:
        order = (("i", 0), ("ci", 1), ("f", 2), ("o", 3))
        fb = np.float32(0 if d["forget_bias"] is None else d["forget_bias"])

        def eltwise(j, n0, k0):
            csp = t["csp"][0, n0:n0 + bn, k0:k0 + bk] if j == 0 else out["cs"][j - 1, n0:n0 + bn, k0:k0 + bk]
            v = {key: view(key, j, n0, k0) for key in out}
            v["i"][...] = sigmoid(v["i"], log); v["f"][...] = sigmoid(v["f"], log); v["o"][...] = sigmoid(v["o"], log)
            v["ci"][...] = tanh(v["ci"], log)
            v["cs"][...] = mul(v["f"], csp)
            v["cs"][...] = fma_ld(v["i"], v["ci"], v["cs"], fused)
            v["co"][...] = tanh(v["cs"], log)
            v["h"][...] = mul(v["o"], v["co"])

        if C == 2048 and K == 2048:  # the fused body
            for j in range(T):
                for cb in range(bf):
                    for n0, ikb in blocks:
                        for key, q in order:
                            if cb == 0:
                                init(key, q, j, n0, ikb * bk, fb if key == "f" else None)
                            wx(key, q, j, cb, n0, ikb)
                            rh(key, q, j, cb, n0, ikb, hsrc(j))
                        if cb == bf - 1:
                            eltwise(j, n0, ikb * bk)
        else:                        # the diffused body: all of w.x for all steps first
            for j in range(T):
                for cb in range(bf):
                    for n0, ikb in blocks:
                        for key, q in order:
                            if cb == 0:
                                init(key, q, j, n0, ikb * bk, fb if key == "f" else None)
                            wx(key, q, j, cb, n0, ikb)
            for j in range(T):
                for cb in range(bf):
                    for n0, ikb in blocks:
                        for key, q in order:
                            rh(key, q, j, cb, n0, ikb, hsrc(j))
                        if cb == bf - 1:
                            eltwise(j, n0, ikb * bk)
        return out
    # GRU: i, c (INTERNAL_CI), f; two phases per step
    for j in range(T):
        hprev = lambda n0, k0: (t["hp"][0] if j == 0 else out["h"][j - 1])[n0:n0 + bn, k0:k0 + bk]  # noqa: E731
        for cb in range(bf):
            for n0, ikb in blocks:
                k0 = ikb * bk
                for key, q in (("i", 0), ("ci", 1)):
                    if cb == 0:
                        init(key, q, j, n0, k0)
                    wx(key, q, j, cb, n0, ikb)
                    rh(key, q, j, cb, n0, ikb, hsrc(j))
                if cb == bf - 1:
                    view("i", j, n0, k0)[...] = sigmoid(view("i", j, n0, k0), log)
                    view("o", j, n0, k0)[...] = mul(hprev(n0, k0), view("i", j, n0, k0))
        for cb in range(bf):
            for n0, ikb in blocks:
                k0 = ikb * bk
                if cb == 0:
                    init("f", 2, j, n0, k0)
                wx("f", 2, j, cb, n0, ikb)
                rh("f", 2, j, cb, n0, ikb, flat["o"][j])
                if cb == bf - 1:
                    view("f", j, n0, k0)[...] = tanh(view("f", j, n0, k0), log)
                    view("ci", j, n0, k0)[...] = sigmoid(view("ci", j, n0, k0), log)
                    with np.errstate(all="ignore"):
                        view("h", j, n0, k0)[...] = np.float32(1) - view("ci", j, n0, k0)
                    view("h", j, n0, k0)[...] = mul(view("h", j, n0, k0), view("f", j, n0, k0))
                    view("h", j, n0, k0)[...] = fma_ld(view("ci", j, n0, k0), hprev(n0, k0), view("h", j, n0, k0), fused)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
CELLS = (RELU, SIGMOID, TANH, LSTM, GRU)


def _compute_cases():
    c = {}
    for cell in CELLS:
        n = CELL_NAMES[cell]
        c["tiny_" + n] = desc(3, 5, 7, 1, cell)                      # blocks 0: all three warnings; T = 1
        c["blk_" + n] = desc(8, 32, 48, 3, cell, bn=4, bc=16, bk=16)   # T = 3
    for cell in (TANH, LSTM, GRU):
        c["seq_" + CELL_NAMES[cell]] = desc(4, 6, 10, 4, cell, bn=2, bc=3, bk=5, seq=2)  # steps 2 and 3 stay as they were
        c["k72_" + CELL_NAMES[cell]] = desc(5, 9, 72, 2, cell, bn=5, bc=9, bk=24)       # crosses a tile of 64
    c["fbias_lstm"] = desc(4, 8, 12, 2, LSTM, bn=2, bc=4, bk=4, forget_bias=1.0)
    c["bf_lstm"] = desc(4, 1040, 1040, 2, LSTM, bn=4, bc=16, bk=16)    # BF = 5, the diffused body
    c["bf_gru"] = desc(4, 1040, 1040, 2, GRU, bn=4, bc=16, bk=16)      # BF = 5, alternating chunks
    for cell in CELLS:  # three tiles of k (the last 8 wide) by three tiles of rows (the last 2 rows); reductions of 32 + 8 and 4 * 32 + 8
        c["rows_" + CELL_NAMES[cell]] = desc(*ROWS_SHAPE, cell, **ROWS_BLOCKS)
    c["fused_lstm"] = desc(2, 2048, 2048, 2, LSTM, bn=2, bc=64, bk=64)     # BF = 8, the fused body: alternating chunks
    c["odd_gru"] = desc(3, 1053, 1053, 2, GRU, bn=3, bc=13, bk=13)         # BF = 3, chunks of 351 = 10 * 32 + 31, alternating
    return c


ROWS_SHAPE, ROWS_BLOCKS = (130, 40, 136, 2), dict(bn=13, bc=8, bk=17)
COMPUTE_CASES = _compute_cases()
# The forced BF = 2 on one block of C: C / bc / BF = 0 blocks per chunk, so no w.x at all. NOT captured: the unmodified reference ends
# with a segmentation fault here (its batch-reduce kernel is called with a count of zero; with the same bc = 2048 and one block per
# chunk -- K = 512 -- it runs). What this engine computes there, bias + r.h, is therefore its own reading of the template's arithmetic,
# held by the restatement alone.
UNCAPTURED_CASES = {"rem_lstm": desc(2, 2048, 1024, 1, LSTM, bn=2, bc=2048, bk=512)}
GPU_COMPUTE_CASES = dict(COMPUTE_CASES, **UNCAPTURED_CASES)
SPECIAL_CASES = {"special_" + CELL_NAMES[cell]: desc(4, 12, 16, 2, cell, bn=2, bc=4, bk=8) for cell in (RELU, LSTM, GRU)}
SPECIAL_CASES["special_rows_lstm"] = desc(*ROWS_SHAPE, LSTM, **ROWS_BLOCKS)  # and a NaN and an Inf in the second tile both ways
SPECIAL_ROWS_PLANTED = {"nan": (70, 130), "inf": (100, 131)}              # (row, column) of hp at step 0
STATUS_CASES = {
    "st_mixed_dt": desc(4, 4, 4, 1, LSTM, dt=F32, dt_out=BF16), "st_i32": desc(4, 4, 4, 1, LSTM, dt=4), "st_bf16": desc(16, 16, 16, 1, LSTM, dt=BF16),
    "st_T0": desc(4, 4, 4, 0, GRU), "st_packed_lstm": desc(8, 32, 48, 2, LSTM, bn=4, bc=16, bk=16, bfmt=FMT_NCPACKED, ffmt=FMT_CKPACKED),
    "st_packed_relu": desc(8, 32, 48, 2, RELU, bn=4, bc=16, bk=16, bfmt=FMT_NCPACKED, ffmt=FMT_CKPACKED),
    "st_nhwc": desc(4, 4, 4, 1, GRU, bfmt=2, ffmt=8), "st_cell7": desc(4, 4, 4, 1, 7),
}


# threads = 3 on four row blocks (tests/test_rnn_gpu.py)
THREAD_CASES = {"threads_" + CELL_NAMES[cell]: desc(8, 12, 20, 2, cell, bn=2, bc=4, bk=5, threads=3) for cell in (TANH, LSTM, GRU)}
# threads = 3 on twenty row blocks of 13: rows [0, 91), [91, 182), [182, 260), each across a tile boundary, two from the middle of a tile
THREAD_CASES.update({"rowshares_" + CELL_NAMES[cell]: desc(260, 40, 136, 2, cell, threads=3, **ROWS_BLOCKS) for cell in (TANH, LSTM, GRU)})

# past the grid limits of kernels/rnn.hip (tests/launch_limits.py: rnn_steps, rnn_rows_per_share) and just below 2^31 elements
LIMIT_CASES = {
    "steps_tanh": desc(2, 3, 5, 65537, TANH, bn=2, bc=3, bk=5),                       # two trips of the split plan's first launch
    "manyrows_relu": desc(65538 * 64, 1, 1, 1, RELU, bn=65538 * 32, bc=1, bk=1),   # 65538 tiles of rows: one share is refused, two run
}
WIDE_PERIOD = 1240  # rows of the seeded block the wide case repeats: a multiple of bn, no multiple of 64
WIDE_CASE = desc(((1 << 31) - 1) // (2 * 72) // WIDE_PERIOD * WIDE_PERIOD, 8, 72, 2, RELU, bn=40, bc=8, bk=72, threads=4)


def wide_period():
    """(inputs, outputs) of one period of the wide case: a layer of WIDE_PERIOD rows (rows are independent recurrences)"""
    d = dict(WIDE_CASE, N=WIDE_PERIOD, threads=1)
    t = inputs("wide_relu", d)
    return d, t, forward(Handle(d), t)


@functools.lru_cache(maxsize=None)
def limit_expected(name):
    """(inputs, outputs, the transcendentals evaluated) of steps_tanh, computed once"""
    d = LIMIT_CASES[name]
    t, seen = inputs(name, d), []
    return t, forward(Handle(d), t, log=seen), seen


def fma_once(a, b, c):
    """dnn_common.fma with its rare halfway cases put right: where the float64 sum lies exactly between two floats and was itself
    rounded, the error of that rounding (exact: TwoSum) says which way the single rounding goes"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = ((s.view(np.int64) & 0x1fffffff) == 0x10000000) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def forward_c1k1(t):
    """a simple ReLU cell with C = K = 1 and one step, all rows at once: z = fma(r, hp, fma(w, x, b)); returns (h, z)"""
    z = fma_once(t["r"].reshape(()), t["hp"][0].reshape(-1), fma_once(t["w"].reshape(()), t["x"][0].reshape(-1), t["b"].reshape(())))
    return relu(z).reshape(1, -1, 1), z.reshape(1, -1, 1)


def sweep_cases():
    """24 seeded descriptors: all five cells, N <= 12, C and K <= 80, T <= 3, blocks drawn from divisors and non-divisors"""
    rng = np.random.default_rng(20240)
    cases = {}
    for idx in range(24):
        cell = CELLS[idx % 5]
        N, Cc, K, T = int(rng.integers(1, 13)), int(rng.integers(1, 81)), int(rng.integers(1, 81)), int(rng.integers(1, 4))
        blk = lambda n: int(rng.choice([0, 1, n] + [q for q in range(2, n + 1) if n % q == 0] + [n + 1, 7]))  # noqa: E731
        cases["sweep%02d_%s" % (idx, CELL_NAMES[cell])] = desc(N, Cc, K, T, cell, bn=blk(N), bc=blk(Cc), bk=blk(K),
                                                                     forget_bias=(0.5 if idx % 10 == 3 else None))
    return cases


SWEEP = sweep_cases()


def captured_cases():
    return dict(list(COMPUTE_CASES.items()) + list(SPECIAL_CASES.items()) + list(STATUS_CASES.items()))


def inputs(name, d):
    """the seeded inputs of a case: moderate values, so that the gates neither saturate nor vanish; special_*: with +-Inf, NaN, +-0 and
    values beyond +-90 (exp overflows to Inf and underflows) planted in x, hp and b"""
    h = Handle(d)
    rng = np.random.default_rng([zlib.crc32(name.encode()), d["seed"]])
    t = {}
    for key in read(d["cell"]):
        scale = {"w": 1.5 / math.sqrt(d["C"]), "r": 1.5 / math.sqrt(d["K"])}.get(key, 1.0)
        t[key] = ((rng.random(h.shape(key)) * 2 - 1) * scale).astype(np.float32)
    if name.startswith("special_"):
        x, hp, b = t["x"], t["hp"], t["b"]
        x[0, 0, 0], x[0, 1, 1], x[1, 2, 2] = np.inf, -np.inf, np.nan
        x[0, 3, :], x[1, 3, 5] = 0.0, -0.0
        hp[0, 3, :] = -0.0
        hp[0, 2, 3] = np.nan
        b[1], b[2], b[3], b[4] = 95.0, -95.0, 130.0, -130.0
        for q in range(1, h.G):
            b[q * d["K"] + 5], b[q * d["K"] + 6] = 100.0 + q, -100.0 - q
        t["w"][:, 7] = 0.0  # products with +-Inf and NaN there: 0 * Inf
    if name == "special_rows_lstm":  # beyond the first tile both ways: the poison has to stay in its row
        hp[(0,) + SPECIAL_ROWS_PLANTED["nan"]], hp[(0,) + SPECIAL_ROWS_PLANTED["inf"]] = np.nan, np.inf
    return t


@functools.lru_cache(maxsize=None)
def expected(name, log=False):
    """(inputs, outputs[, the transcendentals evaluated]) of a captured (or uncaptured compute) case, computed once"""
    d = dict(captured_cases(), **UNCAPTURED_CASES)[name]
    t = inputs(name, d)
    seen = [] if log else None
    out = forward(Handle(d), t, log=seen)
    return (t, out, seen) if log else (t, out)


def same_bits(got, want, nan_class=False):
    """bitwise equality; nan_class (special_* on the GPU only): an element that is NaN in both counts as equal whatever its sign and
    payload (x86 answers 0 * Inf with the negative default NaN, gfx950 with the positive one)"""
    g, w = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32) for a in (got, want))
    if g.shape != w.shape:
        return False
    if not nan_class:
        return bool(np.array_equal(g, w))
    both = np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))
    return bool(np.array_equal(g[~both], w[~both]))
