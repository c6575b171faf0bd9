"""The backward and update passes of the RNN cell layer restated for the tests: the two generic templates
src/template/libxsmm_dnn_rnncell_st_{rnn,lstm}_bwdupd_nc_ck_generic.tpl.c (the LSTM's with ..._lstm_bwdupd_nc_kcck_core.tpl.c, the branch
without LIBXSMM_RNN_CELL_AVX512) loop for loop -- every SMM or batch-reduce SMM call of a template is a call of the CPU oracle's SMM
(tests/oracle_binding.py) on the transposed and blocked copies the templates make first, and the elementwise loops of
src/libxsmm_dnn_elementwise.c are evaluated with numpy in fp32, the transcendentals with the platform libm (rnn_common.sigmoid, tanh).
tests/test_rnn_bwd_cpu.py holds all of it against the reference's captured outputs (tests/golden/rnn_bwd.npz, written by
tools/golden/rnn_bwd_capture.py). The one liberty: the LSTM template accumulates dw and dr in a blocked scratch copy and reformats it
at the end; here the same SMM calls write the plain tensor directly (no arithmetic differs)."""
import functools
import zlib

import numpy as np

import oracle_binding as orc
import rnn_common as rc
from rnn_common import RELU, SIGMOID, TANH, LSTM, BWD, UPD, BWDUPD, desc, filled, mul  # noqa: F401

KINDS = (BWD, UPD, BWDUPD)
KIND_NAMES = {BWD: "bwd", UPD: "upd", BWDUPD: "bwdupd"}
GRADS = ("dx", "dcsp", "dhp", "dw", "dr", "db")
GRAD_TYPE = {"dx": rc.DX, "dcsp": rc.DCSP, "dhp": rc.DHP, "dw": rc.DW, "dr": rc.DR, "db": rc.DB, "dcs": rc.DCS, "dh": rc.DH}
CELLS = (RELU, SIGMOID, TANH, LSTM)


def grad_shape(h, key):
    d = h.d
    N, C, K, T, G = d["N"], d["C"], d["K"], d["max_T"], h.G
    return {"dx": (T, N, C), "dw": (C, G * K), "dr": (K, G * K), "db": (G * K,)}.get(key, (T, N, K))


def written(cell, kind):
    """the gradient tensors a kind writes; the others keep their bytes"""
    out = ()
    if kind in (BWD, BWDUPD):
        out += ("dx",)
    if kind in (UPD, BWDUPD):
        out += ("dw", "dr", "db")
    if cell == LSTM:
        out += ("dcsp", "dhp")
    return out


def launches(cell, kind, T):
    """one launch per step, the LSTM's dhp, dx of all steps per 65535 of them, and dw, dr, db: a function of T and the kind alone"""
    return T + (1 if cell == LSTM else 0) + ((T + 65534) // 65535 if kind in (BWD, BWDUPD) else 0) + (3 if kind in (UPD, BWDUPD) else 0)


def bwd_blocking_factor(K, kblocks):
    """the backward templates' BF: a function of K alone (lstm bwdupd template :255-270)"""
    bf = 1
    if 1024 < K <= 2048:
        bf = 8
        while kblocks % bf:
            bf -= 1
    if K > 2048:
        bf = 16
        while kblocks % bf:
            bf -= 1
    return bf


def sub(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float32) - np.asarray(b, dtype=np.float32)


def add(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        return rc._first_nan(a, b, a + b)


ONE = np.float32(1)


def inverse(cell, z, log=None):
    """libxsmm_internal_matrix_{relu,sigmoid,tanh}_inverse_ld: act'(z), every operation rounded on its own"""
    if cell == RELU:
        with np.errstate(invalid="ignore"):
            return np.where(np.asarray(z) < 0, np.float32(0), ONE).astype(np.float32)
    if cell == SIGMOID:
        s = rc.sigmoid(z, log)
        return mul(sub(ONE, s), s)
    t = rc.tanh(z, log)
    return sub(ONE, mul(t, t))


def backward(h, t, kind, log=None):
    """the gradient tensors after `kind` with threads = 1, everything not written left as 0xff bytes; also "delta": the deltas of all
    steps [T][N][G * K] (the template's scratch). t: the inputs, the forward pass's tensors and dh (LSTM: dcs)."""
    d = h.d
    N, C, K, maxT, T, cell, G = d["N"], d["C"], d["K"], d["max_T"], h.T, d["cell"], h.G
    bn, bc, bk = h.bn, h.bc, h.bk
    bwd, upd = kind in (BWD, BWDUPD), kind in (UPD, BWDUPD)
    out = {key: filled(grad_shape(h, key)) for key in GRADS}
    out["delta"] = np.zeros((maxT, N, G * K), dtype=np.float32)
    if T < 1:
        return out
    x, w, r, dh = t["x"], t["w"], t["r"], t["dh"]
    hp, hh = t["hp"][0], t["h"]
    if bwd:
        out["dx"][:T] = 0
    if upd:
        out["dw"][...] = 0
        out["dr"][...] = 0
        out["db"][...] = 0
    dxf, dwf, drf = out["dx"].reshape(maxT, -1), out["dw"].reshape(-1), out["dr"].reshape(-1)
    nk_blocks = [((q // (K // bk)) * bn, (q % (K // bk)) * bk) for q in range((N // bn) * (K // bk))]

    def update(j, deltas):
        """db, dr and dw of step j; deltas: the [N][K] arrays in the order of the filter's column blocks"""
        xT = np.ascontiguousarray(x[j].T).reshape(-1)
        hT = np.ascontiguousarray((hp if j == 0 else hh[j - 1]).T).reshape(-1)  # (T == 1 on a simple cell: the reference reads h[-1])
        for q, dq in enumerate(deltas):
            for n in range(N):
                out["db"][q * K:(q + 1) * K] = add(out["db"][q * K:(q + 1) * K], dq[n])
        ld = G * K
        for q, dq in enumerate(deltas):
            flat = dq.reshape(-1)
            for ic in range(0, K, bk):
                for ik in range(0, K, bk):
                    a_list = [flat[n0 * K + ik:] for n0 in range(0, N, bn)]
                    b_list = [hT[ic * N + n0:] for n0 in range(0, N, bn)]
                    orc.smm_reduce(orc.FMA, 0, bk, bk, bn, K, N, ld, a_list, b_list, drf[ic * ld + q * K + ik:])
            for ic in range(0, C, bc):
                for ik in range(0, K, bk):
                    a_list = [flat[n0 * K + ik:] for n0 in range(0, N, bn)]
                    b_list = [xT[ic * N + n0:] for n0 in range(0, N, bn)]
                    orc.smm_reduce(orc.FMA, 0, bk, bc, bn, K, N, ld, a_list, b_list, dwf[ic * ld + q * K + ik:])

    if h.simple():
        z = t["z"]
        delta = out["delta"]
        dflat = delta.reshape(maxT, -1)
        wT, rT = np.ascontiguousarray(w.T).reshape(-1), np.ascontiguousarray(r.T).reshape(-1)
        for i in range(T - 1, -1, -1):
            for n0, k0 in nk_blocks:
                blk = (i, slice(n0, n0 + bn), slice(k0, k0 + bk))
                if i == T - 1:
                    delta[blk] = inverse(cell, z[blk], log)
                    delta[blk] = mul(delta[blk], dh[blk])
                else:
                    delta[blk] = dh[blk]
                    for ic in range(0, K, bk):
                        orc.smm(orc.FMA, 0, bk, bn, bk, K, K, K, rT[ic * K + k0:], dflat[i + 1][n0 * K + ic:], dflat[i][n0 * K + k0:])
                    delta[blk] = mul(delta[blk], inverse(cell, z[blk], log))
            if bwd:
                for n0 in range(0, N, bn):
                    for ic in range(0, C, bc):
                        for ik in range(0, K, bk):
                            orc.smm(orc.FMA, 0, bc, bn, bk, C, K, C, wT[ik * C + ic:], dflat[i][n0 * K + ik:], dxf[i][n0 * C + ic:])
            if upd:
                update(i, [delta[i]])
        return out

    # LSTM
    kblocks = K // bk
    bf = bwd_blocking_factor(K, kblocks)
    kbb = kblocks // bf
    # the transposed blocked copies: wT[q][icb][ikb][jk][jc] = w_q[icb * bc + jc][ikb * bk + jk], rT likewise with bk for bc
    tb = lambda m, q, red, bred: np.ascontiguousarray(m[:, q * K:(q + 1) * K].reshape(red // bred, bred, kblocks, bk).transpose(0, 2, 3, 1))  # noqa: E731
    wT, rT = [tb(w, q, C, bc) for q in range(4)], [tb(r, q, K, bk) for q in range(4)]
    gi, gf, go, gci, gco, cs = t["i"], t["f"], t["o"], t["ci"], t["co"], t["cs"]
    csp, dcs = t["csp"][0], t["dcs"][0]
    di, dci, df, dp = (np.zeros((N, K), dtype=np.float32) for _ in range(4))
    dout = np.zeros((N, K), dtype=np.float32)
    dcp, dhp = out["dcsp"][0], out["dhp"][0]
    for j in range(T - 1, -1, -1):
        for n0, k0 in nk_blocks:
            b2, b3 = (slice(n0, n0 + bn), slice(k0, k0 + bk)), (j, slice(n0, n0 + bn), slice(k0, k0 + bk))
            dout[b2] = dh[b3] if j == T - 1 else add(dout[b2], dh[b3])
            t1 = mul(dout[b2], go[b3]); t2 = sub(ONE, mul(gco[b3], gco[b3])); t1 = mul(t1, t2)
            dcp[b2] = add(dcs[b2] if j == T - 1 else dcp[b2], t1)
            t1 = mul(dcp[b2], gi[b3]); t2 = sub(ONE, mul(gci[b3], gci[b3])); dci[b2] = mul(t1, t2)
            t1 = mul(dcp[b2], gci[b3]); t2 = sub(ONE, gi[b3]); di[b2] = mul(gi[b3], t2); di[b2] = mul(t1, di[b2])
            t1 = mul(dcp[b2], csp[b2] if j == 0 else cs[j - 1][b2]); t2 = sub(ONE, gf[b3]); df[b2] = mul(gf[b3], t2); df[b2] = mul(t1, df[b2])
            t1 = mul(dout[b2], gco[b3]); t2 = sub(ONE, go[b3]); t2 = mul(go[b3], t2); dp[b2] = mul(t1, t2)
            dcp[b2] = mul(gf[b3], dcp[b2])
        for q, dq in enumerate((di, dci, df, dp)):
            out["delta"][j][:, q * K:(q + 1) * K] = dq
        flats = [dq.reshape(-1) for dq in (di, dci, df, dp)]
        if bwd:
            for kb in range(bf):
                for icb in range(C // bc):
                    for n0 in range(0, N, bn):
                        for q in range(4):
                            a_list = [wT[q][icb, kb * kbb + b].reshape(-1) for b in range(kbb)]
                            b_list = [flats[q][n0 * K + (kb * kbb + b) * bk:] for b in range(kbb)]
                            orc.smm_reduce(orc.FMA, 0, bc, bn, bk, bc, K, C, a_list, b_list, dxf[j][n0 * C + icb * bc:])
        dst = (dout if j > 0 else dhp)
        dstf = dst.reshape(-1)
        for kb in range(bf):
            for ikb in range(kblocks):
                for n0 in range(0, N, bn):
                    if kb == 0:
                        dst[n0:n0 + bn, ikb * bk:(ikb + 1) * bk] = 0
                    for q in range(4):
                        a_list = [rT[q][ikb, kb * kbb + b].reshape(-1) for b in range(kbb)]
                        b_list = [flats[q][n0 * K + (kb * kbb + b) * bk:] for b in range(kbb)]
                        orc.smm_reduce(orc.FMA, 0, bk, bn, bk, bk, K, K, a_list, b_list, dstf[n0 * K + ikb * bk:])
        if upd:
            update(j, (di, dci, df, dp))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _compute_cases():
    c = {}
    for cell in CELLS:
        n = rc.CELL_NAMES[cell]
        c["one_" + n] = desc(4, 12, 16, 3, cell, bn=2, bc=4, bk=8, seq=2)   # inside one block; step 2 stays as it was
        c["rows_" + n] = desc(130, 40, 136, 3, cell, **rc.ROWS_BLOCKS)       # three tiles each way, the last ones partial, k tails
    c["bf5_lstm"] = desc(2, 8, 1040, 2, LSTM, bn=2, bc=8, bk=208)           # BF = 5
    c["bf12_lstm"] = desc(2, 8, 2064, 2, LSTM, bn=2, bc=8, bk=172)          # BF = 12
    c["t1_lstm"] = desc(4, 12, 16, 1, LSTM, bn=2, bc=4, bk=8)               # a single step
    return c


COMPUTE_CASES = _compute_cases()
# a single step on a simple cell: the reference's UPD transposes h[T - 2], that is, it reads before the tensor; here step 0 multiplies
# hp as in every other path. Not captured; held by the restatement alone.
UNCAPTURED_CASES = {"t1_tanh": desc(4, 12, 16, 1, TANH, bn=2, bc=4, bk=8)}
SPECIAL_CASES = {"special_" + rc.CELL_NAMES[cell]: desc(4, 12, 16, 3, cell, bn=2, bc=4, bk=8) for cell in (RELU, TANH, LSTM)}
SPECIAL_CASES["special_rows_lstm"] = desc(130, 40, 136, 2, LSTM, **rc.ROWS_BLOCKS)
# (step, row, column) of the NaN and the Inf in dh, and of those in z (simple cells) or o (LSTM)
PLANTED = {"dh_nan": (1, 1, 3), "dh_inf": (0, 2, 5), "fwd_nan": (0, 3, 9), "fwd_inf": (1, 0, 11)}
# beyond the first tile both ways and all at step 0, the last one computed: the poison has to stay in its row of dx, dhp and dcsp and in
# its column (of every gate) of dw, dr and db
PLANTED_ROWS = {"dh_nan": (0, 70, 130), "dh_inf": (0, 100, 131), "fwd_nan": (0, 129, 5), "fwd_inf": (0, 3, 70)}
THREAD_CASES = {"threads_" + rc.CELL_NAMES[cell]: desc(260, 40, 136, 2, cell, threads=3, **rc.ROWS_BLOCKS) for cell in (TANH, LSTM)}
LIMIT_CASES = {
    "steps_relu": desc(2, 3, 5, 65537, RELU, bn=2, bc=3, bk=5),                      # the dx launch splits at 65535 steps
    "manyrows_relu": desc(4194432, 8, 8, 1, RELU, bn=2097216, bc=8, bk=8),         # 65538 tiles of rows: one share is refused, two run
}


def captured_cases():
    return dict(list(COMPUTE_CASES.items()) + list(SPECIAL_CASES.items()))


def all_cases():
    return dict(captured_cases(), **UNCAPTURED_CASES)


def planted(name):
    return PLANTED_ROWS if name == "special_rows_lstm" else PLANTED


def inputs(name, d):
    """the forward pass's inputs (rnn_common.inputs under the name "bwd_" + name), its outputs as the restatement gives them, and
    the seeded dh (LSTM: and dcs); special_*: with a NaN and an Inf planted in dh and in z (simple cells) or o (LSTM)"""
    h = rc.Handle(d)
    t = dict(rc.inputs("bwd_" + name, d))
    t.update(rc.forward(h, t))
    rng = np.random.default_rng([zlib.crc32(("bwd_" + name).encode()), d["seed"], 1])
    shape = (d["max_T"], d["N"], d["K"])
    t["dh"] = (rng.random(shape) * 2 - 1).astype(np.float32)
    if d["cell"] == LSTM:
        t["dcs"] = (rng.random(shape) * 2 - 1).astype(np.float32)
    if name.startswith("special_"):
        p = planted(name)
        fwd = "o" if d["cell"] == LSTM else "z"
        t[fwd] = t[fwd].copy()
        t["dh"][p["dh_nan"]], t["dh"][p["dh_inf"]] = np.nan, np.inf
        t[fwd][p["fwd_nan"]], t[fwd][p["fwd_inf"]] = np.nan, np.inf
    return t


def read(cell):
    """what a backward pass reads, in a fixed order"""
    return rc.read(cell) + rc.written(cell) + (("dh", "dcs") if cell == LSTM else ("dh",))


@functools.lru_cache(maxsize=None)
def expected(name, kind, threads1=True):
    """(inputs, gradient tensors) of a case under a kind, computed once and left unchanged"""
    d = dict(all_cases(), **THREAD_CASES)[name]
    if threads1:
        d = dict(d, threads=1)
    t = cached_inputs(name)
    return t, backward(rc.Handle(d), t, kind)


@functools.lru_cache(maxsize=None)
def cached_inputs(name):
    d = dict(all_cases(), **THREAD_CASES)[name]
    return inputs(name, dict(d, threads=1))
