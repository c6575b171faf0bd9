"""The backward and update passes of the RNN cell layer restated for the tests: the two generic templates
src/template/libxsmm_dnn_rnncell_st_{rnn,lstm}_bwdupd_nc_ck_generic.tpl.c (the LSTM's with ..._lstm_bwdupd_nc_kcck_core.tpl.c, the branch
without LIBXSMM_RNN_CELL_AVX512) loop for loop -- every SMM or batch-reduce SMM call of a template is a call of the CPU oracle's SMM
(tests/oracle_binding.py) on the transposed and blocked copies the templates make first, and the elementwise loops of
src/libxsmm_dnn_elementwise.c are evaluated with numpy in fp32, the transcendentals with the platform libm (rnn_common.sigmoid, tanh).
tests/test_rnn_bwd_cpu.py holds all of it against the reference's captured outputs (tests/golden/rnn_bwd.npz, written by
tools/golden/rnn_bwd_capture.py). The one liberty: the LSTM template accumulates dw and dr in a blocked scratch copy and reformats it
at the end; here the same SMM calls write the plain tensor directly (no arithmetic differs).

Beside the restatement, and independent of it: contract64, a float64 definition of every gradient tensor written from the text of
include/libxsmm_dnn_rnncell.h with derived error bounds (and forward64, the forward cell in the same terms), and sweep_cases, 32 seeded
descriptors with their census."""
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


# ---- the float64 contract ------------------------------------------------------------------------------------------------------------
# What include/libxsmm_dnn_rnncell.h says each tensor is, in float64 numpy on the plain tensors: no blocks, no segments, no oracle call.
# Beside every value runs a bound of what the fp32 evaluation the header describes may be off by, derived and never measured:
#   one rounded operation (multiply, add, subtract, divide, the float conversion of a double exp or tanh) on operands that are off by
#     at most p in the result's terms: p + u * (|result| + p);
#   a chain of L fused multiply-adds from a start s: with P the operands' errors carried through (|a| eb + ea |b| + ea eb, summed, + es),
#     P + g * (|s| + sum |a| |b| + P), g = L u / (1 - L u): the order of the chain plays no part, so neither do blocks and segments;
#   plain adds from +0.0 (db) are such a chain with a = 1; ReLU's derivative is exact; a transcendental of an argument that is itself
#     off by e: |tanh'| <= 1 gives e, exp(-z) gives exp(-z) * expm1(e).
# u = 2^-24. SLACK covers the float64 evaluation of the values and of the bounds themselves (chains of a few thousand terms at 2^-53,
# the double exp and tanh of the libm at an ulp: below 2^-40 of any term that u multiplies).
U32 = 2.0 ** -24
SLACK = 1 + 2.0 ** -20
# mistakes made on purpose in the definition (tests/test_rnn_bwd_cpu.py shows that the bounds reject each)
WRONG = ("dr_from_h_of_the_step", "hp_not_used_at_step_0", "df_from_cs_of_the_step", "dw_c_and_f_columns_swapped", "dout_without_dh",
         "dcsp_without_f", "act_prime_of_the_neighbouring_step", "db_without_the_last_step", "dx_over_r", "steps_beyond_seq",
         "recurrence_over_r_untransposed", "dp_with_ci_for_co")


class V:
    """float64 values beside the bounds of what fp32 may be off by"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros(self.v.shape) if e is None else np.asarray(e, dtype=np.float64)

    def cols(self, a, b):
        return V(self.v[:, a:b], self.e[:, a:b])


def hcat(parts):
    return V(np.concatenate([p.v for p in parts], axis=1), np.concatenate([p.e for p in parts], axis=1))


def vcat(parts):
    return V(np.concatenate([p.v for p in parts], axis=0), np.concatenate([p.e for p in parts], axis=0))


class Rounding:
    """the operations of the header's text at unit roundoff u"""

    def __init__(self, u=U32):
        self.u = u

    def rounded(self, v, p):
        return V(v, p + self.u * (np.abs(v) + p))

    def mul(self, a, b):
        return self.rounded(a.v * b.v, np.abs(a.v) * b.e + a.e * np.abs(b.v) + a.e * b.e)

    def add(self, a, b):
        return self.rounded(a.v + b.v, a.e + b.e)

    def sub(self, a, b):
        return self.rounded(a.v - b.v, a.e + b.e)

    def chain(self, start, a, b):
        """start (None: +0.0) continued by one fma chain over the inner dimension of a @ b"""
        L = a.v.shape[-1]
        g = L * self.u / (1 - L * self.u)
        v, mag = a.v @ b.v, np.abs(a.v) @ np.abs(b.v)
        p = np.abs(a.v) @ b.e + a.e @ np.abs(b.v) + a.e @ b.e
        if start is not None:
            v, mag, p = v + start.v, mag + np.abs(start.v), p + start.e
        return V(v, p + g * (mag + p))

    def sigmoid(self, z):
        """1.0f / (1.0f + (float)exp((double)-z))"""
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-z.v)
            den = self.add(V(1.0), self.rounded(e, e * np.expm1(z.e)))
            return self.rounded(1 / den.v, np.where(den.v > den.e, den.e / (den.v * (den.v - den.e)), np.inf))

    def tanh(self, z):
        return self.rounded(np.tanh(z.v), z.e)

    def act(self, cell, z):
        if cell == RELU:
            return V(np.where(z.v < 0, 0.0, z.v), z.e)
        return self.sigmoid(z) if cell == SIGMOID else self.tanh(z)

    def act_prime(self, cell, z):
        """of an argument taken as exact"""
        one = V(1.0)
        if cell == RELU:
            return V(np.where(z.v < 0, 0.0, 1.0))
        if cell == SIGMOID:
            s = self.sigmoid(z)
            return self.mul(self.sub(one, s), s)
        t = self.tanh(z)
        return self.sub(one, self.mul(t, t))


def forward64(h, t, u=U32):
    """the forward cell of the header's text: key -> V of the steps below the sequence length, [T][N][K]; t: x, hp, w, r, b (csp)"""
    d = h.d
    K, T, cell = d["K"], h.T, d["cell"]
    R = Rounding(u)
    f = lambda key: np.asarray(t[key], dtype=np.float64)  # noqa: E731
    x, b, both = f("x"), f("b"), V(np.concatenate([f("w"), f("r")], axis=0))
    hprev = V(f("hp")[0])
    steps = {key: [] for key in rc.written(cell)}
    if h.simple():
        for s in range(T):
            z = R.chain(V(np.broadcast_to(b, hprev.v.shape)), hcat([V(x[s]), hprev]), both)
            hprev = R.act(cell, z)
            steps["z"].append(z)
            steps["h"].append(hprev)
    else:
        start = V(b)
        if d["forget_bias"] is not None:  # b_f + forget_bias: one rounded add
            fb = np.zeros(4 * K)
            fb[2 * K:3 * K] = np.float32(d["forget_bias"])
            start = R.add(start, V(fb))
        csprev = V(f("csp")[0])
        for s in range(T):
            pre = R.chain(V(np.broadcast_to(start.v, (x.shape[1], 4 * K)), np.broadcast_to(start.e, (x.shape[1], 4 * K))), hcat([V(x[s]), hprev]), both)
            gi, gci, gf, go = R.sigmoid(pre.cols(0, K)), R.tanh(pre.cols(K, 2 * K)), R.sigmoid(pre.cols(2 * K, 3 * K)), R.sigmoid(pre.cols(3 * K, 4 * K))
            csprev = R.add(R.mul(gf, csprev), R.mul(gi, gci))
            co = R.tanh(csprev)
            hprev = R.mul(go, co)
            for key, val in (("i", gi), ("ci", gci), ("f", gf), ("o", go), ("cs", csprev), ("co", co), ("h", hprev)):
                steps[key].append(val)
    return {key: V(np.stack([s.v for s in val]), np.stack([s.e for s in val]) * SLACK) for key, val in steps.items() if val}


def contract64(h, t, kind, wrong=None, u=U32):
    """key -> (value, bound) of every gradient tensor the kind writes: dx [T][N][C] (the steps below the sequence length), dw, dr, db,
    and of the LSTM dcsp and dhp [N][K] (step 0 of their tensors). t: the inputs, the forward pass's tensors and dh (LSTM: dcs), all taken
    as exact (fp32 or float64). wrong: one of WRONG."""
    d = h.d
    N, C, K, cell = d["N"], d["C"], d["K"], d["cell"]
    T = d["max_T"] if wrong == "steps_beyond_seq" else h.T
    R, one = Rounding(u), V(1.0)
    f = lambda key: np.asarray(t[key], dtype=np.float64)  # noqa: E731
    x, w, r, dh, hp, hh = f("x"), f("w"), f("r"), f("dh"), f("hp")[0], f("h")
    rec = V(r if wrong == "recurrence_over_r_untransposed" and h.simple() else r.T)  # [q][k]: sum over q of delta[n][q] * r[k][q]
    delta, out = [None] * T, {}
    if h.simple():
        z = f("z")
        for s in range(T - 1, -1, -1):
            near = s - 1 if s > 0 else min(s + 1, T - 1)
            ap = R.act_prime(cell, V(z[near if wrong == "act_prime_of_the_neighbouring_step" else s]))
            if s == T - 1:
                delta[s] = R.mul(ap, V(dh[s]))
            else:
                delta[s] = R.mul(R.chain(None if wrong == "dout_without_dh" else V(dh[s]), delta[s + 1], rec), ap)
    else:
        gates = [f(key) for key in ("i", "f", "o", "ci", "co")]
        cs, csp, dcp = f("cs"), f("csp")[0], V(f("dcs")[0])
        for j in range(T - 1, -1, -1):
            gi, gf, go, gci, gco = (V(a[j]) for a in gates)
            if j == T - 1:
                dout = V(dh[j])
            else:
                dout = R.chain(None, delta[j + 1], rec)
                if wrong != "dout_without_dh":
                    dout = R.add(dout, V(dh[j]))
            dcp = R.add(dcp, R.mul(R.mul(dout, go), R.sub(one, R.mul(gco, gco))))
            dci = R.mul(R.mul(dcp, gi), R.sub(one, R.mul(gci, gci)))
            di = R.mul(R.mul(dcp, gci), R.mul(gi, R.sub(one, gi)))
            before = cs[j] if wrong == "df_from_cs_of_the_step" else (csp if j == 0 else cs[j - 1])
            df = R.mul(R.mul(dcp, V(before)), R.mul(gf, R.sub(one, gf)))
            dp = R.mul(R.mul(dout, gci if wrong == "dp_with_ci_for_co" else gco), R.mul(go, R.sub(one, go)))
            if not (wrong == "dcsp_without_f" and j == 0):
                dcp = R.mul(gf, dcp)
            delta[j] = hcat([di, dci, df, dp])  # the filters' column order: i, c, f, o
        if T > 0:
            out["dcsp"], out["dhp"] = dcp, R.chain(None, delta[0], rec)
    if T < 1:
        return {}
    filt = V((r[np.arange(C) % K] if wrong == "dx_over_r" else w).T)
    dx = [R.chain(None, delta[s], filt) for s in range(T)]
    out["dx"] = V(np.stack([s.v for s in dx]), np.stack([s.e for s in dx]))
    before = lambda s: (np.zeros_like(hp) if wrong == "hp_not_used_at_step_0" else hp) if s == 0 else hh[s - 1]  # noqa: E731
    order = range(T - 1, -1, -1)
    deltas = vcat([delta[s] for s in order])
    out["dw"] = R.chain(None, V(np.concatenate([x[s] for s in order], axis=0).T), deltas)
    out["dr"] = R.chain(None, V(np.concatenate([hh[s] if wrong == "dr_from_h_of_the_step" else before(s) for s in order], axis=0).T), deltas)
    if wrong == "dw_c_and_f_columns_swapped" and cell == LSTM:
        swap = np.concatenate([np.arange(K), np.arange(2 * K, 3 * K), np.arange(K, 2 * K), np.arange(3 * K, 4 * K)])
        out["dw"] = V(out["dw"].v[:, swap], out["dw"].e[:, swap])
    summed = vcat([delta[s] for s in order if not (wrong == "db_without_the_last_step" and s == T - 1)] or [V(np.zeros((1, h.G * K)))])
    db = R.chain(None, V(np.ones((1, summed.v.shape[0]))), summed)
    out["db"] = V(db.v[0], db.e[0])
    return {key: (out[key].v, out[key].e * SLACK) for key in written(cell, kind)}


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
    # the segment walk: 129 = 4 * 32 + 1 columns a segment, so every segment ends in the vector-ALU tail and the matrix steps resume
    c["oddseg8_lstm"] = desc(2, 8, 1032, 2, LSTM, bn=2, bc=8, bk=129)       # BF = 8: 32 segments
    c["maxseg_lstm"] = desc(2, 8, 2064, 2, LSTM, bn=2, bc=8, bk=129)        # BF = 16: 64 segments, the capacity of the segment array
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


# one handle run at the lengths 4, 1 and 3 in turn, and FWD followed by BWDUPD on one handle (tests/test_rnn_bwd_gpu.py): 37 rows (odd,
# beyond one chunk of the weight reduction), K beyond one tile, blocks of 0 (64 divides nothing here: all three warnings)
SEQ_CASES = {"seqlen_" + rc.CELL_NAMES[cell]: desc(37, 12, 70, 4, cell) for cell in (TANH, LSTM)}
SEQ_LENGTHS = (4, 1, 3)


# ---- the seeded sweep ---------------------------------------------------------------------------------------------------------------
SWEEP_COUNT = 32
SWEEP_THREADS = (1, 2, 3, 5)
CENSUS = ("N > 64", "N odd and > 32", "K > 64", "C > 64", "seq < max_T", "seq == 1 with max_T > 1", "bn does not divide or is 0",
          "bc does not divide or is 0", "bk does not divide or is 0", "a share begins inside a tile of 64 rows", "more threads than row blocks")


def sweep_cases_from(seed):
    """32 descriptors, 8 per cell, from one block of uniform numbers (one generator call a seed, so that looking for the seed is cheap);
    per case in this order: N in 1..70; C, then K: one in four from 65..150, else 1..80; max_T in 1..4; seq from {unset, 1..max_T};
    bn, bc, bk from the forward sweep's list (0, 1, n, the divisors of n from 2, n + 1, 7); threads from 1, 2, 3, 5"""
    u = np.random.default_rng(seed).random((SWEEP_COUNT, 11))
    pick = lambda x, seq: seq[min(int(x * len(seq)), len(seq) - 1)]  # noqa: E731
    extent = lambda wide, x: pick(x, range(65, 151)) if wide < 0.25 else pick(x, range(1, 81))  # noqa: E731
    blk = lambda x, n: pick(x, [0, 1, n] + [q for q in range(2, n + 1) if n % q == 0] + [n + 1, 7])  # noqa: E731
    cases = {}
    for idx in range(SWEEP_COUNT):
        cell, r = CELLS[idx % 4], [float(v) for v in u[idx]]
        N, Cc, K, T = pick(r[0], range(1, 71)), extent(r[1], r[2]), extent(r[3], r[4]), pick(r[5], range(1, 5))
        cases["sweep%02d_%s" % (idx, rc.CELL_NAMES[cell])] = desc(N, Cc, K, T, cell, bn=blk(r[7], N), bc=blk(r[8], Cc), bk=blk(r[9], K),
                                                                     threads=pick(r[10], SWEEP_THREADS), seq=pick(r[6], [-1] + list(range(1, T + 1))))
    return cases


def census(cases):
    """per cell, what the sweep is for -> the number of its cases that have it"""
    n = {cell: dict.fromkeys(CENSUS, 0) for cell in CELLS}
    for d in cases.values():
        h, c = rc.Handle(d), n[d["cell"]]
        shares = [s for s in h.shares() if s[1] > s[0]]
        c["N > 64"] += d["N"] > 64
        c["N odd and > 32"] += d["N"] % 2 == 1 and d["N"] > 32
        c["K > 64"] += d["K"] > 64
        c["C > 64"] += d["C"] > 64
        c["seq < max_T"] += 0 <= d["seq"] < d["max_T"]
        c["seq == 1 with max_T > 1"] += d["seq"] == 1 and d["max_T"] > 1
        for key, ext in (("bn", "N"), ("bc", "C"), ("bk", "K")):
            c[key + " does not divide or is 0"] += d[key] == 0 or d[ext] % d[key] != 0
        c["a share begins inside a tile of 64 rows"] += d["threads"] > 1 and any(s[0] % 64 for s in shares)
        c["more threads than row blocks"] += d["threads"] > d["N"] // h.bn
    return n


def census_passes(cases):
    return all(v >= 1 for c in census(cases).values() for v in c.values())


# the first seed whose census passes and whose backward pass meets no hard transcendental (tests/test_rnn_bwd_cpu.py asserts both)
SWEEP_SEED = 41
# the seeds below SWEEP_SEED whose census passes, each with the transcendental that rules it out: (seed, case, "exp" or "tanh", argument)
SWEEP_SEEDS_RULED_OUT = ()


@functools.lru_cache(maxsize=None)
def sweep_cases():
    return sweep_cases_from(SWEEP_SEED)


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


def case(name):
    """the descriptor of any named case that is computed"""
    for cases in (all_cases(), THREAD_CASES, SEQ_CASES, sweep_cases()):
        if name in cases:
            return cases[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, kind, threads1=True, seq=None):
    """(inputs, gradient tensors) of a case under a kind, computed once and left unchanged; seq: another sequence length on the same
    inputs (the forward tensors of the case's own length, of which a shorter pass reads its first steps)"""
    d = case(name)
    if threads1:
        d = dict(d, threads=1)
    if seq is not None:
        d = dict(d, seq=seq)
    t = cached_inputs(name)
    return t, backward(rc.Handle(d), t, kind)


@functools.lru_cache(maxsize=None)
def cached_inputs(name):
    return inputs(name, dict(case(name), threads=1))
