"""Shared by tests/test_packed_cpu.py, tests/test_packed_chain_cpu.py and tests/test_packed_gpu.py: random cases for the packed kernels (pgemm, getrf, trmm,
trsm over packs of interleaved matrices), a plain numpy implementation of the four operations in the kernel's own type, and
the componentwise backward-error bounds every result must meet.

The bounds are the textbook ones (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.: eq. 3.13 for inner
products, Thm 8.5 for substitution, Thm 9.3 for LU), with u the unit round-off of the kernel's type and
gamma_p = p u / (1 - p u); the +1 / +2 cover the scaling by alpha and a rounded reciprocal of the pivot:
    pgemm  |C^ - (C0 + alpha op(A) op(B))| <= gamma_{k+1} (|C0| + |op(A)| |op(B)|)
    trmm   |B^ - alpha op(T) B0|           <= gamma_{nT+1} |alpha| |op(T)| |B0|             (side R likewise)
    trsm   |op(T) X^ - alpha B0|           <= gamma_{nT+2} (|op(T)| |X^| + |alpha| |B0|)
    getrf  |L^ U^ - A0|                    <= gamma_{min(m,n)+2} |L^| |U^|
The left sides are evaluated from the kernel's output in the next wider type (float64 for fp32, numpy.longdouble for fp64; if
longdouble is no wider than float64 on the machine, exactly with fractions.Fraction on the first 64 matrices)."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np

PGEMM, GETRF, TRMM, TRSM = 3, 4, 5, 6
KIND_NAME = {PGEMM: "pgemm", GETRF: "getrf", TRMM: "trmm", TRSM: "trsm"}
COL, ROW = 102, 101
GUARD = 96  # elements of canary before and after every operand
LONGDOUBLE_IS_WIDER = bool(np.finfo(np.longdouble).eps < 2.0 ** -60)


def canary(dtype):
    """a NaN with a payload: arithmetic on it shows in the result, a store over it shows in the bits"""
    return np.array([0x7FC0DEAD], dtype=np.uint32).view(np.float32)[0] if np.dtype(dtype) == np.float32 else \
        np.array([0x7FF8DEADBEEF0BAD], dtype=np.uint64).view(np.float64)[0]


class Case:
    """one descriptor with nmat random matrices; operands as (nmat, rows, cols) arrays (a, b, c as the kernel takes them)"""

    def __init__(self, kind, dtype, m, n, k=0, layout=COL, transa="N", transb="N", side="L", uplo="L", diag="N", alpha=1.0, pad=0,
                 nmat=8, seed=0):
        self.kind, self.dtype, self.m, self.n, self.k, self.layout = kind, np.dtype(dtype), m, n, k, layout
        self.transa, self.transb, self.side, self.uplo, self.diag, self.alpha, self.nmat = transa, transb, side, uplo, diag, alpha, nmat
        rng = np.random.default_rng(seed)
        rnd = lambda *shape: rng.uniform(-1.0, 1.0, size=(nmat,) + shape).astype(self.dtype)
        lead = lambda rows, cols: (rows if layout == COL else cols) + pad
        self.ops = {}   # name -> (nmat, rows, cols) array as stored
        if kind == PGEMM:
            self.ops["a"] = rnd(k, m) if transa == "T" else rnd(m, k)
            self.ops["b"] = rnd(n, k) if transb == "T" else rnd(k, n)
            self.ops["c"] = rnd(m, n)
            self.written = "c"
        elif kind == GETRF:
            a = rnd(m, n)
            d = min(m, n)  # strictly diagonally dominant by columns: LU without pivoting exists
            colsum = np.abs(a).sum(axis=1)
            idx = np.arange(d)
            a[:, idx, idx] = (colsum[:, :d] + 1.0) * np.where(rng.random((nmat, d)) < 0.5, -1.0, 1.0)
            self.ops["a"] = a.astype(self.dtype)
            self.written = "a"
        else:
            nt = n if side == "R" else m
            t = rnd(nt, nt)
            idx = np.arange(nt)
            if kind == TRSM:  # |t_ii| >= 1
                t[:, idx, idx] = np.where(t[:, idx, idx] < 0, t[:, idx, idx] - 1.0, t[:, idx, idx] + 1.0)
            # what is never read holds NaN: the strict other triangle, and the diagonal of a unit triangle
            other = np.triu(np.ones((nt, nt), bool), 1) if uplo == "L" else np.tril(np.ones((nt, nt), bool), -1)
            if diag == "U":
                other |= np.eye(nt, dtype=bool)
            t[:, other] = np.nan
            self.ops["a"] = t
            self.ops["b"] = rnd(m, n)
            self.written = "b"
        self.ld = {name: lead(*x.shape[1:]) for name, x in self.ops.items()}

    # ---- the descriptor through the C-ABI ----
    def dispatch(self, xs):
        blob, d = xs.packed_descriptor(self.kind, self.dtype.itemsize, self.m, self.n, self.k, lda=self.ld.get("a"), ldb=self.ld.get("b"),
                                       ldc=self.ld.get("c"), alpha=self.alpha, transa=self.transa, transb=self.transb, side=self.side,
                                       uplo=self.uplo, diag=self.diag, layout=self.layout)
        assert d, "descriptor init failed"
        fn = xs.packed_dispatch(self.kind, d)
        assert fn, "dispatch returned NULL for %r" % (self,)
        return fn

    def __repr__(self):
        return "%s %s m=%d n=%d k=%d layout=%d %s%s %s%s%s alpha=%g ld=%s nmat=%d" % (
            KIND_NAME[self.kind], self.dtype.name, self.m, self.n, self.k, self.layout, self.transa, self.transb, self.side, self.uplo, self.diag,
            self.alpha, self.ld, self.nmat)

    # ---- packed buffers with guard zones ----
    def buffers(self, xs):
        """name -> flat array: GUARD canaries, the packs back to back (padding = canaries), GUARD canaries"""
        g = np.full(GUARD, canary(self.dtype), dtype=self.dtype)
        return {name: np.concatenate([g, xs.pack(x, self.ld[name], self.layout, fill=canary(self.dtype)), g]) for name, x in self.ops.items()}

    def pack_elems(self, name):
        rows, cols = self.ops[name].shape[1:]
        return self.ld[name] * (cols if self.layout == COL else rows) * (64 // self.dtype.itemsize)

    def valid_mask(self, xs, name):
        """True where the buffer of operand `name` holds an element of a matrix"""
        x = self.ops[name]
        z = np.zeros(GUARD, self.dtype)
        body = xs.pack(np.ones_like(x), self.ld[name], self.layout, fill=0)
        return np.concatenate([z, body, z]) != 0

    def result(self, xs, buf):
        """the written operand's matrices out of its buffer"""
        x = self.ops[self.written]
        return xs.unpack(buf[GUARD:-GUARD], self.nmat, x.shape[1], x.shape[2], self.ld[self.written], self.layout)

    def chain(self, xs, orc):
        """the oracle's ordered chain (oracle/xsmm_oracle.c: xo_packed_*) in place on buffers(), canaries included: the buffers
        after the call. Every kernel result is held against the written one bit for bit."""
        bufs = self.buffers(xs)
        v = 64 // self.dtype.itemsize
        npacks = (self.nmat + v - 1) // v
        at = {name: x[GUARD:] for name, x in bufs.items()}
        ld = self.ld
        if self.kind == PGEMM:
            rc = orc.packed_pgemm(v, self.layout, self.m, self.n, self.k, ld["a"], ld["b"], ld["c"], self.transa, self.transb, self.alpha,
                                  at["a"], at["b"], at["c"], npacks)
        elif self.kind == GETRF:
            rc = orc.packed_getrf(v, self.layout, self.m, self.n, ld["a"], at["a"], npacks)
        else:
            f = orc.packed_trmm if self.kind == TRMM else orc.packed_trsm
            rc = f(v, self.layout, self.m, self.n, ld["a"], ld["b"], self.side, self.uplo, self.transa, self.diag, self.alpha, at["a"], at["b"], npacks)
        assert rc == 0, "the oracle refused %r" % (self,)
        return bufs

    def untouched(self, xs, before, after):
        """every operand's canaries (guards, padding) and everything that is only read keep their bits; returns a message or None"""
        bits = np.uint32 if self.dtype == np.float32 else np.uint64
        for name in self.ops:
            same = before[name].view(bits) == after[name].view(bits)
            keep = np.ones(same.shape, bool) if name != self.written else ~self.valid_mask(xs, name)
            if not np.all(same[keep]):
                return "operand %s: %d elements outside the result changed" % (name, int(np.count_nonzero(~same[keep])))
        return None

    # ---- mathematics ----
    def op_t(self, wide):
        """op(T) with explicit zeros / unit diagonal, in type `wide`"""
        t = widen(self.ops["a"], wide)
        nt = t.shape[1]
        tri = np.tril(np.ones((nt, nt), bool), -1) if self.uplo == "L" else np.triu(np.ones((nt, nt), bool), 1)
        out = np.where(tri, t, zero_like(t))
        idx = np.arange(nt)
        out[:, idx, idx] = one_like(t) if self.diag == "U" else t[:, idx, idx]
        return out.transpose(0, 2, 1) if self.transa == "T" else out

    def reference(self):
        """the operation lane by lane in the kernel's own type (plain numpy: multiply, then add)"""
        dt = self.dtype.type
        al = dt(self.alpha)
        if self.kind == PGEMM:
            a = self.ops["a"].transpose(0, 2, 1) if self.transa == "T" else self.ops["a"]
            b = self.ops["b"].transpose(0, 2, 1) if self.transb == "T" else self.ops["b"]
            c = self.ops["c"].copy()
            for l in range(self.k):
                c = c + al * a[:, :, l, None] * b[:, None, l, :]
            return c
        if self.kind == GETRF:
            a = self.ops["a"].copy()
            for p in range(min(self.m, self.n)):
                rinv = dt(1) / a[:, p, p]
                a[:, p + 1:, p] = a[:, p + 1:, p] * rinv[:, None]
                a[:, p + 1:, p + 1:] = a[:, p + 1:, p + 1:] - a[:, p + 1:, p, None] * a[:, None, p, p + 1:]
            return a
        with np.errstate(invalid="ignore"):
            e = np.nan_to_num(self.op_t(self.dtype), nan=0.0)
        b = self.ops["b"]
        if self.side == "R":  # X op(T) = alpha B  <=>  op(T)^T X^T = alpha B^T
            e, b = e.transpose(0, 2, 1), b.transpose(0, 2, 1)
        nt = e.shape[1]
        lower = (self.uplo == "L") ^ (self.transa == "T") ^ (self.side == "R")
        if self.kind == TRMM:
            x = (al * np.matmul(e, b)).astype(self.dtype)
        else:
            x = (al * b).astype(self.dtype)
            for c in (range(nt) if lower else range(nt - 1, -1, -1)):
                x[:, c, :] = x[:, c, :] * (dt(1) / e[:, c, c])[:, None]
                rows = slice(c + 1, nt) if lower else slice(0, c)
                x[:, rows, :] = x[:, rows, :] - e[:, rows, c, None] * x[:, None, c, :]
        return np.ascontiguousarray(x.transpose(0, 2, 1) if self.side == "R" else x)

    def check(self, out):
        """the bound of the module's docstring for every element of every matrix; returns (worst ratio residual / bound, message or None)"""
        if not np.all(np.isfinite(out)):
            return np.inf, "%d results are not finite" % int(np.count_nonzero(~np.isfinite(out)))
        wide = np.float64 if self.dtype == np.float32 else (np.longdouble if LONGDOUBLE_IS_WIDER else object)
        sel = slice(None) if wide is not object else slice(0, 64)
        w = lambda x: widen(x[sel], wide)
        u = w(np.array([2.0 ** -24 if self.dtype == np.float32 else 2.0 ** -53]))[0]
        gamma = lambda p: (p * u) / (1 - p * u)
        al = w(np.array([self.alpha], dtype=self.dtype))[0]
        o = w(out)
        if self.kind == PGEMM:
            a = w(self.ops["a"]); b = w(self.ops["b"]); c0 = w(self.ops["c"])
            a = a.transpose(0, 2, 1) if self.transa == "T" else a
            b = b.transpose(0, 2, 1) if self.transb == "T" else b
            res = abs(o - (c0 + al * np.matmul(a, b)))
            bound = gamma(self.k + 1) * (abs(c0) + np.matmul(abs(a), abs(b)))
        elif self.kind == GETRF:
            d = min(self.m, self.n)
            low = np.tril(np.ones((self.m, d), bool), -1)
            lo = np.where(low, o[:, :, :d], zero_like(o[:, :, :d]))
            idx = np.arange(d)
            lo[:, idx, idx] = one_like(o)
            up = np.where(np.triu(np.ones((d, self.n), bool)), o[:, :d, :], zero_like(o[:, :d, :]))
            res = abs(np.matmul(lo, up) - w(self.ops["a"]))
            bound = gamma(d + 2) * np.matmul(abs(lo), abs(up))
        else:
            sub = Case.__new__(Case); sub.__dict__.update(self.__dict__); sub.ops = {"a": self.ops["a"][sel]}
            t = sub.op_t(wide)
            b0 = w(self.ops["b"])
            nt = t.shape[1]
            mm = (lambda x, y: np.matmul(x, y)) if self.side == "L" else (lambda x, y: np.matmul(y, x))
            if self.kind == TRMM:
                res = abs(o - al * mm(t, b0))
                bound = gamma(nt + 1) * abs(al) * mm(abs(t), abs(b0))
            else:
                res = abs(mm(t, o) - al * b0)
                bound = gamma(nt + 2) * (mm(abs(t), abs(o)) + abs(al) * abs(b0))
        bad = res > bound
        r, b = worst(res, bound)
        ratio = float(r / b) if b != 0 else (0.0 if r == 0 else np.inf)
        if np.any(bad):
            i = np.argwhere(bad)[0]
            return ratio, "%d of %d elements beyond the bound; first at %s: residual %.3e, bound %.3e" % (
                int(np.count_nonzero(bad)), bad.size, tuple(int(v) for v in i), float(res[tuple(i)]), float(bound[tuple(i)]))
        return ratio, None


def worst(res, bound):
    """the element with the largest residual relative to its bound"""
    flat_r, flat_b = res.reshape(-1), bound.reshape(-1)
    if res.dtype == object:
        best = max(range(flat_r.size), key=lambda i: (flat_r[i] / flat_b[i]) if flat_b[i] != 0 else (0 if flat_r[i] == 0 else 10 ** 9))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(flat_b != 0, flat_r / np.where(flat_b != 0, flat_b, 1), np.where(flat_r == 0, 0, np.inf))
        best = int(np.argmax(q))
    return flat_r[best], flat_b[best]


def widen(x, wide):
    if wide is object:
        flat = [Fraction(float(v)) if np.isfinite(v) else Fraction(0) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
        return np.array(flat, dtype=object).reshape(np.shape(x))  # (NaN only where op_t masks it out)
    return np.asarray(x).astype(wide)


def zero_like(x):
    return Fraction(0) if x.dtype == object else x.dtype.type(0)


def one_like(x):
    return Fraction(1) if x.dtype == object else x.dtype.type(1)


# ---- the cases of the GPU sweeps (tests/test_packed_gpu.py runs them on the kernels, tests/test_packed_chain_cpu.py on the oracle) ----
SIZES = (1, 2, 3, 5, 8, 13, 16, 23, 32)
RECT = ((1, 32), (32, 1), (2, 13), (13, 2), (3, 23), (23, 5), (5, 16), (16, 8), (8, 3), (32, 13), (13, 32), (23, 16))
PACKS = (1, 7, 8, 9)
FLAGS = list(itertools.product("LR", "LU", "NT", "NU"))
MNK = [(s, s, s) for s in SIZES] + [(1, 32, 5), (32, 1, 13), (2, 13, 32), (13, 2, 1), (3, 23, 16), (23, 5, 8), (5, 16, 3), (16, 8, 23), (8, 3, 2)]


def width(dtype):
    """matrices per pack: a line of a pack is 64 bytes per element (libxsmm_amd_packed_width)"""
    return 64 // np.dtype(dtype).itemsize


def flag_sweep(kind, dtype, layout):
    """the sixteen flag combinations, each on a tight and a padded shape (shapes, alpha and pack counts rotate through their sets)"""
    v = width(dtype)
    shapes = [(s, s) for s in SIZES] + list(RECT)
    out = []
    for i, (side, uplo, trans, diag) in enumerate(FLAGS):
        for j, pad in enumerate((0, 3)):
            m, n = shapes[(2 * i + j + (7 if kind == TRMM else 0)) % len(shapes)]
            out.append(Case(kind, dtype, m, n, layout=layout, side=side, uplo=uplo, transa=trans, diag=diag, alpha=(1.0, -1.0, 0.75)[(i + j) % 3],
                            pad=pad, nmat=v * PACKS[(i + j) % 4], seed=100 * i + j))
    return out


def shape_sweep(kind, dtype, layout):
    """every square size and the rectangular ones, tight and padded in turn, flags rotating"""
    v = width(dtype)
    out = []
    for i, (m, n) in enumerate([(s, s) for s in SIZES] + list(RECT)):
        side, uplo, trans, diag = FLAGS[(5 * i + 3) % 16]
        out.append(Case(kind, dtype, m, n, layout=layout, side=side, uplo=uplo, transa=trans, diag=diag, alpha=(0.75, 1.0, -1.0)[i % 3],
                        pad=(0, 5)[i % 2], nmat=v * PACKS[i % 4], seed=7 * i))
    return out


def pgemm_sweep(dtype, layout):
    """every trans and alpha, tight and padded; then every shape once more with rotating flags"""
    v = width(dtype)
    out = []
    for i, (ta, tb, alpha) in enumerate(itertools.product("NT", "NT", (1.0, -1.0))):
        for j, pad in enumerate((0, 2)):
            m, n, k = MNK[(2 * i + j) % len(MNK)]
            out.append(Case(PGEMM, dtype, m, n, k, layout=layout, transa=ta, transb=tb, alpha=alpha, pad=pad, nmat=v * PACKS[(i + j) % 4], seed=i))
    for i, (m, n, k) in enumerate(MNK):
        ta, tb = "NT"[i % 2], "NT"[(i // 2) % 2]
        out.append(Case(PGEMM, dtype, m, n, k, layout=layout, transa=ta, transb=tb, alpha=(1.0, -1.0)[i % 2], pad=(4, 0)[i % 2], nmat=v * PACKS[i % 4], seed=50 + i))
    return out


ONE_ANSWER = [(TRSM, 8, 8, 0, dict(side="L", uplo="L")), (TRSM, 13, 5, 0, dict(side="R", uplo="U", transa="T", alpha=0.75, pad=3)),
              (TRMM, 8, 16, 0, dict(uplo="U", diag="U", alpha=-1.0)), (GETRF, 8, 8, 0, dict()), (GETRF, 16, 13, 0, dict(pad=1)),
              (PGEMM, 8, 8, 8, dict(alpha=-1.0)), (PGEMM, 5, 16, 13, dict(transa="T", pad=2))]


def one_answer_case(kind, m, n, k, kw, dtype):
    return Case(kind, dtype, m, n, k, nmat=1000 * width(dtype), seed=11, layout=ROW if kw.get("pad") else COL, **kw)


RESIDENT_CASES = [(TRSM, 8, 8, 0, dict(side="R", uplo="U", alpha=0.75)), (TRSM, 5, 8, 0, dict(transa="T", alpha=-1.0)), (TRMM, 8, 5, 0, dict(uplo="U")),
                  (TRMM, 3, 8, 0, dict(side="R", diag="U", alpha=0.75)), (GETRF, 8, 8, 0, dict()), (GETRF, 5, 8, 0, dict()), (PGEMM, 8, 5, 8, dict(alpha=-1.0, transb="T"))]


def resident_case(kind, m, n, k, kw, dtype, layout):
    return Case(kind, dtype, m, n, k, nmat=9 * width(dtype), seed=21, layout=layout, pad=(1 if layout == ROW else 0), **kw)


UNALIGNED_CASES = [(TRSM, 8, 5, 0, dict(uplo="U", pad=2)), (TRMM, 13, 3, 0, dict()), (GETRF, 8, 8, 0, dict(pad=1)), (PGEMM, 5, 8, 3, dict())]


def unaligned_case(kind, m, n, k, kw, dtype):
    return Case(kind, dtype, m, n, k, nmat=9 * width(dtype), seed=31, **kw)


def redispatch_case(kind):
    return Case(kind, np.float32, 5, 3, 2, nmat=16, seed=2)


# ---- operands past 2^31 elements and 2^32 bytes (tests/test_wide_offsets_gpu.py; the offsets are checked in tests/test_packed_chain_cpu.py) ----
WIDE_LD, WIDE_LINES = 4096, 32  # the largest leading dimension (PK_MAXLD), column major, 32 columns: a pack spans 2^21 fp32 elements
# (id, kind, type, m, n, k, the wide operand, packs, flags)
WIDE_CASES = [("getrf-a", GETRF, np.float32, 2, 32, 0, "a", 1026, dict()),
              ("trsm-b", TRSM, np.float32, 4, 32, 0, "b", 1026, dict(side="L", uplo="L", transa="N", diag="N")),
              ("pgemm-c", PGEMM, np.float32, 2, 32, 2, "c", 1026, dict()),
              ("pgemm-a", PGEMM, np.float32, 2, 2, 32, "a", 1026, dict()),
              ("trmm-b", TRMM, np.float64, 4, 32, 0, "b", 520, dict())]


# ---- the caller's loop over packs, in C(a Python loop is too slow to keep a burst of deferred calls open) ----
LOOP_C = r"""
typedef void (*fn3)(const void*, const void*, void*);
void pack_loop(fn3 f, const char* a, const char* b, char* c, long long sa, long long sb, long long sc, long long n)
{ long long i; for (i = 0; i < n; ++i) f(a ? a + i * sa : 0, b ? b + i * sb : 0, c ? c + i * sc : 0); }
"""


def build_loop(directory):
    import subprocess
    src = directory / "pack_loop.c"
    src.write_text(LOOP_C)
    so = directory / "pack_loop.so"
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.pack_loop.argtypes = [C.c_void_p] * 4 + [C.c_longlong] * 4
    lib.pack_loop.restype = None
    return lib


def call_args(case, ptrs):
    """(a, b, c, byte strides) of the kernel call for the operands' base addresses: getrf is kernel(A, A, NULL), the third argument
    of trmm / trsm is NULL"""
    ts = case.dtype.itemsize
    off = GUARD * ts
    st = {name: case.pack_elems(name) * ts for name in case.ops}
    if case.kind == PGEMM:
        return (ptrs["a"] + off, ptrs["b"] + off, ptrs["c"] + off, st["a"], st["b"], st["c"])
    if case.kind == GETRF:
        return (ptrs["a"] + off, ptrs["a"] + off, None, st["a"], st["a"], 0)
    return (ptrs["a"] + off, ptrs["b"] + off, None, st["a"], st["b"], 0)
