"""What the low-precision GEMM tests share: input generators, the numpy reference and the pair-packed reading of A.

The reference is a loop over k, vectorised over m x n, in the arithmetic of the oracle's gold loops (xo_gemm_lowp with
scf = 1): kind 0 the wrapping 32-bit sum of the 32-bit products, kind 1 acc = acc + float32(product), kind 2
acc = acc + a * b on the widened bf16 operands, every float32 operation rounded on its own. tests/test_lowp_gemm_cpu.py
pins it against the oracle at even k and no transpose, which is all the oracle computes."""
import numpy as np

KINDS = (0, 1, 2)  # i16 -> i32, i16 -> f32, bf16 -> f32 (the kinds of xo_gemm_lowp)
NAMES = {0: "tgemm_i16i32_", 1: "tgemm_i16f32_", 2: "tgemm_bf16_"}


def precisions(xs, kind):
    return ((xs.I16, xs.I32), (xs.I16, xs.F32), (xs.BF16, xs.F32))[kind]


def out_dtype(kind):
    return np.int32 if kind == 0 else np.float32


def widen(x):
    """bf16 bit patterns (uint16) -> float32"""
    return (x.astype(np.uint32) << 16).view(np.float32)


def rand_bf16(rng, count):
    """mixed signs and exponents (2^-6 ... 2^6: no product underflows), the full 8-bit significand"""
    v = rng.uniform(0.5, 1.0, count) * np.exp2(rng.integers(-6, 7, count)) * rng.choice([-1.0, 1.0], count)
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def rand_inputs(rng, kind, count):
    if kind == 2:
        return rand_bf16(rng, count)
    return rng.integers(-32768, 32768, count).astype(np.int16).view(np.uint16)  # the full range: the i32 sum wraps


def rand_c(rng, kind, count):
    if kind == 0:
        return rng.integers(-2 ** 31, 2 ** 31, count).astype(np.int32)
    return rng.uniform(-4, 4, count).astype(np.float32)


def op(x, ld, rows, cols, trans):
    """op(X) as a rows x cols array from flat column-major storage (trans: X is stored cols x rows)"""
    if trans:
        return x.reshape(rows, ld)[:, :cols].copy()
    return x.reshape(cols, ld)[:, :rows].T.copy()


def reference(kind, ta, tb, m, n, k, a, lda, b, ldb, beta, c, ldc):
    """-> the expected C (flat, ldc * n, what lies between m and ldc unchanged)"""
    A, B = op(a, lda, m, k, ta), op(b, ldb, k, n, tb)
    out = c.copy()
    tile = out.reshape(n, ldc)[:, :m].T
    if kind == 0:
        A, B = A.view(np.int16).astype(np.int64), B.view(np.int16).astype(np.int64)
        acc = tile.astype(np.int64) & 0xFFFFFFFF if beta else np.zeros((m, n), np.int64)
        for kk in range(k):
            acc = (acc + A[:, kk, None] * B[None, kk, :]) & 0xFFFFFFFF
        res = acc.astype(np.uint32).view(np.int32)
    elif kind == 1:
        A, B = A.view(np.int16).astype(np.int32), B.view(np.int16).astype(np.int32)
        acc = tile.copy() if beta else np.zeros((m, n), np.float32)
        for kk in range(k):
            acc = acc + (A[:, kk, None] * B[None, kk, :]).astype(np.float32)
        res = acc
    else:
        A, B = widen(A), widen(B)
        acc = tile.copy() if beta else np.zeros((m, n), np.float32)
        for kk in range(k):
            acc = acc + A[:, kk, None] * B[None, kk, :]
        res = acc
    assert res.dtype == out.dtype
    out.reshape(n, ldc)[:, :m] = res.T
    return out


def pairs_gold(kind, beta0, m, n, k, lda, ldb, ldc, a, b, c, scf):
    """the gold loops of the dispatched kernels (A in pairs of k; tests/test_lowp.py pins the oracle with them), vectorised over the C tile: one term after the other in ascending k, every step rounded to
    float32 (numpy float32 arithmetic rounds each operation)."""
    out = c.copy()
    A = a.reshape(k // 2, lda, 2)   # a[(s*lda + i)*2 + k2]
    B = b.reshape(n, ldb)           # b[j*ldb + kk]
    C2 = out.reshape(n, ldc)
    if kind == 0:
        acc = np.zeros((n, m), dtype=np.int64) if beta0 else C2[:, :m].astype(np.int64)
        for kk in range(k):
            acc += np.outer(B[:, kk].view(np.int16).astype(np.int64), A[kk // 2, :m, kk % 2].view(np.int16).astype(np.int64))
        C2[:, :m] = (acc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        return out
    if kind == 3:
        acc = np.zeros((n, m), dtype=np.float32) if beta0 else widen(C2[:, :m])
    else:
        acc = np.zeros((n, m), dtype=np.float32) if beta0 else C2[:, :m].astype(np.float32)
    for kk in range(k):
        if kind == 1:
            iprod = np.outer(B[:, kk].view(np.int16).astype(np.int32), A[kk // 2, :m, kk % 2].view(np.int16).astype(np.int32))
            term = (iprod.astype(np.float32) * np.float32(scf)).astype(np.float32)
        else:
            term = np.outer(widen(B[:, kk]), widen(A[kk // 2, :m, kk % 2])).astype(np.float32)
        acc = (acc + term).astype(np.float32)
    C2[:, :m] = (np.ascontiguousarray(acc, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16) if kind == 3 else acc
    return out


def pack_pairs(a, lda, m, k):
    """plain column-major A (m x k, lda) -> the reading of the dispatched kernels: a[(kk/2)*lda*2 + i*2 + kk%2]"""
    assert k % 2 == 0
    plain = a.reshape(k, lda)
    return plain.reshape(k // 2, 2, lda).transpose(0, 2, 1).copy().ravel()


def bits(x):
    return x.view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


class Case(object):
    """operands of one product in host memory (flat, column major, leading dimensions padded by `pad`) and its reference"""

    def __init__(self, kind, trans, m, n, k, beta, pad=3, seed=0, a=None, b=None, c=None):
        rng = np.random.default_rng(seed)
        self.kind, self.trans, self.m, self.n, self.k, self.beta = kind, trans, m, n, k, beta
        self.ta, self.tb = trans[0] == "T", trans[1] == "T"
        self.lda = (k if self.ta else m) + pad
        self.ldb = (n if self.tb else k) + pad
        self.ldc = m + pad
        self.a = rand_inputs(rng, kind, self.lda * (m if self.ta else k)) if a is None else a
        self.b = rand_inputs(rng, kind, self.ldb * (k if self.tb else n)) if b is None else b
        self.c = rand_c(rng, kind, self.ldc * n) if c is None else c
        self._gold = None

    @property
    def gold(self):
        if self._gold is None:
            self._gold = reference(self.kind, self.ta, self.tb, self.m, self.n, self.k, self.a, self.lda, self.b, self.ldb, self.beta, self.c, self.ldc)
        return self._gold

    def run(self, xs, a, b, c, tid=None, nthreads=None):
        ip, op_ = precisions(xs, self.kind)
        args = (ip, op_, self.trans[0], self.trans[1], self.m, self.n, self.k, a, self.lda, b, self.ldb, self.beta, c, self.ldc)
        if tid is None:
            return xs.gemm_lowp(*args)
        return xs.gemm_lowp_thread(*(args + (tid, nthreads)))

    def on_device(self, torch):
        return [torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x.copy()).cuda() for x in (self.a.copy(), self.b.copy(), self.c)]

    def run_device(self, xs, torch, tasks=None):
        da, db, dc = self.on_device(torch)
        for task in (tasks if tasks is not None else [None]):
            rc = self.run(xs, da, db, dc) if task is None else self.run(xs, da, db, dc, task[0], task[1])
            assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(da.cpu().numpy().view(np.uint16), self.a) and np.array_equal(db.cpu().numpy().view(np.uint16), self.b)
        return dc.cpu().numpy()
