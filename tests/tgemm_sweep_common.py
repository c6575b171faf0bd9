"""The seeded sweep of the tiled GEMM (kernels/tgemm.hip) and of the GEMM with 16-bit inputs (kernels/tgemm_lowp.hip): the drawn
cases, their operand buffers, the expected bits, a restatement of the product that can carry one mistake, and the float64 contract.
tests/test_tgemm_sweep_cpu.py holds the expectation to the contract and counts what the set holds; tests/test_tgemm_sweep_gpu.py
demands the bits of the kernels. DESIGN.md 8v.

A case is a dict: kind (one of KINDS), trans ("NN", "TN", "NT", "TT": transa, transb), beta, m, n, k, pads and offs (of A, B, C:
ld = extent + pad, and the operand starts offs elements into its allocation), nthreads, order (the task ids in the order they
run) and mem (of A, B, C: "device", "pinned", "pageable").

The drawing is dealt, not independent. Twelve cases per kind cannot hold two cases each of k = BK, k = 2 BK, k below the
instruction depth and a tail behind a chunk multiple by chance (fp64 has three tails, which alone makes twelve), nor two each of
the three extents around a kind's instruction tile, so per kind those values are cards of a deck that is shuffled over the kind's
cases; what a deck leaves free is drawn as the edge list or the value list against a uniform value, by a coin. The transposes and
beta are dealt as well (every pair of kind and transposes three times, with both betas). Everything else is drawn case by case, and
tests/test_tgemm_sweep_cpu.py::census says what the set has to hold by chance: the seed is the first from 0 up that passes it."""
import functools
import os
import re

import numpy as np

import lowp_gemm_common as lg
import oracle_binding as orc
from test_lowp_gemm_gpu import small_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "libxsmm-1_amd", "csrc", "kernels")

KINDS = ("f32", "f64", "i16i32", "i16f32", "bf16", "bf16fast")
TRANS = ("NN", "TN", "NT", "TT")
LOWP = {"i16i32": 0, "i16f32": 1, "bf16": 2, "bf16fast": 2}  # the kind of lowp_gemm_common (the fast mode is a switch of kind 2)
KERNEL = {"f32": "tgemm_f32_", "f64": "tgemm_f64_", "i16i32": "tgemm_i16i32_", "i16f32": "tgemm_i16f32_", "bf16": "tgemm_bf16_",
          "bf16fast": "tgemm_bf16fast_"}
EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
MAX_MN, MAX_K = 300, 200
PADS = (0, 1, 3, 5, 8)
MEMS = ("device", "pinned", "pageable")
SWEEP_SEED, SWEEP_CASES = 4, 72
GUARD = 16            # elements of the canary band on either side of an operand
CANARY = 0xA5         # every byte of a band, and of the elements in front of an operand's offset
TILE = 128            # the work-group tile, xsmm::TGEMM_TILE (tests/test_tgemm_sweep_cpu.py asks libxsmm_amd_gemm_tile)


def _find(path, pattern):
    with open(os.path.join(KERNELS, path)) as f:
        found = re.findall(pattern, f.read(), re.S)
    assert 1 == len(found), (path, pattern, found)
    return tuple(int(v) for v in found[0]) if isinstance(found[0], tuple) else int(found[0])


@functools.lru_cache(maxsize=None)
def geometry():
    """kind -> (D, BK, TS): the depth of the kind's arithmetic step, its k chunk and the extent of its instruction tile (None on the
    vector ALU), read from where the kernels define them, so that no second copy exists: the instruction traits of tile_gemm.cuh,
    Cfg of tgemm.hip, and for the 16-bit kinds libxsmm_amd_lowp_gemm_chunk (bf16 exact runs the fp32 instruction, the i16 kinds
    step by the two elements of a 32-bit k pair, the fast mode by the depth its instruction has in its name)."""
    import importlib
    xs = importlib.import_module("libxsmm-1_amd")
    if not os.path.exists(xs.LIB_PATH):
        xs.build()
    chunk = xs.lib().libxsmm_amd_lowp_gemm_chunk
    t32, d32 = _find("tile_gemm.cuh", r"struct MfmaF32 \{.*?TS = (\d+), DEPTH = (\d+)")
    t64, d64 = _find("tile_gemm.cuh", r"struct MfmaF64 \{.*?TS = (\d+), DEPTH = (\d+)")
    fast = _find("tgemm_lowp.hip", r"= __builtin_amdgcn_mfma_f32_32x32x(\d+)_bf16\(")
    pair = np.dtype(np.uint32).itemsize // np.dtype(np.uint16).itemsize
    return {"f32": (d32, _find("tgemm.hip", r"struct Cfg<float> \{[^}]*?BK = (\d+)"), t32),
            "f64": (d64, _find("tgemm.hip", r"struct Cfg<double> \{[^}]*?BK = (\d+)"), t64),
            "i16i32": (pair, chunk(xs.I16), None), "i16f32": (pair, chunk(xs.I16), None),
            "bf16": (d32, chunk(xs.BF16), t32), "bf16fast": (fast, chunk(xs.BF16), t32)}


def k_values(kind):
    """the value list of k for a kind, in its instruction depth and chunk"""
    D, BK, _ = geometry()[kind]
    vals = [1, D - 1, D, D + 1, BK - 1, BK, BK + 1, 2 * BK - 1, 2 * BK, 2 * BK + 1, 2 * BK + D + 1, 3 * BK - 1]
    if kind == "f64":
        vals += [2 * BK + 1, 2 * BK + 2, 2 * BK + 3]
    return sorted({v for v in vals if 1 <= v <= MAX_K})


def tail_of(kind, k):
    """t in 1 ... D - 1 where k is a chunk multiple (at least one chunk) plus t, else 0"""
    D, BK, _ = geometry()[kind]
    return k % BK if (k > BK and 0 < k % BK < D) else 0


# ---- the partition rule, restated (tests/test_tgemm_sweep_cpu.py holds it to libxsmm_amd_gemm_task) ------------------
def task_grid(m, n, nthreads):
    """(mt, nt): the cut of the tile grid of C into mt x nt parts, mt * nt <= nthreads as large as the grid allows, ties: the squarer"""
    tm, tn = -(-m // TILE), -(-n // TILE)
    mt, nt = 1, 1
    for j in range(1, min(tn, nthreads) + 1):
        i = min(nthreads // j, tm)
        if i * j > mt * nt or (i * j == mt * nt and abs(i - j) < abs(mt - nt)):
            mt, nt = i, j
    return mt, nt


def task_rect(m, n, tid, nthreads):
    """(m0, m1, n0, n1) of task tid, all zero for a task without work"""
    tm, tn = -(-m // TILE), -(-n // TILE)
    mt, nt = task_grid(m, n, nthreads)
    if tid >= mt * nt:
        return 0, 0, 0, 0
    im, jn = tid % mt, tid // mt
    return tm * im // mt * TILE, min(tm * (im + 1) // mt * TILE, m), tn * jn // nt * TILE, min(tn * (jn + 1) // nt * TILE, n)


# ---- the drawing ----------------------------------------------------------------------------------------------------------------------
def _deal_k(rng, kind, count):
    D, BK, _ = geometry()[kind]
    vals = k_values(kind)
    pick = lambda seq: int(seq[int(rng.integers(0, len(seq)))])  # noqa: E731
    below = [v for v in vals if v < D]
    deck = [pick(below), pick(below), BK, BK, 2 * BK, 2 * BK]
    for t in (range(1, D) if kind == "f64" else (None,)):
        for _ in range(2):  # a tail behind a chunk multiple: of the value list, or any such k up to the cap, by a coin
            listed = [v for v in vals if tail_of(kind, v) and (t is None or tail_of(kind, v) == t)]
            anyk = [v for v in range(1, MAX_K + 1) if tail_of(kind, v) and (t is None or tail_of(kind, v) == t)]
            deck.append(pick(listed) if 0 == rng.integers(0, 2) else pick(anyk))
    assert len(deck) <= count
    while len(deck) < count:
        deck.append(pick(vals) if 0 == rng.integers(0, 2) else int(rng.integers(1, MAX_K + 1)))
    return [deck[i] for i in rng.permutation(count)]


def _deal_mn(rng, kind, count):
    _, _, TS = geometry()[kind]
    deck = [] if TS is None else [TS - 1, TS, TS + 1] * 2
    while len(deck) < count:
        deck.append(int(EDGES[int(rng.integers(0, len(EDGES)))]) if 0 == rng.integers(0, 2) else int(rng.integers(1, MAX_MN + 1)))
    return [deck[i] for i in rng.permutation(count)]


def sweep_cases_from(seed, count=SWEEP_CASES):
    rng = np.random.default_rng(seed)
    per = count // len(KINDS)
    assert per * len(KINDS) == count and 0 == per % len(TRANS)
    dealt = {}
    for kind in KINDS:
        reps = per // len(TRANS)  # of a pair of transposes: beta 0, beta 1, and drawn from there on
        tb = [(t, r if r < 2 else int(rng.integers(0, 2))) for t in TRANS for r in range(reps)]
        mn = _deal_mn(rng, kind, 2 * per)
        dealt[kind] = ([tb[i] for i in rng.permutation(per)], _deal_k(rng, kind, per), mn[:per], mn[per:])
    out = {}
    for idx in range(count):
        kind, j = KINDS[idx % len(KINDS)], idx // len(KINDS)
        tb, ks, ms, ns = dealt[kind]
        nthreads = int(rng.integers(1, 8))
        mem = tuple(MEMS[int(v)] for v in rng.integers(0, 3, 3))
        case = dict(kind=kind, trans=tb[j][0], beta=tb[j][1], m=ms[j], n=ns[j], k=ks[j],
                    pads=tuple(int(PADS[int(v)]) for v in rng.integers(0, len(PADS), 3)), offs=tuple(int(v) for v in rng.integers(0, 8, 3)),
                    nthreads=nthreads, order=tuple(int(v) for v in rng.permutation(nthreads)),
                    mem=mem if 1 == j % 2 else ("device",) * 3)  # every other case of a kind: all operands on the device
        out["sweep_%02d_%s_%s" % (idx, kind, case["trans"].lower())] = case
    return out


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """name -> case: SWEEP_CASES cases dealt and drawn from SWEEP_SEED (see the module's docstring)"""
    return sweep_cases_from(SWEEP_SEED)


# ---- a case's geometry and buffers ----------------------------------------------------------------------------------------------------
def dims(case):
    """-> ((rows, cols) of A, B, C as stored, (lda, ldb, ldc))"""
    m, n, k = case["m"], case["n"], case["k"]
    ta, tb = case["trans"][0] == "T", case["trans"][1] == "T"
    shapes = ((k, m) if ta else (m, k), (n, k) if tb else (k, n), (m, n))
    return shapes, tuple(s[0] + p for s, p in zip(shapes, case["pads"]))


def in_dtype(kind):
    return {"f32": np.float32, "f64": np.float64}.get(kind, np.uint16)


def out_dtype(kind):
    return {"f32": np.float32, "f64": np.float64, "i16i32": np.int32}.get(kind, np.float32)


def origin(case, which):
    """index of an operand's first element in its allocation (which: 0, 1, 2 for A, B, C)"""
    return GUARD + case["offs"][which]


def embed(case, which, body):
    """the allocation of an operand: canary band, offset, the operand as it lies (ld * cols elements), canary band"""
    alloc = np.empty(GUARD + case["offs"][which] + body.size + GUARD, dtype=body.dtype)
    alloc.view(np.uint8)[:] = CANARY
    alloc[origin(case, which):origin(case, which) + body.size] = body
    return alloc


def body_of(case, which, alloc):
    (_, cols), ld = dims(case)[0][which], dims(case)[1][which]
    return alloc[origin(case, which):origin(case, which) + ld * cols]


def _seed_of(name, ints):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + (7919 if ints else 0)


@functools.lru_cache(maxsize=None)
def operands(name, ints=False):
    """(A, B, C) allocations of a case before the call (read only). The values are those of the named tests: uniform(-1, 1) for
    fp32 / fp64, lg.rand_inputs / lg.rand_c for the 16-bit kinds; ints (bf16 fast only): the integers of
    test_lowp_gemm_gpu.small_ints with an integer C in [-8, 8] and no -0.0. With beta = 0 all of C, gaps included, is NaN
    (0x7fffffff for i32)."""
    case = sweep_cases()[name]
    kind = case["kind"]
    rng = np.random.default_rng(_seed_of(name, ints))
    shapes, lds = dims(case)
    sizes = [ld * cols for (_, cols), ld in zip(shapes, lds)]
    if kind in ("f32", "f64"):
        a, b, c = (rng.uniform(-1, 1, s).astype(in_dtype(kind)) for s in sizes)
    elif ints:
        assert kind == "bf16fast"
        a, b = small_ints(rng, sizes[0]), small_ints(rng, sizes[1])
        c = rng.integers(-8, 9, sizes[2]).astype(np.float32)
    else:
        a, b = lg.rand_inputs(rng, LOWP[kind], sizes[0]), lg.rand_inputs(rng, LOWP[kind], sizes[1])
        c = lg.rand_c(rng, LOWP[kind], sizes[2])
    if 0 == case["beta"]:
        c = np.full(sizes[2], 0x7fffffff, dtype=np.int32) if kind == "i16i32" else np.full(sizes[2], np.nan, dtype=out_dtype(kind))
    res = tuple(embed(case, w, x) for w, x in enumerate((a, b, c)))
    for x in res:
        x.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def expected(name, ints=False):
    """the C allocation after the call, bit for bit (read only), from what the GPU tests of the families trust: orc.smm with orc.FMA
    for fp32 / fp64, op(A) materialised as test_tgemm_gpu.Case does, and lg.reference for the 16-bit kinds -- for bf16 fast that is
    the exact mode's chain, which is the fast mode's expectation on the integer operands only."""
    case = sweep_cases()[name]
    kind, m, n, k, beta = case["kind"], case["m"], case["n"], case["k"], case["beta"]
    ta, tb = case["trans"][0] == "T", case["trans"][1] == "T"
    _, (lda, ldb, ldc) = dims(case)
    allocs = operands(name, ints)
    a, b, c = (body_of(case, w, x) for w, x in enumerate(allocs))
    if kind in ("f32", "f64"):
        opa = a.reshape(-1, lda)[:m, :k].T.copy().ravel() if ta else a.copy()
        gold = c.copy()
        orc.smm(orc.FMA, (orc.FLAG_TRANS_B if tb else 0) | (orc.FLAG_BETA_0 if 0 == beta else 0), m, n, k, m if ta else lda, ldb, ldc, opa, b.copy(), gold)
    else:
        gold = lg.reference(LOWP[kind], ta, tb, m, n, k, a, lda, b, ldb, beta, c, ldc)
    want = embed(case, 2, gold)
    want.setflags(write=False)
    return want


# ---- the product restated by index formulas, with room for one mistake ----------------------------------------------------------------
WRONG = ("k tail dropped", "term at k = BK twice", "ldb read as lda", "ldc read as lda", "offset of A ignored", "operand read untransposed",
         "beta = 0 reads C", "i16 read unsigned", "task rectangle short", "last task skipped")


def gather(alloc, at, ld, rows, cols, trans):
    """op(X) as a rows x cols array: element (i, j) lies at at + j * ld + i, or at + i * ld + j where X is stored transposed. (An
    index that a mistake pushes past the allocation wraps around: the outcome is wrong values, not an exception.)"""
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return alloc[(at + (i * ld + j if trans else j * ld + i)) % alloc.size]


def chain(kind, A, B, C0, unsigned=False):
    """C0 + A B element by element in the kind's arithmetic, by the trusted routines on tight operands: A (m x k), B (k x n) and
    C0 (m x n, None: the chain starts from zero) as 2-D arrays -> m x n. The routines compute every element as its own chain over
    k, so the bits do not depend on the leading dimensions they are handed."""
    m, k = A.shape
    n = B.shape[1]
    dt = out_dtype(kind)
    c = np.zeros(m * n, dtype=dt) if C0 is None else np.ascontiguousarray(C0.T, dtype=dt).ravel()
    if 0 == k:
        return c.reshape(n, m).T.copy()
    a, b = np.ascontiguousarray(A.T).ravel(), np.ascontiguousarray(B.T).ravel()
    if unsigned:  # the mistake "i16 read unsigned": no trusted routine reads that way, so the chains of lg.reference are spelt out on 0 ... 65535
        Au, Bu = A.astype(np.int64), B.astype(np.int64)
        acc = (np.zeros((m, n), dt) if C0 is None else C0.astype(dt)).astype(np.int64 if kind == "i16i32" else np.float32)
        for kk in range(k):
            term = Au[:, kk, None] * Bu[None, kk, :]
            acc = (acc + term) & 0xFFFFFFFF if kind == "i16i32" else acc + term.astype(np.float32)
        return acc.astype(np.uint32).view(np.int32) if kind == "i16i32" else acc
    if kind in ("f32", "f64"):
        orc.smm(orc.FMA, orc.FLAG_BETA_0 if C0 is None else 0, m, n, k, m, k, m, a, b, c)
    else:
        c = lg.reference(LOWP[kind], False, False, m, n, k, a, m, b, k, 0 if C0 is None else 1, c, m)
    return c.reshape(n, m).T.copy()


def restated(name, ints=False, wrong=None):
    """the C allocation after the call, built without lg.op and the reshapes of Case: the operands are taken apart by the
    column-major index formula with the case's own leading dimensions and offsets, multiplied tight, and every task's rectangle is
    written back by the same formula. wrong: one of WRONG, the one mistake made on the way."""
    assert wrong is None or wrong in WRONG
    case = sweep_cases()[name]
    kind, m, n, k, beta = case["kind"], case["m"], case["n"], case["k"], case["beta"]
    D, BK, _ = geometry()[kind]
    ta, tb = case["trans"][0] == "T", case["trans"][1] == "T"
    _, (lda, ldb, ldc) = dims(case)
    xa, xb, xc = operands(name, ints)
    if wrong == "ldb read as lda":
        ldb = lda
    if wrong == "ldc read as lda":
        ldc = lda
    if wrong == "operand read untransposed":
        ta, tb = (False, tb) if ta else (ta, False)
    A = gather(xa, GUARD if wrong == "offset of A ignored" else origin(case, 0), lda, m, k, ta)
    B = gather(xb, origin(case, 1), ldb, k, n, tb)
    C0 = gather(xc, origin(case, 2), ldc, m, n, False)
    if wrong == "k tail dropped":
        A, B = A[:, :k - k % D], B[:k - k % D, :]
    if wrong == "term at k = BK twice" and k > BK:
        A, B = np.concatenate([A[:, :BK + 1], A[:, BK:]], axis=1), np.concatenate([B[:BK + 1, :], B[BK:, :]], axis=0)
    full = chain(kind, A, B, C0 if (0 != beta or wrong == "beta = 0 reads C") else None,
                 unsigned=(wrong == "i16 read unsigned" and kind in ("i16i32", "i16f32")))
    out = xc.copy()
    rects = [task_rect(m, n, tid, case["nthreads"]) for tid in case["order"]]
    busy = [r for r in rects if r[0] < r[1]]
    if wrong == "last task skipped":
        busy = busy[:-1]
    for m0, m1, n0, n1 in busy:
        if wrong == "task rectangle short":
            m1, n1 = (m1 - 1, n1) if m1 - m0 > 1 else (m1, n1 - 1)
        i, j = np.arange(m0, m1)[:, None], np.arange(n0, n1)[None, :]
        out[(origin(case, 2) + j * ldc + i) % out.size] = full[m0:m1, n0:n1]
    return out


# ---- the float64 contract ---------------------------------------------------------------------------------------------------------------
U24, U53 = 2.0 ** -24, 2.0 ** -53


def gamma(j, u):
    return j * u / (1 - j * u)


def contract64(name, ints=False):
    """(value, bound, exact) of op(A) op(B) + beta C as m x n float64 arrays (exact: the value as int64 where the contract is
    equality, else None), from the operands taken apart by the index formula. With S = |c| + sum |a_i b_i| over the k terms of an
    element and gamma_j = j u / (1 - j u) (the standard bound of j compounded roundings of relative size u):

      fp32, fp64      u = 2^-24, 2^-53. The element is a chain of k fused multiply-adds from c (or +0.0): k roundings.  gamma_k S
      bf16 exact      u = 2^-24. A bf16 x bf16 product has 16 significant bits and is exact in fp32 while it stays above 2^-126
                      (asserted here), so only the k adds round.                                           gamma_k S
      i16 -> f32      u = 2^-24. Each 31-bit product is rounded once by its conversion, then k adds round.            gamma_(k+1) S
      i16 -> i32      nothing rounds: the Python-integer sum reduced mod 2^32, as a signed 32-bit value.                  equality
      bf16 fast       drawn bf16 operands: DESIGN.md 8d's model of the instruction, exact products and internal adds that err by
                      at most 2^-23 relative each, at most k + 1 of them on the way of a term, c included.        (k + 1) 2^-23 S
                      integer operands: every partial sum is an integer of magnitude <= 16 * 200 + 8 < 2^24 and therefore exact
                      in any order.                                                                                       equality
    """
    case = sweep_cases()[name]
    kind, m, n, k, beta = case["kind"], case["m"], case["n"], case["k"], case["beta"]
    ta, tb = case["trans"][0] == "T", case["trans"][1] == "T"
    _, (lda, ldb, ldc) = dims(case)
    xa, xb, xc = operands(name, ints)
    i, j, kk = np.arange(m)[:, None], np.arange(n)[None, :], np.arange(k)
    A = xa[origin(case, 0) + (i * lda + kk[None, :] if ta else kk[None, :] * lda + i)]
    B = xb[origin(case, 1) + (kk[:, None] + j * ldb if not tb else kk[:, None] * ldb + j)]
    C0 = xc[origin(case, 2) + j * ldc + i] if 0 != beta else np.zeros((m, n), dtype=out_dtype(kind))
    if kind in ("i16i32", "i16f32"):
        A, B = A.view(np.int16).astype(np.int64), B.view(np.int16).astype(np.int64)
    elif kind in ("bf16", "bf16fast"):
        A, B = ((x.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for x in (A, B))
        least = [float(np.min(np.abs(x)[x != 0], initial=1.0)) for x in (A, B)]  # (the smallest product there can be)
        assert least[0] * least[1] >= 2.0 ** -126, "a product underflows: it would not be exact in fp32"
    else:
        A, B = A.astype(np.float64), B.astype(np.float64)
    if kind == "i16i32":
        total = C0.astype(np.int64) + A @ B  # |.| < 2^31 + 200 * 2^30: exact in int64
        exact = ((total + 2 ** 31) % 2 ** 32) - 2 ** 31
        return exact.astype(np.float64), np.zeros((m, n)), exact
    value = A.astype(np.float64) @ B.astype(np.float64) + C0.astype(np.float64)
    S = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64) + np.abs(C0.astype(np.float64))
    if kind == "bf16fast" and ints:
        assert float(S.max()) <= 16 * 200 + 8
        return value, np.zeros((m, n)), value.astype(np.int64)
    bound = {"f32": gamma(k, U24), "f64": gamma(k, U53), "bf16": gamma(k, U24), "i16f32": gamma(k + 1, U24), "bf16fast": (k + 1) * 2.0 ** -23}[kind] * S
    return value, bound, None


def compare(name, c_alloc, ints=False, label=None, fast=False):
    """None, or what is wrong with a C allocation after the call: the m x n elements against contract64 (fast: a bf16 fast case on
    drawn operands is held to the fast mode's bound, otherwise to the exact mode's, which its expected bits are); every other
    byte of the allocation -- canary bands, the elements in front of the offset, what lies between m and ldc -- against the
    allocation before the call. label: print the worst error / bound."""
    case = sweep_cases()[name]
    kind, m, n, k = case["kind"], case["m"], case["n"], case["k"]
    _, (_, _, ldc) = dims(case)
    before = operands(name, ints)[2]
    if c_alloc.dtype != before.dtype or c_alloc.shape != before.shape:
        return "C has the wrong type or size"
    i, j = np.arange(m)[:, None], np.arange(n)[None, :]
    at = origin(case, 2) + j * ldc + i
    rest = np.ones(before.size, dtype=bool)
    rest[at.ravel()] = False
    if c_alloc[rest].tobytes() != before[rest].tobytes():
        return "a byte outside the m x n elements of C changed"
    value, bound, exact = contract64(name, ints)
    if kind == "bf16fast" and not ints and not fast:
        bound = bound * (gamma(k, U24) / ((k + 1) * 2.0 ** -23))
    got = c_alloc[at]
    if exact is not None:
        if not np.all(np.isfinite(got.astype(np.float64))) or not np.array_equal(got.astype(np.int64), exact) or not np.array_equal(got.astype(np.float64), value):
            return "%d elements differ from the exact value" % int(np.sum(got.astype(np.float64) != value))
        return None
    got = got.astype(np.float64)
    if not np.all(np.isfinite(got)):
        return "%d elements are not finite" % int(np.sum(~np.isfinite(got)))
    err = np.abs(got - value)
    if label:
        print("%s: worst error / bound %.3g" % (label, worst_ratio(err, bound)))
    if not np.all(err <= bound):
        return "%d elements beyond their bound (worst error / bound %.3g)" % (int(np.sum(err > bound)), worst_ratio(err, bound))
    return None


def worst_ratio(err, bound):
    return float(np.max((err / np.where(bound > 0, bound, 1))[bound > 0], initial=0))


def ratio_of(name, c_alloc, ints=False, fast=False):
    """the worst error / bound of a C allocation (0 where the contract is equality)"""
    case = sweep_cases()[name]
    value, bound, exact = contract64(name, ints)
    if exact is not None:
        return 0.0
    if case["kind"] == "bf16fast" and not fast:
        bound = bound * (gamma(case["k"], U24) / ((case["k"] + 1) * 2.0 ** -23))
    i, j = np.arange(case["m"])[:, None], np.arange(case["n"])[None, :]
    got = c_alloc[origin(case, 2) + j * dims(case)[1][2] + i].astype(np.float64)
    return worst_ratio(np.abs(got - value), bound)
