"""What tests/test_hostile_operands_{cpu,gpu}.py share: operands whose surroundings are poisoned, operand values at the
edges of the number line, and the comparison that goes with them. The packed kernels' hostile matrices (packed_hostile(), at the
end of the file) serve tests/test_packed_hostile_gpu.py and tests/test_packed_chain_cpu.py.

Layout. An operand is a batch of column-major matrices inside one flat array: a guard band of GUARD elements in front and
behind, leading dimensions of extent + 3, and (where a call takes strides) items that lie size + 4 or size + 1 elements
apart. Everything that is not an element of a matrix holds the fill (fills(): quiet NaN then +Inf, for i16 the two ends of
the range). All of it is allocated: a kernel that reads a neighbour of an element still reads the test's own memory.

Values. Three generators per floating type, as (batch, rows, cols) arrays of the logical matrices:
  underflow  A, B = +-uniform(0.5, 1) * 2^e whose products have exponents spread evenly over emin - 26 ... emin + 10 (fp32:
             2^-152 ... 2^-116), one row or column in eight down to emin - p - 3; C at the scale of the smallest normal number;
  overflow   the same with the products at 2^(emax - 7) ... 2^(emax + 1): some chains run to +-Inf, others stay finite. The
             signs are mixed, but most terms of a chain pull the same way (else Inf - Inf = NaN would take over);
  specials   uniform(-1, 1) with +-Inf, NaN, an all-zero row of A that meets an Inf in B, and -0.0 planted (plant()).
The exponent is a property of the row of A or of the column of B (plus a jitter of +-1), so that the rows and columns of C
differ in magnitude and the conditions of conditions() hold on the reference alone. bf16 operands are float32 arrays whose
lower 16 bits are zero (bf16_bits() packs them). Seeds are fixed per case (seed_of); tests/test_hostile_operands_cpu.py
holds every case of the GPU file against conditions().

Comparison. same_values(): equal NaN positions, equal bits everywhere else (signed zeros, subnormals, Inf); the sign and
payload of a NaN are not compared -- x86 and the GPU produce different default NaNs and the reference fixes none."""
import numpy as np

GUARD = 64
KINDS = ("underflow", "overflow", "specials")

# (smallest normal exponent, largest exponent, explicit significand bits) of the type the chain is accumulated in
RANGE = {"f32": (-126, 127, 23), "f64": (-1022, 1023, 52), "bf16": (-126, 127, 23)}


def fmt_of(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def np_dtype(fmt):
    return np.float64 if fmt == "f64" else np.float32


def fills(fmt):
    """the two fills of a format, as values of the array's dtype (bf16 and i16: 16-bit patterns as uint16)"""
    if fmt == "bf16":
        return (np.uint16(0x7fc0), np.uint16(0x7f80))
    if fmt == "i16":
        return (np.int16(-32768).view(np.uint16), np.uint16(32767))
    if fmt == "i32":  # a C of 32-bit sums: the ends of its range
        return (np.int32(-2 ** 31), np.int32(2 ** 31 - 1))
    t = np_dtype(fmt)
    return (t(np.nan), t(np.inf))


class Layout(object):
    """a batch of column-major rows x cols matrices in one flat array (see the module's docstring). ld: the leading dimension
    (None: rows + 3); extra: what the item stride adds to ld * cols"""

    def __init__(self, rows, cols, batch=1, ld=None, extra=4, guard=GUARD):
        self.rows, self.cols, self.batch, self.guard = rows, cols, batch, guard
        self.ld = rows + 3 if ld is None else ld
        assert self.ld >= rows and extra >= 0
        self.size = self.ld * cols
        self.stride = self.size + extra
        self.total = 2 * guard + batch * self.stride

    def offsets(self):
        """where the items start, in elements from the start of the array"""
        return self.guard + np.arange(self.batch, dtype=np.int64) * self.stride

    def index(self):
        """flat positions of the elements, as (batch, rows, cols)"""
        item = np.arange(self.cols)[None, :] * self.ld + np.arange(self.rows)[:, None]
        return self.offsets()[:, None, None] + item[None, :, :]

    def mask(self):
        m = np.zeros(self.total, dtype=bool)
        m[self.index().ravel()] = True
        return m


def surround(logical, layout, fill):
    """the flat array of `layout` that holds the matrices `logical` ((batch, rows, cols) or (rows, cols)) and `fill` everywhere else"""
    logical = logical.reshape((-1,) + logical.shape[-2:])
    assert logical.shape == (layout.batch, layout.rows, layout.cols), (logical.shape, layout.batch, layout.rows, layout.cols)
    flat = np.full(layout.total, fill, dtype=logical.dtype)
    flat[layout.index()] = logical
    return flat


def peel(flat, layout):
    """the matrices of a flat array, as (batch, rows, cols)"""
    assert flat.shape == (layout.total,)
    return flat[layout.index()]


def gaps(flat, layout):
    """everything that is not an element of a matrix, as raw bytes"""
    return np.ascontiguousarray(flat[~layout.mask()]).view(np.uint8)


def raw(x):
    return np.ascontiguousarray(x).view(np.uint8)


def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16) by truncation (exact for what the generators make)"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_widen(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def is_nan(x):
    if x.dtype == np.uint16:  # bf16 bit patterns
        return (x & 0x7fff) > 0x7f80
    if x.dtype.kind == "f":
        return np.isnan(x)
    return np.zeros(x.shape, dtype=bool)


def same_values(got, want):
    """NaN exactly where the reference has NaN, the reference's bits everywhere else"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = is_nan(got), is_nan(want)
    if not np.array_equal(gn, wn):
        return False
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    return bool(np.array_equal(g[~gn], w[~wn]))


def differences(got, want):
    """for assertion messages: how many NaN positions differ, how many other elements differ in their bits"""
    gn, wn = is_nan(got), is_nan(want)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    both = ~gn & ~wn
    return int(np.sum(gn != wn)), int(np.sum((np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)) & both))


def assert_environment(orc):
    """a host that flushes subnormals must fail here, loudly, not make every kernel look wrong"""
    tiny = np.float32(2.0 ** -126) * np.float32(0.5)
    assert tiny != 0 and tiny.view(np.uint32) == 0x00400000, "numpy float32 flushes subnormals on this host"
    a, b, c = np.array([2.0 ** -126], np.float32), np.array([0.5], np.float32), np.zeros(1, np.float32)
    orc.smm(orc.FMA, 0, 1, 1, 1, 1, 1, 1, a, b, c)
    assert c.view(np.uint32)[0] == 0x00400000, "the oracle flushes subnormals on this host: %#x" % c.view(np.uint32)[0]


# ---- generators -------------------------------------------------------------------------------------------------------------
def _scaled(rng, shape, exps, signs=None):
    signs = rng.choice([-1.0, 1.0], shape) if signs is None else signs
    return rng.uniform(0.5, 1.0, shape) * np.exp2(exps.astype(np.float64)) * signs


def _products(rng, fmt, batch, m, n, k, lo, hi, deep, c_exps, coherent=False, owner=None):
    """A (batch, m, k), B (batch, k, n) whose products a * b have exponents spread evenly over lo ... hi: the exponent is a
    property of the row of A (even items) or of the column of B (odd items), so that the elements of C differ in magnitude
    by rows or by columns; one row or column in eight lies in deep ... lo instead. Every element jitters by +-1.
    coherent: a row of A and a column of B have a sign of their own and one element in eight has the other one, so that most
    terms of a chain pull the same way (a chain that overflows then mostly stays +-Inf and does not end as Inf - Inf = NaN).
    C (batch, m, n) = +-uniform(0.5, 1) * 2^(one of c_exps)"""
    half = lo // 2
    ea, eb = np.full((batch, m, 1), half), np.full((batch, 1, n), lo - half)
    drawn = {}
    for t in range(batch):
        blk = t if owner is None else int(owner[t])  # (items that add to one block of C share its exponents)
        lines = m if blk % 2 == 0 else n
        if blk not in drawn:
            e = rng.integers(0, hi - lo + 1, lines)
            if deep < lo:
                e = np.where(rng.integers(0, 8, lines) == 0, rng.integers(deep - lo, 1, lines), e)
            drawn[blk] = e
        e = drawn[blk]
        if blk % 2 == 0:
            ea[t, :, 0] += e
        else:
            eb[t, 0, :] += e
    sa = sb = None
    if coherent:
        sa = rng.choice([-1.0, 1.0], (batch, m, 1)) * np.where(rng.integers(0, 8, (batch, m, k)) == 0, -1.0, 1.0)
        sb = rng.choice([-1.0, 1.0], (batch, 1, n)) * np.where(rng.integers(0, 8, (batch, k, n)) == 0, -1.0, 1.0)
    a = _scaled(rng, (batch, m, k), ea + rng.integers(-1, 2, (batch, m, k)), sa)
    b = _scaled(rng, (batch, k, n), eb + rng.integers(-1, 2, (batch, k, n)), sb)
    c = _scaled(rng, (batch, m, n), rng.choice(np.asarray(c_exps), (batch, m, n)))
    return a, b, c


def plant(a, b, c, rng, owner=None):
    """the special entries (see the module's docstring). A batch spreads them over its items: item t takes the groups g with
    g % min(batch, 5) == t % 5; a single matrix (needs m >= 5) takes them all. Rows 0 and 1 of A are the +0 and the -0 row,
    the last row and column carry what has to sit on an edge. owner: item -> its block of C (None: every item its own).
    A NaN of B costs a column of C and a NaN of A a row, whatever a kernel does. A single matrix with fewer than 8 rows or
    columns (the passes of the fully-connected cases, N = 5 or 6) could not stay below a quarter of NaN with the layout above,
    so it takes the compact one of _plant_compact()."""
    batch, m, k = a.shape
    n = b.shape[2]
    assert m >= 3 and n >= 3 and (batch > 1 or m >= 5)
    if batch == 1 and min(m, n) < 8:
        return _plant_compact(a, b, c, rng)
    owner = np.arange(batch) if owner is None else owner
    inf, nan = np.inf, np.nan
    for t in range(batch):
        for g in range(5):
            if g % min(batch, 5) != t % 5:
                continue
            if g == 0:    # an all-zero row of A meets an Inf of B: 0 * Inf = NaN, which a kernel that skips zeros loses
                a[t, 0, :] = 0.0
                b[t, k // 2, 0] = inf
            elif g == 1:  # Inf in A at the first k, in the last row; -Inf in B at the last k, in the last column
                a[t, m - 1, 0] = inf
                b[t, k - 1, n - 1] = -inf
            elif g == 2:  # NaN in A at the last k (the last row of a batch item; row 2 where row m - 1 carries the Inf), NaN in B at the first k
                a[t, (m - 1 if batch > 1 else 2), k - 1] = nan
                b[t, 0, n - 2] = nan
            elif g == 3:  # a row of -0.0 against a column of positive numbers and a C of -0.0: the chain stays -0.0 (in every
                for u in np.nonzero(owner == owner[t])[0]:  # item that adds to this block of C)
                    a[u, 1, :] = -0.0
                    b[u, :, 1] = np.abs(b[u, :, 1])
                c[owner[t], 1, 1] = -0.0
                b[t, rng.integers(0, k), 2] = -0.0
            else:         # -Inf in A at the last k and +Inf at the first k of B, away from the edges
                a[t, m // 2, k - 1] = -inf
                b[t, 0, n // 2] = inf
    return a, b, c


def _plant_compact(a, b, c, rng):
    """one matrix with few rows or columns (5 <= min(m, n) < 8, the other extent >= 8): the same kinds of entries, placed so that
    they share rows and columns of C. Column n - 2 of C is NaN (NaN of B at the first k; it hides a +Inf of B at the second k),
    row m - 1 is NaN (NaN of A at the last k; it hides the +Inf of A at the first k), the all-zero row 0 of A meets the Inf of
    B in columns 0 and n - 1 (two more NaN), and the -Inf of A in row m // 2 meets them with the signs that keep an Inf: m + n + 1
    NaN in all. -0.0 entries of A and B are single elements (no chain that starts from +0 can end in -0.0 anyway)."""
    _, m, k = a.shape
    n = b.shape[2]
    assert m >= 5 and n >= 5 and k >= 4
    inf, nan = np.inf, np.nan
    a[0, 0, :] = 0.0
    b[0, k // 2, 0] = inf                    # 0 x Inf in the middle of the chain; rows 1 ... m - 2 of column 0 are +-Inf
    b[0, k - 1, n - 1] = -inf                # last k, last column
    b[0, 0, n - 2], b[0, 1, n - 2] = nan, inf  # first k
    a[0, m - 1, 0], a[0, m - 1, k - 1] = inf, nan  # last row: first k and last k
    a[0, m // 2, k - 1] = -inf               # last k, away from the edges: (-Inf)(-Inf) = +Inf in column n - 1 ...
    b[0, k - 1, 0] = -np.abs(b[0, k - 1, 0]) * np.sign(a[0, m // 2, k // 2])  # ... and in column 0 the sign of a * (+Inf) at k // 2
    a[0, 1, 1], a[0, 2, k - 2] = -0.0, -0.0
    b[0, rng.integers(1, k - 1), 2] = -0.0
    return a, b, c


def operands(kind, fmt, seed, batch, m, n, k, owner=None):
    """-> A (batch, m, k), B (batch, k, n), C (batch, m, n) in the numpy type of `fmt` (bf16: float32 with 8-bit significands)"""
    rng = np.random.default_rng(seed)
    emin, emax, p = RANGE[fmt]
    if kind == "underflow":
        a, b, c = _products(rng, fmt, batch, m, n, k, emin - 26, emin + 10, emin - p - 3, (emin - 1, emin, emin + 1, emin + 2), owner=owner)
    elif kind == "overflow":
        a, b, c = _products(rng, fmt, batch, m, n, k, emax - 7, emax + 1, emax - 7, (emax - 3, emax - 2, emax - 1, emax), coherent=True, owner=owner)
    else:
        assert kind == "specials"
        a, b, c = (rng.uniform(-1, 1, s) for s in ((batch, m, k), (batch, k, n), (batch, m, n)))
        a, b, c = plant(a, b, c, rng, owner)
    t = np_dtype(fmt)
    a, b, c = a.astype(t), b.astype(t), c.astype(t)
    if fmt == "bf16":
        a, b = bf16_widen(bf16_bits(a)), bf16_widen(bf16_bits(b))
    return a, b, c


def conditions(kind, ref, beta=1):
    """what the reference result of a generator has to show, so that a comparison with it compares something. ref: the logical C
    (any shape). A chain that starts from +0 (beta = 0) cannot end in -0.0 -- (+0) + (-0) = +0 --, so that one condition is asked
    for under beta = 1 only."""
    ref = np.asarray(ref)
    count = float(ref.size)
    finite = np.isfinite(ref)
    tiny = np.finfo(ref.dtype).tiny
    if kind == "underflow":
        sub = np.sum(finite & (ref != 0) & (np.abs(ref) < tiny))
        normal = np.sum(finite & (np.abs(ref) >= tiny))
        assert sub >= count / 4, ("subnormal", int(sub), ref.size)
        assert normal >= count / 4, ("normal", int(normal), ref.size)
    elif kind == "overflow":
        ninf = np.sum(np.isinf(ref))
        assert count / 8 <= ninf <= 7 * count / 8, ("Inf", int(ninf), ref.size)
    else:
        nnan = np.sum(np.isnan(ref))
        assert 1 <= nnan <= count / 4, ("NaN", int(nnan), ref.size)
        assert np.isinf(ref).any(), "no Inf"
        if beta:
            assert np.any((ref == 0) & np.signbit(ref)), "no -0.0"


# ---- references on the logical matrices --------------------------------------------------------------------------------------
def chain(orc, a, b, c, beta=1, arith=None, transb=False):
    """the oracle's chain per item on tight copies of the logical matrices: (batch, m, n). arith: orc.FMA (default) or orc.MULADD"""
    batch, m, k = a.shape
    n = b.shape[2]
    out = np.empty_like(c)
    flags = (orc.FLAG_BETA_0 if 0 == beta else 0) | (orc.FLAG_TRANS_B if transb else 0)
    for t in range(batch):
        at = np.ascontiguousarray(a[t].T).ravel()                            # column major, lda = m
        bt = np.ascontiguousarray(b[t] if transb else b[t].T).ravel()        # ldb = k, or B^T with ldb = n
        ct = np.array(c[t].T, order="C").ravel()                           # (a copy: the oracle works in place)
        orc.smm(orc.FMA if arith is None else arith, flags, m, n, k, m, n if transb else k, m, at, bt, ct)
        out[t] = ct.reshape(n, m).T
    return out


def reduce_chain(orc, a, b, c, beta=1):
    """one C (m, n) that takes the products of all items in batch order: the chain of a run and of batch-reduce"""
    acc = c.reshape((1,) + c.shape[-2:]).copy()
    for t in range(a.shape[0]):
        acc = chain(orc, a[t:t + 1], b[t:t + 1], acc, beta if t == 0 else 1)
    return acc[0]


def gold_bf16(a, b, c, beta=1):
    """the gold loop of the bf16 kinds on the logical matrices: acc = acc + a * b, product and sum each rounded to float32"""
    acc = c.astype(np.float32).copy() if beta else np.zeros(c.shape, np.float32)
    with np.errstate(all="ignore"):
        for kk in range(a.shape[2]):
            acc = acc + a[:, :, kk, None] * b[:, kk, None, :]
    return acc


def inexact_product(a, b):
    """(batch, m, n): True where the chain of an element meets a product of two bf16 numbers that float32 cannot hold exactly:
    one that is nonzero and below the smallest normal number, or one beyond the largest finite number. There, and only there,
    one rounding (fma) and two (multiply, then add) can differ."""
    hit = np.zeros((a.shape[0], a.shape[1], b.shape[2]), dtype=bool)
    tiny, big = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        for kk in range(a.shape[2]):
            p = np.abs(a[:, :, kk, None].astype(np.float64) * b[:, kk, None, :].astype(np.float64))
            hit |= ((p != 0) & (p < tiny)) | (np.isfinite(p) & (p > big))
    return hit


# ---- the cases of the dense SMM families (both test files walk this table) ---------------------------------------------------
def seed_of(*parts):
    """a fixed seed per case: tests/test_hostile_operands_cpu.py checks conditions() on every one of them"""
    import zlib
    return zlib.crc32(repr(parts).encode())


class SmmCase(object):
    """one batch of dense products. ld: None tight, "pad" extent + 3, or (lda, ldb, ldc); mode: "strided", "index" (every item
    its own C), "runs" (index arrays, consecutive items share a C as `runs` lists), "reduce" (the dispatched batch-reduce
    kernel); distinct: the caller's promise of a negative batch size; env: environment of the call; kernel: format ->
    name(s) that libxsmm_amd_last_kernel has to report (a name that ends in "_" is a prefix); shift: (format, kind, beta) -> added
    to the case's seed where the plain one misses a condition of conditions() by a few elements"""

    def __init__(self, id, shape, batch, kernel, ld=None, mode="strided", runs=None, mfma=0, env=None, transb=False, fmts=("f32", "f64"),
                 betas=(1, 0), extras=(4, 1), distinct=False, shift=None):
        self.id, self.shape, self.batch, self.kernel, self.ld, self.mode, self.runs = id, shape, batch, kernel, ld, mode, runs
        self.mfma, self.env, self.transb, self.fmts, self.betas, self.extras, self.distinct = mfma, dict(env or {}), transb, fmts, betas, extras, distinct
        self.shift = dict(shift or {})
        assert all(f in fmts and g in KINDS and be in betas for f, g, be in self.shift)
        assert runs is None or sum(runs) == batch

    def lds(self):
        m, n, k = self.shape
        tight = (m, n if self.transb else k, m)
        if self.ld is None:
            return tight
        return tuple(x + 3 for x in tight) if self.ld == "pad" else self.ld

    def owners(self):
        """item -> its C block"""
        if self.mode == "reduce":
            return np.zeros(self.batch, dtype=np.int64)
        if self.runs is None:
            return np.arange(self.batch, dtype=np.int64)
        return np.repeat(np.arange(len(self.runs), dtype=np.int64), self.runs)

    def operands(self, kind, fmt, beta):
        """-> A (batch, m, k), B (batch, k, n), C (blocks, m, n); kind None: uniform(-1, 1), the data of the gap tests"""
        m, n, k = self.shape
        nc = int(self.owners().max()) + 1
        seed = seed_of(self.id, fmt, kind, beta) + self.shift.get((fmt, kind, beta), 0)
        if kind is None:
            rng = np.random.default_rng(seed)
            t = np_dtype(fmt)
            return tuple(rng.uniform(-1, 1, s).astype(t) for s in ((self.batch, m, k), (self.batch, k, n), (nc, m, n)))
        a, b, c = operands(kind, fmt, seed, self.batch, m, n, k, self.owners())
        return a, b, np.ascontiguousarray(c[:nc])

    def reference(self, orc, a, b, c, beta):
        """the oracle's chain on the logical matrices alone: (blocks, m, n)"""
        own = self.owners()
        if self.runs is None and self.mode != "reduce":
            return chain(orc, a, b, c, beta)
        out = np.empty_like(c)
        for blk in range(c.shape[0]):
            items = np.nonzero(own == blk)[0]
            out[blk] = reduce_chain(orc, a[items], b[items], c[blk], beta)
        return out


_JIT = {"LIBXSMM_AMD_JIT": "1", "LIBXSMM_AMD_JIT_MINBATCH": "1"}
_NOJIT = {"LIBXSMM_AMD_JIT": "0"}
_F = lambda pattern: {"f32": pattern % 32, "f64": pattern % 64}

SMM_CASES = [
    # generic SMM, matrix cores off: the pre-compiled kernels of smm_generic.hip
    SmmCase("generic-3x5x7", (3, 5, 7), 5, _F("smm_f%d_generic_"), ld="pad", shift={("f32", "underflow", 0): 2}),
    SmmCase("generic-23x29x31", (23, 29, 31), 5, _F("smm_f%d_generic_"), ld=(32, 32, 32)),
    # tuned 32^3 and 64^3 (tight operands: the gaps are the guard bands and what lies between the items)
    SmmCase("tuned-32-fma-67", (32, 32, 32), 67, {"f32": "smm_f32_32x32x32_fma"}, fmts=("f32",)),
    SmmCase("tuned-32-mfma-67", (32, 32, 32), 67, {"f32": "smm_f32_32x32x32_mfma"}, mfma=1, fmts=("f32",)),
    SmmCase("tuned-32-mfma-5-index", (32, 32, 32), 5, {"f32": "smm_f32_32x32x32_mfma"}, mode="index", distinct=True, mfma=1, fmts=("f32",)),
    SmmCase("tuned-64-mfma-5", (64, 64, 64), 5, {"f32": "smm_f32_64x64x64_mfma", "f64": "smm_f64_mfma_wg"}, mfma=1, env=_NOJIT),
    SmmCase("tuned-64-mfma-67-index", (64, 64, 64), 67, {"f32": "smm_f32_64x64x64_mfma", "f64": "smm_f64_mfma_wg"}, mode="index", distinct=True,
            mfma=1, env=_NOJIT, extras=(1,)),
    # the work-group matrix-core form, pre-compiled: TIGHT + TIGHTC, plain with gaps, odd K
    SmmCase("wg-40", (40, 40, 40), 5, _F("smm_f%d_mfma_wg"), mfma=1, env=_NOJIT),
    SmmCase("wg-43x9x27", (43, 9, 27), 5, _F("smm_f%d_mfma_wg"), ld=(48, 32, 48), mfma=1, env=_NOJIT),
    SmmCase("wg-33x64x7", (33, 64, 7), 5, _F("smm_f%d_mfma_wg"), mfma=1, env=_NOJIT, shift={("f64", "underflow", 0): 2}),
    # ... and built by hiprtc with the descriptor baked in: the one-wave-per-item form serves both shapes
    SmmCase("wgjit-40", (40, 40, 40), 5, _F("smm_f%d_mfma_wave_jit"), mfma=1, env=_JIT),
    SmmCase("wgjit-33x64x7", (33, 64, 7), 5, _F("smm_f%d_mfma_wave_jit"), mfma=1, env=_JIT, shift={("f64", "underflow", 0): 1}),
    SmmCase("wgjit-40x36x20-nt", (40, 36, 20), 5, _F("smm_f%d_mfma_wave_jit"), mfma=1, env=_JIT, transb=True),
    # the wave kernels on the matrix cores for M, N <= 32: independent items (streaming form, several small items per pass), TRANS_B,
    # runs that share a C
    SmmCase("wave-13", (13, 13, 13), 9, _F("smm_f%d_mfma_stream_jit"), mfma=1, env=dict(_JIT, XSMM_SMMJIT_GAPS_MFMA="2")),
    SmmCase("wave-16x8x5", (16, 8, 5), 9, _F("smm_f%d_mfma_stream_jit"), ld="pad", mfma=1, env=dict(_JIT, XSMM_SMMJIT_GAPS_MFMA="2")),
    # (TRANS_B at M, N <= 32 with every item its own C has no matrix-core form: the vector-ALU kernel serves it)
    SmmCase("wave-23-nt", (23, 23, 23), 9, _F("smm_f%d_jit_shape"), mfma=1, env=_JIT, transb=True),
    SmmCase("wave-23-runs", (23, 23, 23), 9, _F("smm_f%d_mfma_runs_"), mode="runs", runs=(3, 1, 2, 1, 1, 1), mfma=1, env=_JIT, betas=(1,)),
    SmmCase("wave-16x8x5-runs", (16, 8, 5), 9, _F("smm_f%d_mfma_runs_"), ld="pad", mode="runs", runs=(1, 3, 1, 1, 1, 2), mfma=1, env=_JIT, betas=(1,)),
    # hiprtc-built kernels on the vector ALU: dense, with gaps, the run form
    SmmCase("jit-13", (13, 13, 13), 9, {"f64": "smm_f64_jit_shape"}, env=_JIT, fmts=("f64",)),
    SmmCase("jit-23-gaps", (23, 23, 23), 9, {"f32": "smm_f32_jit_shape"}, ld="pad", env=dict(_JIT, XSMM_SMMJIT_GAPS_MFMA="0"), fmts=("f32",)),
    SmmCase("jit-23-runs", (23, 23, 23), 9, _F("smm_f%d_jit_shape_runs"), ld="pad", mode="runs", runs=(3, 1, 2, 1, 1, 1), env=_JIT, betas=(1,)),
    # batch-reduce through the dispatched kernel
    SmmCase("reduce-23", (23, 23, 23), 3, _F("smm_f%d_jit_shape_runs"), mode="reduce", shift={("f64", "underflow", 0): 1}),
]

# grouped launch (libxsmm_amd_gemm_batch_groups): three shapes in one call, batch 9 each, the last one TRANS_B
GROUPED = [SmmCase("grouped-13", (13, 13, 13), 9, None, mode="runs", runs=(3, 1, 2, 1, 1, 1), betas=(1,)),
           SmmCase("grouped-32", (32, 32, 32), 9, None, mode="runs", runs=(1, 1, 1, 1, 1, 1, 1, 1, 1), betas=(1,)),
           SmmCase("grouped-23-nt", (23, 23, 23), 9, None, mode="runs", runs=(2, 2, 2, 3), transb=True, betas=(1,))]


def smm_variants(cases=None):
    """(case, format, beta) of every dense SMM run of the GPU file"""
    return [(c, f, be) for c in (SMM_CASES if cases is None else cases) for f in c.fmts for be in c.betas]


# ---- fsspmdm: a PyFR operator whose values travel as text into the generated kernel ---------------------------------------------
FSSPMDM_N, FSSPMDM_PANELS = 96, 7


def fsspmdm_operator(orc, fmt, extreme):
    """tests/golden/mtx/pyfr/p2_quad_m132 (9 x 18, 48 entries) as a dense row-major matrix. extreme: three entries become the
    smallest subnormal, the largest finite number and -0.0 (which is no entry any more, to the reference and to the kernel)"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mtx", "pyfr", "p2_quad_m132-sp.mtx")
    rowptr, colidx, vals, rows, cols, nnz = orc.read_csr(path)
    t = np_dtype(fmt)
    a = np.zeros((rows, cols), dtype=t)
    for r in range(rows):
        for q in range(rowptr[r], rowptr[r + 1]):
            a[r, colidx[q]] = vals[q]
    if extreme:
        info = np.finfo(t)
        (r0, c0), (r1, c1), (r2, c2) = [(r, int(np.nonzero(a[r])[0][-1])) for r in (1, 4, 7)]
        a[r0, c0] = info.smallest_subnormal
        a[r1, c1] = -info.max
        a[r2, c2] = -0.0
    return a


def fsspmdm_operands(kind, fmt, seed, a, beta):
    """-> B (K, ncols), C (M, ncols) for FSSPMDM_PANELS panels of FSSPMDM_N columns; kind None: uniform(-1, 1). The magnitudes of
    underflow and overflow change from column to column; the specials sit in B (the first and last row and column among them)"""
    rng = np.random.default_rng(seed)
    m, k = a.shape
    ncols = FSSPMDM_N * FSSPMDM_PANELS
    t = np_dtype(fmt)
    emin, emax, p = RANGE[fmt]
    if kind in ("underflow", "overflow"):
        lo, hi = (emin - 26, emin + 10) if kind == "underflow" else (emax - 6, emax - 1)  # (B itself stays finite)
        e = rng.integers(lo, hi + 1, (1, ncols))
        sign = rng.choice([-1.0, 1.0], (1, ncols)) * np.where(rng.integers(0, 8, (k, ncols)) == 0, -1.0, 1.0) if kind == "overflow" else None
        b = _scaled(rng, (k, ncols), e + rng.integers(-1, 2, (k, ncols)), sign)
        c = _scaled(rng, (m, ncols), rng.choice(np.asarray((emin - 1, emin, emin + 1, emin + 2) if kind == "underflow" else (emax - 3, emax - 2, emax - 1, emax)), (m, ncols)))
        return b.astype(t), c.astype(t)
    b, c = rng.uniform(-1, 1, (k, ncols)), rng.uniform(-1, 1, (m, ncols))
    if kind == "specials":
        b[0, 0], b[k - 1, ncols - 1], b[0, ncols // 2], b[k // 2, 5] = np.inf, -np.inf, np.nan, np.inf
        b[k - 1, FSSPMDM_N - 1], b[0, FSSPMDM_N], b[3, 17] = np.nan, -np.inf, -0.0
        r = 2  # a row of the operator against a column of zeros whose signs make every product -0.0, and a C of -0.0
        b[:, 40] = np.where(a[r] > 0, -0.0, 0.0)
        c[r, 40] = -0.0
    return b.astype(t), c.astype(t)


def fsspmdm_reference(orc, a, b, c, beta, ldb=None, ldc=None):
    """the oracle's handle on tight copies, panel by panel: (M, ncols)"""
    m, k = a.shape
    ncols = b.shape[1]
    out = np.ascontiguousarray(c).copy()
    bb = np.ascontiguousarray(b)
    h = orc.Fsspmdm(np.ascontiguousarray(a), m, FSSPMDM_N, k, k, ncols, ncols, 1.0, float(beta), have_avx512=True)
    for pnl in range(ncols // FSSPMDM_N):
        h.execute(bb.reshape(-1)[pnl * FSSPMDM_N:], out.reshape(-1)[pnl * FSSPMDM_N:])
    h.close()
    return out


# ---- the fully-connected layer: one generated chain per pass -------------------------------------------------------------------
FC_CASES = ("b_6_15_14", "lb_5_32_48")  # the smallest blocked fp32 case and the smallest 16-bit case of tests/fc_common.py
FC_FWD, FC_BWD, FC_UPD = 0, 1, 2


# (case, generator, pass) -> added to the seed where the plain one misses a condition of conditions() by a few elements
FC_SHIFT = {("b_6_15_14", "underflow", FC_BWD): 1, ("lb_5_32_48", "underflow", FC_FWD): 2, ("lb_5_32_48", "underflow", FC_UPD): 3,
            ("lb_5_32_48", "overflow", FC_UPD): 1}


def fc_inputs(name, kind, which):
    """plain x [N][C], w [K][C], dy [N][K] (float32) of the case `name` of tests/fc_common.py whose pass `which` is a generated
    chain of `kind` -- y = x w^T, dx = dy w, dw = dy^T x are products of m x n x k = K x N x C, C x N x K, K x C x N --, the third
    tensor uniform(-1, 1); and the chain's operands A (1, m, k), B (1, k, n). The values of the 16-bit case are bf16 numbers."""
    import fc_common
    desc = fc_common.COMPUTE_CASES[name]
    N, C, K = desc["N"], desc["C"], desc["K"]
    lowp = desc["datatype_in"] == 2
    fmt = "bf16" if lowp else "f32"
    seed = seed_of("fc", N, C, K, fmt, kind, which) + FC_SHIFT.get((name, kind, which), 0)
    rng = np.random.default_rng(seed + 1)
    free = lambda shape: bf16_widen(bf16_bits(rng.uniform(-1, 1, shape).astype(np.float32)))
    m, n, k = {FC_FWD: (K, N, C), FC_BWD: (C, N, K), FC_UPD: (K, C, N)}[which]
    if kind is None:
        a, b = free((1, m, k)), free((1, k, n))
    else:
        a, b, _ = operands(kind, fmt, seed, 1, m, n, k)
    if which == FC_FWD:
        w, x, dy = a[0], b[0].T, free((N, K))
    elif which == FC_BWD:
        w, dy, x = a[0].T, b[0].T, free((N, C))
    else:
        dy, x, w = a[0].T, b[0], free((K, C))
    return tuple(np.ascontiguousarray(t) for t in (x, w, dy)), (a, b)


def fc_chains(orc, name, kind):
    """the three passes' inputs and the chains' float32 results: [((x, w, dy), (m, n) result)] for FWD, BWD, UPD. conditions()
    is asked of every result on its own."""
    out = []
    for which in (FC_FWD, FC_BWD, FC_UPD):
        plain, (a, b) = fc_inputs(name, kind, which)
        out.append((plain, chain(orc, a, b, np.zeros((1, a.shape[1], b.shape[2]), np.float32), 0)[0]))
    return out


# ---- low-precision SMM (dispatched kernels: A in pairs of k) ----------------------------------------------------------------------
class LowpCase(object):
    """kind: 0 i16 -> i32, 2 bf16 -> f32, 3 bf16 -> bf16 (the kinds of xo_gemm_lowp); tight items; extras: what the item stride
    adds, in elements of 16 bits (0: back to back, the layout at which several small items share a wave; 8: 16 bytes, the other
    aligned layout; 4 and 1: items that start on 8 and on 2 bytes); reduce: the batch-reduce kernel (arrays of pointers);
    kernel: the name libxsmm_amd_last_kernel has to report; unaligned: the name where the items do not start on 16 bytes (None:
    the same kernel); shift: (generator, beta) -> added to the case's seed"""

    def __init__(self, id, kind, shape, batch, kernel, mfma=0, jit=True, extras=(0, 8, 4, 1), reduce=False, betas=(1, 0), unaligned=None, shift=None):
        self.id, self.kind, self.shape, self.batch, self.kernel, self.mfma, self.jit = id, kind, shape, batch, kernel, mfma, jit
        self.extras, self.reduce, self.betas, self.unaligned, self.shift = extras, reduce, betas, unaligned, dict(shift or {})
        assert all(g in KINDS and be in betas for g, be in self.shift)

    def kernel_at(self, extra):
        return self.kernel if 0 == extra % 8 or self.unaligned is None else self.unaligned

    def operands(self, gen, beta):
        """-> A (batch, m, k), B (batch, k, n) as 16-bit patterns, C (batch or 1, m, n) as int32 / float32 / bf16 patterns"""
        m, n, k = self.shape
        seed = seed_of(self.id, gen, beta) + self.shift.get((gen, beta), 0)
        rng = np.random.default_rng(seed)
        nc = 1 if self.reduce else self.batch
        if self.kind == 0:
            a, b = (rng.integers(-32768, 32768, s).astype(np.int16).view(np.uint16) for s in ((self.batch, m, k), (self.batch, k, n)))
            return a, b, rng.integers(-2 ** 31, 2 ** 31, (nc, m, n)).astype(np.int32)
        if gen is None:
            a, b, c = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((self.batch, m, k), (self.batch, k, n), (nc, m, n)))
        else:
            a, b, c = operands(gen, "bf16", seed, self.batch, m, n, k, np.zeros(self.batch, dtype=np.int64) if self.reduce else None)
            c = np.ascontiguousarray(c[:nc])
        a, b = bf16_bits(a), bf16_bits(b)
        return a, b, (bf16_bits(c) if self.kind == 3 else c)

    def sums(self, a, b, c, beta, fma=None):
        """the float32 sums of the bf16 kinds on the logical matrices: the gold loop (fma None) or the oracle's fma chain"""
        af, bf = bf16_widen(a), bf16_widen(b)
        cf = bf16_widen(c) if self.kind == 3 else c
        one = (lambda x, y, z, be: gold_bf16(x, y, z, be)) if fma is None else (lambda x, y, z, be: chain(fma, x, y, z, be))
        if not self.reduce:
            return one(af, bf, cf, beta)
        acc = cf
        for t in range(self.batch):
            acc = one(af[t:t + 1], bf[t:t + 1], acc, beta if t == 0 else 1)
        return acc

    def inexact(self, a, b):
        hit = inexact_product(bf16_widen(a), bf16_widen(b))
        return hit.any(axis=0, keepdims=True) if self.reduce else hit


LOWP_CASES = [
    LowpCase("lowp-i16-16", 0, (16, 16, 16), 5, "smm_i16i32_jit_shape_lowp"),
    LowpCase("lowp-i16-23x23x22", 0, (23, 23, 22), 5, "smm_i16i32_lowp", jit=False),
    LowpCase("lowp-bf16f32-16", 2, (16, 16, 16), 5, "smm_bf16f32_jit_shape_lowp"),
    LowpCase("lowp-bf16-16", 3, (16, 16, 16), 5, "smm_bf16_jit_shape_lowp"),
    LowpCase("lowp-bf16f32-23x23x22", 2, (23, 23, 22), 5, "smm_bf16f32_jit_shape_lowp"),
    LowpCase("lowp-bf16f32-23x23x22-precompiled", 2, (23, 23, 22), 5, "smm_bf16f32_lowp", jit=False),
    LowpCase("lowp-bf16-32-precompiled", 3, (32, 32, 32), 5, "smm_bf16_lowp", jit=False),
    LowpCase("lowp-bf16f32-32-wave", 2, (32, 32, 32), 5, "smm_bf16f32_mfma_wave_jit_lowp", mfma=1, unaligned="smm_bf16f32_jit_shape_lowp"),
    LowpCase("lowp-bf16-32-wave", 3, (32, 32, 32), 5, "smm_bf16_mfma_wave_jit_lowp", mfma=1, unaligned="smm_bf16_jit_shape_lowp"),
    LowpCase("lowp-bf16f32-32-reduce", 2, (32, 32, 32), 3, "smm_bf16f32_reduce_lowp", reduce=True, extras=(8, 4, 1)),
    LowpCase("lowp-bf16-32-reduce", 3, (32, 32, 32), 3, "smm_bf16_reduce_lowp", reduce=True, extras=(8, 4, 1)),
]


# ---- the packed kernels (pgemm, getrf, trmm, trsm): hostile matrices in three lanes of every pack ----------------------------------
PACKED_PACKS = 3


def packed_cases():
    """(op, format, size) of every descriptor of tests/test_packed_hostile_gpu.py: 8 (register-resident; pgemm 8 x 8 x 8) and 16 (the
    in-place loops) per operation and type. The descriptor does not depend on the kind of values."""
    import packed_common as pc
    return [(op, fmt, size) for op in (pc.PGEMM, pc.GETRF, pc.TRMM, pc.TRSM) for fmt in ("f32", "f64") for size in (8, 16)]


def packed_case(op, fmt, size):
    """the benign case of a descriptor (tests/packed_common.py:Case, three packs). Layout, alpha, side / uplo / trans rotate with the
    format and the size so that every operation sees both layouts and every alpha it takes; triangles are non-unit."""
    import packed_common as pc
    fi, si = ("f32", "f64").index(fmt), (8, 16).index(size)
    j = 2 * fi + si
    layout = pc.COL if fi == si else pc.ROW
    kw = dict(layout=layout, nmat=PACKED_PACKS * pc.width(np_dtype(fmt)), seed=seed_of("packed", op, fmt, size) % (2 ** 31))
    if op == pc.PGEMM:
        ta, tb = (("N", "N"), ("T", "N"), ("N", "T"), ("T", "T"))[j]
        return pc.Case(op, np_dtype(fmt), size, size, size, transa=ta, transb=tb, alpha=(1.0, -1.0)[(j + j // 2) % 2], **kw)
    if op == pc.GETRF:
        return pc.Case(op, np_dtype(fmt), size, size, **kw)
    side, uplo, trans = (("L", "L", "N"), ("R", "U", "N"), ("L", "U", "T"), ("R", "L", "T"))[(j + (1 if op == pc.TRMM else 0)) % 4]
    return pc.Case(op, np_dtype(fmt), size, size, side=side, uplo=uplo, transa=trans, diag="N", alpha=(1.0, -1.0, 0.75)[(j + op) % 3], **kw)


def packed_hostile_lanes(case):
    """indexes (into the case's nmat matrices) of lanes 1, VLEN / 2 and VLEN - 1 of every pack"""
    v = 64 // case.dtype.itemsize
    return np.array([p * v + lane for p in range(case.nmat // v) for lane in (1, v // 2, v - 1)])


class _Tri(object):
    """the effective triangle E (op(A) for side L, its transpose for side R) and the vectors (columns of B for side L, rows for
    side R) of a trmm / trsm case, addressed as the kernels' contract states them"""

    def __init__(self, case):
        self.side_r = case.side == "R"
        self.teff = (case.transa == "T") ^ self.side_r
        self.lower = (case.uplo == "L") ^ self.teff
        self.nt = case.n if self.side_r else case.m
        self.nv = case.m if self.side_r else case.n
        self.order = list(range(self.nt)) if self.lower else list(range(self.nt - 1, -1, -1))  # elimination order of trsm

    def e(self, r, c):
        return (c, r) if self.teff else (r, c)

    def v(self, r, q):
        return (q, r) if self.side_r else (r, q)

    def triangle(self):
        """[(r, c)] of the strict triangle of E"""
        return [(r, c) for r in range(self.nt) for c in range(self.nt) if (c < r if self.lower else c > r)]


def packed_hostile(case, kind):
    """a copy of `case` whose lanes packed_hostile_lanes() hold hostile matrices of `kind`; everything else (the benign lanes, the
    NaN in what a triangle never reads) stays. Per operation, hostile matrix h = 0 ... 8 takes recipe h modulo the number of recipes:

    specials   pgemm: operands("specials") (its -0.0 row of A takes the sign that alpha = -1 turns into -0.0).
               getrf: (0) NaN in the last element, Inf in the first line; (1) a(0,0) = 0; (2) an all-zero row 2 against an Inf in the
               last column of row 0; (3) -0.0 in the last element of column 0 (l = -0.0 is stored).
               trsm: (0) NaN in the last element of B, Inf in its first line; (1) t(1,1) = 0; (2) a triangle whose off-diagonal entries
               are all zero against an Inf in the first unknown of a vector; (3) a vector of -0.0 and a vector of +0.0 (alpha = 1, -1
               or 0.75 and the sign of the pivot decide which of the two ends as -0.0).
               trmm: (0) as trsm; (1) an all-zero triangle (diagonal included) against an Inf in B: 0 * Inf in one vector, signed zeros
               in all others; (2) the two vectors of zeros.
    underflow  pgemm: operands("underflow"). The others: matrix 0 has the pivot 1.5 * 2^(emin - 1) (subnormal, its reciprocal finite and
               inexact), matrix 1 the pivot 2^(emin - 4) (its reciprocal is Inf) -- getrf a(0,0), trsm t(1,1); trmm, which has no pivot,
               takes these two as entries of the diagonal. All other matrices are the benign ones with their vectors (getrf: the columns
               of A) scaled by powers of two, so that X, C or U land among the subnormals and round there.
               Changed against the first recipe (one scale of 2^(emin + 2) for a whole matrix), which left fewer than a quarter of the
               results subnormal: the vectors alternate between 2^(emin - 4) and 2^(emin + 4) (getrf: seven columns of eight at
               2^(emin - 2), where the reciprocal of every pivot stays finite, the eighth at 2^(emin + 4)), and seven of the nine
               matrices are of this kind.
    overflow   pgemm: operands("overflow"), and in matrix 0 a triple whose product 2^(emax + 1) overflows on its own while the fused
               result 2^emax is finite. The others: matrix 0 holds such a triple where the kernel has its fma (getrf: the update of
               w(1,1); trsm: the first update of the second unknown; trmm: the first term after the diagonal), in benign surroundings;
               the other matrices have entries of one sign per vector but for one in eight, and chains that pass 2^(emax + 1) in some
               elements and stay finite in others. Changed against the first recipe (benign matrices scaled to 2^(emax - 7) ...
               2^(emax + 1)), which left fewer than an eighth of the results Inf: trmm takes a positive triangle in 1 ... 2 and vectors at
               2^(emax - 3) ... 2^emax; trsm a diagonal in 0.5 ... 1 and a negative triangle, so that the unknowns of a vector grow with
               one sign; getrf a left half that is nearly lower triangular with l in -4 ... -1 and a positive right half at 2^(emax - 1)
               and 2^emax, whose updates all add (the comments in the code give the details)."""
    import copy
    import packed_common as pc
    assert kind in KINDS
    fmt = fmt_of(case.dtype)
    emin, emax, p = RANGE[fmt]
    half = (emax + 1) // 2
    out = copy.copy(case)
    ops = {name: x.astype(np.float64) for name, x in case.ops.items()}
    lanes = packed_hostile_lanes(case)
    rng = np.random.default_rng(seed_of("packed-hostile", case.kind, fmt, case.m, kind))
    m, n = case.m, case.n
    alpha = case.alpha
    sgn = 1.0 if alpha > 0 else -1.0
    if case.kind == pc.PGEMM:
        k = case.k
        a, b, c = operands(kind, fmt, seed_of("packed-hostile", fmt, case.m, kind), len(lanes), m, n, k)
        a, b, c = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
        if kind == "specials":
            for t in range(len(lanes)):
                if np.all(a[t, 1, :] == 0) and np.all(np.signbit(a[t, 1, :])):
                    a[t, 1, :] *= alpha  # (alpha = -1: +0.0, which the kernel negates)
        elif kind == "overflow":
            a[0, m - 1, :] = 0.0
            a[0, m - 1, 0] = alpha * 2.0 ** half
            b[0, 0, n - 1] = 2.0 ** half
            c[0, m - 1, n - 1] = -2.0 ** emax
        ops["a"][lanes] = a.transpose(0, 2, 1) if case.transa == "T" else a
        ops["b"][lanes] = b.transpose(0, 2, 1) if case.transb == "T" else b
        ops["c"][lanes] = c
    elif case.kind == pc.GETRF:
        a = ops["a"]
        for h, t in enumerate(lanes):
            if kind == "specials":
                r = h % 4
                if r == 0:
                    a[t, m - 1, n - 1] = np.nan
                    if case.layout == pc.COL:
                        a[t, m // 2, 0] = np.inf
                    else:
                        a[t, 0, n // 2] = np.inf
                elif r == 1:
                    a[t, 0, 0] = 0.0
                elif r == 2:
                    a[t, 2, :] = 0.0
                    a[t, 0, n - 1] = np.inf
                else:
                    a[t, 0, 0] = abs(a[t, 0, 0])
                    a[t, m - 1, 0] = -0.0
            elif kind == "underflow":
                if h == 0:
                    a[t, 0, 0] = 1.5 * 2.0 ** (emin - 1)
                elif h == 1:
                    a[t, 0, 0] = 2.0 ** (emin - 4)
                else:
                    a[t] *= np.exp2(np.where(np.arange(n) % 8 != 7, emin - 2, emin + 4).astype(np.float64))[None, :]
            else:
                if h == 0:
                    a[t, 0, 0], a[t, 1, 0], a[t, 0, 1], a[t, 1, 1] = 1.0, -2.0 ** half, 2.0 ** half, -2.0 ** emax
                else:
                    # the left half of the columns is nearly lower triangular -- a diagonal in 0.25 ... 0.5, -0.5 ... -1 below it, 2^-10
                    # above it --, so that every l is negative, 1 ... 4 in magnitude, and stays so; the right half is positive but for one
                    # sign in eight, at 2^emax and 2^(emax - 1) in turn: its updates all add, the chains pass 2^(emax + 1) from the second
                    # or third row on and stay +Inf (the rows below the first pivot that is Inf end as NaN, whatever a kernel does)
                    nl = n // 2
                    rr, cc = np.arange(m)[:, None], np.arange(n)[None, :]
                    mag = rng.uniform(0.5, 1.0, (m, n))
                    left = np.where(rr > cc, -mag, np.where(rr == cc, 0.5 * mag, mag * 2.0 ** -10))
                    right = mag * np.where(rng.integers(0, 8, (m, n)) == 0, -1.0, 1.0) * np.exp2((emax - cc % 2).astype(np.float64))
                    a[t] = np.where(cc < nl, left, right)
    else:
        tri = _Tri(case)
        a, b = ops["a"], ops["b"]
        nt, nv = tri.nt, tri.nv
        c0, r1 = tri.order[0], tri.order[1]
        solve = case.kind == pc.TRSM
        for h, t in enumerate(lanes):
            A, B = a[t], b[t]
            if kind == "specials":
                r = h % (4 if solve else 3)
                if not solve and r > 0:
                    r += 1  # (trmm has no pivot: recipes 0, 2, 3)
                if r == 0:
                    B[m - 1, n - 1] = np.nan
                    if case.layout == pc.COL:
                        B[m // 2, 0] = np.inf
                    else:
                        B[0, n // 2] = np.inf
                elif r == 1:
                    A[1, 1] = 0.0
                elif r == 2:
                    for rc in tri.triangle():
                        A[tri.e(*rc)] = 0.0
                    if not solve:
                        A[np.arange(nt), np.arange(nt)] = 0.0
                    B[tri.v(c0 if solve else nt // 2, 1)] = np.inf
                else:
                    for rr in range(nt):
                        B[tri.v(rr, 0)] = -0.0
                        B[tri.v(rr, nv - 1)] = 0.0
            elif kind == "underflow":
                if h == 0:
                    A[1, 1] = 1.5 * 2.0 ** (emin - 1)
                elif h == 1:
                    A[1, 1] = 2.0 ** (emin - 4)
                else:
                    for q in range(nv):
                        for rr in range(nt):
                            B[tri.v(rr, q)] *= 2.0 ** (emin - 4 if q % 2 == 0 else emin + 4)
            else:
                if h == 0:
                    # |alpha| = 1: product 2^(emax + 1), addend -2^emax; alpha = 0.75: product 1.5 * 2^(emax + 1), addend -1.125 * 2^emax
                    big = half if abs(alpha) == 1.0 else half + 1
                    if solve:  # x[r1] = fma(-E(r1, c0), x[c0], x[r1]) with x = alpha b and E(c0, c0) = 1
                        A[tri.e(c0, c0)] = 1.0
                        A[tri.e(r1, c0)] = -sgn * 2.0 ** big
                        B[tri.v(c0, 0)] = 2.0 ** half
                        B[tri.v(r1, 0)] = -sgn * 2.0 ** emax * (1.0 if abs(alpha) == 1.0 else 1.5)
                    else:      # s = E(r, r) x[r], then s = fma(E(r, c), x[c], s) with c the only entry of the row's triangle
                        r, c = r1, c0
                        A[tri.e(r, r)] = 1.0
                        A[tri.e(r, c)] = 2.0 ** half
                        B[tri.v(c, 0)] = 2.0 ** half
                        B[tri.v(r, 0)] = -2.0 ** emax
                else:
                    # trsm: a positive diagonal in 0.5 ... 1 and negative entries in the triangle, so that every update adds to an unknown
                    # of the vector's sign; trmm: a positive triangle. One sign in eight flipped. Vector q at 2^(e_q).
                    flip = lambda: (-1.0 if rng.integers(0, 8) == 0 else 1.0)
                    for rc in tri.triangle():
                        A[tri.e(*rc)] = (-rng.uniform(0.5, 1.0) if solve else rng.uniform(1.0, 2.0)) * flip()
                    for rr in range(nt):
                        A[tri.e(rr, rr)] = rng.uniform(0.5, 1.0)
                    for q in range(nv):
                        e = emax - (4 * q) // nv
                        s = rng.choice([-1.0, 1.0])
                        for rr in range(nt):
                            B[tri.v(rr, q)] = s * flip() * rng.uniform(0.5, 1.0) * 2.0 ** e
    with np.errstate(over="ignore"):
        out.ops = {name: x.astype(case.dtype) for name, x in ops.items()}
    for name in out.ops:  # the benign lanes keep their bits
        keep = np.ones(case.nmat, bool); keep[lanes] = False
        assert raw(out.ops[name][keep]).tobytes() == raw(case.ops[name][keep]).tobytes()
    return out


def packed_fused_spot(case):
    """(matrix, row, column) of the written operand where hostile matrix 0 of the overflow kind has its planted triple: the product
    alone is beyond the largest finite number, the fused result is finite"""
    import packed_common as pc
    t = int(packed_hostile_lanes(case)[0])
    if case.kind == pc.PGEMM:
        return t, case.m - 1, case.n - 1
    if case.kind == pc.GETRF:
        return t, 1, 1
    tri = _Tri(case)
    return (t,) + tri.v(tri.order[1], 0)


def packed_conditions(kind, ref):
    """what the oracle's results in the hostile lanes (any shape) have to show, so that the comparison with them compares something: the
    fractions of conditions(), but for the share of NaN among the specials, which may reach three quarters (a zero pivot of getrf leaves a
    whole trailing matrix NaN, whatever a kernel does)"""
    ref = np.asarray(ref)
    if kind != "specials":
        return conditions(kind, ref)
    nnan = np.sum(np.isnan(ref))
    assert 1 <= nnan <= 3 * ref.size / 4, ("NaN", int(nnan), ref.size)
    assert np.isinf(ref).any(), "no Inf"
    assert np.any((ref == 0) & np.signbit(ref)), "no -0.0"
