"""What tests/test_sparse_text_{cpu,gpu}.py share: seeded sparsity patterns, the shapes, the operands with their layouts and two
references for the kernels generated per pattern (libxsmm-1_amd/csrc/xsmm_generator.cpp): spgemm_{csr_asparse,csc_bsparse,
csc_asparse}_text, soa_{asparse,bsparse,rm_ac,rm_bc}_text and the csr_reg kernels of libxsmm_create_{d,s}csr_reg. Plain numpy.

One form for all kinds. Every kernel computes  C[line, f] (+)= sum over statements p of  val_p * X[k_p, f] : `line` is the index of C
that belongs to the sparse (or shared) operator, f the index that C shares with the dense operand X (a column n, a row m, or a pair
(n, v) / (m, v) of the SOA forms), k the contracted index. The kinds differ in (i) which statements a pattern leaves and in which
order they are met per element of C (Kind.statements), (ii) where X[k, f] and C[line, f] lie in memory (Kind.place), (iii) what
becomes of a line without statements under beta = 0. The tests keep logical arrays X (items, K, F), C (items, lines, F) and the values
array, and place them into flat arrays with hostile_operands.Layout.

Reference 1 (bits): the oracle's statement-order functions on tight copies, item by item (reference1).
Reference 2 (independent of the oracle): the dense operator built from the pattern here, the product in np.longdouble, and a bound
per element: with L statements in the chain and u = 2^-24 / 2^-53, (L + 1) u (|c| + sum |val_p| |x_p|) (reference2).
canonical(): the same chain once more through the oracle's csr_asparse function on a CSR operator made of Kind.statements -- the
vehicle for deliberately wrong restatements (another arithmetic, zeros skipped, the last duplicate wins, ...)."""
import numpy as np

import hostile_operands as ho

PLAIN = ("csr_asparse", "csc_bsparse", "csc_asparse")
SOA = ("soa_asparse", "soa_bcsr", "soa_bcsc")
RM = ("rm_ac", "rm_bc")
KINDS = PLAIN + SOA + RM + ("csr_reg",)
KERNEL = {"csr_asparse": "spgemm_csr_asparse_text", "csc_bsparse": "spgemm_csc_bsparse_text", "csc_asparse": "spgemm_csc_asparse_text",
          "soa_asparse": "soa_asparse_text", "soa_bcsr": "soa_bsparse_text", "soa_bcsc": "soa_bsparse_text", "rm_ac": "soa_rm_ac_text",
          "rm_bc": "soa_rm_bc_text", "csr_reg": "fsspmdm_f%d_csr_cols"}  # (csr_reg: the pre-compiled panel kernel, per format)
# the sparse operator is stored by lines (major = line, idx = k) or by k (major = k, idx = line)
BY_LINE = ("csr_asparse", "csc_bsparse", "soa_asparse", "soa_bcsc", "csr_reg")
A_SHARED = ("csr_asparse", "csc_asparse", "soa_asparse", "rm_bc", "csr_reg")   # the shared operand is the kernel's A (else B)
LEAVES_EMPTY_LINES = ("soa_asparse", "csr_reg")                                  # under beta = 0
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}


def soa_width(fmt):
    return 8 if fmt == "f64" else 16


# ---- patterns: (majors, minors, seed) -> ptr, idx (uint32), values (float64) --------------------------------------------------------
def _csr(lines):
    ptr = np.zeros(len(lines) + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(l) for l in lines])
    idx = np.array([i for l in lines for i, _ in l], dtype=np.uint32)
    val = np.array([v for l in lines for _, v in l], dtype=np.float64)
    # (arrays with a base address even where they are empty: a pattern without entries still passes pointers)
    keep = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])[:len(a)]
    return ptr, keep(idx), keep(val)


def _value(rng):
    return float(rng.choice([-1.0, 1.0]) * rng.uniform(0.125, 1.0))


def p1(rows, cols, seed):
    """about 40 % filled; every major line has an entry and every index occurs; indices ascend within a line"""
    rng = np.random.default_rng(seed)
    fill = rng.random((rows, cols)) < 0.4
    for r in range(rows):
        if not fill[r].any():
            fill[r, rng.integers(cols)] = True
    for c in range(cols):
        if not fill[:, c].any():
            fill[rng.integers(rows), c] = True
    return _csr([[(c, _value(rng)) for c in range(cols) if fill[r, c]] for r in range(rows)])


def _lines(ptr, idx, val):
    return [[(int(idx[p]), float(val[p])) for p in range(ptr[r], ptr[r + 1])] for r in range(len(ptr) - 1)]


def p2(rows, cols, seed):
    """P1 with one major line emptied and one index that never occurs"""
    lines = _lines(*p1(rows, cols, seed))
    gone_line, gone_idx = rows // 2, 1
    return _csr([[] if r == gone_line else [(c, v) for c, v in l if c != gone_idx] for r, l in enumerate(lines)])


def p3(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return _csr([[(c, _value(rng)) for c in range(cols)] for r in range(rows)])


def p4(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return _csr([[] for r in range(rows - 1)] + [[(cols - 1, _value(rng))]])


def p5(rows, cols, seed):
    """P1 with the entries of every line shuffled (a line that the shuffle left ascending is reversed), and one (line, index) pair
    stored twice with two values: the copy goes to the end of the longest line, whose first entry it repeats (the two are not
    neighbours)"""
    rng = np.random.default_rng(seed)
    lines = [[l[i] for i in rng.permutation(len(l))] for l in _lines(*p1(rows, cols, seed))]
    lines = [l[::-1] if all(l[i][0] < l[i + 1][0] for i in range(len(l) - 1)) else l for l in lines]
    l = max(lines, key=len)
    assert len(l) >= 2, "no line of two entries: another seed"
    l.append((l[0][0], -0.5 * l[0][1] + 0.03125))
    return _csr(lines)


def p6(rows, cols, seed):
    """entries at and beyond the cut: P1 over two more indices than the kernel's extent; line 0 holds only such entries"""
    rng = np.random.default_rng(seed)
    lines = _lines(*p1(rows, cols + 2, seed))
    lines[0] = [(cols, _value(rng)), (cols + 1, _value(rng))]
    return _csr(lines)


def p7(rows, cols, seed):
    return _csr([[] for r in range(rows)])


PATTERNS = {"P1": p1, "P2": p2, "P3": p3, "P4": p4, "P5": p5, "P6": p6, "P7": p7}
PALETTE = np.array([0.5, -1.25, 2.0, 0.0625, -0.75])  # csr_reg: at most 31 kinds of values


# ---- a case ---------------------------------------------------------------------------------------------------------------------------
class Case(object):
    """kind, pattern (None for the dense rm forms), format, beta (0 / 1), fma (plain kinds: 0 is multiply-then-add), ld ("gap" /
    "tight"), batch, extra (what the item strides add to ld * extent), shared (stride_dense = 0: one dense operand for all items)"""

    def __init__(self, kind, pattern, fmt, beta, fma=1, ld="gap", batch=1, extra=4, shared=False):
        self.kind, self.pattern, self.fmt, self.beta, self.fma, self.ld, self.batch, self.extra, self.shared = kind, pattern, fmt, beta, fma, ld, batch, extra, shared
        self.dtype = ho.np_dtype(fmt)
        if kind in PLAIN:
            self.M, self.N, self.K, self.V = 7, 5, 6, 1
        elif kind == "csr_reg":
            self.M, self.N, self.K, self.V = 7, soa_width(fmt), 6, 1
        else:
            self.M, self.N, self.K, self.V = 3, 5, 4, soa_width(fmt)
        M, N, K, V = self.M, self.N, self.K, self.V
        self.lines = M if kind in ("csr_asparse", "csc_asparse", "soa_asparse", "rm_bc", "csr_reg") else N
        self.F = {"csr_asparse": N, "csc_bsparse": M, "csc_asparse": N, "soa_asparse": N * V, "soa_bcsr": M * V, "soa_bcsc": M * V,
                  "rm_ac": M * V, "rm_bc": N * V, "csr_reg": N}[kind]
        self.place = "fk" if kind == "csc_asparse" else ("mkv" if kind in ("soa_bcsr", "soa_bcsc", "rm_ac") else "kf")
        gap = (ld == "gap")
        if kind == "csr_asparse":
            self.lda, self.ldb, self.ldc = 0, N + (2 if gap else 0), N + (1 if gap else 0)
        elif kind == "csc_bsparse":
            self.lda, self.ldb, self.ldc = M + (3 if gap else 0), 0, M + (1 if gap else 0)
        elif kind == "csc_asparse":
            self.lda, self.ldb, self.ldc = 0, K + (2 if gap else 0), M + (1 if gap else 0)
        elif kind == "csr_reg":
            self.lda, self.ldb, self.ldc = 0, N + 3, N + 5
        else:
            self.lda, self.ldb, self.ldc = K + 2, N + 3, N + 1
            if kind == "soa_asparse":
                self.lda = 0
            elif kind in ("soa_bcsr", "soa_bcsc"):
                self.ldb = 0
        self.ld_dense = {"kf": self.ldb if kind in A_SHARED else self.lda, "fk": self.ldb, "mkv": self.lda}[self.place]
        self.seed = ho.seed_of("sparse_text", kind, pattern, fmt, beta, fma, ld)
        if kind in RM:  # the shared operand is a plain matrix (K x ldb, or M x lda): every (line, k) is a statement
            self.sr, self.sc, self.sld = (K, N, self.ldb) if kind == "rm_ac" else (M, K, self.lda)
            self.ptr = self.idx = None
            self.nnz = (self.sr - 1) * self.sld + self.sc
        else:
            nmajor, nminor = (self.lines, K) if kind in BY_LINE else (K, self.lines)
            self.ptr, self.idx, vals = PATTERNS[pattern](nmajor, nminor, ho.seed_of("pattern", pattern, nmajor, nminor))
            if kind == "csr_reg":
                vals = PALETTE[np.random.default_rng(self.seed).integers(0, len(PALETTE), len(vals))]
            self.pattern_values = vals
            self.nnz = len(self.idx)

    def id(self):
        return "%s-%s-%s-b%d-%s-%s-n%d+%d%s" % (self.kind, self.pattern, self.fmt, self.beta, "fma" if self.fma else "muladd", self.ld, self.batch,
                                                self.extra, "-shared" if self.shared else "")

    def descriptor_args(self):
        return (self.M, self.N, self.K, self.lda, self.ldb, self.ldc)

    def lanes(self):
        """threads per item (xsmm_generator.cpp: sp_lanes)"""
        if self.kind == "csr_asparse":
            return self.ldc if 0 == self.beta else self.N
        return {"csc_bsparse": self.M, "csc_asparse": self.N, "csr_reg": None}.get(self.kind, self.F)

    # -- which statements a pattern leaves: [(p, line, k)] in the order an element of C meets them; p indexes the shared operand
    def statements(self, last_wins=False):
        kind, K = self.kind, self.K
        if kind in RM:
            if kind == "rm_ac":   # B[k][n], ldb
                return [(k * self.sld + n, n, k) for n in range(self.lines) for k in range(K)]
            return [(m * self.sld + k, m, k) for m in range(self.lines) for k in range(K)]
        ptr, idx = self.ptr, self.idx
        raw = []
        for major in range(len(ptr) - 1):
            for p in range(ptr[major], ptr[major + 1]):
                line, k = (major, int(idx[p])) if kind in BY_LINE else (int(idx[p]), major)
                raw.append((p, line, k))
        inside = [(p, line, k) for p, line, k in raw if line < self.lines and k < K]   # (plain kinds and SOA B sparse drop the rest)
        if kind in ("soa_asparse", "csr_reg"):
            assert len(inside) == len(raw), "entries beyond the operator: soa_pattern_ok rejects them"
        if kind in ("soa_bcsr", "soa_bcsc"):   # per (k, n) the first entry contributes, k ascending
            seen = {}
            for p, line, k in inside:
                if last_wins or (line, k) not in seen:
                    seen[(line, k)] = p
            return sorted(((p, line, k) for (line, k), p in seen.items()), key=lambda t: (t[1], t[2]))
        if kind == "csc_asparse":              # for k ascending, the column's entries in storage order
            return sorted(inside, key=lambda t: (t[1], t[2], t[0]))
        return sorted(inside, key=lambda t: (t[1], t[0]))

    def empty_lines(self):
        """lines of C whose major line of the operator holds no entry at all (the kinds of LEAVES_EMPTY_LINES)"""
        return [m for m in range(self.lines) if self.ptr[m] == self.ptr[m + 1]]

    # -- layouts
    def dense_layout(self, guard=ho.GUARD):
        batch = 1 if self.shared else self.batch
        if self.place == "kf":
            return ho.Layout(self.F, self.K, batch, self.ld_dense * self.V, self.extra, guard)
        if self.place == "fk":
            return ho.Layout(self.K, self.F, batch, self.ld_dense, self.extra, guard)
        return ho.Layout(self.K * self.V, self.M, batch, self.ld_dense * self.V, self.extra, guard)

    def c_layout(self, guard=ho.GUARD):
        if self.place == "kf":
            return ho.Layout(self.F, self.lines, self.batch, self.ldc * self.V, self.extra, guard)
        if self.place == "fk":
            return ho.Layout(self.lines, self.F, self.batch, self.ldc, self.extra, guard)
        return ho.Layout(self.lines * self.V, self.M, self.batch, self.ldc * self.V, self.extra, guard)

    def stride_dense(self):
        return 0 if self.shared else self.dense_layout().stride

    def arrange(self, x):
        """logical (items, R, F) -> the (items, rows, cols) of the layout"""
        if self.place == "kf":
            return np.swapaxes(x, 1, 2)
        if self.place == "fk":
            return x
        t, r = x.shape[0], x.shape[1]
        return x.reshape(t, r, self.M, self.V).transpose(0, 1, 3, 2).reshape(t, r * self.V, self.M)

    def logical(self, y):
        if self.place == "kf":
            return np.swapaxes(y, 1, 2)
        if self.place == "fk":
            return y
        t, r = y.shape[0], y.shape[1] // self.V
        return y.reshape(t, r, self.V, self.M).transpose(0, 1, 3, 2).reshape(t, r, self.M * self.V)

    def flat_dense(self, x, fill, guard=ho.GUARD):
        return ho.surround(np.ascontiguousarray(self.arrange(x)), self.dense_layout(guard), fill)

    def flat_c(self, c, fill, guard=ho.GUARD):
        return ho.surround(np.ascontiguousarray(self.arrange(c)), self.c_layout(guard), fill)

    def peel_c(self, flat, guard=ho.GUARD):
        return np.ascontiguousarray(self.logical(ho.peel(flat, self.c_layout(guard))))

    def peel_dense(self, flat, guard=ho.GUARD):
        return np.ascontiguousarray(self.logical(ho.peel(flat, self.dense_layout(guard))))

    def flat_shared(self, vals, fill, guard=ho.GUARD):
        """guard, the shared operand (values array, or the plain matrix with `fill` in its leading-dimension gap), guard"""
        body = vals
        if self.kind in RM:
            body = np.full(self.nnz, fill, dtype=self.dtype)
            body[(np.arange(self.sr)[:, None] * self.sld + np.arange(self.sc)[None, :]).ravel()] = vals
        band = np.full(guard, fill, dtype=self.dtype)
        return np.concatenate([band, body.astype(self.dtype), band])

    def owned_gap(self, guard=ho.GUARD):
        """flat positions of C outside the matrices that the kernel writes: csr_asparse under beta = 0 clears ldc entries per row"""
        if not (self.kind == "csr_asparse" and 0 == self.beta):
            return np.zeros(0, dtype=np.int64)
        lay = self.c_layout(guard)
        row = np.arange(self.lines)[:, None] * self.ldc + np.arange(self.N, self.ldc)[None, :]
        return (lay.offsets()[:, None, None] + row[None, :, :]).ravel()

    def extent(self, lay, c=False):
        """elements from the first item's start to the last element the kernel touches (the layout's guard aside)"""
        one = (lay.cols - 1) * lay.ld + lay.rows
        if c and self.kind == "csr_asparse" and 0 == self.beta:
            one = lay.cols * lay.ld
        return (lay.batch - 1) * lay.stride + one

    # -- operands
    def shared_values(self, rng):
        if self.kind in RM:
            return rng.uniform(-1, 1, self.sr * self.sc).astype(self.dtype)
        return self.pattern_values.astype(self.dtype)

    def shapes(self):
        return ((1 if self.shared else self.batch), self.K, self.F), (self.batch, self.lines, self.F)

    def uniform(self):
        """-> values, X, C: uniform(-1, 1) (the operator: its pattern's values)"""
        rng = np.random.default_rng(self.seed)
        sx, sc = self.shapes()
        vals = self.shared_values(rng)
        return vals, rng.uniform(-1, 1, sx).astype(self.dtype), rng.uniform(-1, 1, sc).astype(self.dtype)

    def hostile(self, gen):
        """-> values, X, C of one of hostile_operands.KINDS. underflow / overflow: values and X are +-uniform(0.5, 1) * 2^e with the
        exponents of the products spread over emin - 10 ... emin + 9 / emax - 3 ... emax + 4 as a property of (item, f), C at the scale of
        the smallest normal / the largest finite number. specials: uniform(-1, 1) with, in item i, a NaN of X in column i % N, +Inf and
        -Inf in the next two columns -- the +Inf at the k of a stored 0.0 of the values array --, and in the fourth the zeros that make
        every product of one line -0.0 onto a C of -0.0; the values array also takes a -0.0 (away from both Inf)"""
        rng = np.random.default_rng(ho.seed_of(self.seed, gen))
        emin, emax, _ = ho.RANGE[self.fmt]
        sx, sc = self.shapes()
        nv = self.sr * self.sc if self.kind in RM else self.nnz
        if gen in ("underflow", "overflow"):
            # exponents of the products spread over lo ... hi: a property of (item, f), so that the elements of C differ in magnitude
            lo, hi = (emin - 10, emin + 9) if gen == "underflow" else (emax - 3, emax + 4)
            half = lo // 2
            ev = half + rng.integers(-1, 2, nv)
            ex = (lo - half) + rng.integers(0, hi - lo + 1, (sx[0], 1, sx[2])) + rng.integers(-1, 2, sx)
            sv = sxs = None
            if gen == "overflow":  # most terms of a chain pull the same way (else Inf - Inf = NaN would take over)
                sv = np.where(rng.integers(0, 8, nv) == 0, -1.0, 1.0)
                sxs = rng.choice([-1.0, 1.0], (sx[0], 1, sx[2])) * np.where(rng.integers(0, 8, sx) == 0, -1.0, 1.0)
            cexp = (emin - 1, emin, emin + 1, emin + 2) if gen == "underflow" else (emax - 3, emax - 2, emax - 1, emax)
            vals = ho._scaled(rng, (nv,), ev, sv)
            x = ho._scaled(rng, sx, ex, sxs)
            c = ho._scaled(rng, sc, rng.choice(np.asarray(cexp), sc))
            return vals.astype(self.dtype), x.astype(self.dtype), c.astype(self.dtype)
        assert gen == "specials" and not self.shared
        vals = self.shared_values(rng).astype(np.float64)
        x, c = rng.uniform(-1, 1, sx), rng.uniform(-1, 1, sc)
        st = self.statements()
        if self.kind in RM:  # values indexed by statement below: map p (with gap) -> position in the gap-free matrix
            tight = {p: (p // self.sld) * self.sc + p % self.sld for p, _, _ in st}
        else:
            tight = {p: p for p, _, _ in st}
        by_line = {}
        for p, line, k in st:
            by_line.setdefault(line, []).append((p, k))
        dup = set()
        if self.kind not in RM:   # lines that hold a (line, k) pair twice take no planted chain
            seen = set()
            for p, line, k in st:
                if (line, k) in seen:
                    dup.add(line)
                seen.add((line, k))
        la = max(by_line, key=lambda l: (len(by_line[l]), -l))          # the longest line: the stored 0.0 and the -0.0
        assert len(by_line[la]) >= 2
        (p0, k1), (pneg, kneg) = by_line[la][0], by_line[la][1]
        assert k1 != kneg or la in dup
        if k1 == kneg:
            (pneg, kneg) = [(p, k) for p, k in by_line[la] if k != k1][0]
        vals[tight[p0]], vals[tight[pneg]] = 0.0, -0.0
        m1 = [l for l in sorted(by_line) if l != la and l not in dup][0]  # the line whose products are all -0.0
        k0 = st[len(st) // 2][2]                                         # the NaN's k: any k that is read
        k2 = [k for _, _, k in st if k not in (k1, kneg)][0]             # the -Inf's k: neither the 0.0's nor the -0.0's
        N = self.N
        for i in range(sx[0]):
            f0 = i % N
            f1, f2, f3 = (f0 + 1) % N, (f0 + 2) % N, (f0 + 3) % N
            x[i, k0, f0] = np.nan
            x[i, k1, f1] = np.inf            # meets the stored 0.0 in line la: NaN
            x[i, k2, f2] = -np.inf
            for p, k in by_line[m1]:
                v = vals[tight[p]]
                x[i, k, f3] = -0.0 if (v > 0 or (v == 0 and not np.signbit(v))) else 0.0
            c[i, m1, f3] = -0.0
        return vals.astype(self.dtype), x.astype(self.dtype), c.astype(self.dtype)


# ---- references -----------------------------------------------------------------------------------------------------------------------
def _tight(case, arr):
    """one item (R, F) -> flat tight storage of its layout"""
    y = case.arrange(arr[None])[0]
    return np.ascontiguousarray(y.T).ravel()


def _untight(case, flat, r):
    rows = {"kf": case.F, "fk": r, "mkv": r * case.V}[case.place]
    y = flat.reshape(-1, rows).T
    return case.logical(y[None])[0]


def reference1(orc, case, vals, x, c, arith=None):
    """the oracle's function of the kind on tight copies, item by item: (items, lines, F)"""
    kind, M, N, K, V = case.kind, case.M, case.N, case.K, case.V
    arith = (orc.FMA if case.fma else orc.MULADD) if arith is None else arith
    flags = orc.FLAG_BETA_0 if 0 == case.beta else 0
    out = np.empty_like(c)
    vals = np.ascontiguousarray(vals)
    for i in range(c.shape[0]):
        xt = _tight(case, x[0 if case.shared else i])
        ct = _tight(case, c[i]).copy()
        if kind == "csr_asparse":
            orc.csr_asparse(arith, flags, M, N, K, N, N, case.ptr, case.idx, vals, xt, ct)
        elif kind == "csc_bsparse":
            orc.csc_bsparse(arith, flags, M, N, K, M, M, case.ptr, case.idx, xt, vals, ct)
        elif kind == "csc_asparse":
            orc.csc_asparse(arith, flags, M, N, K, K, M, case.ptr, case.idx, vals, xt, ct)
        elif kind == "soa_asparse":
            orc.soa_csr_asparse(flags, M, N, K, N, N, V, case.ptr, case.idx, vals, xt, ct)
        elif kind in ("soa_bcsr", "soa_bcsc"):
            orc.soa_bsparse(flags, kind == "soa_bcsr", M, N, K, K, N, V, case.ptr, case.idx, xt, vals, ct)
        elif kind == "rm_ac":
            orc.soa_rm_ac(flags, M, N, K, K, N, N, V, xt, vals, ct)
        elif kind == "rm_bc":
            orc.soa_rm_bc(flags, M, N, K, K, N, N, V, vals, xt, ct)
        else:
            assert 0 == orc.csr_reg(flags, M, N, K, N, N, case.ptr, case.idx, vals, xt, ct)
        out[i] = _untight(case, ct, case.lines)
    return out


def _operator(case, vals, statements):
    """dense (lines, K) operator, the sum of |values| and the number of statements per line, in long double"""
    s = np.zeros((case.lines, case.K), dtype=np.longdouble)
    sabs = np.zeros_like(s)
    count = np.zeros(case.lines, dtype=np.int64)
    tight = (lambda p: (p // case.sld) * case.sc + p % case.sld) if case.kind in RM else (lambda p: p)
    for p, line, k in statements:
        v = np.longdouble(vals[tight(p)])
        s[line, k] += v
        sabs[line, k] += abs(v)
        count[line] += 1
    return s, sabs, count


def reference2(case, vals, x, c):
    """-> (value, bound) as long double (items, lines, F): see the module's docstring"""
    s, sabs, count = _operator(case, vals, case.statements())
    xl, cl = x.astype(np.longdouble), c.astype(np.longdouble)
    if case.shared:
        xl = np.broadcast_to(xl, (c.shape[0],) + xl.shape[1:])
    start = cl if case.beta else np.zeros_like(cl)
    if 0 == case.beta and case.kind in LEAVES_EMPTY_LINES:
        start[:, case.empty_lines(), :] = cl[:, case.empty_lines(), :]
    value = start + np.einsum("lk,tkf->tlf", s, xl)
    bound = (count[None, :, None] + 1) * np.longdouble(U[case.fmt]) * (np.abs(start) + np.einsum("lk,tkf->tlf", sabs, np.abs(xl)))
    return value, bound


def canonical(orc, case, vals, x, c, arith=None, statements=None, skip_zeros=False, zero_empty=False):
    """the chain of every element of C through the oracle's csr_asparse function on a CSR operator made of the statements, line by
    line in their order. With the defaults this is Reference 1 once more; the arguments make the wrong kernels of the CPU file."""
    st = case.statements() if statements is None else statements
    tight = (lambda p: (p // case.sld) * case.sc + p % case.sld) if case.kind in RM else (lambda p: p)
    if skip_zeros:
        st = [t for t in st if vals[tight(t[0])] != 0]
    lines = [[] for _ in range(case.lines)]
    for p, line, k in st:
        lines[line].append((k, vals[tight(p)]))
    ptr, idx, v = _csr(lines)
    v = np.ascontiguousarray(v.astype(case.dtype))
    arith = (orc.FMA if case.fma else orc.MULADD) if arith is None else arith
    out = np.empty_like(c)
    for i in range(c.shape[0]):
        xi = np.ascontiguousarray(x[0 if case.shared else i])
        ci = np.ascontiguousarray(c[i]).copy()
        orc.csr_asparse(arith, orc.FLAG_BETA_0 if 0 == case.beta else 0, case.lines, case.F, case.K, case.F, case.F, ptr, idx, v, xi.ravel(), ci.reshape(-1))
        if 0 == case.beta and case.kind in LEAVES_EMPTY_LINES and not zero_empty:
            ci[case.empty_lines(), :] = c[i][case.empty_lines(), :]
        out[i] = ci
    return out


# ---- the runs of the GPU file (the CPU file walks the same lists) ---------------------------------------------------------------------
def patterns_of(kind):
    if kind in RM:
        return (None,)
    if kind == "csr_reg":
        return ("P1", "P2", "P4")
    if kind in PLAIN:
        return ("P1", "P2", "P3", "P4", "P5", "P6", "P7")
    return ("P1", "P2", "P3", "P4", "P5", "P7")   # (P6: the plain kinds only; SOA A sparse refuses it)


def combos(kind):
    """(format, beta, fma) in the order of rotation"""
    flavours = (1, 0) if kind in PLAIN else (1,)
    return [(f, b, a) for a in flavours for b in (1, 0) for f in ("f32", "f64")]


def batches(kind):
    return (None,) if kind == "csr_reg" else ((103, 1) if kind in PLAIN else (7, 1))


def pattern_runs(kind):
    """(pattern, format, beta, fma, ld): every pattern twice (the rm forms: every combination once), the combinations in rotation
    so that each occurs; the first run of a plain pattern has gaps in its leading dimensions, the second is tight"""
    cs = combos(kind)
    runs, i = [], 0
    pats = patterns_of(kind)
    times = len(cs) if kind in RM else 2
    for pat in pats:
        for j in range(times):
            f, b, a = cs[i % len(cs)]
            runs.append((pat, f, b, a, "tight" if (kind in PLAIN and j == 1) else "gap"))
            i += 1
    assert set(cs) == set((f, b, a) for _, f, b, a, _ in runs), kind
    return runs


def hostile_runs(kind):
    """(pattern, format, beta, fma) of the gap and value tests: P1 and P2, the plain kinds and SOA B sparse P5 as well; the
    combinations rotate in steps of five (both formats, both betas and, for the plain kinds, both flavours occur)"""
    cs = combos(kind)
    pats = (None, None) if kind in RM else (("P1", "P2", "P5") if (kind in PLAIN or kind in ("soa_bcsr", "soa_bcsc")) else ("P1", "P2"))
    return [(pat,) + cs[(5 * i + 1) % len(cs)] for i, pat in enumerate(pats)]


# ---- the product's side: descriptor and kernel text (argument marshalling only; xs is the binding libxsmm-1_amd) -----------------------
SOA_FORM = {"soa_asparse": 0, "soa_bcsr": 0, "soa_bcsc": 1, "rm_ac": 2, "rm_bc": 3}


def descriptor(xs, fmt, m, n, k, lda, ldb, ldc, beta):
    blob, d = xs.descriptor(xs.F64 if fmt == "f64" else xs.F32, m, n, k, lda, ldb, ldc, 1.0, float(beta), 0, 0)
    assert d
    return blob, d


def pattern_arguments(kind, ptr, idx):
    """(is_csr, row_idx, column_idx) in the reference's argument order"""
    return (1, ptr, idx) if kind in ("csr_asparse", "soa_asparse", "soa_bcsr", "csr_reg") else (0, idx, ptr)


def text_of(xs, kind, fmt, beta, fma, dims, ptr, idx, name="xsmm_spgemm_op"):
    """the kernel text of a plain kind (libxsmm_amd_spgemm_source) or of an SOA kind, the dense rm forms included
    (libxsmm_amd_soa_source), as the translation unit the library compiles -- fma = 0: the same statements as multiply, then add --,
    without compiling it; or None with the entry point's return code"""
    import ctypes as C
    L = xs.lib()
    blob, d = descriptor(xs, fmt, *dims, beta=beta)
    buf = C.create_string_buffer(1 << 18)
    if kind in PLAIN:
        is_csr, ri, ci = pattern_arguments(kind, ptr, idx)
        rc = L.libxsmm_amd_spgemm_source(d, is_csr, xs.dptr(ri), xs.dptr(ci), fma, buf, len(buf), 0)
    else:
        rc = L.libxsmm_amd_soa_source(d, SOA_FORM[kind], xs.dptr(ptr), xs.dptr(idx), fma, buf, len(buf), 0)
    if rc <= 0:
        return None, rc
    text = buf.value.decode()
    assert len(text) == rc
    return text.replace("xsmm_spgemm_op", name), 0


def soa_body(xs, kind, fmt, beta, dims, ptr, idx):
    """the statements libxsmm_generator_spgemm_{csr,csc}_soa_kernel append (the reference's text entry points), or None with the
    generator's error code"""
    import ctypes as C
    L = xs.lib()
    blob, d = descriptor(xs, fmt, *dims, beta=beta)
    is_csr, ri, ci = pattern_arguments(kind, ptr, idx)
    code = xs.GeneratedCode()
    f = L.libxsmm_generator_spgemm_csr_soa_kernel if is_csr else L.libxsmm_generator_spgemm_csc_soa_kernel
    f(C.byref(code), d, b"gfx950", xs.dptr(ri), xs.dptr(ci), xs.dptr(np.ones(max(1, len(idx)))))
    if 0 != code.last_error:
        return None, code.last_error
    body = code.text()
    code.release()
    return body, 0


def hostile_case(kind, pat, fmt, beta, fma):
    return Case(kind, pat, fmt, beta, fma, "gap", batches(kind)[0] or 1, 4)
