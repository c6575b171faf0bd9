"""The kernel forms of the spmdm batch family (libxsmm_amd_spmdm_batch_create_slices / _compute; csrc/kernels/sparse.hip), as the
shape tests assume them, and the table of shapes those tests run.

The launchers pick a kernel by geometry alone. plan() restates their choice: the create kernel (staged, or one wavefront per slice
with its eight-rows path "rows8" for slices of at most 64 columns and its loop over chunks of 64 columns "chunks" beyond), and the
compute kernel with its instantiation -- ("wg", NB), ("mfma", NT, FULL), ("mfma|wg", NT, FULL, NB) when both are launched and
spm_batch_is_dense decides on the device which one works, ("elem",). SOURCE lists the lines of the sources this restatement rests
on; check_source() holds them against the sources and names the line that changed. tests/test_spmdm_batch_census_cpu.py fails when
a class (an instantiation the source compiles, a create kernel or sub-path) has no case in CASES that makes it do the work;
tests/test_spmdm_batch_shapes_gpu.py runs every case.

Operands come from operands(case): flat arrays in the layout the interface takes (tight items; a transposed operand is stored
transposed), made from a seed that depends on the case's id only."""
import collections
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libxsmm-1_amd", "csrc")
SPARSE, HOST = "kernels/sparse.hip", "xsmm_sparse.cpp"

SPW_LDB, SPW_META, SPM_META, LDS_B_BYTES = 64, 2560, 2304, 49152
NB_LADDER = (1, 2, 3, 4, 6, 8, 12)
DENSE_PERCENT = 28

# (file, the line as the source spells it with <N> for a number the cases assume, those numbers)
SOURCE = [
    (SPARSE, "constexpr int SPW_LDB = <N>;", (SPW_LDB,)),
    (SPARSE, "constexpr int SPW_META = <N>;", (SPW_META,)),
    (SPARSE, "constexpr int SPM_META = <N>;", (SPM_META,)),
    (HOST, "sb->g.cap = (M * K + <N>) & ~<N>; sb->g.rstride = (M + 2) & ~1;", (7, 7)),
    (HOST, "(long long)M * K > <N> || K > <N>) return nullptr;", (65535, 65535)),
    # create
    (SPARSE, "if (0 != staged && g.k <= <N> && g.m <= <N> && 0 == (g.cap & 7)) {", (64, 255)),
    (SPARSE, '*name = "spmdm_create_slices_staged";', ()),
    (SPARSE, '*name = "spmdm_create_slices_wave";\n if (0 == g.batch) return 0;', ()),
    (SPARSE, "if (ncols <= <N>) { // one 64-column chunk per row: fetch eight rows at a time", (64,)),
    (SPARSE, "for (; r_done + <N> <= nrows; r_done += <N>) {", (8, 8)),
    (SPARSE, "for (int r = r_done; r < nrows; ++r) {", ()),
    (SPARSE, "for (int c0 = 0; c0 < ncols; c0 += <N>) {", (64,)),
    # compute
    (SPARSE, "const bool gather_fits = (0 == transb && 0 == transc && g.n <= <N> && 0 == (g.n & <N>) && 16 * g.k <= SPW_META"
             " && (long long)g.k * SPW_LDB * 4 <= <N> && 0 < g.batch && g.m <= <N> && 0 == (g.cap & 7));", (64, 3, LDS_B_BYTES, 255)),
    (SPARSE, "const bool mfma_fits = ((0 <= mfma_env ? 0 != mfma_env : 0 != libxsmm_amd_get_mfma()) && 0 == transb && 0 == transc && 0 < g.batch"
             " && g.m <= <N> && 0 == (g.m & <N>) && g.k <= <N> && 0 == (g.k & <N>) && g.n <= <N> && 0 == (g.n & <N>) && 0 == (g.cap & 7));",
     (64, 15, 64, 3, 64, 15)),
    (SPARSE, "const int paired = (mfma_fits && gather_fits && 0 > mfma_env) ? 1 : 0;", ()),
    (SPARSE, "if (gather_fits && (0 != paired || !mfma_fits)) {", ()),
    (SPARSE, "const int nb = (int)((tile / <N> + <N>) / <N>);", (4, 255, 256)),
    (SPARSE, "if (nb <= <N>) XSMM_SPW(<N>); else if (nb <= <N>) XSMM_SPW(<N>); else if (nb <= <N>) XSMM_SPW(<N>); else if (nb <= <N>) XSMM_SPW(<N>);"
             " else if (nb <= <N>) XSMM_SPW(<N>); else if (nb <= <N>) XSMM_SPW(<N>); else XSMM_SPW(<N>);",
     (1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 12)),
    (SPARSE, '*name = "spmdm_compute_wg_lds";', ()),
    (SPARSE, "if (0 == paired) return (int)hipGetLastError();", ()),
    (SPARSE, "const int nt = g.n / <N>;", (16,)),
    (SPARSE, '*name = (0 != paired) ? "spmdm_compute_mfma|wg_lds" : "spmdm_compute_mfma";', ()),
    (SPARSE, "if (<N> == g.m && <N> == g.k) { if (1 == nt) XSMM_SPM(1, true); else if (2 == nt) XSMM_SPM(2, true); else if (3 == nt) XSMM_SPM(3, true);"
             " else XSMM_SPM(4, true); }", (64, 64)),
    (SPARSE, "else { if (1 == nt) XSMM_SPM(1, false); else if (2 == nt) XSMM_SPM(2, false); else if (3 == nt) XSMM_SPM(3, false); else XSMM_SPM(4, false); }", ()),
    (SPARSE, '*name = "spmdm_compute_elem";', ()),
    # the device's choice between the two kernels of a pair
    (SPARSE, "for (int j = 0; j < <N>; ++j) total += rowidx[((batch * j) >> <N>) * rstride + M];", (16, 4)),
    (SPARSE, "return 100 * total >= <N>LL * 16 * M * K;", (DENSE_PERCENT,)),
]


def _read(path):
    with open(os.path.join(CSRC, path)) as f:
        return f.read()


def _pattern(line):
    """the regular expression of a SOURCE line: numbers at <N>, any spacing and line breaks where the line has a blank"""
    parts = [r"\s*".join(re.escape(w) for w in piece.split()) for piece in line.split("<N>")]
    return r"\s*(\d+)\s*".join(parts)


def check_source(source=None):
    """every line of SOURCE against the sources; returns the list of complaints"""
    bad = []
    for path, line, values in (SOURCE if source is None else source):
        found = re.search(_pattern(line), _read(path))
        if found is None:
            bad.append("%s no longer has the line: %s" % (path, line))
        elif tuple(int(v) for v in found.groups()) != tuple(values):
            bad.append("%s: %s -- has %s where the cases assume %s" % (path, line, found.groups(), tuple(values)))
    return bad


def compiled_classes():
    """the classes the source compiles: every XSMM_SPW(n), every XSMM_SPM(n, true|false), the element kernel, and the two create
    kernels with the wave kernel's two sub-paths"""
    text = _read(SPARSE)
    classes = set(("wg", int(n)) for n in re.findall(r"XSMM_SPW\((\d+)\);", text))
    classes |= set(("mfma", int(n), full == "true") for n, full in re.findall(r"XSMM_SPM\((\d+),\s*(true|false)\);", text))
    if re.search(r"hipLaunchKernelGGL\(spmdm_compute_kernel,", text):
        classes.add(("elem",))
    if re.search(r"hipLaunchKernelGGL\(spmdm_create_staged_kernel, dim3\(grid_for\(g\.batch", text):
        classes.add(("create", "staged"))
    if re.search(r"hipLaunchKernelGGL\(spmdm_create_kernel, dim3\(grid_for\(g\.batch", text):
        classes |= set([("create", "wave", "rows8"), ("create", "wave", "chunks")])
    return classes


Plan = collections.namedtuple("Plan", "create create_path compute inst")


def plan(M, N, K, transb=False, transc=False, mfma=1):
    """what launch_spmdm_create and launch_spmdm_compute do with this geometry (XSMM_SPMDM_MFMA and XSMM_SPMDM_CREATE_STAGED unset)"""
    cap = (M * K + 7) & ~7
    if K <= 64 and M <= 255 and 0 == (cap & 7):
        create, path = "spmdm_create_slices_staged", "staged"
    else:
        create, path = "spmdm_create_slices_wave", ("rows8" if K <= 64 else "chunks")
    plain = not transb and not transc
    gather_fits = plain and N <= 64 and 0 == (N & 3) and 16 * K <= SPW_META and K * SPW_LDB * 4 <= LDS_B_BYTES and M <= 255 and 0 == (cap & 7)
    mfma_fits = bool(mfma) and plain and M <= 64 and 0 == (M & 15) and K <= 64 and 0 == (K & 3) and N <= 64 and 0 == (N & 15) and 0 == (cap & 7)
    nb = (K * N // 4 + 255) // 256
    NB = next((step for step in NB_LADDER if nb <= step), NB_LADDER[-1])
    NT, FULL = N // 16, (64 == M and 64 == K)
    if mfma_fits and gather_fits:
        return Plan(create, path, "spmdm_compute_mfma|wg_lds", ("mfma|wg", NT, FULL, NB))
    if gather_fits:
        return Plan(create, path, "spmdm_compute_wg_lds", ("wg", NB))
    if mfma_fits:  # (no geometry: what fits the matrix cores fits the gather kernel)
        return Plan(create, path, "spmdm_compute_mfma", ("mfma", NT, FULL))
    return Plan(create, path, "spmdm_compute_elem", ("elem",))


def batch_is_dense(counts, M, K):
    """spm_batch_is_dense: the entry counts of sixteen items spread over the batch against 28 % of their capacity"""
    batch = len(counts)
    total = sum(int(counts[(batch * j) >> 4]) for j in range(16))
    return 100 * total >= DENSE_PERCENT * 16 * M * K


# pattern: ("density", d) entries kept with probability d; ("dense",) no zero at all; ("even_dense",) / ("odd_dense",) every other item
# full and the rest empty; ("counts", n) the items' entry counts sum to exactly n; ("hostile", d) density d with -0 (no entry), NaN and
# subnormal entries, an all-zero item, an all-zero first row in the first item and an all-zero last row in the last
Case = collections.namedtuple("Case", "id M N K batch pattern trans betas mfma")
BETAS = (0.0, 1.0, 0.5)


def _case(id, M, N, K, batch, pattern, trans="NNN", betas=BETAS, mfma=1):
    return Case(id, M, N, K, batch, pattern, tuple(trans), betas, mfma)


def _build():
    cases = [
        # ---- gather kernel alone, every NB, with K * N at and just past an edge of the ladder
        _case("wg1-window-walk", 255, 4, 160, 24, ("density", 0.15)),      # 6120 entries an item: several windows with NB = 1
        _case("wg6-partial-piece", 30, 36, 114, 40, ("density", 0.3)),      # K * N = 4104: the fifth piece holds 2 of 256 vectors
        _case("wg6-full", 65, 64, 96, 24, ("density", 0.3)),                # K * N = 6144: six full pieces
        _case("wg8", 100, 64, 128, 20, ("density", 0.3)),
        _case("wg12-sparse", 255, 64, 160, 20, ("density", 0.15)),
        _case("wg12-dense", 255, 64, 160, 20, ("dense",)),                  # 40800 entries, sixteen windows of exactly SPW_META
        _case("wg12-odd", 97, 60, 140, 24, ("density", 0.5)),
    ]
    # ---- matrix cores, all eight <NT, FULL>, paired with the gather kernel (mfma = 1) and the gather kernel alone (mfma = 0):
    # 2 % goes to the gather kernel either way, 50 % and 100 % to the matrix cores; 100 % exceeds SPM_META: the tail comes from HBM
    for M, N, K in ((64, 16, 64), (64, 32, 64), (64, 48, 64), (64, 64, 64), (16, 16, 4), (32, 32, 60), (48, 48, 32), (48, 64, 64), (64, 64, 60)):
        for tag, pattern in (("d2", ("density", 0.02)), ("d50", ("density", 0.5)), ("d100", ("dense",))):
            for mfma in (1, 0):
                cases.append(_case("%s-%dx%dx%d-%s" % ("pair" if mfma else "wg", M, N, K, tag), M, N, K, 27, pattern, mfma=mfma))
    cases += [
        # ---- the device's choice: spm_batch_is_dense samples the even items 0 .. 30 of 33
        _case("choice-even-dense", 64, 48, 64, 33, ("even_dense",)),        # the matrix-core kernel works the empty odd items too
        _case("choice-odd-dense", 64, 48, 64, 33, ("odd_dense",)),          # the gather kernel works the dense odd items
        _case("choice-1146", 16, 16, 16, 16, ("counts", 1146)),             # 100 * 1146 < 28 * 16 * 256 = 114688: gather
        _case("choice-1147", 16, 16, 16, 16, ("counts", 1147)),             # 100 * 1147 >= 114688: matrix cores
        _case("choice-batch1", 32, 32, 32, 1, ("density", 0.5)),            # the one item sampled sixteen times
        _case("choice-batch15", 32, 32, 32, 15, ("density", 0.5)),          # item 0 sampled twice
        # ---- element kernel at ordinary sizes, each trigger
        _case("elem-n68", 64, 68, 64, 20, ("density", 0.3)),
        _case("elem-n63", 64, 63, 64, 20, ("density", 0.3)),
        _case("elem-5x1x7", 5, 1, 7, 60, ("density", 0.5), trans="NTT"),
        _case("elem-m256", 256, 64, 64, 20, ("density", 0.3)),
        _case("elem-k161", 64, 64, 161, 20, ("density", 0.3)),
        _case("elem-300x20x200", 300, 20, 200, 20, ("density", 0.15), trans="TNT"),
        _case("elem-transb", 64, 48, 64, 20, ("density", 0.5), trans="NTN"),
        _case("elem-transc", 64, 48, 64, 20, ("density", 0.5), trans="NNT"),
        # ---- create: staged with more than one chunk of rows and several flushes an item
        _case("staged-255x64-dense", 255, 8, 64, 20, ("dense",)),
        _case("staged-255x63-d90", 255, 12, 63, 20, ("hostile", 0.9), trans="TNN"),
        _case("staged-65x1", 65, 4, 1, 40, ("hostile", 0.7)),
        # ---- create: a wavefront per slice, eight rows at a time (at most 64 columns, so 256 rows or more)
        _case("rows8-259x64", 259, 4, 64, 20, ("hostile", 0.5)),            # three rows left for the row loop
        _case("rows8-256x8", 256, 4, 8, 20, ("hostile", 0.5), trans="TNN"),
        _case("rows8-65535x1", 65535, 4, 1, 3, ("hostile", 0.999)),         # row starts up to 65535; seven rows left
        # ---- create: a wavefront per slice, 64 columns a step
        _case("chunks-1x65", 1, 4, 65, 40, ("hostile", 0.5)),
        _case("chunks-40x128", 40, 8, 128, 30, ("hostile", 0.5), trans="TNN"),
        _case("chunks-255x160", 255, 8, 160, 20, ("hostile", 0.9), trans="TNN"),
        _case("chunks-7x200", 7, 4, 200, 40, ("hostile", 0.5)),
        _case("chunks-1x65535", 1, 4, 65535, 3, ("hostile", 0.999)),        # column indexes up to 65534, 65535 entries at most
        _case("chunks-1x65535-full", 1, 4, 65535, 3, ("dense",), betas=(1.0,)),  # the entry count at the end of uint16
        _case("rows8-65535x1-full", 65535, 4, 1, 3, ("dense",), betas=(1.0,)),
    ]
    assert len(set(c.id for c in cases)) == len(cases)
    return cases


CASES = _build()
BY_ID = dict((c.id, c) for c in CASES)

TINY = np.array([2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127], dtype=np.float32)


def seed_of(case):
    return zlib.crc32(case.id.encode())


def _nonzero(rng, shape):
    """uniform in +-[0.25, 1): no zero, nothing that cancels to one"""
    return (rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def logical_a(case):
    """A as (batch, M, K)"""
    rng = np.random.default_rng(seed_of(case))
    batch, M, K = case.batch, case.M, case.K
    kind = case.pattern[0]
    A = _nonzero(rng, (batch, M, K))
    if kind in ("density", "hostile"):
        A[rng.random((batch, M, K)) >= case.pattern[1]] = 0.0
    elif kind in ("even_dense", "odd_dense"):
        A[(1 if kind == "even_dense" else 0)::2] = 0.0
    elif kind == "counts":
        total = case.pattern[1]
        for i in range(batch):
            n = total // batch + (1 if i < total % batch else 0)
            flat = A[i].reshape(-1)
            flat[rng.permutation(M * K)[n:]] = 0.0
    else:
        assert kind == "dense", kind
    if kind == "hostile":
        entries = A != 0
        pick = rng.random((batch, M, K))
        A[pick < 0.03] = -0.0                                               # no entry
        A[(pick >= 0.03) & (pick < 0.05) & entries] = np.nan                # an entry
        if K >= 8:  # subnormal entries, in rows that keep an ordinary entry (the bound of the CPU test is relative to the row's products)
            tiny = (pick >= 0.05) & (pick < 0.08) & entries
            tiny[..., 0] = False
            A[..., 0] = np.where(np.isnan(A[..., 0]) | (A[..., 0] == 0), np.float32(0.75), A[..., 0])
            A[tiny] = rng.choice(TINY, int(tiny.sum()))
        if batch >= 4:
            A[batch // 2] = 0.0                                             # an all-zero item
        A[0, 0, :] = 0.0                                                    # an all-zero first row
        A[batch - 1, M - 1, :] = 0.0                                        # an all-zero last row
    return A


def operands(case):
    """(a, b): flat float32 arrays as the interface takes them; a holds K x M items for TRANS_A, b holds N x K items for TRANS_B"""
    A = logical_a(case)
    rng = np.random.default_rng(seed_of(case) ^ 0x5bd1e995)
    B = rng.uniform(-1, 1, (case.batch, case.K, case.N)).astype(np.float32)
    ta, tb, _ = case.trans
    a = np.ascontiguousarray(A.transpose(0, 2, 1) if ta == "T" else A).reshape(-1)
    b = np.ascontiguousarray(B.transpose(0, 2, 1) if tb == "T" else B).reshape(-1)
    return a, b


def c_operand(case, beta):
    """C before the call, flat, in the layout of the case (N x M items for TRANS_C); NaN where beta == 0 says C is not read"""
    rng = np.random.default_rng(seed_of(case) ^ int(beta * 1024 + 77))
    c = rng.uniform(-1, 1, case.batch * case.M * case.N).astype(np.float32)
    if beta == 0.0:
        c[:] = np.nan
    return c


def views(case, a, b, c):
    """the logical matrices of flat operands: A (batch, M, K), B (batch, K, N), C (batch, M, N)"""
    ta, tb, tc = case.trans
    batch, M, N, K = case.batch, case.M, case.N, case.K
    A = a.reshape(batch, K, M).transpose(0, 2, 1) if ta == "T" else a.reshape(batch, M, K)
    B = b.reshape(batch, N, K).transpose(0, 2, 1) if tb == "T" else b.reshape(batch, K, N)
    Cm = c.reshape(batch, N, M).transpose(0, 2, 1) if tc == "T" else c.reshape(batch, M, N)
    return A, B, Cm


def slice_of(A_item):
    """createSparseSlice by a plain row scan: (rowidx, colidx, values) of one M x K item; -0 is no entry, NaN is one"""
    M, K = A_item.shape
    keep = A_item != 0
    rowidx = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    assert rowidx[-1] <= 65535
    cols = np.broadcast_to(np.arange(K, dtype=np.uint16), (M, K))
    return rowidx.astype(np.uint16), cols[keep], A_item[keep]


def reference(orc, case, a, b, c, beta):
    """the oracle's C (flat, the case's layout) for C before the call = c"""
    ta, tb, tc = case.trans
    ref = c.copy()
    orc.spmdm_exec_batch(orc.FMA, case.M, case.N, case.K, 48, ta, tb, tc, beta, a, b, ref, case.batch, 4)
    return ref


def plan_of(case):
    return plan(case.M, case.N, case.K, case.trans[1] == "T", case.trans[2] == "T", case.mfma)


def covered(case):
    """the classes this case makes do the work: its create kernel (and sub-path), and the compute instantiation -- of a pair, the
    one that spm_batch_is_dense picks for the case's own operands"""
    p = plan_of(case)
    out = set([("create", "staged") if p.create_path == "staged" else ("create", "wave", p.create_path)])
    if p.inst[0] == "mfma|wg":
        counts = (logical_a(case) != 0).reshape(case.batch, -1).sum(axis=1)
        out.add(("mfma", p.inst[1], p.inst[2]) if batch_is_dense(counts, case.M, case.K) else ("wg", p.inst[3]))
    else:
        out.add(p.inst)
    return out


def census(cases=None):
    """class -> ids of the cases that cover it, for every class the source compiles"""
    reached = dict((cls, []) for cls in compiled_classes())
    for case in (CASES if cases is None else cases):
        for cls in covered(case):
            reached.setdefault(cls, []).append(case.id)
    return reached


def missing(cases=None):
    """complaints: the classes no case covers"""
    return ["no case of tests/spmdm_batch_cases.py reaches %s" % (cls,) for cls, ids in sorted(census(cases).items(), key=repr) if not ids]
