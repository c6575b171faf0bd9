"""The cases, references and comparison of tests/test_sparse_text_gpu.py checked without a GPU, and the generated text itself:

  1. the conditions on every generated case (hostile_operands.conditions on the reference alone) and Reference 1 (the oracle's
     statement-order functions) within the derived bound of Reference 2 (the dense operator built here, the product in long double):
     a rule that the oracle and the generator misread in the same way -- which duplicate counts, what a cut drops, what becomes of a
     line without entries -- shows here;
  2. deliberately wrong restatements of a kernel, each of which the comparison has to reject;
  3. the generated text run on the host: every plain and SOA case (A or B sparse, and the dense rm_ac / rm_bc), both arithmetics,
     the translation units of libxsmm_amd_spgemm_source / libxsmm_amd_soa_source compiled by the host compiler with the address and
     undefined-behaviour sanitizers into a stand-alone program that calls the kernel once per (block, thread) on heap blocks of
     exactly the extent the kernel may touch. The result must be the bits of Reference 1. (csr_reg is no text kernel on this
     engine: the GPU file alone covers it.)
  4. leading dimensions at which an element offset passes 2^31, or begins within an item's lanes of it: every literal offset in the
     text is the 64-bit product, and every index expression that adds a lane to it holds the sum in 64 bits."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import hostile_operands as ho
import sparse_text_cases as st

TEXT_KINDS = st.PLAIN + st.SOA + st.RM


# ---- 1. conditions and references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.KINDS)
def test_reference_1_within_the_bound_of_reference_2(orc, kind):
    ho.assert_environment(orc)
    seen = set()
    for (pat, fmt, beta, fma, ld) in st.pattern_runs(kind):
        for batch in st.batches(kind):
            for extra, shared in ((4, False), (1, True)):
                case = st.Case(kind, pat, fmt, beta, fma, ld, batch or 1, extra, shared)
                vals, x, c = case.uniform()
                r1 = st.reference1(orc, case, vals, x, c)
                value, bound = st.reference2(case, vals, x, c)
                excess = np.abs(r1.astype(np.longdouble) - value) - bound
                assert np.all(excess <= 0), (case.id(), float(excess.max()))
                assert np.array_equal(ho.raw(r1), ho.raw(st.canonical(orc, case, vals, x, c))), case.id()
                # the layouts give back what was put in, and nothing lies outside the allocation
                for flat, peel, lay, src, is_c in ((case.flat_dense(x, case.dtype(np.nan)), case.peel_dense, case.dense_layout(), x, False),
                                                   (case.flat_c(c, case.dtype(np.nan)), case.peel_c, case.c_layout(), c, True)):
                    assert np.array_equal(peel(flat), src) and np.isnan(flat[~lay.mask()]).all() and lay.mask().sum() == src.size
                    assert 2 * lay.guard + case.extent(lay, c=is_c) <= lay.total
                own = case.owned_gap()
                assert not case.c_layout().mask()[own].any() and (own.size > 0) == (kind == "csr_asparse" and beta == 0 and ld == "gap")
                seen.add((pat, fmt, beta, fma))
    # every pattern at least twice, every combination at least once
    for pat in st.patterns_of(kind):
        assert sum(1 for p, _, _, _ in seen if p == pat) >= (2 if kind not in st.RM else 4), pat
    assert set((f, b, a) for _, f, b, a in seen) == set(st.combos(kind))


def test_patterns_are_what_they_claim():
    for rows, cols in ((7, 6), (5, 6), (6, 7), (3, 4), (4, 5), (5, 4)):
        seed = ho.seed_of("pattern", rows, cols)
        ptr, idx, val = st.p1(rows, cols, seed)
        assert all(ptr[r] < ptr[r + 1] for r in range(rows)) and set(idx.tolist()) == set(range(cols)) and 0.25 <= len(idx) / (rows * cols) <= 0.7
        assert all(list(idx[ptr[r]:ptr[r + 1]]) == sorted(idx[ptr[r]:ptr[r + 1]]) for r in range(rows))
        ptr, idx, val = st.p2(rows, cols, seed)
        assert sum(ptr[r] == ptr[r + 1] for r in range(rows)) >= 1 and 1 not in idx
        ptr, idx, val = st.p3(rows, cols, seed)
        assert len(idx) == rows * cols
        ptr, idx, val = st.p4(rows, cols, seed)
        assert list(ptr) == [0] * rows + [1] and list(idx) == [cols - 1]
        ptr, idx, val = st.p5(rows, cols, seed)
        pairs = [(r, int(idx[p])) for r in range(rows) for p in range(ptr[r], ptr[r + 1])]
        assert len(pairs) - len(set(pairs)) == 1
        twice = [q for q in set(pairs) if pairs.count(q) == 2][0]
        first, second = [i for i, q in enumerate(pairs) if q == twice]
        assert second - first >= 2 and val[first] != val[second]
        assert any(idx[p] > idx[p + 1] for r in range(rows) for p in range(ptr[r], ptr[r + 1] - 1))
        ptr, idx, val = st.p6(rows, cols, seed)
        assert (idx == cols).any() and (idx > cols).any() and all(i >= cols for i in idx[ptr[0]:ptr[1]])
        ptr, idx, val = st.p7(rows, cols, seed)
        assert len(idx) == 0 and list(ptr) == [0] * (rows + 1)


@pytest.mark.parametrize("gen", ho.KINDS)
def test_conditions_on_the_hostile_cases(orc, gen):
    ho.assert_environment(orc)
    for kind in st.KINDS:
        runs = st.hostile_runs(kind)
        assert {b for _, _, b, _ in runs} == {0, 1} and {f for _, f, _, _ in runs} == {"f32", "f64"}
        for (pat, fmt, beta, fma) in runs:
            case = st.hostile_case(kind, pat, fmt, beta, fma)
            vals, x, c = case.hostile(gen)
            assert np.isfinite(vals).all() and (gen == "specials" or (np.isfinite(x).all() and np.isfinite(c).all()))
            with np.errstate(all="ignore"):
                want = st.reference1(orc, case, vals, x, c)
            try:
                ho.conditions(gen, want, beta)
            except AssertionError as e:
                raise AssertionError((case.id(),) + e.args)
            if gen == "specials":  # what was planted: the stored zero and the -0.0 among the values, NaN, both Inf and -0.0 in every item of X
                assert np.sum(vals == 0) == 2 and np.sum(np.signbit(vals) & (vals == 0)) == 1
                assert all(np.isnan(x[i]).sum() == 1 and np.isposinf(x[i]).sum() == 1 and np.isneginf(x[i]).sum() == 1 for i in range(x.shape[0]))
                assert np.isnan(want).mean() <= (case.lines + 1) / (case.lines * case.F)   # a column of C and the 0 x Inf, at most
                assert len({int(np.nonzero(np.isnan(x[i]).any(axis=0))[0][0]) for i in range(x.shape[0])}) == min(x.shape[0], case.N)  # placement varies per item


# ---- 2. the comparison rejects wrong kernels --------------------------------------------------------------------------------------------
def flush(a):
    out = a.copy()
    out[np.abs(out) < np.finfo(a.dtype).tiny] *= 0
    return out


def wrong_inputs_flushed(orc, case, vals, x, c):
    return st.canonical(orc, case, flush(vals), flush(x), flush(c))


def wrong_outputs_flushed(orc, case, vals, x, c):
    return flush(st.canonical(orc, case, vals, x, c))


def wrong_other_arithmetic(orc, case, vals, x, c):
    """multiply-then-add where the kernel is fma, fma where it is multiply-then-add"""
    return st.canonical(orc, case, vals, x, c, arith=orc.MULADD if case.fma else orc.FMA)


def wrong_zeros_skipped(orc, case, vals, x, c):
    return st.canonical(orc, case, vals, x, c, skip_zeros=True)


def wrong_last_entry_wins(orc, case, vals, x, c):
    return st.canonical(orc, case, vals, x, c, statements=case.statements(last_wins=True))


def wrong_empty_line_zeroed(orc, case, vals, x, c):
    return st.canonical(orc, case, vals, x, c, zero_empty=True)


def wrong_cut_entries_kept(orc, case, vals, x, c):
    """an entry at the cut (idx == k) read as the last index inside: what a `<=` in the cut would do"""
    extra = [(p, (m if case.kind in st.BY_LINE else case.lines - 1), (case.K - 1 if case.kind in st.BY_LINE else m))
             for m in range(len(case.ptr) - 1) for p in range(case.ptr[m], case.ptr[m + 1]) if case.idx[p] == (case.K if case.kind in st.BY_LINE else case.lines)]
    assert extra
    return st.canonical(orc, case, vals, x, c, statements=sorted(case.statements() + extra, key=lambda t: (t[1], t[0])))


def _rejected(orc, case, wrong, generators):
    hits = []
    for gen in generators:
        vals, x, c = case.uniform() if gen is None else case.hostile(gen)
        with np.errstate(all="ignore"):
            want = st.reference1(orc, case, vals, x, c)
            assert ho.same_values(want, st.canonical(orc, case, vals, x, c)), (case.id(), gen)   # (the vehicle itself is right)
            got = wrong(orc, case, vals, x, c)
        if not ho.same_values(got, want):
            hits.append(gen)
    return hits


@pytest.mark.parametrize("kind", st.KINDS)
@pytest.mark.parametrize("wrong", [wrong_inputs_flushed, wrong_outputs_flushed, wrong_other_arithmetic, wrong_zeros_skipped], ids=lambda w: w.__name__)
def test_same_values_rejects_a_wrong_kernel(orc, kind, wrong):
    ho.assert_environment(orc)
    hits = []
    for (pat, fmt, beta, fma) in st.hostile_runs(kind):
        case = st.hostile_case(kind, pat, fmt, beta, fma)
        here = _rejected(orc, case, wrong, ho.KINDS)
        # the other arithmetic is told apart in every run on its own: fma given for multiply-then-add, and the reverse. (Flushed inputs
        # show only where the chain starts from C, the one operand that holds subnormals: under beta = 1.)
        assert here or wrong is not wrong_other_arithmetic, case.id()
        hits += here
    assert hits, "no generator tells this kernel from a correct one"
    print(kind, wrong.__name__, "rejected on", sorted(set(hits)))


@pytest.mark.parametrize("kind", ["soa_bcsr", "soa_bcsc"])
def test_last_entry_wins_is_rejected(orc, kind):
    """... on plain uniform data already: the two values of the duplicate differ"""
    fmt, beta, fma = [r[1:4] for r in st.pattern_runs(kind) if r[0] == "P5"][0]
    assert _rejected(orc, st.Case(kind, "P5", fmt, beta, fma, "gap", 7, 4), wrong_last_entry_wins, (None,)) == [None]
    # and Reference 2 (first entry wins, written down independently) is not within its bound of such a kernel
    case = st.Case(kind, "P5", fmt, beta, fma, "gap", 7, 4)
    vals, x, c = case.uniform()
    value, bound = st.reference2(case, vals, x, c)
    assert np.any(np.abs(wrong_last_entry_wins(orc, case, vals, x, c).astype(np.longdouble) - value) > bound)


@pytest.mark.parametrize("kind", st.LEAVES_EMPTY_LINES)
def test_an_empty_line_zeroed_is_rejected(orc, kind):
    fmt = [r[1] for r in st.pattern_runs(kind) if r[0] == "P2"][0]
    case = st.Case(kind, "P2", fmt, 0, 1, "gap", 1, 4)
    assert case.empty_lines()
    assert _rejected(orc, case, wrong_empty_line_zeroed, (None,)) == [None]
    vals, x, c = case.uniform()
    value, bound = st.reference2(case, vals, x, c)
    assert np.any(np.abs(wrong_empty_line_zeroed(orc, case, vals, x, c).astype(np.longdouble) - value) > bound)


@pytest.mark.parametrize("kind", st.PLAIN)
def test_an_entry_at_the_cut_kept_is_rejected(orc, kind):
    case = st.Case(kind, "P6", "f64", 1, 1, "gap", 1, 4)
    assert _rejected(orc, case, wrong_cut_entries_kept, (None,)) == [None]


# ---- 3. the generated text on the host -----------------------------------------------------------------------------------------------------
HARNESS_HEAD = r"""
#include <cstdio>
#include <cstdlib>
#define __global__
#define __launch_bounds__(x)
struct xs_dim3 { unsigned x, y, z; };
static xs_dim3 blockIdx, blockDim, threadIdx;
"""

HARNESS_TAIL = r"""
template<class T> static int run(void* fn, const long long* h, FILE* in, FILE* out)
{ /* heap blocks of exactly h[1], h[2], h[3] elements: one element beyond is the sanitizer's */
  typedef void (*kernel_t)(const T*, const T*, T*, long long, long long, long long);
  T* const a = static_cast<T*>(malloc(sizeof(T) * h[1]));
  T* const b = static_cast<T*>(malloc(sizeof(T) * h[2]));
  T* const c = static_cast<T*>(malloc(sizeof(T) * h[3]));
  if ((0 < h[1] && (size_t)h[1] != fread(a, sizeof(T), h[1], in)) || (0 < h[2] && (size_t)h[2] != fread(b, sizeof(T), h[2], in))
    || (0 < h[3] && (size_t)h[3] != fread(c, sizeof(T), h[3], in))) return 1;
  blockDim.x = 256;
  for (long long blk = 0; blk < h[7]; ++blk) for (unsigned t = 0; t < 256; ++t) {
    blockIdx.x = (unsigned)blk; threadIdx.x = t;
    reinterpret_cast<kernel_t>(fn)(a, b, c, h[4], h[5], h[6]);
  }
  if ((size_t)h[3] != fwrite(c, sizeof(T), h[3], out)) return 1;
  free(a); free(b); free(c);
  return 0;
}

int main(int argc, char** argv)
{ /* records: int64[8] = kernel, elements of A, B, C, stride_dense, stride_c, batch, blocks; then A, B, C */
  if (3 != argc) return 2;
  FILE* const in = fopen(argv[1], "rb"); FILE* const out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  long long h[8]; int done = 0;
  while (8 == fread(h, sizeof(long long), 8, in)) {
    if (h[0] < 0 || h[0] >= (long long)(sizeof(table) / sizeof(*table))) return 3;
    if (0 != (4 == table[h[0]].typesize ? run<float>(table[h[0]].fn, h, in, out) : run<double>(table[h[0]].fn, h, in, out))) return 4;
    ++done;
  }
  fclose(in); fclose(out);
  printf("%d records\n", done);
  return 0;
}
"""

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]


def datasets(kind):
    big = st.batches(kind)[0]
    return ((big, 4, False), (1, 1, False), (big, 1, True))


def host_operands(case, vals, x, c):
    """A, B, C of the kernel's argument list as flat arrays without guard bands, cut to the touched extent"""
    fill = case.dtype(np.nan)
    dense = case.flat_dense(x, fill, guard=0)[:case.extent(case.dense_layout(0))]
    cflat = case.flat_c(c, fill, guard=0)[:case.extent(case.c_layout(0), c=True)]
    shared = np.ascontiguousarray(case.flat_shared(vals, fill, guard=0))   # (rm forms: the plain matrix with its gap)
    return ((shared, dense) if case.kind in st.A_SHARED else (dense, shared)) + (cflat,)


def expected_flat(case, ref, guard, fill):
    flat = case.flat_c(ref, fill, guard=guard)
    flat[case.owned_gap(guard)] = 0
    return flat


@pytest.fixture(scope="module")
def host_run(xs, orc, tmp_path_factory):
    """builds one program out of every text and runs every record through it once: {record id: (case, flavour, C as the program left it)}"""
    ho.assert_environment(orc)
    d = tmp_path_factory.mktemp("sparse_text_host")
    units, table, records, payload = [], [], [], []
    for kind in TEXT_KINDS:
        for (pat, fmt, beta, _, ld) in st.pattern_runs(kind):
            for fma in (1, 0):
                proto = st.Case(kind, pat, fmt, beta, fma, ld)
                name = "k%d_op" % len(table)
                text, err = st.text_of(xs, kind, fmt, beta, fma, proto.descriptor_args(), proto.ptr, proto.idx, name)
                assert text is not None, (proto.id(), err)
                units.append("namespace ns_%s {\n%s}\n#undef XACC\n" % (name, text))
                table.append("  { %d, reinterpret_cast<void*>(&ns_%s::%s) }" % (8 if fmt == "f64" else 4, name, name))
                for batch, extra, shared in datasets(kind):
                    case = st.Case(kind, pat, fmt, beta, fma, ld, batch, extra, shared)
                    vals, x, c = case.uniform()
                    a, b, cf = host_operands(case, vals, x, c)
                    blocks = (batch * case.lanes() + 255) // 256
                    head = np.array([len(table) - 1, a.size, b.size, cf.size, case.stride_dense(), case.c_layout().stride, batch, blocks], dtype=np.int64)
                    payload += [head.tobytes(), a.tobytes(), b.tobytes(), cf.tobytes()]
                    records.append((case, vals, x, c, cf.size))
    src = d / "host.cpp"
    src.write_text(HARNESS_HEAD + "".join(units) + "struct entry { int typesize; void* fn; };\nstatic const entry table[] = {\n" + ",\n".join(table) + "\n};\n" + HARNESS_TAIL)
    (d / "in.bin").write_bytes(b"".join(payload))
    base = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-w", str(src), "-o", str(d / "host")]
    # the sanitizers are given up only where an empty program does not build and run with them (no runtime on this machine): then
    # the out-of-extent check is lost, and a warning in the run's summary says so. Any other failure of the build is a failure.
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    sanitized = (0 == subprocess.run(["g++", str(probe), "-o", str(d / "probe")] + SANITIZE, capture_output=True).returncode
                 and 0 == subprocess.run([str(d / "probe")], capture_output=True).returncode)
    if not sanitized:
        warnings.warn("no sanitizer runtime here: the generated text ran on the host WITHOUT the address / undefined-behaviour checks")
    res = subprocess.run(base + (SANITIZE if sanitized else []), capture_output=True, text=True)
    assert 0 == res.returncode, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the leak check needs ptrace, which a container may not grant)
    res = subprocess.run([str(d / "host"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, env=env)
    assert 0 == res.returncode and ("%d records" % len(records)) in res.stdout, (res.returncode, res.stdout[-500:], res.stderr[-3000:])
    out = (d / "out.bin").read_bytes()
    results, at = [], 0
    for case, vals, x, c, n in records:
        results.append((case, vals, x, c, np.frombuffer(out, dtype=case.dtype, count=n, offset=at).copy()))
        at += n * case.dtype().itemsize
    assert at == len(out)
    print("[sparse text on the host] %d kernels, %d records, sanitizers %s" % (len(table), len(records), "on" if sanitized else "NOT AVAILABLE"))
    return results, sanitized


@pytest.mark.parametrize("kind", TEXT_KINDS)
def test_generated_text_on_the_host(orc, host_run, kind):
    results, sanitized = host_run
    mine = [r for r in results if r[0].kind == kind]
    assert len(mine) == len(st.pattern_runs(kind)) * 2 * 3
    assert {(r[0].pattern, r[0].fma) for r in mine} == {(p, a) for p in st.patterns_of(kind) for a in (1, 0)}
    for case, vals, x, c, got in mine:
        if kind in st.PLAIN or case.fma:
            ref = st.reference1(orc, case, vals, x, c)
        else:  # (the oracle's SOA functions are fma: the same chain through its plain function, multiply-then-add)
            ref = st.canonical(orc, case, vals, x, c, arith=orc.MULADD)
        want = expected_flat(case, ref, 0, case.dtype(np.nan))[:got.size]
        assert ho.same_values(got, want), (case.id(),) + ho.differences(got, want)


def test_soa_a_sparse_refuses_entries_beyond_the_operator(xs):
    """P6 (entries at and beyond k): the plain kinds drop them, SOA A sparse has no cut -- its statements are unconditional -- and
    refuses the pattern (soa_pattern_ok)"""
    for fmt in ("f32", "f64"):
        proto = st.Case("soa_asparse", "P1", fmt, 1)
        ptr, idx, _ = st.p6(proto.M, proto.K, 1)
        assert st.text_of(xs, "soa_asparse", fmt, 1, 1, proto.descriptor_args(), ptr, idx) == (None, -1)
        assert st.soa_body(xs, "soa_asparse", fmt, 1, proto.descriptor_args(), ptr, idx) == (None, 90010)
        text, err = st.text_of(xs, "soa_asparse", fmt, 1, 1, proto.descriptor_args(), proto.ptr, proto.idx)
        assert text is not None and text.count("= XACC(") == len(proto.idx)


def test_soa_translation_unit_holds_the_body_of_the_text_entry_points(xs):
    """libxsmm_amd_soa_source (what the host run compiles, and what libxsmm_create_x*_soa builds) is the prologue, the signature and
    exactly the statements that libxsmm_generator_spgemm_{csr,csc}_soa_kernel append; its two arithmetics differ in XACC alone"""
    for kind in st.SOA:
        for (pat, fmt, beta, _, ld) in st.pattern_runs(kind):
            proto = st.Case(kind, pat, fmt, beta, 1, ld)
            body, err = st.soa_body(xs, kind, fmt, beta, proto.descriptor_args(), proto.ptr, proto.idx)
            assert body is not None, (proto.id(), err)
            units = [st.text_of(xs, kind, fmt, beta, fma, proto.descriptor_args(), proto.ptr, proto.idx)[0] for fma in (1, 0)]
            for fma, unit in zip((1, 0), units):
                head, rest = unit.split("{\n", 1)
                assert rest == body + "}\n", proto.id()
                assert ("__builtin_fma" in head) == bool(fma) and ("((c) + (a) * (b))" in head) == (not fma) and 'void xsmm_spgemm_op(' in head


# ---- 4. offsets past 2^31 in the text ----------------------------------------------------------------------------------------------------------
W30, W26, INT_MAX = 1 << 30, 1 << 26, (1 << 31) - 1


def dense_pattern(majors, minors):
    return st.p3(majors, minors, 3)[:2]


def literals(text, pattern, span):
    """the values of every match of `pattern` (one group for the digits, one for the suffix). span: the largest lane the text adds to
    such a literal in an int (0: none). The literal is LL exactly where literal + span passes INT_MAX -- the sum is then 64-bit as a
    whole; anywhere else the text is as ever"""
    found = [(int(v), s == "LL") for v, s in re.findall(pattern, text)]
    assert found, pattern
    for v, wide in found:
        assert v >= 0, (pattern, v)
        assert wide == (v + span > INT_MAX), (pattern, v, span, wide)
    return sorted(v for v, _ in found)


def every_index_expression_holds_its_sum_in_64_bits(text, m, n):
    """whatever the regular expression of a case looks at: no negative literal, no literal beyond int without LL, and wherever the
    text adds the int lane `n` (< n) or `m` (< m) to a literal, the literal is LL as soon as the sum can pass INT_MAX"""
    assert not re.search(r"[\[ (]-\d", text), "a negative literal"
    for v in re.findall(r"\b(\d{10,})\b(?!LL)", text):
        assert int(v) <= INT_MAX, v
    assert "const int n = xs_l;" in text or "const int m = xs_l;" in text or not re.search(r"\d(LL)? \+ [nm]\]", text)
    for v, suffix, lane in re.findall(r"\[(\d+)(LL)? \+ ([nm])\]", text):
        assert suffix == "LL" or int(v) + ((n if lane == "n" else m) - 1) <= INT_MAX, (v, lane)
    # every other sum or product with a lane has a 64-bit operand in front
    for expr in re.findall(r"\[([^\]]*xs_[lmv][^\]]*)\]", text) + re.findall(r"= [ABC] \+ ([^;]*);", text):
        for term in re.findall(r"((?:\(long long\))?\w+) \* \d+", expr):
            assert term.startswith("(long long)"), expr


WIDE_CASES = [
    # id, kind, format, beta, (m, n, k, lda, ldb, ldc), regular expression of the offsets, the products they have to be
    ("csr_asparse-ldb", "csr_asparse", "f32", 1, (2, 5, 3, 0, W30, 5), r"b\[(-?\d+)(LL)? \+ n\]", [k * W30 for k in range(3)]),
    ("csr_asparse-ldc", "csr_asparse", "f32", 1, (3, 5, 3, 0, 5, W30), r"c\[(-?\d+)(LL)? \+ n\]", sorted(2 * [m * W30 for m in range(3)])),
    ("csr_asparse-ldc-beta0", "csr_asparse", "f32", 0, (3, 5, 3, 0, 5, W30), r" c\[(-?\d+)(LL)? \+ n\] = acc", [m * W30 for m in range(3)]),
    ("csc_bsparse-lda", "csc_bsparse", "f64", 1, (2, 5, 3, W30, 0, 2), r"a\[(-?\d+)(LL)? \+ m\]", [k * W30 for k in range(3)]),
    ("csc_bsparse-ldc", "csc_bsparse", "f64", 0, (2, 3, 3, 2, 0, W30), r" c\[(-?\d+)(LL)? \+ m\] = acc", [n * W30 for n in range(3)]),
    ("csc_asparse-ldb-ldc", "csc_asparse", "f32", 1, (2, 3, 3, 0, W30, W30), r"\(long long\)xs_l \* (-?\d+)(LL)?;", [W30, W30]),
    ("soa_asparse-ldb", "soa_asparse", "f32", 1, (2, 5, 3, 0, W26, 5), r" b\[(-?\d+)(LL)?\];", [k * W26 * 16 for k in range(3)]),
    ("soa_asparse-ldc", "soa_asparse", "f32", 0, (3, 5, 3, 0, 5, W26), r" c\[(-?\d+)(LL)?\] = acc", [m * W26 * 16 for m in range(3)]),
    ("soa_bsparse-lda", "soa_bcsr", "f32", 1, (3, 5, 3, W26, 0, 5), r"A \+ xs_item \* stride_dense \+ \(long long\)xs_m \* (-?\d+)(LL)? \+ xs_v", [W26 * 16]),
    ("soa_bsparse-lda-2^28", "soa_bcsc", "f32", 1, (3, 5, 3, 1 << 28, 0, 5), r"A \+ xs_item \* stride_dense \+ \(long long\)xs_m \* (-?\d+)(LL)? \+ xs_v", [1 << 32]),
    ("soa_bsparse-ldc-2^28", "soa_bcsc", "f64", 1, (3, 5, 3, 3, 0, 1 << 29), r"C \+ xs_item \* stride_c \+ \(long long\)xs_m \* (-?\d+)(LL)? \+ xs_v", [1 << 32]),
    # a row that begins within an item's lanes of 2^31: the literal fits an int, literal + lane does not (2^30 - 1: the third row at
    # 2^31 - 2; 2^31 - 1: the second row at INT_MAX)
    ("csr_asparse-ldb-below", "csr_asparse", "f32", 1, (2, 5, 3, 0, W30 - 1, 5), r"b\[(-?\d+)(LL)? \+ n\]", [k * (W30 - 1) for k in range(3)]),
    ("csr_asparse-ldb-intmax", "csr_asparse", "f32", 1, (2, 5, 3, 0, INT_MAX, 5), r"b\[(-?\d+)(LL)? \+ n\]", [k * INT_MAX for k in range(3)]),
    ("csr_asparse-ldc-below", "csr_asparse", "f32", 1, (3, 5, 3, 0, 5, W30 - 1), r"c\[(-?\d+)(LL)? \+ n\]", sorted(2 * [m * (W30 - 1) for m in range(3)])),
    ("csr_asparse-ldc-intmax-beta0", "csr_asparse", "f32", 0, (3, 5, 3, 0, 5, INT_MAX), r" c\[(-?\d+)(LL)? \+ n\] = acc", [m * INT_MAX for m in range(3)]),
    ("csc_bsparse-lda-below", "csc_bsparse", "f64", 1, (2, 5, 3, W30 - 1, 0, 2), r"a\[(-?\d+)(LL)? \+ m\]", [k * (W30 - 1) for k in range(3)]),
    ("csc_bsparse-lda-intmax", "csc_bsparse", "f64", 1, (2, 5, 3, INT_MAX, 0, 2), r"a\[(-?\d+)(LL)? \+ m\]", [k * INT_MAX for k in range(3)]),
    ("csc_bsparse-ldc-below", "csc_bsparse", "f64", 0, (2, 3, 3, 2, 0, W30 - 1), r" c\[(-?\d+)(LL)? \+ m\] = acc", [n * (W30 - 1) for n in range(3)]),
    ("csc_bsparse-ldc-intmax", "csc_bsparse", "f64", 1, (2, 3, 3, 2, 0, INT_MAX), r"c\[(-?\d+)(LL)? \+ m\]", sorted(2 * [n * INT_MAX for n in range(3)])),
    ("csc_asparse-intmax", "csc_asparse", "f32", 1, (2, 3, 3, 0, INT_MAX, INT_MAX), r"\(long long\)xs_l \* (-?\d+)(LL)?;", [INT_MAX, INT_MAX]),
    ("soa_asparse-ldb-below", "soa_asparse", "f32", 1, (2, 5, 3, 0, W26 - 1, 5), r" b\[(-?\d+)(LL)?\];", [k * (W26 - 1) * 16 for k in range(3)]),
]


@pytest.mark.parametrize("wide", WIDE_CASES, ids=[w[0] for w in WIDE_CASES])
def test_offsets_past_2_31_in_the_text(xs, wide):
    name, kind, fmt, beta, dims, pattern, want = wide
    m, n, k = dims[:3]
    lines = m if kind in ("csr_asparse", "csc_asparse", "soa_asparse") else n
    ptr, idx = dense_pattern(*((lines, k) if kind in st.BY_LINE else (k, lines)))
    for fma in (1, 0):
        text, err = st.text_of(xs, kind, fmt, beta, fma, dims, ptr, idx)
        assert text is not None, err
        span = {"csr_asparse": n - 1, "csc_bsparse": m - 1}.get(kind, 0)   # (the other kinds add no int lane to a literal)
        assert literals(text, pattern, span) == want, name
        every_index_expression_holds_its_sum_in_64_bits(text, m, n)
        assert text.count("= XACC(") == m * n * k // (n if kind in ("csr_asparse", "csc_asparse", "soa_asparse") else m)
    # (the case is at the boundary: an offset beyond int or within an item's lanes of it; csc_asparse and SOA B sparse multiply a
    # literal that fits by a 64-bit index, which is pinned)
    assert max(want) > INT_MAX - 128 or kind in ("csc_asparse", "soa_bcsr")


def test_the_clear_loop_indexes_in_64_bits(xs):
    """csr_asparse under beta = 0 with ldc > n: the padding lanes clear c[m * ldc + n] for every row -- m * ldc in 64 bits"""
    ptr, idx = dense_pattern(3, 3)
    for ldc in (8, W30):
        text, err = st.text_of(xs, "csr_asparse", "f32", 0, 1, (3, 5, 3, 0, 5, ldc), ptr, idx)
        assert text is not None, err
        loop = re.findall(r"for \(int m = 0; m < 3; \+\+m\) c\[(.*?)\] = \(T\)0;", text)
        assert loop == ["(long long)m * %d + n" % ldc], loop
        assert ("xs_gid / %d;" % ldc) in text   # ldc lanes per item


def test_text_of_ordinary_leading_dimensions_has_plain_literals(xs):
    """no LL suffix and no cast appears where every offset fits an int: the text (and so the arithmetic) of the fixtures is unchanged"""
    for kind in TEXT_KINDS:
        for (pat, fmt, beta, fma, ld) in st.pattern_runs(kind):
            proto = st.Case(kind, pat, fmt, beta, fma, ld)
            text, err = st.text_of(xs, kind, fmt, beta, fma, proto.descriptor_args(), proto.ptr, proto.idx)
            body = text.split("{\n", 1)[1]
            assert not re.search(r"\dLL", body), proto.id()


def test_dimensions_the_index_arithmetic_cannot_hold_are_refused(xs):
    """a descriptor holds no extent beyond int, but an SOA lane count is n * 16: beyond int from n = 2^27 on, and then there is no
    kernel (the lane index is an int); just below there is"""
    ptr, idx = dense_pattern(2, 3)
    for n, expect in (((1 << 27) - 1, 0), (1 << 27, 90010)):
        text, err = st.text_of(xs, "soa_asparse", "f32", 1, 1, (2, n, 3, 0, n, n), ptr, idx)
        assert (text is None) == (0 != expect)
        assert st.soa_body(xs, "soa_asparse", "f32", 1, (2, n, 3, 0, n, n), ptr, idx)[1] == expect
    assert ("xs_gid / %d;" % (((1 << 27) - 1) * 16)) in st.text_of(xs, "soa_asparse", "f32", 1, 1, (2, (1 << 27) - 1, 3, 0, (1 << 27) - 1, (1 << 27) - 1), ptr, idx)[0]
