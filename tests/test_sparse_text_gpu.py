"""The kernels generated per sparsity pattern on the GPU -- spgemm_{csr_asparse,csc_bsparse,csc_asparse}_text, soa_{asparse,bsparse,
rm_ac,rm_bc}_text and the csr_reg kernels of libxsmm_create_{d,s}csr_reg -- on the seeded cases of tests/sparse_text_cases.py:
patterns with empty lines, cut, duplicate and unsorted entries and none at all; lane counts that divide no work-group; operands
whose guard bands, leading-dimension gaps and inter-item spaces hold NaN and +Inf; values at the edges of the number line; items
that straddle work-groups; leading dimensions at which an element offset passes 2^31; and a text kernel between two recorded dense
calls of a libxsmm_amd_defer_begin/end bracket.

Every result is compared with Reference 1 (the oracle's statement-order functions on the logical operands alone) bit for bit -- with
hostile data through hostile_operands.same_values: NaN where the reference has NaN, its bits elsewhere -- and, on uniform data, held
within the derived bound of Reference 2. tests/test_sparse_text_cpu.py checks the cases, the references and the generated text
itself without a GPU."""
import ctypes as C
import threading

import numpy as np
import pytest

import hostile_operands as ho
import sparse_text_cases as st
from test_wide_offsets_gpu import need

pytestmark = pytest.mark.gpu

CALL = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)


class Built(object):
    """the kernel of a case (batch size, strides and data aside): created once, run many times"""

    def __init__(self, xs, case, vals=None):
        self.xs, self.L, self.case, self.kind = xs, xs.lib(), case, case.kind
        self.blob, d = st.descriptor(xs, case.fmt, *case.descriptor_args(), beta=case.beta)
        L, kind = self.L, case.kind
        self.h = self.fn = None
        if kind in st.PLAIN:
            is_csr, ri, ci = st.pattern_arguments(kind, case.ptr, case.idx)
            self.h = L.libxsmm_amd_spgemm_create(d, is_csr, xs.dptr(ri), xs.dptr(ci), case.fma)
        elif kind in st.RM:
            self.fn = getattr(L, "libxsmm_create_%s_soa" % kind)(d)
        elif kind == "csr_reg":  # the values are the kernel's
            self.fn = getattr(L, "libxsmm_create_%scsr_reg" % ("d" if case.fmt == "f64" else "s"))(d, xs.dptr(case.ptr), xs.dptr(case.idx), xs.dptr(np.ascontiguousarray(vals)))
        else:
            create = L.libxsmm_create_xcsc_soa if kind == "soa_bcsc" else L.libxsmm_create_xcsr_soa
            self.fn = create(d, xs.dptr(case.ptr), xs.dptr(case.idx), xs.dptr(np.ones(max(1, case.nnz), case.dtype)))

    def ok(self):
        return bool(self.h or self.fn)

    def kernel_name(self):
        name = st.KERNEL[self.kind]
        return name % (64 if self.case.fmt == "f64" else 32) if "%" in name else name

    def order(self, shared, dense):
        return (shared, dense) if self.kind in st.A_SHARED else (dense, shared)

    def batch(self, shared, dense, c, stride_dense, stride_c, batch):
        """the batch entry; operands: anything xs.dptr takes"""
        xs = self.xs
        if self.kind in st.PLAIN:
            return self.L.libxsmm_amd_spgemm_execute_batch(self.h, xs.dptr(shared), xs.dptr(dense), xs.dptr(c), stride_dense, stride_c, batch)
        if self.kind == "csr_reg":
            assert batch == 1
            xs.call_kernel(self.fn, None, dense, c)
            return 0
        a, b = self.order(shared, dense)
        return self.L.libxsmm_amd_kernel_execute_batch(self.fn, xs.dptr(a), xs.dptr(b), xs.dptr(c), stride_dense, stride_c, batch)

    def single(self, shared, dense, c):
        """one product the other way: the plain kinds' batch entry on host operands, the bare pointer of the others"""
        if self.kind in st.PLAIN or self.kind == "csr_reg":
            return self.batch(shared, dense, c, 0, 0, 1)
        a, b = self.order(shared, dense)
        CALL(self.fn)(self.xs.dptr(a), self.xs.dptr(b), self.xs.dptr(c))
        return 0

    def close(self):
        if self.h:
            self.L.libxsmm_amd_spgemm_destroy(self.h)
        if self.fn:
            self.L.libxsmm_release_kernel(self.fn)
        self.h = self.fn = None


def run(torch, xs, built, case, vals, x, c, fill):
    """the batch entry on device operands with `fill` around and between the matrices -> the flat arrays afterwards, and before"""
    itemsize = case.dtype().itemsize
    fs, fd, fc = case.flat_shared(vals, fill), case.flat_dense(x, fill), case.flat_c(c, fill)
    ds, dd, dc = (torch.from_numpy(f).cuda() for f in (fs, fd, fc))
    g = ho.GUARD * itemsize
    rc = built.batch(ds.data_ptr() + g, dd.data_ptr() + g, dc.data_ptr() + g, case.stride_dense(), case.c_layout().stride, case.batch)
    torch.cuda.synchronize()
    assert rc == 0, case.id()
    assert xs.last_kernel() == built.kernel_name(), (case.id(), xs.last_kernel())
    return (ds.cpu().numpy(), dd.cpu().numpy(), dc.cpu().numpy()), (fs, fd, fc)


def expected_flat(case, ref, fill):
    flat = case.flat_c(ref, fill)
    flat[case.owned_gap()] = 0
    return flat


def check(case, after, before, ref, fill, what=""):
    """C: the reference's values in the matrices, in the gaps only what the kernel owns; the inputs keep their bytes"""
    (gs, gd, gc), (fs, fd, fc) = after, before
    want = expected_flat(case, ref, fill)
    got = case.peel_c(gc)
    assert ho.same_values(got, ref), (case.id(), what) + ho.differences(got, ref)
    assert np.array_equal(ho.gaps(gc, case.c_layout()), ho.gaps(want, case.c_layout())), (case.id(), what, "gaps of C")
    assert np.array_equal(ho.raw(gs), ho.raw(fs)) and np.array_equal(ho.raw(gd), ho.raw(fd)), (case.id(), what, "inputs")


def reference(orc, case, vals, x, c):
    with np.errstate(all="ignore"):
        return st.reference1(orc, case, vals, x, c)


# ---- patterns -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.KINDS)
def test_patterns(xs, orc, torch_gpu, kind):
    """every pattern of the kind twice, format, beta and flavour in rotation; the batch entry at both batch sizes, and once the bare
    pointer or host operands. Bit-equal to Reference 1, within the derived bound of Reference 2."""
    torch = torch_gpu
    ho.assert_environment(orc)
    for (pat, fmt, beta, fma, ld) in st.pattern_runs(kind):
        proto = st.Case(kind, pat, fmt, beta, fma, ld)
        fill = ho.fills(fmt)[0]
        built = Built(xs, proto, proto.uniform()[0])
        assert built.ok(), proto.id()
        try:
            for batch in st.batches(kind):
                case = st.Case(kind, pat, fmt, beta, fma, ld, batch or 1, 4)
                vals, x, c = case.uniform()
                ref = reference(orc, case, vals, x, c)
                after, before = run(torch, xs, built, case, vals, x, c, fill)
                check(case, after, before, ref, fill)
                value, bound = st.reference2(case, vals, x, c)
                excess = np.abs(case.peel_c(after[2]).astype(np.longdouble) - value) - bound
                assert np.all(excess <= 0), (case.id(), float(excess.max()))
            # one product on host operands (staged), tight in their extents: the bare pointer where the kind has one
            case = st.Case(kind, pat, fmt, beta, fma, ld, 1, 1)
            vals, x, c = case.uniform()
            ref = reference(orc, case, vals, x, c)
            hs = np.ascontiguousarray(case.flat_shared(vals, fill, guard=0)) if case.nnz else np.zeros(1, case.dtype)  # (P7: no values, a pointer still)
            hd = np.ascontiguousarray(case.flat_dense(x, fill, guard=0))
            hc = np.ascontiguousarray(case.flat_c(c, fill, guard=0))
            assert 0 == built.single(hs, hd, hc)
            assert xs.last_kernel() == built.kernel_name()
            want = case.flat_c(ref, fill, guard=0)
            want[case.owned_gap(0)] = 0
            assert ho.same_values(hc, want), (case.id(), "host") + ho.differences(hc, want)
        finally:
            built.close()


def test_soa_a_sparse_has_no_kernel_for_entries_beyond_the_operator(xs, torch_gpu):
    """P6: the plain kinds drop such entries (test_patterns), SOA A sparse refuses the pattern"""
    for fmt in ("f32", "f64"):
        proto = st.Case("soa_asparse", "P1", fmt, 1)
        ptr, idx, _ = st.p6(proto.M, proto.K, 1)
        blob, d = st.descriptor(xs, fmt, *proto.descriptor_args(), beta=1)
        assert not xs.lib().libxsmm_create_xcsr_soa(d, xs.dptr(ptr), xs.dptr(idx), xs.dptr(np.ones(len(idx), proto.dtype)))


@pytest.mark.parametrize("kind", st.PLAIN)
def test_operator_without_entries_on_host_memory(xs, orc, torch_gpu, kind):
    """P7 with host operands on a thread that never staged anything: its scratch slot for the values is empty, and there is nothing
    to stage. beta = 0 clears C, beta = 1 leaves it."""
    torch_gpu.cuda.synchronize()
    out = {}

    def body():
        try:
            for beta in (0, 1):
                case = st.Case(kind, "P7", "f64", beta, 1, "gap", 3, 1)
                vals, x, c = case.uniform()
                built = Built(xs, case)
                assert built.ok()
                try:
                    hd, hc = case.flat_dense(x, np.float64(7), guard=0), case.flat_c(c, np.float64(7), guard=0)
                    rc = built.batch(np.zeros(1), hd, hc, case.stride_dense(), case.c_layout(0).stride, case.batch)
                    want = case.flat_c(reference(orc, case, vals, x, c), np.float64(7), guard=0)
                    want[case.owned_gap(0)] = 0
                    out[beta] = (rc, xs.last_kernel(), np.array_equal(ho.raw(hc), ho.raw(want)))
                finally:
                    built.close()
        except Exception as e:  # (an assertion in a thread is lost otherwise)
            out["error"] = repr(e)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    assert out == {0: (0, st.KERNEL[kind], True), 1: (0, st.KERNEL[kind], True)}, out


# ---- hostile gaps and values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.KINDS)
def test_gaps(xs, orc, torch_gpu, kind):
    """guard bands, leading-dimension gaps and the space between items hold NaN, then +Inf: the same bytes both times, Reference 1
    on the logical operands alone; of C's gaps only what the kernel owns changes; the inputs stay"""
    torch = torch_gpu
    ho.assert_environment(orc)
    for (pat, fmt, beta, fma) in st.hostile_runs(kind):
        case = st.hostile_case(kind, pat, fmt, beta, fma)
        vals, x, c = case.uniform()
        ref = reference(orc, case, vals, x, c)
        built = Built(xs, case, vals)
        assert built.ok(), case.id()
        try:
            results = []
            for fill in ho.fills(fmt):
                after, before = run(torch, xs, built, case, vals, x, c, fill)
                check(case, after, before, ref, fill, "fill %r" % fill)
                results.append(case.peel_c(after[2]))
            assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), case.id()
            assert np.array_equal(ho.raw(results[0]), ho.raw(ref)), case.id()
        finally:
            built.close()


@pytest.mark.parametrize("gen", ho.KINDS)
@pytest.mark.parametrize("kind", st.KINDS)
def test_values(xs, orc, torch_gpu, kind, gen):
    torch = torch_gpu
    ho.assert_environment(orc)
    for (pat, fmt, beta, fma) in st.hostile_runs(kind):
        case = st.hostile_case(kind, pat, fmt, beta, fma)
        vals, x, c = case.hostile(gen)
        ref = reference(orc, case, vals, x, c)
        ho.conditions(gen, ref, beta)
        built = Built(xs, case, vals)
        assert built.ok(), case.id()
        try:
            fill = ho.fills(fmt)[0]
            after, before = run(torch, xs, built, case, vals, x, c, fill)
            check(case, after, before, ref, fill, gen)
        finally:
            built.close()


# ---- items that straddle work-groups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.PLAIN + st.SOA + st.RM)
def test_items_straddle_work_groups(xs, orc, torch_gpu, kind):
    """lane counts of 5, 7, 6 (ldc lanes), 24, 40, 48 and 80 divide no work-group of 256: at batch 103 (plain; three work-groups) and 7
    (SOA) items lie across the borders. Item strides of extent + 1, and stride_dense = 0: one dense operand for all items."""
    torch = torch_gpu
    pat = None if kind in st.RM else "P1"
    lanes = set()
    for (fmt, beta, fma) in st.combos(kind)[:4]:
        proto = st.Case(kind, pat, fmt, beta, fma)
        built = Built(xs, proto)
        assert built.ok()
        fill = ho.fills(fmt)[0]
        try:
            for shared in (False, True):
                case = st.Case(kind, pat, fmt, beta, fma, "gap", st.batches(kind)[0], 1, shared)
                assert 256 % case.lanes() != 0 and (case.stride_dense() == 0) == shared
                assert kind not in st.PLAIN or (case.batch * case.lanes() + 255) // 256 == 3
                lanes.add(case.lanes())
                vals, x, c = case.uniform()
                after, before = run(torch, xs, built, case, vals, x, c, fill)
                check(case, after, before, reference(orc, case, vals, x, c), fill, "shared" if shared else "strided")
        finally:
            built.close()
    print("[straddle]", kind, "lanes", sorted(lanes))


# ---- leading dimensions past 2^31 elements --------------------------------------------------------------------------------------------------
WIDE = [("csr_asparse-ldb", "csr_asparse", (2, 5, 3, 0, 1 << 30, 5)), ("csr_asparse-ldc", "csr_asparse", (3, 5, 3, 0, 5, 1 << 30)),
        ("soa_asparse-ldb", "soa_asparse", (2, 5, 3, 0, 1 << 26, 5)),
        # the third row of B begins two elements below 2^31: the literal fits an int, literal + lane does not
        ("csr_asparse-ldb-below", "csr_asparse", (2, 5, 3, 0, (1 << 30) - 1, 5))]


@pytest.mark.parametrize("wide", WIDE, ids=[w[0] for w in WIDE])
def test_leading_dimension_past_2_31_elements(xs, orc, torch_gpu, wide):
    """fp32, one item, beta = 1, a dense operator: the third row of B (or of C) starts at element 2^31, or two below. The operand is one allocation of
    about 8 GiB, of which only the rows the kernel touches are written and compared -- against the oracle on tight copies (the leading
    dimension only places the rows). (beta = 0 at a wide ldc would clear 2^30 lanes of padding: tests/test_sparse_text_cpu.py holds
    its text.)"""
    torch = torch_gpu
    name, kind, (m, n, k, lda, ldb, ldc) = wide
    v = 16 if kind == "soa_asparse" else 1
    ptr, idx, vals = st.p3(m, k, 11)
    vals = vals.astype(np.float32)
    rng = np.random.default_rng(ho.seed_of("wide", name))
    b, c = rng.uniform(-1, 1, (k, n * v)).astype(np.float32), rng.uniform(-1, 1, (m, n * v)).astype(np.float32)
    ref = c.copy()
    if kind == "csr_asparse":
        orc.csr_asparse(orc.FMA, 0, m, n, k, n, n, ptr, idx, vals, b.ravel(), ref.reshape(-1))
    else:
        orc.soa_csr_asparse(0, m, n, k, n, n, v, ptr, idx, vals, b.ravel(), ref.reshape(-1))
    nb, nc = ((k - 1) * ldb + n) * v, ((m - 1) * ldc + n) * v
    assert max(nb, nc) > (1 << 31) and max((k - 1) * ldb, (m - 1) * ldc) * v in ((1 << 31), (1 << 31) - 2)
    need(torch, 4 * (nb + nc))
    db, dc = torch.empty(nb, dtype=torch.float32, device="cuda"), torch.empty(nc, dtype=torch.float32, device="cuda")
    rows_b = torch.as_strided(db, (k, n * v), (ldb * v, 1))
    rows_c = torch.as_strided(dc, (m, n * v), (ldc * v, 1))
    rows_b.copy_(torch.from_numpy(b))
    rows_c.copy_(torch.from_numpy(c))
    dv = torch.from_numpy(vals).cuda()
    blob, d = st.descriptor(xs, "f32", m, n, k, lda, ldb, ldc, beta=1)
    L = xs.lib()
    if kind == "csr_asparse":
        h = L.libxsmm_amd_spgemm_create(d, 1, xs.dptr(ptr), xs.dptr(idx), 1)
        assert h
        try:
            assert 0 == L.libxsmm_amd_spgemm_execute_batch(h, xs.dptr(dv), xs.dptr(db), xs.dptr(dc), 0, 0, 1)
            torch.cuda.synchronize()
        finally:
            L.libxsmm_amd_spgemm_destroy(h)
    else:
        fn = L.libxsmm_create_xcsr_soa(d, xs.dptr(ptr), xs.dptr(idx), xs.dptr(vals))
        assert fn
        try:
            assert 0 == L.libxsmm_amd_kernel_execute_batch(fn, xs.dptr(dv), xs.dptr(db), xs.dptr(dc), 0, 0, 1)
            torch.cuda.synchronize()
        finally:
            L.libxsmm_release_kernel(fn)
    assert xs.last_kernel() == st.KERNEL[kind]
    got = rows_c.cpu().numpy()
    assert np.array_equal(ho.raw(got), ho.raw(ref)), np.argwhere(got != ref)[:4]
    assert np.array_equal(rows_b.cpu().numpy(), b)


# ---- a text kernel between recorded calls -------------------------------------------------------------------------------------------------
def test_text_kernel_inside_a_bracket(xs, orc, torch_gpu):
    """inside libxsmm_amd_defer_begin/end: (1) a dispatched dense 32^3 kernel, recorded into a burst, adds p * q to X; (2) an SOA
    kernel called through its pointer reads X as its dense operand B[8][8][16] and writes C[8][8][16]; (3) the dense kernel reads C.
    Asking for the stream launches what is open (xsmm_device.cpp: device()), so (2) sees what (1) wrote. The bits of the same calls
    outside the bracket, and of the oracle (vector-ALU dense kernel: the fma chain)."""
    torch, L = torch_gpu, xs.lib()
    rng = np.random.default_rng(ho.seed_of("bracket"))
    f32 = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    p, q, x0, c0, z0 = f32(1024), f32(1024), f32(1024), f32(1024), f32(1024)
    m = n = k = 8
    ptr, idx, vals = st.p1(m, k, 5)
    vals = vals.astype(np.float32)
    # the oracle: X = x0 + p q; C = c0 + S X (SOA); Z = z0 + C q
    X = x0.copy(); orc.smm(orc.FMA, 0, 32, 32, 32, 32, 32, 32, p, q, X)
    Cc = c0.copy(); orc.soa_csr_asparse(0, m, n, k, n, n, 16, ptr, idx, vals, X, Cc)
    Z = z0.copy(); orc.smm(orc.FMA, 0, 32, 32, 32, 32, 32, 32, Cc, q, Z)
    old_mfma = L.libxsmm_amd_set_mfma(0)
    try:
        dense = L.libxsmm_smmdispatch(32, 32, 32, None, None, None, None, None, None, None)
        blob, d = st.descriptor(xs, "f32", m, n, k, 0, n, n, beta=1)
        soa = L.libxsmm_create_xcsr_soa(d, xs.dptr(ptr), xs.dptr(idx), xs.dptr(vals))
        assert dense and soa

        def sequence(bracket):
            dp, dq, dx, dc, dz, dv = (torch.from_numpy(t.copy()).cuda() for t in (p, q, x0, c0, z0, vals))
            torch.cuda.synchronize()
            names = []
            if bracket:
                L.libxsmm_amd_defer_begin()
            xs.call_kernel(dense, dp, dq, dx)
            CALL(soa)(xs.dptr(dv), xs.dptr(dx), xs.dptr(dc))
            names.append(xs.last_kernel())
            xs.call_kernel(dense, dc, dq, dz)
            if bracket:
                L.libxsmm_amd_defer_end()
            torch.cuda.synchronize()
            names.append(xs.last_kernel())
            return [t.cpu().numpy() for t in (dx, dc, dz)], names

        try:
            plain, names_plain = sequence(False)
            deferred, names = sequence(True)
        finally:
            L.libxsmm_release_kernel(soa)
    finally:
        L.libxsmm_amd_set_mfma(old_mfma)
    # (outside the bracket the dense call is a launch of its own; inside, the recorded calls run as one launch at defer_end)
    assert names_plain[0] == "soa_asparse_text" and names_plain[1].startswith("smm_f32"), names_plain
    assert names == ["soa_asparse_text", "smm_deferred_calls"], names
    for what, u, w, gold in zip(("X", "C", "Z"), plain, deferred, (X, Cc, Z)):
        assert np.array_equal(ho.raw(u), ho.raw(w)), what
        assert np.array_equal(ho.raw(w), ho.raw(gold)), what
