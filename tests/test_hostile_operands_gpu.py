"""Every arithmetic kernel on poisoned gaps and on values at the edges of the number line (helpers: tests/hostile_operands.py).

Part A (test_gaps_*): the operands lie in arrays whose every other element -- guard bands, leading-dimension gaps, the space
between batch items -- is NaN in one run and +Inf in the next (i16: the two ends of the range). Both runs must give the same
bytes, equal to the reference computed from the logical matrices alone; the gaps and guard bands of C keep their bytes; A
and B come back unchanged. A kernel that multiplies a neighbour's element by a padded zero passes with finite gaps and fails
here.

Part B (test_values_*): the generators underflow, overflow and specials against the family's reference with
hostile_operands.same_values: NaN where the reference has NaN, the reference's bits everywhere else (signed zeros, subnormals,
Inf). The conditions on the inputs (hostile_operands.conditions) are asserted first, so no case compares nothing.

Every case asserts the kernel it is meant for (libxsmm_amd_last_kernel)."""
import ctypes as C
import os

import numpy as np
import pytest

import fc_common as fc
import hostile_operands as ho
import lowp_gemm_common as lg
from test_tgemm_gpu import Case as TgemmCase

pytestmark = pytest.mark.gpu


class Settings(object):
    """environment and matrix-core switch of one call, restored afterwards"""

    def __init__(self, xs, mfma, env):
        self.xs, self.mfma, self.env = xs, mfma, env

    def __enter__(self):
        self.old_env = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        self.old = self.xs.lib().libxsmm_amd_set_mfma(self.mfma)

    def __exit__(self, *exc):
        self.xs.lib().libxsmm_amd_set_mfma(self.old)
        for k, v in self.old_env.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def kernel_matches(name, want):
    wants = want if isinstance(want, tuple) else (want,)
    return any(name.startswith(w) if w.endswith("_") else name == w for w in wants)


def upload(torch, flat):
    """-> device tensor of a flat numpy array (16-bit patterns travel as int16)"""
    return torch.from_numpy(flat.view(np.int16) if flat.dtype == np.uint16 else flat).cuda()


def download(t, like):
    out = t.cpu().numpy()
    return out.view(like.dtype) if out.dtype != like.dtype else out


def at(t, layout):
    """address of the first item of a device tensor laid out as `layout`: behind the guard band"""
    return t.data_ptr() + layout.guard * t.element_size()


def check_untouched(da, db, fa, fb):
    assert np.array_equal(ho.raw(download(da, fa)), ho.raw(fa)), "A was written"
    assert np.array_equal(ho.raw(download(db, fb)), ho.raw(fb)), "B was written"


# ---- dense SMM: generic, tuned, work-group and wave matrix-core forms, hiprtc-built kernels, batch-reduce ----------------------
def smm_layouts(case, extra):
    m, n, k = case.shape
    lda, ldb, ldc = case.lds()
    nc = int(case.owners().max()) + 1
    return (ho.Layout(m, k, case.batch, lda, extra), ho.Layout(n if case.transb else k, k if case.transb else n, case.batch, ldb, extra),
            ho.Layout(m, n, nc, ldc, extra))


def smm_run(xs, torch, case, fmt, beta, extra, a, b, c, fill):
    """-> (C as it comes back, C as it went in, its layout); asserts the kernel's name and that A and B are unchanged"""
    L = xs.lib()
    m, n, k = case.shape
    lda, ldb, ldc = case.lds()
    la, lb, lc = smm_layouts(case, extra)
    fa = ho.surround(a, la, fill)
    fb = ho.surround(np.ascontiguousarray(b.transpose(0, 2, 1)) if case.transb else b, lb, fill)
    fc = ho.surround(c, lc, fill)
    da, db, dc = (upload(torch, x) for x in (fa, fb, fc))
    prec = xs.F64 if fmt == "f64" else xs.F32
    ts = 8 if fmt == "f64" else 4
    own = case.owners()
    with Settings(xs, case.mfma, case.env):
        if case.mode == "strided":
            blob, desc = xs.descriptor(prec, m, n, k, lda, ldb, ldc, 1.0, float(beta), flags=xs.FLAG_TRANS_B if case.transb else 0)
            assert desc
            assert 0 == L.libxsmm_amd_gemm_batch_strided(desc, at(da, la), at(db, lb), at(dc, lc), la.stride, lb.stride, lc.stride, case.batch)
        elif case.mode == "reduce":
            ct = C.c_double if fmt == "f64" else C.c_float
            disp = L.libxsmm_dmmdispatch_reducebatch if fmt == "f64" else L.libxsmm_smmdispatch_reducebatch
            be = ct(beta)
            fn = disp(m, n, k, xs.iptr(lda), xs.iptr(ldb), xs.iptr(ldc), None, C.byref(be), None, None)
            assert fn
            pa = (da.data_ptr() + la.offsets() * ts).astype(np.uint64)
            pb = (db.data_ptr() + lb.offsets() * ts).astype(np.uint64)
            launches = L.libxsmm_amd_launch_count()
            xs.call_kernel(fn, pa, pb, at(dc, lc), np.array([case.batch], dtype=np.uint64))
            # beta = 0: the first product on its own, then the rest as one run (test_reduce_first_product pins the first one's kernel)
            assert L.libxsmm_amd_launch_count() - launches == (1 if beta else 2)
        else:
            sa, sb = la.offsets().astype(np.int32), lb.offsets().astype(np.int32)
            sc = lc.offsets()[own].astype(np.int32)
            xs.gemm_batch(prec, "N", "T" if case.transb else "N", m, n, k, 1.0, da, lda, db, ldb, float(beta), dc, ldc, 0, 4, sa, sb, sc,
                          -case.batch if case.distinct else case.batch)
        torch.cuda.synchronize()
        name = xs.last_kernel()
    print("kernel %-28s %s %s beta %d extra %d" % (name, case.id, fmt, beta, extra))
    assert kernel_matches(name, case.kernel[fmt]), (name, case.kernel[fmt])
    check_untouched(da, db, fa, fb)
    return download(dc, fc), fc, lc


SMM_VARIANTS = ho.smm_variants()
SMM_IDS = ["%s-%s-beta%d" % (c.id, f, be) for c, f, be in SMM_VARIANTS]


@pytest.mark.parametrize("variant", SMM_VARIANTS, ids=SMM_IDS)
def test_gaps_smm(xs, orc, torch_gpu, variant):
    case, fmt, beta = variant
    ho.assert_environment(orc)
    a, b, c = case.operands(None, fmt, beta)
    want = case.reference(orc, a, b, c, beta)
    for extra in case.extras:
        results = []
        for fill in ho.fills(fmt):
            got, before, lc = smm_run(xs, torch_gpu, case, fmt, beta, extra, a, b, c, fill)
            assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
            got = ho.peel(got, lc)
            assert ho.same_values(got, want), (case.id, fmt, beta, extra, float(fill), ho.differences(got, want))
            results.append(got)
        assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("variant", SMM_VARIANTS, ids=SMM_IDS)
def test_values_smm(xs, orc, torch_gpu, variant, kind):
    case, fmt, beta = variant
    ho.assert_environment(orc)
    a, b, c = case.operands(kind, fmt, beta)
    want = case.reference(orc, a, b, c, beta)
    ho.conditions(kind, want, beta)
    extra = case.extras[0]
    got, before, lc = smm_run(xs, torch_gpu, case, fmt, beta, extra, a, b, c, ho.fills(fmt)[0])
    assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
    got = ho.peel(got, lc)
    assert ho.same_values(got, want), (case.id, fmt, beta, kind, ho.differences(got, want))


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_reduce_first_product(xs, orc, torch_gpu, fmt):
    """a dispatched batch-reduce kernel with beta = 0 runs its first product alone (it overwrites C) and the rest as a run with
    beta = 1, whose name the reduce case of SMM_CASES asserts (smm_*_jit_shape_runs). Called with one product, the call is that
    first step alone: the batch engine takes beta = 0 items as independent overwrites, so it is the kernel for items that own
    their C, smm_*_jit_shape, and C = A_0 B_0 whatever C held (NaN here), between poisoned gaps."""
    ho.assert_environment(orc)
    torch, L = torch_gpu, xs.lib()
    case = [c for c in ho.SMM_CASES if c.mode == "reduce"][0]
    m, n, k = case.shape
    lda, ldb, ldc = case.lds()
    a, b, c = case.operands(None, fmt, 0)
    want = ho.chain(orc, a[:1], b[:1], c, 0)
    la, lb, lc = smm_layouts(case, 1)
    fill = ho.fills(fmt)[0]
    fa, fb, fc = ho.surround(a, la, fill), ho.surround(b, lb, fill), ho.surround(np.full_like(c, np.nan), lc, fill)
    da, db, dc = (upload(torch, x) for x in (fa, fb, fc))
    ts = 8 if fmt == "f64" else 4
    with Settings(xs, case.mfma, case.env):
        be = (C.c_double if fmt == "f64" else C.c_float)(0)
        fn = (L.libxsmm_dmmdispatch_reducebatch if fmt == "f64" else L.libxsmm_smmdispatch_reducebatch)(
            m, n, k, xs.iptr(lda), xs.iptr(ldb), xs.iptr(ldc), None, C.byref(be), None, None)
        assert fn
        pa = (da.data_ptr() + la.offsets() * ts).astype(np.uint64)
        pb = (db.data_ptr() + lb.offsets() * ts).astype(np.uint64)
        launches = L.libxsmm_amd_launch_count()
        xs.call_kernel(fn, pa, pb, at(dc, lc), np.array([1], dtype=np.uint64))
        torch.cuda.synchronize()
        name = xs.last_kernel()
        assert L.libxsmm_amd_launch_count() - launches == 1
    print("kernel %-28s first product of %s %s" % (name, case.id, fmt))
    assert name == "smm_f%d_jit_shape" % (64 if fmt == "f64" else 32), name
    check_untouched(da, db, fa, fb)
    got = download(dc, fc)
    assert np.array_equal(ho.gaps(got, lc), ho.gaps(fc, lc)), "the gaps of C changed"
    assert ho.same_values(ho.peel(got, lc), want), ho.differences(ho.peel(got, lc), want)


def grouped_run(xs, torch, fmt, ops, fill, extra=4):
    """the three groups of ho.GROUPED in one libxsmm_amd_gemm_batch_groups call -> per group (C back, C before, layout)"""
    prec = xs.F64 if fmt == "f64" else xs.F32
    dev, host = [], []
    for case, (a, b, c) in zip(ho.GROUPED, ops):
        la, lb, lc = smm_layouts(case, extra)
        fa = ho.surround(a, la, fill)
        fb = ho.surround(np.ascontiguousarray(b.transpose(0, 2, 1)) if case.transb else b, lb, fill)
        fc = ho.surround(c, lc, fill)
        host.append((fa, fb, fc, la, lb, lc))
        dev.append([upload(torch, x) for x in (fa, fb, fc)] +
                   [la.offsets().astype(np.int32), lb.offsets().astype(np.int32), lc.offsets()[case.owners()].astype(np.int32)])
    with Settings(xs, 0, {"LIBXSMM_AMD_JIT": "1", "LIBXSMM_AMD_JIT_MINBATCH": "1"}):
        rc = xs.gemm_batch_groups(prec, [c.shape for c in ho.GROUPED], [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev],
                                  [d[3] for d in dev], [d[4] for d in dev], [d[5] for d in dev], [c.batch for c in ho.GROUPED],
                                  transa=["N"] * 3, transb=["T" if c.transb else "N" for c in ho.GROUPED],
                                  lda=[c.lds()[0] for c in ho.GROUPED], ldb=[c.lds()[1] for c in ho.GROUPED], ldc=[c.lds()[2] for c in ho.GROUPED])
        assert rc == 0
        torch.cuda.synchronize()
        name = xs.last_kernel()
    print("kernel %-28s grouped %s" % (name, fmt))
    assert name == "smm_f%d_jit_shape_runs_grouped" % (64 if fmt == "f64" else 32), name
    out = []
    for d, (fa, fb, fc, la, lb, lc) in zip(dev, host):
        check_untouched(d[0], d[1], fa, fb)
        out.append((download(d[2], fc), fc, lc))
    return out


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_gaps_grouped_launch(xs, orc, torch_gpu, fmt):
    ho.assert_environment(orc)
    ops = [case.operands(None, fmt, 1) for case in ho.GROUPED]
    wants = [case.reference(orc, a, b, c, 1) for case, (a, b, c) in zip(ho.GROUPED, ops)]
    results = []
    for fill in ho.fills(fmt):
        outs = grouped_run(xs, torch_gpu, fmt, ops, fill)
        for case, (got, before, lc), want in zip(ho.GROUPED, outs, wants):
            assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), case.id
            assert ho.same_values(ho.peel(got, lc), want), (case.id, float(fill), ho.differences(ho.peel(got, lc), want))
        results.append([ho.peel(got, lc) for got, before, lc in outs])
    for r0, r1 in zip(*results):
        assert np.array_equal(ho.raw(r0), ho.raw(r1)), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_values_grouped_launch(xs, orc, torch_gpu, fmt, kind):
    ho.assert_environment(orc)
    ops = [case.operands(kind, fmt, 1) for case in ho.GROUPED]
    wants = [case.reference(orc, a, b, c, 1) for case, (a, b, c) in zip(ho.GROUPED, ops)]
    for want in wants:
        ho.conditions(kind, want, 1)
    outs = grouped_run(xs, torch_gpu, fmt, ops, ho.fills(fmt)[0])
    for case, (got, before, lc), want in zip(ho.GROUPED, outs, wants):
        assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), case.id
        assert ho.same_values(ho.peel(got, lc), want), (case.id, kind, ho.differences(ho.peel(got, lc), want))


# ---- tiled GEMM (kernels/tgemm.hip) and its 16-bit forms (kernels/tgemm_lowp.hip) ----------------------------------------------
def stored(x, trans):
    """a logical (1, rows, cols) operand as the matrix that lies in memory"""
    return np.ascontiguousarray(x.transpose(0, 2, 1)) if trans else x


def tgemm_layouts(m, n, k, ta, tb):
    return (ho.Layout(k if ta else m, m if ta else k, 1, extra=0), ho.Layout(n if tb else k, k if tb else n, 1, extra=0), ho.Layout(m, n, 1, extra=0))


def inner(flat, layout):
    """the caller's view of a guarded array: what lies between the guard bands"""
    return flat[layout.guard:layout.total - layout.guard]


def tgemm_run(xs, orc, torch, fmt, trans, m, n, k, beta, a, b, c, fill):
    ta, tb = trans[0] == "T", trans[1] == "T"
    la, lb, lc = tgemm_layouts(m, n, k, ta, tb)
    fa, fb, fc = ho.surround(stored(a, ta), la, fill), ho.surround(stored(b, tb), lb, fill), ho.surround(c, lc, fill)
    case = TgemmCase(orc, xs, ho.np_dtype(fmt), ta, tb, m, n, k, beta, pad=3, a=inner(fa, la), b=inner(fb, lb), c=inner(fc, lc))
    assert (case.lda, case.ldb, case.ldc) == (la.ld, lb.ld, lc.ld)
    keep, h = case.handle(xs)
    da, db, dc = (upload(torch, x) for x in (fa, fb, fc))
    xs.gemm_thread(h, at(da, la), at(db, lb), at(dc, lc))
    torch.cuda.synchronize()
    name = xs.last_kernel()
    assert name == "tgemm_%s_%s" % (fmt, trans.lower()), name
    check_untouched(da, db, fa, fb)
    gold = fc.copy()
    inner(gold, lc)[:] = case.gold  # the family's reference: the oracle on the operands as they lie
    return download(dc, fc), fc, lc, ho.peel(gold, lc)


TGEMM_SHAPE = lambda xs: (xs.lib().libxsmm_amd_gemm_tile() + 1, 33, 35)


@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("trans", ["NN", "NT", "TN", "TT"])
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_gaps_tgemm(xs, orc, torch_gpu, fmt, trans, beta):
    ho.assert_environment(orc)
    m, n, k = TGEMM_SHAPE(xs)
    rng = np.random.default_rng(ho.seed_of("tgemm", fmt, trans, beta))
    a, b, c = (rng.uniform(-1, 1, s).astype(ho.np_dtype(fmt)) for s in ((1, m, k), (1, k, n), (1, m, n)))
    want = ho.chain(orc, a, b, c, beta)
    results = []
    for fill in ho.fills(fmt):
        got, before, lc, gold = tgemm_run(xs, orc, torch_gpu, fmt, trans, m, n, k, beta, a, b, c, fill)
        assert ho.same_values(gold, want)
        assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
        got = ho.peel(got, lc)
        assert ho.same_values(got, want), (fmt, trans, beta, float(fill), ho.differences(got, want))
        results.append(got)
    assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("trans", ["NN", "NT", "TN", "TT"])
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_values_tgemm(xs, orc, torch_gpu, fmt, trans, beta, kind):
    ho.assert_environment(orc)
    m, n, k = TGEMM_SHAPE(xs)
    a, b, c = ho.operands(kind, fmt, ho.seed_of("tgemm", fmt, kind, beta), 1, m, n, k)
    want = ho.chain(orc, a, b, c, beta)
    ho.conditions(kind, want, beta)
    got, before, lc, gold = tgemm_run(xs, orc, torch_gpu, fmt, trans, m, n, k, beta, a, b, c, ho.fills(fmt)[0])
    assert ho.same_values(gold, want)
    assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
    got = ho.peel(got, lc)
    assert ho.same_values(got, want), (fmt, trans, beta, kind, ho.differences(got, want))


LOWP_NAMES = dict(lg.NAMES, fast="tgemm_bf16fast_")


def lowp_run(xs, torch, kind, trans, m, n, k, beta, a, b, c, fill_ab, fill_c, fast=False):
    """kind: 0 / 1 / 2 of lowp_gemm_common; a, b: uint16 (1, rows, cols), c: int32 or float32 -> (C back, C before, layout, gold)"""
    ta, tb = trans[0] == "T", trans[1] == "T"
    la, lb, lc = tgemm_layouts(m, n, k, ta, tb)
    fa, fb, fc = ho.surround(stored(a, ta), la, fill_ab), ho.surround(stored(b, tb), lb, fill_ab), ho.surround(c, lc, fill_c)
    case = lg.Case(kind, trans, m, n, k, beta, pad=3, a=inner(fa, la), b=inner(fb, lb), c=inner(fc, lc))
    assert (case.lda, case.ldb, case.ldc) == (la.ld, lb.ld, lc.ld)
    da, db, dc = (upload(torch, x) for x in (fa, fb, fc))
    before = xs.set_lowp_fast(fast)
    try:
        assert 0 == case.run(xs, at(da, la), at(db, lb), at(dc, lc))
        torch.cuda.synchronize()
    finally:
        xs.set_lowp_fast(before)
    name = xs.last_kernel()
    assert name == LOWP_NAMES["fast" if fast else kind] + trans.lower(), name
    check_untouched(da, db, fa, fb)
    gold = fc.copy()
    inner(gold, lc)[:] = case.gold
    return download(dc, fc), fc, lc, ho.peel(gold, lc)


def lowp_shapes(xs):
    T = xs.lib().libxsmm_amd_gemm_tile()
    return [(T + 1, 33, 35), (T + 1, 33, 34)]


@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("trans", ["NN", "TT"])
@pytest.mark.parametrize("kind", [0, 1, 2, "fast"])
def test_gaps_tgemm_lowp(xs, orc, torch_gpu, kind, trans, beta):
    """the 16-bit tiled GEMM: i16 -> i32, i16 -> f32, bf16 -> f32 and the opt-in fast bf16 mode (whose sums have no fixed order:
    its two runs must still agree byte for byte, and its values keep the bound of test_fast_mode_error_bound_and_determinism)"""
    ho.assert_environment(orc)
    fast = kind == "fast"
    k3 = 2 if fast else kind
    in_fmt, out_fmt = ("bf16" if k3 == 2 else "i16"), ("i32" if k3 == 0 else "f32")
    for m, n, k in lowp_shapes(xs):
        rng = np.random.default_rng(ho.seed_of("tgemm_lowp", kind, trans, beta, k))
        a, b = (lg.rand_inputs(rng, k3, s[0] * s[1]).reshape((1,) + s) for s in ((m, k), (k, n)))
        c = lg.rand_c(rng, k3, m * n).reshape(1, m, n)
        results = []
        for fill_ab, fill_c in zip(ho.fills(in_fmt), ho.fills(out_fmt)):
            got, before, lc, gold = lowp_run(xs, torch_gpu, k3, trans, m, n, k, beta, a, b, c, fill_ab, fill_c, fast)
            assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
            got = ho.peel(got, lc)
            if fast:
                A, B = lg.widen(a[0]).astype(np.float64), lg.widen(b[0]).astype(np.float64)
                exact = A @ B + (c[0] if beta else 0)
                bound = (k + 1) * 2.0 ** -23 * (np.abs(A) @ np.abs(B) + (np.abs(c[0]) if beta else 0))
                assert np.all(np.abs(got[0].astype(np.float64) - exact) <= bound)
            else:
                assert ho.same_values(got, gold), (kind, trans, beta, k, ho.differences(got, gold))
            results.append(got)
        assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("trans", ["NN", "TT"])
def test_values_tgemm_i16f32(xs, orc, torch_gpu, trans):
    """i16 -> f32 has no floating inputs, so no generator applies: what can sit at the edge of the number line is C under
    beta = 1. acc = acc + (float)(a * b): a NaN, +-Inf stay what they are, +-FLT_MAX and its neighbour do not move (a term is
    below 2^31, their last place is 2^104), -0.0 and subnormals take part in the first rounded add like any number."""
    ho.assert_environment(orc)
    edge = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7ffffe, 0x80000000, 0x00000001, 0x807fffff, 0x00800000],
                    dtype=np.uint32).view(np.float32)
    for m, n, k in lowp_shapes(xs):
        rng = np.random.default_rng(ho.seed_of("tgemm_i16f32", trans, k))
        a, b = (lg.rand_inputs(rng, 1, s[0] * s[1]).reshape((1,) + s) for s in ((m, k), (k, n)))
        a[0, 1, :] = 0                                   # a row of zero products: C keeps its value there, but -0.0 + (+0.0) = +0.0
        c = lg.rand_c(rng, 1, m * n).reshape(1, m, n)
        c[0][rng.random((m, n)) < 0.3] = 0
        where = rng.random((m, n)) < 0.3
        c[0][where] = rng.choice(edge, int(where.sum()))
        c[0, 1, :edge.size] = edge
        c[0, m - 1, n - 1], c[0, 0, 0] = np.float32(np.nan), np.float32(-np.inf)
        got, before, lc, gold = lowp_run(xs, torch_gpu, 1, trans, m, n, k, 1, a, b, c, ho.fills("i16")[0], ho.fills("f32")[0])
        assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
        assert np.isnan(gold).any() and np.isinf(gold).any() and 4 * np.isnan(gold).sum() <= gold.size
        assert gold[0, 1, 6] == 0 and not np.signbit(gold[0, 1, 6]) and gold[0, 1, 3] == edge[3] and gold[0, 1, 7] == edge[7]
        got = ho.peel(got, lc)
        assert ho.same_values(got, gold), (trans, k, ho.differences(got, gold))


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("trans", ["NN", "TT"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_values_tgemm_bf16(xs, orc, torch_gpu, mode, trans, beta, kind):
    """bf16 -> f32 on the matrix cores. The exact mode is one fma chain per element (v_mfma_f32_32x32x2_f32 on the widened
    operands): where a product of the chain is subnormal or beyond the largest float32 -- the only places where a bf16 x bf16 product
    is not exact in float32 -- the element equals the oracle's fma chain, one rounding per step; everywhere else it equals the gold
    loop, which rounds product and sum separately. The fast mode promises no order of its sums: NaN and Inf must stand where every order puts
    them, finite values keep the bound of tests/test_lowp_gemm_gpu.py::test_fast_mode_error_bound_and_determinism."""
    ho.assert_environment(orc)
    for m, n, k in lowp_shapes(xs):
        a, b, c = ho.operands(kind, "bf16", ho.seed_of("tgemm_bf16", kind, beta, k), 1, m, n, k)
        gold = ho.gold_bf16(a, b, c, beta)
        ho.conditions(kind, gold, beta)
        fill_ab, fill_c = ho.fills("bf16")[0], ho.fills("f32")[0]
        got, before, lc, family = lowp_run(xs, torch_gpu, 2, trans, m, n, k, beta, ho.bf16_bits(a), ho.bf16_bits(b), c, fill_ab, fill_c, mode == "fast")
        assert ho.same_values(family, gold)  # the family's reference is the gold loop
        assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
        got = ho.peel(got, lc)
        if mode == "exact":
            fma, sub = ho.chain(orc, a, b, c, beta), ho.inexact_product(a, b)
            assert kind != "underflow" or (sub.any() and not sub.all())
            assert ho.same_values(got[~sub], gold[~sub]), (trans, beta, kind, k, ho.differences(got[~sub], gold[~sub]))
            assert ho.same_values(got[sub], fma[sub]), (trans, beta, kind, k, ho.differences(got[sub], fma[sub]))
            continue
        A, B, C0 = a[0].astype(np.float64), b[0].astype(np.float64), (c[0].astype(np.float64) if beta else 0.0)
        with np.errstate(all="ignore"):
            exact, mag = A @ B + C0, np.abs(A) @ np.abs(B) + np.abs(C0)
        big = float(np.finfo(np.float32).max)
        if kind == "specials":   # a NaN or Inf of the exact sum does not depend on the order of the terms
            assert np.array_equal(np.isnan(got[0]), np.isnan(exact)) and np.array_equal(got[0][np.isinf(exact)], exact[np.isinf(exact)].astype(np.float32))
            ok = np.isfinite(exact)
            assert np.all(np.abs(got[0][ok] - exact[ok]) <= (k + 1) * 2.0 ** -23 * mag[ok])
        elif kind == "underflow":  # nothing here can leave the finite range; an add errs by half a unit of the smallest subnormal at most
            assert np.isfinite(got[0]).all()
            assert np.all(np.abs(got[0] - exact) <= (k + 1) * (2.0 ** -23 * mag + 2.0 ** -149))
        else:                      # no partial sum of any order exceeds the sum of the magnitudes; a total beyond the range cannot stay finite
            assert np.isfinite(got[0][mag < big / 2]).all()
            assert not np.isfinite(got[0][np.abs(exact) > big * 1.01]).any()


# ---- fsspmdm: the operator's values travel as text into a hiprtc-built kernel ------------------------------------------------------
def fsspmdm_run(xs, torch, fmt, jit, a, b, c, beta, fill, batched):
    """B and C are row major with leading dimensions of ncols + 3 between guard bands, A row major with lda = K + 3; everything
    that is no element holds `fill`. -> (C back, C before, layout)"""
    L = xs.lib()
    m, k = a.shape
    ncols = b.shape[1]
    la, lb, lc = ho.Layout(k, m, 1, extra=0), ho.Layout(ncols, k, 1, extra=0), ho.Layout(ncols, m, 1, extra=0)  # (row major: the roles of rows and columns swap)
    fa, fb, fc = (ho.surround(np.ascontiguousarray(x.T), lay, fill) for x, lay in ((a, la), (b, lb), (c, lc)))
    sfx = "d" if fmt == "f64" else "s"
    create, destroy = getattr(L, "libxsmm_%sfsspmdm_create" % sfx), getattr(L, "libxsmm_%sfsspmdm_destroy" % sfx)
    execute, execb = getattr(L, "libxsmm_%sfsspmdm_execute" % sfx), getattr(L, "libxsmm_amd_%sfsspmdm_execute_batch" % sfx)
    with Settings(xs, 1, {"LIBXSMM_AMD_JIT": "1" if jit else "0"}):
        hd = create(m, ho.FSSPMDM_N, k, la.ld, lb.ld, lc.ld, 1.0, float(beta), fa.ctypes.data + la.guard * fa.itemsize)
        assert hd
        db, dc = upload(torch, fb), upload(torch, fc)
        if batched:
            assert 0 == execb(hd, at(db, lb), at(dc, lc), ho.FSSPMDM_PANELS)
        else:
            for p in range(ho.FSSPMDM_PANELS):
                execute(hd, at(db, lb) + p * ho.FSSPMDM_N * fb.itemsize, at(dc, lc) + p * ho.FSSPMDM_N * fc.itemsize)
        torch.cuda.synchronize()
        name = xs.last_kernel()
        destroy(hd)
    want = "fsspmdm_%s_%s" % (fmt, "jit_operator" if jit else "csr_cols")
    assert name == want, (name, want)
    assert np.array_equal(ho.raw(download(db, fb)), ho.raw(fb)), "B was written"
    return download(dc, fc), fc, lc


@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("jit", [True, False], ids=["jit", "precompiled"])
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_gaps_fsspmdm(xs, orc, torch_gpu, fmt, jit, beta):
    ho.assert_environment(orc)
    a = ho.fsspmdm_operator(orc, fmt, False)
    b, c = ho.fsspmdm_operands(None, fmt, ho.seed_of("fsspmdm", fmt, None, beta), a, beta)
    want = ho.fsspmdm_reference(orc, a, b, c, beta)
    results = []
    for fill, batched in zip(ho.fills(fmt), (True, False)):
        got, before, lc = fsspmdm_run(xs, torch_gpu, fmt, jit, a, b, c, beta, fill, batched)
        assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
        got = ho.peel(got, lc)[0].T
        assert ho.same_values(got, want), (fmt, jit, beta, float(fill), ho.differences(got, want))
        results.append(got)
    assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("beta", [1, 0])
@pytest.mark.parametrize("jit", [True, False], ids=["jit", "precompiled"])
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_values_fsspmdm(xs, orc, torch_gpu, fmt, jit, beta, kind):
    """operator entries of 2^-149 / 2^-1074 and -FLT_MAX / -DBL_MAX have to arrive in the generated kernel bit for bit, an entry of
    -0.0 is no entry; the dense operand carries the specials"""
    ho.assert_environment(orc)
    a = ho.fsspmdm_operator(orc, fmt, True)
    b, c = ho.fsspmdm_operands(kind, fmt, ho.seed_of("fsspmdm", fmt, kind, beta), a, beta)
    want = ho.fsspmdm_reference(orc, a, b, c, beta)
    ho.conditions(kind, want, beta)
    got, before, lc = fsspmdm_run(xs, torch_gpu, fmt, jit, a, b, c, beta, ho.fills(fmt)[0], True)
    assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
    got = ho.peel(got, lc)[0].T
    assert ho.same_values(got, want), (fmt, jit, beta, kind, ho.differences(got, want))


# ---- the fully-connected layer (kernels/fc.hip): fwd, bwd, upd; fp32 and 16-bit; both tiles ------------------------------------------
FC_DEST = {fc.FWD: fc.REG_OUT, fc.BWD: fc.GRAD_IN, fc.UPD: fc.GRAD_FIL}
FC_KERNEL = {False: {k: "fc_f32" for k in FC_DEST}, True: {fc.FWD: "fc_bf16_fwd", fc.BWD: "fc_bf16_bwd", fc.UPD: "fc_bf16_upd"}}


def fc_run(xs, torch, name, tile, kind, plain, fill_index):
    """one pass of a layer whose six tensors lie between guard bands of the fill; the destinations hold the fill as well (they are
    never read). -> (the destination's elements, the expectation of tests/fc_common.py)"""
    L = xs.lib()
    d = fc.COMPUTE_CASES[name]
    h = fc.Handle(d)
    with np.errstate(all="ignore"):
        want = fc.tensors(h, *plain)
    with Settings(xs, 1, {"LIBXSMM_AMD_FC_TILE": tile}):
        handle, st = xs.fc_create(d["N"], d["C"], d["K"], d["bn"], d["bk"], d["bc"], 1, d["datatype_in"], d["datatype_out"], d["buffer_format"],
                                  d["filter_format"], d["fuse_ops"])
        assert handle and st == h.status
        host, dev, tensors = {}, {}, []
        for t in fc.TENSOR_TYPES:
            dt = fc.dtype_of(h, t)
            lay = ho.Layout(want[t].size, 1, 1, ld=want[t].size, extra=0)
            content = np.full(want[t].size, ho.fills("bf16" if dt == np.uint16 else "f32")[fill_index], dtype=dt) if t in FC_DEST.values() else want[t].astype(dt)
            host[t] = ho.surround(content.reshape(1, -1, 1), lay, ho.fills("bf16" if dt == np.uint16 else "f32")[fill_index])
            dev[t] = upload(torch, host[t])
            tensors.append(xs.fc_bind_new(handle, t, dev[t][ho.GUARD:ho.GUARD + want[t].size]))
        size = L.libxsmm_dnn_fullyconnected_get_scratch_size(handle, C.byref(C.c_uint()))
        scratch = torch.full((size,), 0x5a, dtype=torch.uint8, device="cuda")
        assert 0 == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))
        assert 0 == xs.fc_execute(handle, kind)
        torch.cuda.synchronize()
        name_ran = xs.last_kernel()
        got = {t: download(dev[t], host[t]) for t in fc.TENSOR_TYPES}
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == L.libxsmm_dnn_destroy_fullyconnected(handle)
    assert name_ran == "%s_t%s" % (FC_KERNEL[h.mixed][kind], tile), name_ran
    for t in fc.TENSOR_TYPES:
        if t != FC_DEST[kind]:
            assert np.array_equal(ho.raw(got[t]), ho.raw(host[t])), "tensor %d was written" % t
    out = got[FC_DEST[kind]]
    assert np.array_equal(ho.raw(out[:ho.GUARD]), ho.raw(host[FC_DEST[kind]][:ho.GUARD])) and np.array_equal(ho.raw(out[-ho.GUARD:]), ho.raw(host[FC_DEST[kind]][-ho.GUARD:]))
    return out[ho.GUARD:-ho.GUARD], want[FC_DEST[kind]]


@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("name", ho.FC_CASES)
def test_gaps_fc(xs, orc, torch_gpu, name, tile):
    """the tensors of the layer are dense: what can be poisoned is what lies around them and the destinations themselves"""
    ho.assert_environment(orc)
    chains = ho.fc_chains(orc, name, None)
    for kind, (plain, _) in zip((fc.FWD, fc.BWD, fc.UPD), chains):
        results = []
        for fill_index in (0, 1):
            got, want = fc_run(xs, torch_gpu, name, tile, kind, plain, fill_index)
            assert ho.same_values(got, want), (name, tile, kind, fill_index, ho.differences(got, want))
            results.append(got)
        assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes around the tensors"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("name", ho.FC_CASES)
def test_values_fc(xs, orc, torch_gpu, name, tile, kind):
    """every pass on a generated chain of its own; dx and dw of the 16-bit case leave as bf16, rounded to nearest even in the
    kernel's own code: overflow to Inf and NaN-stays-NaN are part of the expectation (fc_common.expected)"""
    ho.assert_environment(orc)
    chains = ho.fc_chains(orc, name, kind)
    for which, (plain, result) in zip((fc.FWD, fc.BWD, fc.UPD), chains):
        ho.conditions(kind, result, 0)  # of every pass on its own
        got, want = fc_run(xs, torch_gpu, name, tile, which, plain, 0)
        assert ho.same_values(got, want), (name, tile, which, kind, ho.differences(got, want))


# ---- low-precision SMM: the dispatched kernels (kernels/smm_lowp.hip) and their hiprtc-built forms --------------------------------------
LOWP_TYPES = {0: ("i16", "i32"), 2: ("bf16", "f32"), 3: ("bf16", "bf16")}
# what a kernel does with a product that float32 cannot hold exactly: the matrix-core form is one fma chain (one rounding per step),
# the others round product and sum separately like the gold loop
LOWP_FMA = {"smm_bf16f32_mfma_wave_jit_lowp": True, "smm_bf16_mfma_wave_jit_lowp": True}


def lowp_smm_run(xs, orc, torch, case, beta, extra, a, b, c, fill_index):
    """-> (C back, C before, its layout, the family's reference: xo_gemm_lowp item by item on A in pairs of k)"""
    L = xs.lib()
    m, n, k = case.shape
    in_fmt, out_fmt = LOWP_TYPES[case.kind]
    nc = c.shape[0]
    packed = np.stack([lg.pack_pairs(np.ascontiguousarray(a[t].T).ravel(), m, m, k) for t in range(case.batch)])
    la, lb, lc = ho.Layout(m * k, 1, case.batch, m * k, extra), ho.Layout(k, n, case.batch, k, extra), ho.Layout(m, n, nc, m, extra)
    fa = ho.surround(packed.reshape(case.batch, m * k, 1), la, ho.fills(in_fmt)[fill_index])
    fb, fc_ = ho.surround(b, lb, ho.fills(in_fmt)[fill_index]), ho.surround(c, lc, ho.fills(out_fmt)[fill_index])
    ref = np.empty_like(c)
    for t in range(case.batch):  # (batch-reduce: the chain goes on in one C, whose fp32 sums the references below restate)
        if not case.reduce:
            ct = np.array(c[t].T, order="C").ravel()
            assert 0 == orc.gemm_lowp(case.kind, 0 if beta else 1, m, n, k, m, k, m, packed[t], np.ascontiguousarray(b[t].T).ravel(), ct, 1.0)
            ref[t] = ct.reshape(n, m).T
    da, db, dc = (upload(torch, x) for x in (fa, fb, fc_))
    ip, op = {0: (xs.I16, xs.I32), 2: (xs.BF16, xs.F32), 3: (xs.BF16, xs.BF16)}[case.kind]
    with Settings(xs, case.mfma, {"LIBXSMM_AMD_JIT_MINBATCH": "1" if case.jit else "100000"}):
        if case.reduce:
            disp = L.libxsmm_bsmmdispatch_reducebatch if case.kind == 2 else L.libxsmm_bmmdispatch_reducebatch
            disp.restype, disp.argtypes = C.c_void_p, [C.c_int] * 3 + [C.c_void_p] * 7
            be = C.c_float(float(beta))
            fn = disp(m, n, k, None, None, None, None, C.addressof(be), None, None)
            assert fn
            pa = (da.data_ptr() + la.offsets() * 2).astype(np.uint64)
            pb = (db.data_ptr() + lb.offsets() * 2).astype(np.uint64)
            xs.call_kernel(fn, pa, pb, at(dc, lc), np.array([case.batch], dtype=np.uint64))
        else:
            blob = xs.DescriptorBlob()
            L.libxsmm_gemm_descriptor_dinit2.restype = C.c_void_p
            L.libxsmm_gemm_descriptor_dinit2.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_double, C.c_double, C.c_int, C.c_int]
            desc = L.libxsmm_gemm_descriptor_dinit2(C.byref(blob), ip, op, m, n, k, m, k, m, 1.0, float(beta), 0, 0)
            assert desc
            assert 0 == L.libxsmm_amd_gemm_batch_strided(C.c_void_p(desc), at(da, la), at(db, lb), at(dc, lc), la.stride, lb.stride, lc.stride, case.batch)
        torch.cuda.synchronize()
        name = xs.last_kernel()
    print("kernel %-32s %s beta %d extra %d" % (name, case.id, beta, extra))
    assert name == case.kernel_at(extra), (name, case.kernel_at(extra))
    check_untouched(da, db, fa, fb)
    return download(dc, fc_), fc_, lc, (None if case.reduce else ref)


def lowp_expectation(case, orc, a, b, c, beta, name):
    """bf16 kinds: the gold loop, and where a product is not exact in float32 what the kernel `name` is pinned to; a bf16 result is
    the upper half of the float32 sum"""
    gold, hit = case.sums(a, b, c, beta), case.inexact(a, b)
    want = np.where(hit, case.sums(a, b, c, beta, fma=orc), gold) if LOWP_FMA.get(name) else gold
    return (ho.bf16_bits(want) if case.kind == 3 else want), gold, hit


LOWP_VARIANTS = [(c, be) for c in ho.LOWP_CASES for be in c.betas]
LOWP_IDS = ["%s-beta%d" % (c.id, be) for c, be in LOWP_VARIANTS]


@pytest.mark.parametrize("variant", LOWP_VARIANTS, ids=LOWP_IDS)
def test_gaps_smm_lowp(xs, orc, torch_gpu, variant):
    case, beta = variant
    ho.assert_environment(orc)
    a, b, c = case.operands(None, beta)
    for extra in case.extras:
        results = []
        for fill_index in (0, 1):
            got, before, lc, ref = lowp_smm_run(xs, orc, torch_gpu, case, beta, extra, a, b, c, fill_index)
            assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
            got = ho.peel(got, lc)
            if case.kind != 0:
                want, gold, hit = lowp_expectation(case, orc, a, b, c, beta, case.kernel_at(extra))
                assert not hit.any() and (ref is None or ho.same_values(ref, want))  # uniform data: the family's reference is the gold loop
                ref = want
            assert ho.same_values(got, ref), (case.id, beta, extra, fill_index, ho.differences(got, ref))
            results.append(got)
        assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes in the gaps"


@pytest.mark.parametrize("kind", ho.KINDS)
@pytest.mark.parametrize("variant", [v for v in LOWP_VARIANTS if v[0].kind != 0], ids=[i for i, v in zip(LOWP_IDS, LOWP_VARIANTS) if v[0].kind != 0])
def test_values_smm_lowp(xs, orc, torch_gpu, variant, kind):
    case, beta = variant
    ho.assert_environment(orc)
    a, b, c = case.operands(kind, beta)
    want, gold, hit = lowp_expectation(case, orc, a, b, c, beta, case.kernel)
    ho.conditions(kind, gold, beta)
    got, before, lc, ref = lowp_smm_run(xs, orc, torch_gpu, case, beta, case.extras[0], a, b, c, 0)
    if ref is not None:  # the family's reference (xo_gemm_lowp) is the gold loop
        assert ho.same_values(ref, ho.bf16_bits(gold) if case.kind == 3 else gold)
    assert np.array_equal(ho.gaps(got, lc), ho.gaps(before, lc)), "the gaps of C changed"
    got = ho.peel(got, lc)
    assert ho.same_values(got[~hit], want[~hit]), (case.id, beta, kind, "exact products", ho.differences(got[~hit], want[~hit]))
    assert ho.same_values(got[hit], want[hit]), (case.id, beta, kind, "inexact products", int(hit.sum()), ho.differences(got[hit], want[hit]))


# ---- spmdm: create + compute of the batch interface (kernels/sparse.hip), gather and matrix-core forms ----------------------------------
@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("mfma", [0, 1], ids=["gather", "matrix-cores"])
def test_gaps_and_subnormal_entries_spmdm(xs, orc, torch_gpu, mfma, beta):
    """the smallest batch problem of tests/test_sparse_gpu.py (M = K = 64, N = 48) at 50 % density, five items. The interface takes
    tight operands, so the gaps are the guard bands around A, B and C. A carries subnormal entries (+-2^-149 and +-2^-127): create
    keeps them as entries (only +-0 is no entry), and C equals the oracle's chain, in which they meet B's largest numbers."""
    ho.assert_environment(orc)
    torch, L = torch_gpu, xs.lib()
    M, N, K, batch = 64, 48, 64, 5
    rng = np.random.default_rng(ho.seed_of("spmdm", mfma, beta))
    a = rng.uniform(-1, 1, (batch, M, K)).astype(np.float32)
    a[rng.random((batch, M, K)) < 0.5] = 0.0
    tiny = rng.random((batch, M, K)) < 0.05
    a[tiny] = rng.choice(np.array([2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127], np.float32), int(tiny.sum()))
    a[1, 3, :] = -0.0                                    # -0 counts as zero
    a[:, 2, :] = np.where(rng.random((batch, K)) < 0.5, rng.choice(np.array([2.0 ** -149, -2.0 ** -127], np.float32), (batch, K)), 0.0)
    b = rng.uniform(-1, 1, (batch, K, N)).astype(np.float32)
    b[:, :, 5] *= np.float32(2.0 ** 120)                 # a row of subnormal entries only, times large numbers: flushing them shows
    c = rng.uniform(-1, 1, (batch, M, N)).astype(np.float32)

    def oracle(av):
        out = c.copy().ravel()
        orc.spmdm_exec_batch(orc.FMA, M, N, K, 48, "N", "N", "N", beta, av.ravel(), b.ravel(), out, batch, 1)
        return out.reshape(batch, M, N)
    ref = oracle(a)
    assert np.isfinite(ref).all() and not ho.same_values(ref[:, 2, 5], oracle(np.where(np.abs(a) < 2.0 ** -126, np.float32(0), a))[:, 2, 5])
    la, lb, lc = (ho.Layout(x.shape[2], x.shape[1], batch, ld=x.shape[2], extra=0) for x in (a, b, c))  # (row major, tight)
    results = []
    old = L.libxsmm_amd_set_mfma(mfma)
    try:
        for fill in ho.fills("f32"):
            fa, fb, fc_ = (ho.surround(np.ascontiguousarray(x.transpose(0, 2, 1)), lay, fill) for x, lay in ((a, la), (b, lb), (c, lc)))
            da, db, dc = (upload(torch, x) for x in (fa, fb, fc_))
            sb = L.libxsmm_amd_spmdm_batch_create(M, N, K, batch)
            assert sb
            assert 0 == L.libxsmm_amd_spmdm_batch_create_slices(sb, b"N", C.c_void_p(at(da, la)))
            assert xs.last_kernel() == "spmdm_create_slices_staged", xs.last_kernel()
            ri = np.zeros(M + 1, dtype=np.uint16); ci = np.zeros(M * K, dtype=np.uint16); va = np.zeros(M * K, dtype=np.float32)
            for item in (0, 1, batch - 1):
                assert 0 == L.libxsmm_amd_spmdm_batch_get_slice(sb, item, xs.dptr(ri), xs.dptr(ci), xs.dptr(va), M * K)
                hnd, sl = orc.spmdm_slices(M, N, K, 48, "N", a[item].ravel())
                oi, oc, ov = sl[0]
                nnz = int(oi[M])
                assert nnz == int(np.sum(a[item] != 0)) and np.array_equal(ri, oi) and np.array_equal(ci[:nnz], oc)
                assert np.array_equal(va[:nnz].view(np.uint32), ov.view(np.uint32))  # subnormal entries arrive bit for bit
            be = C.c_float(beta)
            assert 0 == L.libxsmm_amd_spmdm_batch_compute(sb, b"N", C.c_void_p(at(db, lb)), b"N", C.byref(be), C.c_void_p(at(dc, lc)))
            torch.cuda.synchronize()
            name = xs.last_kernel()
            L.libxsmm_amd_spmdm_batch_destroy(sb)
            print("kernel %s mfma %d beta %g" % (name, mfma, beta))
            # the gather form alone with the matrix cores off; with them on both are launched and the device picks per item
            assert name == ("spmdm_compute_mfma|wg_lds" if mfma else "spmdm_compute_wg_lds"), name
            check_untouched(da, db, fa, fb)
            got = download(dc, fc_)
            assert np.array_equal(ho.gaps(got, lc), ho.gaps(fc_, lc)), "the guard bands of C changed"
            got = ho.peel(got, lc).transpose(0, 2, 1)
            assert ho.same_values(np.ascontiguousarray(got), ref), (mfma, beta, float(fill), ho.differences(np.ascontiguousarray(got), ref))
            results.append(np.ascontiguousarray(got))
    finally:
        L.libxsmm_amd_set_mfma(old)
    assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes around the operands"


def banded(x, fill):
    """a tight array between two guard bands of `fill`"""
    band = np.full(ho.GUARD, fill, dtype=x.dtype)
    return np.concatenate([band, x.ravel(), band])


@pytest.mark.parametrize("beta_bits", [1, 0])
def test_gaps_and_subnormal_entries_spmdm_bfloat16(xs, orc, torch_gpu, beta_bits):
    """the bf16 twins of the per-problem interface (libxsmm_spmdm_createSparseSlice_bfloat16_thread / compute_bfloat16_thread) on
    the shape of tests/test_sparse_gpu.py::test_spmdm_bfloat16_twins (M = 150, N = 70, K = 200, 70 % zeros). The operands are
    tight: the gaps are guard bands of 0x7fc0, then 0x7f80 around A and B and of NaN, then Inf around C. A carries bf16 subnormals
    (exponent field 0: 0x0001, 0x8001, 0x0040, 0x807f); create has to keep them as entries -- only +-0 is none --, which shows in
    C: row 2 of A holds nothing else, and column 5 of B is large enough to lift their products into the normal range, so the
    reference of an A with the subnormals flushed differs there. *beta is the number its 16 bits spell (pattern 1: beta = 1)."""
    ho.assert_environment(orc)
    torch, L = torch_gpu, xs.lib()
    M, N, K = 150, 70, 200
    rng = np.random.default_rng(ho.seed_of("spmdm-bf16", beta_bits))
    a = ho.bf16_bits(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    a[rng.random((M, K)) < 0.7] = 0
    subs = np.array([0x0001, 0x8001, 0x0040, 0x807f], dtype=np.uint16)
    tiny = rng.random((M, K)) < 0.03
    a[tiny] = rng.choice(subs, int(tiny.sum()))
    a[2, :] = np.where(rng.random(K) < 0.5, rng.choice(subs, K), 0)
    a[3, :] = 0x8000                                        # -0 counts as zero
    b = ho.bf16_bits(rng.uniform(-1, 1, (K, N)).astype(np.float32))
    b[:, 5] = ho.bf16_bits(ho.bf16_widen(b[:, 5]) * np.float32(2.0 ** 120))
    c = rng.uniform(-1, 1, (M, N)).astype(np.float32)

    def oracle(av):
        out = c.copy().ravel()
        orc.spmdm_exec_bf16(orc.FMA, M, N, K, 48, "N", "N", "N", beta_bits, np.ascontiguousarray(av).ravel(), b.ravel(), out)
        return out.reshape(M, N)
    ref = oracle(a)
    flushed = np.where((a & 0x7f80) == 0, np.uint16(0), a)
    assert np.isfinite(ref).all() and ref[2, 5] != 0 and not ho.same_values(ref[2], oracle(flushed)[2])
    results = []
    for fill_ab, fill_c in zip(ho.fills("bf16"), ho.fills("f32")):
        fa, fb, fc_ = banded(a, fill_ab), banded(b, fill_ab), banded(c, fill_c)
        da, db, dc = (upload(torch, x) for x in (fa, fb, fc_))
        pa, pb, pc = (C.c_void_p(t.data_ptr() + ho.GUARD * t.element_size()) for t in (da, db, dc))
        h = xs.SpmdmHandle(); slices = C.POINTER(xs.CSRSlice)()
        L.libxsmm_spmdm_init(M, N, K, 1, C.byref(h), C.byref(slices))
        alpha, be = C.c_ushort(0x3F80), C.c_ushort(beta_bits)
        for blk in range(L.libxsmm_spmdm_get_num_createSparseSlice_blocks(C.byref(h))):
            L.libxsmm_spmdm_createSparseSlice_bfloat16_thread(C.byref(h), b"N", pa, slices, blk, 0, 1)
        created = xs.last_kernel()
        for blk in range(L.libxsmm_spmdm_get_num_compute_blocks(C.byref(h))):
            L.libxsmm_spmdm_compute_bfloat16_thread(C.byref(h), b"N", b"N", C.byref(alpha), slices, pb, b"N", C.byref(be), pc, blk, 0, 1)
        torch.cuda.synchronize()
        name = xs.last_kernel()
        L.libxsmm_spmdm_destroy(C.byref(h))
        print("kernel %s, %s beta bits %d" % (created, name, beta_bits))
        assert created == "spmdm_create_slice_wg" and name == "spmdm_compute_tiled", (created, name)
        check_untouched(da, db, fa, fb)
        got = download(dc, fc_)
        assert np.array_equal(ho.raw(got[:ho.GUARD]), ho.raw(fc_[:ho.GUARD])) and np.array_equal(ho.raw(got[-ho.GUARD:]), ho.raw(fc_[-ho.GUARD:])), "the guard bands of C changed"
        got = got[ho.GUARD:-ho.GUARD].reshape(M, N)
        assert ho.same_values(got, ref), (beta_bits, ho.differences(got, ref))
        results.append(got)
    assert np.array_equal(ho.raw(results[0]), ho.raw(results[1])), "the result depends on the bytes around the operands"
