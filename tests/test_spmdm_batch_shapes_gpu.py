"""Every kernel form of the spmdm batch family at a shape that makes it do the work: the table of tests/spmdm_batch_cases.py
(tests/test_spmdm_batch_census_cpu.py holds it against the sources), create and compute.

Per case: the slices of the first, the last and three seeded items through libxsmm_amd_spmdm_batch_get_slice against a plain numpy
row scan, bit for bit (the oracle cuts its slices at 64 columns, the batch interface does not); C for every beta of the case
bit-equal to the oracle's chain; A, B and C between guard bands (tests/hostile_operands.py: quiet NaN around A and C, +Inf around
B), A, B and the bands unchanged afterwards; and xs.last_kernel() after create and after compute as plan() says."""
import ctypes as C

import numpy as np
import pytest

import hostile_operands as ho
import spmdm_batch_cases as sc

pytestmark = pytest.mark.gpu

G = ho.GUARD
_references = {}


def bits32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def banded(x, fill):
    """a tight array between two guard bands of `fill`"""
    band = np.full(G, fill, dtype=x.dtype)
    return np.concatenate([band, x.ravel(), band])


def reference(orc, case, a, b, beta):
    """(C before the call, the oracle's C): computed once per case and beta, never written to"""
    key = (case.id, beta)
    if key not in _references:
        c = sc.c_operand(case, beta)
        ref = sc.reference(orc, case, a, b, c, beta)
        c.setflags(write=False); ref.setflags(write=False)
        _references[key] = (c, ref)
    return _references[key]


class Batch(object):
    """a batch handle with the matrix-core setting of the case, A and B on the device between their bands"""
    def __init__(self, xs, torch, case, a, b):
        self.xs, self.torch, self.case, self.L = xs, torch, case, xs.lib()
        nan, inf = ho.fills("f32")
        self.fa, self.fb = banded(a, nan), banded(b, inf)
        self.old = self.L.libxsmm_amd_set_mfma(case.mfma)
        self.sb = None

    def __enter__(self):
        self.da, self.db = self.torch.from_numpy(self.fa).cuda(), self.torch.from_numpy(self.fb).cuda()
        self.sb = self.L.libxsmm_amd_spmdm_batch_create(self.case.M, self.case.N, self.case.K, self.case.batch)
        assert self.sb
        return self

    def __exit__(self, *exc):
        if self.sb:
            self.L.libxsmm_amd_spmdm_batch_destroy(self.sb)
        self.L.libxsmm_amd_set_mfma(self.old)

    def create(self):
        assert 0 == self.L.libxsmm_amd_spmdm_batch_create_slices(self.sb, self.case.trans[0].encode(), self.xs.dptr(self.da[G:]))
        return self.xs.last_kernel()

    def compute(self, c, beta, fill):
        """C after the call (flat, without its bands, which are checked here)"""
        fc = banded(c, fill)
        dc = self.torch.from_numpy(fc).cuda()
        be = C.c_float(beta)
        tb, tc = self.case.trans[1:]
        assert 0 == self.L.libxsmm_amd_spmdm_batch_compute(self.sb, tb.encode(), self.xs.dptr(self.db[G:]), tc.encode(), C.byref(be), self.xs.dptr(dc[G:]))
        self.torch.cuda.synchronize()
        name = self.xs.last_kernel()
        got = dc.cpu().numpy()
        assert np.array_equal(ho.raw(got[:G]), ho.raw(fc[:G])) and np.array_equal(ho.raw(got[-G:]), ho.raw(fc[-G:])), "the guard bands of C changed"
        return name, got[G:-G]

    def untouched(self):
        assert np.array_equal(ho.raw(self.da.cpu().numpy()), ho.raw(self.fa)), "A or its guard bands changed"
        assert np.array_equal(ho.raw(self.db.cpu().numpy()), ho.raw(self.fb)), "B or its guard bands changed"


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_spmdm_batch_shape(xs, orc, torch_gpu, case):
    ho.assert_environment(orc)
    M, N, K, batch = case.M, case.N, case.K, case.batch
    a, b = sc.operands(case)
    want = sc.plan_of(case)
    A = sc.views(case, a, b, np.zeros(batch * M * N, np.float32))[0]
    with Batch(xs, torch_gpu, case, a, b) as run:
        assert run.create() == want.create
        # ---- slices
        ri = np.zeros(M + 1, dtype=np.uint16); ci = np.zeros(M * K, dtype=np.uint16); va = np.zeros(M * K, dtype=np.float32)
        seeded = np.random.default_rng(sc.seed_of(case)).integers(0, batch, 3)
        for item in sorted(set([0, batch - 1] + [int(i) for i in seeded])):
            ri[:] = 0xDEAD
            assert 0 == run.L.libxsmm_amd_spmdm_batch_get_slice(run.sb, item, xs.dptr(ri), xs.dptr(ci), xs.dptr(va), M * K)
            wi, wc, wv = sc.slice_of(A[item])
            nnz = int(wi[M])
            assert np.array_equal(ri, wi), (case.id, item, "rowidx", int(np.argmax(ri != wi)))
            assert np.array_equal(ci[:nnz], wc), (case.id, item, "colidx", int(np.argmax(ci[:nnz] != wc)))
            assert np.array_equal(bits32(va[:nnz]), bits32(wv)), (case.id, item, "values", int(np.argmax(bits32(va[:nnz]) != bits32(wv))))
        # ---- C
        nan, inf = ho.fills("f32")
        for beta in case.betas:
            c, ref = reference(orc, case, a, b, beta)
            name, got = run.compute(c, beta, inf if beta == 0.0 else nan)  # (beta == 0: C itself is NaN, the bands differ from it)
            assert name == want.compute, (case.id, beta, name)
            bad = np.flatnonzero(bits32(got) != bits32(ref))
            print("%s beta %g: %s, %d of %d elements differ from the oracle" % (case.id, beta, name, bad.size, ref.size))
            assert bad.size == 0, (case.id, beta, bad.size, int(bad[0]) // (M * N), int(bad[0]) % (M * N))
        run.untouched()


@pytest.mark.parametrize("mfma", [0, 1], ids=["gather", "pair"])
def test_spmdm_batch_negative_zero_under_an_empty_row(xs, orc, torch_gpu, mfma):
    """The documented exception of sparse.hip: "an accumulator that is exactly -0 may end as +0". C = -0 with beta = 1 under an
    empty row of A: the oracle leaves -0. The gather kernel alone gives the oracle's bits. With the matrix cores on, this batch (50 %
    dense) is worked by the matrix-core kernel, which adds the row's zeros: the values compare equal everywhere and the bits are equal
    wherever the oracle's result is not a zero -- nothing wider than that."""
    case = sc._case("negzero", 64, 48, 64, 24, ("density", 0.5), betas=(1.0,), mfma=mfma)
    M, N, K, batch = case.M, case.N, case.K, case.batch
    A = sc.logical_a(case)
    A[:, 5, :] = 0.0
    A[3, 63, :] = 0.0
    a = A.reshape(-1)
    b = sc.operands(case)[1]
    c = sc.c_operand(case, 1.0)
    Cm = c.reshape(batch, M, N)
    Cm[:, 5, :] = -0.0
    Cm[3, 63, ::2] = -0.0
    Cm[7, 9, 11] = -0.0  # under a row with entries: the result is no zero
    ref = sc.reference(orc, case, a, b, c, 1.0)
    R = ref.reshape(batch, M, N)
    assert (bits32(R[:, 5, :]) == 0x80000000).all() and (bits32(R[3, 63, ::2]) == 0x80000000).all() and R[7, 9, 11] != 0
    if mfma:
        assert sc.covered(case) >= set([("mfma", 3, True)])
    with Batch(xs, torch_gpu, case, a, b) as run:
        assert run.create() == "spmdm_create_slices_staged"
        name, got = run.compute(c, 1.0, ho.fills("f32")[0])
        run.untouched()
    assert name == sc.plan_of(case).compute
    differ = bits32(got) != bits32(ref)
    print("%s: %d elements differ in their bits, %d of the oracle's are zeros" % (name, int(differ.sum()), int((ref == 0).sum())))
    if not mfma:
        assert not differ.any()
    else:
        assert np.array_equal(got, ref)       # -0 == +0; no NaN in this problem
        assert not (differ & (ref != 0)).any()
