"""The seeded sweep of tests/tgemm_sweep_common.py (sweep_cases) on the GPU: the tiled GEMM (libxsmm_gemm_thread, libxsmm_xgemm_omp)
and the GEMM with 16-bit inputs (libxsmm_amd_lowp_gemm_thread) bit for bit against the expectation that
tests/test_tgemm_sweep_cpu.py holds to a float64 contract, on 72 cases over six kinds and all four transposes: m and n around the
instruction tiles, the wave quarter and the work-group tile, k below the instruction depth, at one and two chunks and with every
tail, three different leading-dimension pads, operands that start at odd element offsets inside their allocations, in device,
pinned and pageable memory, and 1 ... 7 tasks in a drawn order. Every operand lies between canary bands, and the whole allocation
is compared: C with its gaps (NaN where beta = 0) and bands, A and B unchanged. The bf16 fast mode gets the bits of the exact mode
on integer operands, whose partial sums are exact, and its own bound on the drawn bf16 operands. The front ends libxsmm_wigemm /
libxsmm_wsgemm / libxsmm_bsgemm are run at and next to LIBXSMM_MAX_MNK, where they change the layout of A. DESIGN.md 8v."""
import numpy as np
import pytest

import lowp_gemm_common as lg
import tgemm_sweep_common as ts

pytestmark = pytest.mark.gpu

CASES = ts.sweep_cases()
FAST = sorted(name for name, c in CASES.items() if c["kind"] == "bf16fast")
FAST_RATIO = {}


@pytest.fixture(autouse=True)
def keep_mode(xs):
    before = xs.lib().libxsmm_amd_get_lowp_fast()
    yield
    xs.set_lowp_fast(before)


class Placed(object):
    """a copy of an allocation in a memory kind"""

    def __init__(self, torch, alloc, mem):
        self.dtype = alloc.dtype
        src = (alloc.view(np.int16) if alloc.dtype == np.uint16 else alloc).copy()
        self.mem = {"device": lambda: torch.from_numpy(src).cuda(), "pinned": lambda: torch.from_numpy(src).pin_memory(), "pageable": lambda: src}[mem]()

    def ptr(self, elements):
        base = self.mem.data_ptr() if hasattr(self.mem, "data_ptr") else self.mem.ctypes.data
        return base + elements * self.dtype.itemsize

    def read(self):
        return (self.mem.cpu().numpy() if hasattr(self.mem, "cpu") else self.mem).view(self.dtype)


def run(xs, torch, name, ints=False, tasks=None, omp=False):
    """one product of a case on fresh copies of its operands: the tasks in the drawn order (tasks: another list of (tid, nthreads)),
    or libxsmm_xgemm_omp -> the allocations of A, B and C afterwards. A task with work is one launch, one without is none."""
    L = xs.lib()
    case = CASES[name]
    kind, m, n, k, beta = case["kind"], case["m"], case["n"], case["k"], case["beta"]
    ta, tb = case["trans"]
    _, (lda, ldb, ldc) = ts.dims(case)
    placed = [Placed(torch, x, mem) for x, mem in zip(ts.operands(name, ints), case["mem"])]
    pa, pb, pc = (p.ptr(ts.origin(case, w)) for w, p in enumerate(placed))
    fp = kind in ("f32", "f64")
    prec = {"f32": xs.F32, "f64": xs.F64}.get(kind)
    if omp:
        assert fp
        xs.xgemm_omp(prec, ta, tb, m, n, k, 1.0, pa, lda, pb, ldb, float(beta), pc, ldc)
    else:
        keep, h = xs.gemm_handle(prec, prec, ta, tb, m, n, k, lda, ldb, ldc, 1.0, float(beta)) if fp else xs.gemm_handle(xs.F32, xs.F32, "N", "N", m, n, 1)
        assert h
        for tid, nthreads in ([(t, case["nthreads"]) for t in case["order"]] if tasks is None else tasks):
            rc, (m0, m1, n0, n1) = xs.gemm_task(h, tid, nthreads)
            assert rc == 0 and (m0, m1, n0, n1) == ts.task_rect(m, n, tid, nthreads)
            launches = L.libxsmm_amd_launch_count()
            if fp:
                xs.gemm_thread(h, pa, pb, pc, tid, nthreads)
            else:
                ip, op = lg.precisions(xs, ts.LOWP[kind])
                assert 0 == xs.gemm_lowp_thread(ip, op, ta, tb, m, n, k, pa, lda, pb, ldb, beta, pc, ldc, tid, nthreads)
            assert (1 if m0 < m1 else 0) == L.libxsmm_amd_launch_count() - launches, "a task with work is one launch, one without is none"
    assert 0 == L.libxsmm_amd_synchronize()
    torch.cuda.synchronize()
    return [p.read() for p in placed]


def check(name, got, ints=False, c_want=None):
    a, b, c = got
    xa, xb, _ = ts.operands(name, ints)
    assert a.tobytes() == xa.tobytes() and b.tobytes() == xb.tobytes(), "A or B, or a canary band around them, was written"
    want = ts.expected(name, ints) if c_want is None else c_want
    case = CASES[name]
    body = slice(ts.origin(case, 2), c.size - ts.GUARD)
    assert c[:body.start].tobytes() == want[:body.start].tobytes() and c[body.stop:].tobytes() == want[body.stop:].tobytes(), "a canary band of C was written"
    assert c.tobytes() == want.tobytes(), "%d elements of C differ" % int(np.sum(c.view(np.uint8) != want.view(np.uint8)) // c.dtype.itemsize)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_bit_equal(xs, orc, torch_gpu, name):
    case = CASES[name]
    kind, fast = case["kind"], case["kind"] == "bf16fast"
    xs.set_lowp_fast(fast)  # (the fast mode runs the integer operands: there its expectation is the exact mode's bits)
    got = run(xs, torch_gpu, name, ints=fast)
    assert xs.last_kernel() == ts.KERNEL[kind] + case["trans"].lower(), xs.last_kernel()
    check(name, got, ints=fast)
    if kind in ("f32", "f64"):
        again = run(xs, torch_gpu, name, omp=True)
        assert xs.last_kernel() == ts.KERNEL[kind] + case["trans"].lower(), xs.last_kernel()
        check(name, again)
    if fast:  # the exact mode on the same operands, on the GPU as well
        xs.set_lowp_fast(False)
        exact = run(xs, torch_gpu, name, ints=True)
        assert xs.last_kernel() == ts.KERNEL["bf16"] + case["trans"].lower(), xs.last_kernel()
        check(name, exact, ints=True)
        assert exact[2].tobytes() == got[2].tobytes()


@pytest.mark.parametrize("name", FAST)
def test_fast_mode_on_the_drawn_operands(xs, orc, torch_gpu, name):
    """random bf16 in the fast mode: within the bound of tgemm_sweep_common.contract64 -- (k + 1) 2^-23 S, DESIGN.md 8d's model of
    the instruction's adder -- against float64; what lies outside the m x n elements keeps its bytes; the same bits from two calls,
    and from one task and from the drawn tasks."""
    xs.set_lowp_fast(True)
    first = run(xs, torch_gpu, name)
    assert xs.last_kernel() == ts.KERNEL["bf16fast"] + CASES[name]["trans"].lower(), xs.last_kernel()
    second = run(xs, torch_gpu, name)
    single = run(xs, torch_gpu, name, tasks=[(0, 1)])
    FAST_RATIO[name] = ts.ratio_of(name, first[2], fast=True)
    print("%s: fast mode, worst error / bound %.3g" % (name, FAST_RATIO[name]))
    xa, xb, _ = ts.operands(name)
    for a, b, c in (first, second, single):
        assert a.tobytes() == xa.tobytes() and b.tobytes() == xb.tobytes()
        assert c.tobytes() == first[2].tobytes()
    assert ts.compare(name, first[2], fast=True) is None, ts.compare(name, first[2], fast=True)


def test_fast_mode_worst_ratio(torch_gpu):
    """prints the worst error / bound of the fast mode over the cases above (DESIGN.md 8v records it next to 8d's 0.0079)"""
    if FAST_RATIO:
        print("fast mode over %d cases: worst error / bound %.3g (%s)" % (len(FAST_RATIO), max(FAST_RATIO.values()), max(FAST_RATIO, key=FAST_RATIO.get)))
    assert all(v <= 1.0 for v in FAST_RATIO.values())


MAX_MNK = 262144  # LIBXSMM_MAX_MNK (include/libxsmm.h)
AROUND = (("NN", 64, 64, 64), ("NN", 64, 64, 66), ("NN", 66, 64, 64), ("NN", 128, 32, 64), ("NN", 64, 64, 63), ("TN", 64, 64, 64))


@pytest.mark.parametrize("front", ("wigemm", "wsgemm", "bsgemm"))
def test_front_ends_around_max_mnk(xs, orc, torch_gpu, front):
    """the front ends flip the layout of A at m n k <= LIBXSMM_MAX_MNK: the dispatched kernel reads A in pairs of k, the tiled kernel
    reads it plain. Each shape is called once with A plain to learn the route, then on fresh operands with A in the
    layout of that route, and the result is held to the expectation of that layout. Where 8d's table fixes the route it is
    asserted; at 128 x 32 x 64 (at the threshold, m above 64) it is read and printed."""
    torch = torch_gpu
    kind, one = {"wigemm": (0, 1), "wsgemm": (1, 1.0), "bsgemm": (2, 1.0)}[front]
    fe = getattr(xs, front)
    for idx, (trans, m, n, k) in enumerate(AROUND):
        for beta in (1, 0):
            case = lg.Case(kind, trans, m, n, k, beta, pad=3, seed=41 + 10 * idx + kind)

            def call(a):
                da, db, dc = (torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x.copy()).cuda() for x in (a.copy(), case.b.copy(), case.c))
                fe(trans[0], trans[1], m, n, k, one, da, case.lda, db, case.ldb, type(one)(beta), dc, case.ldc)
                torch.cuda.synchronize()
                assert np.array_equal(da.cpu().numpy().view(np.uint16), a) and np.array_equal(db.cpu().numpy().view(np.uint16), case.b)
                return xs.last_kernel(), dc.cpu().numpy()
            route, _ = call(case.a)
            tiled, small = route == lg.NAMES[kind] + trans.lower(), route.startswith("smm_") and route.endswith("_lowp")
            assert tiled != small, route
            if k % 2 or trans != "NN" or m * n * k > MAX_MNK:
                assert tiled, (route, trans, m, n, k)
            elif max(m, n, k) <= 64:
                assert small, (route, trans, m, n, k)
            else:
                print("%s %d x %d x %d beta %d: %s" % (front, m, n, k, beta, route))
            if tiled:
                again, got = call(case.a)
                want = case.gold
            else:
                packed = lg.pack_pairs(case.a, case.lda, m, k)
                again, got = call(packed)
                want = case.c.copy()
                assert 0 == orc.gemm_lowp(kind, 1 if 0 == beta else 0, m, n, k, case.lda, case.ldb, case.ldc, packed, case.b, want, 1.0)
                assert lg.same_bits(want, lg.pairs_gold(kind, 0 == beta, m, n, k, case.lda, case.ldb, case.ldc, packed, case.b, case.c, 1.0))
                assert lg.same_bits(want, case.gold)  # (the same product: the layout of A differs, the chain does not)
            assert again == route
            assert lg.same_bits(got, want), (front, trans, m, n, k, beta, route, int(np.sum(lg.bits(got) != lg.bits(want))))
