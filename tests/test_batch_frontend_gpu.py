"""Branches of the batch front end (csrc/xsmm_batch.cpp: batch_execute, lowp_batch_execute; csrc/xsmm_call.cpp) that no other
test reaches: a wide index stride together with index_base 1, task slices over host arrays of pointers (a batch that does not
divide evenly, more tasks than items), arrays of pointers in memory the CPU addresses as well, low-precision batches with
device index arrays, and the error returns. Batches of 7 whose C blocks repeat in consecutive runs only: every path is
order-deterministic, so the scalar-FMA kernels must equal the oracle's k-ordered fma chain bit for bit (as tests/test_smm_gpu.py).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH = 7
RUNS = np.array([0, 0, 1, 2, 2, 2, 3])      # the C block of every item: a repeated C first, in the middle, a single one last
SHAPES = [(5, 4, 3), (23, 23, 23)]
DTYPES = [np.float32, np.float64]


class Case:
    """operands of one batch (tight matrices, A and B shuffled), its element offsets and the oracle's result"""

    def __init__(self, orc, dtype, shape, blocks, beta0=False):
        m, n, k = shape
        self.m, self.n, self.k, self.dtype, self.ts = m, n, k, dtype, np.dtype(dtype).itemsize
        rng = np.random.default_rng(100 * m + 10 * n + k + self.ts)
        self.a = rng.uniform(-1, 1, BATCH * m * k).astype(dtype); self.b = rng.uniform(-1, 1, BATCH * k * n).astype(dtype)
        self.c = rng.uniform(-1, 1, (int(blocks.max()) + 1) * m * n).astype(dtype)
        self.ea = (rng.permutation(BATCH) * m * k).astype(np.int32); self.eb = (rng.permutation(BATCH) * k * n).astype(np.int32)
        self.ec = (blocks * m * n).astype(np.int32)
        self.ref = self.c.copy()
        assert 0 == orc.gemm_batch_idx(orc.FMA, orc.FLAG_BETA_0 if beta0 else 0, m, n, k, m, k, m, self.a, self.b, self.ref, 0, self.ea, self.eb, self.ec, BATCH)

    def pointers(self, base_a, base_b, base_c):
        return tuple((base + e.astype(np.uint64) * np.uint64(self.ts)).astype(np.uint64) for base, e in ((base_a, self.ea), (base_b, self.eb), (base_c, self.ec)))


@pytest.fixture(scope="module")
def cases(orc):
    made = {}

    def get(dtype, shape, distinct=False):
        key = (dtype, shape, distinct)
        if key not in made:
            made[key] = Case(orc, dtype, shape, np.arange(BATCH) if distinct else RUNS)
        return made[key]
    return get


@pytest.fixture
def scalar_fma(xs):
    old = xs.lib().libxsmm_amd_set_mfma(0)
    yield
    xs.lib().libxsmm_amd_set_mfma(old)


def spaced(values, step, base=0):
    """values + base, `step` 4-byte (int32) or 8-byte (pointer) slots apart: what a caller's array of structs looks like"""
    out = np.zeros(len(values) * step, dtype=values.dtype)
    out[::step] = values + values.dtype.type(base)
    return out


@pytest.mark.parametrize("where", ["device", "device_host_indexes", "pageable"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_index_stride_with_index_base_one(xs, cases, torch_gpu, scalar_fma, dtype, shape, where):
    """index arrays of 4-byte indexes 8 bytes apart, counted from 1 (src/libxsmm_gemm.c:1333-1364): device matrices with device and
    with host index arrays, and everything in pageable memory (the staged element ranges start at the lowest index)"""
    torch = torch_gpu
    t = cases(dtype, shape)
    prec = xs.F64 if dtype == np.float64 else xs.F32
    ia, ib, ic = (spaced(e, 2, 1) for e in (t.ea, t.eb, t.ec))
    launches = xs.lib().libxsmm_amd_launch_count()
    if where == "pageable":
        out = t.c.copy()
        xs.gemm_batch(prec, "N", "N", t.m, t.n, t.k, 1.0, t.a, t.m, t.b, t.k, 1.0, out, t.m, 1, 8, ia, ib, ic, BATCH)
    else:
        da, db, dc = (torch.from_numpy(x).cuda() for x in (t.a, t.b, t.c))
        if where == "device":
            ia, ib, ic = (torch.from_numpy(x).cuda() for x in (ia, ib, ic))
        xs.gemm_batch(prec, "N", "N", t.m, t.n, t.k, 1.0, da, t.m, db, t.k, 1.0, dc, t.m, 1, 8, ia, ib, ic, BATCH)
        torch.cuda.synchronize()
        out = dc.cpu().numpy()
    assert xs.last_kernel().startswith("smm_"), xs.last_kernel()
    assert 1 == xs.lib().libxsmm_amd_launch_count() - launches  # (the C-ordering check is not counted: one multiply)
    assert np.array_equal(out, t.ref), xs.last_kernel()


@pytest.mark.parametrize("where", ["device", "pageable"])
@pytest.mark.parametrize("ntasks", [3, 9])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_task_slices_over_host_pointer_arrays(xs, cases, torch_gpu, scalar_fma, dtype, shape, ntasks, where):
    """libxsmm_mmbatch(..., tid, ntasks) over host arrays of pointers 16 bytes apart with index_base 1 (the reference's byte
    step, src/libxsmm_gemm.c:1426-1428): 7 items on 3 tasks (3 + 3 + 1) and on 9 tasks (the last two get nothing). Pageable
    matrices: staged slice by slice, C repeats in runs that cross the slices. Device matrices: every item its own C and a
    negative batchsize (the caller's promise), so no update of C needs an atomic."""
    torch = torch_gpu
    L = xs.lib()
    t = cases(dtype, shape, distinct=(where == "device"))
    prec = xs.F64 if dtype == np.float64 else xs.F32
    ct = C.c_double if dtype == np.float64 else C.c_float
    one = ct(1.0)
    if where == "pageable":
        out = t.c.copy()
        pa, pb, pc = t.pointers(t.a.ctypes.data, t.b.ctypes.data, out.ctypes.data)
    else:
        da, db, dc = (torch.from_numpy(x).cuda() for x in (t.a, t.b, t.c))
        pa, pb, pc = t.pointers(da.data_ptr(), db.data_ptr(), dc.data_ptr())
    pa, pb, pc = (spaced(x, 2) for x in (pa, pb, pc))
    step = np.array([24], dtype=np.int32)  # minus index_base * sizeof(void*): 16 bytes from pointer to pointer
    launches = L.libxsmm_amd_launch_count()
    for tid in range(ntasks):
        L.libxsmm_mmbatch(prec, prec, b"N", b"N", t.m, t.n, t.k, C.byref(one), pa.ctypes.data, None, pb.ctypes.data, None, C.byref(one), pc.ctypes.data, None,
                          1, 0, step.ctypes.data, step.ctypes.data, step.ctypes.data, -BATCH if where == "device" else BATCH, tid, ntasks)
    if where == "device":
        torch.cuda.synchronize()
        out = dc.cpu().numpy()
    assert xs.last_kernel().startswith("smm_"), xs.last_kernel()
    assert min(ntasks, BATCH) == L.libxsmm_amd_launch_count() - launches  # one multiply per slice that has items
    assert np.array_equal(out, t.ref), xs.last_kernel()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pointer_arrays_and_matrices_in_pinned_memory(xs, cases, torch_gpu, scalar_fma, dtype, shape):
    """arrays of pointers and matrices in libxsmm_malloc memory (the GPU works on it in place, the CPU reads it): the call looks
    behind the arrays, so C is complete when it returns -- it is read here without any synchronisation"""
    L = xs.lib()
    t = cases(dtype, shape)
    prec = xs.F64 if dtype == np.float64 else xs.F32
    bufs = []
    for x in (t.a, t.b, t.c):
        ptr = L.libxsmm_malloc(x.nbytes); assert ptr
        C.memmove(ptr, x.ctypes.data, x.nbytes); bufs.append(ptr)
    arrays = []
    for x in t.pointers(*bufs):
        ptr = L.libxsmm_malloc(x.nbytes); assert ptr
        C.memmove(ptr, x.ctypes.data, x.nbytes); arrays.append(ptr)
    eight = np.array([8], dtype=np.int32)
    xs.gemm_batch(prec, "N", "N", t.m, t.n, t.k, 1.0, arrays[0], t.m, arrays[1], t.k, 1.0, arrays[2], t.m, 0, 0, eight, eight, eight, BATCH)
    out = np.frombuffer((C.c_char * t.c.nbytes).from_address(bufs[2]), dtype=dtype).copy()
    kernel = xs.last_kernel()
    for ptr in bufs + arrays:
        L.libxsmm_free(ptr)
    assert kernel.startswith("smm_"), kernel
    assert np.array_equal(out, t.ref), kernel


def _bf16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("kind", [0, 2])
def test_low_precision_batch_with_device_index_arrays(xs, orc, torch_gpu, kind):
    """libxsmm_mmbatch_kernel on a kernel of 16-bit inputs with index arrays that live in device memory (tests/test_lowp.py passes
    host arrays), index_base 1, every item its own C: the gold loop (samples/xgemm/kernel.c) bit for bit"""
    torch = torch_gpu
    L = xs.lib()
    m, n, k = 16, 12, 24
    rng = np.random.default_rng(40 + kind)
    if kind == 0:
        a = rng.integers(-300, 300, BATCH * m * k).astype(np.int16).view(np.uint16); b = rng.integers(-300, 300, BATCH * k * n).astype(np.int16).view(np.uint16)
        c = rng.integers(-1000, 1000, BATCH * m * n).astype(np.int32)
    else:
        a = _bf16(rng.uniform(-1, 1, BATCH * m * k)); b = _bf16(rng.uniform(-1, 1, BATCH * k * n)); c = rng.uniform(-1, 1, BATCH * m * n).astype(np.float32)
    pa, pb = rng.permutation(BATCH), rng.permutation(BATCH)
    ref = c.copy()
    for i in range(BATCH):
        assert 0 == orc.gemm_lowp(kind, 0, m, n, k, m, k, m, a[pa[i] * m * k:(pa[i] + 1) * m * k], b[pb[i] * k * n:(pb[i] + 1) * k * n], ref[i * m * n:(i + 1) * m * n], 1.0)
    fn = getattr(L, {0: "libxsmm_wimmdispatch", 2: "libxsmm_bsmmdispatch"}[kind])(m, n, k, None, None, None, None, None, None, None)
    assert fn
    da, db = (torch.from_numpy(x.view(np.int16)).cuda() for x in (a, b)); dc = torch.from_numpy(c).cuda()
    sa, sb, sc = (torch.from_numpy((e + 1).astype(np.int32)).cuda() for e in (pa * m * k, pb * k * n, np.arange(BATCH) * m * n))
    launches = L.libxsmm_amd_launch_count()
    assert 0 == L.libxsmm_mmbatch_kernel(C.c_void_p(fn), 1, 4, xs.dptr(sa), xs.dptr(sb), xs.dptr(sc), da.data_ptr(), db.data_ptr(), dc.data_ptr(), BATCH, 0, 1, 2, 4, 0)
    torch.cuda.synchronize()
    assert xs.last_kernel().endswith("_lowp"), xs.last_kernel()
    assert 1 == L.libxsmm_amd_launch_count() - launches
    assert np.array_equal(dc.cpu().numpy().view(np.uint8), ref.view(np.uint8))


def test_error_returns_launch_nothing_and_leave_c_alone(xs, cases, torch_gpu, capfd):
    """what the front end cannot serve is an error, never a launch: pageable matrices with index arrays in device memory, and
    low-precision batches (index arrays, arrays of pointers, batch-reduce) whose matrices the GPU does not reach"""
    torch = torch_gpu
    L = xs.lib()
    t = cases(np.float64, (5, 4, 3))
    fn = L.libxsmm_dmmdispatch(t.m, t.n, t.k, None, None, None, None, None, None, None)
    assert fn
    out = t.c.copy()
    ia, ib, ic = (torch.from_numpy(e).cuda() for e in (t.ea, t.eb, t.ec))
    launches = L.libxsmm_amd_launch_count()
    assert 1 == L.libxsmm_mmbatch_kernel(C.c_void_p(fn), 0, 4, xs.dptr(ia), xs.dptr(ib), xs.dptr(ic), t.a.ctypes.data, t.b.ctypes.data, out.ctypes.data, BATCH, 0, 1, 8, 8, 0)
    assert "host matrices with device index arrays are not supported" in capfd.readouterr().err
    assert np.array_equal(out, t.c)
    # low precision: nothing is staged
    m, n, k = 16, 12, 24
    a = _bf16(np.linspace(-1, 1, BATCH * m * k)); b = _bf16(np.linspace(1, -1, BATCH * k * n)); c = np.linspace(-2, 2, BATCH * m * n).astype(np.float32)
    out = c.copy()
    lowp = L.libxsmm_bsmmdispatch(m, n, k, None, None, None, None, None, None, None)
    assert lowp
    idx = [(np.arange(BATCH) * size).astype(np.int32) for size in (m * k, k * n, m * n)]
    assert 1 == L.libxsmm_mmbatch_kernel(C.c_void_p(lowp), 0, 4, xs.dptr(idx[0]), xs.dptr(idx[1]), xs.dptr(idx[2]), a.ctypes.data, b.ctypes.data, out.ctypes.data, BATCH, 0, 1, 2, 4, 0)
    assert "batches of low-precision products need operands the GPU can reach" in capfd.readouterr().err
    ptrs = [(x.ctypes.data + e.astype(np.uint64) * np.uint64(x.itemsize)).astype(np.uint64) for x, e in zip((a, b, out), idx)]
    eight = np.array([8], dtype=np.int32)
    assert 1 == L.libxsmm_mmbatch_kernel(C.c_void_p(lowp), 0, 0, xs.dptr(eight), xs.dptr(eight), xs.dptr(eight), xs.dptr(ptrs[0]), xs.dptr(ptrs[1]), xs.dptr(ptrs[2]), BATCH, 0, 1, 2, 4, 0)
    assert "batches of low-precision products need operands the GPU can reach" in capfd.readouterr().err
    L.libxsmm_bsmmdispatch_reducebatch.restype = C.c_void_p; L.libxsmm_bsmmdispatch_reducebatch.argtypes = [C.c_int] * 3 + [C.c_void_p] * 7
    reduce = L.libxsmm_bsmmdispatch_reducebatch(m, n, k, None, None, None, None, None, None, None)
    assert reduce
    dc = torch.from_numpy(c[:m * n].copy()).cuda()
    xs.call_kernel(reduce, ptrs[0], ptrs[1], dc, np.array([BATCH], dtype=np.uint64))  # device C, host arrays of pointers to pageable A and B
    assert "low-precision batch-reduce kernels need matrices the GPU can reach" in capfd.readouterr().err
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy(), c[:m * n]) and np.array_equal(out, c)
    assert launches == L.libxsmm_amd_launch_count()
