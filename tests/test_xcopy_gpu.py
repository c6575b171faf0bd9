"""Matrix copy and transposition on the GPU: libxsmm_matcopy / otrans / itrans, their _thread forms, the dispatched mcopy /
trans kernels, the stack forms of libxsmm_amd.h, operands beyond 4 GiB, and the order of calls inside the defer bracket.

Every result is compared bit for bit with numpy on whole buffers (tests/xcopy_common.py): guards, padding, gaps between items
and the complete input must keep their bits. The shape grid m, n in SIZES is run in full for every typesize and operation;
the leading-dimension paddings (0, +1, +13 on either side) and the base offset (16-byte aligned, one element past) rotate
through all their combinations along the grid, and a smaller set of shapes runs their full cross product."""
import ctypes as C
import itertools
import os
import subprocess
import threading

import numpy as np
import pytest

import xcopy_common as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 16, 31, 32, 33, 63, 64, 65, 100, 257]
LARGE = [(1000, 3), (3, 1000), (2048, 2048), (4097, 1025)]
TYPESIZES = [1, 2, 3, 4, 8, 12, 16, 24, 255]
PADS = [0, 1, 13]
VARIANTS = list(itertools.product(PADS, PADS, (0, 1), (0, 1)))  # ldi pad, ldo pad, offset of in, offset of out
OPS = ["matcopy", "zero", "otrans", "itrans", "otrans_inplace"]


def run_device(xs, torch, op, ts, m, n, pi, po, oi, oo, seed):
    """one case on device memory; returns a message or None"""
    rng = np.random.default_rng(seed)
    if op in ("itrans", "otrans_inplace"):
        a = xc.Stack(ts, m, m, ld=m + pi, off=oi, rng=rng)
        want = xc.expected_itrans(a)
        da = xc.Device(torch, a)
        if op == "itrans":
            xs.itrans(da.ptr(), ts, m, m, a.ld)
        else:
            xs.otrans(da.ptr(), da.ptr(), ts, m, m, a.ld, a.ld)
        return xc.first_difference(da.get(), want)
    src = xc.Stack(ts, m, n, ld=m + pi, off=oi, rng=rng)
    if op == "otrans":
        dst = xc.Stack(ts, n, m, ld=n + po, off=oo, fill=False)
        want = xc.expected_trans(dst, src)
    else:
        dst = xc.Stack(ts, m, n, ld=m + po, off=oo, fill=False)
        want = xc.expected_copy(dst, None if op == "zero" else src)
    di, do = xc.Device(torch, src), xc.Device(torch, dst)
    if op == "otrans":
        xs.otrans(do.ptr(), di.ptr(), ts, m, n, src.ld, dst.ld)
    else:
        xs.matcopy(do.ptr(), None if op == "zero" else di.ptr(), ts, m, n, src.ld, dst.ld, prefetch=(1 if seed % 2 else None))
    return xc.first_difference(do.get(), want) or xc.first_difference(di.get(), src.host)


@pytest.mark.parametrize("ts", TYPESIZES)
@pytest.mark.parametrize("op", OPS)
def test_shape_grid(xs, torch_gpu, op, ts):
    count = 0
    for m in SIZES:
        for n in (SIZES if op in ("matcopy", "zero", "otrans") else [m]):
            pi, po, oi, oo = VARIANTS[count % len(VARIANTS)]
            count += 1
            msg = run_device(xs, torch_gpu, op, ts, m, n, pi, po, oi, oo, count)
            assert msg is None, (op, ts, m, n, pi, po, oi, oo, msg, xs.last_kernel())


@pytest.mark.parametrize("ts", TYPESIZES)
@pytest.mark.parametrize("op", OPS)
def test_leading_dimensions_and_offsets_cross_product(xs, torch_gpu, op, ts):
    for m, n in ((7, 33), (64, 65), (100, 31)):
        for seed, (pi, po, oi, oo) in enumerate(VARIANTS):
            msg = run_device(xs, torch_gpu, op, ts, m, n, pi, po, oi, oo, seed)
            assert msg is None, (op, ts, m, n, pi, po, oi, oo, msg, xs.last_kernel())


@pytest.mark.parametrize("ts", [4, 8])
@pytest.mark.parametrize("shape", LARGE)
def test_large_shapes(xs, torch_gpu, shape, ts):
    m, n = shape
    for seed, (pi, po, oi, oo) in enumerate(((0, 0, 0, 0), (1, 13, 1, 0), (13, 1, 0, 1))):
        for op in OPS:
            if op in ("itrans", "otrans_inplace") and m != n:
                continue
            msg = run_device(xs, torch_gpu, op, ts, m, n, pi, po, oi, oo, seed)
            assert msg is None, (op, ts, m, n, pi, po, oi, oo, msg, xs.last_kernel())


@pytest.mark.parametrize("kind", ["device", "pinned", "pageable"])
def test_memory_kinds_with_pitched_destination(xs, torch_gpu, kind):
    def hold(stack):
        return xc.Device(torch_gpu, stack) if kind == "device" else (xc.Pinned(xs, stack) if kind == "pinned" else None)
    for ts, m, n, pi, po, oi, oo in ((4, 65, 33, 1, 13, 1, 0), (8, 100, 257, 13, 1, 0, 1), (3, 31, 7, 1, 1, 0, 0), (16, 33, 64, 0, 13, 0, 0), (8, 300, 200, 5, 7, 1, 1)):
        rng = np.random.default_rng(ts + m)
        for op in OPS:
            if op in ("itrans", "otrans_inplace"):
                a = xc.Stack(ts, m, m, ld=m + pi, off=oi, rng=rng)
                want, h = xc.expected_itrans(a), hold(a)
                p = h.ptr() if h else a.ptr()
                xs.itrans(p, ts, m, m, a.ld) if op == "itrans" else xs.otrans(p, p, ts, m, m, a.ld, a.ld)
                got = h.get() if h else a.host  # (host memory: complete on return, no synchronisation by the caller)
                assert xc.first_difference(got, want) is None, (kind, op, ts, m)
                continue
            src = xc.Stack(ts, m, n, ld=m + pi, off=oi, rng=rng)
            dst = xc.Stack(ts, n, m, ld=n + po, off=oo, fill=False) if op == "otrans" else xc.Stack(ts, m, n, ld=m + po, off=oo, fill=False)
            want = xc.expected_trans(dst, src) if op == "otrans" else xc.expected_copy(dst, None if op == "zero" else src)
            hi, ho = hold(src), hold(dst)
            pin, pout = (hi.ptr() if hi else src.ptr()), (ho.ptr() if ho else dst.ptr())
            if op == "otrans":
                xs.otrans(pout, pin, ts, m, n, src.ld, dst.ld)
            else:
                xs.matcopy(pout, None if op == "zero" else pin, ts, m, n, src.ld, dst.ld)
            assert xc.first_difference(ho.get() if ho else dst.host, want) is None, (kind, op, ts, m, n, xs.last_kernel())
            assert xc.first_difference(hi.get() if hi else src.host, src.host) is None
        # mixed: pageable input, device output
        src = xc.Stack(ts, m, n, ld=m + pi, off=oi, rng=rng)
        dst = xc.Stack(ts, n, m, ld=n + po, off=oo, fill=False)
        do = xc.Device(torch_gpu, dst)
        xs.otrans(do.ptr(), src.ptr(), ts, m, n, src.ld, dst.ld)
        assert xc.first_difference(do.get(), xc.expected_trans(dst, src)) is None


def test_dispatched_kernels(xs, torch_gpu):
    L = xs.lib()
    keep = []
    for ts, m, n, pi, po in ((8, 23, 17, 1, 2), (4, 64, 64, 0, 0), (12, 9, 31, 3, 0), (16, 33, 5, 0, 13)):
        rng = np.random.default_rng(m)
        src = xc.Stack(ts, m, n, ld=m + pi, rng=rng)
        # transposition kernel: device and host memory, a release, a fresh dispatch
        dst = xc.Stack(ts, n, m, ld=n + po, fill=False)
        keep.append(xs.trans_descriptor(ts, m, n, dst.ld))
        f = xs.trans_dispatch(keep[-1][1])
        assert f
        kind, ti = C.c_int(-1), xs.TransKernelInfo()
        assert 0 == L.libxsmm_get_kernel_kind(f, C.byref(kind)) and kind.value == xs.KIND_TRANS
        assert 0 == L.libxsmm_get_transkernel_info(f, C.byref(ti), None) and (ti.m, ti.n, ti.ldo, ti.typesize) == (m, n, dst.ld, ts)
        want = xc.expected_trans(dst, src)
        for round_ in range(2):
            di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
            xs.call_xcopy_kernel(f, di.ptr(), src.ld, do.ptr(), dst.ld)
            assert xc.first_difference(do.get(), want) is None, ("trans kernel, device", ts, m, n)
            host = xc.Stack(ts, n, m, ld=n + po, fill=False)
            xs.call_xcopy_kernel(f, src.ptr(), src.ld, host.ptr(), host.ld)
            assert xc.first_difference(host.host, want) is None, ("trans kernel, host", ts, m, n)
            L.libxsmm_release_kernel(f)
            keep.append(xs.trans_descriptor(ts, m, n, dst.ld))
            f2 = xs.trans_dispatch(keep[-1][1])
            assert f2 == f
        # matcopy kernels (typesize a multiple of 4): plain, and zero source with a prefetch argument
        dst = xc.Stack(ts, m, n, ld=m + po, fill=False)
        keep.append(xs.mcopy_descriptor(ts, m, n, dst.ld, src.ld))
        g = xs.mcopy_dispatch(keep[-1][1])
        keep.append(xs.mcopy_descriptor(ts, m, n, dst.ld, src.ld, flags=xs.MATCOPY_FLAG_ZERO_SOURCE, prefetch=1))
        z = xs.mcopy_dispatch(keep[-1][1])
        assert g and z and g != z
        mi = xs.McopyKernelInfo()
        assert 0 == L.libxsmm_get_kernel_kind(z, C.byref(kind)) and kind.value == xs.KIND_MCOPY
        assert 0 == L.libxsmm_get_mcopykernel_info(z, C.byref(mi), None)
        assert (mi.typesize, mi.m, mi.n, mi.ldi, mi.ldo, mi.flags) == (4, m * ts // 4, n, src.ld * ts // 4, dst.ld * ts // 4, 1)
        for fn, source, prefetch in ((g, src, False), (z, None, True), (g, src, True)):
            want = xc.expected_copy(dst, source)
            di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
            xs.call_xcopy_kernel(fn, di.ptr(), src.ld, do.ptr(), dst.ld, prefetch=prefetch)  # (a zero-source kernel ignores `in`)
            assert xc.first_difference(do.get(), want) is None, ("mcopy kernel, device", ts, m, n)
            host = xc.Stack(ts, m, n, ld=m + po, fill=False)
            xs.call_xcopy_kernel(fn, src.ptr(), src.ld, host.ptr(), host.ld, prefetch=prefetch)
            assert xc.first_difference(host.host, want) is None, ("mcopy kernel, host", ts, m, n)
        L.libxsmm_release_kernel(g)
        keep.append(xs.mcopy_descriptor(ts, m, n, dst.ld, src.ld))
        assert xs.mcopy_dispatch(keep[-1][1]) == g


@pytest.mark.parametrize("nthreads", [1, 3, 8])
def test_thread_forms(xs, torch_gpu, nthreads):
    rng = np.random.default_rng(nthreads)
    for op, ts, m, n in (("matcopy", 4, 100, 65), ("otrans", 8, 65, 100), ("zero", 3, 7, 5), ("otrans", 2, 5, 33), ("matcopy", 16, 3, 2)):
        src = xc.Stack(ts, m, n, ld=m + 1, rng=rng)
        dst = xc.Stack(ts, n, m, ld=n + 13, fill=False) if op == "otrans" else xc.Stack(ts, m, n, ld=m + 13, fill=False)
        want = xc.expected_trans(dst, src) if op == "otrans" else xc.expected_copy(dst, None if op == "zero" else src)

        def task(pout, pin, tid):
            if op == "otrans":
                xs.otrans(pout, pin, ts, m, n, src.ld, dst.ld, tid=tid, nthreads=nthreads)
            else:
                xs.matcopy(pout, None if op == "zero" else pin, ts, m, n, src.ld, dst.ld, tid=tid, nthreads=nthreads)
        # every task alone: it writes its part only; the parts are disjoint and cover the destination
        written = np.zeros(dst.host.size, dtype=np.int32)
        for tid in range(nthreads):
            di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
            task(do.ptr(), di.ptr(), tid)
            got = do.get()
            changed = got != dst.host
            assert np.array_equal(got[changed], want[changed]), (op, nthreads, tid)  # (what changed, changed to the right bytes)
            written += changed
        should = (want != dst.host)
        assert written.max() <= 1 and np.array_equal(written == 1, should), (op, nthreads)
        # all tasks, shuffled
        di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
        for tid in rng.permutation(nthreads):
            task(do.ptr(), di.ptr(), int(tid))
        assert xc.first_difference(do.get(), want) is None, (op, nthreads, "shuffled")
        # all tasks from concurrent host threads, on device memory and on pageable host memory
        di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
        host = xc.Stack(ts, dst.rows, dst.cols, ld=dst.ld, fill=False)
        for pout, pin in ((do.ptr(), di.ptr()), (host.ptr(), src.ptr())):
            threads = [threading.Thread(target=task, args=(pout, pin, tid)) for tid in range(nthreads)]
            [t.start() for t in threads]; [t.join() for t in threads]
        torch_gpu.cuda.synchronize()
        assert xc.first_difference(do.get(), want) is None, (op, nthreads, "concurrent, device")
        assert xc.first_difference(host.host, want) is None, (op, nthreads, "concurrent, host")


STACK_CASES = [  # typesize, m, n, ldi pad, ldo pad, gap in, gap out, batch
    (4, 1, 1, 0, 0, 0, 0, 1000), (8, 1, 1, 0, 0, 3, 1, 7), (4, 32, 32, 0, 0, 0, 0, 1000), (8, 23, 23, 0, 0, 0, 0, 1000), (8, 13, 13, 1, 2, 5, 3, 1000),
    (4, 64, 64, 0, 0, 0, 0, 7), (8, 64, 64, 1, 1, 0, 7, 7), (16, 64, 64, 0, 0, 0, 0, 7), (4, 5, 40, 0, 3, 2, 0, 1000), (8, 40, 5, 2, 0, 0, 1, 7),
    (2, 17, 9, 1, 0, 1, 1, 1000), (1, 64, 3, 0, 1, 0, 0, 7), (3, 7, 11, 1, 1, 2, 2, 7), (12, 13, 13, 0, 0, 0, 0, 1000), (255, 5, 4, 0, 1, 1, 0, 7),
    (24, 64, 64, 0, 0, 0, 0, 1), (8, 3, 3, 0, 0, 0, 0, 100003), (4, 4, 6, 0, 0, 1, 0, 100003), (8, 100, 70, 0, 3, 0, 0, 7), (4, 1, 64, 0, 0, 0, 0, 1)]


@pytest.mark.parametrize("case", STACK_CASES)
def test_stack_calls(xs, torch_gpu, case):
    ts, m, n, pi, po, gi, go, batch = case
    rng = np.random.default_rng(batch + m)
    src = xc.Stack(ts, m, n, ld=m + pi, stride=(n - 1) * (m + pi) + m + gi, batch=batch, off=1 if gi else 0, rng=rng)
    for op in ("otrans", "matcopy", "zero"):
        rows, cols = (n, m) if op == "otrans" else (m, n)
        dst = xc.Stack(ts, rows, cols, ld=rows + po, stride=(cols - 1) * (rows + po) + rows + go, batch=batch, off=1 if go else 0, fill=False)
        want = xc.expected_trans(dst, src) if op == "otrans" else xc.expected_copy(dst, None if op == "zero" else src)
        strided = xs.otrans_batch if op == "otrans" else xs.matcopy_batch
        byptr = xs.otrans_batch_ptr if op == "otrans" else xs.matcopy_batch_ptr
        di = xc.Device(torch_gpu, src)
        # strided, device memory
        do = xc.Device(torch_gpu, dst)
        assert 0 == strided(do.ptr(), None if op == "zero" else di.ptr(), ts, m, n, src.ld, dst.ld, src.stride, dst.stride, batch)
        assert xc.first_difference(do.get(), want) is None, ("strided", op, case, xs.last_kernel())
        # pointer arrays in host memory and in device memory
        do = xc.Device(torch_gpu, dst)
        hin, hout = di.item_ptrs(), do.item_ptrs()
        assert 0 == byptr(hout, None if op == "zero" else hin, ts, m, n, src.ld, dst.ld, batch)
        assert xc.first_difference(do.get(), want) is None, ("host pointers", op, case, xs.last_kernel())
        do = xc.Device(torch_gpu, dst)
        din = torch_gpu.from_numpy(di.item_ptrs().view(np.int64)).cuda()
        dout = torch_gpu.from_numpy(do.item_ptrs().view(np.int64)).cuda()
        assert 0 == byptr(dout, None if op == "zero" else din, ts, m, n, src.ld, dst.ld, batch)
        assert xc.first_difference(do.get(), want) is None, ("device pointers", op, case, xs.last_kernel())
        assert xc.first_difference(di.get(), src.host) is None
        if batch <= 1000:  # strided, pageable host memory: the gaps keep their bytes as well
            host = xc.Stack(ts, rows, cols, ld=dst.ld, stride=dst.stride, batch=batch, off=dst.off, fill=False)
            assert 0 == strided(host.ptr(), None if op == "zero" else src.ptr(), ts, m, n, src.ld, dst.ld, src.stride, dst.stride, batch)
            assert xc.first_difference(host.host, want) is None, ("strided, host", op, case)
    if m == n:  # in place: every item onto itself
        want = xc.expected_itrans(src)
        da = xc.Device(torch_gpu, src)
        assert 0 == xs.otrans_batch(da.ptr(), da.ptr(), ts, m, n, src.ld, src.ld, src.stride, src.stride, batch)
        assert xc.first_difference(da.get(), want) is None, ("in place", case, xs.last_kernel())
        da = xc.Device(torch_gpu, src)
        ptrs = torch_gpu.from_numpy(da.item_ptrs().view(np.int64)).cuda()
        assert 0 == xs.otrans_batch_ptr(ptrs, ptrs, ts, m, n, src.ld, src.ld, batch)
        assert xc.first_difference(da.get(), want) is None, ("in place, pointers", case, xs.last_kernel())


def test_stack_calls_empty_and_failing(xs, torch_gpu):
    src = xc.Stack(4, 8, 6, ld=9, batch=5)
    dst = xc.Stack(4, 6, 8, ld=7, batch=5, fill=False)
    di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
    launches = xs.lib().libxsmm_amd_launch_count()
    assert 0 == xs.otrans_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 7, src.stride, dst.stride, 0)
    assert 0 == xs.matcopy_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 9, src.stride, dst.stride, 0)
    assert 0 == xs.otrans_batch_ptr(do.item_ptrs(), di.item_ptrs(), 4, 8, 6, 9, 7, 0)
    assert 0 != xs.otrans_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 7, src.stride, dst.stride, -1)
    assert 0 != xs.otrans_batch(do.ptr(), di.ptr(), 4, 8, 6, 7, 7, src.stride, dst.stride, 5)        # m > ldi
    assert 0 != xs.otrans_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 5, src.stride, dst.stride, 5)        # n > ldo
    assert 0 != xs.otrans_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 7, src.stride, dst.extent - 1, 5)    # items of out overlap
    assert 0 != xs.matcopy_batch(do.ptr(), di.ptr(), 4, 8, 6, 9, 7, src.stride, dst.stride, 5)       # m > ldo
    assert 0 != xs.otrans_batch(di.ptr(), di.ptr(), 4, 8, 6, 9, 9, src.stride, src.stride, 5)        # in place, not square
    assert 0 != xs.matcopy_batch(di.ptr(), di.ptr(), 4, 8, 6, 9, 9, src.stride, src.stride, 5)       # out == in
    assert 0 != xs.otrans_batch(None, di.ptr(), 4, 8, 6, 9, 7, src.stride, dst.stride, 5)
    assert 0 != xs.otrans_batch_ptr(do.item_ptrs(), None, 4, 8, 6, 9, 7, 5)
    assert 0 != xs.otrans_batch(do.ptr(), di.ptr(), 0, 8, 6, 9, 7, src.stride, dst.stride, 5)
    assert xs.lib().libxsmm_amd_launch_count() == launches
    assert xc.first_difference(do.get(), dst.host) is None and xc.first_difference(di.get(), src.host) is None


def test_operands_beyond_4gib(xs, torch_gpu):
    """typesize 8, 23 200 x 23 200 with padded leading dimensions: 4.3 GB per operand, produced and compared on the device"""
    torch = torch_gpu
    n, ldi, ldo = 23200, 23208, 23213
    canary = -0x0123456789ABCDEF
    a = torch.randint(-2 ** 62, 2 ** 62, (n, ldi), dtype=torch.int64, device="cuda")  # a[j, i]: element (i, j), column major
    assert a.numel() * 8 > 2 ** 32
    a[0, 0] = 0x7FF4DEADBEEF0BAD
    a[n - 1, n - 1] = -2 ** 63
    keep = a.clone()
    for op in ("otrans", "matcopy"):
        b = torch.full((n, ldo), canary, dtype=torch.int64, device="cuda")
        if op == "otrans":
            xs.otrans(b.data_ptr(), a.data_ptr(), 8, n, n, ldi, ldo)
        else:
            xs.matcopy(b.data_ptr(), a.data_ptr(), 8, n, n, ldi, ldo)
        torch.cuda.synchronize()
        for r0 in range(0, n, 2048):  # in slabs: no second copy of the whole array
            r1 = min(n, r0 + 2048)
            want = a[:n, r0:r1].t() if op == "otrans" else a[r0:r1, :n]
            assert torch.equal(b[r0:r1, :n], want), (op, r0)
            assert bool((b[r0:r1, n:] == canary).all()), (op, r0, "padding")
        del b
    assert torch.equal(a, keep)
    # in place, the same size
    xs.itrans(a.data_ptr(), 8, n, n, ldi)
    torch.cuda.synchronize()
    for r0 in range(0, n, 2048):
        r1 = min(n, r0 + 2048)
        assert torch.equal(a[r0:r1, :n], keep[:n, r0:r1].t()), ("itrans", r0)
        assert torch.equal(a[r0:r1, n:], keep[r0:r1, n:])


def test_call_order_inside_the_defer_bracket(xs, torch_gpu):
    """kernel -> otrans of its C -> kernel that reads the transposed C; gemm_batch -> stack transposition -> gemm_batch:
    inside libxsmm_amd_defer_begin/end the results equal those of the same calls outside (the copy calls seal the open burst)"""
    torch = torch_gpu
    L = xs.lib()
    m = 16
    rng = np.random.default_rng(3)
    host = [rng.uniform(-1, 1, m * m) for _ in range(5)]
    fn = L.libxsmm_dmmdispatch(m, m, m, None, None, None, None, None, None, None)
    assert fn

    def single(bracket):
        a, b, c, ct, d = (torch.from_numpy(x.copy()).cuda() for x in host)
        if bracket:
            xs.defer_begin()
        xs.call_kernel(fn, a, b, c)                                  # c += a * b
        xs.otrans(ct.data_ptr(), c.data_ptr(), 8, m, m, m, m)        # ct = c^T
        xs.call_kernel(fn, ct, b, d)                                 # d += ct * b
        xs.itrans(d.data_ptr(), 8, m, m, m)
        xs.call_kernel(fn, d, a, c)                                  # c += d * a
        if bracket:
            xs.defer_end()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (c, ct, d)]
    plain, deferred = single(False), single(True)
    for x, y in zip(plain, deferred):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert not np.array_equal(plain[1], host[3])

    batch = 300
    stacks = [rng.uniform(-1, 1, batch * m * m) for _ in range(4)]
    stride = (np.arange(batch, dtype=np.int32) * m * m)

    def stacked(bracket):
        a, b, c, ct = (torch.from_numpy(x.copy()).cuda() for x in stacks)
        s = torch.from_numpy(stride).cuda()
        if bracket:
            xs.defer_begin()
        xs.gemm_batch(xs.F64, "N", "N", m, m, m, 1.0, a, m, b, m, 1.0, c, m, 0, 4, s, s, s, batch)
        assert 0 == xs.otrans_batch(ct.data_ptr(), c.data_ptr(), 8, m, m, m, m, m * m, m * m, batch)
        xs.gemm_batch(xs.F64, "N", "N", m, m, m, 1.0, ct, m, b, m, 1.0, a, m, 0, 4, s, s, s, batch)
        if bracket:
            xs.defer_end()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (a, c, ct)]
    plain, deferred = stacked(False), stacked(True)
    for x, y in zip(plain, deferred):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.array_equal(plain[2].reshape(batch, m, m), plain[1].reshape(batch, m, m).transpose(0, 2, 1))


def test_example_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "xcopy_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "xcopy_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "xcopy_caller: ok" in res.stdout
