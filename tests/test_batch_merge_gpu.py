"""Batch calls inside a libxsmm_amd_defer_begin/end bracket (GPU): a caller's loop of libxsmm_gemm_batch calls, one per shape
(samples/cp2k/cp2k.cpp:328-360), is recorded and leaves as fused launches -- segments of calls that are independent of each
other, in call order (include/libxsmm_amd.h; csrc/xsmm_batch_record.cpp: record_batch_call / batch_flush_record; the address hulls of
calls whose arrays live in device memory: csrc/kernels/batch_hull.hip).

Every case issues the same sequence of calls twice, on fresh copies of the operands: outside the bracket (a launch per call, as
always) and inside. The two results must be equal BIT FOR BIT; where the sums are sequential chains (fp64, and fp32 on the scalar
kernels) both must equal the oracle's sequential program bit for bit as well, as in tests/test_grouped_mixed_gpu.py.

All operands of a case live in one pool, calls address it through index arrays (or arrays of pointers into it): a call that reads
what another one wrote is then simply a call whose A indexes point into the other one's C region.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FLUSH_BOUND = 64  # recorded calls after which the record is flushed (include/libxsmm_amd.h)


class _Jit:
    """small test batches on the run-time specialised kernels (the fused launch is one of them), matrix cores on or off"""
    def __init__(self, xs, mfma=1):
        self.xs = xs; self.mfma = mfma

    def __enter__(self):
        self.old_env = os.environ.get("LIBXSMM_AMD_JIT_MINBATCH")
        os.environ["LIBXSMM_AMD_JIT_MINBATCH"] = "1"
        self.old = self.xs.lib().libxsmm_amd_set_mfma(self.mfma)

    def __exit__(self, *exc):
        self.xs.lib().libxsmm_amd_set_mfma(self.old)
        if self.old_env is None:
            del os.environ["LIBXSMM_AMD_JIT_MINBATCH"]
        else:
            os.environ["LIBXSMM_AMD_JIT_MINBATCH"] = self.old_env


class Pool:
    """operands of a case, back to back (with a gap in front of each region: touching regions would still be independent)"""
    def __init__(self, dtype, seed):
        self.dtype = dtype; self.rng = np.random.default_rng(seed); self.parts = []; self.size = 0

    def alloc(self, n):
        self.parts.append(self.rng.uniform(-1, 1, n + 5).astype(self.dtype))
        off = self.size + 5
        self.size += n + 5
        return off

    def data(self):
        return np.concatenate(self.parts)


class Call:
    def __init__(self, shape, ia, ib, ic, transb="N", ldb=None, alpha=1.0, beta=1.0):
        self.m, self.n, self.k = shape
        self.ia, self.ib, self.ic = (None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (ia, ib, ic))
        self.transb = transb; self.alpha = alpha; self.beta = beta
        self.ldb = ldb if ldb is not None else (self.n if transb == "T" else self.k)
        self.size = len(self.ia)

    def spans(self):
        m, n, k = self.m, self.n, self.k
        return ((k - 1) * m + m, (self.ldb * (k - 1) + n) if self.transb == "T" else (self.ldb * (n - 1) + k), (n - 1) * m + m)

    def hull(self, base, ts):
        out = []
        for idx, span in zip((self.ia, self.ib, self.ic), self.spans()):
            out += [base + int(idx.min()) * ts, base + (int(idx.max()) + span) * ts]
        return tuple(out)


def stack(pool, shape, s, run, transb="N", perm=True):
    """a CP2K-style stack: s products, every `run` consecutive ones into one C block; returns (call, (a, b, c) region offsets)"""
    m, n, k = shape
    nc = (s + run - 1) // run
    oa, ob, oc = pool.alloc(s * m * k), pool.alloc(s * k * n), pool.alloc(nc * m * n)
    i = np.arange(s)
    ia = oa + (pool.rng.permutation(s) if perm else i) * m * k
    return Call(shape, ia, ob + i * k * n, oc + (i // run) * m * n, transb=transb), (oa, ob, oc)


def oracle(orc, data, calls):
    ref = data.copy()
    for c in calls:
        assert c.alpha == 1.0 and c.beta == 1.0
        flags = orc.FLAG_TRANS_B if c.transb == "T" else 0
        assert 0 == orc.gemm_batch_idx(orc.FMA, flags, c.m, c.n, c.k, c.m, c.ldb, c.m, ref, ref, ref, 0, c.ia, c.ib, c.ic, c.size)
    return ref


def issue(xs, torch, dev, c, where, mode, keep, scribble=False):
    """one libxsmm_gemm_batch call on the pool `dev`; where: 'device' / 'host' arrays; mode: 'index' / 'pointer'"""
    prec = xs.F64 if dev.dtype == torch.float64 else xs.F32
    ts = dev.element_size()
    if mode == "index":
        arrays = [x.copy() for x in (c.ia, c.ib, c.ic)]
        base, stride, strides = (dev, dev, dev), 4, None
    else:
        arrays = [(dev.data_ptr() + x.astype(np.int64) * ts).astype(np.uint64) for x in (c.ia, c.ib, c.ic)]
        eight = np.array([8], dtype=np.int32)
        base, stride, strides = None, 0, (eight, eight, eight)
    if where == "device":
        arrays = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in arrays]
    keep.append(arrays)  # (device arrays are read at the flush: they stay alive)
    if mode == "index":
        xs.gemm_batch(prec, "N", c.transb, c.m, c.n, c.k, c.alpha, dev, c.m, dev, c.ldb, c.beta, dev, c.m, 0, stride, arrays[0], arrays[1], arrays[2], c.size)
    else:
        xs.gemm_batch(prec, "N", c.transb, c.m, c.n, c.k, c.alpha, arrays[0], c.m, arrays[1], c.ldb, c.beta, arrays[2], c.m, 0, 0,
                      strides[0], strides[1], strides[2], c.size)
    if scribble:  # the caller reuses its buffers: indexes / pointers that are in range, but not the ones that were passed
        assert where == "host"
        for x in arrays:
            x[:] = x[0]


def run(xs, torch, data, calls, bracket, where="device", mode="index", scribble=False):
    """the calls in order on a fresh copy of the pool; returns (result, launches, last kernel, plan of the last flush or None, address of the pool)"""
    L = xs.lib()
    dev = torch.from_numpy(data.copy()).cuda()
    keep = []
    torch.cuda.synchronize()
    before = L.libxsmm_amd_launch_count()
    if bracket:
        xs.defer_begin()
    for c in calls:
        issue(xs, torch, dev, c, where, mode, keep, scribble)
    if bracket:
        xs.defer_end()
    launches = L.libxsmm_amd_launch_count() - before
    kernel = xs.last_kernel()
    torch.cuda.synchronize()
    return dev.cpu().numpy(), launches, kernel, (xs.merge_last_plan() if bracket else None), dev.data_ptr()


def bits(x):
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def show(label, **figures):
    print("[batch merge] %s: %s" % (label, ", ".join("%s=%s" % kv for kv in figures.items())))


# ---- 1. the CP2K loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
def test_cp2k_loop_inside_the_bracket_is_one_fused_launch(xs, orc, torch_gpu, where):
    """all 27 shapes of {13, 23, 32}^3, fp64, beta 1, C blocks repeating inside a shape, disjoint between shapes: one call per shape.
    Outside the bracket a launch per shape; inside at most three launches (hull, C-order check, multiplication), the last one the
    grouped form. Device index arrays: the hulls come from the hull kernel (and equal the ones computed here); host arrays: from the host."""
    torch = torch_gpu
    pool = Pool(np.float64, 2718)
    calls = []
    for gi, shape in enumerate((m, n, k) for m in (13, 23, 32) for n in (13, 23, 32) for k in (13, 23, 32)):
        s = 1500 + 37 * gi
        calls.append(stack(pool, shape, s, max(1, math.isqrt(s * 160 // 240)))[0])
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs):
        plain, launches_plain, kernel_plain, _, _ = run(xs, torch, data, calls, False, where)
        got, launches, kernel, plan, base = run(xs, torch, data, calls, True, where)
    show("cp2k loop, %s index arrays" % where, launches_plain=launches_plain, launches_bracket=launches, kernel_plain=kernel_plain, kernel=kernel,
         segments=plan["segments"], device_hulls=plan["device_hulls"], differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert launches_plain >= 27
    assert launches <= 3
    assert kernel == "smm_f64_jit_shape_runs_grouped", kernel
    assert plan["calls"] == 27 and plan["segments"] == 1
    assert plan["device_hulls"] == (27 if where == "device" else 0)
    assert plan["hulls"] == [c.hull(base, 8) for c in calls]
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


# ---- 2. dependent calls keep their order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
def test_dependent_calls_keep_their_order(xs, orc, torch_gpu, where):
    """call 1 reads as A the C of call 0; call 2 is independent; call 3 updates the C of call 0 again with another k"""
    torch = torch_gpu
    pool = Pool(np.float64, 31)
    m = n = k = 16
    s = 400
    c0, (_, _, oc0) = stack(pool, (m, n, k), s, 1)
    ob1, oc1 = pool.alloc(s * k * n), pool.alloc(s * m * n)
    i = np.arange(s)
    c1 = Call((m, n, k), oc0 + i[::-1] * m * n, ob1 + i * k * n, oc1 + (i // 4) * m * n)  # A = the C blocks of call 0, back to front
    c2, _ = stack(pool, (13, 13, 13), 300, 5)
    k3 = 24
    oa3, ob3 = pool.alloc(s * m * k3), pool.alloc(s * k3 * n)
    c3 = Call((m, n, k3), oa3 + i * m * k3, ob3 + i * k3 * n, oc0 + i * m * n)
    calls = [c0, c1, c2, c3]
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs):
        plain, _, _, _, _ = run(xs, torch, data, calls, False, where)
        got, launches, kernel, plan, base = run(xs, torch, data, calls, True, where)
    nseg, seg = xs.merge_segments(plan["hulls"])
    show("dependent calls, %s arrays" % where, launches=launches, kernel=kernel, segments=plan["segments"], segment_of=plan["segment_of"],
         differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 4 and plan["hulls"] == [c.hull(base, 8) for c in calls]
    assert nseg >= 3 and plan["segments"] == nseg and plan["segment_of"] == seg == [0, 1, 1, 2]
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


# ---- 3. host arrays are snapshotted -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["index", "pointer"])
def test_host_arrays_are_copied_at_the_call(xs, orc, torch_gpu, mode):
    """after every recorded call the caller overwrites its index (pointer) arrays with entries that are in range but wrong"""
    torch = torch_gpu
    pool = Pool(np.float64, 5)
    calls = [stack(pool, shape, s, run)[0] for shape, s, run in (((13, 13, 13), 500, 7), ((23, 23, 23), 300, 1), ((32, 13, 23), 200, 200), ((5, 7, 3), 90, 4))]
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs):
        plain, _, _, _, _ = run(xs, torch, data, calls, False, "host", mode)
        got, launches, kernel, plan, _ = run(xs, torch, data, calls, True, "host", mode, scribble=True)
    show("host %s arrays overwritten after the call" % mode, launches=launches, kernel=kernel, segments=plan["segments"],
         differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 4 and plan["segments"] == 1 and plan["device_hulls"] == 0
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


# ---- 4. arrays of pointers in device memory, one group with B transposed ----------------------------------------------------------------
def test_device_pointer_arrays_with_a_transposed_group(xs, orc, torch_gpu):
    """three shapes through arrays of pointers that live in device memory (the hull kernel's pointer mode); the 23^3 group with
    TRANS_B is not eligible for the matrix-core run form, the other two are: the fused launch mixes the forms"""
    torch = torch_gpu
    pool = Pool(np.float64, 77)
    calls = [stack(pool, (13, 13, 13), 700, 9)[0], stack(pool, (23, 23, 23), 600, 6, transb="T")[0], stack(pool, (32, 32, 32), 500, 11)[0]]
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs):
        plain, launches_plain, _, _, _ = run(xs, torch, data, calls, False, "device", "pointer")
        got, launches, kernel, plan, base = run(xs, torch, data, calls, True, "device", "pointer")
    show("device pointer arrays", launches_plain=launches_plain, launches=launches, kernel=kernel, segments=plan["segments"],
         device_hulls=plan["device_hulls"], differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 3 and plan["segments"] == 1 and plan["device_hulls"] == 3
    assert plan["hulls"] == [c.hull(base, 8) for c in calls]
    assert launches == 1 and kernel.endswith("_jit_shape_runs_grouped"), (launches, kernel)
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("where", ["device", "host"])
def test_shared_operands_and_index_base_one(xs, orc, torch_gpu, where):
    """the remaining ways to address a batch: index_base 1 with stride_a == NULL (one A for the whole batch, the base pointer itself),
    index_base 1 with three arrays, and arrays of pointers with one shared A (stride_a == NULL: every item reads entry 0). With
    arrays in device memory the hulls come from the hull kernel, with host arrays from the host: both must be the ones computed here."""
    torch = torch_gpu
    L = xs.lib()
    pool = Pool(np.float64, 404)
    rng = pool.rng
    # X: 13^3, A shared, runs of 4; Y: 16^3, all three arrays, base 1; Z: pointers, 23x13x32, A shared, every item its own C
    sx, sy, sz = 400, 300, 250
    ax, bx, cx = pool.alloc(13 * 13), pool.alloc(sx * 169), pool.alloc((sx // 4) * 169)
    ay, by, cy = pool.alloc(sy * 256), pool.alloc(sy * 256), pool.alloc(sy * 256)
    az, bz, cz = pool.alloc(23 * 32), pool.alloc(sz * 32 * 13), pool.alloc(sz * 23 * 13)
    ix, iy, iz = np.arange(sx), np.arange(sy), np.arange(sz)
    X = Call((13, 13, 13), np.full(sx, ax), bx + ix * 169, cx + (ix // 4) * 169)
    Y = Call((16, 16, 16), ay + rng.permutation(sy) * 256, by + iy * 256, cy + iy * 256)
    Z = Call((23, 13, 32), np.full(sz, az), bz + iz * 32 * 13, cz + iz * 23 * 13)
    data = pool.data()
    ref = oracle(orc, data, [X, Y, Z])

    def go(bracket):
        dev = torch.from_numpy(data.copy()).cuda()
        base = dev.data_ptr()
        put = (lambda x: torch.from_numpy(x).cuda()) if where == "device" else (lambda x: x)
        keep = [put((X.ib + 1).astype(np.int32)), put((X.ic + 1).astype(np.int32))]
        keep += [put((v + 1).astype(np.int32)) for v in (Y.ia, Y.ib, Y.ic)]
        keep += [put(np.array([base + az * 8], dtype=np.int64)), put((base + Z.ib.astype(np.int64) * 8)), put((base + Z.ic.astype(np.int64) * 8))]
        eight = np.array([8], dtype=np.int32)
        torch.cuda.synchronize()
        before = L.libxsmm_amd_launch_count()
        if bracket:
            xs.defer_begin()
        xs.gemm_batch(xs.F64, "N", "N", 13, 13, 13, 1.0, base + ax * 8, 13, dev, 13, 1.0, dev, 13, 1, 4, None, keep[0], keep[1], sx)
        xs.gemm_batch(xs.F64, "N", "N", 16, 16, 16, 1.0, dev, 16, dev, 16, 1.0, dev, 16, 1, 4, keep[2], keep[3], keep[4], sy)
        xs.gemm_batch(xs.F64, "N", "N", 23, 13, 32, 1.0, keep[5], 23, keep[6], 32, 1.0, keep[7], 23, 0, 0, None, eight, eight, sz)
        if bracket:
            xs.defer_end()
        launches = L.libxsmm_amd_launch_count() - before
        torch.cuda.synchronize()
        return dev.cpu().numpy(), launches, (xs.merge_last_plan() if bracket else None), base

    with _Jit(xs):
        plain, launches_plain, _, _ = go(False)
        got, launches, plan, base = go(True)
    show("shared A, index_base 1, %s arrays" % where, launches_plain=launches_plain, launches=launches, kernel=xs.last_kernel(), segments=plan["segments"],
         device_hulls=plan["device_hulls"], differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 3 and plan["segments"] == 1 and plan["device_hulls"] == (3 if where == "device" else 0)
    assert plan["hulls"] == [c.hull(base, 8) for c in (X, Y, Z)]
    assert launches < launches_plain
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


# ---- 5. a call that cannot be recorded ---------------------------------------------------------------------------------------------------
def test_a_call_outside_the_smm_domain_runs_in_its_place(xs, torch_gpu):
    """alpha = 2 takes the general path: it flushes the record, runs, and the following calls are recorded anew. Call 1 (alpha = 2)
    reads as A what call 0 wrote; call 2 updates the C of call 0 and call 3 reads as A what call 1 wrote."""
    torch = torch_gpu
    pool = Pool(np.float64, 9)
    m = n = k = 16
    s = 250
    i = np.arange(s)
    c0, (_, _, oc0) = stack(pool, (m, n, k), s, 1)
    ob1, oc1 = pool.alloc(s * k * n), pool.alloc(s * m * n)
    c1 = Call((m, n, k), oc0 + i * m * n, ob1 + i * k * n, oc1 + i * m * n, alpha=2.0)
    oa2, ob2 = pool.alloc(s * m * k), pool.alloc(s * k * n)
    c2 = Call((m, n, k), oa2 + i * m * k, ob2 + i * k * n, oc0 + i * m * n)
    ob3, oc3 = pool.alloc(s * k * n), pool.alloc(s * m * n)
    c3 = Call((m, n, k), oc1 + i * m * n, ob3 + i * k * n, oc3 + (i // 5) * m * n)
    calls = [c0, c1, c2, c3]
    data = pool.data()
    # the sequential program in numpy (the general path is not an fma chain: rounding-level tolerance against this, bits against the plain run)
    ref = data.copy()
    for c in calls:
        for j in range(c.size):
            A = ref[c.ia[j]:c.ia[j] + m * k].reshape(k, m).T; B = ref[c.ib[j]:c.ib[j] + k * n].reshape(n, k).T
            ref[c.ic[j]:c.ic[j] + m * n] += c.alpha * (A @ B).T.reshape(-1)
    with _Jit(xs):
        plain, _, _, _, _ = run(xs, torch, data, calls, False)
        got, launches, kernel, plan, _ = run(xs, torch, data, calls, True)
    err = float(np.max(np.abs(got - ref)))
    show("alpha = 2 in the middle", launches=launches, kernel=kernel, last_plan_calls=plan["calls"], err_vs_numpy=err,
         differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 2  # calls 2 and 3, recorded after the general call
    assert np.array_equal(bits(got), bits(plain))
    # k products of magnitude <= 1 per element, three chained calls: eps * k * growth, with a margin
    assert err <= np.finfo(np.float64).eps * k * 64 * max(1.0, float(np.max(np.abs(ref))))


# ---- 6. the caller's own work between calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bracket", [False, True])
def test_caller_modifies_b_on_the_stream_after_a_flush(xs, orc, torch_gpu, bracket):
    """inside the bracket: two calls, libxsmm_amd_flush(), a torch operation on the library's stream that halves B, two more calls
    that read the new B (tests/test_call_order_gpu.py: the caller's side of the contract is the flush)"""
    torch = torch_gpu
    L = xs.lib()
    pool = Pool(np.float64, 12)
    shape = (23, 23, 23)
    s = 300
    first, (oa, ob, oc) = stack(pool, shape, s, 6)
    i = np.arange(s)
    oc2, oc3 = pool.alloc(s * 23 * 23), pool.alloc(s * 23 * 23)
    other, _ = stack(pool, (13, 13, 13), 200, 4)
    second = Call(shape, first.ia, first.ib, oc2 + i * 23 * 23)   # the same A and B as `first`
    third = Call(shape, first.ia, first.ib, oc3 + (i // 3) * 23 * 23)
    data = pool.data()
    ref = oracle(orc, data, [first, other])
    ref[ob:ob + s * 23 * 23] *= 0.5
    ref = oracle(orc, ref, [second, third])
    stream = torch.cuda.Stream()
    keep = []
    dev = torch.from_numpy(data.copy()).cuda()
    torch.cuda.synchronize()
    L.libxsmm_amd_set_stream(C.c_void_p(stream.cuda_stream))
    try:
        with _Jit(xs), torch.cuda.stream(stream):
            if bracket:
                xs.defer_begin()
            issue(xs, torch, dev, first, "device", "index", keep)
            issue(xs, torch, dev, other, "host", "index", keep)
            if bracket:
                xs.flush()
                plan1 = xs.merge_last_plan()
            dev[ob:ob + s * 23 * 23].mul_(0.5)
            issue(xs, torch, dev, second, "device", "index", keep)
            issue(xs, torch, dev, third, "device", "index", keep)
            if bracket:
                xs.defer_end()
                plan2 = xs.merge_last_plan()
        stream.synchronize()
    finally:
        L.libxsmm_amd_set_stream(None)
    got = dev.cpu().numpy()
    show("caller halves B between calls, bracket=%s" % bracket, differing=int(np.count_nonzero(bits(got) != bits(ref))))
    if bracket:
        assert plan1["calls"] == 2 and plan1["segments"] == 1 and plan1["device_hulls"] == 1
        assert plan2["calls"] == 2 and plan2["segments"] == 1 and plan2["device_hulls"] == 2
    assert np.array_equal(bits(got), bits(ref))


# ---- 7. many calls -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", [0, 1])
def test_more_calls_than_the_flush_bound(xs, orc, torch_gpu, mfma):
    """fp32, tiny batches: 150 independent calls -- more than the record holds (it is flushed at the bound and goes on), more than the 32
    groups one fused launch takes in one segment -- and a last call that depends on the first one"""
    torch = torch_gpu
    dtype = np.float32
    pool = Pool(dtype, 150)
    shapes = [(13, 13, 13), (8, 8, 8), (23, 23, 23), (5, 7, 3)]  # (a cycle of four: the fused launches of 32 calls are made of the same bodies)
    calls, first_c = [], None
    for j in range(150):
        c, (_, _, oc) = stack(pool, shapes[j % len(shapes)], 12 + j % 9, 1 + j % 4)
        calls.append(c)
        first_c = oc if first_c is None else first_c
    m, n, k = shapes[0]
    ob, oc = pool.alloc(5 * k * n), pool.alloc(m * n)
    i = np.arange(5)
    calls.append(Call(shapes[0], first_c + i * m * n, ob + i * k * n, oc + 0 * i))  # reads the first call's C blocks; one C for the batch
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs, mfma):
        plain, launches_plain, _, _, _ = run(xs, torch, data, calls, False, "device")
        got, launches, kernel, plan, _ = run(xs, torch, data, calls, True, "device")
        got_h, launches_h, _, plan_h, _ = run(xs, torch, data, calls, True, "host")
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))))
    show("151 tiny fp32 calls, mfma=%d" % mfma, launches_plain=launches_plain, launches=launches, launches_host_arrays=launches_h, kernel=kernel,
         last_plan_calls=plan["calls"], last_plan_segments=plan["segments"], err_vs_oracle=err,
         differing=int(np.count_nonzero(bits(got) != bits(plain))), differing_host=int(np.count_nonzero(bits(got_h) != bits(plain))))
    assert len(calls) > 2 * FLUSH_BOUND and launches_plain >= len(calls)
    assert plan["calls"] == len(calls) - 2 * FLUSH_BOUND == plan_h["calls"]   # the record was flushed twice on the way
    assert plan["segments"] == 1 and plan["device_hulls"] == plan["calls"] and plan_h["device_hulls"] == 0
    assert launches < launches_plain // 8 and launches_h < launches_plain // 8
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got_h), bits(plain))
    if 0 == mfma:
        assert np.array_equal(bits(got), bits(ref))  # scalar kernels: the oracle's fma chain
    else:  # products of up to 23 terms of magnitude <= 1, runs of up to 5 products: eps * terms, with a margin
        assert err <= np.finfo(dtype).eps * 23 * 5 * 4 * max(1.0, float(np.max(np.abs(ref))))


def test_dependent_call_inside_a_long_record(xs, orc, torch_gpu):
    """40 calls in one record: 35 independent ones (two fused launches: a launch takes 32 groups), then calls that read and update
    what earlier ones wrote -- segments in call order"""
    torch = torch_gpu
    pool = Pool(np.float64, 40)
    calls, regions = [], []
    for j in range(35):
        c, reg = stack(pool, (13, 13, 13) if j % 2 else (16, 16, 16), 60 + j, 1 + j % 3)
        calls.append(c); regions.append(reg)
    i = np.arange(20)
    ob, oc = pool.alloc(20 * 256), pool.alloc(20 * 256)
    calls.append(Call((16, 16, 16), regions[0][2] + i * 256, ob + i * 256, oc + i * 256))          # reads C of call 0 (unique blocks there: 60 of them)
    calls.append(stack(pool, (13, 13, 13), 50, 2)[0])                                               # independent
    oa, ob2 = pool.alloc(20 * 256), pool.alloc(20 * 256)
    calls.append(Call((16, 16, 16), oa + i * 256, ob2 + i * 256, regions[0][2] + i * 256))          # updates C of call 0: behind the reader
    calls.append(Call((16, 16, 16), oc + i * 256, ob2 + i * 256, regions[2][2] + (i // 2) * 256))   # reads the reader's C, updates C of call 2
    calls.append(stack(pool, (16, 16, 16), 30, 3)[0])
    data = pool.data()
    ref = oracle(orc, data, calls)
    with _Jit(xs):
        plain, launches_plain, _, _, _ = run(xs, torch, data, calls, False)
        got, launches, kernel, plan, base = run(xs, torch, data, calls, True)
    show("40 calls, dependent ones at the end", launches_plain=launches_plain, launches=launches, kernel=kernel, segment_of=plan["segment_of"],
         differing=int(np.count_nonzero(bits(got) != bits(plain))))
    assert plan["calls"] == 40 and plan["hulls"] == [c.hull(base, 8) for c in calls]
    assert plan["segment_of"] == [0] * 35 + [1, 1, 2, 2, 2] == xs.merge_segments(plan["hulls"])[1]
    assert np.array_equal(bits(got), bits(plain))
    assert np.array_equal(bits(got), bits(ref))


# ---- 8. nesting and idle -----------------------------------------------------------------------------------------------------------------
def test_nesting_idle_bracket_and_synchronize(xs, orc, torch_gpu):
    torch = torch_gpu
    L = xs.lib()
    pool = Pool(np.float64, 8)
    calls = [stack(pool, (13, 13, 13), 300, 5)[0], stack(pool, (23, 23, 23), 200, 3)[0]]
    data = pool.data()
    ref = oracle(orc, data, calls)
    keep = []
    with _Jit(xs):
        # an idle bracket launches nothing
        torch.cuda.synchronize()
        before = L.libxsmm_amd_launch_count()
        xs.defer_begin(); xs.defer_end()
        xs.defer_begin(); xs.defer_begin(); xs.defer_end(); xs.defer_end()
        assert L.libxsmm_amd_launch_count() == before
        # an inner end does not flush, the outer one does
        dev = torch.from_numpy(data.copy()).cuda()
        torch.cuda.synchronize()
        before = L.libxsmm_amd_launch_count()
        xs.defer_begin()
        issue(xs, torch, dev, calls[0], "device", "index", keep)
        xs.defer_begin()
        issue(xs, torch, dev, calls[1], "device", "index", keep)
        xs.defer_end()
        assert L.libxsmm_amd_launch_count() == before and 1 == L.libxsmm_amd_defer_active()
        torch.cuda.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(data))  # nothing has run yet
        xs.defer_end()
        assert 1 == L.libxsmm_amd_launch_count() - before and xs.last_kernel().endswith("_jit_shape_runs_grouped")
        assert xs.merge_last_plan()["calls"] == 2
        torch.cuda.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(ref))
        # a bracket left open: libxsmm_amd_synchronize() launches what was recorded and waits for it
        dev = torch.from_numpy(data.copy()).cuda()
        torch.cuda.synchronize()
        xs.defer_begin()
        try:
            for c in calls:
                issue(xs, torch, dev, c, "host", "index", keep)
            before = L.libxsmm_amd_launch_count()
            assert 0 == L.libxsmm_amd_synchronize()
            assert 1 == L.libxsmm_amd_launch_count() - before
            assert np.array_equal(bits(dev.cpu().numpy()), bits(ref))
        finally:
            xs.defer_end()
        assert 0 == L.libxsmm_amd_defer_active()


def test_without_a_bracket_the_environment_variable_alone_records_nothing(xs, torch_gpu):
    """LIBXSMM_AMD_DEFER=1 merges per-product kernel calls only (a child process: the variable is read once)"""
    code = ("import importlib, sys, numpy as np, torch\n"
            "sys.path.insert(0, %r)\n"
            "xs = importlib.import_module('libxsmm-1_amd'); L = xs.lib()\n"
            "a = torch.rand(100 * 64, dtype=torch.float64, device='cuda'); b = torch.rand(100 * 64, dtype=torch.float64, device='cuda')\n"
            "c = torch.zeros(100 * 64, dtype=torch.float64, device='cuda'); i = (torch.arange(100, device='cuda') * 64).to(torch.int32)\n"
            "assert 1 == L.libxsmm_amd_defer_active()\n"
            "before = L.libxsmm_amd_launch_count()\n"
            "for _ in range(3): xs.gemm_batch(xs.F64, 'N', 'N', 8, 8, 8, 1.0, a, 8, b, 8, 1.0, c, 8, 0, 4, i, i, i, 100)\n"
            "assert 3 == L.libxsmm_amd_launch_count() - before, L.libxsmm_amd_launch_count() - before\n"
            "assert 0 == xs.merge_last_plan()['calls']\n"
            "torch.cuda.synchronize(); print('launch per call')\n") % ROOT
    import sys
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LIBXSMM_AMD_DEFER="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "launch per call" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------------
def test_bracket_example_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    """examples/cp2k_bracket_caller.c: compiled against include/ only, checks itself (bracketed == unbracketed bit for bit, fewer launches)"""
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "cp2k_bracket_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cp2k_bracket_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(res.stdout[-1000:], res.stderr[-1000:])
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "cp2k_bracket_caller" in res.stdout
