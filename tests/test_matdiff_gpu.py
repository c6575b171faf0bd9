"""libxsmm_matdiff on operands in device memory, libxsmm_amd_matdiff_async and libxsmm_amd_matdiff_batch against the numpy
restatement of tests/matdiff_common.py (exact sums), which tests/test_matdiff_cpu.py holds against what the reference returns.

Tolerances are derived in tests/matdiff_common.py: fields that take no sum (minima, maxima, linf_*, m, n, *item, every +inf
of the non-finite case, the return value) bit for bit; summed fields within 4 * N * 2^-53 relative, variances within
16 * N * 2^-53, N the number of elements that enter. The shapes are the smallest at which the kernels can go wrong: a single
element, the reference's 3 x 3, vectors both ways, pitches that forbid 16-byte loads with NaN in the padding, one element
past the tile in both directions, and 1000 x 70: several strips and several tile rows."""
import ctypes as C

import numpy as np
import pytest

import matdiff_common as mc

pytestmark = pytest.mark.gpu
CASES = mc.cases()
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def feature(xs):
    """before any device pointer reaches libxsmm_matdiff: a library without the device path fails here, by assertion"""
    assert hasattr(xs.lib(), "libxsmm_amd_matdiff_async") and hasattr(xs.lib(), "libxsmm_amd_matdiff_batch")
    yield
    if WORST:
        print("largest relative deviation on the GPU: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def dev(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def call(xs, dt, m, n, ref, tst, ldr, ldt):
    info = xs.MatdiffInfo()
    rc = xs.lib().libxsmm_matdiff(C.byref(info), dt, m, n, xs.dptr(ref), xs.dptr(tst), xs.iptr(ldr), xs.iptr(ldt))
    return rc, info


def check(got, want, count, name, **kw):
    special = name.rsplit("_", 1)[0]
    if special in mc.NONFINITE:
        assert got == want, (name, got, want)  # the nine +inf, the cleared rest, the first location: all exact
    else:
        mc.compare(got, want, count, name, worst=WORST, skip=mc.skipped(name), **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_call(xs, torch_gpu, name):
    dt, m, n, ldr, ldt, ref, tst = mc.case_operands(CASES[name])
    rc_want, want = mc.matdiff(m, n, ref, tst, ldr, ldt)
    dref, dtst = dev(torch_gpu, ref), dev(torch_gpu, tst)
    rc, info = call(xs, dt, m, n, dref, dtst, ldr, ldt)
    assert rc == rc_want == 0
    assert xs.last_kernel().startswith("matdiff_")
    check(mc.fields_of(info), want, m * n, name)
    rc2, again = call(xs, dt, m, n, dref, dtst, ldr, ldt)  # the same call, the same bytes
    assert 0 == rc2 and bytes(info) == bytes(again)


def test_what_the_value_cases_are_about(xs, torch_gpu):
    """the properties the cases were built for, stated directly"""
    get = lambda name: (lambda c: (c, call(xs, c[0], c[1], c[2], dev(torch_gpu, c[5]), dev(torch_gpu, c[6]), c[3], c[4])))(mc.case_operands(CASES[name]))
    for size in ("small", "large"):
        c, (rc, info) = get("huge_" + size)
        assert 0 == rc and info.linf_abs == 1e200 and np.isfinite(info.l2_abs) and info.l2_abs < 1e4  # kept; its square is left out
        c, (rc, info) = get("tie_" + size)
        assert 0 == rc and info.linf_abs == 128.0 and (info.m, info.n) == (c[1] - 1, 1)  # the first of two equal maxima
        c, (rc, info) = get("identical_" + size)
        assert 0 == rc and (info.m, info.n) == (-1, -1) and 0 == info.linf_abs == info.l2_abs == info.norm1_abs
        c, (rc, info) = get("two_nan_" + size)
        assert 0 == rc and (info.m, info.n) == (c[1] - 1, 2) and info.linf_abs == mc.INF and 0 == info.l1_ref
        c, (rc, info) = get("nan_both_" + size)
        assert 0 == rc and (info.m, info.n) == (1, 1) and info.l2_rel == mc.INF
    c, (rc, info) = get("known_3x1_f64")
    assert (info.m, info.n) == (2, 0)
    c, (rc, info) = get("known_1x3_f64")
    assert (info.m, info.n) == (0, 2)


def test_wrong_calls_and_empty_calls(xs, torch_gpu):
    x = dev(torch_gpu, np.ones(64))
    info = xs.MatdiffInfo()
    L = xs.lib()
    assert 0 != call(xs, mc.F64, 8, 4, x, x, 7, 8)[0] and 0 != call(xs, mc.F64, 8, 4, x, x, 8, 7)[0]  # m > ld
    assert 0 != call(xs, mc.F64, -1, 4, x, x, 8, 8)[0] and 0 != call(xs, 2, 8, 4, x, x, 8, 8)[0] and 0 != call(xs, 3, 8, 4, x, x, 8, 8)[0]
    assert 0 != L.libxsmm_amd_matdiff_async(C.byref(info), mc.F64, 8, 4, xs.dptr(x), xs.dptr(x), None, None)  # info the GPU does not reach
    n0 = L.libxsmm_amd_launch_count()
    rc, info = call(xs, mc.F64, 0, 4, x, x, 8, 8)
    assert 0 == rc and mc.fields_of(info) == mc.cleared() and n0 == L.libxsmm_amd_launch_count()
    dinfo = torch_gpu.zeros(C.sizeof(xs.MatdiffInfo), dtype=torch_gpu.uint8, device="cuda")
    assert 0 == xs.matdiff(x, x, 8, 0, info=dinfo)
    assert mc.fields_of(xs.MatdiffInfo.from_buffer_copy(dinfo.cpu().numpy().tobytes())) == mc.cleared()


def test_mixed_device_and_pageable_operands(xs, torch_gpu):
    dt, m, n, ldr, ldt, ref, tst = mc.case_operands(CASES["33x5_f32"])
    want = mc.matdiff(m, n, ref, tst, ldr, ldt)[1]
    for a, b in ((dev(torch_gpu, ref), tst), (ref, dev(torch_gpu, tst))):
        rc, info = call(xs, dt, m, n, a, b, ldr, ldt)
        assert 0 == rc and xs.last_kernel().startswith("matdiff_")
        mc.compare(mc.fields_of(info), want, m * n, "mixed")


@pytest.mark.parametrize("name", sorted(mc.BATCHES))
def test_batch(xs, torch_gpu, name):
    case = mc.BATCHES[name]
    dt, m, n, ldr, ldt, sr, st, batch = case[:8]
    ref, tst = mc.batch_operands(case)
    infos, total, item = mc.batch_expected(case)
    dref, dtst = dev(torch_gpu, ref), dev(torch_gpu, tst)
    rc, info, items, which = xs.matdiff_batch(dref, dtst, dt, m, n, ldr, ldt, sr, st, batch, items=True)
    assert 0 == rc and which == item and xs.last_kernel().startswith("matdiff_")
    bad = "nan" == case[9]
    for b in range(batch):  # entry by entry against single calls
        rc1, single = call(xs, dt, m, n, dref[b * sr:], dtst[b * st:], ldr, ldt)
        assert 0 == rc1 and bytes(single) == bytes(items[b]), (name, b)
        if bad and 2 == b:
            assert mc.fields_of(items[b]) == infos[b]
        else:
            mc.compare(mc.fields_of(items[b]), infos[b], m * n, (name, b), worst=WORST)
    if bad:
        assert mc.fields_of(info) == total and 2 == which
    else:
        mc.compare(mc.fields_of(info), total, m * n, name, worst=WORST, count_l1=m * n * batch)
    # items and info in device memory: the same bytes
    ditems = torch_gpu.zeros(batch * C.sizeof(xs.MatdiffInfo), dtype=torch_gpu.uint8, device="cuda")
    dinfo = torch_gpu.zeros(C.sizeof(xs.MatdiffInfo), dtype=torch_gpu.uint8, device="cuda")
    rc, _, _, which2 = xs.matdiff_batch(dref, dtst, dt, m, n, ldr, ldt, sr, st, batch, items=ditems, info=dinfo)
    torch_gpu.cuda.synchronize()
    assert 0 == rc and which2 == item
    assert ditems.cpu().numpy().tobytes() == b"".join(bytes(x) for x in items) and dinfo.cpu().numpy().tobytes() == bytes(info)


def test_batch_larger_than_the_grid_and_a_tie_across_items(xs, torch_gpu):
    """more items than the waves of the largest grid take at once (4 per work-group, 2048 work-groups): the loop over items"""
    m, n, batch = 3, 3, 4 * 2048 + 5
    rng = np.random.default_rng(7)
    ref = rng.integers(-50, 51, batch * 9).astype(np.float32)
    tst = ref.copy()
    for b in (batch - 2, 4097, batch - 1):  # the same largest difference in three items: the lowest index wins
        tst[b * 9 + 4] += 1000
    rc, info, items, which = xs.matdiff_batch(dev(torch_gpu, ref), dev(torch_gpu, tst), mc.F32, m, n, 3, 3, 9, 9, batch, items=True)
    assert 0 == rc and 4097 == which and (info.m, info.n) == (1, 1) and info.linf_abs == 1000.0
    assert info.l1_ref == float(np.abs(ref).sum()) and info.l1_tst == float(np.abs(tst.astype(np.float64)).sum())  # integers: exact in any order
    assert info.avg_ref == info.l1_ref / (9 * batch)
    assert [i for i in range(batch) if 0 != items[i].linf_abs] == [4097, batch - 2, batch - 1]
    assert items[batch - 1].l1_ref == float(np.abs(ref[-9:]).sum()) and (items[0].m, items[0].n) == (-1, -1)


@pytest.mark.parametrize("bracket", [False, True])
def test_async_sees_the_product_queued_before_it(xs, torch_gpu, bracket):
    torch, L = torch_gpu, xs.lib()
    m, batch = 8, 64
    rng = np.random.default_rng(11)
    a = rng.integers(-4, 5, batch * m * m).astype(np.float64)
    b = rng.integers(-4, 5, batch * m * m).astype(np.float64)
    want = np.concatenate([(b[i * 64:(i + 1) * 64].reshape(m, m) @ a[i * 64:(i + 1) * 64].reshape(m, m)).reshape(-1) for i in range(batch)])  # column-major A * B
    idx = (np.arange(batch) * m * m).astype(np.int32)
    da, db, dwant = dev(torch, a), dev(torch, b), dev(torch, want)
    dc = torch.full((batch * m * m,), 12345.0, dtype=torch.float64, device="cuda")
    dinfo = torch.zeros(C.sizeof(xs.MatdiffInfo), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if bracket:
        L.libxsmm_amd_defer_begin()
    xs.gemm_batch(xs.F64, "N", "N", m, m, m, 1.0, da, m, db, m, 0.0, dc, m, 0, 4, idx, idx, idx, batch)
    rc = xs.matdiff(dc, dwant, batch * m * m, 1, info=dinfo)  # queued behind the product, nobody waits in between
    if bracket:
        L.libxsmm_amd_defer_end()
    assert 0 == rc
    torch.cuda.synchronize()
    info = xs.MatdiffInfo.from_buffer_copy(dinfo.cpu().numpy().tobytes())
    assert 0 == info.linf_abs and (info.m, info.n) == (-1, -1)
    assert info.l1_ref == float(np.abs(want).sum()) == info.l1_tst and info.l1_ref > 0  # the product, not the 12345s


def test_c_caller(xs, tmp_path):
    """examples/matdiff_caller.c: a device batch, libxsmm_amd_matdiff_batch, the fields printed"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir, exe = os.path.dirname(xs.LIB_PATH), tmp_path / "matdiff_caller"
    subprocess.run(["gcc", "-std=c89", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "matdiff_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "matdiff_caller: ok (item 617, m 3, n 5)" in res.stdout and "var_tst" in res.stdout
