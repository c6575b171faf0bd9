"""Tiled GEMM on the GPU: libxsmm_gemm_handle_init / libxsmm_gemm_thread / libxsmm_xgemm_omp (kernels/tgemm.hip).

Every comparison is bit for bit (results viewed as unsigned integers) against the oracle's fused multiply-add chain
(xo_dsmm / xo_ssmm with XO_ARITH_FMA): each element of C is one chain over k in ascending order that starts from C
(beta = 1) or from 0 (beta = 0). For TRANS_A, op(A) is materialised in numpy and the oracle runs NN; TRANS_B is the
oracle's own flag. T is the work-group tile of the kernel (xsmm::TGEMM_TILE, asked for through libxsmm_amd_gemm_tile);
the matrix instructions are 2 (fp32) and 4 (fp64) deep and the k chunk in LDS is 32 (fp32) and 16 (fp64) deep, so
k = 1, 3, 34, 130 lie below, at and just past both."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def uview(x):
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def same_bits(x, y):
    return np.array_equal(uview(x), uview(y))


class Case(object):
    """operands of one product in host memory (flat, column major) and its gold result"""

    def __init__(self, orc, xs, dtype, ta, tb, m, n, k, beta, pad=0, seed=0, a=None, b=None, c=None):
        rng = np.random.default_rng(seed)
        self.dtype, self.ta, self.tb, self.m, self.n, self.k, self.beta = dtype, ta, tb, m, n, k, beta
        self.prec = xs.F64 if dtype == np.float64 else xs.F32
        self.lda = (k if ta else m) + pad
        self.ldb = (n if tb else k) + pad
        self.ldc = m + pad
        self.a = rng.uniform(-1, 1, self.lda * (m if ta else k)).astype(dtype) if a is None else a
        self.b = rng.uniform(-1, 1, self.ldb * (k if tb else n)).astype(dtype) if b is None else b
        self.c = rng.uniform(-1, 1, self.ldc * n).astype(dtype) if c is None else c
        # gold: op(A) tight and not transposed, B as it lies
        opa = self.a.reshape(-1, self.lda)[:m, :k].T.copy().ravel() if ta else self.a
        self.gold = self.c.copy()
        flags = (orc.FLAG_TRANS_B if tb else 0) | (orc.FLAG_BETA_0 if 0 == beta else 0)
        orc.smm(orc.FMA, flags, m, n, k, m if ta else self.lda, self.ldb, self.ldc, opa, self.b, self.gold)

    def handle(self, xs, ntasks=1):
        keep, h = xs.gemm_handle(self.prec, self.prec, "T" if self.ta else "N", "T" if self.tb else "N", self.m, self.n, self.k,
                                 self.lda, self.ldb, self.ldc, 1.0, float(self.beta), ntasks=ntasks)
        assert h
        return keep, h

    def on_device(self, torch):
        return [torch.from_numpy(x.copy()).cuda() for x in (self.a, self.b, self.c)]


def run_device(xs, torch, case, tasks=((0, 1),)):
    keep, h = case.handle(xs)
    da, db, dc = case.on_device(torch)
    for tid, nthreads in tasks:
        xs.gemm_thread(h, da, db, dc, tid, nthreads)
    torch.cuda.synchronize()
    assert same_bits(da.cpu().numpy(), case.a) and same_bits(db.cpu().numpy(), case.b)
    return dc.cpu().numpy()


def shapes(xs):
    T = xs.lib().libxsmm_amd_gemm_tile()
    return T, [(1, 1, 1), (T - 1, T + 1, 3), (T + 1, T - 1, 34), (2 * T + 1, 33, 130), (33, 2 * T + 1, 1)]


@pytest.mark.parametrize("trans", ["NN", "NT", "TN", "TT"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity(xs, orc, torch_gpu, dtype, trans):
    ta, tb = trans[0] == "T", trans[1] == "T"
    T, cases = shapes(xs)
    for beta in (0, 1):
        for idx, (m, n, k) in enumerate(cases):
            for pad in (0, 3):
                case = Case(orc, xs, dtype, ta, tb, m, n, k, beta, pad, seed=100 * idx + 10 * beta + pad)
                got = run_device(xs, torch_gpu, case)
                assert xs.last_kernel().startswith("tgemm_f%d_" % (64 if dtype == np.float64 else 32))
                assert same_bits(got, case.gold), (trans, beta, m, n, k, pad, int(np.sum(uview(got) != uview(case.gold))))


@pytest.mark.parametrize("k", [3, 35])
@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_zero_survives_the_k_tail(xs, orc, torch_gpu, dtype, k):
    """beta = 1, C = -0.0 everywhere, B all zeros, A negative: every product is -0.0 and fma(a, 0, -0.0) stays -0.0, while a
    zero-padded step through the accumulator, fma(0, 0, -0.0), would give +0.0"""
    T, _ = shapes(xs)
    m, n = T + 1, 33
    rng = np.random.default_rng(k)
    a = (-rng.uniform(0.25, 1, m * k)).astype(dtype)
    b = np.zeros(k * n, dtype=dtype)
    c = np.full(m * n, -0.0, dtype=dtype)
    case = Case(orc, xs, dtype, False, False, m, n, k, 1, a=a, b=b, c=c)
    got = run_device(xs, torch_gpu, case)
    assert same_bits(got, c), int(np.sum(uview(got) != uview(c)))
    assert same_bits(got, case.gold)


@pytest.mark.parametrize("dtype", DTYPES)
def test_beta_zero_never_reads_c(xs, orc, torch_gpu, dtype):
    T, _ = shapes(xs)
    for ta, tb, (m, n, k) in ((False, False, (T + 1, 33, 34)), (True, True, (33, T + 1, 3))):
        c = np.full((m + 3) * n, np.nan, dtype=dtype)
        case = Case(orc, xs, dtype, ta, tb, m, n, k, 0, pad=3, seed=5, c=c)
        got = run_device(xs, torch_gpu, case).reshape(n, m + 3)
        assert not np.isnan(got[:, :m]).any()
        assert same_bits(got[:, m:], c.reshape(n, m + 3)[:, m:])  # the padding keeps its NaN bytes
        assert same_bits(got.ravel(), case.gold)


@pytest.mark.parametrize("config", [(np.float64, True, False), (np.float32, False, True)])
def test_gemm_thread_tasks(xs, orc, torch_gpu, config):
    dtype, ta, tb = config
    T, _ = shapes(xs)
    m, n, k = 2 * T + 1, 2 * T + 5, 34
    case = Case(orc, xs, dtype, ta, tb, m, n, k, 1, pad=3, seed=11)
    single = run_device(xs, torch_gpu, case)
    assert same_bits(single, case.gold)
    for nthreads in (1, 3, 16):
        order = np.random.default_rng(nthreads).permutation(nthreads)
        got = run_device(xs, torch_gpu, case, tasks=[(int(tid), nthreads) for tid in order])
        assert same_bits(got, single), nthreads
    # one task alone: its rectangle, nothing else
    keep, h = case.handle(xs, ntasks=5)
    rc, (m0, m1, n0, n1) = xs.gemm_task(h, 1, 3)
    assert rc == 0 and m0 < m1 and n0 < n1
    got = run_device(xs, torch_gpu, case, tasks=[(1, 3)]).reshape(n, case.ldc)
    want = case.c.copy().reshape(n, case.ldc)
    want[n0:n1, m0:m1] = case.gold.reshape(n, case.ldc)[n0:n1, m0:m1]
    assert same_bits(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_memory_kinds(xs, orc, torch_gpu, dtype):
    L = xs.lib()
    T, _ = shapes(xs)
    case = Case(orc, xs, dtype, True, False, T + 1, T + 5, 35, 1, pad=3, seed=7)
    keep, h = case.handle(xs)
    # device memory of the library's allocator
    ptrs = []
    for x in (case.a, case.b, case.c):
        p = L.libxsmm_amd_device_malloc(x.nbytes)
        assert p and 0 == L.libxsmm_amd_memcpy_h2d(p, xs.dptr(x), x.nbytes)
        ptrs.append(p)
    xs.gemm_thread(h, ptrs[0], ptrs[1], ptrs[2])
    dev = np.empty_like(case.c)
    assert 0 == L.libxsmm_amd_synchronize() and 0 == L.libxsmm_amd_memcpy_d2h(xs.dptr(dev), ptrs[2], dev.nbytes)
    # pageable numpy arrays: complete on return, all three tasks of three
    host = case.c.copy()
    for tid in range(3):
        xs.gemm_thread(h, case.a, case.b, host, tid, 3)
    # A on the device, B and C on the host
    mixed = case.c.copy()
    xs.gemm_thread(h, ptrs[0], case.b, mixed)
    for p in ptrs:
        L.libxsmm_amd_device_free(p)
    assert same_bits(dev, case.gold) and same_bits(host, case.gold) and same_bits(mixed, case.gold)


def test_xgemm_omp(xs, orc, torch_gpu):
    torch = torch_gpu
    T, _ = shapes(xs)
    for dtype in DTYPES:
        case = Case(orc, xs, dtype, False, True, T + 1, 33, 34, 0, pad=3, seed=13)
        da, db, dc = case.on_device(torch)
        xs.xgemm_omp(case.prec, "N", "T", case.m, case.n, case.k, 1.0, da, case.lda, db, case.ldb, 0.0, dc, case.ldc)
        torch.cuda.synchronize()
        assert xs.last_kernel().startswith("tgemm_")
        got = dc.cpu().numpy()
        assert same_bits(got, run_device(xs, torch, case)) and same_bits(got, case.gold)
    # outside the handle's domain: the path of libxsmm_blas_dgemm
    case = Case(orc, xs, np.float64, True, False, 70, 45, 34, 1, pad=3, seed=17)
    da, db, dc = case.on_device(torch)
    xs.xgemm_omp(xs.F64, "T", "N", case.m, case.n, case.k, 2.0, da, case.lda, db, case.ldb, 0.5, dc, case.ldc)
    torch.cuda.synchronize()
    assert not xs.last_kernel().startswith("tgemm_")
    ea, eb, ec = case.on_device(torch)
    al, be = C.c_double(2.0), C.c_double(0.5)
    xs.lib().libxsmm_blas_dgemm(b"T", b"N", xs.iptr(case.m), xs.iptr(case.n), xs.iptr(case.k), C.byref(al), xs.dptr(ea), xs.iptr(case.lda),
                                xs.dptr(eb), xs.iptr(case.ldb), C.byref(be), xs.dptr(ec), xs.iptr(case.ldc))
    torch.cuda.synchronize()
    assert same_bits(dc.cpu().numpy(), ec.cpu().numpy())
    assert not same_bits(dc.cpu().numpy(), case.c)
    # other precisions do nothing
    before = xs.lib().libxsmm_amd_launch_count()
    xs.xgemm_omp(xs.I16, "N", "N", 8, 8, 8, None, da, 8, db, 8, None, dc, 8, oprec=xs.I32)
    assert xs.lib().libxsmm_amd_launch_count() == before


def test_call_order_inside_the_defer_bracket(xs, orc, torch_gpu):
    """dispatched kernel writes X -> libxsmm_gemm_thread reads X -> dispatched kernel reads its result: inside
    libxsmm_amd_defer_begin/end the tiled GEMM seals the open burst, so the outcome is the oracle's chain of three products"""
    torch = torch_gpu
    L = xs.lib()
    m = 32
    rng = np.random.default_rng(3)
    p, q, x, r, y, z = (rng.uniform(-1, 1, m * m) for _ in range(6))
    fn = L.libxsmm_dmmdispatch(m, m, m, None, None, None, None, None, None, None)
    assert fn
    keep, h = xs.gemm_handle(xs.F64, xs.F64, "N", "N", m, m, m)
    assert h
    gx, gy, gz = x.copy(), y.copy(), z.copy()
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, p, q, gx)    # X += P * Q
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, gx, r, gy)   # Y += X * R
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, gy, q, gz)   # Z += Y * Q

    def run(bracket):
        dp, dq, dx, dr, dy, dz = (torch.from_numpy(v.copy()).cuda() for v in (p, q, x, r, y, z))
        if bracket:
            xs.defer_begin()
        xs.call_kernel(fn, dp, dq, dx)
        xs.gemm_thread(h, dx, dr, dy)
        xs.call_kernel(fn, dy, dq, dz)
        if bracket:
            xs.defer_end()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (dx, dy, dz)]
    for bracket in (False, True):
        for got, gold in zip(run(bracket), (gx, gy, gz)):
            assert same_bits(got, gold), bracket


CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
xs = importlib.import_module("libxsmm-1_amd")
L = xs.lib()
n = 300
rng = np.random.default_rng(29)
a, b, c = (rng.uniform(-1, 1, n * n).astype(np.float32) for _ in range(3))
np.save(sys.argv[2] + "_in.npy", np.stack([a, b, c]))
L.libxsmm_sgemm(b"N", b"T", xs.iptr(n), xs.iptr(n), xs.iptr(n), None, xs.dptr(a), xs.iptr(n), xs.dptr(b), xs.iptr(n), None, xs.dptr(c), xs.iptr(n))
np.save(sys.argv[2] + "_out.npy", c)
print("kernel:", xs.last_kernel())
"""


def test_opt_in_routing_of_sgemm(xs, orc, torch_gpu, tmp_path):
    env = dict(os.environ, LIBXSMM_AMD_TGEMM="1")
    base = str(tmp_path / "route")
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, base], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "kernel: tgemm_f32_nt" in res.stdout, res.stdout
    n = 300
    a, b, c = np.load(base + "_in.npy")
    orc.smm(orc.FMA, orc.FLAG_TRANS_B, n, n, n, n, n, n, a, b, c)
    assert same_bits(np.load(base + "_out.npy"), c)


def test_example_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "tgemm_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tgemm_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "tgemm_caller: ok" in res.stdout
