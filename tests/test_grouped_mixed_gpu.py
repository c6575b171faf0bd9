"""Grouped launches on the matrix cores with groups of mixed forms (GPU).

One group off the matrix-core run form -- B transposed, or a B span beyond 2560 elements -- turns every body of the grouped
kernel into a called function (tests/test_handwait_invariant.py checks the code objects). Here the numbers: every C block
equals the oracle's sequential chain bit for bit (relaxed orders and out-of-order repeats: the tolerance of
tests/test_jit.py::test_grouped_batches_one_launch), through libxsmm_amd_gemm_batch_groups and through libxsmm_?gemm_batch
with host pointer arrays, always as ONE multiplication launch.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANS_B = 2  # LIBXSMM_GEMM_FLAG_TRANS_B


class _MatrixCoresJit:
    """matrix cores on, small batches on the run-time specialised kernels; both restored on the way out"""
    def __init__(self, xs):
        self.xs = xs
    def __enter__(self):
        self.old_env = os.environ.get("LIBXSMM_AMD_JIT_MINBATCH")
        os.environ["LIBXSMM_AMD_JIT_MINBATCH"] = "1"
        self.old = self.xs.lib().libxsmm_amd_set_mfma(1)
    def __exit__(self, *exc):
        self.xs.lib().libxsmm_amd_set_mfma(self.old)
        if self.old_env is None:
            del os.environ["LIBXSMM_AMD_JIT_MINBATCH"]
        else:
            os.environ["LIBXSMM_AMD_JIT_MINBATCH"] = self.old_env


def _wide_ldb(dtype):
    # B span 31 * ldb + 32 beyond 2560 elements: not the run form. (fp64: ldb 100 puts the operands of an item beyond the
    # 40 KiB the grouped wave forms take, and the call would not be fused -- 90 keeps it in)
    return 100 if dtype == np.float32 else 90


def _tolerance(dtype, longest, k, ref):
    # two orders of the same sum: rounding errors random-walk, eps * sqrt(terms) with a margin of 4 (test_grouped_batches_one_launch)
    return np.finfo(dtype).eps * np.sqrt(float(longest) * k) * 4 * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("relaxed", [False, True])
def test_grouped_mixed_forms_on_the_matrix_cores(xs, orc, torch_gpu, dtype, relaxed):
    """libxsmm_amd_gemm_batch_groups: 13^3 and 32^3 runs (run form), 23^3 runs with B transposed, 32^3 runs with a wide ldb,
    5x7x3 runs, a group with one C, a group whose C blocks repeat out of order -- one multiplication launch"""
    torch = torch_gpu
    L = xs.lib()
    prec = xs.F64 if dtype == np.float64 else xs.F32
    rng = np.random.default_rng(2024)
    wide = _wide_ldb(dtype)
    # (m, n, k), transb, ldb (None: tight), products, C layout
    spec = [((13, 13, 13), "N", None, 700, "runs"), ((32, 32, 32), "N", None, 500, "runs"), ((23, 23, 23), "T", None, 600, "runs"),
            ((32, 32, 32), "N", wide, 400, "runs"), ((5, 7, 3), "N", None, 333, "runs"), ((13, 13, 13), "N", None, 300, "one"),
            ((8, 8, 8), "N", None, 500, "repeat")]
    shapes, transb, ldbs, sizes, groups = [], [], [], [], []
    for gi, ((m, n, k), tb, ldb, s, layout) in enumerate(spec):
        ldb_ = ldb if ldb is not None else (n if tb == "T" else k)
        bspan = ldb_ * ((k if tb == "T" else n) - 1) + (n if tb == "T" else k)  # elements of one B in memory
        bstride = bspan + 3
        a = rng.uniform(-1, 1, s * m * k).astype(dtype)
        b = rng.uniform(-1, 1, s * bstride).astype(dtype)
        if layout == "runs":      # runs of ~ u consecutive products per C (cp2k.cpp:155)
            cidx = np.arange(s) // max(1, int(np.sqrt(s * 160 / 240)))
        elif layout == "one":     # one C for the whole group (stride_c NULL)
            cidx = None
        else:                     # C blocks repeat out of order (atomics)
            cidx = rng.integers(0, 40, s)
        nc = 1 if cidx is None else int(cidx.max()) + 1
        c = rng.uniform(-1, 1, nc * m * n).astype(dtype)
        sa = (rng.permutation(s) * m * k).astype(np.int32)
        sb = (np.arange(s) * bstride).astype(np.int32)
        sc = None if cidx is None else (cidx * m * n).astype(np.int32)
        ref = c.copy()
        flags = TRANS_B if tb == "T" else 0
        assert 0 == orc.gemm_batch_idx(orc.FMA, flags, m, n, k, m, ldb_, m, a, b, ref, 0, sa, sb,
                                       sc if sc is not None else np.zeros(s, dtype=np.int32), s)
        dev = [torch.from_numpy(x).cuda() for x in (a, b, c, sa, sb)] + [None if sc is None else torch.from_numpy(sc).cuda()]
        groups.append((dev, ref, cidx))
        shapes.append((m, n, k)); transb.append(tb); ldbs.append(ldb_); sizes.append(s)
    with _MatrixCoresJit(xs):
        launches = L.libxsmm_amd_launch_count()
        rc = xs.gemm_batch_groups(prec, shapes, [g[0][0] for g in groups], [g[0][1] for g in groups], [g[0][2] for g in groups],
                                  [g[0][3] for g in groups], [g[0][4] for g in groups], [g[0][5] for g in groups], sizes,
                                  relaxed=relaxed, transb=transb, ldb=ldbs)
        assert rc == 0
        torch.cuda.synchronize()
        assert xs.last_kernel().endswith("_jit_shape_runs_grouped"), xs.last_kernel()
        assert L.libxsmm_amd_launch_count() == launches + 1  # (the C-ordering check is not a compute kernel)
    for gi, ((dev, ref, cidx), ((m, n, k), tb, ldb, s, layout)) in enumerate(zip(groups, spec)):
        out = dev[2].cpu().numpy()
        if relaxed or layout == "repeat":
            longest = s if cidx is None else int(np.bincount(cidx).max())
            err = np.max(np.abs(out.astype(np.float64) - ref.astype(np.float64)))
            assert err <= _tolerance(dtype, longest, k, ref), (gi, err)
        else:
            assert np.array_equal(out, ref), (gi, float(np.max(np.abs(out.astype(np.float64) - ref.astype(np.float64)))))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gemm_batch_groups_with_transposed_and_wide_b_fused(xs, orc, torch_gpu, dtype):
    """libxsmm_dgemm_batch / libxsmm_sgemm_batch with host pointer arrays to device matrices (the fused path of several
    groups): transb N, T, N and a group with a wide ldb -- one multiplication launch, every C block bit for bit"""
    torch = torch_gpu
    L = xs.lib()
    rng = np.random.default_rng(99)
    wide = _wide_ldb(dtype)
    # (m, n, k), transb, ldb, products, products per C
    spec = [((13, 13, 13), "N", 13, 240, 12), ((23, 23, 23), "T", 23, 200, 10), ((32, 32, 32), "N", 32, 160, 8),
            ((32, 32, 32), "N", wide, 120, 6)]
    tot = sum(g[3] for g in spec)
    pa = np.zeros(tot, dtype=np.uint64); pb = np.zeros(tot, dtype=np.uint64); pc = np.zeros(tot, dtype=np.uint64)
    keep, checks = [], []
    j = 0
    for (m, n, k), tb, ldb, cnt, run in spec:
        bspan = ldb * ((k if tb == "T" else n) - 1) + (n if tb == "T" else k)
        sa_, sb_, sc_ = m * k + 3, bspan + 5, m * n + 7
        nc = (cnt + run - 1) // run
        pool_a = rng.uniform(-1, 1, cnt * sa_).astype(dtype); pool_b = rng.uniform(-1, 1, cnt * sb_).astype(dtype)
        pool_c = rng.uniform(-1, 1, nc * sc_).astype(dtype)
        ref = pool_c.copy()
        for i in range(cnt):
            ci = i // run
            orc.smm(orc.FMA, TRANS_B if tb == "T" else 0, m, n, k, m, ldb, m, pool_a[i * sa_:i * sa_ + m * k],
                    pool_b[i * sb_:i * sb_ + bspan], ref[ci * sc_:ci * sc_ + m * n])
        dpa, dpb, dpc = (torch.from_numpy(x).cuda() for x in (pool_a, pool_b, pool_c))
        esz = np.dtype(dtype).itemsize
        for i in range(cnt):  # C blocks at increasing addresses, each a run of `run` consecutive products
            pa[j] = dpa.data_ptr() + i * sa_ * esz; pb[j] = dpb.data_ptr() + i * sb_ * esz; pc[j] = dpc.data_ptr() + (i // run) * sc_ * esz
            j += 1
        keep.append((dpa, dpb))
        checks.append((dpc, ref, sc_, m * n, nc))
    ng = len(spec)
    ta = (C.c_char * ng)(*[b"N"] * ng); tb_ = (C.c_char * ng)(*[g[1].encode() for g in spec])
    ms = (C.c_int * ng)(*[g[0][0] for g in spec]); ns = (C.c_int * ng)(*[g[0][1] for g in spec]); ks = (C.c_int * ng)(*[g[0][2] for g in spec])
    ldas = (C.c_int * ng)(*[g[0][0] for g in spec]); ldbs = (C.c_int * ng)(*[g[2] for g in spec]); ldcs = (C.c_int * ng)(*[g[0][0] for g in spec])
    ct = C.c_double if dtype == np.float64 else C.c_float
    al = (ct * ng)(*[1.0] * ng); be = (ct * ng)(*[1.0] * ng)
    gs = (C.c_int * ng)(*[g[3] for g in spec]); gc = C.c_int(ng)
    f = L.libxsmm_dgemm_batch if dtype == np.float64 else L.libxsmm_sgemm_batch
    with _MatrixCoresJit(xs):
        launches = L.libxsmm_amd_launch_count()
        f(ta, tb_, ms, ns, ks, al, xs.dptr(pa), ldas, xs.dptr(pb), ldbs, be, xs.dptr(pc), ldcs, C.byref(gc), gs)
        torch.cuda.synchronize()
        assert xs.last_kernel().endswith("_jit_shape_runs_grouped"), xs.last_kernel()
        assert L.libxsmm_amd_launch_count() == launches + 1
    for gi, (dpc, ref, sc_, mn, nc) in enumerate(checks):
        out = dpc.cpu().numpy()
        for ci in range(nc):
            assert np.array_equal(out[ci * sc_:ci * sc_ + mn], ref[ci * sc_:ci * sc_ + mn]), (gi, ci)
        assert np.array_equal(out, ref), gi  # (the gaps between the C blocks untouched)


@pytest.mark.gpu
def test_cp2k_shapes_with_called_bodies(xs):
    """the 27 CP2K shapes and the call with more groups than one launch takes (tests/test_mfma_runs_gpu.py) once more with
    XSMM_SMMJIT_GROUPED_INLINE=0 -- every body a called function -- in a child process (the knob is read once)"""
    env = dict(os.environ, XSMM_SMMJIT_GROUPED_INLINE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "cp2k_27_shape_grouped_launch or more_groups_than_one_launch",
                        os.path.join(ROOT, "tests", "test_mfma_runs_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-2000:])
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
