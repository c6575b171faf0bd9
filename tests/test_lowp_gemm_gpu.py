"""GEMM with 16-bit inputs on the GPU: libxsmm_amd_lowp_gemm / _thread and the front ends libxsmm_wigemm / libxsmm_wsgemm /
libxsmm_bsgemm (kernels/tgemm_lowp.hip).

Every comparison is bit for bit (results viewed as unsigned integers) unless stated, against the numpy reference of
tests/lowp_gemm_common.py, which tests/test_lowp_gemm_cpu.py pins to the oracle's xo_gemm_lowp. T is the work-group tile
(libxsmm_amd_gemm_tile) and kc the kernel's k chunk (libxsmm_amd_lowp_gemm_chunk); the shapes lie below, at and just past
both."""
import os
import subprocess

import numpy as np
import pytest

import lowp_gemm_common as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TRANS = ["NN", "NT", "TN", "TT"]


def tile_and_chunk(xs, kind):
    L = xs.lib()
    return L.libxsmm_amd_gemm_tile(), L.libxsmm_amd_lowp_gemm_chunk(lg.precisions(xs, kind)[0])


@pytest.fixture(autouse=True)
def keep_mode(xs):
    before = xs.lib().libxsmm_amd_get_lowp_fast()
    yield
    xs.set_lowp_fast(before)


@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("kind", lg.KINDS)
def test_parity(xs, torch_gpu, kind, trans):
    T, kc = tile_and_chunk(xs, kind)
    shapes = [(1, 1, 1), (T, T, kc), (T + 1, T - 1, kc + 1), (130, 3, 70), (257, 129, 17)]
    for beta in (0, 1):
        for idx, (m, n, k) in enumerate(shapes):
            case = lg.Case(kind, trans, m, n, k, beta, pad=3, seed=100 * idx + 10 * beta + kind)
            got = case.run_device(xs, torch_gpu)
            assert xs.last_kernel() == lg.NAMES[kind] + trans.lower(), xs.last_kernel()
            assert lg.same_bits(got, case.gold), (kind, trans, beta, m, n, k, int(np.sum(lg.bits(got) != lg.bits(case.gold))))


@pytest.mark.parametrize("k", ["1", "3", "kc+1"])
def test_signed_zero_survives_the_k_tail(xs, torch_gpu, k):
    """bf16, beta = 1, C = -0.0 everywhere, B all zeros, A negative: every product is -0.0 and the sum stays -0.0, while a
    zero-padded matrix step through the accumulator, fma(0, 0, -0.0), would give +0.0"""
    T, kc = tile_and_chunk(xs, 2)
    k = {"1": 1, "3": 3, "kc+1": kc + 1}[k]
    m, n = T + 1, 33
    rng = np.random.default_rng(k)
    a = lg.rand_bf16(rng, m * k) | np.uint16(0x8000)
    b = np.zeros(k * n, dtype=np.uint16)
    c = np.full(m * n, -0.0, dtype=np.float32)
    case = lg.Case(2, "NN", m, n, k, 1, pad=0, a=a, b=b, c=c)
    got = case.run_device(xs, torch_gpu)
    assert lg.same_bits(got, c), int(np.sum(lg.bits(got) != lg.bits(c)))
    assert lg.same_bits(got, case.gold)


@pytest.mark.parametrize("kind", lg.KINDS)
def test_beta_zero_never_reads_c(xs, torch_gpu, kind):
    T, kc = tile_and_chunk(xs, kind)
    for trans, (m, n, k) in (("NN", (T + 1, 33, kc + 2)), ("TT", (33, T + 1, 3))):
        fill = np.full((m + 3) * n, 0x7fffffff, dtype=np.int32) if kind == 0 else np.full((m + 3) * n, np.nan, dtype=np.float32)
        case = lg.Case(kind, trans, m, n, k, 0, pad=3, seed=5, c=fill)
        got = case.run_device(xs, torch_gpu)
        assert lg.same_bits(got, case.gold)
        got = got.reshape(n, m + 3)
        if kind != 0:
            assert not np.isnan(got[:, :m]).any()
        assert lg.same_bits(got[:, m:], fill.reshape(n, m + 3)[:, m:])  # the padding keeps its bytes


@pytest.mark.parametrize("config", [(0, "TN"), (1, "NT"), (2, "NN")])
def test_tasks(xs, torch_gpu, config):
    kind, trans = config
    m, n, k = 300, 260, 40
    case = lg.Case(kind, trans, m, n, k, 1, pad=3, seed=11)
    single = case.run_device(xs, torch_gpu)
    assert lg.same_bits(single, case.gold)
    keep, h = xs.gemm_handle(xs.F32, xs.F32, "N", "N", m, n, 1)
    for nthreads in (1, 3, 4, 7):
        cover = np.zeros((n, m), dtype=np.int32)
        for tid in range(nthreads):
            rc, (m0, m1, n0, n1) = xs.gemm_task(h, tid, nthreads)
            assert rc == 0
            cover[n0:n1, m0:m1] += 1
            # one task alone: its rectangle, nothing else
            got = case.run_device(xs, torch_gpu, tasks=[(tid, nthreads)]).reshape(n, case.ldc)
            want = case.c.copy().reshape(n, case.ldc)
            want[n0:n1, m0:m1] = case.gold.reshape(n, case.ldc)[n0:n1, m0:m1]
            assert lg.same_bits(got, want), (nthreads, tid)
        assert (cover == 1).all()  # the tasks cover C and are disjoint
        order = np.random.default_rng(nthreads).permutation(nthreads)
        got = case.run_device(xs, torch_gpu, tasks=[(int(tid), nthreads) for tid in order])
        assert lg.same_bits(got, single), nthreads


@pytest.mark.parametrize("kind", lg.KINDS)
def test_memory_kinds(xs, torch_gpu, kind):
    torch = torch_gpu
    T, kc = tile_and_chunk(xs, kind)
    case = lg.Case(kind, "TN", T + 1, T + 5, kc + 3, 1, pad=3, seed=7)
    dev = case.run_device(xs, torch)
    host = case.c.copy()  # pageable numpy arrays: complete on return, all three tasks of three
    for tid in range(3):
        assert 0 == case.run(xs, case.a, case.b, host, tid, 3)
    pa, pb, pc = (torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x.copy()).pin_memory() for x in (case.a, case.b, case.c))
    assert 0 == case.run(xs, pa, pb, pc)  # host-pinned: complete on return
    pinned = pc.numpy().copy()
    da, _, _ = case.on_device(torch)
    mixed = case.c.copy()  # A on the device, B and C on the host
    assert 0 == case.run(xs, da, case.b, mixed)
    for got in (dev, host, pinned, mixed):
        assert lg.same_bits(got, case.gold)


def small_ints(rng, count):
    """bf16 bit patterns of integers in [-4, 4]"""
    v = rng.integers(-4, 5, count).astype(np.float32)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("trans", TRANS)
def test_fast_mode_is_exact_on_exact_sums(xs, torch_gpu, trans):
    """integers in [-4, 4], k <= 64: every partial sum is exact in any order, so the matrix instruction's own order and
    fragment layout must give the bits of the exact mode"""
    T, kc = tile_and_chunk(xs, 2)
    for k in (40, 17):
        m, n = T + 1, T - 1
        rng = np.random.default_rng(k)
        lda, ldb = (k if trans[0] == "T" else m) + 3, (n if trans[1] == "T" else k) + 3
        a = small_ints(rng, lda * (m if trans[0] == "T" else k))
        b = small_ints(rng, ldb * (k if trans[1] == "T" else n))
        c = rng.integers(-8, 9, (m + 3) * n).astype(np.float32)
        for beta in (0, 1):
            case = lg.Case(2, trans, m, n, k, beta, pad=3, a=a, b=b, c=c)
            exact = case.run_device(xs, torch_gpu)
            assert xs.last_kernel().startswith("tgemm_bf16_")
            xs.set_lowp_fast(True)
            fast = case.run_device(xs, torch_gpu)
            xs.set_lowp_fast(False)
            assert xs.last_kernel().startswith("tgemm_bf16fast_")
            assert lg.same_bits(exact, case.gold)
            assert lg.same_bits(fast, exact), (trans, k, beta, int(np.sum(lg.bits(fast) != lg.bits(exact))))


def test_fast_mode_error_bound_and_determinism(xs, torch_gpu):
    """random bf16 at 130 x 70 x 200 against the fp64 sum of the exact products. Bound per element: k * 2^-23 * sum |a_i b_i|,
    which holds for a k-term fp32 sum in any order if each internal add errs by at most 2^-23 relative (truncation allowed).
    The measured maximum of error over bound is printed, and written to the file LIBXSMM_AMD_LOWP_ERROR_FILE names
    (profiles/lowp_gemm_fast_error.txt is made that way)."""
    m, n, k = 130, 70, 200
    case = lg.Case(2, "NN", m, n, k, 0, pad=0, seed=23)
    A, B = lg.widen(lg.op(case.a, case.lda, m, k, False)).astype(np.float64), lg.widen(lg.op(case.b, case.ldb, k, n, False)).astype(np.float64)
    want, mag = A @ B, np.abs(A) @ np.abs(B)
    xs.set_lowp_fast(True)
    first = case.run_device(xs, torch_gpu)
    second = case.run_device(xs, torch_gpu)
    xs.set_lowp_fast(False)
    assert xs.last_kernel() == "tgemm_bf16fast_nn"
    assert lg.same_bits(first, second)  # two calls give identical bits
    err = np.abs(first.reshape(n, m).T.astype(np.float64) - want)
    bound = k * 2.0 ** -23 * mag
    ratio = float(np.max(err / bound))
    print("fast mode: max error / bound = %.6g (max abs error %.6g)" % (ratio, float(err.max())))
    out = os.environ.get("LIBXSMM_AMD_LOWP_ERROR_FILE")
    if out:
        with open(out, "w") as f:
            f.write("libxsmm_amd_lowp_gemm, BF16 -> F32, fast mode (v_mfma_f32_32x32x16_bf16), %d x %d x %d, NN, beta 0, random bf16\n" % (m, n, k))
            f.write("reference: fp64 sum of the exact products; bound per element: k * 2^-23 * sum |a_i * b_i|\n")
            f.write("max error / bound = %.6g\nmax abs error = %.6g\n" % (ratio, float(err.max())))
    assert ratio <= 1.0, ratio


def test_default_mode_is_exact(xs):
    assert "LIBXSMM_AMD_LOWP_FAST" not in os.environ
    assert xs.lib().libxsmm_amd_get_lowp_fast() == 0


def test_front_ends(xs, orc, torch_gpu):
    torch = torch_gpu
    for kind, fe, one, name in ((2, xs.bsgemm, 1.0, "smm_bf16f32"), (0, xs.wigemm, 1, "smm_i16i32"), (1, xs.wsgemm, 1.0, "smm_i16f32")):
        # small, even k, NN: the dispatched kernel, which reads A in pairs of k
        m, n, k = 24, 9, 10
        case = lg.Case(kind, "NN", m, n, k, 1, pad=3, seed=31 + kind)
        da, db, dc = case.on_device(torch)
        fe("N", "N", m, n, k, one, da, case.lda, db, case.ldb, one, dc, case.ldc)
        torch.cuda.synchronize()
        assert xs.last_kernel().startswith(name) and xs.last_kernel().endswith("_lowp"), xs.last_kernel()
        gold = case.c.copy()
        assert 0 == orc.gemm_lowp(kind, 0, m, n, k, case.lda, case.ldb, case.ldc, case.a, case.b, gold, 1.0)  # a as given: pairs of k
        assert lg.same_bits(dc.cpu().numpy(), gold)
        # above LIBXSMM_MAX_MNK, and a transposed product: the tiled kernel on plain operands
        for trans, (m, n, k), beta in (("NN", (70, 70, 70), 0), ("TN", (24, 9, 10), 1), ("NN", (24, 9, 11), None)):
            case = lg.Case(kind, trans, m, n, k, 1 if beta is None else beta, pad=3, seed=37 + kind)
            da, db, dc = case.on_device(torch)
            fe(trans[0], trans[1], m, n, k, None, da, case.lda, db, case.ldb, None if beta is None else type(one)(beta), dc, case.ldc)
            torch.cuda.synchronize()
            assert xs.last_kernel() == lg.NAMES[kind] + trans.lower(), xs.last_kernel()
            assert lg.same_bits(dc.cpu().numpy(), case.gold), (kind, trans, m, n, k)
        # alpha = 2 leaves C untouched
        before = xs.lib().libxsmm_amd_launch_count()
        fe("N", "N", m, n, k, type(one)(2), da, case.lda, db, case.ldb, one, dc, case.ldc)
        torch.cuda.synchronize()
        assert xs.lib().libxsmm_amd_launch_count() == before
        assert lg.same_bits(dc.cpu().numpy(), case.gold)


def test_call_order_inside_the_defer_bracket(xs, orc, torch_gpu):
    """dispatched kernel writes X -> libxsmm_amd_lowp_gemm adds a bf16 product to X -> dispatched kernel reads X: inside
    libxsmm_amd_defer_begin/end the low-precision GEMM seals the open burst, so the outcome is the chain of three calls"""
    torch = torch_gpu
    L = xs.lib()
    m = 32
    rng = np.random.default_rng(3)
    p, q, x, z = (rng.uniform(-1, 1, m * m).astype(np.float32) for _ in range(4))
    fn = L.libxsmm_smmdispatch(m, m, m, None, None, None, None, None, None, None)
    assert fn
    low = lg.Case(2, "NN", m, m, m, 1, pad=0, seed=4, c=x)
    gx, gz = x.copy(), z.copy()
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, p, q, gx)                                         # X += P * Q
    gx = lg.reference(2, False, False, m, m, m, low.a, m, low.b, m, 1, gx, m)              # X += A * B (bf16)
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, gx, q, gz)                                        # Z += X * Q

    def run(bracket):
        dp, dq, dx, dz = (torch.from_numpy(v.copy()).cuda() for v in (p, q, x, z))
        da, db, _ = low.on_device(torch)
        if bracket:
            xs.defer_begin()
        xs.call_kernel(fn, dp, dq, dx)
        assert 0 == low.run(xs, da, db, dx)
        xs.call_kernel(fn, dx, dq, dz)
        if bracket:
            xs.defer_end()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (dx, dz)]
    for bracket in (False, True):
        for got, gold in zip(run(bracket), (gx, gz)):
            assert lg.same_bits(got, gold), bracket


def test_example_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "lowp_gemm_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lowp_gemm_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "lowp_gemm_caller" in res.stdout
