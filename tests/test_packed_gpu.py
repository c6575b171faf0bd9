"""Packed kernels on the GPU through the C-ABI (libxsmm_dispatch_pgemm / getrf / trmm / trsm, libxsmm_amd_packed_execute_batch, the
defer bracket): every result against the derived componentwise bounds of tests/packed_common.py and bit for bit against the ordered chain of the
CPU oracle (oracle/xsmm_oracle.c, xo_packed_*), memory that must stay untouched,
one answer whatever the entry point and the kernel form, the number of launches, and the C caller examples/packed_caller.c."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import packed_common as pc
from packed_common import PGEMM, GETRF, TRMM, TRSM, COL, ROW, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    return pc.build_loop(tmp_path_factory.mktemp("packloop"))


def run(xs, torch, case, mode, loop=None, fn=None, shift=0):
    """the case through one entry: 'batch' (libxsmm_amd_packed_execute_batch), 'loop' (kernel call per pack, device memory), 'bracket'
    (the same loop between defer_begin / defer_end), 'host' (kernel call per pack on host memory). shift: the device
    buffers start that many elements off their allocation (1: operands that are not 16-byte aligned). -> (buffers before, buffers after)"""
    L = xs.lib()
    fn = case.dispatch(xs) if fn is None else fn
    before = case.buffers(xs)
    npacks = case.nmat // xs.packed_width(case.dtype.itemsize)
    if mode == "host":
        after = {name: x.copy() for name, x in before.items()}
        a, b, c, sa, sb, sc = pc.call_args(case, {name: x.ctypes.data for name, x in after.items()})
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
        return before, after
    hold = {name: torch.zeros(len(x) + shift, dtype=torch.from_numpy(x).dtype, device="cuda") for name, x in before.items()}
    dev = {name: t[shift:] for name, t in hold.items()}
    for name, x in before.items():
        dev[name].copy_(torch.from_numpy(x))
    a, b, c, sa, sb, sc = pc.call_args(case, {name: t.data_ptr() for name, t in dev.items()})
    torch.cuda.synchronize()
    if mode == "batch":
        assert 0 == L.libxsmm_amd_packed_execute_batch(fn, a, b, c, npacks)
    elif mode == "loop":
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
    else:
        L.libxsmm_amd_defer_begin()
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
        L.libxsmm_amd_defer_end()
    assert 0 == L.libxsmm_amd_synchronize()
    return before, {name: t.cpu().numpy() for name, t in dev.items()}


def verify(xs, orc, case, before, after):
    """the derived bound, nothing else touched, and the written operand's whole buffer (canaries included) bit for bit the oracle's ordered
    chain (Case.chain: one fixed order per element, explicit fma, the rounded reciprocal of the pivot, alpha = +-1 without a rounding)"""
    out = case.result(xs, after[case.written])
    ratio, msg = case.check(out)
    print("%r: worst residual / bound = %.3f" % (case, ratio))
    assert msg is None, (case, msg)
    msg = case.untouched(xs, before, after)
    assert msg is None, (case, msg)
    want = case.chain(xs, orc)[case.written]
    bits = np.uint32 if case.dtype == np.float32 else np.uint64
    diff = np.flatnonzero(after[case.written].view(bits) != want.view(bits))
    assert diff.size == 0, (case, "%d elements differ from the oracle's chain; first at %d: %r, oracle %r" % (
        diff.size, int(diff[0]), after[case.written][diff[0]], want[diff[0]]))
    return out


@pytest.mark.parametrize("layout", [COL, ROW])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", [TRSM, TRMM])
def test_every_side_uplo_trans_diag(xs, orc, torch_gpu, kind, dtype, layout):
    """the sixteen flag combinations, each on a tight and a padded shape (packed_common.flag_sweep)"""
    for case in pc.flag_sweep(kind, dtype, layout):
        verify(xs, orc, case, *run(xs, torch_gpu, case, "batch"))


@pytest.mark.parametrize("layout", [COL, ROW])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", [TRSM, TRMM, GETRF])
def test_every_shape(xs, orc, torch_gpu, kind, dtype, layout):
    """every square size and the rectangular ones, tight and padded in turn, flags rotating (packed_common.shape_sweep)"""
    for case in pc.shape_sweep(kind, dtype, layout):
        verify(xs, orc, case, *run(xs, torch_gpu, case, "batch"))


@pytest.mark.parametrize("layout", [COL, ROW])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pgemm_every_trans_and_alpha(xs, orc, torch_gpu, dtype, layout):
    """packed_common.pgemm_sweep: every trans and alpha, then every shape once more with rotating flags"""
    for case in pc.pgemm_sweep(dtype, layout):
        verify(xs, orc, case, *run(xs, torch_gpu, case, "batch"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,m,n,k,kw", pc.ONE_ANSWER)
def test_one_answer_from_every_entry_and_form(xs, orc, torch_gpu, loop, monkeypatch, kind, m, n, k, kw, dtype):
    """1000 packs: per-call loop on device memory, the same loop inside the bracket, the batch entry, a per-call loop on host memory
    (fewer packs: it is staged call by call), and both kernel forms -- the same bits"""
    v = xs.packed_width(np.dtype(dtype).itemsize)
    case = pc.one_answer_case(kind, m, n, k, kw, dtype)
    assert case.nmat == 1000 * v
    fn = case.dispatch(xs)
    ref = verify(xs, orc, case, *run(xs, torch_gpu, case, "batch", fn=fn))
    for mode in ("loop", "bracket"):
        before, after = run(xs, torch_gpu, case, mode, loop, fn)
        assert np.array_equal(case.result(xs, after[case.written]), ref), (case, mode)
        assert case.untouched(xs, before, after) is None
    for form in ("1", "2"):  # LIBXSMM_AMD_PACKED_FORM: 1 = packs staged through LDS, 2 = lanes on global memory
        monkeypatch.setenv("LIBXSMM_AMD_PACKED_FORM", form)
        before, after = run(xs, torch_gpu, case, "batch", fn=fn)
        assert xs.last_kernel().endswith("_lds" if form == "1" else "_direct"), xs.last_kernel()
        assert np.array_equal(case.result(xs, after[case.written]), ref), (case, form)
        before, after = run(xs, torch_gpu, case, "bracket", loop, fn)
        assert np.array_equal(case.result(xs, after[case.written]), ref), (case, form, "bracket")
    monkeypatch.delenv("LIBXSMM_AMD_PACKED_FORM")
    small = Case(kind, dtype, m, n, k, nmat=9 * v, seed=11, layout=case.layout, **kw)
    small.ops = {name: np.ascontiguousarray(x[:9 * v]) for name, x in case.ops.items()}  # the first nine packs of the same matrices
    want = verify(xs, orc, small, *run(xs, torch_gpu, small, "batch", fn=fn))
    before, after = run(xs, torch_gpu, small, "host", loop, fn)
    assert np.array_equal(small.result(xs, after[small.written]), want)
    assert small.untouched(xs, before, after) is None
    assert np.array_equal(want, ref[:9 * v])  # (the same matrices: the batch size does not change a result either)


@pytest.mark.parametrize("layout", [COL, ROW])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,m,n,k,kw", pc.RESIDENT_CASES)
def test_register_resident_and_in_place_arithmetic_agree(xs, orc, torch_gpu, monkeypatch, kind, m, n, k, kw, dtype, layout):
    """one shape through the register-resident text and through the loops that large shapes run (LIBXSMM_AMD_PACKED_RESIDENT=0),
    each staged through LDS and on global memory: the same bits"""
    case = pc.resident_case(kind, m, n, k, kw, dtype, layout)
    fn = case.dispatch(xs)
    blob, d = xs.packed_descriptor(kind, case.dtype.itemsize, m, n, k)
    assert "#define RESIDENT 1" in xs.packed_kernel_source(kind, d)[1]
    monkeypatch.setenv("LIBXSMM_AMD_PACKED_RESIDENT", "0")
    assert "#define RESIDENT 0" in xs.packed_kernel_source(kind, d)[1]
    monkeypatch.delenv("LIBXSMM_AMD_PACKED_RESIDENT")
    ref = verify(xs, orc, case, *run(xs, torch_gpu, case, "batch", fn=fn))
    for resident, form in itertools.product(("1", "0"), ("1", "2")):
        monkeypatch.setenv("LIBXSMM_AMD_PACKED_RESIDENT", resident)
        monkeypatch.setenv("LIBXSMM_AMD_PACKED_FORM", form)
        before, after = run(xs, torch_gpu, case, "batch", fn=fn)
        assert np.array_equal(case.result(xs, after[case.written]), ref), (case, resident, form)
        assert case.untouched(xs, before, after) is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,m,n,k,kw", pc.UNALIGNED_CASES)
def test_operands_that_are_not_16_byte_aligned(xs, orc, torch_gpu, loop, monkeypatch, kind, m, n, k, kw, dtype):
    """operands one element off a 16-byte boundary take the form that works on global memory, whatever form is asked for -- in the
    batch entry, per call, and inside the bracket (such calls are not recorded) -- with the bits of the aligned run, nothing else touched"""
    case = pc.unaligned_case(kind, m, n, k, kw, dtype)
    fn = case.dispatch(xs)
    monkeypatch.setenv("LIBXSMM_AMD_PACKED_FORM", "1")
    ref = verify(xs, orc, case, *run(xs, torch_gpu, case, "batch", fn=fn))
    assert xs.last_kernel().endswith("_lds"), xs.last_kernel()
    for mode in ("batch", "loop", "bracket"):
        before, after = run(xs, torch_gpu, case, mode, loop, fn, shift=1)
        assert xs.last_kernel().endswith("_direct"), (mode, xs.last_kernel())
        assert np.array_equal(case.result(xs, after[case.written]), ref), (case, mode)
        assert case.untouched(xs, before, after) is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", [TRSM, TRMM, GETRF, PGEMM])
def test_bracketed_calls_that_write_one_operand_twice(xs, torch_gpu, loop, kind, dtype):
    """the packed overlap rule: a call of the same kernel whose written operand meets one the open burst writes seals the burst (there are
    no runs) -- the loop over the packs, twice over the same operands, equals the unbracketed sequence bit for bit"""
    torch, L = torch_gpu, xs.lib()
    v = xs.packed_width(np.dtype(dtype).itemsize)
    npacks = 40
    case = Case(kind, dtype, 8, 8, 8, diag="U", nmat=npacks * v, seed=9)  # (unit triangles: nothing grows in the second sweep)
    fn = case.dispatch(xs)
    results = []
    for bracket in (False, True):
        dev = {name: torch.from_numpy(x).cuda() for name, x in case.buffers(xs).items()}
        a, b, c, sa, sb, sc = pc.call_args(case, {name: t.data_ptr() for name, t in dev.items()})
        torch.cuda.synchronize()
        n0 = L.libxsmm_amd_launch_count()
        if bracket:
            L.libxsmm_amd_defer_begin()
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
        if bracket:
            L.libxsmm_amd_defer_end()
            assert 2 <= L.libxsmm_amd_launch_count() - n0 < npacks  # sealed between the two sweeps, not a launch per call
        L.libxsmm_amd_synchronize()
        results.append(dev[case.written].cpu().numpy())
    bits = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    assert np.array_equal(results[0].view(bits), results[1].view(bits))
    once = run(xs, torch_gpu, case, "batch", fn=fn)[1][case.written]
    assert not np.array_equal(once.view(bits), results[1].view(bits))  # (the second sweep did change the operand)


@pytest.mark.parametrize("kind", [TRSM, TRMM, GETRF, PGEMM])
def test_launches(xs, torch_gpu, loop, kind):
    """a batch call of 1000 packs is one launch; 1000 bracketed per-call invocations on contiguous packs cost what a burst of three costs"""
    torch, L = torch_gpu, xs.lib()
    v = 8
    counts = {}
    for npacks in (3, 1000):
        case = Case(kind, np.float64, 8, 8, 8, nmat=npacks * v, seed=1)
        fn = case.dispatch(xs)
        run(xs, torch, case, "batch", fn=fn)  # (compiled)
        dev = {name: torch.from_numpy(x).cuda() for name, x in case.buffers(xs).items()}
        a, b, c, sa, sb, sc = pc.call_args(case, {name: t.data_ptr() for name, t in dev.items()})
        torch.cuda.synchronize()
        n0 = L.libxsmm_amd_launch_count()
        assert 0 == L.libxsmm_amd_packed_execute_batch(fn, a, b, c, npacks)
        assert L.libxsmm_amd_launch_count() - n0 == 1
        L.libxsmm_amd_synchronize()
        n0 = L.libxsmm_amd_launch_count()
        L.libxsmm_amd_defer_begin()
        loop.pack_loop(fn, a, b, c, sa, sb, sc, npacks)
        L.libxsmm_amd_defer_end()
        counts[npacks] = L.libxsmm_amd_launch_count() - n0
        assert xs.last_kernel().endswith("_deferred"), xs.last_kernel()
        L.libxsmm_amd_synchronize()
    assert counts[1000] == counts[3] == 1, counts  # (the gate and the kernel behind it are noted as one launch, as for SMM bursts)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bracketed_getrf_then_trsm_on_its_factor(xs, torch_gpu, loop, dtype):
    """a call whose operand overlaps what the open burst writes seals it: LU, then the solve with the factor just written, both inside the
    bracket, equals the unbracketed sequence bit for bit"""
    torch, L = torch_gpu, xs.lib()
    v = xs.packed_width(np.dtype(dtype).itemsize)
    npacks = 40
    lu = Case(GETRF, dtype, 8, 8, nmat=npacks * v, seed=5)
    solve = Case(TRSM, dtype, 8, 4, side="L", uplo="L", diag="U", nmat=npacks * v, seed=6)
    f_lu, f_solve = lu.dispatch(xs), solve.dispatch(xs)
    results = []
    for bracket in (False, True):
        da = torch.from_numpy(lu.buffers(xs)["a"]).cuda()
        db = torch.from_numpy(solve.buffers(xs)["b"]).cuda()
        pa, pb = da.data_ptr() + pc.GUARD * da.element_size(), db.data_ptr() + pc.GUARD * db.element_size()
        sa, sb = lu.pack_elems("a") * da.element_size(), solve.pack_elems("b") * db.element_size()
        torch.cuda.synchronize()
        if bracket:
            L.libxsmm_amd_defer_begin()
        loop.pack_loop(f_lu, pa, pa, None, sa, sa, 0, npacks)
        loop.pack_loop(f_solve, pa, pb, None, sa, sb, 0, npacks)
        if bracket:
            L.libxsmm_amd_defer_end()
        L.libxsmm_amd_synchronize()
        results.append((da.cpu().numpy(), db.cpu().numpy()))
    bits = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    assert np.array_equal(results[0][0].view(bits), results[1][0].view(bits))
    assert np.array_equal(results[0][1].view(bits), results[1][1].view(bits))
    x = xs.unpack(results[1][1][pc.GUARD:-pc.GUARD], npacks * v, 8, 4, 8, COL)
    assert np.all(np.isfinite(x))
    # and it is the solve with the unit-lower factor: L x = b within the trsm bound, L taken from the LU result
    solve.ops["a"] = xs.unpack(results[1][0][pc.GUARD:-pc.GUARD], npacks * v, 8, 8, 8, COL)
    ratio, msg = solve.check(x)
    assert msg is None, msg


def test_kinds_and_redispatch(xs, orc, torch_gpu):
    L = xs.lib()
    for kind, want in ((PGEMM, 3), (GETRF, 4), (TRMM, 5), (TRSM, 6)):
        case = pc.redispatch_case(kind)
        fn = case.dispatch(xs)
        got = C.c_int(-1)
        assert 0 == L.libxsmm_get_kernel_kind(fn, C.byref(got)) and got.value == want
        verify(xs, orc, case, *run(xs, torch_gpu, case, "batch", fn=fn))
        L.libxsmm_release_kernel(fn)
        fn2 = case.dispatch(xs)
        verify(xs, orc, case, *run(xs, torch_gpu, case, "batch", fn=fn2))
    fn = L.libxsmm_smmdispatch(4, 4, 4, None, None, None, None, None, None, None)
    got = C.c_int(-1)
    assert 0 == L.libxsmm_get_kernel_kind(fn, C.byref(got)) and got.value == 0


def test_packed_c_caller_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    """examples/packed_caller.c: written against the reference API only, compiled as C, linked against libxsmm.so"""
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "packed_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "packed_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "packed_caller" in res.stdout
