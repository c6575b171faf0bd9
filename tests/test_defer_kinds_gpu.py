"""Every kind of call the opt-in bracket libxsmm_amd_defer_begin/end records, one after the other inside ONE bracket: a burst of
per-call dense kernels, a recorded libxsmm_gemm_batch, recorded spmdm block calls, a burst of a packed kernel, a burst of
fsspmdm panel calls, a transposition (which asks for the stream), the dense kernel again, and a batch call inside an inner
bracket. At most one kind is open on a thread, and each is launched before the next begins (DESIGN.md, section 1;
libxsmm-1_amd/csrc/xsmm_defer.cpp: record_begin / record_flush) -- so every step here reads what the step before it wrote, and the
results must be the bits of the same calls outside the bracket (a launch per call; those paths are pinned to the oracle in
test_defer_gpu.py, test_batch_merge_gpu.py, test_sparse_gpu.py, test_packed_gpu.py and test_xcopy_gpu.py).

Only the public C-ABI is used. The two panel calls are issued from C (a Python loop may leave the helper thread time to seal
the burst between them)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import packed_common as pc

pytestmark = pytest.mark.gpu

PANELS_C = r"""
typedef void (*fnx)(const void*, const void*, void*);
void two_panels(fnx execute, const void* handle, const char* b, char* c, long long bytes)
{ execute(handle, b, c); execute(handle, b + bytes, c + bytes); }
"""

# libxsmm_amd_launch_count() over the bracketed sequence below. Measured by running this test on the commit BEFORE the open-record
# state of the bracket was unified (three thread-local flags, hand-written flush sequences): the refactoring must not change it.
# It is not derived from the code under test. (The same calls outside the bracket: 10; the panel pair is one launch inside.)
LAUNCHES_IN_BRACKET = 9


@pytest.fixture(scope="module")
def two_panels(tmp_path_factory):
    d = tmp_path_factory.mktemp("panels")
    (d / "panels.c").write_text(PANELS_C)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", str(d / "panels.c"), "-o", str(d / "panels.so")])
    lib = C.CDLL(str(d / "panels.so"))
    lib.two_panels.argtypes = [C.c_void_p] * 4 + [C.c_longlong]; lib.two_panels.restype = None
    return lib.two_panels


def test_every_kind_of_record_follows_every_other_in_one_bracket(xs, torch_gpu, two_panels):
    torch, L = torch_gpu, xs.lib()
    rng = np.random.default_rng(41)
    f32 = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    # dense 32^3: z += x * y
    x, y, z = f32(1024), f32(1024), f32(1024)
    dense = L.libxsmm_smmdispatch(32, 32, 32, None, None, None, None, None, None, None)
    assert dense
    # two-item batch of 23^3, device index arrays: A items out of z (495 + 529 = 1024), C items into the head of the spmdm A
    ia, ib, ic = (np.array(v, dtype=np.int32) for v in ((0, 495), (0, 529), (0, 529)))
    gb = f32(2 * 529)
    # spmdm M, N, K = 64, 32, 64: A (64 x 64, four entries in ten kept beyond the part the batch writes), B, C
    M, N, K = 64, 32, 64
    sa = f32(M * K); sa[1058:][rng.random(M * K - 1058) < 0.6] = 0.0
    sb, sc = f32(K * N), f32(M * N)
    # one pack of 8 x 8 x 8 pgemm (16 fp32 matrices interleaved: 1024 numbers per operand): A = head of the spmdm C, C = head of the operator's B
    packed = pc.Case(pc.PGEMM, np.float32, 8, 8, 8, nmat=xs.packed_width(4)).dispatch(xs)
    pb = f32(1024)
    # fsspmdm operator 35 x 35 on two panels of 48 columns
    OM, OK, ON = 35, 35, 48
    op = np.ascontiguousarray(np.where(rng.random((OM, OK)) < 0.15, rng.uniform(-1, 1, (OM, OK)), 0.0).astype(np.float32))
    fb, fc, ft = f32(OK * 2 * ON), f32(OM * 2 * ON), f32(OM * 2 * ON)
    hop = L.libxsmm_sfsspmdm_create(OM, ON, OK, OK, 2 * ON, 2 * ON, 1.0, 1.0, xs.dptr(op))
    assert hop
    execute = C.cast(L.libxsmm_sfsspmdm_execute, C.c_void_p)
    alpha, beta0 = C.c_float(1.0), C.c_float(0.0)

    def sequence(bracket):
        h = xs.SpmdmHandle(); slices = C.POINTER(xs.CSRSlice)()
        L.libxsmm_spmdm_init(M, N, K, 1, C.byref(h), C.byref(slices))
        assert L.libxsmm_spmdm_get_num_compute_blocks(C.byref(h)) == 1
        dx, dy, dz, dgb, dsa, dsb, dsc, dpb, dfb, dfc, dft = (torch.from_numpy(v.copy()).cuda() for v in (x, y, z, gb, sa, sb, sc, pb, fb, fc, ft))
        dia, dib, dic = (torch.from_numpy(v).cuda() for v in (ia, ib, ic))
        begin, end = (L.libxsmm_amd_defer_begin, L.libxsmm_amd_defer_end) if bracket else (lambda: None, lambda: None)
        batch = lambda: xs.gemm_batch(xs.F32, "N", "N", 23, 23, 23, 1.0, dz, 23, dgb, 23, 1.0, dsa, 23, 0, 4, dia, dib, dic, 2)
        torch.cuda.synchronize()
        n0 = L.libxsmm_amd_launch_count()
        begin()
        xs.call_kernel(dense, dx, dy, dz)                                                                     # 1. opens a burst
        batch()                                                                                               # 2. recorded; reads z
        L.libxsmm_spmdm_createSparseSlice_fp32_thread(C.byref(h), b"N", xs.dptr(dsa), slices, 0, 0, 1)        # 3. recorded; reads what 2 wrote
        L.libxsmm_spmdm_compute_fp32_thread(C.byref(h), b"N", b"N", C.byref(alpha), slices, xs.dptr(dsb), b"N", C.byref(beta0), xs.dptr(dsc), 0, 0, 1)
        xs.call_kernel(packed, dsc, dpb, dfb)                                                                 # 4. a burst; reads the spmdm C
        two_panels(execute, hop, dfb.data_ptr(), dfc.data_ptr(), ON * 4)                                      # 5. a panel burst; B = what 4 wrote
        xs.otrans(dft.data_ptr(), dfc.data_ptr(), 4, 2 * ON, OM, 2 * ON, OM)                                  # 6. asks for the stream
        xs.call_kernel(dense, dft, dy, dz)                                                                    # 7. the first kernel again
        begin()
        batch()                                                                                               # 8. reads z once more
        inner = L.libxsmm_amd_launch_count()
        end()
        inner = L.libxsmm_amd_launch_count() - inner                                                          # (c)
        end()                                                                                                 # 9.
        launches = L.libxsmm_amd_launch_count() - n0
        torch.cuda.synchronize()
        out = [t.cpu().numpy() for t in (dz, dsa, dsc, dfb, dfc, dft)]
        L.libxsmm_spmdm_destroy(C.byref(h))
        return out, launches, inner

    try:
        plain, launches_plain, _ = sequence(False)
        deferred, launches, inner = sequence(True)
    finally:
        L.libxsmm_sfsspmdm_destroy(hop)
    print("[defer kinds] launches: %d outside the bracket, %d inside, %d across the inner defer_end" % (launches_plain, launches, inner))
    for name, u, v, v0 in zip(("z", "spmdm A", "spmdm C", "operator B", "operator C", "transposed C"), plain, deferred, (z, sa, sc, fb, fc, ft)):
        assert not np.array_equal(u, v0), name  # (every step did write)
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), name                                     # (a)
    assert np.all(np.isfinite(deferred[0]))
    assert launches == LAUNCHES_IN_BRACKET, (launches, launches_plain)                                        # (b)
    assert inner == 0                                                                                         # (c)
