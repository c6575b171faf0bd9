"""Packed kernels (libxsmm_dispatch_pgemm / getrf / trmm / trsm), everything that needs no device: descriptor layouts against the
reference's packed structs (src/libxsmm_main.h:193-226, offsets written out here), the rules of the initialisers and of dispatch,
the generated kernel text (it compiles for gfx950, the register-resident forms have no private segment), pack / unpack, and the
error bounds of tests/packed_common.py checked against a plain numpy implementation before any GPU is involved."""
import ctypes as C
import itertools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import packed_common as pc
from packed_common import PGEMM, GETRF, TRMM, TRSM, COL, ROW, Case


def _bytes(blob):
    return bytes(blob.data) if isinstance(blob.data, bytes) and len(blob.data) == 64 else C.string_at(C.addressof(blob), 64)


def test_descriptor_layouts(xs):
    # pgemm: m n k lda ldb ldc (u32 at 0..20), typesize 24, layout 25, transa 26, transb 27, alpha_val 28 -- 29 bytes
    blob, d = xs.packed_descriptor(PGEMM, 8, 5, 6, 7, lda=9, ldb=10, ldc=11, alpha=-1.0, transa="T", transb="N", layout=ROW)
    raw = _bytes(blob)
    assert d == C.addressof(blob)
    assert struct.unpack_from("<6I", raw, 0) == (5, 6, 7, 9, 10, 11)
    assert raw[24] == 8 and raw[25] == 101 and raw[26:28] == b"TN" and raw[28] == 1 and raw[29:] == bytes(35)
    blob, d = xs.packed_descriptor(PGEMM, 4, 5, 6, 7, alpha=1.0)
    assert _bytes(blob)[28] == 0 and _bytes(blob)[24] == 4
    # getrf: m n lda (u32 at 0..8), typesize 12, layout 13 -- 14 bytes
    blob, d = xs.packed_descriptor(GETRF, 4, 13, 8, lda=20, layout=COL)
    raw = _bytes(blob)
    assert struct.unpack_from("<3I", raw, 0) == (13, 8, 20) and raw[12] == 4 and raw[13] == 102 and raw[14:] == bytes(50)
    # trmm / trsm: alpha (union double / float at 0), m n lda ldb (u32 at 8..20), typesize 24, layout 25, diag 26, side 27, uplo 28, transa 29 -- 30 bytes
    for kind in (TRMM, TRSM):
        blob, d = xs.packed_descriptor(kind, 8, 3, 5, lda=7, ldb=9, alpha=0.75, transa="T", diag="U", side="R", uplo="L", layout=COL)
        raw = _bytes(blob)
        assert struct.unpack_from("<d", raw, 0) == (0.75,)
        assert struct.unpack_from("<4I", raw, 8) == (3, 5, 7, 9)
        assert raw[24] == 8 and raw[25] == 102 and raw[26:30] == b"URLT" and raw[30:] == bytes(34)
        blob, d = xs.packed_descriptor(kind, 4, 3, 5, alpha=-2.5)
        raw = _bytes(blob)
        assert struct.unpack_from("<f", raw, 0) == (-2.5,) and raw[4:8] == bytes(4)
    # dimensions are stored in full (the reference's initialisers narrow them modulo 256)
    blob, d = xs.packed_descriptor(GETRF, 8, 300, 2, lda=1000)
    assert struct.unpack_from("<3I", _bytes(blob), 0) == (300, 2, 1000)


def test_pgemm_init_rejects_other_alpha(xs):
    for ts in (4, 8):
        for alpha, ok in ((1.0, True), (-1.0, True), (2.0, False), (0.0, False), (0.5, False), (None, True)):
            blob, d = xs.packed_descriptor(PGEMM, ts, 4, 4, 4, alpha=alpha)
            assert bool(d) == ok, (ts, alpha)


def test_width_and_unsupported_dispatch(xs):
    assert xs.packed_width(8) == 8 and xs.packed_width(4) == 16 and xs.packed_width(2) == 0
    L = xs.lib()
    for f in (L.libxsmm_dispatch_pgemm, L.libxsmm_dispatch_getrf, L.libxsmm_dispatch_trmm, L.libxsmm_dispatch_trsm):
        assert not f(None)
    bad = [(GETRF, dict(typesize=8, m=33, n=4)), (GETRF, dict(typesize=8, m=4, n=0)), (GETRF, dict(typesize=2, m=4, n=4)),
           (GETRF, dict(typesize=8, m=4, n=4, lda=3)), (GETRF, dict(typesize=8, m=4, n=4, layout=100)),
           (TRSM, dict(typesize=4, m=4, n=4, side="X")), (TRSM, dict(typesize=4, m=4, n=4, uplo="Q")), (TRSM, dict(typesize=4, m=40, n=4)),
           (TRMM, dict(typesize=8, m=4, n=4, diag="Z")), (TRMM, dict(typesize=8, m=4, n=6, side="R", lda=5)),
           (PGEMM, dict(typesize=8, m=4, n=4, k=64)), (PGEMM, dict(typesize=8, m=4, n=4, k=4, transa="C"))]
    for kind, kw in bad:
        blob, d = xs.packed_descriptor(kind, kw.pop("typesize"), kw.pop("m"), kw.pop("n"), **kw)
        assert d and not xs.packed_dispatch(kind, d), (kind, kw)
    # inside the domain: a function pointer, the same one for the same descriptor, known by its kind
    for kind, want in ((PGEMM, 3), (GETRF, 4), (TRMM, 5), (TRSM, 6)):
        blob, d = xs.packed_descriptor(kind, 8, 5, 4, 3)
        fn = xs.packed_dispatch(kind, d)
        assert fn and fn == xs.packed_dispatch(kind, d)
        got = C.c_int(-1)
        assert 0 == L.libxsmm_get_kernel_kind(fn, C.byref(got)) and got.value == want
        L.libxsmm_release_kernel(fn)  # a registered kernel stays
        assert fn == xs.packed_dispatch(kind, d)
    fn = L.libxsmm_dmmdispatch(4, 4, 4, None, None, None, None, None, None, None)
    got = C.c_int(-1)
    assert 0 == L.libxsmm_get_kernel_kind(fn, C.byref(got)) and got.value == 0


SOURCES = [  # (kind, m, n, k, flags): one register-resident and one large shape of every kind
    (TRSM, 8, 8, 0, dict()), (TRSM, 32, 32, 0, dict(side="R", uplo="U", transa="T", alpha=0.5)),
    (TRMM, 8, 5, 0, dict(diag="U")), (TRMM, 32, 23, 0, dict(uplo="U")),
    (GETRF, 8, 8, 0, dict()), (GETRF, 32, 32, 0, dict()),
    (PGEMM, 8, 8, 8, dict(alpha=-1.0)), (PGEMM, 32, 32, 32, dict(transa="T", transb="T")),
]


@pytest.mark.parametrize("layout", [COL, ROW])
@pytest.mark.parametrize("typesize", [8, 4])
@pytest.mark.parametrize("kind,m,n,k,flags", SOURCES)
def test_generated_source_compiles(xs, kind, m, n, k, flags, typesize, layout):
    blob, d = xs.packed_descriptor(kind, typesize, m, n, k, layout=layout, **flags)
    size, text = xs.packed_kernel_source(kind, d, compile=0)
    assert size == len(text) and "xsmm_packed_op" in text
    resident = int(re.search(r"#define RESIDENT (\d)", text).group(1))
    assert resident == (1 if max(m, n) <= 8 else 0)
    rc, _ = xs.packed_kernel_source(kind, d, compile=1)
    assert rc == 0


@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("typesize,kind,m,n,k", [(8, TRSM, 10, 10, 0), (4, TRSM, 15, 15, 0), (8, TRMM, 10, 7, 0), (4, TRMM, 15, 16, 0),
                                                  (8, GETRF, 8, 8, 0), (4, GETRF, 11, 11, 0), (8, PGEMM, 8, 8, 8), (4, PGEMM, 11, 11, 11)])
def test_register_resident_forms_have_no_scratch(xs, tmp_path, monkeypatch, typesize, kind, m, n, k, form):
    """the largest register-resident shapes of every kind: a spilled per-lane matrix would silently be a memory-bound kernel of another kind"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    monkeypatch.setenv("LIBXSMM_AMD_PACKED_FORM", form)
    blob, d = xs.packed_descriptor(kind, typesize, m, n, k)
    _, text = xs.packed_kernel_source(kind, d, compile=0)
    assert "#define RESIDENT 1" in text and ("#define FORM %s" % form) in text
    src = tmp_path / "k.hip"
    src.write_text(text)
    out = tmp_path / "k.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-include", "hip/hip_runtime.h", "-x", "hip",
                    str(src), "-o", str(out)], check=True, capture_output=True)
    asm = out.read_text()
    assert re.search(r"\.private_segment_fixed_size:\s*0\b", asm), re.findall(r"\.private_segment_fixed_size:.*", asm)
    assert re.search(r"\.vgpr_spill_count:\s*0\b", asm)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", [COL, ROW])
def test_pack_unpack_round_trip(xs, dtype, layout):
    rng = np.random.default_rng(1)
    v = xs.packed_width(np.dtype(dtype).itemsize)
    for nmat, rows, cols, pad in ((v, 3, 5, 0), (3 * v, 8, 2, 4), (2 * v + 1, 1, 1, 0)):
        x = rng.random((nmat, rows, cols)).astype(dtype)
        ld = (rows if layout == COL else cols) + pad
        p = xs.pack(x, ld, layout, fill=-7)
        npacks = -(-nmat // v)
        assert p.shape == (npacks * ld * (cols if layout == COL else rows) * v,)
        # element (i, j) of matrix w of pack q where the interface says it is
        for (q, w, i, j) in ((0, 0, 0, 0), (npacks - 1, (nmat - 1) % v, rows - 1, cols - 1), (0, v - 1, rows // 2, cols // 2)):
            at = (i + j * ld) if layout == COL else (j + i * ld)
            assert p[q * ld * (cols if layout == COL else rows) * v + at * v + w] == x[q * v + w, i, j]
        assert np.array_equal(xs.unpack(p, nmat, rows, cols, ld, layout), x)
        assert np.count_nonzero(p == -7) == p.size - npacks * v * rows * cols + (npacks * v - nmat) * rows * cols


FLAGS = list(itertools.product("LR", "LU", "NT", "NU"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounds_hold_for_plain_numpy(dtype):
    """the harness against itself: the numpy implementation in the kernel's type meets every bound, a perturbed result does not"""
    seed = 0
    for kind in (TRSM, TRMM):
        for i, (side, uplo, trans, diag) in enumerate(FLAGS):
            m, n = ((5, 8), (13, 3), (16, 16), (1, 23), (32, 2))[i % 5]
            case = Case(kind, dtype, m, n, side=side, uplo=uplo, transa=trans, diag=diag, alpha=(1.0, -1.0, 0.75)[i % 3], nmat=16, seed=seed)
            seed += 1
            ratio, msg = case.check(case.reference())
            assert msg is None and ratio <= 1.0, (case, ratio, msg)
    for m, n in ((1, 1), (8, 8), (13, 5), (5, 13), (32, 32)):
        case = Case(GETRF, dtype, m, n, nmat=16, seed=seed)
        ratio, msg = case.check(case.reference())
        assert msg is None, (case, ratio, msg)
    for (ta, tb, alpha), (m, n, k) in zip(itertools.product("NT", "NT", (1.0, -1.0)), ((1, 1, 1), (8, 8, 8), (3, 5, 13), (32, 2, 16), (16, 23, 32), (2, 2, 2), (5, 5, 1), (13, 16, 8))):
        case = Case(PGEMM, dtype, m, n, k, transa=ta, transb=tb, alpha=alpha, nmat=16, seed=seed)
        ratio, msg = case.check(case.reference())
        assert msg is None, (case, ratio, msg)
    # the check has teeth: a relative error of 64 u in one element is found
    case = Case(TRSM, dtype, 8, 8, nmat=16, seed=3)
    out = case.reference()
    out[5, 0, 0] *= 1 + 64 * np.finfo(dtype).eps
    assert case.check(out)[1] is not None
    out = case.reference(); out[2, 1, 1] = np.nan
    assert case.check(out)[1] is not None


def test_exact_fallback_agrees(monkeypatch):
    """where numpy.longdouble is no wider than float64 the fp64 residuals are evaluated exactly: the same verdicts"""
    monkeypatch.setattr(pc, "LONGDOUBLE_IS_WIDER", False)
    for kind, kw in ((TRSM, dict(side="R", uplo="U")), (TRMM, dict(diag="U")), (GETRF, {}), (PGEMM, dict(k=4))):
        case = Case(kind, np.float64, 4, 5, nmat=8, seed=7, **kw)
        out = case.reference()
        assert case.check(out)[1] is None
        out[0, 0, 0] *= 1 + 2.0 ** -44
        assert case.check(out)[1] is not None
