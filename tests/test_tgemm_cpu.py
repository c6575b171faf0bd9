"""Tiled GEMM, the part that needs no GPU: exported symbols, the header, the handle rules of libxsmm_gemm_handle_init and the
partition of C into task rectangles (libxsmm_amd_gemm_task)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <libxsmm.h>
#include <libxsmm_amd.h>
int main(void) {
  const libxsmm_blasint m = 8;
  const double one = 1;
  double a[64] = { 0 }, b[64] = { 0 }, c[64] = { 0 };
  libxsmm_gemm_blob blob;
  unsigned int rect[4];
  const libxsmm_gemm_handle_flags flags = LIBXSMM_GEMM_HANDLE_FLAG_AUTO;
  const libxsmm_gemm_handle* const h = libxsmm_gemm_handle_init(&blob, LIBXSMM_GEMM_PRECISION_F64, LIBXSMM_GEMM_PRECISION_F64,
    "N", "N", &m, &m, &m, &m, &m, &m, &one, &one, flags | LIBXSMM_GEMM_HANDLE_FLAG_COPY_A | LIBXSMM_GEMM_HANDLE_FLAG_COPY_B | LIBXSMM_GEMM_HANDLE_FLAG_COPY_C, 1);
  if (0 != h && 0 == libxsmm_gemm_handle_get_scratch_size(h) && 0 == libxsmm_amd_gemm_task(h, 0, 1, rect)) {
    libxsmm_gemm_thread(h, 0, a, b, c, 0, 1);
  }
  libxsmm_dgemm_omp("N", "N", &m, &m, &m, &one, a, &m, b, &m, &one, c, &m);
  return sizeof(float) == sizeof(&libxsmm_xgemm_omp) ? 1 : 0;
}
"""


def test_symbols_are_exported(xs):
    L = C.CDLL(xs.LIB_PATH)
    for name in ("libxsmm_gemm_handle_init", "libxsmm_gemm_handle_get_scratch_size", "libxsmm_gemm_thread", "libxsmm_xgemm_omp",
                 "libxsmm_amd_gemm_task"):
        assert getattr(L, name)


def test_header_compiles_a_caller(tmp_path):
    src = tmp_path / "snippet.c"
    src.write_text(SNIPPET)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        res = subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                              "-o", str(tmp_path / "snippet.o")], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_init_writes_only_inside_the_blob(xs):
    L = xs.lib()
    guard = 64
    buf = (C.c_ubyte * (guard + 128 + guard))(*([0xA5] * (2 * guard + 128)))
    blob = C.c_void_p(C.addressof(buf) + guard)
    h = L.libxsmm_gemm_handle_init(blob, xs.F64, xs.F64, b"N", b"T", xs.iptr(300), xs.iptr(200), xs.iptr(100), None, None, None, None, None, 7, 4)
    assert h == blob.value  # (the handle lives in the blob)
    raw = bytes(buf)
    assert raw[:guard] == b"\xA5" * guard and raw[guard + 128:] == b"\xA5" * guard
    assert raw[guard:guard + 128] != b"\xA5" * 128
    # plain data: a copy of the bytes is a handle as well
    copy = xs.GemmBlob.from_buffer_copy(raw[guard:guard + 128])
    assert xs.gemm_task(C.addressof(copy), 1, 3) == xs.gemm_task(h, 1, 3)
    assert xs.gemm_task(h, 0, 1) == (0, (0, 300, 0, 200))


def test_null_rules(xs):
    L = xs.lib()
    ok = dict(iprec=xs.F64, oprec=xs.F64, transa="N", transb="N", m=40, n=30, k=20)
    assert xs.gemm_handle(**ok)[1]
    blob = xs.GemmBlob()
    m = xs.iptr(40)
    assert not L.libxsmm_gemm_handle_init(None, xs.F64, xs.F64, b"N", b"N", m, m, m, None, None, None, None, None, 0, 1)  # NULL blob
    assert not L.libxsmm_gemm_handle_init(C.byref(blob), xs.F64, xs.F64, b"N", b"N", None, m, m, None, None, None, None, None, 0, 1)  # NULL m
    assert not xs.gemm_handle(**dict(ok, ntasks=0))[1]
    assert not xs.gemm_handle(**dict(ok, ntasks=-1))[1]
    assert not xs.gemm_handle(**dict(ok, m=0))[1]
    assert not xs.gemm_handle(**dict(ok, n=0))[1]
    assert not xs.gemm_handle(**dict(ok, k=0))[1]
    assert not xs.gemm_handle(**dict(ok, lda=39))[1]                 # NN: lda < m
    assert xs.gemm_handle(**dict(ok, lda=40))[1]
    assert not xs.gemm_handle(**dict(ok, transa="T", lda=19))[1]     # TN: lda < k
    assert xs.gemm_handle(**dict(ok, transa="T", lda=20))[1]
    assert not xs.gemm_handle(**dict(ok, ldb=19))[1]                 # NN: ldb < k
    assert not xs.gemm_handle(**dict(ok, transb="T", ldb=29))[1]     # NT: ldb < n
    assert not xs.gemm_handle(**dict(ok, ldc=39))[1]
    assert not xs.gemm_handle(**dict(ok, alpha=2.0))[1]
    assert not xs.gemm_handle(**dict(ok, beta=0.5))[1]
    assert xs.gemm_handle(**dict(ok, alpha=1.0, beta=0.0))[1]
    assert xs.gemm_handle(**dict(ok, iprec=xs.F32, oprec=xs.F32, alpha=1.0, beta=1.0))[1]
    assert not xs.gemm_handle(**dict(ok, iprec=xs.I16, oprec=xs.I32))[1]
    assert not xs.gemm_handle(**dict(ok, iprec=xs.BF16, oprec=xs.F32))[1]
    assert not xs.gemm_handle(**dict(ok, iprec=xs.F32, oprec=xs.F64))[1]
    for flags in (1, 2, 4, 7):  # the COPY_* flags are accepted
        assert xs.gemm_handle(**dict(ok, flags=flags))[1]


def test_defaults(xs):
    # NULL k: m; NULL n: k; NULL leading dimensions: tight (per transpose); NULL alpha, beta, transa, transb: 1, 1, 'N', 'N'
    keep, h = xs.gemm_handle(xs.F32, xs.F32, None, None, 300, None, None)
    assert h and xs.gemm_task(h, 0, 1) == (0, (0, 300, 0, 300))
    keep, h = xs.gemm_handle(xs.F32, xs.F32, None, None, 300, None, 17)
    assert h and xs.gemm_task(h, 0, 1) == (0, (0, 300, 0, 17))
    keep, h = xs.gemm_handle(xs.F32, xs.F32, "T", "T", 300, 20, 17, lda=17, ldb=20, ldc=300)
    assert h
    assert not xs.gemm_handle(xs.F32, xs.F32, "T", "T", 300, 20, 17, lda=16)[1]


def test_scratch_size_is_zero(xs):
    L = xs.lib()
    keep, h = xs.gemm_handle(xs.F64, xs.F64, "T", "N", 1000, 1000, 1000, flags=7, ntasks=16)
    assert h and 0 == L.libxsmm_gemm_handle_get_scratch_size(h)
    assert 0 == L.libxsmm_gemm_handle_get_scratch_size(None)


def test_task_arguments(xs):
    keep, h = xs.gemm_handle(xs.F64, xs.F64, "N", "N", 300, 200, 10)
    assert xs.gemm_task(None, 0, 1)[0] != 0
    for tid, nthreads in ((-1, 1), (1, 1), (3, 3), (0, 0)):
        rc, rect = xs.gemm_task(h, tid, nthreads)
        assert rc != 0 and rect[0] == rect[1]
    # a NULL handle or a tid outside [0, nthreads) does nothing (no device is asked for either)
    xs.lib().libxsmm_gemm_thread(None, None, None, None, None, 0, 1)
    xs.lib().libxsmm_gemm_thread(h, None, None, None, None, 5, 5)


@pytest.mark.parametrize("ntasks", [1, 5])
def test_partition_is_disjoint_and_covers_c(xs, ntasks):
    T = xs.lib().libxsmm_amd_gemm_tile()
    assert T >= 16
    for (m, n), nthreads in itertools.product(((1, 1), (129, 1), (1, 257), (300, 200), (1000, 37)), (1, 2, 3, 7, 16, 17, 64)):
        keep, h = xs.gemm_handle(xs.F32, xs.F32, "N", "T", m, n, 9, ntasks=ntasks)
        assert h
        cover = [[0] * n for _ in range(m)]
        area = 0
        for tid in range(nthreads):
            rc, (m0, m1, n0, n1) = xs.gemm_task(h, tid, nthreads)
            assert rc == 0
            if m0 == m1:
                continue  # a task without work
            assert m0 < m1 <= m and n0 < n1 <= n, (m, n, nthreads, tid)
            assert m0 % T == 0 and n0 % T == 0 and (m1 % T == 0 or m1 == m) and (n1 % T == 0 or n1 == n)  # cut on tile multiples
            area += (m1 - m0) * (n1 - n0)
            for i in range(m0, m1):
                row = cover[i]
                for j in range(n0, n1):
                    row[j] += 1
        assert area == m * n and all(v == 1 for row in cover for v in row), (m, n, nthreads)
