"""GEMM with 16-bit inputs, the part that needs no GPU: exported symbols, the header, argument errors (all of them before any
device probe), the fast-mode switch, and the numpy reference of the GPU tests against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lowp_gemm_common as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <libxsmm.h>
#include <libxsmm_amd.h>
int main(void) {
  const libxsmm_blasint m = 8;
  const int ione = 1; const float one = 1;
  short a[64] = { 0 }; libxsmm_bfloat16 b[64] = { 0 }; int ci[64] = { 0 }; float cf[64] = { 0 };
  libxsmm_wigemm("N", "N", &m, &m, &m, &ione, a, &m, a, &m, &ione, ci, &m);
  libxsmm_wsgemm("N", "T", &m, &m, &m, &one, a, &m, a, &m, &one, cf, &m);
  libxsmm_bsgemm("T", "N", &m, &m, &m, &one, b, &m, b, &m, &one, cf, &m);
  libxsmm_amd_set_lowp_fast(libxsmm_amd_get_lowp_fast());
  return libxsmm_amd_lowp_gemm(LIBXSMM_GEMM_PRECISION_BF16, LIBXSMM_GEMM_PRECISION_F32, 'N', 'N', m, m, m, b, m, b, m, 1, cf, m)
    + libxsmm_amd_lowp_gemm_thread(LIBXSMM_GEMM_PRECISION_I16, LIBXSMM_GEMM_PRECISION_I32, 'N', 'N', m, m, m, a, m, a, m, 1, ci, m, 0, 1);
}
"""


def test_symbols_are_exported(xs):
    L = C.CDLL(xs.LIB_PATH)
    for name in ("libxsmm_wigemm", "libxsmm_wsgemm", "libxsmm_bsgemm", "libxsmm_amd_lowp_gemm", "libxsmm_amd_lowp_gemm_thread",
                 "libxsmm_amd_set_lowp_fast", "libxsmm_amd_get_lowp_fast", "libxsmm_amd_lowp_gemm_chunk"):
        assert getattr(L, name)
    for name in ("gemm_lowp", "gemm_lowp_thread", "set_lowp_fast", "wigemm", "wsgemm", "bsgemm"):
        assert callable(getattr(xs, name))


def test_header_compiles_a_caller(tmp_path):
    src = tmp_path / "snippet.c"
    src.write_text(SNIPPET)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        res = subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                              "-o", str(tmp_path / "snippet.o")], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
xs = importlib.import_module("libxsmm-1_amd")
L = xs.lib()
a = np.zeros(64 * 64, np.uint16); c = np.zeros(64 * 64, np.float32)
ok = dict(iprec=xs.BF16, oprec=xs.F32, transa="N", transb="N", m=40, n=30, k=20, a=a, lda=40, b=a, ldb=20, beta=1, c=c, ldc=40)
def rc(**kw):
    return xs.gemm_lowp(**dict(ok, **kw))
bad = [dict(iprec=xs.F32), dict(oprec=xs.BF16), dict(iprec=xs.I16, oprec=xs.BF16), dict(iprec=xs.BF16, oprec=xs.I32), dict(iprec=xs.F64, oprec=xs.F64),
       dict(m=-1), dict(n=-1), dict(k=-1), dict(lda=39), dict(transa="T", lda=19), dict(ldb=19), dict(transb="T", ldb=29), dict(ldc=39),
       dict(a=None), dict(b=None), dict(c=None), dict(beta=2), dict(beta=-1), dict(transa="X"), dict(transb="C")]
for kw in bad:
    assert rc(**kw) != 0, kw
# a tid outside [0, nthreads) does nothing
for tid, nthreads in ((-1, 1), (1, 1), (3, 3), (0, 0)):
    assert xs.gemm_lowp_thread(tid=tid, nthreads=nthreads, **ok) != 0
# an empty product succeeds and does nothing
for kw in (dict(m=0), dict(n=0), dict(k=0)):
    assert rc(**kw) == 0, kw
assert not c.any()
# alpha and beta the front ends refuse: C stays as it is
xs.bsgemm("N", "N", 40, 30, 20, 2.0, a, 40, a, 20, 1.0, c, 40)
xs.wigemm("N", "N", 40, 30, 20, 1, a, 40, a, 20, 3, c, 40)
xs.wsgemm("N", "N", 40, 30, 20, None, a, 40, a, 20, 0.5, c, 40)
assert not c.any()
print("launches:", L.libxsmm_amd_launch_count(), "fast:", L.libxsmm_amd_get_lowp_fast())
"""


def run_child(env_extra):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", **env_extra)  # a probe would find no device and complain
    return subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)


def test_argument_errors_come_before_any_device_probe():
    res = run_child({})
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "launches: 0 fast: 0" in res.stdout
    assert "no HIP device" not in res.stderr and "LIBXSMM-AMD ERROR" not in res.stderr, res.stderr


def test_fast_mode_switch(xs):
    L = xs.lib()
    before = L.libxsmm_amd_get_lowp_fast()
    try:
        assert xs.set_lowp_fast(True) == before
        assert L.libxsmm_amd_get_lowp_fast() == 1
        assert xs.set_lowp_fast(False) == 1
        assert L.libxsmm_amd_get_lowp_fast() == 0
        assert L.libxsmm_amd_set_lowp_fast(7) == 0 and L.libxsmm_amd_get_lowp_fast() == 1
    finally:
        L.libxsmm_amd_set_lowp_fast(before)
    assert L.libxsmm_amd_lowp_gemm_chunk(xs.BF16) >= 16 and L.libxsmm_amd_lowp_gemm_chunk(xs.I16) >= 2
    assert L.libxsmm_amd_lowp_gemm_chunk(xs.F32) == 0


@pytest.mark.parametrize("value, want", [("1", 1), ("0", 0), ("", 0)])
def test_fast_mode_environment(value, want):
    res = run_child({"LIBXSMM_AMD_LOWP_FAST": value})
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "fast: %d" % want in res.stdout


@pytest.mark.parametrize("shape", [(5, 3, 4), (33, 17, 64)])
@pytest.mark.parametrize("kind", lg.KINDS)
def test_numpy_reference_equals_the_oracle(orc, kind, shape):
    """even k, no transpose: the oracle reads A in pairs of k, the reference reads the same matrix plain"""
    m, n, k = shape
    for beta in (0, 1):
        case = lg.Case(kind, "NN", m, n, k, beta, pad=3, seed=10 * kind + beta)
        gold = case.c.copy()
        assert 0 == orc.gemm_lowp(kind, 0 if beta else 1, m, n, k, case.lda, case.ldb, case.ldc, lg.pack_pairs(case.a, case.lda, m, k), case.b, gold, 1.0)
        assert lg.same_bits(case.gold, gold), (kind, shape, beta)
        assert not lg.same_bits(gold, case.c)
