"""The LDS geometry of the generated dense SMM kernels (csrc/kernels/smm_jit_geom.h), checked without a GPU.

Host and generated kernels compile the same header, so a number can no longer differ between them; what is left to pin is
that the header compiles on both sides -- as strict host C++17, and as device text behind nothing but the HIP runtime
header hiprtc effectively provides -- and that its functions still give the numbers the launches were sized with before
the geometry moved there: the rows below are the values of the former host functions (smm_jit_wave_lds, smm_jit_wg_buf,
smm_mfma_wave_lds, smm_mfma_wave2_lds, smm_mfma_runs_lds, smm_jit_big_buf), taken at the shapes where a term switches.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "libxsmm-1_amd", "csrc", "kernels", "smm_jit_geom.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (expression, value): bytes unless the expression says otherwise; 0: the shape is not served
ROWS = [
    # register-tiled wave form -- tiled(typesize, m, n, k, TRANS_B, pack, XRUNS): fp64 / fp32 32^3 and 23^3 at pack 1
    ("geom::tiled(8, 32, 32, 32, false, 1, 0).wave_lds * 8", 25088),
    ("geom::tiled(4, 32, 32, 32, false, 1, 0).wave_lds * 4", 12544),
    ("geom::tiled(8, 23, 23, 23, false, 1, 0).wave_lds * 8", 13120),
    ("geom::tiled(4, 23, 23, 23, false, 1, 0).wave_lds * 4", 6560),
    # ... 13^3 at pack 4 (4 x 4 lanes per item), 5 x 7 x 3 at pack 16 (2 x 2)
    ("geom::tiled(8, 13, 13, 13, false, 4, 0).wave_lds * 8", 18080),
    ("geom::tiled(4, 13, 13, 13, false, 4, 0).wave_lds * 4", 9040),
    ("geom::tiled(8, 5, 7, 3, false, 16, 0).wave_lds * 8", 10624),
    ("geom::tiled(4, 5, 7, 3, false, 16, 0).wave_lds * 4", 5312),
    # ... TRANS_B (B's image is [k][n])
    ("geom::tiled(8, 23, 23, 23, true, 1, 0).wave_lds * 8", 13152),
    ("geom::tiled(4, 13, 23, 32, true, 2, 0).wave_lds * 4", 11936),
    # ... fp64, eight columns per lane (tn * typesize / 4 a multiple of 16): the odd-stride branch of kp, k odd and even
    ("geom::tiled(8, 13, 32, 13, false, 2, 0).wave_lds * 8", 16320),
    ("geom::tiled(8, 16, 32, 16, false, 2, 0).wave_lds * 8", 21248),
    # ... wave run form (C's image lies over the operands'): C larger than A + B, and smaller
    ("geom::tiled(8, 32, 32, 2, false, 1, 1).wave_lds * 8", 8192),
    ("geom::tiled(8, 32, 32, 32, false, 1, 1).wave_lds * 8", 16896),
    ("geom::tiled(4, 23, 23, 23, false, 1, 1).wave_lds * 4", 4432),
    # work-group form: an operand buffer, and whether two of them fit 64 KiB (fp64 32 x 32 x 64: 2 x 33280 do not)
    ("geom::tiled(8, 32, 32, 32, false, 1, 2).wg_buf * 8", 16896),
    ("geom::tiled(8, 32, 32, 32, false, 1, 2).wg_nbuf", 2),
    ("geom::tiled(8, 32, 32, 64, false, 1, 2).wg_buf * 8", 33280),
    ("geom::tiled(8, 32, 32, 64, false, 1, 2).wg_nbuf", 1),
    ("geom::tiled(4, 23, 23, 23, true, 1, 2).wg_buf * 4", 4480),
    ("geom::tiled(4, 23, 23, 23, true, 1, 2).wg_nbuf", 2),
    # matrix-core wave form -- mfma_wave(typesize, m, n, k, vec, TRANS_B): m and n at the steps of the image rows (16, 17, 48, 49, 64)
    ("geom::mfma_wave(4, 16, 16, 16, 4, false).lds_bytes", 2816),
    ("geom::mfma_wave(8, 16, 16, 16, 2, false).lds_bytes", 4864),
    ("geom::mfma_wave(4, 17, 17, 1, 1, false).lds_bytes", 1956),
    ("geom::mfma_wave(8, 17, 17, 1, 1, false).lds_bytes", 7720),
    ("geom::mfma_wave(4, 48, 48, 48, 4, false).lds_bytes", 20224),
    ("geom::mfma_wave(8, 48, 48, 48, 2, false).lds_bytes", 38144),
    ("geom::mfma_wave(4, 49, 49, 63, 1, false).lds_bytes", 29380),
    ("geom::mfma_wave(8, 49, 49, 63, 1, false).lds_bytes", 58760),
    ("geom::mfma_wave(4, 64, 64, 64, 4, false).lds_bytes", 35072),
    ("geom::mfma_wave(8, 64, 64, 64, 2, false).lds_bytes", 75264),
    ("geom::mfma_wave(4, 40, 40, 40, 4, true).lds_bytes", 15616),
    ("geom::mfma_wave(8, 33, 17, 63, 1, true).lds_bytes", 49664),
    # ... not served: m resp. (TRANS_B) n no multiple of the chunk, k beyond 64
    ("geom::mfma_wave(4, 18, 40, 40, 4, false).lds_bytes", 0),
    ("geom::mfma_wave(4, 40, 18, 40, 4, true).lds_bytes", 0),
    ("geom::mfma_wave(8, 40, 40, 65, 1, false).lds_bytes", 0),
    # ... the columns of C in two halves (fp64 56^3), n odd: not served
    ("geom::mfma_wave2(8, 56, 56, 56).lds_bytes", 38592),
    ("geom::mfma_wave2(8, 16, 64, 64).lds_bytes", 25600),
    ("geom::mfma_wave2(8, 56, 55, 56).lds_bytes", 0),
    # matrix-core run form -- mfma_runs_lds_bytes(typesize, m, n, k, ldb, streaming): k = 64 with ldb = 80; B's span beyond 2560
    # elements (ldb = 100, n = 32) and k beyond 64: not served
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 64, 80, false)", 16640),
    ("geom::mfma_runs_lds_bytes(4, 32, 32, 64, 80, false)", 8448),
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 32, 100, false)", 0),
    ("geom::mfma_runs_lds_bytes(8, 13, 13, 13, 0, false)", 1792),
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 65, 0, false)", 0),
    # ... streaming form: k in chunks from 65 up to 256
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 65, 0, true)", 6400),
    ("geom::mfma_runs_lds_bytes(4, 32, 32, 65, 0, true)", 3328),
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 256, 0, true)", 8448),
    ("geom::mfma_runs_lds_bytes(4, 13, 23, 256, 300, true)", 3136),
    ("geom::mfma_runs_lds_bytes(8, 32, 32, 257, 0, true)", 0),
    # work-group-per-item form -- big(typesize, m, n, kc): one of the two buffers of 64 x 64 at each chunk length
    ("geom::big(8, 64, 64, 32).buf * 8", 33280),
    ("geom::big(8, 64, 64, 16).buf * 8", 16640),
    ("geom::big(8, 64, 64, 8).buf * 8", 8320),
    ("geom::big(4, 64, 64, 32).buf * 4", 16896),
    ("geom::big(4, 64, 64, 16).buf * 4", 8448),
    ("geom::big(4, 64, 64, 8).buf * 4", 4224),
]


def _asserts():
    lines = ['static_assert(sizeof(DevAddr) == 96, "DevAddr");']
    lines += ['static_assert(%s == %d, "row %d");' % (expr, value, i) for i, (expr, value) in enumerate(ROWS)]
    return "\n".join(lines) + "\n"


def test_header_is_strict_host_cxx17(tmp_path):
    """included by a host translation unit: no warning under -Wall -Wextra, every row holds"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    assert cxx, "no host compiler"
    src = tmp_path / "geom_host.cpp"
    src.write_text('#include "%s"\n' % HEADER + _asserts())
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_is_device_text(tmp_path):
    """as the text in front of a generated kernel (no standard library, no include of its own), compiled for gfx950 the way
    test_handwait_invariant compiles the generated kernels: every row holds there as well"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not available here")
    with open(HEADER) as f:
        text = f.read()
    assert not re.search(r"^\s*#\s*include", text, re.M)
    hip, asm = tmp_path / "geom_device.hip", tmp_path / "geom_device.s"
    hip.write_text("#include <hip/hip_runtime.h>\n" + text + _asserts())
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", str(hip), "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_rows_can_fail(tmp_path):
    """the check is live: a row that is off by one element does not compile"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    src = tmp_path / "geom_off.cpp"
    src.write_text('#include "%s"\nstatic_assert(%s == %d, "off by one");\n' % (HEADER, ROWS[0][0], ROWS[0][1] + 8))
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "off by one" in r.stderr
