"""examples/dnn_copy_caller.c, written against the reference API only (include/libxsmm_dnn.h as the reference declares it), is
compiled with gcc against include/ alone, linked against libxsmm.so and run on the GPU box: copy-in of input, filter and bias
from NCHW / KCRS, a FWD pass of a convolution layer with the bias fused, copy-out, checked exactly against a plain-C convolution
over the plain buffers. It returns 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_dnn_copy_caller_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "dnn_copy_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "dnn_copy_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "dnn_copy_caller:" in res.stdout and " 0 mismatches" in res.stdout
