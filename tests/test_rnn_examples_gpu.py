"""examples/rnn_caller.c, written against the reference API only (include/libxsmm_dnn.h and include/libxsmm_dnn_rnncell.h as the
reference declares them), is compiled with gcc against include/ alone, linked against libxsmm.so and run on the GPU box: an LSTM and a
GRU forward pass over three steps on host tensors, every element of h checked against plain loops. It returns 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_rnn_caller_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "rnn_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rnn_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "rnn_caller: lstm" in res.stdout and "rnn_caller: gru" in res.stdout and res.stdout.count(" 0 mismatches") == 2
