"""examples/rnn_bwd_caller.c, written against the reference API only (include/libxsmm_dnn.h and include/libxsmm_dnn_rnncell.h as the
reference declares them), is compiled with gcc against include/ alone, linked against libxsmm.so and run on the GPU box: an LSTM and a
tanh cell, FWD and then BWDUPD over three steps on host tensors, every gradient checked against plain loops. It returns 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_rnn_bwd_caller_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "rnn_bwd_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rnn_bwd_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert res.stdout.count("rnn_bwd_caller: lstm") == 6 and res.stdout.count("rnn_bwd_caller: tanh") == 4 and res.stdout.count(" 0 mismatches") == 10
