"""examples/hash_caller.c, a caller written against the reference's hash and compare functions, compiled as C89 and run: host
buffers and device copies of them must give the same answers."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_caller(xs, torch_gpu, tmp_path):
    libdir, exe = os.path.dirname(xs.LIB_PATH), tmp_path / "hash_caller"
    subprocess.run(["gcc", "-std=c89", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "hash_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "hash_caller: device copies agree" in res.stdout and "hash_caller: ok (hash " in res.stdout and "found 617" in res.stdout
