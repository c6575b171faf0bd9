"""bench.py's contract: a plain run prints the headline fields and nothing that takes runs of its own (those come with --full);
--dump-outputs writes C after the last timed step, the same bits for the same arguments, and --steps / --warmup count the
launches that built it (beta = 1: every launch adds A*B to C once more)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tmp_path, steps, warmup, name):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--batch", "4096", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(out / "c.npy")


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(torch_gpu, tmp_path):
    line, c3 = bench(tmp_path, 2, 1, "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert not {"secondary", "cpu_baseline", "headline_variants"} & set(line) and "stream_probe_gbs" not in line["roofline"]
    assert c3.shape == (4096, 32 * 32) and c3.dtype == np.float32   # 16 MB: the whole array, no sample
    _, c3_again = bench(tmp_path, 3, 0, "b")
    assert np.array_equal(c3, c3_again)                             # same inputs, same number of launches: same bits
    _, c1 = bench(tmp_path, 1, 0, "c")
    _, c2 = bench(tmp_path, 2, 0, "d")
    step = c2.astype(np.float64) - c1
    assert np.abs(step).max() > 1.0                                 # a launch changes C ...
    assert np.allclose(c3 - c2.astype(np.float64), step, rtol=0, atol=1e-4)  # ... by the same A*B every time
