"""Packs what the reference's libxsmm_matdiff and libxsmm_matdiff_reduce return into tests/golden/matdiff.npz (data only: per
case the 19 fields, m, n and the return value; per batch the same per item and for the reduced info).

    python tools/golden/matdiff_capture.py <matdiff_capture binary built from tools/golden/matdiff_capture.c against the reference>

The cases and their inputs are those of tests/matdiff_common.py: the inputs are regenerated from seeds and not stored."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matdiff_common as mc  # noqa: E402


def stored(tmp, name, x):
    if x is None:
        return "-"
    path = os.path.join(tmp, name)
    np.ascontiguousarray(x).tofile(path)
    return path


def main(exe):
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "out.bin")
    pack = {}
    for name, case in mc.cases().items():
        dt, m, n, ldr, ldt, ref, tst = mc.case_operands(case)
        subprocess.run([exe, "single"] + [str(v) for v in (dt, m, n, ldr, ldt)] + [stored(tmp, "ref.bin", ref), stored(tmp, "tst.bin", tst), out], check=True)
        pack[name] = np.fromfile(out, dtype=np.float64)
        assert pack[name].shape == (22,), name
    for name, case in mc.BATCHES.items():
        dt, m, n, ldr, ldt, sr, st, batch = case[:8]
        ref, tst = mc.batch_operands(case)
        subprocess.run([exe, "batch"] + [str(v) for v in (dt, m, n, ldr, ldt, sr, st, batch)] + [stored(tmp, "ref.bin", ref), stored(tmp, "tst.bin", tst), out], check=True)
        pack["batch_" + name] = np.fromfile(out, dtype=np.float64).reshape(batch + 1, 22)
    # the guard: the first call of the reference's own test gives the numbers its source states
    g = dict(zip(mc.FIELDS, pack["known_3x3_f64"][:19]))
    assert abs(g["norm1_abs"] - 1.83) < 3e-7 and abs(g["normi_abs"] - 2.44) < 2e-7 and abs(g["linf_abs"] - 0.93) < 4e-7, g
    np.savez_compressed(os.path.join(mc.GOLDEN, "matdiff.npz"), **pack)


if __name__ == "__main__":
    main(sys.argv[1])
