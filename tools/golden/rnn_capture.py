"""Packs what the reference's RNN cell layer returns into tests/golden/rnn.npz (data only): per case the desc with the sequence length
and the forget bias, the statuses, sizes and layouts of tools/golden/rnn_capture.c's META, and what FWD wrote: h, cs, i, f, o, ci, co
and, for the simple cells, the internal state z.

    python tools/golden/rnn_capture.py <rnn_capture binary built from tools/golden/rnn_capture.c against the reference>

The reference is a scratch copy built with `make BLAS=0 FORTRAN=0 STATIC=1 ECFLAGS=-fcommon`. The cases and their seeded inputs are
those of tests/rnn_common.py (captured_cases). Inputs are not stored: they are regenerated from their seeds and only their CRC-32 is
kept. An output above 1024 elements is kept as its CRC-32 only (equality is bitwise, so nothing is lost). The reference runs with
LIBXSMM_TARGET=hsw and threads = 1: the generic templates are the contract. Destinations start as 0xff bytes. The status cases are
not executed. rnn_common.UNCAPTURED_CASES are not captured at all: the reference ends with a segmentation fault on them."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnn_common as rc  # noqa: E402

NMETA = 710
SMALL = 1024  # elements: a larger output is stored as a checksum only


def capture(exe, tmp, d, files, run):
    prefix = os.path.join(tmp, "out")
    for suffix in ("meta",) + rc.OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            os.remove(prefix + "." + suffix)
    fb = "-" if d["forget_bias"] is None else repr(float(d["forget_bias"]))
    args = [exe] + [str(d[k]) for k in rc.DESC_FIELDS] + [str(d["seq"]), fb, str(run)] + files + [prefix]
    subprocess.run(args, env=dict(os.environ, LIBXSMM_TARGET="hsw"), check=True)
    out = {"meta": np.fromfile(prefix + ".meta", dtype=np.int64)}
    assert out["meta"].shape == (NMETA,)
    for suffix in rc.OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            out[suffix] = np.fromfile(prefix + "." + suffix, dtype=np.uint8)
    return out


def main(exe):
    tmp = tempfile.mkdtemp()
    pack = {}
    for name, d in rc.captured_cases().items():
        assert d["threads"] == 1
        pack[name + "/desc"] = np.array([d[k] for k in rc.DESC_FIELDS] + [d["seq"], d["seed"]], dtype=np.int64)
        pack[name + "/forget_bias"] = np.array([np.nan if d["forget_bias"] is None else d["forget_bias"]], dtype=np.float32)
        files = ["-"] * len(rc.INPUTS)
        with_data = name not in rc.STATUS_CASES
        crcs = np.full(len(rc.INPUTS) + len(rc.OUTPUTS), -1, dtype=np.int64)  # one array per case: inputs, then outputs; -1: not there
        if with_data:
            t = rc.inputs(name, d)
            for i, key in enumerate(rc.INPUTS):
                if key in t:
                    files[i] = os.path.join(tmp, key + ".bin")
                    t[key].tofile(files[i])
                    crcs[i] = rc.crc(t[key])
        out = capture(exe, tmp, d, files, 1 if with_data else 0)
        pack[name + "/meta"] = out["meta"]
        if not with_data:
            continue
        assert out["meta"][704] == 0, name
        for key in rc.written(d["cell"]):
            crcs[len(rc.INPUTS) + rc.OUTPUTS.index(key)] = rc.crc(out[key])
            if out[key].size // 4 <= SMALL:
                pack[name + "/" + key] = out[key]
        pack[name + "/crc"] = crcs
    # the guard: one pre-activation of the simple cell, recomputed naively in float64
    name = "seq_tanh"
    d = rc.COMPUTE_CASES[name]
    t = rc.inputs(name, d)
    got = pack[name + "/z"].view(np.float32).reshape(d["max_T"], d["N"], d["K"])
    want = t["b"][5] + t["w"].astype(np.float64)[:, 5] @ t["x"].astype(np.float64)[0, 3] + t["r"].astype(np.float64)[:, 5] @ t["hp"].astype(np.float64)[0, 3]
    assert abs(got[0, 3, 5] - want) <= 1e-5 * max(1.0, abs(want)), "the capture does not compute what it is believed to"
    path = os.path.join(rc.GOLDEN, "rnn.npz")
    np.savez_compressed(path, **pack)
    print("rnn.npz: %d bytes, %d cases" % (os.path.getsize(path), len(rc.captured_cases())))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
