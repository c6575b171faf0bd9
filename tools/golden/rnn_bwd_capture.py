"""Packs what the reference's RNN cell layer returns for BWD, UPD and BWDUPD into tests/golden/rnn_bwd.npz (data only): per case the
desc with the sequence length and the seed, the statuses, the CRC-32 of every input, and per kind every gradient tensor (dx, dcsp,
dhp, dw, dr, db) as its CRC-32, its bytes if it has at most 1024 elements, and whether the kind left it at its 0xff fill.

    python tools/golden/rnn_bwd_capture.py <rnn_bwd_capture binary built from tools/golden/rnn_bwd_capture.c against the reference>

The reference is a scratch copy built with `make BLAS=0 FORTRAN=0 STATIC=1 ECFLAGS=-fcommon`. The cases and their seeded inputs are
those of tests/rnn_bwd_common.py (captured_cases). The binary runs the reference's own FWD first; what it wrote is compared here with
the restatement's forward tensors (the special cases replace z or o afterwards). The reference runs with LIBXSMM_TARGET=hsw and
threads = 1: the generic templates are the contract. rnn_bwd_common.UNCAPTURED_CASES are not captured: the reference reads before a
tensor there."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnn_common as rc  # noqa: E402
import rnn_bwd_common as rb  # noqa: E402

SMALL = 1024  # elements: a larger output is stored as a checksum only
FILES = ("x", "hp", "csp", "w", "r", "b", "dh", "dcs")


def main(exe):
    tmp = tempfile.mkdtemp()
    pack = {}
    for name, d in rb.captured_cases().items():
        t = rb.inputs(name, d)
        pack[name + "/desc"] = np.array([d[k] for k in rc.DESC_FIELDS] + [d["seq"], d["seed"]], dtype=np.int64)
        paths = []
        for key in FILES:
            paths.append(os.path.join(tmp, key + ".bin") if key in t else "-")
            if key in t:
                t[key].tofile(paths[-1])
        plant = {"z": "-", "o": "-"}
        if name in rb.SPECIAL_CASES:
            key = "o" if d["cell"] == rc.LSTM else "z"
            plant[key] = os.path.join(tmp, "plant.bin")
            t[key].tofile(plant[key])
        prefix = os.path.join(tmp, "out")
        args = [exe] + [str(d[k]) for k in ("N", "C", "K", "max_T", "cell", "bn", "bc", "bk")] + [str(d["seq"])] + paths + [plant["z"], plant["o"], prefix]
        subprocess.run(args, env=dict(os.environ, LIBXSMM_TARGET="hsw"), check=True)
        meta = np.fromfile(prefix + ".meta.bin", dtype=np.int64)
        assert meta.shape == (5,) and meta[0] == rc.Handle(d).status and not meta[1:].any(), (name, meta)
        pack[name + "/meta"] = meta
        for key in rc.written(d["cell"]):  # the reference's own forward pass against the restatement's
            got = np.fromfile(prefix + ".fwd." + key, dtype=np.uint32)
            assert np.array_equal(got, t[key].reshape(-1).view(np.uint32)), (name, key)
        pack[name + "/in_crc"] = np.array([rc.crc(t[key]) for key in rb.read(d["cell"])], dtype=np.int64)
        for kind in rb.KINDS:
            crcs, untouched = [], []
            for key in rb.GRADS:
                got = np.fromfile("%s.%d.%s" % (prefix, kind, key), dtype=np.uint8)
                crcs.append(rc.crc(got))
                untouched.append(int(np.all(got == 0xff)))
                if got.size // 4 <= SMALL:
                    pack["%s/%d/%s" % (name, kind, key)] = got
            pack["%s/%d/crc" % (name, kind)] = np.array(crcs, dtype=np.int64)
            pack["%s/%d/untouched" % (name, kind)] = np.array(untouched, dtype=np.int64)
    path = os.path.join(rc.GOLDEN, "rnn_bwd.npz")
    np.savez_compressed(path, **pack)
    print("rnn_bwd.npz: %d bytes, %d cases" % (os.path.getsize(path), len(rb.captured_cases())))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
