"""Packs what the reference's pooling layer returns into tests/golden/pool.npz (data only): per case the desc, the create status,
the layouts of eight tensor types with their sizes (the error statuses of a filter type and of an NHWC mask among them), the
scratch size and the bind statuses, the status of execute_st for every kind, and the outputs of FWD (output and mask, the mask
pre-filled with -1) and BWD.

    python tools/golden/pool_capture.py <pool_capture binary built from tools/golden/pool_capture.c against the reference>

The cases and their seeded inputs are those of tests/pool_common.py (captured_cases). Inputs are not stored: they are
regenerated from their seeds and only their CRC-32 is kept. An output above 8192 elements is kept as its CRC-32 only
(equality is bitwise, so nothing is lost). The reference runs with LIBXSMM_TARGET=hsw: the generic templates are the contract
(the AVX-512 ones fuse the multiply-add of the average BWD and compare differently). BWD of a max pooling whose mask still
holds a -1 is not run (pool_capture.c), and the cases of pool_common.NO_RUN are not executed at all."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pool_common as pc  # noqa: E402

NMETA = 226
SMALL = 8192  # elements: a larger output is stored as a checksum only
OUTPUTS = ("out", "mask", "din")


def capture(exe, tmp, name, d, files, run):
    prefix = os.path.join(tmp, "out")
    for suffix in ("meta",) + OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            os.remove(prefix + "." + suffix)
    unbound = sum(1 << pc.BINDABLE.index(t) for t in pc.UNBOUND.get(name, ()))
    args = [exe] + [str(d[k]) for k in pc.DESC_FIELDS] + [str(unbound), str(run)] + files + [prefix]
    subprocess.run(args, env=dict(os.environ, LIBXSMM_TARGET="hsw"), check=True)
    out = {"meta": np.fromfile(prefix + ".meta", dtype=np.int64)}
    assert out["meta"].shape == (NMETA,)
    for suffix in OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            out[suffix] = np.fromfile(prefix + "." + suffix, dtype=np.uint8)
    return out


def main(exe):
    tmp = tempfile.mkdtemp()
    pack = {}
    for name, d in pc.captured_cases().items():
        h = pc.Handle(d)
        pack[name + "/desc"] = np.array([d[k] for k in pc.DESC_FIELDS], dtype=np.int64)
        files = ["-", "-"]
        run = int(name not in pc.NO_RUN)
        if h.ok and h.runnable() and d["buffer_format"] == pc.FMT_LIBXSMM:
            x, dout = pc.inputs(name, d)
            files = []
            for key, a in (("x", x), ("dout", dout)):
                path = os.path.join(tmp, key + ".bin")
                np.ascontiguousarray(a).tofile(path)
                files.append(path)
                pack[name + "/crc_" + key] = np.array([pc.crc(a)], dtype=np.int64)
        out = capture(exe, tmp, name, d, files, run)
        pack[name + "/meta"] = out["meta"]
        executed = out["meta"][220:222]
        for key in OUTPUTS:
            if key not in out or files[0] == "-":
                continue
            if (key == "din" and executed[1] != 0) or (key != "din" and executed[0] != 0):
                continue  # (the pass did not run: the destination is still its fill)
            if key == "mask" and d["pooling_type"] != pc.MAX:
                continue
            pack[name + "/crc_" + key] = np.array([pc.crc(out[key])], dtype=np.int64)
            if out[key].size // (4 if (h.f32 or key == "mask") else 2) <= SMALL:
                pack[name + "/" + key] = out[key]
    # the guard: a 2x2 / 2 max pooling of the seeded input, recomputed naively for one item
    name = "c_max_f32_n"
    x = pc.inputs(name, pc.COMPUTE_CASES[name])[0]
    got = pack[name + "/out"].view(np.float32).reshape(4, 4, 4, 16)
    assert np.array_equal(got[1], x[1].reshape(4, 2, 4, 2, 16).max(axis=(1, 3))), "the capture does not compute what it is believed to"
    np.savez_compressed(os.path.join(pc.GOLDEN, "pool.npz"), **pack)
    print("pool.npz: %d bytes, %d cases" % (os.path.getsize(os.path.join(pc.GOLDEN, "pool.npz")), len(pc.captured_cases())))


if __name__ == "__main__":
    main(sys.argv[1])
