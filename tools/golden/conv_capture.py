"""Packs what the reference's convolution layer returns into tests/golden/conv.npz (data only): per case the desc, the create status,
the layouts of fourteen tensor types with their sizes, the scratch sizes per kind, the statuses of the scratch, binding and helper
functions, the status of execute_st for every kind, and the outputs of FWD, BWD, UPD and trans_reg_filter.

    python tools/golden/conv_capture.py <conv_capture binary built from tools/golden/conv_capture.c against the reference>

The cases and their seeded inputs are those of tests/conv_common.py (captured_cases). Inputs are not stored: they are regenerated
from their seeds and only their CRC-32 is kept. An output above 1024 elements is kept as its CRC-32 only (equality is bitwise, so
nothing is lost). The reference runs with LIBXSMM_TARGET=hsw and threads = 1: its generic templates over AVX2 SMM kernels are the
contract. Destinations start as ones bits where a pass overwrites and as seeded values where it accumulates (conv_common.inputs).
The cases of conv_common.NO_RUN are not executed; for those of CREATE_ONLY nothing but create is called.

The guard: once per pass the captured outputs of an overwriting case are held against a plain float64 convolution, per element
within n * 2^-24 * sum|a * b| (n the number of terms: the standard bound of an fp32 chain; derived, not measured)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_common as cc  # noqa: E402

NMETA = 40 + 26 * len(cc.LAYOUT_TYPES)
SMALL = 1024  # elements: a larger output is stored as a checksum only (the issue allows up to 8192; the file is to stay below 400 KB)
INPUT_KEYS = ("x", "w", "dout", "bias", "out0", "din0", "dw0")
GUARD = "k3x3_s2_log"


def capture(exe, tmp, name, d, files, run, scratch):
    prefix = os.path.join(tmp, "out")
    for suffix in ("meta",) + cc.OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            os.remove(prefix + "." + suffix)
    unbound = sum(1 << cc.BINDABLE.index(t) for t in cc.UNBOUND.get(name, ()))
    args = [exe] + [str(d[k]) for k in cc.DESC_FIELDS] + [str(unbound), str(run), str(scratch)] + files + [prefix]
    subprocess.run(args, env=dict(os.environ, LIBXSMM_TARGET="hsw"), check=True)
    out = {"meta": np.fromfile(prefix + ".meta", dtype=np.int64)}
    assert out["meta"].shape == (NMETA,)
    for suffix in cc.OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            out[suffix] = np.fromfile(prefix + "." + suffix, dtype=np.uint8)
    return out


def main(exe):
    tmp = tempfile.mkdtemp()
    pack, guarded = {}, {}
    for name, d in cc.captured_cases().items():
        pack[name + "/desc"] = np.array([d[k] for k in cc.DESC_FIELDS], dtype=np.int64)
        files = ["-"] * len(INPUT_KEYS)
        run = -1 if name in cc.CREATE_ONLY else int(name not in cc.NO_RUN)
        if run == 1 and cc.ref_create_status(d) == cc.SUCCESS:
            t = cc.inputs(name, d)
            files = []
            for key in INPUT_KEYS:
                path = os.path.join(tmp, key + ".bin")
                np.ascontiguousarray(t[key]).tofile(path)
                files.append(path)
                pack[name + "/crc_" + key] = np.array([cc.crc(t[key])], dtype=np.int64)
        out = capture(exe, tmp, name, d, files, run, int(name not in cc.NO_SCRATCH))
        pack[name + "/meta"] = out["meta"]
        executed = dict(out=out["meta"][16], din=out["meta"][17], dw=out["meta"][18], wtr=out["meta"][33])
        for key in cc.OUTPUTS:
            if key not in out or files[0] == "-" or executed[key] != 0:
                continue  # (the pass did not run: the destination is still its fill)
            pack[name + "/crc_" + key] = np.array([cc.crc(out[key])], dtype=np.int64)
            if name == GUARD:
                guarded[key] = out[key]
            if out[key].size // 4 <= SMALL:
                pack[name + "/" + key] = out[key]
    # the guard
    d = cc.COMPUTE_CASES[GUARD]
    h = cc.Handle(d)
    want, terms = cc.naive64(h, cc.inputs(GUARD, d))
    for key in ("out", "din", "dw"):
        got = cc.interior(h, key, guarded[key].view(np.float32)).astype(np.float64)
        value, weight = want[key]
        assert np.all(np.abs(got - value) <= terms[key] * 2.0 ** -24 * weight), "the capture does not compute what it is believed to (%s)" % key
    np.savez_compressed(os.path.join(cc.GOLDEN, "conv.npz"), **pack)
    print("conv.npz: %d bytes, %d cases" % (os.path.getsize(os.path.join(cc.GOLDEN, "conv.npz")), len(cc.captured_cases())))


if __name__ == "__main__":
    main(sys.argv[1])
