"""Packs what the reference's fused batch-norm layer returns into tests/golden/bn.npz (data only): per case the desc, the create
status, the layouts of eighteen tensor types with their sizes (the error statuses of a filter type among them), the scratch size
and the bind statuses, the status of execute_st for every kind, and what FWD and BWD wrote: output, mean, rstd, var, dinput,
dinput_add, doutput (BWD with RELU rewrites it), dgamma and dbeta.

    python tools/golden/bn_capture.py <bn_capture binary built from tools/golden/bn_capture.c against the reference>

The reference is a scratch copy built with `make BLAS=0 FORTRAN=0 STATIC=1 ECFLAGS=-fcommon`. The cases and their seeded inputs
are those of tests/bn_common.py (captured_cases). Inputs are not stored: they are regenerated from their seeds and only their
CRC-32 is kept. An output above 8192 elements is kept as its CRC-32 only (equality is bitwise, so nothing is lost). The
reference runs with LIBXSMM_TARGET=hsw and threads = 1: the generic templates are the contract. Destinations start as 0xff
bytes. The cases of bn_common.NO_RUN are not executed at all, BWD is not run for bn_common.SPECIAL_CASES, and no case has
H % u != 0 or W % v != 0 (the reference would write outside its tensors)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bn_common as bc  # noqa: E402

NMETA = 486
SMALL = 8192  # elements: a larger output is stored as a checksum only
INPUTS = ("x", "add", "dout", "gamma", "beta", "mean", "rstd", "dgamma", "dbeta")
OUTPUTS = ("out", "mean", "rstd", "var", "din", "dadd", "dout", "dgamma", "dbeta")


def capture(exe, tmp, name, d, files, run):
    prefix = os.path.join(tmp, "out")
    for suffix in ("meta",) + OUTPUTS:
        if os.path.exists(prefix + "." + suffix):
            os.remove(prefix + "." + suffix)
    unbound = sum(1 << bc.BINDABLE.index(t) for t in bc.UNBOUND.get(name, ()))
    args = [exe] + [str(d[k]) for k in bc.DESC_FIELDS] + [str(unbound), str(run)] + files + [prefix]
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
    for name, d in bc.captured_cases().items():
        assert d["threads"] == 1 and d["H"] % d["u"] == 0 and d["W"] % d["v"] == 0
        h = bc.Handle(d)
        pack[name + "/desc"] = np.array([d[k] for k in bc.DESC_FIELDS], dtype=np.int64)
        files = ["-"] * len(INPUTS)
        run = 0 if name in bc.NO_RUN else (2 if name in bc.SPECIAL_CASES else 1)
        with_data = name not in bc.STATUS_CASES
        crcs = np.full(len(INPUTS) + len(OUTPUTS), -1, dtype=np.int64)  # one array per case: inputs, then outputs; -1: not there
        if with_data:
            t = bc.inputs(name, d)
            for i, key in enumerate(INPUTS):
                if key in t:
                    files[i] = os.path.join(tmp, key + ".bin")
                    t[key].tofile(files[i])
                    crcs[i] = bc.crc(t[key])
        out = capture(exe, tmp, name, d, files, run)
        pack[name + "/meta"] = out["meta"]
        if not with_data:
            continue
        assert out["meta"][480] == 0 and (run == 2 or out["meta"][481] == 0), name
        keys = bc.written(d, bc.FWD) + (bc.written(d, bc.BWD) if run == 1 else [])
        for key in keys:
            crcs[len(INPUTS) + OUTPUTS.index(key)] = bc.crc(out[key])
            chan = key in ("mean", "rstd", "var", "dgamma", "dbeta")
            if out[key].size // (4 if (h.f32 or chan) else 2) <= SMALL:
                pack[name + "/" + key] = out[key]
        pack[name + "/crc"] = crcs
    # the guard: the mean of one channel, recomputed naively in float64
    name = "fuse1_f32_n"
    x = bc.inputs(name, bc.COMPUTE_CASES[name])["x"]           # [item = img * 2 + block][5][3][16]
    got = pack[name + "/mean"].view(np.float32).reshape(2, 16)
    want = x.astype(np.float64)[1::2, :, :, 4].mean()          # block 1, lane 4: channel 20
    assert abs(got[1, 4] - want) <= 1e-5 * abs(want), "the capture does not compute what it is believed to"
    path = os.path.join(bc.GOLDEN, "bn.npz")
    np.savez_compressed(path, **pack)
    print("bn.npz: %d bytes, %d cases" % (os.path.getsize(path), len(bc.captured_cases())))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(bc.GOLDEN, "pool.npz"))


if __name__ == "__main__":
    main(sys.argv[1])
