"""Packs what the reference's fully-connected layer returns into tests/golden/fc.npz (data only): per case the desc, the create
status, the six datalayouts with their sizes, the scratch size, the status of execute_st for every kind, the inputs in the
tensors' own layout, the outputs of FWD, BWD and UPD, and for the blocked format the result of copy-in from and copy-out to
plain NCHW / KCRS.

    python tools/golden/fc_capture.py <fc_capture binary built from tools/golden/fc_capture.c against the reference>

The cases and their seeded inputs are those of tests/fc_common.py. The inputs are bf16 numbers, so they are stored as their
upper 16 bits -- the small ones; a larger input is regenerated from its seed by tests/fc_common.py and only its CRC-32 is kept.
A case the reference cannot execute on this CPU (the process dies in a kernel dispatch that returned NULL)
keeps its statuses and layouts and has no outputs; such cases are printed."""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fc_common as fc  # noqa: E402
import quant_common as qc  # noqa: E402

NMETA = 169
SMALL = 8192  # elements: larger inputs are regenerated from their seed and stored as a checksum only


def capture(exe, tmp, name, d, files, run):
    prefix = os.path.join(tmp, "out")
    for suffix in ("meta", "y", "dx", "dw", "cin_x", "cin_w", "cout_x", "cout_w"):
        if os.path.exists(prefix + "." + suffix):
            os.remove(prefix + "." + suffix)
    unbound = sum(1 << fc.TENSOR_TYPES.index(t) for t in fc.UNBOUND.get(name, ()))
    args = [exe] + [str(d[k]) for k in fc.DESC_FIELDS] + [str(unbound), str(run)] + files + [prefix]
    # the AVX-512 drivers of FWD and BWD answer LIBXSMM_DNN_ERR_UNSUPPORTED_ARCH in a build whose compiler flags leave the AVX-512
    # intrinsics out (the plain static build does); the generic drivers behind them dispatch the same SMM kernels: run those
    res = subprocess.run(args, env=dict(os.environ, LIBXSMM_TARGET="hsw"))
    if 0 != res.returncode:
        return None
    out = {"meta": np.fromfile(prefix + ".meta", dtype=np.int64)}
    assert out["meta"].shape == (NMETA,)
    for suffix in ("y", "dx", "dw", "cin_x", "cin_w", "cout_x", "cout_w"):
        if os.path.exists(prefix + "." + suffix):
            out[suffix] = np.fromfile(prefix + "." + suffix, dtype=np.uint8)
    return out


def stored(tmp, fname, a):
    path = os.path.join(tmp, fname)
    np.ascontiguousarray(a).tofile(path)
    return path


def main(exe):
    tmp = tempfile.mkdtemp()
    pack, dead = {}, []
    cases = fc.all_cases()
    cases["selfcheck"] = fc.desc(4, 16, 16)
    for name, d in cases.items():
        h = fc.Handle(d)
        x, w, dy = fc.plain_inputs(name, d)
        if "selfcheck" == name:
            w = np.eye(16, dtype=np.float32)
        pack[name + "/desc"] = np.array([d[k] for k in fc.DESC_FIELDS], dtype=np.int64)
        files = ["-"] * 5
        executable = h.ok and (h.f32 or h.mixed) and (h.custom or h.packed) and not (h.packed and h.mixed)
        if executable:
            lo = (lambda a: qc.bf16_rne(a).reshape(a.shape)) if h.mixed else (lambda a: a)
            tx, tw, tdy = fc.block_act(h, lo(x), "c"), fc.block_fil(h, lo(w)), fc.block_act(h, dy, "k")
            files = [stored(tmp, "x.bin", tx), stored(tmp, "w.bin", tw), stored(tmp, "dy.bin", tdy), stored(tmp, "xp.bin", lo(x)), stored(tmp, "wp.bin", lo(w))]
            for key, a in (("x", x), ("w", w), ("dy", dy)):
                if a.size <= SMALL:
                    pack[name + "/in_" + key] = qc.bf16_truncate(a).reshape(a.shape)  # (exact: the values are bf16 numbers)
                pack[name + "/crc_" + key] = np.array([zlib.crc32(np.ascontiguousarray(a).tobytes())], dtype=np.int64)
        out = capture(exe, tmp, name, d, files, 1)
        if out is None:
            dead.append(name)
            out = capture(exe, tmp, name, d, files, 0)
            assert out is not None, name
        for key, value in out.items():
            if key.startswith("c") and (not h.custom or value.size > 4 * SMALL):
                continue  # (copies are served for the blocked format only: the status is in meta; the large cases' images stay out)
            pack[name + "/" + key] = value
    # the guard: FWD of an identity filter returns the input
    if "selfcheck" not in dead:
        x = fc.plain_inputs("selfcheck", cases["selfcheck"])[0]
        assert np.array_equal(pack["selfcheck/y"].view(np.float32).reshape(4, 16), x), "the capture does not compute what it is believed to"
    print("cases without outputs (the reference cannot execute them here):", dead)
    np.savez_compressed(os.path.join(fc.GOLDEN, "fc.npz"), **pack)
    print("fc.npz: %d bytes" % os.path.getsize(os.path.join(fc.GOLDEN, "fc.npz")))


if __name__ == "__main__":
    main(sys.argv[1])
