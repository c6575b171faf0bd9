"""Packs what the reference computes into tests/golden/quant_*.npz (data only: inputs, outputs, scf bytes).

    python tools/golden/quant_capture.py <quant_capture binary built from tools/golden/quant_capture.c against the reference>

The cases are those of tests/quant_common.py. One check guards the capture itself: FPHW_ROUND must map a scaled +-2.5 to +-3
(halves away from zero); +-2 would mean that the reference was built with its AVX-512 branch, which is not the path of record."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quant_common as qc  # noqa: E402


def run(exe, tmp, args, data, out_dtype, n, with_scf):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.ascontiguousarray(data).tofile(fin)
    subprocess.run([exe] + [str(a) for a in args] + [fin, fout], check=True)
    raw = open(fout, "rb").read()
    out = np.frombuffer(raw[:n * np.dtype(out_dtype).itemsize], dtype=out_dtype).copy()
    return (out, raw[-1]) if with_scf else out


def main(exe):
    tmp = tempfile.mkdtemp()
    modes = {"no": qc.NO_ROUND, "bias": qc.BIAS_ROUND, "nearest": qc.NEAREST_ROUND, "fphw": qc.FPHW_ROUND}
    # the guard: 2.5 / 4 with a maximum of 4096 and add_shift 2 keeps the scale at 1 (frexp(4096) = 13; 13 - 13 = 0)
    probe = np.array([4096.0, 2.5, -2.5, 0.5, -1.5], dtype=np.float32)
    out, scf = run(exe, tmp, ["flat", qc.FPHW_ROUND, 2, probe.size], probe, np.int16, probe.size, True)
    assert scf == 0 and list(out) == [4096, 3, -3, 1, -2], ("the reference rounds ties to even: AVX-512 branch?", out, scf)

    flat = {}
    for n in qc.FLAT_GOLDEN_LENGTHS:
        x = qc.golden_input(100 + n, n, 3.0)
        if n >= 5:
            x[1:5] = np.array([0.0, -0.0, 1e-40, -3.0], dtype=np.float32)  # zeros, a denormal, the maximum negative
        flat["in_%d" % n] = x
        for name, mode in modes.items():
            for shift in (0, 2):
                out, scf = run(exe, tmp, ["flat", mode, shift, n], x, np.int16, n, True)
                flat["out_%s_%d_%d" % (name, shift, n)] = out
                flat["scf_%s_%d_%d" % (name, shift, n)] = np.uint8(scf)
    np.savez_compressed(os.path.join(qc.GOLDEN, "quant_flat.npz"), **flat)

    for kind, cases in (("act", qc.ACT_CASES), ("fil", qc.FIL_CASES)):
        pack = {}
        for ci, case in enumerate(cases):
            n = int(np.prod(case[:4]))
            x = qc.golden_input(200 + 10 * ci + len(case), n, 0.7)
            pack["in_%d" % ci] = x
            for shift in (0, 2):
                base = None
                for name, mode in modes.items():  # ("no" comes first: the others are stored as their difference to it)
                    out, scf = run(exe, tmp, [kind, mode, shift] + list(case), x, np.int16, n, True)
                    pack["scf_%s_%d_%d" % (name, shift, ci)] = np.uint8(scf)
                    if base is None:
                        base = pack["out_no_%d_%d" % (shift, ci)] = out
                    else:
                        delta = (out.view(np.uint16) - base.view(np.uint16)).view(np.int16)
                        assert (np.abs(delta) <= 1).all(), (kind, case, name, shift)
                        pack["delta_%s_%d_%d" % (name, shift, ci)] = delta.astype(np.int8)
                    assert np.array_equal(qc.golden_layout(pack, name, shift, ci)[0], out)
        np.savez_compressed(os.path.join(qc.GOLDEN, "quant_%s.npz" % kind), **pack)

    conv = {"in_bits": qc.BF16_SPECIALS}
    x = qc.from_bits(qc.BF16_SPECIALS)
    for which, name in enumerate(("truncate", "rnaz", "rne")):
        conv[name] = run(exe, tmp, ["bf16", which, x.size], x, np.uint16, x.size, False)
    conv["widen_in"] = conv["rne"]
    conv["widen"] = run(exe, tmp, ["bf16", 3, x.size], conv["rne"], np.float32, x.size, False).view(np.uint32)
    q = np.array([0, 1, -1, 4096, -1229, 32767, -32768, 12345], dtype=np.int16)
    conv["deq_in"] = q
    for scf in qc.DEQUANT_SCF:
        conv["deq_%d" % scf] = run(exe, tmp, ["deq", scf, q.size], q, np.float32, q.size, False).view(np.uint32)
    fout = os.path.join(tmp, "sexp2.bin")
    subprocess.run([exe, "sexp2", fout], check=True)
    s = np.fromfile(fout, dtype=np.uint32).reshape(3, 256)
    conv["sexp2_u8"], conv["sexp2_i8"], conv["sexp2_i8i"] = s[0], s[1], s[2]
    text = subprocess.run([exe, "consts"], check=True, capture_output=True, text=True).stdout
    names = [ln.split("=")[0] for ln in text.split()]
    conv["const_names"] = np.array(names)
    conv["const_values"] = np.array([int(ln.split("=")[1]) for ln in text.split()], dtype=np.uint64)
    np.savez_compressed(os.path.join(qc.GOLDEN, "quant_misc.npz"), **conv)


if __name__ == "__main__":
    main(sys.argv[1])
