"""Packs what the reference's libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n return into tests/golden/hash.npz
(data only: per case of tests/hash_common.py the returned value).

    python tools/golden/hash_capture.py <hash_capture binary built from tools/golden/hash_capture.c against the reference>

The cases and their inputs are those of tests/hash_common.py: the inputs are regenerated from seeds and not stored. The guard
is the published check value of CRC-32C: hash("123456789", 9, 0xFFFFFFFF) == 0xE3069283 ^ 0xFFFFFFFF."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hash_common as hc  # noqa: E402


def stored(tmp, name, x):
    path = os.path.join(tmp, name)
    np.ascontiguousarray(x).tofile(path)
    return path


def main(exe):
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "out.bin")
    subprocess.run([exe, "check"], check=True)  # the guard
    hashes = []
    for size, offset, seed in hc.HASH_CASES:
        subprocess.run([exe, "hash", str(seed), stored(tmp, "a.bin", hc.hash_case_input(size, offset, seed)), out], check=True)
        hashes.append(np.fromfile(out, dtype=np.uint32)[0])
    compares = []  # per hash case: equal copies, then a copy whose last byte differs (sizes above 0)
    for size, offset, seed in hc.HASH_CASES:
        a = hc.hash_case_input(size, offset, seed)
        b = a.copy()
        row = []
        for flip in (False, True):
            if flip and 0 < size:
                b[-1] ^= 0x40
            subprocess.run([exe, "cmp", stored(tmp, "a.bin", a), stored(tmp, "b.bin", b), out], check=True)
            row.extend(np.fromfile(out, dtype=np.int32).tolist())
        compares.append(row)
    found = []
    for index, (size, stride, hint, n, _) in enumerate(hc.DIFF_N_CASES):
        a, bn = hc.diff_n_case_input(index)
        subprocess.run([exe, "diff_n", str(size), str(stride), str(hint), str(n), stored(tmp, "a.bin", a), stored(tmp, "b.bin", bn), out], check=True)
        found.append(np.fromfile(out, dtype=np.uint32)[0])
    np.savez_compressed(os.path.join(hc.GOLDEN, "hash.npz"), hash=np.array(hashes, dtype=np.uint32), compare=np.array(compares, dtype=np.int32),
                        diff_n=np.array(found, dtype=np.uint32))


if __name__ == "__main__":
    main(sys.argv[1])
