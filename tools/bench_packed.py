#!/usr/bin/env python3
"""Packed kernels (pgemm, getrf, trmm, trsm): time per batch call and the share of the HBM peak in algorithmic bytes (every operand
read once, the written one also written once), next to libxsmm_amd_stream_probe over the same number of bytes.
    python3 tools/bench_packed.py [--sizes 4 8 16 32] [--mbytes 512] [--reps 20] [--forms 0 1 2] [--out profiles/packed_x.txt]
--forms: LIBXSMM_AMD_PACKED_FORM values to time (0: the library's choice, 1: packs staged through LDS, 2: lanes on global memory)."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK = 8.0e12  # bytes/s, MI355X datasheet
PGEMM, GETRF, TRMM, TRSM = 3, 4, 5, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4, 8, 16, 32])
    ap.add_argument("--mbytes", type=int, default=512, help="operand bytes per call, about (fills the device)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forms", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    assert torch.cuda.is_available()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        f(); f()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e-3 / args.reps

    emit("# kind type size form kernel packs bytes time_us GB/s %%peak | stream probe over the same bytes: GB/s %%peak   (peak: the MI355X datasheet figure, %.1f TB/s)" % (PEAK / 1e12))
    for ts, tname in ((8, "f64"), (4, "f32")):
        dtype = torch.float64 if ts == 8 else torch.float32
        for s in args.sizes:
            for kind, name, nops in ((PGEMM, "pgemm", 3), (GETRF, "getrf", 1), (TRMM, "trmm", 2), (TRSM, "trsm", 2)):
                per_pack = s * s * 64  # bytes of one operand of one pack
                npacks = max(1, args.mbytes * (1 << 20) // (per_pack * nops))
                elems = npacks * per_pack // ts
                a = torch.rand(elems, device="cuda", dtype=dtype) + (2.0 if kind != PGEMM else 0.0)
                b = torch.rand(elems, device="cuda", dtype=dtype) if nops > 1 else a
                c = torch.rand(elems, device="cuda", dtype=dtype) if nops > 2 else None
                if kind == GETRF:  # a heavy diagonal keeps repeated factorisations of the same buffer finite
                    a.view(npacks, s, s, 64 // ts)[:, range(s), range(s), :] += 4.0 * s
                # getrf, trmm and trsm work in place: every repetition starts from the same operand (the copy is timed apart and taken off)
                wr = a if kind == GETRF else b
                keep = wr.clone() if kind != PGEMM else None
                blob, d = xs.packed_descriptor(kind, ts, s, s, s, diag="U" if kind in (TRMM, TRSM) else "N")
                fn = xs.packed_dispatch(kind, d)
                assert fn
                traffic = per_pack * npacks * (nops + 1)  # reads of every operand + the write
                pa, pb, pc = xs.dptr(a), xs.dptr(b), xs.dptr(c)
                # the probe moves 4 * bytes (3 reads, 1 write): the same traffic
                nb = traffic // 4 // 4096 * 4096
                x, y, z = (torch.zeros(nb // 4, device="cuda", dtype=torch.float32) for _ in range(3))
                def probe():
                    assert 0 == L.libxsmm_amd_stream_probe(xs.dptr(x), xs.dptr(y), xs.dptr(z), nb)
                tp = timed(probe)
                del x, y, z
                for form in args.forms:
                    os.environ["LIBXSMM_AMD_PACKED_FORM"] = str(form)

                    def call():
                        if keep is not None:
                            wr.copy_(keep)
                        assert 0 == L.libxsmm_amd_packed_execute_batch(fn, pa, pb, pc, npacks)
                    t = timed(call)
                    if keep is not None:
                        t -= timed(lambda: wr.copy_(keep))
                    emit("%-5s %s %2d form=%d %-26s %8d %11d %9.1f %7.0f %5.1f | %7.0f %5.1f" % (
                        name, tname, s, form, xs.last_kernel(), npacks, traffic, t * 1e6, traffic / t / 1e9, 100 * traffic / t / PEAK,
                        4 * nb / tp / 1e9, 100 * 4 * nb / tp / PEAK))
                del a, b, c, keep, wr
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
