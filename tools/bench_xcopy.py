#!/usr/bin/env python3
"""Copy and transposition (libxsmm_otrans / libxsmm_matcopy of one large matrix, libxsmm_amd_otrans_batch / _matcopy_batch over a
stack of small items, strided and pointer forms): time per call, event to event, warm, the minimum over the repetitions; GB/s of
algorithmic bytes (every element read once and written once) next to libxsmm_amd_stream_probe over the same number of bytes in
the same process, and the per-call cost of one small libxsmm_otrans on device memory.
    python3 tools/bench_xcopy.py [--mbytes 512] [--reps 10] [--out profiles/xcopy_bench.txt]"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=512, help="bytes of one operand of the large-matrix cases, about (two operands: 1 GB)")
    ap.add_argument("--items", type=int, default=1 << 20, help="items of the stack cases")
    ap.add_argument("--reps", type=int, default=10)
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
        best = None
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); f(); t1.record()
            torch.cuda.synchronize()
            t = t0.elapsed_time(t1) * 1e-3
            best = t if best is None else min(best, t)
        return best

    def probe_gbs(traffic):
        nb = traffic // 4 // 4096 * 4096  # the probe moves 4 * nb bytes (three reads, one write)
        x, y, z = (torch.zeros(nb // 4, device="cuda", dtype=torch.float32) for _ in range(3))
        t = timed(lambda: L.libxsmm_amd_stream_probe(xs.dptr(x), xs.dptr(y), xs.dptr(z), nb))
        return 4 * nb / t / 1e9

    def report(what, kernel, traffic, t):
        p = probe_gbs(traffic)
        g = traffic / t / 1e9
        emit("%-46s %-20s %11d %9.1f %7.0f | %7.0f %5.2f" % (what, kernel, traffic, t * 1e6, g, p, g / p))

    emit("# case kernel bytes(read+written) time_us GB/s | stream probe over the same bytes: GB/s, ratio to the probe")
    for ts in (4, 8):
        n = int((args.mbytes * (1 << 20) / ts) ** 0.5) // 64 * 64
        for pad in (0, 13):
            ld = n + pad
            a = torch.randint(0, 255, (n * ld * ts,), device="cuda", dtype=torch.uint8)
            b = torch.zeros(n * ld * ts, device="cuda", dtype=torch.uint8)
            traffic = 2 * n * n * ts
            for name, f in (("otrans", lambda: xs.otrans(b.data_ptr(), a.data_ptr(), ts, n, n, ld, ld)),
                            ("matcopy", lambda: xs.matcopy(b.data_ptr(), a.data_ptr(), ts, n, n, ld, ld)),
                            ("itrans", lambda: xs.itrans(b.data_ptr(), ts, n, n, ld))):
                t = timed(f)
                report("%s ts=%d %dx%d ld=%d" % (name, ts, n, n, ld), xs.last_kernel(), traffic, t)
            del a, b
    for ts, s in ((4, 32), (8, 23), (8, 13)):
        batch = args.items
        a = torch.randint(0, 255, (batch * s * s * ts,), device="cuda", dtype=torch.uint8)
        b = torch.zeros(batch * s * s * ts, device="cuda", dtype=torch.uint8)
        step = s * s * ts
        pa = (a.data_ptr() + torch.arange(batch, device="cuda", dtype=torch.int64) * step)
        pb = (b.data_ptr() + torch.arange(batch, device="cuda", dtype=torch.int64) * step)
        traffic = 2 * batch * step
        for name, f in (("otrans_batch", lambda: xs.otrans_batch(b.data_ptr(), a.data_ptr(), ts, s, s, s, s, s * s, s * s, batch)),
                        ("otrans_batch_ptr", lambda: xs.otrans_batch_ptr(pb, pa, ts, s, s, s, s, batch)),
                        ("matcopy_batch", lambda: xs.matcopy_batch(b.data_ptr(), a.data_ptr(), ts, s, s, s, s, s * s, s * s, batch)),
                        ("matcopy_batch_ptr", lambda: xs.matcopy_batch_ptr(pb, pa, ts, s, s, s, s, batch))):
            t = timed(f)
            report("%s ts=%d %dx%d x %d" % (name, ts, s, s, batch), xs.last_kernel(), traffic, t)
        del a, b, pa, pb
    # the cost of one small call on device memory (host side: calls issued back to back, the queue drained at the end)
    a = torch.zeros(32 * 32, device="cuda", dtype=torch.float32)
    b = torch.zeros(32 * 32, device="cuda", dtype=torch.float32)
    pa, pb, ncalls = a.data_ptr(), b.data_ptr(), 20000
    f = L.libxsmm_otrans
    for _ in range(1000):
        f(pb, pa, 4, 32, 32, 32, 32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ncalls):
        f(pb, pa, 4, 32, 32, 32, 32)
    torch.cuda.synchronize()
    emit("one libxsmm_otrans 32x32 fp32 on device memory, %d calls back to back through ctypes: %.2f us per call" % (ncalls, (time.perf_counter() - t0) / ncalls * 1e6))
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
