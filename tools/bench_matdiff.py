#!/usr/bin/env python3
"""libxsmm_matdiff on device operands as a stream: GB/s in algorithmic bytes next to libxsmm_amd_stream_probe.

Cases, F32 and F64, device operands, the result in device memory (libxsmm_amd_matdiff_async / _batch: nobody waits):
  single   one matrix of 8192 x 8192
  batch    2^20 items of 32 x 32, tight, one call of libxsmm_amd_matdiff_batch (no per-item infos)
Algorithmic bytes: each operand is read twice (the variance needs the averages first), so 2 * (ref + tst) bytes. Beside each
case the yardstick of the same session: libxsmm_amd_stream_probe over the operands' byte count, which moves the same 4 x
bytes (three reads and a write). Every case is warmed up twice, then timed event to event over as many calls as fill about
0.3 s (3 ... 50) in five windows; the median window is reported with the spread. Usage: tools/bench_matdiff.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call(); call(); torch.cuda.synchronize()
    e0.record(); call(); e1.record(); torch.cuda.synchronize()
    once = max(e0.elapsed_time(e1), 1e-3)
    reps = int(min(50, max(3, 300.0 / 5 / once)))
    windows = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            call()
        e1.record(); torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / reps)
    windows.sort()
    return reps, windows[2], windows[0], windows[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matdiff_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="1024 x 1024 and 2^12 items: checks the tool, measures nothing")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_matdiff: no GPU", file=sys.stderr)
        return 1
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    side, items = (1024, 1 << 12) if args.quick else (8192, 1 << 20)
    info = torch.zeros(C.sizeof(xs.MatdiffInfo), dtype=torch.uint8, device="cuda")
    pinfo = C.cast(xs.dptr(info), C.POINTER(xs.MatdiffInfo))
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines = []
    for dtype, dt, name in ((torch.float32, xs.F32, "f32"), (torch.float64, xs.F64, "f64")):
        count = max(side * side, items * 1024)
        ref = torch.empty(count, device="cuda", dtype=dtype)
        for lo in range(0, count, 1 << 26):  # (filled in pieces: no second buffer of the whole size)
            ref[lo:lo + (1 << 26)] = torch.rand(min(1 << 26, count - lo), device="cuda", dtype=torch.float32, generator=gen).to(dtype) * 2 - 1
        tst = ref * (1 + 1e-6)
        acc = torch.zeros(count, device="cuda", dtype=dtype)

        def single():
            assert 0 == L.libxsmm_amd_matdiff_async(pinfo, dt, side, side, xs.dptr(ref), xs.dptr(tst), None, None)

        def batch():
            assert 0 == L.libxsmm_amd_matdiff_batch(pinfo, None, None, dt, 32, 32, xs.dptr(ref), xs.dptr(tst), None, None, 1024, 1024, items)

        for label, call, elements in (("single %dx%d" % (side, side), single, side * side), ("batch %dx32x32" % items, batch, items * 1024)):
            operand = elements * ref.element_size()
            call()
            kernel = xs.last_kernel()
            reps, med, lo, hi = timed(torch, call)
            _, pmed, _, _ = timed(torch, lambda: L.libxsmm_amd_stream_probe(xs.dptr(ref), xs.dptr(tst), xs.dptr(acc), operand))
            line = "RESULT %-22s %s last_kernel=%-14s elements=%d calls/window=%d median_ms=%.4f min_ms=%.4f max_ms=%.4f GB/s=%.0f probe_same_bytes_ms=%.4f probe_GB/s=%.0f share_of_probe=%.2f" % (
                label, name, kernel, elements, reps, med, lo, hi, 4 * operand / (med * 1e-3) / 1e9, pmed, 4 * operand / (pmed * 1e-3) / 1e9, pmed / med)
            print(line, flush=True)
            lines.append(line)
        del ref, tst, acc
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("# tools/bench_matdiff.py%s: GB/s in algorithmic bytes, 2 x (ref + tst): each operand is read twice; probe: libxsmm_amd_stream_probe over the operands' byte count (the same 4 x bytes)\n" % (" --quick" if args.quick else ""))
        f.write("# device: %s\n" % torch.cuda.get_device_name(0))
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
