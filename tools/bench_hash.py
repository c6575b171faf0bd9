#!/usr/bin/env python3
"""libxsmm_hash and libxsmm_memcmp on device operands as streams: GB/s of bytes read next to libxsmm_amd_stream_probe.

Cases, device operands, the result in device memory (libxsmm_amd_hash_async / _hash_batch / _memcmp_async / _memcmp_batch: nobody waits):
  single   one buffer of 4 GiB
  batch    2^20 items of 4 KiB, tight, one call
Bytes read: the buffer for the hash, both buffers for the compare. Beside each case the yardstick of the same session:
libxsmm_amd_stream_probe with operands of a quarter of that byte count, which moves the same number of bytes (three reads and a
write). Every case is warmed up twice, then timed event to event over as many calls as fill about 0.3 s (3 ... 50) in five
windows; the median window is reported with the spread. Usage: tools/bench_hash.py [--out FILE] [--quick]"""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="64 MiB and 2^12 items: checks the tool, measures nothing")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_hash: no GPU", file=sys.stderr)
        return 1
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    total, items, item = (1 << 26, 1 << 12, 4096) if args.quick else (1 << 32, 1 << 20, 4096)
    gen = torch.Generator(device="cuda").manual_seed(7)
    a = torch.empty(total, device="cuda", dtype=torch.uint8)
    for lo in range(0, total, 1 << 28):  # (filled in pieces: no second buffer of the whole size)
        a[lo:lo + (1 << 28)] = torch.randint(0, 256, (min(1 << 28, total - lo),), device="cuda", dtype=torch.uint8, generator=gen)
    b = a.clone()
    probe = [torch.zeros(total // 2, device="cuda", dtype=torch.uint8) for _ in range(3)]
    results = torch.zeros(items, device="cuda", dtype=torch.int32)
    pa, pb, pr = a.data_ptr(), b.data_ptr(), results.data_ptr()
    cases = (
        ("hash single %d MiB" % (total >> 20), total, lambda: L.libxsmm_amd_hash_async(pr, pa, total, 1)),
        ("hash batch %d x %d" % (items, item), items * item, lambda: L.libxsmm_amd_hash_batch(pr, pa, item, 1, 0, item, items, 1)),
        ("memcmp single %d MiB" % (total >> 20), 2 * total, lambda: L.libxsmm_amd_memcmp_async(pr, pa, pb, total)),
        ("memcmp batch %d x %d" % (items, item), 2 * items * item, lambda: L.libxsmm_amd_memcmp_batch(pr, None, pa, pb, item, 1, 0, 0, item, item, items)))
    lines = []
    for label, read, call in cases:
        def checked():
            assert 0 == call()
        checked()
        kernel = xs.last_kernel()
        reps, med, lo, hi = timed(torch, checked)
        _, pmed, _, _ = timed(torch, lambda: L.libxsmm_amd_stream_probe(probe[0].data_ptr(), probe[1].data_ptr(), probe[2].data_ptr(), read // 4))
        line = "RESULT %-28s last_kernel=%-13s bytes_read=%d calls/window=%d median_ms=%.4f min_ms=%.4f max_ms=%.4f GB/s=%.0f probe_same_bytes_ms=%.4f probe_GB/s=%.0f share_of_probe=%.2f" % (
            label, kernel, read, reps, med, lo, hi, read / (med * 1e-3) / 1e9, pmed, read / (pmed * 1e-3) / 1e9, pmed / med)
        print(line, flush=True)
        lines.append(line)
    with open(args.out, "w") as f:
        f.write("# tools/bench_hash.py%s: GB/s of bytes read (the compare reads two buffers); probe: libxsmm_amd_stream_probe moving the same byte count (three reads, one write)\n" % (" --quick" if args.quick else ""))
        f.write("# device: %s\n" % torch.cuda.get_device_name(0))
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
