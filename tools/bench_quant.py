#!/usr/bin/env python3
"""Quantisation and bf16 conversion as streams: GB/s in algorithmic bytes next to a copy of the same byte count.

Cases, device operands, 2^26 elements unless a shape is given:
  quantize <mode>   libxsmm_amd_dnn_quantize_async in every deterministic mode: reads the input twice (maximum, then map): 10 B/element
  act tiled/generic libxsmm_amd_dnn_quantize_act_async, (64, 256, 56, 56) plain input -> blocks (8, 2), with the LDS form and with
                    LIBXSMM_AMD_QUANT_TILED=0
  dequantize        6 B/element
  truncate, rnaz, rne, widen   the four converters, 6 B/element; torch's own .to(torch.bfloat16) beside rne
Beside each case the yardstick of the same session: dst.copy_(src) moving the same number of bytes (half read, half written).
Every case is warmed up twice, then timed event to event over as many calls as fill about 0.3 s (3 ... 50) in five windows; the
median window is reported with the spread (min ... max). Usage: tools/bench_quant.py [--out FILE] [--quick]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="2^20 elements and a small act shape: checks the tool, measures nothing")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_quant: no GPU", file=sys.stderr)
        return 1
    xs = importlib.import_module("libxsmm-1_amd")
    xs.lib()
    torch.cuda.set_device(0)
    n = 1 << (20 if args.quick else 26)
    act = (4, 32, 14, 14, 1, 8, 2) if args.quick else (64, 256, 56, 56, 1, 8, 2)
    nact = act[0] * act[1] * act[2] * act[3]
    nmax = max(n, nact)
    gen = torch.Generator(device="cuda").manual_seed(7)
    f32 = torch.rand(nmax, device="cuda", dtype=torch.float32, generator=gen) * 2 - 1
    f32b = torch.empty(nmax, device="cuda", dtype=torch.float32)
    i16 = torch.empty(nmax, device="cuda", dtype=torch.int16)
    i16b = (torch.rand(nmax, device="cuda", generator=gen) * 60000 - 30000).to(torch.int16)
    scf = torch.zeros(1, device="cuda", dtype=torch.uint8)
    lines = []

    def report(name, kernel, count, bytes_per_element, call):
        nbytes = count * bytes_per_element
        reps, med, lo, hi = timed(torch, call)
        src, dst = f32.view(torch.uint8)[:nbytes // 2], f32b.view(torch.uint8)[:nbytes // 2]
        if nbytes // 2 > src.numel():
            src = torch.empty(nbytes // 2, device="cuda", dtype=torch.uint8); dst = torch.empty_like(src)
        _, cmed, _, _ = timed(torch, lambda: dst.copy_(src))
        line = "RESULT %-18s kernel=%-16s elements=%d calls/window=%d median_ms=%.4f min_ms=%.4f max_ms=%.4f GB/s=%.0f copy_same_bytes_ms=%.4f copy_GB/s=%.0f share_of_copy=%.2f" % (
            name, kernel, count, reps, med, lo, hi, nbytes / (med * 1e-3) / 1e9, cmed, nbytes / (cmed * 1e-3) / 1e9, cmed / med)
        print(line, flush=True)
        lines.append(line)

    for label, mode in (("quantize no", xs.QUANT_NO_ROUND), ("quantize bias", xs.QUANT_BIAS_ROUND), ("quantize nearest", xs.QUANT_NEAREST_ROUND),
                        ("quantize fphw", xs.QUANT_FPHW_ROUND)):
        def call(mode=mode):
            assert 0 == xs.dnn_quantize(f32, i16, n, 2, mode, scf=scf)
        report(label, "quant_flat", n, 10, call)
    for label, env in (("act tiled", "1"), ("act generic", "0")):
        os.environ["LIBXSMM_AMD_QUANT_TILED"] = env

        def call():
            assert 0 == xs.dnn_quantize_act(f32, i16, *act, 2, xs.QUANT_FPHW_ROUND, scf=scf)
        call()
        report(label, xs.last_kernel(), nact, 10, call)
    os.environ.pop("LIBXSMM_AMD_QUANT_TILED")
    report("dequantize", "dequant_flat", n, 6, lambda: xs.dnn_dequantize(i16b, f32b, n, 12))
    for rounding in ("truncate", "rnaz", "rne"):
        report(rounding, "bf16_" + rounding, n, 6, lambda rounding=rounding: xs.convert_f32_bf16(f32, i16, n, rounding))
    report("torch .to(bf16)", "-", n, 6, lambda: f32[:n].to(torch.bfloat16))
    report("widen", "bf16_widen", n, 6, lambda: xs.convert_bf16_f32(i16b, f32b, n))
    with open(args.out, "w") as f:
        f.write("# tools/bench_quant.py%s: GB/s in algorithmic bytes (quantise reads its input twice); copy: dst.copy_(src) of the same byte count\n" % (" --quick" if args.quick else ""))
        f.write("# device: %s\n" % torch.cuda.get_device_name(0))
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
