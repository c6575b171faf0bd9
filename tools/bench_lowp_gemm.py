#!/usr/bin/env python3
"""GEMM with 16-bit inputs next to the fp32 tiled GEMM of the same shape.

Kernels (kernels/tgemm_lowp.hip through libxsmm_amd_lowp_gemm): bf16 exact, bf16 fast (LIBXSMM_AMD_LOWP_FAST), i16 -> i32,
i16 -> f32; and fp32 through libxsmm_gemm_thread (kernels/tgemm.hip). NN and TN, beta = 1, device operands. Every case is
warmed up twice, then timed event to event over as many calls as fill about 0.3 s (3 ... 50) in five windows; the median
window is reported, with the spread (min ... max) next to it. OP = 2 m n k. Usage: tools/bench_lowp_gemm.py [--out FILE] [--quick]"""
import argparse
import importlib
import os
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 1024, 1024), (4096, 4096, 4096), (2047, 2049, 1023)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowp_gemm_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="1024^3 only")
    args = ap.parse_args()
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    xs.lib()
    torch.cuda.set_device(0)
    lines = ["# tools/bench_lowp_gemm.py: libxsmm_amd_lowp_gemm (bf16 exact, bf16 fast, i16 -> i32, i16 -> f32) next to the fp32 tiled GEMM; beta = 1, device operands",
             "# event to event, warm, median of five windows (min ... max: the spread); TOPs = 2 m n k / median"]
    legs = (("f32", None, None, False), ("bf16_exact", xs.BF16, xs.F32, False), ("bf16_fast", xs.BF16, xs.F32, True),
            ("i16_i32", xs.I16, xs.I32, False), ("i16_f32", xs.I16, xs.F32, False))
    for (m, n, k) in (SHAPES[:1] if args.quick else SHAPES):
        for ta in ("N", "T"):
            lda = m if ta == "N" else k
            for name, iprec, oprec, fast in legs:
                gen = torch.Generator(device="cuda").manual_seed(m + k)
                if iprec is None:
                    a = torch.rand(m * k, device="cuda", dtype=torch.float32, generator=gen) * 2 - 1
                    b = torch.rand(k * n, device="cuda", dtype=torch.float32, generator=gen) * 2 - 1
                    c = torch.zeros(m * n, device="cuda", dtype=torch.float32)
                    keep, h = xs.gemm_handle(xs.F32, xs.F32, ta, "N", m, n, k, lda, k, m, 1.0, 1.0)
                    assert h

                    def call():
                        xs.gemm_thread(h, a, b, c)
                else:
                    if iprec == xs.BF16:  # bf16 bit patterns of uniform [-1, 1)
                        a = (torch.rand(m * k, device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16).view(torch.int16)
                        b = (torch.rand(k * n, device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16).view(torch.int16)
                    else:
                        a = torch.randint(-128, 128, (m * k,), device="cuda", generator=gen).to(torch.int16)
                        b = torch.randint(-128, 128, (k * n,), device="cuda", generator=gen).to(torch.int16)
                    c = torch.zeros(m * n, device="cuda", dtype=torch.int32 if oprec == xs.I32 else torch.float32)
                    xs.set_lowp_fast(fast)

                    def call():
                        assert 0 == xs.gemm_lowp(iprec, oprec, ta, "N", m, n, k, a, lda, b, k, 1, c, m)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                call(); torch.cuda.synchronize()
                e0.record(); call(); e1.record(); torch.cuda.synchronize()
                once = max(e0.elapsed_time(e1), 1e-3)
                reps = int(min(50, max(3, 300.0 / 5 / once)))
                windows = []
                for _ in range(5):
                    c.zero_()
                    e0.record()
                    for _ in range(reps):
                        call()
                    e1.record(); torch.cuda.synchronize()
                    windows.append(e0.elapsed_time(e1) / reps)
                windows.sort()
                med = windows[2]
                line = "%s %sN %dx%dx%d kernel=%s calls/window=%d median_ms=%.4f min_ms=%.4f max_ms=%.4f TOPs=%.2f" % (
                    name, ta, m, n, k, xs.last_kernel(), reps, med, windows[0], windows[-1], 2.0 * m * n * k / (med * 1e-3) / 1e12)
                print(line, flush=True)
                lines.append(line)
                xs.set_lowp_fast(False)
                del a, b, c
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
