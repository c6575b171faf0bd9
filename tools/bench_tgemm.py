#!/usr/bin/env python3
"""Tiled GEMM against the two homes a large product has without it.

Legs, each in a process of its own (LIBXSMM_AMD_BLAS is read once per process):
  a  libxsmm_gemm_thread(handle, ..., 0, 1): kernels/tgemm.hip
  b  libxsmm_?gemm as it routes by default (rocBLAS where it can be loaded)
  c  libxsmm_?gemm with LIBXSMM_AMD_BLAS=0: the general form of kernels/smm_generic.hip
fp32 and fp64, NN and TN, beta = 1, device operands drawn from uniform [-1, 1). Every case is warmed up twice, then timed
event to event over as many calls as fill about 0.3 s (3 ... 50) in five windows; the median window is reported, with the
spread (min ... max) next to it. FLOP = 2 m n k. Usage: tools/bench_tgemm.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 1024, 1024), (4096, 4096, 4096), (2047, 2049, 1023)]


def leg(which, quick):
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    for dt, prec, fn, ct in ((torch.float32, xs.F32, L.libxsmm_sgemm, C.c_float), (torch.float64, xs.F64, L.libxsmm_dgemm, C.c_double)):
        for (m, n, k) in (SHAPES[:1] if quick else SHAPES):
            for ta in ("N", "T"):
                lda = m if ta == "N" else k
                gen = torch.Generator(device="cuda").manual_seed(m + k)
                a = torch.rand(m * k, device="cuda", dtype=dt, generator=gen) * 2 - 1
                b = torch.rand(k * n, device="cuda", dtype=dt, generator=gen) * 2 - 1
                c = torch.zeros(m * n, device="cuda", dtype=dt)
                one = ct(1.0)
                if which == "a":
                    keep, h = xs.gemm_handle(prec, prec, ta, "N", m, n, k, lda, k, m, 1.0, 1.0)
                    assert h

                    def call():
                        xs.gemm_thread(h, a, b, c)
                else:
                    im, in_, ik, ila = C.c_int(m), C.c_int(n), C.c_int(k), C.c_int(lda)

                    def call():
                        fn(ta.encode(), b"N", C.byref(im), C.byref(in_), C.byref(ik), C.byref(one), xs.dptr(a), C.byref(ila), xs.dptr(b), C.byref(ik),
                           C.byref(one), xs.dptr(c), C.byref(im))
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
                print("RESULT leg=%s %s %sN %dx%dx%d kernel=%s calls/window=%d median_ms=%.4f min_ms=%.4f max_ms=%.4f TFLOPs=%.2f" % (
                    which, "f32" if dt == torch.float32 else "f64", ta, m, n, k, xs.last_kernel(), reps, med, windows[0], windows[-1],
                    2.0 * m * n * k / (med * 1e-3) / 1e12), flush=True)
                del a, b, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["a", "b", "c"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tgemm_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="1024^3 only")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.quick)
        return 0
    lines = ["# tools/bench_tgemm.py: tiled GEMM (a) vs libxsmm_?gemm by default (b) and with LIBXSMM_AMD_BLAS=0 (c); beta = 1, device operands",
             "# event to event, warm, median of five windows (min ... max: the spread); TFLOPs = 2 m n k / median"]
    for which in ("a", "b", "c"):
        env = dict(os.environ)
        env.pop("LIBXSMM_AMD_TGEMM", None)
        if which == "c":
            env["LIBXSMM_AMD_BLAS"] = "0"
        else:
            env.pop("LIBXSMM_AMD_BLAS", None)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which] + (["--quick"] if args.quick else []),
                             capture_output=True, text=True, env=env)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            return 1
        lines += [ln[len("RESULT "):] for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
