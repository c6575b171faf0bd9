#!/usr/bin/env python3
"""The convolution layer against torch and against this engine's own GEMM.

Per shape and pass: libxsmm_dnn_execute_st with threads = 1 on device tensors (FWD: kernels/conv.hip on the matrix cores, BWD and
UPD: its vector-ALU kernels), and two yardsticks in the same run: torch.nn.functional.conv2d / torch.nn.grad.conv2d_input /
conv2d_weight in fp32 on plain NCHW tensors of the same logical shape, and libxsmm_sgemm_omp (kernels/tgemm.hip) of the equivalent
GEMM (M = K, N = images * ofh * ofw, k = C * R * S for FWD; the transposed roles for BWD and UPD), beta = 0, on operands of that
size -- the ceiling of this engine's fp32 arithmetic, without the gather a convolution needs. Shapes (ResNet-50, N = 64): 1x1
64 -> 256 on 56 x 56; 3x3 128 -> 128 on 28 x 28, pad 1; 3x3 / 2 128 -> 128 on 56 x 56, pad 1; 7x7 / 2 3 -> 64 on 224 x 224, pad 3.
Every case is warmed up twice, then timed event to event in five windows of as many calls as fill about 40 ms (3 ... 50); the
median window is reported with the spread. FLOP: 2 * N * K * C * R * S * ofh * ofw per pass. No gate.
Usage: tools/bench_conv.py [--out FILE] [--quick]"""
import argparse
import importlib
import os
import sys

import numpy as np

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 64
SHAPES = [dict(C=64, K=256, H=56, W=56, R=1, S=1, u=1, pad=0), dict(C=128, K=128, H=28, W=28, R=3, S=3, u=1, pad=1),
          dict(C=128, K=128, H=56, W=56, R=3, S=3, u=2, pad=1), dict(C=3, K=64, H=224, W=224, R=7, S=7, u=2, pad=3)]
FWD, BWD, UPD, ALL = 0, 1, 2, 4
REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, REG_FIL, GRAD_FIL = 0, 3, 5, 6, 10, 12


def timed(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call(); call(); torch.cuda.synchronize()
    e0.record(); call(); e1.record(); torch.cuda.synchronize()
    once = max(e0.elapsed_time(e1), 1e-3)
    reps = int(min(50, max(3, 200.0 / 5 / once)))
    windows = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            call()
        e1.record(); torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / reps)
    windows.sort()
    return windows[2], windows[0], windows[4]


def fmt(t):
    return "not measured" if t is None else "%9.4f ms (%.4f ... %.4f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bench.txt"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    lines = ["# tools/bench_conv.py: ms per pass, median of five windows (min ... max), event to event, warm; N = %d, fp32, threads = 1" % N,
             "# yardsticks: torch (conv2d, nn.grad.conv2d_input, nn.grad.conv2d_weight on plain NCHW fp32) and libxsmm_sgemm_omp of the equivalent GEMM (the engine's ceiling)"]
    for s in (SHAPES[1:2] if args.quick else SHAPES):
        C_, K, H, W, R, S, u, pad = (s[k] for k in ("C", "K", "H", "W", "R", "S", "u", "pad"))
        ofh, ofw = (H + 2 * pad - R) // u + 1, (W + 2 * pad - S) // u + 1
        flop = 2.0 * N * K * C_ * R * S * ofh * ofw
        handle, status = xs.conv_create(N, C_, H, W, K, R, S, u, u, pad, pad, pad, pad, 0, 0, options=xs.DNN_CONV_OPTION_OVERWRITE)
        assert handle and 0 == status
        n_in, n_out, n_w = N * C_ * (H + 2 * pad) * (W + 2 * pad), N * K * ofh * ofw, K * C_ * R * S
        gen = torch.Generator(device="cuda").manual_seed(C_ + K)
        keep = {REG_IN: torch.rand(n_in, device="cuda", generator=gen) - 0.5, REG_FIL: torch.rand(n_w, device="cuda", generator=gen) - 0.5,
                GRAD_OUT: torch.rand(n_out, device="cuda", generator=gen) - 0.5, REG_OUT: torch.zeros(n_out, device="cuda"),
                GRAD_IN: torch.zeros(n_in, device="cuda"), GRAD_FIL: torch.zeros(n_w, device="cuda")}
        tensors = [xs.conv_bind_new(handle, t, a) for t, a in keep.items()]
        scratch = np.zeros(64, dtype=np.uint8)  # (never read or written: host memory will do)
        L.libxsmm_dnn_bind_scratch(handle, ALL, xs.dptr(scratch))
        # the yardsticks
        x = torch.rand((N, C_, H, W), device="cuda", generator=gen) - 0.5
        w = torch.rand((K, C_, R, S), device="cuda", generator=gen) - 0.5
        dy = torch.rand((N, K, ofh, ofw), device="cuda", generator=gen) - 0.5
        ref = {FWD: lambda: F.conv2d(x, w, stride=u, padding=pad), BWD: lambda: torch.nn.grad.conv2d_input(x.shape, w, dy, stride=u, padding=pad),
               UPD: lambda: torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=u, padding=pad)}
        m, n, k = K, N * ofh * ofw, C_ * R * S
        ga, gb, gc = (torch.rand(q, device="cuda", generator=gen) - 0.5 for q in (m * k, max(k * n, m * n), max(m * n, k * n)))
        gemm = {FWD: lambda: xs.xgemm_omp(xs.F32, "N", "N", m, n, k, 1.0, ga, m, gb, k, 0.0, gc, m),
                BWD: lambda: xs.xgemm_omp(xs.F32, "T", "N", k, n, m, 1.0, ga, m, gb, m, 0.0, gc, k),
                UPD: lambda: xs.xgemm_omp(xs.F32, "N", "T", m, k, n, 1.0, gb, m, gc, k, 0.0, ga, m)}
        for kind, name in ((FWD, "fwd"), (BWD, "bwd"), (UPD, "upd")):
            mine = timed(torch, lambda: xs.conv_execute(handle, kind))
            kernel = xs.last_kernel()
            try:
                theirs = timed(torch, ref[kind])
            except Exception as e:  # (a torch build without a convolution for this shape)
                theirs = None
                lines.append("# torch %s failed: %s" % (name, str(e).splitlines()[0][:120]))
            ceiling = timed(torch, gemm[kind])
            lines.append("C=%-3d K=%-3d %3dx%-3d %dx%d/%d %s %-14s %s  %6.2f TFLOP/s | torch %s | sgemm_omp %dx%dx%d %s  %6.2f TFLOP/s"
                         % (C_, K, H, W, R, S, u, name, kernel, fmt(mine), flop / mine[0] * 1e-9, fmt(theirs), m, n, k, fmt(ceiling), flop / ceiling[0] * 1e-9))
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_conv_layer(handle)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
