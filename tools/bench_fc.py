#!/usr/bin/env python3
"""The fully-connected layer against the path the same arithmetic had before it.

Per shape and pass: libxsmm_dnn_fullyconnected_execute_st with threads = 1 (one launch of kernels/fc.hip) on device tensors --
fp32 in format L, fp32 in format B (bn = bk = bc = 64 where they divide), bf16 -> fp32 in format L -- and the yardstick:
libxsmm_sgemm_omp (kernels/tgemm.hip) on the de-blocked plain fp32 operands, beta = 0. Shapes: the fully-connected layers of the
reference's samples/deeplearning/fullyconnecteddriver/run_resnet50.sh (N = 256: 2048 -> 1000... here with K = 1000 in format L
only, its block of 10) and N = 256 with C = K = 1024 and 4096. Every case is warmed up twice, then timed event to event over
as many calls as fill about 0.2 s (3 ... 50) in five windows; the median window is reported with the spread (min ... max).
No gate: the value of this path is the interface, one launch per pass and the reproducible bits. The tile rule
(LIBXSMM_AMD_FC_TILE) and the 64-tile's efficiency at small N are unmeasured until this has run; --tiles times both tiles.
Usage: tools/bench_fc.py [--out FILE] [--quick] [--tiles]"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 2048, 1000), (256, 1024, 1024), (256, 4096, 4096)]
FWD, BWD, UPD = 0, 1, 2
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_bench.txt"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--tiles", action="store_true")
    args = ap.parse_args()
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    lines = ["# tools/bench_fc.py: ms per pass, median of five windows (min ... max), event to event, warm; ratio = yardstick / layer",
             "# yardstick: libxsmm_sgemm_omp (tgemm) on plain fp32 operands, beta = 0. The tile rule and the 64-tile at small N are unmeasured apart from these lines."]
    for (N, Cc, K) in (SHAPES[1:2] if args.quick else SHAPES):
        gen = torch.Generator(device="cuda").manual_seed(N + Cc + K)
        x, w, dy = (torch.rand(n, device="cuda", generator=gen) - 0.5 for n in (N * Cc, K * Cc, N * K))
        y, dx, dw = (torch.zeros(n, device="cuda") for n in (N * K, N * Cc, K * Cc))
        # the yardstick, column-major: y^T (K x N) = w^T (K x C) x^T (C x N); dx^T (C x N) = w (C x K) dy^T (K x N); dw^T (K x C) = dy^T (K x N) x (N x C)
        base = {FWD: lambda: xs.xgemm_omp(xs.F32, "N", "N", K, N, Cc, 1.0, w, K, x, Cc, 0.0, y, K),
                BWD: lambda: xs.xgemm_omp(xs.F32, "N", "N", Cc, N, K, 1.0, w, Cc, dy, K, 0.0, dx, Cc),
                UPD: lambda: xs.xgemm_omp(xs.F32, "N", "T", K, Cc, N, 1.0, dy, K, x, Cc, 0.0, dw, K)}
        yard = {kind: timed(torch, call) for kind, call in base.items()}
        configs = [("L f32", dict()), ("L bf16", dict(datatype_in=xs.DNN_BF16))]
        if 0 == N % 64 and 0 == Cc % 64 and 0 == K % 64:
            configs.append(("B f32", dict(bn=64, bk=64, bc=64, buffer_format=xs.DNN_FORMAT_NCPACKED, filter_format=xs.DNN_FORMAT_CKPACKED)))
        for label, kw in configs:
            for tile in (("64", "128") if args.tiles else (None,)):
                if tile is None:
                    os.environ.pop("LIBXSMM_AMD_FC_TILE", None)
                else:
                    os.environ["LIBXSMM_AMD_FC_TILE"] = tile
                handle, status = xs.fc_create(N, Cc, K, threads=1, **kw)
                if not handle:
                    lines.append("N=%d C=%d K=%d %-7s no handle (status %d)" % (N, Cc, K, label, status))
                    continue
                lowp = "bf16" in label
                i16 = torch.int16
                bufs = {REG_IN: torch.zeros(N * Cc, device="cuda", dtype=i16) if lowp else x, GRAD_IN: torch.zeros(N * Cc, device="cuda", dtype=i16 if lowp else torch.float32),
                        REG_OUT: y, GRAD_OUT: dy, REG_FIL: torch.zeros(K * Cc, device="cuda", dtype=i16) if lowp else w,
                        GRAD_FIL: torch.zeros(K * Cc, device="cuda", dtype=i16 if lowp else torch.float32)}
                if lowp:
                    xs.convert_f32_bf16(x, bufs[REG_IN], N * Cc)
                    xs.convert_f32_bf16(w, bufs[REG_FIL], K * Cc)
                tensors = [xs.fc_bind_new(handle, t, b) for t, b in bufs.items()]
                st = C.c_uint(0)
                scratch = torch.zeros(L.libxsmm_dnn_fullyconnected_get_scratch_size(handle, C.byref(st)), device="cuda", dtype=torch.uint8)
                L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))  # (sized and bound as a caller would; never touched)
                for kind, name in ((FWD, "fwd"), (BWD, "bwd"), (UPD, "upd")):
                    med, lo, hi = timed(torch, lambda: xs.fc_execute(handle, kind))
                    ymed = yard[kind][0]
                    lines.append("N=%d C=%d K=%d %-7s %s tile=%-4s %-16s %8.4f ms (%.4f ... %.4f)  yardstick %8.4f ms (%.4f ... %.4f)  ratio %.2f  %.1f TFLOP/s"
                                 % (N, Cc, K, label, name, tile or "rule", xs.last_kernel(), med, lo, hi, ymed, yard[kind][1], yard[kind][2], ymed / med,
                                    2.0 * N * Cc * K / med * 1e-9))
                for t in tensors:
                    L.libxsmm_dnn_destroy_tensor(t)
                L.libxsmm_dnn_destroy_fullyconnected(handle)
    os.environ.pop("LIBXSMM_AMD_FC_TILE", None)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
