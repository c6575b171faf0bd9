#!/usr/bin/env python3
"""The fused batch-norm layer against this code base's streaming ceiling and against torch.

Per shape, pass and element type: libxsmm_dnn_fusedbatchnorm_execute_st with OPS_BN_RELU and threads = 1 (three launches of
kernels/bn.hip: partial sums, finish, apply) on device tensors, and in the same run: the same pass with OPS_BNSCALE_RELU on the
same tensors, which is the apply launch alone -- so the ordered partial sums (with the tiny finish) are timed as the difference
of the two; libxsmm_matcopy moving the same number of bytes (what a streaming kernel of this code base reaches); and
torch.nn.functional.batch_norm (training mode) followed by relu, forward and autograd backward, on a channels_last tensor of
the same logical shape. Shapes (N = 64), those of tools/bench_pool.py: C = 64, 112 x 112; C = 256, 56 x 56; C = 2048, 7 x 7
(49 pixels: less than one chunk of the partial sums, 8192 items); and C = 256, 28 x 28 for a plane of several chunks with 1024
items. Every case is warmed up twice, then timed event to event in five windows of as many calls as fill about 40 ms (3 ... 50);
the median window is reported with the spread. Algorithmic bytes: FWD reads x twice (statistics, apply) and writes out; BWD reads
x, dout and out and writes dout (first walk), then reads x and dout and writes din.
No gate. Usage: tools/bench_bn.py [--out FILE] [--quick]"""
import argparse
import importlib
import os
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes / s
N = 64
SHAPES = [dict(C=64, H=112, W=112), dict(C=256, H=56, W=56), dict(C=2048, H=7, W=7), dict(C=256, H=28, W=28)]
FWD, BWD = 0, 1
TYPES = dict(x=0, dout=6, out=5, din=3, gamma=20, beta=17, dgamma=21, dbeta=18, mean=23, rstd=24, var=25)
BN_RELU, BNSCALE_RELU = 9, 10


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


def layers(xs, torch, s, bf16):
    """two handles (BN_RELU, BNSCALE_RELU) bound to the same device tensors; returns (handles, things kept alive, elements)"""
    dt = xs.DNN_BF16 if bf16 else xs.DNN_F32
    tdt = torch.bfloat16 if bf16 else torch.float32
    n = N * s["C"] * s["H"] * s["W"]
    gen = torch.Generator(device="cuda").manual_seed(s["C"])
    keep = {k: torch.randn(n, device="cuda", generator=gen).to(tdt) for k in ("x", "dout")}
    keep.update({k: torch.zeros(n, device="cuda", dtype=tdt) for k in ("out", "din")})
    keep.update({k: torch.rand(s["C"], device="cuda", generator=gen) + 0.5 for k in ("gamma", "beta", "dgamma", "dbeta", "mean", "rstd", "var")})
    handles, tensors = [], []
    for ops in (BN_RELU, BNSCALE_RELU):
        handle, st = xs.bn_create(N, s["C"], s["H"], s["W"], datatype_in=dt, datatype_out=dt, fuse_ops=ops)
        assert handle and 0 == st
        tensors += [xs.bn_bind_new(handle, TYPES[k], a) for k, a in keep.items()]
        handles.append(handle)
    return handles, (keep, tensors), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_bench.txt"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    lines = ["# tools/bench_bn.py: ms per pass, median of five windows (min ... max), event to event, warm; N = %d, OPS_BN_RELU, threads = 1" % N,
             "# bytes: FWD 2 reads of x + out; BWD x, dout, out read and dout written, then x, dout read and din written; frac = bytes / ms against 8 TB/s",
             "# apply: the same pass with OPS_BNSCALE_RELU (the apply launch alone); stats = pass - apply: the ordered partial sums and the finish",
             "# items = N * C / 16 work-groups of the partial sums; matcopy: libxsmm_matcopy of the same byte count; torch: batch_norm (training) + relu, channels_last"]
    for s in (SHAPES[1:2] if args.quick else SHAPES):
        for bf16 in (False, True):
            handles, keep, n = layers(xs, torch, s, bf16)
            es = 2 if bf16 else 4
            tdt = torch.bfloat16 if bf16 else torch.float32
            x = torch.randn(N, s["C"], s["H"], s["W"], device="cuda").to(tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            w = torch.ones(s["C"], device="cuda", dtype=tdt, requires_grad=True)
            b = torch.zeros(s["C"], device="cuda", dtype=tdt, requires_grad=True)
            op = lambda: F.relu(F.batch_norm(x, None, None, w, b, True))
            y = op()
            gy = torch.randn_like(y)
            for kind, nbytes, torch_call in ((FWD, 3 * n * es, lambda: op()), (BWD, 7 * n * es, lambda: torch.autograd.grad(y, (x, w, b), gy, retain_graph=True))):
                ms = timed(torch, lambda: xs.bn_execute(handles[0], kind))
                ap_ms = timed(torch, lambda: xs.bn_execute(handles[1], kind))
                half = nbytes // 2  # a copy reads and writes: half the bytes each way
                src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                rows = half // 4096
                cp = timed(torch, lambda: xs.matcopy(dst, src, 1, 4096, rows, 4096, 4096))
                if kind == FWD:
                    with torch.no_grad():
                        tt = timed(torch, torch_call)
                else:
                    tt = timed(torch, torch_call)
                stats_bytes = (n if kind == FWD else 4 * n) * es
                stats_ms = max(ms[0] - ap_ms[0], 1e-6)
                lines.append("C=%-4d %3dx%-3d items %-5d %s %s: %.4f ms (%.4f ... %.4f)  %.1f MB  frac %.3f | apply %.4f ms | stats %.4f ms (%.1f GB/s) | "
                             "matcopy %.4f ms (frac %.3f) | torch %.4f ms | torch / ours %.2f"
                             % (s["C"], s["H"], s["W"], N * s["C"] // 16, "bf16" if bf16 else "f32 ", "fwd" if kind == FWD else "bwd", ms[0], ms[1], ms[2], nbytes / 1e6,
                                nbytes / (ms[0] * 1e-3) / PEAK, ap_ms[0], stats_ms, stats_bytes / (stats_ms * 1e-3) / 1e9, cp[0], nbytes / (cp[0] * 1e-3) / PEAK, tt[0], tt[0] / ms[0]))
                print(lines[-1], flush=True)
            for t in keep[1]:
                L.libxsmm_dnn_destroy_tensor(t)
            for handle in handles:
                L.libxsmm_dnn_destroy_fusedbatchnorm(handle)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
