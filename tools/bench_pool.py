#!/usr/bin/env python3
"""The pooling layer against this code base's streaming ceiling and against torch.

Per shape, pass and element type: libxsmm_dnn_pooling_execute_st with threads = 1 (one launch of kernels/pool.hip) on device
tensors, and two yardsticks in the same run: libxsmm_matcopy moving the same number of bytes (what a streaming kernel of this
code base reaches), and torch.nn.functional.max_pool2d / avg_pool2d, forward and autograd backward, on a channels_last tensor
of the same logical shape. Shapes (N = 64): C = 64, 112 x 112, 3x3 / 2 pad 1, max; C = 256, 56 x 56, 2x2 / 2, max and avg;
C = 2048, 7 x 7 global avg. Every case is warmed up twice, then timed event to event in five windows of as many calls as fill
about 40 ms (3 ... 50); the median window is reported with the spread. Algorithmic bytes: input + output (+ mask) once each.
No gate. Usage: tools/bench_pool.py [--out FILE] [--quick] [--once KIND] (--once: one call of one case, for a counter run)"""
import argparse
import importlib
import os
import sys

os.environ.setdefault("LIBXSMM_AMD_JIT_ASYNC", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes / s
N = 64
SHAPES = [dict(C=64, H=112, W=112, R=3, S=3, u=2, pad=1, pools=("max",)), dict(C=256, H=56, W=56, R=2, S=2, u=2, pad=0, pools=("max", "avg")),
          dict(C=2048, H=7, W=7, R=7, S=7, u=1, pad=0, pools=("avg",))]
FWD, BWD = 0, 1
REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, MASK = 0, 3, 5, 6, 31


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


def layer(xs, torch, s, pool, bf16):
    """(handle, tensors kept alive, bytes of FWD, bytes of BWD)"""
    dt = xs.DNN_BF16 if bf16 else xs.DNN_F32
    handle, st = xs.pool_create(N, s["C"], s["H"], s["W"], s["R"], s["S"], s["u"], s["u"], s["pad"], s["pad"], datatype_in=dt, datatype_out=dt,
                                pooling_type=xs.DNN_POOLING_MAX if pool == "max" else xs.DNN_POOLING_AVG)
    assert handle and 0 == st
    ofh = (s["H"] + 2 * s["pad"] - s["R"]) // s["u"] + 1
    ofw = (s["W"] + 2 * s["pad"] - s["S"]) // s["u"] + 1
    n_in, n_out = N * s["C"] * s["H"] * s["W"], N * s["C"] * ofh * ofw
    tdt = torch.bfloat16 if bf16 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(s["C"])
    keep = {REG_IN: torch.randn(n_in, device="cuda", generator=gen).to(tdt), GRAD_OUT: torch.randn(n_out, device="cuda", generator=gen).to(tdt),
            REG_OUT: torch.zeros(n_out, device="cuda", dtype=tdt), GRAD_IN: torch.zeros(n_in, device="cuda", dtype=tdt)}
    if pool == "max":
        keep[MASK] = torch.full((n_out,), -1, device="cuda", dtype=torch.int32)
    tensors = [xs.pool_bind_new(handle, t, a) for t, a in keep.items()]
    es = 2 if bf16 else 4
    mask_bytes = 4 * n_out if pool == "max" else 0
    return handle, (keep, tensors), (n_in + n_out) * es + mask_bytes, (n_in + n_out) * es + mask_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_bench.txt"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--once", default=None, help="fwd or bwd: one call of max pooling at the first shape in fp32, nothing timed")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    if args.once:
        handle, keep, _, _ = layer(xs, torch, SHAPES[0], "max", False)
        assert 0 == xs.pool_execute(handle, FWD)
        if args.once == "bwd":
            assert 0 == xs.pool_execute(handle, BWD)
        torch.cuda.synchronize()
        return
    lines = ["# tools/bench_pool.py: ms per pass, median of five windows (min ... max), event to event, warm; N = %d" % N,
             "# bytes: input + output (+ mask), once each; frac = bytes / ms against 8 TB/s; matcopy: libxsmm_matcopy of the same byte count;",
             "# torch: max_pool2d / avg_pool2d on a channels_last tensor (forward; autograd backward)"]
    for s in (SHAPES[1:2] if args.quick else SHAPES):
        for pool in s["pools"]:
            for bf16 in (False, True):
                handle, keep, fwd_bytes, bwd_bytes = layer(xs, torch, s, pool, bf16)
                tdt = torch.bfloat16 if bf16 else torch.float32
                x = torch.randn(N, s["C"], s["H"], s["W"], device="cuda").to(tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                if pool == "max":
                    op = lambda: F.max_pool2d(x, (s["R"], s["S"]), s["u"], s["pad"])
                else:
                    op = lambda: F.avg_pool2d(x, (s["R"], s["S"]), s["u"], s["pad"], count_include_pad=True)
                y = op()
                gy = torch.randn_like(y)
                for kind, nbytes, torch_call in ((FWD, fwd_bytes, lambda: op()), (BWD, bwd_bytes, lambda: torch.autograd.grad(y, x, gy, retain_graph=True))):
                    def call():
                        assert 0 == xs.pool_execute(handle, kind)
                    ms = timed(torch, call)
                    half = nbytes // 2  # a copy reads and writes: half the bytes each way
                    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                    rows = half // 4096
                    cp = timed(torch, lambda: xs.matcopy(dst, src, 1, 4096, rows, 4096, 4096))
                    if kind == FWD:
                        with torch.no_grad():
                            tt = timed(torch, torch_call)
                    else:
                        tt = timed(torch, torch_call)
                    lines.append("C=%-4d %3dx%-3d %dx%d/%d %s %s %s: %.4f ms (%.4f ... %.4f)  %.1f MB  frac %.3f | matcopy %.4f ms (frac %.3f) | torch %.4f ms | torch / ours %.2f"
                                 % (s["C"], s["H"], s["W"], s["R"], s["S"], s["u"], pool, "bf16" if bf16 else "f32 ", "fwd" if kind == FWD else "bwd", ms[0], ms[1], ms[2],
                                    nbytes / 1e6, nbytes / (ms[0] * 1e-3) / PEAK, cp[0], nbytes / (cp[0] * 1e-3) / PEAK, tt[0], tt[0] / ms[0]))
                    print(lines[-1], flush=True)
                for t in keep[1]:
                    L.libxsmm_dnn_destroy_tensor(t)
                L.libxsmm_dnn_destroy_pooling(handle)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
