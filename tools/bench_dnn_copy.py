#!/usr/bin/env python3
"""DNN tensor copy-in / copy-out on the GPU (libxsmm_amd_dnn_copyin_tensor_async / _copyout_tensor_async, device to device): time per
call, event to event and warm, the median of five windows with their spread (max - min over the median); GB/s counting the tensor's
bytes once in and once out. Next to each: a hipMemcpyAsync device-to-device of the same bytes in the same session (the
yardstick), and -- with --parent, the path of a libxsmm.so built from the parent commit -- one call of that library's
libxsmm_dnn_copyin_tensor on the same device operands, timed by the host clock (it is complete on return; once per shape: it travels
through a host image).
    python3 tools/bench_dnn_copy.py [--windows 5] [--calls 20] [--parent PATH] [--out profiles/dnn_copy_bench.txt]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    assert torch.cuda.is_available()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    parent = C.CDLL(args.parent) if args.parent else None
    if parent is not None:
        parent.libxsmm_dnn_link_tensor.restype = C.c_void_p
        parent.libxsmm_dnn_link_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        parent.libxsmm_dnn_copyin_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        """seconds per call: (median, spread) over the windows"""
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                f()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e-3 / args.calls)
        med = statistics.median(times)
        return med, (max(times) - min(times)) / med

    def resized(layout, sizes):
        st = C.c_uint()
        copy = L.libxsmm_dnn_duplicate_tensor_datalayout(layout, C.byref(st))
        for j, n in enumerate(sizes):
            copy.contents.dim_size[j] = n
        return copy

    bn32, _ = xs.bn_create(64, 256, 56, 56)
    bn16, _ = xs.bn_create(64, 256, 56, 56, datatype_in=xs.DNN_BF16, datatype_out=xs.DNN_BF16)
    conv, _ = xs.conv_create(1, 512, 3, 3, 512, 3, 3)
    fcl, _ = xs.fc_create(64, 64, 64)
    fc_layout = resized(xs.fc_layout(fcl, xs.DNN_REGULAR_FILTER)[0], [64, 64, 1, 1, 64, 64])
    shapes = [("activation N=64 C=256 56x56 fp32", xs.bn_layout(bn32, xs.DNN_REGULAR_INPUT)[0], xs.DNN_FORMAT_NCHW),
              ("activation N=64 C=256 56x56 bf16", xs.bn_layout(bn16, xs.DNN_REGULAR_INPUT)[0], xs.DNN_FORMAT_NCHW),
              ("filter 512x512x3x3 fp32", xs.conv_layout(conv, xs.DNN_REGULAR_FILTER)[0], xs.DNN_FORMAT_KCRS),
              ("FC filter 4096x4096 fp32, blocks 64x64", fc_layout, xs.DNN_FORMAT_KCRS)]
    emit("# shape | bytes | plan (form ts blocks rows run rows/pass items groups) | direction kernel time_us spread GB/s | hipMemcpyAsync d2d time_us GB/s | "
         "copy / memcpy | parent's copy-in time_us, parent / async")
    for what, layout, fmt in shapes:
        fields = xs.dnn_layout_fields(layout)
        nbytes = (4 if fields[3] == xs.DNN_F32 else 2)
        for s in fields[2]:
            nbytes *= s
        plain = torch.randint(0, 255, (nbytes,), device="cuda", dtype=torch.uint8)
        blocked = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
        tensor, st = xs.dnn_link_tensor(layout, blocked)
        assert tensor and 0 == st
        _, plan = xs.dnn_copy_plan(layout, fmt)
        tm, sm = timed(lambda: hip.hipMemcpyAsync(blocked.data_ptr(), plain.data_ptr(), nbytes, 3, None))
        gm = 2 * nbytes / tm / 1e9
        tp = None
        if parent is not None:
            st = C.c_uint()
            pt = parent.libxsmm_dnn_link_tensor(C.cast(layout, C.c_void_p), blocked.data_ptr(), C.byref(st))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert 0 == parent.libxsmm_dnn_copyin_tensor(pt, plain.data_ptr(), fmt)
            tp = time.perf_counter() - t0
        for direction, f in (("in", lambda: L.libxsmm_amd_dnn_copyin_tensor_async(tensor, plain.data_ptr(), fmt)),
                             ("out", lambda: L.libxsmm_amd_dnn_copyout_tensor_async(tensor, plain.data_ptr(), fmt))):
            assert 0 == f()
            t, s = timed(f)
            g = 2 * nbytes / t / 1e9
            tail = ("| %9.0f %7.1f" % (tp * 1e6, tp / t)) if tp is not None and "in" == direction else "|"
            emit("%-40s | %10d | %s | %-3s %-20s %9.1f %5.2f %7.0f | %9.1f %7.0f | %5.2f %s" % (
                what, nbytes, " ".join(str(x) for x in plan), direction, xs.last_kernel(), t * 1e6, s, g, tm * 1e6, gm, g / gm, tail))
        L.libxsmm_dnn_destroy_tensor(tensor)
        del plain, blocked
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
