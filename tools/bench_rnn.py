"""Developer benchmark of the RNN cell layer's forward pass: LSTM and GRU at N = 64, C = K = 512 and 1024, T = 50, and
the tanh cell at 1024, in both plans (LIBXSMM_AMD_RNN_PLAN=split / whole), warm, event to event on one stream, the median of five
windows with their spread. Two comparison columns, neither a threshold: torch's nn.LSTM / nn.GRU / nn.RNN forward in fp32 (other
bits: informational) and libxsmm_sgemm_omp of the equivalent GEMMs -- per step (G*K x N x C and G*K x N x K, T times each) and w.x
for all steps at once (G*K x T*N x C) plus the T recurrent ones: the ceiling this engine gives those sizes.

    python tools/bench_rnn.py [--reps 5] [--out profiles/rnn_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RELU, SIGMOID, TANH, LSTM, GRU = range(5)
X, CSP, HP, W, R, B, CS, H, GI, GF, GO, GCI, GCO = 33, 34, 35, 36, 37, 40, 41, 42, 51, 52, 53, 54, 55
SHAPES = [("lstm", LSTM, 64, 512, 512, 50), ("lstm", LSTM, 64, 1024, 1024, 50), ("gru", GRU, 64, 512, 512, 50), ("gru", GRU, 64, 1024, 1024, 50),
          ("rnn_tanh", TANH, 64, 1024, 1024, 50)]


def windows(torch, fn, reps, inner=3):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    xs = importlib.import_module("libxsmm-1_amd")
    L = xs.lib()
    torch.cuda.set_device(0)
    L.libxsmm_amd_set_stream(None)
    lines = ["# RNN cell forward, fp32, one MI355X; ms per pass: median [min, max] of %d windows" % args.reps,
             "# cell N C K T | split | whole | torch | sgemm per step | sgemm all steps + T recurrent"]
    for name, cell, N, Cc, K, T in SHAPES:
        G = 4 if cell == LSTM else (3 if cell == GRU else 1)
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s: (torch.rand(*s, device="cuda", generator=g) - 0.5) * 0.1  # noqa: E731
        t = {X: rnd(T, N, Cc), HP: rnd(T, N, K), CSP: rnd(T, N, K), W: rnd(Cc, G * K), R: rnd(K, G * K), B: rnd(G * K)}
        for key in (CS, H, GI, GF, GO, GCI, GCO):
            t[key] = torch.zeros(T, N, K, device="cuda")
        z = torch.zeros(T * N * K + 16, device="cuda")
        handle, st = xs.rnn_create(N, Cc, K, T, cell, bn=N, bc=64, bk=64)
        assert handle and st == 0
        used = [X, HP, W, R, B, H] + ([CSP, CS, GI, GF, GO, GCI, GCO] if cell == LSTM else ([GI, GF, GO, GCI] if cell == GRU else []))
        tensors = [xs.rnn_bind_new(handle, key, t[key]) for key in used]
        assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, 0, xs.dptr(z)) or G > 1
        res = {}
        for plan in ("split", "whole"):
            os.environ["LIBXSMM_AMD_RNN_PLAN"] = plan
            res[plan] = windows(torch, lambda: xs.rnn_execute(handle, 0), args.reps)
        os.environ.pop("LIBXSMM_AMD_RNN_PLAN", None)
        mod = {LSTM: torch.nn.LSTM, GRU: torch.nn.GRU}.get(cell, torch.nn.RNN)(Cc, K).cuda().float()
        with torch.no_grad():
            res["torch"] = windows(torch, lambda: mod(t[X]), args.reps)
        # the GEMMs, column-major: gates (G*K x rows) = w^T-as-stored (G*K x C, ld G*K) times x (C x rows, ld C)
        pre = torch.zeros(T * N, G * K, device="cuda")

        def per_step():
            for j in range(T):
                xs.xgemm_omp(xs.F32, "N", "N", G * K, N, Cc, 1.0, t[W], G * K, t[X][j], Cc, 0.0, pre[j * N:], G * K)
                xs.xgemm_omp(xs.F32, "N", "N", G * K, N, K, 1.0, t[R], G * K, t[H][j], K, 1.0, pre[j * N:], G * K)

        def all_steps():
            xs.xgemm_omp(xs.F32, "N", "N", G * K, T * N, Cc, 1.0, t[W], G * K, t[X], Cc, 0.0, pre, G * K)
            for j in range(T):
                xs.xgemm_omp(xs.F32, "N", "N", G * K, N, K, 1.0, t[R], G * K, t[H][j], K, 1.0, pre[j * N:], G * K)

        res["step"], res["all"] = windows(torch, per_step, args.reps), windows(torch, all_steps, args.reps)
        fmt = lambda r: "%8.3f [%7.3f, %7.3f]" % r  # noqa: E731
        lines.append("%-8s %3d %4d %4d %2d | %s | %s | %s | %s | %s" % (name, N, Cc, K, T, fmt(res["split"]), fmt(res["whole"]), fmt(res["torch"]),
                                                                       fmt(res["step"]), fmt(res["all"])))
        print(lines[-1], flush=True)
        for tensor in tensors:
            L.libxsmm_dnn_destroy_tensor(tensor)
        L.libxsmm_dnn_destroy_rnncell(handle)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
