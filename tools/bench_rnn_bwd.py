"""Developer benchmark of the RNN cell layer's backward and update passes: LSTM at N = 64, C = K = 512 and 1024,
T = 50, and the tanh cell at 1024; kinds BWD, UPD and BWDUPD, warm, event to event on one stream, the median of five windows with
their spread. Two comparison columns, neither a threshold: torch autograd through nn.LSTM / nn.RNN in fp32 (forward plus backward,
and the forward alone; other bits: informational) and libxsmm_sgemm_omp of the equivalent GEMMs of BWDUPD -- T recurrent ones
(K x N x G*K), dx of all steps (C x T*N x G*K) and dw, dr (G*K x C x T*N, G*K x K x T*N): the ceiling this engine gives those sizes.

    python tools/bench_rnn_bwd.py [--reps 5] [--out profiles/rnn_bwd_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TANH, LSTM = 2, 3
BWD, UPD, BWDUPD = 1, 2, 3
X, CSP, HP, W, R, B, CS, H, DX, DCSP, DHP, DW, DR, DB, DCS, DH, GI, GF, GO, GCI, GCO = (33, 34, 35, 36, 37, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50,
                                                                                        51, 52, 53, 54, 55)
SHAPES = [("lstm", LSTM, 64, 512, 512, 50), ("lstm", LSTM, 64, 1024, 1024, 50), ("rnn_tanh", TANH, 64, 1024, 1024, 50)]


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
    lines = ["# RNN cell backward / update, fp32, one MI355X; ms per pass: median [min, max] of %d windows" % args.reps,
             "# cell N C K T | BWD | UPD | BWDUPD | torch fwd+bwd | torch fwd | sgemm equivalents of BWDUPD"]
    for name, cell, N, Cc, K, T in SHAPES:
        G = 4 if cell == LSTM else 1
        LD = G * K
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s: (torch.rand(*s, device="cuda", generator=g) - 0.5) * 0.1  # noqa: E731
        t = {X: rnd(T, N, Cc), HP: rnd(T, N, K), CSP: rnd(T, N, K), W: rnd(Cc, LD), R: rnd(K, LD), B: rnd(LD), DH: rnd(T, N, K), DCS: rnd(T, N, K)}
        for key in (CS, H, GI, GF, GO, GCI, GCO, DCSP, DHP):
            t[key] = torch.zeros(T, N, K, device="cuda")
        t[DX], t[DW], t[DR], t[DB] = torch.zeros(T, N, Cc, device="cuda"), torch.zeros(Cc, LD, device="cuda"), torch.zeros(K, LD, device="cuda"), torch.zeros(LD, device="cuda")
        z = torch.zeros(T * N * K + 16, device="cuda")
        handle, st = xs.rnn_create(N, Cc, K, T, cell, bn=N, bc=64, bk=64)
        assert handle and st == 0
        used = [X, HP, W, R, B, H, DX, DW, DR, DB, DH] + ([CSP, CS, GI, GF, GO, GCI, GCO, DCS, DCSP, DHP] if cell == LSTM else [])
        tensors = [xs.rnn_bind_new(handle, key, t[key]) for key in used]
        assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, 0, xs.dptr(z)) or G > 1
        assert 0 == xs.rnn_execute(handle, 0)  # the forward pass: what the backward reads
        res = {}
        for kind in (BWD, UPD, BWDUPD):
            assert 0 == xs.rnn_execute(handle, kind)
            res[kind] = windows(torch, lambda: xs.rnn_execute(handle, kind), args.reps)
        mod = {LSTM: torch.nn.LSTM}.get(cell, torch.nn.RNN)(Cc, K).cuda().float()
        xin = t[X].clone().requires_grad_(True)

        def autograd():
            out, _ = mod(xin)
            out.backward(t[DH])

        res["torch"] = windows(torch, autograd, args.reps)
        with torch.no_grad():
            res["torch_fwd"] = windows(torch, lambda: mod(t[X]), args.reps)
        # the GEMMs, column-major: a filter [rows][LD] as stored is an LD x rows matrix; the deltas [T*N][LD] an LD x T*N one
        delta, dout = rnd(T * N, LD), torch.zeros(N, K, device="cuda")

        def gemms():
            for j in range(T):
                xs.xgemm_omp(xs.F32, "T", "N", K, N, LD, 1.0, t[R], LD, delta[j * N:], LD, 0.0, dout, K)
            xs.xgemm_omp(xs.F32, "T", "N", Cc, T * N, LD, 1.0, t[W], LD, delta, LD, 0.0, t[DX], Cc)
            xs.xgemm_omp(xs.F32, "N", "T", LD, Cc, T * N, 1.0, delta, LD, t[X], Cc, 0.0, t[DW], LD)
            xs.xgemm_omp(xs.F32, "N", "T", LD, K, T * N, 1.0, delta, LD, t[H], K, 0.0, t[DR], LD)

        res["gemm"] = windows(torch, gemms, args.reps)
        fmt = lambda r: "%8.3f [%7.3f, %7.3f]" % r  # noqa: E731
        lines.append("%-8s %3d %4d %4d %2d | %s | %s | %s | %s | %s | %s" % (name, N, Cc, K, T, fmt(res[BWD]), fmt(res[UPD]), fmt(res[BWDUPD]), fmt(res["torch"]),
                                                                            fmt(res["torch_fwd"]), fmt(res["gemm"])))
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
