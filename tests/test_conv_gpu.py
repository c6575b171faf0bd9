"""The convolution layer on the GPU (include/libxsmm_dnn_convolution.h, kernels/conv.hip): FWD, BWD and UPD of every compute case,
bit for bit against the restatement of tests/conv_common.py (which tests/test_conv_cpu.py holds against the reference's captured
outputs). Destinations start as conv_common.inputs says -- ones bits where a pass overwrites, seeded values where it accumulates --
and lie between canary bands; their physical padding and every element no term reaches are part of the comparison, so whatever
must not be written shows.

One named exception to the bitwise comparison, for the special_* cases only (conv_common.same_bits): where both sides hold a NaN
its sign and payload are not compared -- x86 answers 0 * Inf with the negative default NaN, gfx950 with the positive one."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import conv_common as cc

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a tensor
CANARY = np.float32(-7.25e11)
DEST = {cc.FWD: (cc.REG_OUT, "out"), cc.BWD: (cc.GRAD_IN, "din"), cc.UPD: (cc.GRAD_FIL, "dw")}
FWD_KERNELS = {64: "conv_fwd_t64", 128: "conv_fwd_t128"}


class Layer:
    """a handle with its nine device tensors between canaries: inputs filled, destinations as before the passes"""
    SLOTS = {cc.REG_IN: "x", cc.REG_FIL: "w", cc.GRAD_OUT: "dout", cc.REG_BIAS: "bias", cc.REG_OUT: "out0", cc.GRAD_IN: "din0", cc.GRAD_FIL: "dw0",
             cc.REG_FIL_TR: None, cc.GRAD_BIAS: None}

    def __init__(self, xs, torch, d, data, scratch=True):
        self.xs, self.torch, self.L, self.data = xs, torch, xs.lib(), data
        self.h = cc.Handle(d)
        self.handle, st = xs.conv_create(*[d[k] for k in cc.DESC_FIELDS])
        assert self.handle and 0 == st
        self.buf, self.view, self.tensor = {}, {}, {}
        for t, key in self.SLOTS.items():
            n = cc.layout_size(self.h.layout(t)[1])[1]
            host = np.full(n + 2 * BAND, CANARY, dtype=np.float32)
            if key is None:
                host[BAND:BAND + n].view(np.uint8)[...] = 0xff
            else:
                host[BAND:BAND + n] = data[key].reshape(-1)
            self.buf[t] = torch.from_numpy(host).cuda()
            self.view[t] = self.buf[t][BAND:BAND + n]
            self.tensor[t] = xs.conv_bind_new(self.handle, t, self.view[t])
        # the caller's scratch is never read or written: host memory will do
        self.scratch = np.full(64, 0x5a, dtype=np.uint8)
        if scratch:
            assert 0 == self.L.libxsmm_dnn_bind_scratch(self.handle, cc.ALL, xs.dptr(self.scratch))

    def result(self, t):
        self.torch.cuda.synchronize()
        host = self.buf[t].cpu().numpy()
        assert np.all(host[:BAND] == CANARY) and np.all(host[-BAND:] == CANARY), "a canary band was overwritten"
        return host[BAND:-BAND]

    def check(self, t, want, nan_class=False):
        got = self.result(t)
        bad = int(np.sum(cc.bits(got) != cc.bits(want)))
        assert cc.same_bits(got, want, nan_class), "tensor %d differs in %d of %d elements" % (t, bad, want.size)

    def run(self, kind, start=0, tid=0):
        return self.xs.conv_execute(self.handle, kind, start, tid)

    def close(self):
        assert np.all(self.scratch == 0x5a)
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_conv_layer(self.handle)


def with_tile(tile, f):
    """f() with the FWD tile forced (the library reads the variable per call)"""
    os.environ["LIBXSMM_AMD_CONV_TILE"] = str(tile)
    try:
        return f()
    finally:
        del os.environ["LIBXSMM_AMD_CONV_TILE"]


@pytest.mark.parametrize("name", sorted(cc.COMPUTE_CASES))
def test_three_passes_bit_equal(xs, torch_gpu, name):
    """every compute case and pass; FWD with both tile sizes (the same bits)"""
    d = cc.COMPUTE_CASES[name]
    want = cc.expected(name)
    nan_class = name.startswith("special_")
    layer = Layer(xs, torch_gpu, d, want)
    assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)  # (BWD of the notrans case reads it)
    assert xs.last_kernel() == "conv_trans_filter"
    layer.check(cc.REG_FIL_TR, want["wtr"])
    launches = layer.L.libxsmm_amd_launch_count()
    assert 0 == with_tile(64, lambda: layer.run(cc.FWD))
    assert 1 == layer.L.libxsmm_amd_launch_count() - launches, "a pass with threads = 1 is one launch"
    assert xs.last_kernel() == FWD_KERNELS[64]
    layer.check(cc.REG_OUT, want["out"], nan_class)   # the physical padding keeps what it held: it is part of the comparison
    assert 0 == layer.run(cc.BWD)
    assert xs.last_kernel() == "conv_bwd"
    layer.check(cc.GRAD_IN, want["din"], nan_class)   # ... and so is every pixel no term reaches
    assert 0 == layer.run(cc.UPD)
    assert xs.last_kernel() == ("conv_upd_image" if layer.h.upd_per_image() else "conv_upd_gemm")
    layer.check(cc.GRAD_FIL, want["dw"], nan_class)
    for t, key in ((cc.REG_IN, "x"), (cc.REG_FIL, "w"), (cc.GRAD_OUT, "dout"), (cc.REG_BIAS, "bias")):
        layer.check(t, want[key])
    layer.close()
    layer = Layer(xs, torch_gpu, d, want)
    assert 0 == with_tile(128, lambda: layer.run(cc.FWD))
    assert xs.last_kernel() == FWD_KERNELS[128]
    layer.check(cc.REG_OUT, want["out"], nan_class)
    layer.close()


def test_the_cases_hold_what_they_are_for():
    """the tile crossings, the odd reduction length, the pixels no term reaches and the two forms of UPD"""
    H = lambda name: cc.Handle(cc.COMPUTE_CASES[name])  # noqa: E731
    for name, rows, pixels in (("t_13x11", 16, 2 * 13 * 11), ("t_k144", 144, 2 * 16), ("t_n5", 16, 5 * 36)):
        h = H(name)
        assert (h.d["K"], h.d["N"] * h.ofh * h.ofw) == (rows, pixels)
        assert (rows > 128 and rows % 128) or (pixels > 128 and pixels % 128)
    h = H("b_c3_7x7")
    assert h.d["C"] * h.d["R"] * h.d["S"] == 147 and (h.ifmblock, h.ofmblock) == (3, 16)
    assert [(H(n).ifmblock, H(n).ofmblock) for n in ("b_c24_k40", "b_c5_k7", "b_k18")] == [(8, 8), (5, 7), (16, 2)]
    assert [H(n).upd_per_image() for n in ("k3x3_s2_phys", "k3x3_s2_log", "k1x1_s2", "k1x1_s2_pad", "k3x3_log")] == [True, True, False, False, False]
    e = cc.expected("k1x1_s2_acc")
    assert np.array_equal(cc.bits(e["din"][:, :, 1::2, :, :]), cc.bits(e["din0"][:, :, 1::2, :, :]))  # no term reaches the odd rows
    assert np.all(cc.bits(cc.expected("k1x1_s2")["din"][:, :, 1::2, :, :]) == 0)                        # ... which overwrite sets to +0.0
    e = cc.expected("outpad")
    assert np.all(cc.bits(e["out"][:, :, 0, :, :]) == 0xffffffff) and np.all(cc.bits(e["out"][:, :, :, :2, :]) == 0xffffffff)


@pytest.mark.parametrize("name", ("k3x3_log", "b_c24_k40", "k3x3_s2_phys", "f7_o0"))
def test_threads_do_not_enter_the_bits(xs, torch_gpu, name):
    """threads = 3: the shares in turn, and in reverse order with start_thread = 2, give the bits of threads = 1"""
    d = dict(cc.COMPUTE_CASES[name], threads=3)
    want = cc.expected(name)
    for start, order in ((0, (0, 1, 2)), (2, (2, 1, 0))):
        layer = Layer(xs, torch_gpu, d, want)
        for kind, (dest, key) in DEST.items():
            work = layer.h.work(kind)
            shares = [layer.h.share(kind, t) for t in range(3)]
            assert shares[0][0] == 0 and shares[-1][1] == work and all(a[1] == b[0] for a, b in zip(shares, shares[1:]))
            launches = layer.L.libxsmm_amd_launch_count()
            assert 0 == layer.run(kind, start, start + 3) == layer.run(kind, start, start + 9)  # threads beyond the last
            assert 0 == layer.L.libxsmm_amd_launch_count() - launches
            assert cc.ERR_GENERAL == layer.run(kind, start + 1, start)                           # a negative logical thread
            first = True
            for tid in order:
                assert 0 == layer.run(kind, start, start + tid)
                if first and kind == cc.FWD and shares[tid][0] < shares[tid][1]:  # one share writes its items and nothing else
                    got = layer.result(dest).reshape(-1, layer.h.ofhp * layer.h.ofwp * layer.h.ofmblock)
                    mine = np.zeros(work, dtype=bool)
                    mine[shares[tid][0]:shares[tid][1]] = True
                    assert cc.same_bits(got[mine], want["out"].reshape(got.shape)[mine]) and cc.same_bits(got[~mine], want["out0"].reshape(got.shape)[~mine])
                first = False
            layer.check(dest, want[key])
        layer.close()


def test_shares_from_three_threads_with_own_streams(xs, torch_gpu):
    torch = torch_gpu
    name = "t_13x11"
    layer = Layer(xs, torch, dict(cc.COMPUTE_CASES[name], threads=3, N=2), cc.expected(name))
    torch.cuda.synchronize()
    status = [None] * 3

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = [layer.run(kind, 0, tid) for kind in (cc.FWD, cc.BWD, cc.UPD)]  # (no pass reads what another wrote)
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    workers = [threading.Thread(target=share, args=(tid,)) for tid in range(3)]
    for wk in workers:
        wk.start()
    for wk in workers:
        wk.join()
    assert status == [[0, 0, 0]] * 3
    for kind, (dest, key) in DEST.items():
        layer.check(dest, cc.expected(name)[key])
    layer.close()


def test_execute_runs_all_shares_and_scratch_kinds(xs, torch_gpu):
    """libxsmm_dnn_execute is the logical threads in turn; BWD asks for a scratch bound with BWD or ALL, UPD with UPD or ALL, FWD
    for none; the scratch is host memory and keeps its bytes"""
    name = "k3x3_s2_log"
    want = cc.expected(name)
    layer = Layer(xs, torch_gpu, dict(cc.COMPUTE_CASES[name], threads=2), want, scratch=False)
    assert cc.ERR_DATA_NOT_BOUND == layer.run(cc.BWD) == layer.run(cc.UPD)
    layer.L.libxsmm_dnn_execute(layer.handle, cc.FWD)
    layer.check(cc.REG_OUT, want["out"])
    assert 0 == layer.L.libxsmm_dnn_bind_scratch(layer.handle, cc.BWD, xs.dptr(layer.scratch))
    assert cc.ERR_DATA_NOT_BOUND == layer.run(cc.UPD)
    layer.L.libxsmm_dnn_execute(layer.handle, cc.BWD)
    layer.check(cc.GRAD_IN, want["din"])
    assert 0 == layer.L.libxsmm_dnn_release_scratch(layer.handle, cc.BWD) == layer.L.libxsmm_dnn_bind_scratch(layer.handle, cc.UPD, xs.dptr(layer.scratch))
    assert cc.ERR_DATA_NOT_BOUND == layer.run(cc.BWD)
    layer.L.libxsmm_dnn_execute(layer.handle, cc.UPD)
    layer.check(cc.GRAD_FIL, want["dw"])
    layer.close()


def roles_of(kind, want):
    """key -> (contents before the pass, contents after it, whether the pass writes the tensor)"""
    if kind == cc.FWD:
        return {cc.REG_IN: (want["x"], want["x"], False), cc.REG_FIL: (want["w"], want["w"], False), cc.REG_BIAS: (want["bias"], want["bias"], False),
                cc.REG_OUT: (want["out0"], want["out"], True)}
    if kind == cc.BWD:
        return {cc.GRAD_OUT: (want["dout"], want["dout"], False), cc.REG_FIL: (want["w"], want["w"], False), cc.GRAD_IN: (want["din0"], want["din"], True)}
    return {cc.REG_IN: (want["x"], want["x"], False), cc.GRAD_OUT: (want["dout"], want["dout"], False), cc.GRAD_FIL: (want["dw0"], want["dw"], True)}


def test_mixed_residency_complete_on_return(xs, torch_gpu):
    """only what a pass writes in pageable host memory and what it reads on the device, then the reverse: the one staging block
    skips the device-resident operands and still places the others. A staged destination travels both ways: f7_o0 accumulates
    into it, and the padding of outpad must come back as it went."""
    L = xs.lib()
    scratch = np.zeros(64, dtype=np.uint8)
    for name in ("f7_o0", "outpad", "k3x3_s2_phys"):
        d = cc.COMPUTE_CASES[name]
        want = cc.expected(name)
        for kind in (cc.FWD, cc.BWD, cc.UPD):
            for host_written in (True, False):
                handle, _ = xs.conv_create(*[d[k] for k in cc.DESC_FIELDS])
                assert 0 == L.libxsmm_dnn_bind_scratch(handle, cc.ALL, xs.dptr(scratch))
                tensors = cc.check_mixed_residency(torch_gpu, roles_of(kind, want), host_written, lambda t, m: xs.conv_bind_new(handle, t, m),
                                                   lambda: xs.conv_execute(handle, kind))
                for t in tensors:
                    L.libxsmm_dnn_destroy_tensor(t)
                L.libxsmm_dnn_destroy_conv_layer(handle)


def test_a_share_of_a_pageable_destination_travels_both_ways(xs, torch_gpu):
    """threads = 2, every tensor pageable: each call stages the whole destination, writes its share and brings the whole back"""
    name = "k3x3_log"
    d = dict(cc.COMPUTE_CASES[name], threads=2)
    want = cc.expected(name)
    handle, _ = xs.conv_create(*[d[k] for k in cc.DESC_FIELDS])
    scratch = np.zeros(64, dtype=np.uint8)
    assert 0 == xs.lib().libxsmm_dnn_bind_scratch(handle, cc.ALL, xs.dptr(scratch))
    host = {t: want[key].copy() for t, key in Layer.SLOTS.items() if key is not None}
    tensors = [xs.conv_bind_new(handle, t, a) for t, a in host.items()]
    for kind, (dest, key) in DEST.items():
        for tid in (1, 0):
            assert 0 == xs.conv_execute(handle, kind, 0, tid)
        assert cc.same_bits(host[dest], want[key]), key  # no wait in between
    for t in tensors:
        xs.lib().libxsmm_dnn_destroy_tensor(t)
    xs.lib().libxsmm_dnn_destroy_conv_layer(handle)


def test_trans_reg_filter_of_pageable_tensors(xs, torch_gpu):
    name = "b_c24_k40"
    d = cc.COMPUTE_CASES[name]
    want = cc.expected(name)
    handle, _ = xs.conv_create(*[d[k] for k in cc.DESC_FIELDS])
    w, wtr = want["w"].copy(), np.zeros_like(want["wtr"])
    tensors = [xs.conv_bind_new(handle, cc.REG_FIL, w), xs.conv_bind_new(handle, cc.REG_FIL_TR, wtr)]
    assert 0 == xs.lib().libxsmm_dnn_trans_reg_filter(handle)
    assert cc.same_bits(wtr, want["wtr"]) and cc.same_bits(w, want["w"])
    for t in tensors:
        xs.lib().libxsmm_dnn_destroy_tensor(t)
    xs.lib().libxsmm_dnn_destroy_conv_layer(handle)
