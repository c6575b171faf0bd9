"""The pooling layer on the GPU (include/libxsmm_dnn_pooling.h, kernels/pool.hip): FWD and BWD, max and average, fp32 and bf16,
bit for bit against the numpy restatement of tests/pool_common.py (which tests/test_pool_cpu.py holds against the reference's
captured outputs). Destinations are pre-filled with NaN / 0xffff and the mask with -1; they lie between canary bands, and their
physical padding holds the same fill, so whatever must not be written shows."""
import ctypes as C
import threading

import numpy as np
import pytest

import pool_common as pc

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a tensor (a multiple of 16 bytes in every element type)
CANARY = {np.dtype(np.float32): np.float32(-7.25e11), np.dtype(np.uint16): np.uint16(0x7b7b), np.dtype(np.int32): np.int32(-77)}
_expect = {}


def case_data(name, cases=pc.COMPUTE_CASES):
    """the tensors of a case after FWD and BWD (pool_common.expected), computed once"""
    if name not in _expect:
        _expect[name] = pc.expected(name, cases[name])
    return _expect[name]


class Layer:
    """a handle with its five device tensors: inputs filled, destinations NaN / 0xffff / -1 between canaries"""
    SLOTS = {pc.REG_IN: "x", pc.GRAD_OUT: "dout", pc.REG_OUT: "out", pc.GRAD_IN: "din", pc.MASK: "mask"}

    def __init__(self, xs, torch, d, want, mask_from=None):
        self.xs, self.torch, self.L, self.want = xs, torch, xs.lib(), want
        self.h = pc.Handle(d)
        self.handle, st = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
        assert self.handle and 0 == st
        self.buf, self.view, self.tensor = {}, {}, {}
        shapes = {pc.REG_IN: self.h.in_shape(), pc.GRAD_IN: self.h.in_shape(), pc.REG_OUT: self.h.out_shape(), pc.GRAD_OUT: self.h.out_shape(), pc.MASK: self.h.mask_shape()}
        for t, key in self.SLOTS.items():
            if t == pc.MASK and d["pooling_type"] != pc.MAX:
                continue
            dt = np.dtype(np.int32) if t == pc.MASK else np.dtype(pc.elem_dtype(self.h))
            n = int(np.prod(shapes[t]))
            host = np.full(n + 2 * BAND, CANARY[dt], dtype=dt)
            if t in (pc.REG_IN, pc.GRAD_OUT):
                host[BAND:BAND + n] = want[key].reshape(-1)
            elif t == pc.MASK:
                host[BAND:BAND + n] = pc.SENTINEL if mask_from is None else mask_from.reshape(-1)
            else:
                host[BAND:BAND + n].view(np.uint8)[...] = 0xff
            # (torch has no uint16 arithmetic: the bytes travel as int16)
            self.buf[t] = torch.from_numpy(host.view(np.int16) if dt == np.uint16 else host).cuda()
            self.view[t] = self.buf[t][BAND:BAND + n]
            self.tensor[t] = xs.pool_bind_new(self.handle, t, self.view[t])

    def result(self, t):
        self.torch.cuda.synchronize()
        host = self.buf[t].cpu().numpy()
        if host.dtype == np.int16:
            host = host.view(np.uint16)
        canary = CANARY[host.dtype]
        assert np.all(host[:BAND] == canary) and np.all(host[-BAND:] == canary), "a canary band was overwritten"
        return host[BAND:-BAND]

    def check(self, t, want=None):
        want = self.want[self.SLOTS[t]] if want is None else want
        got = self.result(t)
        assert got.tobytes() == want.tobytes(), "tensor %d differs in %d of %d elements" % (t, int(np.sum(got.view(np.uint8) != want.reshape(-1).view(np.uint8))), want.size)

    def run(self, kind, start=0, tid=0):
        return self.xs.pool_execute(self.handle, kind, start, tid)

    def close(self):
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_pooling(self.handle)


@pytest.mark.parametrize("name", sorted(pc.COMPUTE_CASES))
def test_fwd_and_bwd_bit_equal(xs, torch_gpu, name):
    d = pc.COMPUTE_CASES[name]
    want = case_data(name)
    layer = Layer(xs, torch_gpu, d, want)
    is_max = d["pooling_type"] == pc.MAX
    launches = layer.L.libxsmm_amd_launch_count()
    assert 0 == layer.run(pc.FWD)                       # no scratch is bound: execute_st does not ask for it
    assert 1 == layer.L.libxsmm_amd_launch_count() - launches, "a pass with threads = 1 is one launch"
    assert xs.last_kernel() == "pool_fwd_%s_%s" % ("max" if is_max else "avg", "f32" if layer.h.f32 else "bf16")
    layer.check(pc.REG_OUT)                             # the physical padding keeps its fill: it is part of the comparison
    if is_max:
        layer.check(pc.MASK)
    assert 0 == layer.run(pc.BWD)
    assert xs.last_kernel().startswith("pool_bwd_")
    layer.check(pc.GRAD_IN)
    layer.check(pc.REG_IN)
    layer.check(pc.GRAD_OUT)
    layer.close()


def test_the_cases_hold_what_they_are_for():
    """ties in most windows of the alphabet kind, zeros where no window reaches, nine covering outputs in (g).
    Nine draws from seven values share their maximum with probability 1 - 9/7 * sum((j/7)**8 for j < 7) = 0.522: "most" by a
    small margin, so the share is counted where the sample carries it, over the 15 x 15 whole windows of (h) (14400 windows with
    the lanes, a standard deviation of 0.004). (a) has four whole windows per plane: there the test asks that ties occur and that
    the last maximum would be another element than the first, so a >= in place of > shows in the mask."""
    def whole_windows(name, outputs):
        x = case_data(name)["x"]
        first = 2 * outputs[0] - 1      # 3x3, stride 2, pad 1: output o reads rows 2o-1 .. 2o+1
        last = 2 * outputs[-1] - 1
        return np.stack([x[:, first + kh:last + kh + 1:2, first + kw:last + kw + 1:2, :] for kh in range(3) for kw in range(3)])
    win = whole_windows("h_max_f32_t", range(1, 16))
    assert win.shape[1:] == (4, 15, 15, 16)
    assert np.mean(np.sum(win == win.max(axis=0), axis=0) > 1) > 0.5
    win = whole_windows("a_max_f32_t", range(1, 3))
    assert win.shape[1:] == (4, 2, 2, 16)
    assert np.any(win.argmax(axis=0) != 8 - win[::-1].argmax(axis=0))
    for name, holes in (("d_max_f32_n", (slice(None), 7)), ("e_avg_f32_n", (slice(None), 2))):
        din = case_data(name)["din"]
        assert np.all(din[:, holes[1], :, :].view(np.uint32) == 0) and np.all(din[:, :, holes[1], :].view(np.uint32) == 0)  # +0.0
    h = pc.Handle(pc.COMPUTE_CASES["g_avg_f32_n"])
    assert (h.ofh, h.ofw) == (6, 6) and pc.Handle(pc.COMPUTE_CASES["h_max_f32_n"]).ofw == 17 and pc.Handle(pc.COMPUTE_CASES["f_max_f32_n"]).ofw == 1


@pytest.mark.parametrize("name", sorted(pc.SPECIAL_CASES))
def test_nan_and_lowest_windows(xs, torch_gpu, name):
    """a window of NaN and a window of -FLT_MAX (bf16: -Inf): the output is -FLT_MAX (truncated in bf16), the mask keeps -1,
    and BWD on that mask finishes and ignores those elements -- as it ignores values no FWD could have written"""
    d = pc.SPECIAL_CASES[name]
    want = case_data(name, pc.SPECIAL_CASES)
    layer = Layer(xs, torch_gpu, d, want)
    assert 0 == layer.run(pc.FWD)
    layer.check(pc.REG_OUT)
    layer.check(pc.MASK)
    assert 33 == int(np.sum(layer.result(pc.MASK) == pc.SENTINEL))
    assert 0 == layer.run(pc.BWD)
    layer.check(pc.GRAD_IN)
    layer.close()
    # masks FWD could not have written: far out of range, another lane, an element outside the output's window
    bad = want["mask"].copy()
    bad[0, 1, 1, :] = 2 ** 30
    bad[1, 0, 0, :] = np.roll(bad[1, 0, 0, :], 1)
    bad[2, 2, 2, :] = np.arange(16)          # pixel (0, 0): inside the plane, outside the window of output (2, 2)
    bad[3, 0, 0, :] = -5
    din = np.full(layer.h.in_shape(), 0, dtype=pc.elem_dtype(layer.h))
    din.view(np.uint8)[...] = 0xff
    pc.backward(layer.h, want["dout"], bad, din)
    assert din.tobytes() != want["din"].tobytes()
    layer = Layer(xs, torch_gpu, d, want, mask_from=bad)
    assert 0 == layer.run(pc.BWD)
    layer.check(pc.GRAD_IN, din)
    layer.close()


@pytest.mark.parametrize("name", ("a_max_f32_n", "b_avg_bf16_n", "g_max_bf16_t"))
def test_threads_do_not_enter_the_bits(xs, torch_gpu, name):
    """threads = 3 over four items: shares of 2, 2 and 0; in reverse order with start_thread = 2"""
    d = dict(pc.COMPUTE_CASES[name], threads=3)
    want = case_data(name)
    is_max = d["pooling_type"] == pc.MAX
    for start, order in ((0, (0, 1, 2)), (2, (2, 1, 0))):
        layer = Layer(xs, torch_gpu, d, want)
        assert [layer.h.share(t) for t in range(3)] == [(0, 2), (2, 4), (4, 4)]
        for kind, dest in ((pc.FWD, pc.REG_OUT), (pc.BWD, pc.GRAD_IN)):
            launches = layer.L.libxsmm_amd_launch_count()
            assert 0 == layer.run(kind, start, start + 2) == layer.run(kind, start, start + 9)   # the empty share, a thread beyond
            assert 0 == layer.L.libxsmm_amd_launch_count() - launches
            assert pc.ERR_GENERAL == layer.run(kind, start + 1, start)                          # a negative logical thread
            if kind == pc.FWD:  # one share writes its items and nothing else
                assert 0 == layer.run(kind, start, start + 1)
                got = layer.result(dest).reshape(layer.h.out_shape())
                assert got[2:].tobytes() == want["out"][2:].tobytes() and np.all(got[:2].view(np.uint8) == 0xff)
            for tid in order:
                assert 0 == layer.run(kind, start, start + tid)
            layer.check(dest)
            if is_max:
                layer.check(pc.MASK)
        layer.close()


def test_shares_from_three_threads_with_own_streams(xs, torch_gpu):
    torch = torch_gpu
    name = "h_max_f32_n"
    layer = Layer(xs, torch, dict(pc.COMPUTE_CASES[name], threads=3), case_data(name))
    torch.cuda.synchronize()
    status = [None] * 3

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = [layer.run(kind, 0, tid) for kind in (pc.FWD, pc.BWD)]  # (BWD of a share reads what its own FWD wrote)
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    workers = [threading.Thread(target=share, args=(tid,)) for tid in range(3)]
    for wk in workers:
        wk.start()
    for wk in workers:
        wk.join()
    assert status == [[0, 0]] * 3
    for t in (pc.REG_OUT, pc.MASK, pc.GRAD_IN):
        layer.check(t)
    layer.close()


def test_statuses(xs, torch_gpu):
    """a negative logical thread, a mask that is not I32, and execute_st with and without a bound scratch (never written)"""
    torch = torch_gpu
    name = "c_max_f32_n"
    layer = Layer(xs, torch, pc.COMPUTE_CASES[name], case_data(name))
    assert pc.ERR_GENERAL == layer.run(pc.FWD, 1, 0) == layer.run(pc.BWD, 5, 4)
    size = layer.L.libxsmm_dnn_pooling_get_scratch_size(layer.handle, C.byref(C.c_uint()))
    assert size == layer.h.scratch()
    scratch = torch.full((size,), 0x5a, dtype=torch.uint8, device="cuda")
    assert 0 == layer.L.libxsmm_dnn_pooling_bind_scratch(layer.handle, xs.dptr(scratch))
    assert 0 == layer.run(pc.FWD) == layer.run(pc.BWD)
    assert 0 == layer.L.libxsmm_dnn_pooling_release_scratch(layer.handle)
    assert 0 == layer.run(pc.FWD) == layer.run(pc.BWD)
    for t in (pc.REG_OUT, pc.MASK, pc.GRAD_IN):
        layer.check(t)
    assert np.all(scratch.cpu().numpy() == 0x5a), "the scratch is never written"
    layer.close()
    d = pc.STATUS_CASES["e_mask_i16"]
    handle, _ = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
    h = pc.Handle(d)
    bufs = [torch.zeros(pc.layout_size(h.layout(t)[1])[0], dtype=torch.uint8, device="cuda") for t in pc.BINDABLE]
    tensors = [xs.pool_bind_new(handle, t, b) for t, b in zip(pc.BINDABLE, bufs)]
    assert pc.ERR_UNSUPPORTED_DATATYPE == xs.pool_execute(handle, pc.FWD) == xs.pool_execute(handle, pc.BWD)
    for t in tensors:
        layer.L.libxsmm_dnn_destroy_tensor(t)
    layer.L.libxsmm_dnn_destroy_pooling(handle)


def test_pageable_tensors_complete_on_return(xs, torch_gpu):
    L = xs.lib()
    for name in ("a_max_f32_n", "a_avg_bf16_n"):
        d = pc.COMPUTE_CASES[name]
        h, want = pc.Handle(d), case_data(name)
        handle, _ = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
        host = {pc.REG_IN: want["x"].copy(), pc.GRAD_OUT: want["dout"].copy(), pc.REG_OUT: np.full_like(want["out"], 0), pc.GRAD_IN: np.full_like(want["din"], 0)}
        for t in (pc.REG_OUT, pc.GRAD_IN):
            host[t].view(np.uint8)[...] = 0xff
        if d["pooling_type"] == pc.MAX:
            host[pc.MASK] = np.full(h.mask_shape(), pc.SENTINEL, dtype=np.int32)
        tensors = [xs.pool_bind_new(handle, t, a) for t, a in host.items()]
        assert 0 == xs.pool_execute(handle, pc.FWD)
        assert host[pc.REG_OUT].tobytes() == want["out"].tobytes()          # no wait in between
        if pc.MASK in host:
            assert host[pc.MASK].tobytes() == want["mask"].tobytes()
        assert 0 == xs.pool_execute(handle, pc.BWD)
        assert host[pc.GRAD_IN].tobytes() == want["din"].tobytes()
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_pooling(handle)


def test_mixed_residency_complete_on_return(xs, torch_gpu):
    """only what a pass writes in pageable host memory and what it reads on the device, then the reverse: the one staging block
    skips the device-resident operands and still places the others"""
    L = xs.lib()
    for name in ("a_max_f32_n", "a_avg_bf16_n"):
        d = pc.COMPUTE_CASES[name]
        h, want = pc.Handle(d), case_data(name)
        ones = {k: np.full_like(want[k], 0) for k in ("out", "din")}
        for a in ones.values():
            a.view(np.uint8)[...] = 0xff
        fwd = {pc.REG_IN: (want["x"], want["x"], False), pc.REG_OUT: (ones["out"], want["out"], True)}
        bwd = {pc.GRAD_OUT: (want["dout"], want["dout"], False), pc.GRAD_IN: (ones["din"], want["din"], True)}
        if d["pooling_type"] == pc.MAX:
            fwd[pc.MASK] = (np.full(h.mask_shape(), pc.SENTINEL, dtype=np.int32), want["mask"], True)
            bwd[pc.MASK] = (want["mask"], want["mask"], False)
        for kind, roles in ((pc.FWD, fwd), (pc.BWD, bwd)):
            for host_written in (True, False):
                handle, _ = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
                tensors = pc.check_mixed_residency(torch_gpu, roles, host_written, lambda t, m: xs.pool_bind_new(handle, t, m),
                                                   lambda: xs.pool_execute(handle, kind))
                for t in tensors:
                    L.libxsmm_dnn_destroy_tensor(t)
                L.libxsmm_dnn_destroy_pooling(handle)
