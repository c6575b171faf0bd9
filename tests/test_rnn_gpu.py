"""The RNN cell layer on the GPU (include/libxsmm_dnn_rnncell.h, kernels/rnn.hip): the forward pass of the five cells, bit for bit
against the restatement of tests/rnn_common.py (which tests/test_rnn_cpu.py holds against the reference's captured outputs, and whose
transcendentals it shows to lie far from every float rounding boundary: no tolerance is needed here). Destinations are pre-filled with
ones bits; every tensor lies between canary bands; inputs, the scratch and the steps beyond the sequence length are compared too."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import launch_limits as ll
import rnn_common as rc

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a tensor
CANARY = np.float32(-7.25e11)
ENV = ("LIBXSMM_AMD_RNN_PLAN",)
THREAD_CASES = rc.THREAD_CASES


def keys_of(d):
    return rc.read(d["cell"]) + rc.written(d["cell"])


def launches_of(d, h, split):
    """one launch per step (GRU: two) and, in the split plan, one ahead of them per 65535 steps"""
    trip = ll.per_trip("rnn_steps")
    return (2 if d["cell"] == rc.GRU else 1) * h.T + ((h.T + trip - 1) // trip if split else 0)


def split_legal(d, h):
    if h.simple() or d["cell"] == rc.LSTM and not (d["C"] == 2048 and d["K"] == 2048):
        return True
    return 1 == rc.blocking_factor(d["C"], d["K"], d["C"] // h.bc, d["K"] // h.bk)


class Layer:
    """a handle with the tensors its FWD reads and writes: inputs filled, destinations ones bits, all between canaries; the scratch is
    pageable host memory (it is never dereferenced), the internal state of a simple cell lies with the tensors"""

    def __init__(self, xs, torch, d, t, host=False):
        self.xs, self.torch, self.L, self.d = xs, torch, xs.lib(), d
        self.h = rc.Handle(d)
        self.handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], d["threads"])
        assert self.handle and st == self.h.status
        if d["seq"] >= 0:
            assert 0 == self.L.libxsmm_dnn_rnncell_set_sequence_length(self.handle, d["seq"])
        if d["forget_bias"] is not None:
            assert 0 == self.L.libxsmm_dnn_rnncell_allocate_forget_bias(self.handle, d["forget_bias"])
        self.buf, self.view, self.tensor = {}, {}, {}
        for key in keys_of(d):
            n = int(np.prod(self.h.shape(key)))
            full = np.full(n + 2 * BAND + 16, CANARY, dtype=np.float32)
            full = full[(-full.ctypes.data % 64) // 4:][:n + 2 * BAND]  # 64-byte aligned: bind_internalstate rounds z up to that
            if key in t:
                full[BAND:BAND + n] = t[key].reshape(-1)
            else:
                full[BAND:BAND + n].view(np.uint8)[...] = 0xff
            self.buf[key] = full if host else torch.from_numpy(full).cuda()
            self.view[key] = self.buf[key][BAND:BAND + n]
            if key == "z":
                assert 0 == self.L.libxsmm_dnn_rnncell_bind_internalstate(self.handle, rc.FWD, xs.dptr(self.view[key]))
            else:
                self.tensor[key] = xs.rnn_bind_new(self.handle, rc.IN_TYPE.get(key, rc.OUT_TYPE.get(key)), self.view[key])
        size = self.L.libxsmm_dnn_rnncell_get_scratch_size(self.handle, rc.FWD, C.byref(C.c_uint()))
        assert size == self.h.scratch_size(rc.FWD)[0]
        self.scratch = np.full(size + 64, 0x5a, dtype=np.uint8)
        assert 0 == self.L.libxsmm_dnn_rnncell_bind_scratch(self.handle, rc.FWD, xs.dptr(self.scratch))

    def result(self, key):
        if isinstance(self.buf[key], np.ndarray):
            full = self.buf[key]
        else:
            self.torch.cuda.synchronize()
            full = self.buf[key].cpu().numpy()
        assert np.all(full[:BAND] == CANARY) and np.all(full[-BAND:] == CANARY), "a canary band was overwritten: " + key
        return full[BAND:-BAND]

    def check(self, t, out, nan_class=False):
        """every tensor of the pass: what it writes, and its inputs and the scratch as they were"""
        for key in keys_of(self.d):
            want = (t[key] if key in t else out[key]).reshape(-1)
            got = self.result(key)
            bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
            assert rc.same_bits(got, want, nan_class and key not in t), "%s differs in %d of %d elements" % (key, bad, want.size)
        assert np.all(self.scratch == 0x5a), "the scratch is never written"

    def run(self, kind=rc.FWD, start=0, tid=0):
        return self.xs.rnn_execute(self.handle, kind, start, tid)

    def count(self):
        return self.L.libxsmm_amd_launch_count()

    def close(self):
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_rnncell(self.handle)


@pytest.fixture(autouse=True)
def clean_env():
    for k in ENV:
        os.environ.pop(k, None)
    yield
    for k in ENV:
        os.environ.pop(k, None)


@pytest.mark.parametrize("name", sorted(rc.GPU_COMPUTE_CASES))
def test_fwd_bit_equal(xs, torch_gpu, name):
    """every captured compute case (and rem_lstm, which the reference cannot run): all tensors of the pass, the default plan and its
    launch count"""
    d = rc.GPU_COMPUTE_CASES[name]
    t, out = rc.expected(name)
    layer = Layer(xs, torch_gpu, d, t)
    before = layer.count()
    assert 0 == layer.run()
    assert launches_of(d, layer.h, split_legal(d, layer.h)) == layer.count() - before
    assert xs.last_kernel().startswith("rnn_g")
    layer.check(t, out)
    layer.close()


@pytest.mark.parametrize("name", sorted(rc.SPECIAL_CASES))
def test_special_values(xs, torch_gpu, name):
    """+-Inf, NaN, +-0 and arguments whose exp overflows and underflows; NaNs are compared as a class (their sign differs by machine)"""
    d = rc.SPECIAL_CASES[name]
    t, out = rc.expected(name)
    for plan in ("split", "whole"):
        os.environ["LIBXSMM_AMD_RNN_PLAN"] = plan
        layer = Layer(xs, torch_gpu, d, t)
        assert 0 == layer.run()
        layer.check(t, out, nan_class=True)
        h = layer.result("h")
        assert np.any(np.isnan(h)) and np.any(np.isfinite(h))
        if name == "special_rows_lstm":  # beyond the first tile both ways: the NaN fills its row of step 0 and no other row has one
            h = h.reshape(d["max_T"], d["N"], d["K"])
            assert np.all(np.isnan(h[0, rc.SPECIAL_ROWS_PLANTED["nan"][0]])) and np.all(np.isfinite(h[:, 3:])[:, np.arange(3, d["N"]) != rc.SPECIAL_ROWS_PLANTED["nan"][0]])
        layer.close()


@pytest.mark.parametrize("name", ["blk_" + n for n in rc.CELL_NAMES.values()] + ["k72_gru", "k72_lstm", "k72_tanh", "seq_gru", "fbias_lstm", "bf_gru"]
                         + ["rows_" + n for n in rc.CELL_NAMES.values()] + ["fused_lstm", "rem_lstm"])
def test_plans_give_the_same_bits(xs, torch_gpu, name):
    d = rc.GPU_COMPUTE_CASES[name]
    t, out = rc.expected(name)
    for plan in ("split", "whole"):
        os.environ["LIBXSMM_AMD_RNN_PLAN"] = plan
        layer = Layer(xs, torch_gpu, d, t)
        before = layer.count()
        assert 0 == layer.run()
        # an illegal force of the split plan is ignored
        assert launches_of(d, layer.h, plan == "split" and split_legal(d, layer.h)) == layer.count() - before, plan
        layer.check(t, out)
        layer.close()


@pytest.mark.parametrize("name", sorted(n for n in THREAD_CASES if n.startswith("threads_")))
def test_threads_in_reverse_order_on_three_streams(xs, torch_gpu, name):
    """threads = 3 on four row blocks: shares of two, two and none, issued in reverse order on streams of their own, give the bits of
    threads = 1; a logical thread beyond desc.threads launches nothing"""
    torch = torch_gpu
    d = THREAD_CASES[name]
    t = rc.inputs(name, d)
    out = rc.forward(rc.Handle(dict(d, threads=1)), t)
    layer = Layer(xs, torch, d, t)
    assert layer.h.shares() == [(0, 4), (4, 8), (8, 8)]
    before = layer.count()
    assert 0 == layer.run(rc.FWD, 0, 3) == layer.run(rc.FWD, 0, 2) == layer.run(rc.FWD, 5, 45)
    assert 0 == layer.count() - before
    assert rc.ERR_GENERAL == layer.run(rc.FWD, 1, 0)
    torch.cuda.synchronize()
    status = {}

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = layer.run(rc.FWD, 0, tid)
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    for tid in (2, 1, 0):
        wk = threading.Thread(target=share, args=(tid,))
        wk.start()
        wk.join()
        if tid == 1:  # the rows of the other share hold their fill
            got = layer.result("h").reshape(d["max_T"], d["N"], d["K"])
            assert got[:, 4:].tobytes() == out["h"][:, 4:].tobytes() and np.all(got[:, :4].view(np.uint32) == 0xffffffff)
    assert status == {0: 0, 1: 0, 2: 0}
    layer.check(t, out)
    layer.close()


@pytest.mark.parametrize("name", sorted(n for n in THREAD_CASES if n.startswith("rowshares_")))
def test_row_shares_across_tiles_in_reverse_order(xs, torch_gpu, name):
    """threads = 3 on twenty row blocks of 13: rows [0, 91), [91, 182) and [182, 260), every share across a tile boundary and two of
    them from the middle of a tile, issued in reverse order on streams of their own, give the bits of threads = 1; after each share
    (the middle one too) only its rows are written anew and all rows not yet issued hold their fill"""
    torch = torch_gpu
    d = THREAD_CASES[name]
    t = rc.inputs(name, d)
    out = rc.forward(rc.Handle(dict(d, threads=1)), t)
    layer = Layer(xs, torch, d, t)
    assert layer.h.shares() == [(0, 91), (91, 182), (182, 260)]
    before = layer.count()
    assert 0 == layer.run(rc.FWD, 0, 3) == layer.run(rc.FWD, 5, 45)
    assert 0 == layer.count() - before
    torch.cuda.synchronize()
    status = {}

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = layer.run(rc.FWD, 0, tid)
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    for tid in (2, 1, 0):
        wk = threading.Thread(target=share, args=(tid,))
        wk.start()
        wk.join()
        n0 = layer.h.shares()[tid][0]  # after every share: its rows and those of the shares before it are written, all others hold the fill
        for key in rc.written(d["cell"]):
            got = layer.result(key).reshape(d["max_T"], d["N"], d["K"])
            assert got[:, n0:].tobytes() == out[key][:, n0:].tobytes() and np.all(got[:, :n0].view(np.uint32) == 0xffffffff), (key, tid)
    assert status == {0: 0, 1: 0, 2: 0}
    layer.check(t, out)
    layer.close()


@pytest.mark.parametrize("name", ("blk_lstm", "seq_gru", "k72_tanh"))
def test_pageable_tensors_complete_on_return(xs, torch_gpu, name):
    d = rc.COMPUTE_CASES[name]
    t, out = rc.expected(name)
    layer = Layer(xs, torch_gpu, d, t, host=True)
    assert 0 == layer.run()
    layer.check(t, out)  # no wait in between
    layer.close()


@pytest.mark.parametrize("name", ("blk_lstm", "blk_gru"))
def test_mixed_residency_complete_on_return(xs, torch_gpu, name):
    """only what the pass writes in pageable host memory and what it reads on the device, then the reverse"""
    L = xs.lib()
    d = rc.COMPUTE_CASES[name]
    t, out = rc.expected(name)
    roles = {key: (t[key], t[key], False) for key in rc.read(d["cell"])}
    roles.update({key: (rc.filled(out[key].shape), out[key], True) for key in rc.written(d["cell"])})
    for host_written in (True, False):
        handle, _ = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], d["threads"])
        tensors = rc.check_mixed_residency(torch_gpu, roles, host_written,
                                           lambda key, m: xs.rnn_bind_new(handle, rc.IN_TYPE.get(key, rc.OUT_TYPE.get(key)), m),
                                           lambda: xs.rnn_execute(handle, rc.FWD))
        for tensor in tensors:
            L.libxsmm_dnn_destroy_tensor(tensor)
        assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)


def test_statuses_on_a_bound_layer(xs, torch_gpu):
    """execute_st's check order where a device is there: nothing is launched and nothing written by a refused call"""
    L = xs.lib()
    for name in ("blk_lstm", "blk_gru", "blk_tanh"):
        d = rc.COMPUTE_CASES[name]
        t, out = rc.expected(name)
        layer = Layer(xs, torch_gpu, d, t)
        before = layer.count()
        for kind in (rc.BWD, rc.UPD, rc.BWDUPD, rc.ALL, 7):
            assert rc.ERR_INVALID_KIND == layer.run(kind)
        for key in rc.read(d["cell"]) + tuple(k for k in rc.written(d["cell"]) if k != "z"):
            ttype = rc.IN_TYPE.get(key, rc.OUT_TYPE.get(key))
            assert 0 == L.libxsmm_dnn_rnncell_release_tensor(layer.handle, ttype)
            assert rc.ERR_DATA_NOT_BOUND == layer.run(), key
            assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(layer.handle, layer.tensor[key], ttype)
        if layer.h.simple():
            assert 0 == L.libxsmm_dnn_rnncell_release_internalstate(layer.handle, rc.FWD)
            assert rc.ERR_DATA_NOT_BOUND == layer.run()
            assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(layer.handle, rc.FWD, xs.dptr(layer.view["z"]))
        assert rc.ERR_GENERAL == layer.run(rc.FWD, 1, 0)
        assert 0 == layer.count() - before
        assert 0 == L.libxsmm_dnn_rnncell_release_scratch(layer.handle, rc.FWD)  # no scratch is needed
        assert 0 == layer.run()
        layer.check(t, out)
        layer.close()


SWEEP = rc.SWEEP


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_seeded_sweep(xs, torch_gpu, name):
    d = SWEEP[name]
    t = rc.inputs(name, d)
    h = rc.Handle(d)
    out = rc.forward(h, t)
    # the restatement itself against float64, within the bound of an fp32 chain of n terms: n * 2^-24 * (sum |a * b| + |bias|), for the
    # pre-activations of step 0 (simple cells: z; LSTM and GRU: the gates are inverted)
    x0, hp0 = t["x"][0].astype(np.float64), t["hp"][0].astype(np.float64)
    w, r, b = t["w"].astype(np.float64), t["r"].astype(np.float64), t["b"].astype(np.float64)
    K = d["K"]
    n = d["C"] + K + 1
    for q, key in enumerate({rc.LSTM: ("i",), rc.GRU: ("i", "ci")}.get(d["cell"], ("z",))):
        pre = x0 @ w[:, q * K:(q + 1) * K] + hp0 @ r[:, q * K:(q + 1) * K] + b[q * K:(q + 1) * K]
        mag = np.abs(x0) @ np.abs(w[:, q * K:(q + 1) * K]) + np.abs(hp0) @ np.abs(r[:, q * K:(q + 1) * K]) + np.abs(b[q * K:(q + 1) * K])
        bound = n * 2.0 ** -24 * mag
        got = out[key][0].astype(np.float64)
        if key != "z":  # sigmoid has slope <= 1/4: the bound on the pre-activation bounds the gate too, plus its own roundings
            pre, bound = 1.0 / (1.0 + np.exp(-pre)), bound / 4 + 3 * 2.0 ** -24
        assert np.all(np.abs(got - pre) <= bound), (key, float(np.max(np.abs(got - pre) - bound)))
    layer = Layer(xs, torch_gpu, d, t)
    assert 0 == layer.run()
    layer.check(t, out)
    layer.close()
