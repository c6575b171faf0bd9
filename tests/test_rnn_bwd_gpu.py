"""The backward and update passes of the RNN cell layer on the GPU (include/libxsmm_dnn_rnncell.h, kernels/rnn_bwd.hip): BWD, UPD and
BWDUPD of the simple cells and the LSTM, bit for bit against the restatement of tests/rnn_bwd_common.py (which
tests/test_rnn_bwd_cpu.py holds against the reference's captured outputs, and whose transcendentals it shows to lie far from every
float rounding boundary: no tolerance is needed here). Every comparison is uint32 equality through the C-ABI. Gradient destinations
are pre-filled with ones bits; every tensor lies between canary bands; the inputs, the forward pass's tensors, the scratch, the steps
beyond the sequence length and the tensors a kind does not write are compared too."""
import ctypes as C
import threading

import numpy as np
import pytest

import rnn_common as rc
import rnn_bwd_common as rb

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a tensor
CANARY = np.float32(-7.25e11)
TYPE_OF = dict(rc.IN_TYPE, **rc.OUT_TYPE, **rb.GRAD_TYPE)


class Layer:
    """a handle with every tensor a backward pass reads (filled) and every gradient tensor (ones bits; a simple cell's dcs too, which
    no pass of it touches), all between canaries; the scratch is pageable host memory (it is never dereferenced)"""

    def __init__(self, xs, torch, d, t, host=False):
        self.xs, self.torch, self.L, self.d = xs, torch, xs.lib(), d
        self.h = rc.Handle(d)
        self.handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], d["threads"])
        assert self.handle and st == self.h.status
        if d["seq"] >= 0:
            assert 0 == self.L.libxsmm_dnn_rnncell_set_sequence_length(self.handle, d["seq"])
        self.buf, self.view, self.tensor = {}, {}, {}
        self.keys = rb.read(d["cell"]) + (() if d["cell"] == rc.LSTM else ("dcs",)) + rb.GRADS
        for key in self.keys:
            shape = rb.grad_shape(self.h, key) if key in rb.GRADS else self.h.shape(key)
            n = int(np.prod(shape))
            full = np.full(n + 2 * BAND + 16, CANARY, dtype=np.float32)
            full = full[(-full.ctypes.data % 64) // 4:][:n + 2 * BAND]
            if key in t:
                full[BAND:BAND + n] = t[key].reshape(-1)
            else:
                full[BAND:BAND + n].view(np.uint8)[...] = 0xff
            self.buf[key] = full if host else torch.from_numpy(full).cuda()
            self.view[key] = self.buf[key][BAND:BAND + n]
            if key == "z":
                assert 0 == self.L.libxsmm_dnn_rnncell_bind_internalstate(self.handle, rc.BWDUPD, xs.dptr(self.view[key]))
            else:
                self.tensor[key] = xs.rnn_bind_new(self.handle, TYPE_OF[key], self.view[key])
        size = self.L.libxsmm_dnn_rnncell_get_scratch_size(self.handle, rc.BWDUPD, C.byref(C.c_uint()))
        assert size == self.h.scratch_size(rc.BWDUPD)[0]
        self.scratch = np.full(size + 64, 0x5a, dtype=np.uint8)
        assert 0 == self.L.libxsmm_dnn_rnncell_bind_scratch(self.handle, rc.BWDUPD, xs.dptr(self.scratch))

    def result(self, key):
        if isinstance(self.buf[key], np.ndarray):
            full = self.buf[key]
        else:
            self.torch.cuda.synchronize()
            full = self.buf[key].cpu().numpy()
        assert np.all(full[:BAND] == CANARY) and np.all(full[-BAND:] == CANARY), "a canary band was overwritten: " + key
        return full[BAND:-BAND]

    def check(self, t, out, kind, nan_class=False):
        """every tensor: what the kind writes, and everything else as it was (the gradient tensors of other kinds: ones bits)"""
        wr = rb.written(self.d["cell"], kind) if kind is not None else ()
        for key in self.keys:
            got = self.result(key)
            if key in wr:
                want = out[key].reshape(-1)
            elif key in t:
                want = t[key].reshape(-1)
            else:
                assert np.all(got.view(np.uint32) == 0xffffffff), key + " is not written by this kind"
                continue
            bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
            assert rc.same_bits(got, want, nan_class and key in wr), "%s differs in %d of %d elements" % (key, bad, want.size)
        assert np.all(self.scratch == 0x5a), "the scratch is never written"

    def refill(self):
        for key in rb.GRADS:
            self.view[key].view(self.torch.uint8 if not isinstance(self.view[key], np.ndarray) else np.uint8)[...] = 0xff

    def run(self, kind, start=0, tid=0):
        return self.xs.rnn_execute(self.handle, kind, start, tid)

    def count(self):
        return self.L.libxsmm_amd_launch_count()

    def close(self):
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_rnncell(self.handle)


@pytest.mark.parametrize("name", sorted(rb.COMPUTE_CASES) + sorted(rb.UNCAPTURED_CASES))
def test_all_three_kinds_bit_equal(xs, torch_gpu, name):
    """every captured compute case (and t1_tanh, which the reference cannot run), BWD, UPD and BWDUPD on one handle: all tensors, and
    the launch count, a function of the sequence length and the kind alone"""
    d = rb.all_cases()[name]
    layer = Layer(xs, torch_gpu, d, rb.cached_inputs(name))
    for kind in rb.KINDS:
        t, out = rb.expected(name, kind)
        layer.refill()
        before = layer.count()
        assert 0 == layer.run(kind)
        assert rb.launches(d["cell"], kind, layer.h.T) == layer.count() - before, rb.KIND_NAMES[kind]
        assert xs.last_kernel().startswith("rnn_bwd_")
        layer.check(t, out, kind)
        if "dx" in rb.written(d["cell"], kind):
            dx = layer.result("dx").reshape(d["max_T"], -1)
            assert np.all(dx[layer.h.T:].view(np.uint32) == 0xffffffff) and not np.any(dx[:layer.h.T].view(np.uint32) == 0xffffffff)
    layer.close()


def test_launch_counts_do_not_depend_on_the_shape():
    for cell in rb.CELLS:
        lstm = 1 if cell == rc.LSTM else 0
        assert [rb.launches(cell, kind, 3) for kind in rb.KINDS] == [3 + lstm + 1, 3 + lstm + 3, 3 + lstm + 4]
        assert rb.launches(cell, rb.BWD, 65537) == 65537 + lstm + 2
    # (the GPU tests assert the same numbers on N, C, K from 4, 12, 16 up to 130, 40, 2064)


@pytest.mark.parametrize("name", sorted(rb.SPECIAL_CASES))
def test_special_values(xs, torch_gpu, name):
    """a NaN and an Inf planted in dh and in z (simple cells) or o (LSTM); NaNs are compared as a class (their sign differs by machine)"""
    d = rb.SPECIAL_CASES[name]
    layer = Layer(xs, torch_gpu, d, rb.cached_inputs(name))
    for kind in rb.KINDS:
        t, out = rb.expected(name, kind)
        layer.refill()
        assert 0 == layer.run(kind)
        layer.check(t, out, kind, nan_class=True)
    # after BWDUPD
    dx, dw = layer.result("dx").reshape(d["max_T"], d["N"], d["C"]), layer.result("dw").reshape(d["C"], -1)
    assert np.any(np.isnan(dx)) and np.any(np.isnan(dw))
    if name == "special_rows_lstm":  # beyond the first tile both ways, all planted at step 0
        p, K = rb.PLANTED_ROWS, d["K"]
        rows, cols = sorted(v[1] for v in p.values()), sorted(q * K + v[2] for v in p.values() for q in range(4))
        assert np.all(np.isnan(dx[0, p["dh_nan"][1]])) and np.all(np.isnan(dw[:, [q * K + p["dh_nan"][2] for q in range(4)]]))
        clean = np.ones(d["N"], dtype=bool)
        clean[rows] = False
        assert np.all(np.isfinite(dx[:, clean])) and np.all(np.isfinite(dx[1]))     # the poison stays in its rows of step 0
        assert np.all(np.isfinite(layer.result("dhp").reshape(d["max_T"], d["N"], K)[0, clean]))
        clean = np.ones(4 * K, dtype=bool)
        clean[cols] = False
        assert np.all(np.isfinite(dw[:, clean])) and np.all(np.isfinite(layer.result("dr").reshape(K, -1)[:, clean]))  # and in its columns
        assert np.all(np.isfinite(layer.result("db")[clean]))
    layer.close()


def on_a_stream_of_its_own(torch, layer, kind, tid, status):
    def share():
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = layer.run(kind, 0, tid)
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)
    wk = threading.Thread(target=share)
    wk.start()
    wk.join()


@pytest.mark.parametrize("name", sorted(rb.THREAD_CASES))
def test_threads(xs, torch_gpu, name):
    """N = 260, threads = 3: rows [0, 91), [91, 182), [182, 260). BWD: the shares issued in reverse order on streams of their own give
    the bits of threads = 1, and after each share only its rows of dx are written anew. UPD and BWDUPD: logical threads 1 and 2 launch
    nothing, thread 0 alone completes everything."""
    torch = torch_gpu
    d = rb.THREAD_CASES[name]
    layer = Layer(xs, torch, d, rb.cached_inputs(name))
    assert layer.h.shares() == [(0, 91), (91, 182), (182, 260)]
    t, out = rb.expected(name, rb.BWD)
    before = layer.count()
    assert 0 == layer.run(rb.BWD, 0, 3) == layer.run(rb.BWD, 5, 45)
    assert 0 == layer.count() - before
    assert rc.ERR_GENERAL == layer.run(rb.BWD, 1, 0)
    torch.cuda.synchronize()
    status = {}
    for tid in (2, 1, 0):
        on_a_stream_of_its_own(torch, layer, rb.BWD, tid, status)
        n0 = layer.h.shares()[tid][0]
        got = layer.result("dx").reshape(d["max_T"], d["N"], d["C"])
        assert got[:, n0:].tobytes() == out["dx"][:, n0:].tobytes() and np.all(got[:, :n0].view(np.uint32) == 0xffffffff), tid
    assert status == {0: 0, 1: 0, 2: 0}
    layer.check(t, out, rb.BWD)
    for kind in (rb.UPD, rb.BWDUPD):
        t, out = rb.expected(name, kind)
        layer.refill()
        status = {}
        before = layer.count()
        for tid in (2, 1):
            on_a_stream_of_its_own(torch, layer, kind, tid, status)
        assert 0 == layer.count() - before
        layer.check(t, out, None)  # nothing written yet
        on_a_stream_of_its_own(torch, layer, kind, 0, status)
        assert status == {0: 0, 1: 0, 2: 0} and rb.launches(d["cell"], kind, layer.h.T) == layer.count() - before
        layer.check(t, out, kind)
    layer.close()


@pytest.mark.parametrize("name", ("one_lstm", "one_sigmoid"))
def test_pageable_tensors_complete_on_return(xs, torch_gpu, name):
    d = rb.COMPUTE_CASES[name]
    t, out = rb.expected(name, rb.BWDUPD)
    layer = Layer(xs, torch_gpu, d, t, host=True)
    assert 0 == layer.run(rb.BWDUPD)
    layer.check(t, out, rb.BWDUPD)  # no wait in between
    layer.close()


@pytest.mark.parametrize("name", ("one_lstm", "one_tanh"))
def test_mixed_residency_complete_on_return(xs, torch_gpu, name):
    """only what the pass writes in pageable host memory and what it reads on the device, then the reverse"""
    L = xs.lib()
    d = rb.COMPUTE_CASES[name]
    t, out = rb.expected(name, rb.BWDUPD)
    h = rc.Handle(d)
    roles = {key: (t[key], t[key], False) for key in rb.read(d["cell"]) if key != "z"}
    roles.update({key: (rc.filled(rb.grad_shape(h, key)), out[key], True) for key in rb.written(d["cell"], rb.BWDUPD)})
    for host_written in (True, False):
        handle, _ = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], d["threads"])
        assert 0 == L.libxsmm_dnn_rnncell_set_sequence_length(handle, d["seq"])
        z = None
        if h.simple():
            z = torch_gpu.from_numpy(t["z"]).cuda()
            assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, rb.BWDUPD, xs.dptr(z))
        tensors = rc.check_mixed_residency(torch_gpu, roles, host_written, lambda key, m: xs.rnn_bind_new(handle, TYPE_OF[key], m),
                                           lambda: xs.rnn_execute(handle, rb.BWDUPD))
        for tensor in tensors:
            L.libxsmm_dnn_destroy_tensor(tensor)
        assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)


def test_statuses_on_a_bound_layer(xs, torch_gpu):
    """execute_st's check order where a device is there: nothing is launched and nothing written by a refused call"""
    L = xs.lib()
    needs = {rb.BWD: ("r", "dh", "w", "dx"), rb.UPD: ("r", "dh", "x", "hp", "h", "dw", "dr", "db")}
    lstm_needs = ("csp", "cs", "i", "f", "o", "ci", "co", "dcs", "dcsp", "dhp")
    for name in ("one_lstm", "one_tanh"):
        d = rb.COMPUTE_CASES[name]
        layer = Layer(xs, torch_gpu, d, rb.cached_inputs(name))
        before = layer.count()
        for kind in (rc.ALL, 7):
            assert rc.ERR_INVALID_KIND == layer.run(kind)
        for kind in rb.KINDS:
            need = set(needs[rb.BWD] if kind != rb.UPD else ()) | set(needs[rb.UPD] if kind != rb.BWD else ()) | set(lstm_needs if d["cell"] == rc.LSTM else ())
            for key in layer.tensor:
                assert 0 == L.libxsmm_dnn_rnncell_release_tensor(layer.handle, TYPE_OF[key])
                if key in need:
                    assert rc.ERR_DATA_NOT_BOUND == layer.run(kind), (kind, key)
                assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(layer.handle, layer.tensor[key], TYPE_OF[key])
            if layer.h.simple():
                assert 0 == L.libxsmm_dnn_rnncell_release_internalstate(layer.handle, kind)
                assert rc.ERR_DATA_NOT_BOUND == layer.run(kind)
                assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(layer.handle, kind, xs.dptr(layer.view["z"]))
            assert rc.ERR_GENERAL == layer.run(kind, 1, 0)
        for key in rb.GRADS + ("dh", "dcs"):  # no gradient tensor at all: the answer from before these passes existed
            assert 0 == L.libxsmm_dnn_rnncell_release_tensor(layer.handle, TYPE_OF[key])
        for kind in rb.KINDS:
            assert rc.ERR_INVALID_KIND == layer.run(kind)
        for key in rb.GRADS + ("dh", "dcs"):
            assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(layer.handle, layer.tensor[key], TYPE_OF[key])
        assert 0 == layer.count() - before
        t, out = rb.expected(name, rb.BWDUPD)
        layer.check(t, out, None)  # nothing was written
        assert 0 == L.libxsmm_dnn_rnncell_release_scratch(layer.handle, rb.BWDUPD)  # no scratch is needed
        assert 0 == layer.run(rb.BWDUPD)
        layer.check(t, out, rb.BWDUPD)
        layer.close()


# ---- the seeded sweep (rnn_bwd_common.sweep_cases) ---------------------------------------------------------------------------------------
def check_bits(layer, t, out, kind, name):
    """Layer.check, after a look at what the kind writes that says more where bits differ: whether the result is still inside the
    float64 contract's bound (then an order of summation differs; else a formula or an address)"""
    for key in rb.written(layer.d["cell"], kind):
        got, want = layer.result(key), out[key].reshape(-1)
        if rc.same_bits(got, want):
            continue
        one = rc.Handle(dict(layer.d, threads=1))
        one.T = layer.h.T  # (the length the handle has now)
        value, bound = rb.contract64(one, t, kind)[key]
        part = got.reshape(out[key].shape)
        part = part[:layer.h.T] if key == "dx" else (part[0] if key in ("dcsp", "dhp") else part)
        inside = bool(np.all(np.abs(part.astype(np.float64) - value) <= bound))
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        pytest.fail("%s %s: %s differs in %d of %d elements (first at %d: %r for %r); the result is %s the float64 contract's bound"
                    % (name, rb.KIND_NAMES[kind], key, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]], "inside" if inside else "OUTSIDE"))
    layer.check(t, out, kind)


@pytest.mark.parametrize("name", sorted(rb.sweep_cases()))
def test_seeded_sweep(xs, torch_gpu, name):
    """BWD, UPD and BWDUPD of a drawn descriptor on one handle, bit for bit against the restatement of one thread: every tensor, the
    fill of what a kind does not write and of the steps beyond the sequence length, the scratch, the launch count. With threads > 1
    BWD runs share by share in reverse order (a thread without a share launches nothing), UPD and BWDUPD through thread 0 alone."""
    d = rb.sweep_cases()[name]
    layer = Layer(xs, torch_gpu, d, rb.cached_inputs(name))
    T, per = layer.h.T, lambda kind: rb.launches(d["cell"], kind, layer.h.T)  # noqa: E731
    shares = layer.h.shares()
    for kind in rb.KINDS:
        t, out = rb.expected(name, kind)
        layer.refill()
        before = layer.count()
        if kind == rb.BWD:
            for tid in reversed(range(d["threads"])):
                mark = layer.count()
                assert 0 == layer.run(kind, 0, tid)
                assert (per(kind) if shares[tid][1] > shares[tid][0] else 0) == layer.count() - mark, tid
            assert per(kind) * sum(s[1] > s[0] for s in shares) == layer.count() - before
        else:
            for tid in reversed(range(1, d["threads"])):
                assert 0 == layer.run(kind, 0, tid)
            assert 0 == layer.count() - before
            assert 0 == layer.run(kind, 0, 0)
            assert per(kind) == layer.count() - before
        assert xs.last_kernel().startswith("rnn_bwd_")
        check_bits(layer, t, out, kind, name)
        if "dx" in rb.written(d["cell"], kind):
            dx = layer.result("dx").reshape(d["max_T"], -1)
            assert np.all(dx[T:].view(np.uint32) == 0xffffffff) and not np.any(dx[:T].view(np.uint32) == 0xffffffff)
    layer.close()


@pytest.mark.parametrize("name", sorted(rb.SEQ_CASES))
def test_sequence_length_changes_on_one_handle(xs, torch_gpu, name):
    """BWDUPD at the lengths 4, 1 and 3 on one handle, whose delta buffer keeps the deltas of the longer run before: each result is
    the restatement's at that length and a fresh handle's, bit for bit -- dw, dr and db sum the steps below the current length only --
    and dx beyond the current length keeps what the refill put there"""
    d = rb.SEQ_CASES[name]
    t = rb.cached_inputs(name)
    layer = Layer(xs, torch_gpu, d, t)
    for length in rb.SEQ_LENGTHS:
        _, out = rb.expected(name, rb.BWDUPD, True, length)
        assert 0 == layer.L.libxsmm_dnn_rnncell_set_sequence_length(layer.handle, length)
        layer.refill()
        before = layer.count()
        assert 0 == layer.run(rb.BWDUPD)
        assert rb.launches(d["cell"], rb.BWDUPD, length) == layer.count() - before
        layer.h.T = length
        check_bits(layer, t, out, rb.BWDUPD, "%s at %d" % (name, length))
        dx = layer.result("dx").reshape(d["max_T"], -1)
        assert np.all(dx[length:].view(np.uint32) == 0xffffffff) and not np.any(dx[:length].view(np.uint32) == 0xffffffff)
        fresh = Layer(xs, torch_gpu, dict(d, seq=length), t)
        assert 0 == fresh.run(rb.BWDUPD)
        for key in rb.GRADS:
            assert layer.result(key).tobytes() == fresh.result(key).tobytes(), (length, key)
        fresh.close()
    layer.close()


@pytest.mark.parametrize("name", sorted(rb.SEQ_CASES))
def test_forward_then_backward_on_one_handle(xs, torch_gpu, name):
    """FWD on the GPU into zeroed h, gates and z, then BWDUPD on the same handle and tensors (the internal state and the scratch were
    bound for BWDUPD): the forward tensors and the gradients are the restatement's, bit for bit"""
    d = rb.SEQ_CASES[name]
    t, out = rb.expected(name, rb.BWDUPD)
    zeroed = dict(t, **{key: np.zeros_like(t[key]) for key in rc.written(d["cell"])})
    layer = Layer(xs, torch_gpu, d, zeroed)
    layer.check(zeroed, out, None)
    assert 0 == layer.run(rc.FWD)
    assert xs.last_kernel().startswith("rnn_") and not xs.last_kernel().startswith("rnn_bwd_")
    layer.check(t, out, None)  # the forward tensors as the restatement has them; no gradient tensor written yet
    before = layer.count()
    assert 0 == layer.run(rb.BWDUPD)
    assert rb.launches(d["cell"], rb.BWDUPD, layer.h.T) == layer.count() - before
    check_bits(layer, t, out, rb.BWDUPD, name)
    layer.close()
