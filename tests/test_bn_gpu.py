"""The fused batch-norm layer on the GPU (include/libxsmm_dnn_fusedbatchnorm.h, kernels/bn.hip): FWD and BWD, the eight fuse
combinations, fp32 and bf16, bit for bit against the numpy restatement of tests/bn_common.py (which tests/test_bn_cpu.py holds
against the reference's captured outputs). Destinations are pre-filled with ones bits (NaN / 0xffff); every tensor lies between
canary bands, and its physical padding and the pixels the stride skips hold the same fill, so whatever must not be written shows:
all thirteen tensors are compared whole after every pass."""
import ctypes as C
import threading

import numpy as np
import pytest

import bn_common as bc

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a tensor (a multiple of 16 bytes in every element type)
CANARY = {np.dtype(np.float32): np.float32(-7.25e11), np.dtype(np.uint16): np.uint16(0x7b7b)}
_expect = {}
# the threads cases: six items in three shares of two, whose channel blocks are (0, 1), (2, 0) -- a run that wraps -- and (1, 2)
THREAD_CASES = {"threads_f32_n": bc.desc(5, 3, C=48, ops=13, threads=3), "threads_bf16_n": bc.desc(5, 3, C=48, ops=9, dt=bc.BF16, threads=3)}


def case_data(name, cases=bc.COMPUTE_CASES, bwd=True):
    """the tensors of a case after FWD and BWD (bn_common.expected), computed once and left unchanged"""
    if name not in _expect:
        _expect[name] = bc.expected(name, cases[name], bwd=bwd)
    return _expect[name]


class Layer:
    """a handle with its thirteen tensors on the device: inputs filled, destinations ones bits, all between canaries"""

    def __init__(self, xs, torch, d, want, host=False):
        self.xs, self.torch, self.L, self.want, self.d = xs, torch, xs.lib(), want, d
        self.h = bc.Handle(d)
        self.handle, st = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
        assert self.handle and 0 == st
        seeded = bc.inputs_of(want, d)
        self.buf, self.view, self.tensor = {}, {}, {}
        for key, t in bc.KEYS.items():
            dt = np.dtype(np.float32) if key not in ("x", "add", "dout", "out", "din", "dadd") else np.dtype(bc.elem_dtype(self.h))
            n = int(np.prod(self.h.shape(key)))
            full = np.full(n + 2 * BAND, CANARY[dt], dtype=dt)
            if key in seeded:
                full[BAND:BAND + n] = seeded[key].reshape(-1)
            else:
                full[BAND:BAND + n].view(np.uint8)[...] = 0xff
            if host:  # pageable host memory
                self.buf[key] = full
            else:     # (torch has no uint16 arithmetic: the bytes travel as int16)
                self.buf[key] = torch.from_numpy(full.view(np.int16) if dt == np.uint16 else full).cuda()
            self.view[key] = self.buf[key][BAND:BAND + n]
            self.tensor[key] = xs.bn_bind_new(self.handle, t, self.view[key])

    def result(self, key):
        if isinstance(self.buf[key], np.ndarray):
            full = self.buf[key]
        else:
            self.torch.cuda.synchronize()
            full = self.buf[key].cpu().numpy()
            if full.dtype == np.int16:
                full = full.view(np.uint16)
        canary = CANARY[full.dtype]
        assert np.all(full[:BAND] == canary) and np.all(full[-BAND:] == canary), "a canary band was overwritten: " + key
        return full[BAND:-BAND]

    def check(self, keys, want=None):
        want = self.want if want is None else want
        for key in keys:
            got, ref = self.result(key), want[key].reshape(-1)
            assert got.tobytes() == ref.tobytes(), "%s differs in %d of %d bytes" % (key, int(np.sum(got.view(np.uint8) != ref.view(np.uint8))), ref.nbytes)

    def run(self, kind, start=0, tid=0):
        return self.xs.bn_execute(self.handle, kind, start, tid)

    def close(self):
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_fusedbatchnorm(self.handle)


def after_fwd(want):
    """the state between the passes: what FWD wrote, and doutput / the BWD destinations as they were"""
    t = dict(want)
    t["dout"] = want["dout_in"]
    for key in ("din", "dadd") + (("dgamma", "dbeta") if "dgamma" not in bc.inputs_of(want, None) else ()):
        t[key] = bc.filled(want[key].shape, want[key].dtype)
    return t


ALL_KEYS = tuple(bc.KEYS)


@pytest.mark.parametrize("name", sorted(bc.COMPUTE_CASES))
def test_fwd_and_bwd_bit_equal(xs, torch_gpu, name):
    d = bc.COMPUTE_CASES[name]
    want = case_data(name)
    layer = Layer(xs, torch_gpu, d, want)
    stats = bool(d["fuse_ops"] & bc.OPS_BN)
    dname = "f32" if layer.h.f32 else "bf16"
    launches = layer.L.libxsmm_amd_launch_count()
    assert 0 == layer.run(bc.FWD)                       # no scratch is bound: execute_st does not ask for it
    assert (3 if stats else 1) == layer.L.libxsmm_amd_launch_count() - launches, "partial sums, finish and apply; BNSCALE: apply alone"
    assert xs.last_kernel() == "bn_fwd_apply_" + dname
    layer.check(ALL_KEYS, after_fwd(want))              # padding, skipped pixels and every tensor FWD does not write keep their bytes
    launches = layer.L.libxsmm_amd_launch_count()
    assert 0 == layer.run(bc.BWD)
    assert (3 if stats else 1) == layer.L.libxsmm_amd_launch_count() - launches
    assert xs.last_kernel() == "bn_bwd_apply_" + dname
    layer.check(ALL_KEYS)
    layer.close()


@pytest.mark.parametrize("name", sorted(bc.SPECIAL_CASES))
def test_nan_and_inf_stay_in_their_channel(xs, torch_gpu, name):
    """FWD only: a NaN in lane 2 and an Inf in lane 7 of block 0 -- mean, rstd, var and every output of those two channels are
    what the reference's arithmetic makes of them, and the other lanes of the same pixels are untouched"""
    d = bc.SPECIAL_CASES[name]
    want = case_data(name, bc.SPECIAL_CASES, bwd=False)
    layer = Layer(xs, torch_gpu, d, want)
    assert 0 == layer.run(bc.FWD)
    layer.check(ALL_KEYS)
    out = bc.as_f32(layer.h, layer.result("out").reshape(layer.h.out_shape()))
    assert np.all(np.isfinite(np.delete(out, [2, 7], axis=3))) and np.all(np.isnan(out[..., 2]))
    layer.close()


@pytest.mark.parametrize("name", sorted(THREAD_CASES))
def test_threads_in_reverse_order_give_the_bits_of_one(xs, torch_gpu, name):
    d = THREAD_CASES[name]
    want = case_data(name, THREAD_CASES)
    assert want["out"].tobytes() == bc.expected(name, dict(d, threads=1))["out"].tobytes()  # (the restatement knows no threads)
    for start in (0, 4):
        layer = Layer(xs, torch_gpu, d, want)
        assert [layer.h.share(t) for t in range(4)] == [(0, 2), (2, 4), (4, 6), (6, 6)]
        for kind in (bc.FWD, bc.BWD):
            launches = layer.L.libxsmm_amd_launch_count()
            assert 0 == layer.run(kind, start, start + 3) == layer.run(kind, start, start + 40)      # logical threads beyond desc.threads
            assert 0 == layer.L.libxsmm_amd_launch_count() - launches
            assert bc.ERR_GENERAL == layer.run(kind, start + 1, start)                               # logical thread -1
            if kind == bc.FWD:  # one share computes the whole statistics of its blocks (2 and 0) and writes its own items only
                assert 0 == layer.run(kind, start, start + 1)
                assert 3 == layer.L.libxsmm_amd_launch_count() - launches
                got = layer.result("out").reshape(layer.h.out_shape())
                assert got[2:4].tobytes() == want["out"][2:4].tobytes() and np.all(np.delete(got, [2, 3], axis=0).view(np.uint8) == 0xff)
                mean = layer.result("mean").reshape(3, 16)
                assert mean[[0, 2]].tobytes() == want["mean"][[0, 2]].tobytes() and np.all(mean[1].view(np.uint32) == 0xffffffff)
            for tid in (2, 1, 0):
                assert 0 == layer.run(kind, start, start + tid)
            layer.check(ALL_KEYS, after_fwd(want) if kind == bc.FWD else want)
        layer.close()


def test_shares_from_three_threads_with_own_streams(xs, torch_gpu):
    """a pass is complete before the next begins (BWD reads the outputs of all images of a channel block), as in the reference"""
    torch = torch_gpu
    name = "threads_f32_n"
    layer = Layer(xs, torch, THREAD_CASES[name], case_data(name, THREAD_CASES))
    torch.cuda.synchronize()
    status = [None] * 3
    between = threading.Barrier(3)

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        fwd = layer.run(bc.FWD, 0, tid)
        s.synchronize()
        between.wait()
        status[tid] = [fwd, layer.run(bc.BWD, 0, tid)]
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    workers = [threading.Thread(target=share, args=(tid,)) for tid in range(3)]
    for wk in workers:
        wk.start()
    for wk in workers:
        wk.join()
    assert status == [[0, 0]] * 3
    layer.check(ALL_KEYS)
    layer.close()


def test_statuses_in_check_order(xs, torch_gpu):
    """every row of execute_st's check order on one bound layer, then what this engine refuses on its own"""
    torch = torch_gpu
    L = xs.lib()
    name = "fuse13_f32_n"
    base = bc.COMPUTE_CASES[name]
    want = case_data(name)
    assert bc.ERR_INVALID_HANDLE == xs.bn_execute(None, bc.FWD)
    for change, status in ((dict(), None), (dict(buffer_format=bc.FMT_LIBXSMM | bc.FMT_NHWC), bc.ERR_INVALID_FORMAT_FUSEDBN),
                           (dict(fuse_order=1), bc.ERR_FUSEBN_UNSUPPORTED_ORDER), (dict(fuse_ops=15), bc.ERR_FUSEBN_UNSUPPORTED_FUSION),
                           (dict(fuse_ops=12), bc.ERR_FUSEBN_UNSUPPORTED_FUSION)):
        layer = Layer(xs, torch, dict(base, **change), want)
        for kind in (bc.UPD, bc.BWDUPD, bc.ALL, 7):
            assert bc.ERR_INVALID_KIND == layer.run(kind)
        if status is not None:
            assert status == layer.run(bc.FWD) == layer.run(bc.BWD)
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_release_tensor(layer.handle, bc.REG_GAMMA)     # an unbound tensor comes before order and fusion
            assert (status if change.get("buffer_format") else bc.ERR_DATA_NOT_BOUND) == layer.run(bc.FWD) == layer.run(bc.BWD)
        else:
            for t, kinds in ((bc.REG_ADD, (bc.FWD,)), (bc.GRAD_ADD, (bc.BWD,)), (bc.VAR, (bc.FWD,)), (bc.REG_OUT, (bc.FWD, bc.BWD)), (bc.GRAD_BETA, (bc.BWD,)),
                             (bc.MEAN, (bc.FWD, bc.BWD))):
                tensor = L.libxsmm_dnn_fusedbatchnorm_get_tensor(layer.handle, t, C.byref(C.c_uint()))
                assert 0 == L.libxsmm_dnn_fusedbatchnorm_release_tensor(layer.handle, t)
                for kind in (bc.FWD, bc.BWD):
                    if kind in kinds:
                        assert bc.ERR_DATA_NOT_BOUND == layer.run(kind), (t, kind)
                assert 0 == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(layer.handle, tensor, t)
            assert bc.ERR_GENERAL == layer.run(bc.FWD, 1, 0) == layer.run(bc.BWD, 5, 4)
            # a device tensor that is not 16-byte aligned (the same layout, four bytes further)
            n = int(np.prod(layer.h.in_shape()))
            shifted = xs.bn_bind_new(layer.handle, bc.REG_IN, layer.buf["x"][BAND + 1:BAND + 1 + n])
            assert bc.ERR_GENERAL == layer.run(bc.FWD) == layer.run(bc.BWD)
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(layer.handle, layer.tensor["x"], bc.REG_IN)
            L.libxsmm_dnn_destroy_tensor(shifted)
            # the scratch: bound or not, device or host memory, never written
            size = L.libxsmm_dnn_fusedbatchnorm_get_scratch_size(layer.handle, C.byref(C.c_uint()))
            assert size == layer.h.scratch()
            scratch = torch.full((size,), 0x5a, dtype=torch.uint8, device="cuda")
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_bind_scratch(layer.handle, xs.dptr(scratch))
            assert 0 == layer.run(bc.FWD) == layer.run(bc.BWD)
            host_scratch = np.full(size, 0x5a, dtype=np.uint8)
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_bind_scratch(layer.handle, xs.dptr(host_scratch))
            assert 0 == layer.run(bc.FWD) == layer.run(bc.BWD)                                         # (BWD twice: the RELU select is idempotent)
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_release_scratch(layer.handle)
            layer.check(ALL_KEYS)
            assert np.all(scratch.cpu().numpy() == 0x5a) and np.all(host_scratch == 0x5a), "the scratch is never written"
        layer.check(["out", "din", "mean", "dgamma"], None if status is None else after_fwd_nothing(want))
        layer.close()
    # H % u != 0, W % v != 0: refused (the reference would walk past its tensors; never captured)
    for change in (dict(u=2), dict(v=2), dict(H=5, W=3, u=5, v=2)):
        d = dict(base, **change)
        handle, st = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
        h = bc.Handle(d)
        assert handle and 0 == st and bc.ERR_GENERAL == h.execute_status(bc.FWD, bc.BINDABLE)
        bufs = [torch.zeros(bc.layout_size(h.layout(t)[1])[0] + 64, dtype=torch.uint8, device="cuda") for t in bc.BINDABLE]
        tensors = [xs.bn_bind_new(handle, t, b) for t, b in zip(bc.BINDABLE, bufs)]
        assert bc.ERR_GENERAL == xs.bn_execute(handle, bc.FWD) == xs.bn_execute(handle, bc.BWD)
        torch.cuda.synchronize()
        assert all(int(b.sum()) == 0 for b in bufs)
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_fusedbatchnorm(handle)


def after_fwd_nothing(want):
    """nothing ran: the destinations hold their fill"""
    return {k: bc.filled(want[k].shape, want[k].dtype) for k in ("out", "din", "mean", "dgamma")}


@pytest.mark.parametrize("name", ("pad_f32_n", "fuse13_bf16_n", "stride_scale_f32_n"))
def test_pageable_tensors_complete_on_return(xs, torch_gpu, name):
    """all thirteen tensors in pageable host memory: staged, and what a pass writes is back when the call returns"""
    d = bc.COMPUTE_CASES[name]
    want = case_data(name)
    layer = Layer(xs, torch_gpu, d, want, host=True)
    assert 0 == layer.run(bc.FWD)
    layer.check(ALL_KEYS, after_fwd(want))          # no wait in between
    assert 0 == layer.run(bc.BWD)
    layer.check(ALL_KEYS)
    layer.close()


@pytest.mark.parametrize("name", ("pad_f32_n", "fuse13_bf16_n"))
def test_mixed_residency_complete_on_return(xs, torch_gpu, name):
    """only what a pass writes in pageable host memory and what it reads on the device, then the reverse: the one staging block
    skips the device-resident operands and still places the others"""
    L = xs.lib()
    d = bc.COMPUTE_CASES[name]
    h, want = bc.Handle(d), case_data(name)
    key_of = {t: key for key, t in bc.KEYS.items()}
    between = after_fwd(want)
    start = dict(between, **{key: bc.filled(want[key].shape, want[key].dtype) for key in bc.written(d, bc.FWD)})
    for kind, before, after in ((bc.FWD, start, between), (bc.BWD, between, want)):
        roles = {key_of[t]: (before[key_of[t]], after[key_of[t]], key_of[t] in bc.written(d, kind)) for t in h.needed(kind)}
        for host_written in (True, False):
            handle, _ = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
            tensors = bc.check_mixed_residency(torch_gpu, roles, host_written, lambda key, m: xs.bn_bind_new(handle, bc.KEYS[key], m),
                                               lambda: xs.bn_execute(handle, kind))
            for t in tensors:
                L.libxsmm_dnn_destroy_tensor(t)
            assert 0 == L.libxsmm_dnn_destroy_fusedbatchnorm(handle)
