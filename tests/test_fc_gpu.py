"""The fully-connected layer on the GPU (include/libxsmm_dnn_fullyconnected.h, kernels/fc.hip): every pass, both storage
formats and the 16-bit form, bit for bit against the expectation of tests/fc_common.py (the CPU oracle's fma chains).
Destinations are pre-filled with NaN (they are never read) and lie between canary bands that must survive."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import fc_common as fc
import quant_common as qc

pytestmark = pytest.mark.gpu

BAND = 256  # canary elements on either side of a destination
CANARY32, CANARY16 = np.float32(-7.25e11), np.uint16(0x7b7b)
DEST = {fc.FWD: fc.REG_OUT, fc.BWD: fc.GRAD_IN, fc.UPD: fc.GRAD_FIL}
_expect = {}


def case_data(name):
    """(handle restatement, plain inputs, the six tensors' expected contents), computed once per case"""
    if name not in _expect:
        d = fc.COMPUTE_CASES[name]
        h = fc.Handle(d)
        x, w, dy = fc.plain_inputs(name, d)
        _expect[name] = (h, (x, w, dy), fc.tensors(h, x, w, dy))
    return _expect[name]


class Layer:
    """a handle with six device tensors: inputs filled, destinations NaN between canaries"""

    def __init__(self, xs, torch, name, threads=1, contents=None, sweep=False):
        """sweep: name is a case of fc_common.sweep_cases(), which has its own number of threads"""
        self.xs, self.torch, self.L = xs, torch, xs.lib()
        self.h, _, self.want = fc.sweep_expected(name) if sweep else case_data(name)
        want = self.want if contents is None else contents
        d = fc.sweep_cases()[name] if sweep else dict(fc.COMPUTE_CASES[name], threads=threads)
        threads = d["threads"]
        self.handle, st = xs.fc_create(d["N"], d["C"], d["K"], d["bn"], d["bk"], d["bc"], threads, d["datatype_in"], d["datatype_out"],
                                       d["buffer_format"], d["filter_format"], d["fuse_ops"])
        assert self.handle and st == self.h.status
        self.buf, self.view, self.tensor = {}, {}, {}
        for t in fc.TENSOR_TYPES:
            dt = fc.dtype_of(self.h, t)
            n = want[t].size
            host = np.full(n + 2 * BAND, CANARY16 if dt == np.uint16 else CANARY32, dtype=dt)
            if t in DEST.values():
                host[BAND:BAND + n] = 0xffff if dt == np.uint16 else np.nan
            else:
                host[BAND:BAND + n] = want[t].astype(dt)
            # (torch has no uint16 arithmetic: the bytes travel as int16)
            self.buf[t] = torch.from_numpy(host.view(np.int16) if dt == np.uint16 else host).cuda()
            self.view[t] = self.buf[t][BAND:BAND + n]
            self.tensor[t] = xs.fc_bind_new(self.handle, t, self.view[t])
        size = self.L.libxsmm_dnn_fullyconnected_get_scratch_size(self.handle, C.byref(C.c_uint()))
        assert size == self.h.scratch()
        self.scratch = torch.full((size,), 0x5a, dtype=torch.uint8, device="cuda")
        assert 0 == self.L.libxsmm_dnn_fullyconnected_bind_scratch(self.handle, xs.dptr(self.scratch))

    def result(self, t):
        """the destination's elements; asserts the canaries"""
        self.torch.cuda.synchronize()
        dt = fc.dtype_of(self.h, t)
        host = self.buf[t].cpu().numpy()
        host = host.view(np.uint16) if dt == np.uint16 else host
        canary = CANARY16 if dt == np.uint16 else CANARY32
        assert np.all(host[:BAND] == canary) and np.all(host[-BAND:] == canary), "a canary band was overwritten"
        return host[BAND:-BAND]

    def check(self, kind):
        got, want = self.result(DEST[kind]), self.want[DEST[kind]]
        assert np.array_equal(got.view(np.uint32 if got.dtype == np.float32 else np.uint16), want.view(np.uint32 if want.dtype == np.float32 else np.uint16)), \
            "pass %d differs in %d of %d elements" % (kind, int(np.sum(got != want)), want.size)

    def close(self):
        for t in self.tensor.values():
            self.L.libxsmm_dnn_destroy_tensor(t)
        assert 0 == self.L.libxsmm_dnn_destroy_fullyconnected(self.handle)


@pytest.fixture
def tile_env():
    old = os.environ.pop("LIBXSMM_AMD_FC_TILE", None)
    yield
    if old is None:
        os.environ.pop("LIBXSMM_AMD_FC_TILE", None)
    else:
        os.environ["LIBXSMM_AMD_FC_TILE"] = old


@pytest.mark.parametrize("name", sorted(fc.COMPUTE_CASES))
def test_three_passes_bit_equal(xs, orc, torch_gpu, tile_env, name):
    layer = Layer(xs, torch_gpu, name)
    for kind in (fc.FWD, fc.BWD, fc.UPD):
        launches = layer.L.libxsmm_amd_launch_count()
        assert 0 == xs.fc_execute(layer.handle, kind)
        assert 1 == layer.L.libxsmm_amd_launch_count() - launches, "a pass with threads = 1 is one launch"
        assert xs.last_kernel().startswith("fc_")
        layer.check(kind)
    assert np.all(layer.scratch.cpu().numpy() == 0x5a), "the scratch is never written"
    layer.close()


@pytest.mark.parametrize("tile", ("64", "128"))
def test_both_tiles_same_bits(xs, orc, torch_gpu, tile_env, tile):
    os.environ["LIBXSMM_AMD_FC_TILE"] = tile
    for name in ("l_130_32_144", "b_6_15_14", "lb_5_32_48"):
        layer = Layer(xs, torch_gpu, name)
        for kind in (fc.FWD, fc.BWD, fc.UPD):
            assert 0 == xs.fc_execute(layer.handle, kind)
            assert xs.last_kernel().endswith("_t" + tile)
            layer.check(kind)
        layer.close()


def test_bf16_ties_are_in_the_data(orc):
    h, (x, w, dy), want = case_data("lb_5_32_48")
    dx32 = (w[:2, :2].T.astype(np.float64) @ dy[1, :2].astype(np.float64))
    assert dx32[0] == 1 + 2.0 ** -8 and dx32[1] == 1 + 3 * 2.0 ** -8           # halfway between bf16 neighbours
    dx = fc.unblock_act(h, want[fc.GRAD_IN], "c")
    assert dx[1, 0] == 0x3f80 and dx[1, 1] == 0x3f82                             # to even: down, up
    assert fc.unblock_fil(h, want[fc.GRAD_FIL])[2, 3] == 0x3f80


def test_signed_zero(xs, orc, torch_gpu, tile_env):
    """products that are all -0.0 give +0.0, because the chain starts from +0.0. A partial sum can still become -0.0: a negative
    product that underflows. An odd-length chain (N = 5, UPD) must keep it through the tail: a zero-padded matrix step would
    turn it into +0.0, since fma(0, 0, -0.0) is +0.0."""
    name = "l_5_32_48"
    h, (x, w, dy), _ = case_data(name)
    minus_zero = np.float32(-0.0)
    for first, bits in ((minus_zero, 0), (np.float32(-(2.0 ** -80)), 0x80000000)):
        x2 = np.full_like(x, np.float32(2.0 ** -80))
        dy2 = np.full_like(dy, minus_zero)
        dy2[0, :] = first                            # -2^-80 * 2^-80 underflows to -0.0; every later product is -0.0
        want = fc.tensors(h, x2, np.abs(w), dy2)
        assert np.all(want[fc.GRAD_FIL].view(np.uint32) == bits)
        layer = Layer(xs, torch_gpu, name, contents=want)
        layer.want = want
        for kind in (fc.FWD, fc.BWD, fc.UPD):
            assert 0 == xs.fc_execute(layer.handle, kind)
            layer.check(kind)
        layer.close()


@pytest.mark.parametrize("name", ("l_70_48_80", "b_6_15_14", "b_64_64_96", "lb_5_32_48"))
def test_threads_do_not_enter_the_bits(xs, orc, torch_gpu, tile_env, name):
    for start in (0, 2):
        layer = Layer(xs, torch_gpu, name, threads=3)
        for kind in (fc.FWD, fc.BWD, fc.UPD):
            launches = layer.L.libxsmm_amd_launch_count()
            assert 0 == xs.fc_execute(layer.handle, kind, start, start + 5)   # no work, success
            assert 0 == layer.L.libxsmm_amd_launch_count() - launches
            assert fc.ERR_GENERAL == xs.fc_execute(layer.handle, kind, start + 1, start)  # a negative logical thread
            for tid in range(3):
                assert 0 == xs.fc_execute(layer.handle, kind, start, start + tid)
            assert layer.L.libxsmm_amd_launch_count() - launches <= 3
            layer.check(kind)
        layer.close()


def test_partial_shares_leave_the_rest_alone(xs, orc, torch_gpu, tile_env):
    """one share of three writes its blocks and nothing else (UPD in format L: a range of filter blocks that is no rectangle)"""
    name = "l_70_48_80"
    layer = Layer(xs, torch_gpu, name, threads=2)   # 15 blocks: 8 + 7, the first share ends inside a row of three
    h = fc.Handle(dict(fc.COMPUTE_CASES[name], threads=2))
    assert 0 == xs.fc_execute(layer.handle, fc.UPD, 0, 0)
    got = layer.result(fc.GRAD_FIL)
    b0, b1 = h.share(fc.UPD, 0)
    blk = 16 * 16
    assert (b0, b1) == (0, 8)
    assert np.array_equal(got[:b1 * blk].view(np.uint32), layer.want[fc.GRAD_FIL][:b1 * blk].view(np.uint32))
    assert np.all(np.isnan(got[b1 * blk:]))
    layer.close()


def test_shares_from_three_threads_with_own_streams(xs, orc, torch_gpu, tile_env):
    torch = torch_gpu
    layer = Layer(xs, torch, "l_70_48_80", threads=3)
    torch.cuda.synchronize()
    status = [None] * 3

    def share(tid):
        s = torch.cuda.Stream()
        layer.L.libxsmm_amd_set_stream(C.c_void_p(s.cuda_stream))
        status[tid] = [xs.fc_execute(layer.handle, kind, 0, tid) for kind in (fc.FWD, fc.BWD, fc.UPD)]
        s.synchronize()
        layer.L.libxsmm_amd_set_stream(None)

    workers = [threading.Thread(target=share, args=(tid,)) for tid in range(3)]
    for wk in workers:
        wk.start()
    for wk in workers:
        wk.join()
    assert status == [[0, 0, 0]] * 3
    for kind in (fc.FWD, fc.BWD, fc.UPD):
        layer.check(kind)
    layer.close()


def test_pageable_tensors_complete_on_return(xs, orc, torch_gpu, tile_env):
    L = xs.lib()
    for name in ("l_5_32_48", "b_7_10_9", "lb_5_32_48"):
        h, _, want = case_data(name)
        d = fc.COMPUTE_CASES[name]
        handle, _ = xs.fc_create(d["N"], d["C"], d["K"], d["bn"], d["bk"], d["bc"], 1, d["datatype_in"], d["datatype_out"], d["buffer_format"], d["filter_format"])
        host, tensors = {}, []
        for t in fc.TENSOR_TYPES:
            dt = fc.dtype_of(h, t)
            host[t] = want[t].astype(dt).copy() if t not in DEST.values() else np.full(want[t].size, 0xffff if dt == np.uint16 else np.nan, dtype=dt)
            tensors.append(xs.fc_bind_new(handle, t, host[t]))
        scratch = np.zeros(h.scratch(), dtype=np.uint8)
        assert fc.ERR_SCRATCH_NOT_ALLOCED == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, None)
        assert fc.ERR_DATA_NOT_BOUND == xs.fc_execute(handle, fc.BWD) == xs.fc_execute(handle, fc.UPD)   # the reference asks for a scratch there
        assert 0 == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))
        for kind in (fc.FWD, fc.BWD, fc.UPD):
            assert 0 == xs.fc_execute(handle, kind)
            assert np.array_equal(host[DEST[kind]].view(np.uint8), want[DEST[kind]].view(np.uint8))      # no wait in between
        assert not scratch.any()
        assert 0 == L.libxsmm_dnn_fullyconnected_release_scratch(handle)
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_fullyconnected(handle)


def test_mixed_residency_complete_on_return(xs, orc, torch_gpu, tile_env):
    """only what a pass writes in pageable host memory and what it reads on the device, then the reverse: the one staging block
    skips the device-resident operands and still places the others"""
    L = xs.lib()
    reads = {fc.FWD: (fc.REG_FIL, fc.REG_IN), fc.BWD: (fc.REG_FIL, fc.GRAD_OUT), fc.UPD: (fc.GRAD_OUT, fc.REG_IN)}
    for name in ("l_5_32_48", "b_7_10_9"):
        h, _, want = case_data(name)
        d = fc.COMPUTE_CASES[name]
        scratch = np.zeros(h.scratch(), dtype=np.uint8)
        for kind in (fc.FWD, fc.BWD, fc.UPD):
            after = {t: want[t].astype(fc.dtype_of(h, t)) for t in reads[kind] + (DEST[kind],)}
            roles = {t: (after[t], after[t], False) for t in reads[kind]}
            roles[DEST[kind]] = (np.full_like(after[DEST[kind]], 0xffff if after[DEST[kind]].dtype == np.uint16 else np.nan), after[DEST[kind]], True)
            for host_written in (True, False):
                handle, _ = xs.fc_create(d["N"], d["C"], d["K"], d["bn"], d["bk"], d["bc"], 1, d["datatype_in"], d["datatype_out"], d["buffer_format"], d["filter_format"])
                assert 0 == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))
                tensors = fc.check_mixed_residency(torch_gpu, roles, host_written, lambda t, m: xs.fc_bind_new(handle, t, m),
                                                   lambda: xs.fc_execute(handle, kind))
                for t in tensors:
                    L.libxsmm_dnn_destroy_tensor(t)
                L.libxsmm_dnn_destroy_fullyconnected(handle)
        assert not scratch.any()


def test_copyin_copyout_round_trip_on_a_device_tensor(xs, orc, torch_gpu, tile_env):
    torch = torch_gpu
    L = xs.lib()
    for name in ("l_5_32_48", "lb_5_32_48"):
        layer = Layer(xs, torch, name)
        h, (x, w, dy), want = case_data(name)
        lo = (lambda a: qc.bf16_rne(a).reshape(a.shape)) if h.mixed else (lambda a: a)
        for t, plain, fmt in ((fc.REG_IN, lo(x), fc.FMT_NCHW), (fc.REG_FIL, lo(w), fc.FMT_KCRS)):
            assert 0 == L.libxsmm_dnn_zero_tensor(layer.tensor[t])
            assert not layer.result(t).any()
            assert 0 == L.libxsmm_dnn_copyin_tensor(layer.tensor[t], xs.dptr(np.ascontiguousarray(plain)), fmt)
            assert np.array_equal(layer.result(t), want[t].astype(plain.dtype))
            back = torch.zeros(plain.size, dtype=torch.int16 if plain.dtype == np.uint16 else torch.float32, device="cuda")
            assert 0 == L.libxsmm_dnn_copyout_tensor(layer.tensor[t], xs.dptr(back), fmt)
            got = back.cpu().numpy()
            assert np.array_equal(got.view(plain.dtype).reshape(plain.shape), plain)
            assert fc.ERR_UNSUPPORTED_SRC_FORMAT == L.libxsmm_dnn_copyin_tensor(layer.tensor[t], xs.dptr(np.ascontiguousarray(plain)), fc.FMT_NHWC)
            assert fc.ERR_UNSUPPORTED_DST_FORMAT == L.libxsmm_dnn_copyout_tensor(layer.tensor[t], xs.dptr(back), fc.FMT_RSCK)
        layer.close()


def test_call_order_inside_the_defer_bracket(xs, orc, torch_gpu, tile_env):
    """a dispatched SMM call that produces FWD's input is recorded before FWD: FWD seals the burst and sees its result"""
    torch = torch_gpu
    L = xs.lib()
    name = "l_5_32_48"
    h, (x, w, dy), _ = case_data(name)
    N, Cc = x.shape
    rng = np.random.default_rng(11)
    p = fc.bf16_values(rng, (Cc, Cc))
    x_new = x.copy().reshape(-1)                    # x_new (C x N column-major, i.e. [N][C]) = x + p * x
    orc.smm(orc.FMA, 0, Cc, N, Cc, Cc, Cc, Cc, p.reshape(-1), x.reshape(-1), x_new)
    x_new = x_new.reshape(N, Cc)
    want = fc.tensors(h, x_new, w, dy)
    assert not np.array_equal(want[fc.REG_OUT], case_data(name)[2][fc.REG_OUT])
    fn = L.libxsmm_smmdispatch(Cc, N, Cc, None, None, None, None, None, None, None)
    assert fn
    for bracket in (False, True):
        layer = Layer(xs, torch, name)
        dp, dx = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(x.copy()).cuda()
        if bracket:
            xs.defer_begin()
        xs.call_kernel(fn, dp, dx, layer.view[fc.REG_IN])
        assert 0 == xs.fc_execute(layer.handle, fc.FWD)
        if bracket:
            xs.defer_end()
        layer.want = want
        layer.check(fc.FWD)
        layer.close()


def test_end_to_end_on_the_device_without_a_copy_back(xs, orc, torch_gpu, tile_env):
    """rne convert of x and w -> bf16 FWD -> libxsmm_matdiff against the fp32 FWD of the same data, all on the device"""
    torch = torch_gpu
    L = xs.lib()
    N, Cc, K = 33, 64, 48
    rng = np.random.default_rng(5)
    x = (rng.random((N, Cc)) - 0.5).astype(np.float32)
    w = (rng.random((K, Cc)) - 0.5).astype(np.float32)
    h32, h16 = fc.Handle(fc.desc(N, Cc, K)), fc.Handle(fc.desc(N, Cc, K, dt="bf16"))
    dx, dw = torch.from_numpy(fc.block_act(h32, x, "c")).cuda(), torch.from_numpy(fc.block_fil(h32, w)).cuda()
    dx16, dw16 = torch.zeros(N * Cc, dtype=torch.int16, device="cuda"), torch.zeros(K * Cc, dtype=torch.int16, device="cuda")
    y32, y16 = (torch.full((N * K,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    info = torch.zeros(C.sizeof(xs.MatdiffInfo), dtype=torch.uint8, device="cuda")
    keep = []
    f32, _ = xs.fc_create(N, Cc, K)
    b16, _ = xs.fc_create(N, Cc, K, datatype_in=xs.DNN_BF16)
    for handle, tx, tw, ty in ((f32, dx, dw, y32), (b16, dx16, dw16, y16)):
        keep += [xs.fc_bind_new(handle, fc.REG_IN, tx), xs.fc_bind_new(handle, fc.REG_FIL, tw), xs.fc_bind_new(handle, fc.REG_OUT, ty)]
    xs.convert_f32_bf16(dx, dx16, N * Cc)
    xs.convert_f32_bf16(dw, dw16, K * Cc)
    assert 0 == xs.fc_execute(f32, fc.FWD) == xs.fc_execute(b16, fc.FWD)
    assert 0 == xs.matdiff(y32, y16, m=K, n=N, info=info)
    torch.cuda.synchronize()
    got = xs.MatdiffInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    bound = Cc * 2.0 ** -8 * float(np.max(np.abs(w))) * float(np.max(np.abs(x)))
    assert 0 < got.linf_abs <= bound
    for t in keep:
        L.libxsmm_dnn_destroy_tensor(t)
    L.libxsmm_dnn_destroy_fullyconnected(f32)
    L.libxsmm_dnn_destroy_fullyconnected(b16)


@pytest.mark.parametrize("fmt", ("L", "B"))
def test_example_caller(xs, torch_gpu, tile_env, tmp_path, fmt):
    """examples/fc_caller.c: the reference sample's call sequence against the reference API only, checked by libxsmm_matdiff
    against naive loops; it fails above the sample's own threshold (Check-norm 1 %)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "fc_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "fc_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe), fmt], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "fc_caller %s: check norm" % fmt in res.stdout
