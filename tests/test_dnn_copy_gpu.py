"""libxsmm_dnn_copyin_tensor / _copyout_tensor on the GPU (kernels/dnn_copy.hip) and their forms without a wait: every layout of
tests/dnn_copy_common.py bit for bit against the numpy restatement of the reference's templates, one launch per call, every mix
of device, pinned and pageable operands, bases off their 16-byte boundary, the async forms in a chain with a layer, their
refusals, and call order inside the defer bracket. Every buffer lies between 64-byte canaries of 0xA5 that must survive; the
bits are arbitrary (NaN payloads, +-0, Inf, subnormals among them): nothing here may round."""
import ctypes as C

import numpy as np
import pytest

import dnn_copy_common as dc
import fc_common as fc

pytestmark = pytest.mark.gpu

# layouts no handle here returns, as copies of a case's layout with other extents
RESIZED = {
    "fil_bf16_3x3_lpb2": ("fil_fc_bf16", [2, 16, 8, 3, 3, 2, 2]),
    "fil_64x64_blocks": ("fil_fc_f32", [64, 64, 1, 1, 2, 2]),
    "fil_cut_odd_rest": ("fil_c16_k16_11x11", [19, 16, 11, 11, 1, 2]),       # 19 rows in passes of 8: a rest of 3
    "fil_row_beyond_lds": ("fil_fc_f32", [2, 64, 17, 17, 2, 1]),              # 73 984 bytes per row: without LDS
    "act_two_tiles": ("act_8x8", [16, 20, 20, 2, 1]),                         # 400 pixels: tiles of 256
    "act_wide_block": ("act_8x8", [300, 9, 9, 1, 1]),                         # rows and run cut
    "act_bf16_odd_block": ("act_bn_bf16_6x6", [1, 3, 30, 30, 1, 1]),
}


class Layout:
    """a case's layout, or a resized copy of one"""

    def __init__(self, xs, name):
        self.xs, self.copy = xs, None
        self.case = dc.Case(xs, RESIZED[name][0] if name in RESIZED else name)
        self.layout, self.fmt = self.case.layout, self.case.fmt
        if name in RESIZED:
            self.layout = self.copy = dc.resized(xs, self.case.layout, RESIZED[name][1])
        self.fields = xs.dnn_layout_fields(self.layout)
        self.ts = dc.typesize(self.fields)
        self.nbytes = dc.elements(self.fields) * self.ts

    def tensor(self, buf):
        t, st = self.xs.dnn_link_tensor(self.layout, buf.ptr)
        assert t and 0 == st
        return t

    def close(self):
        if self.copy is not None:
            self.xs.lib().libxsmm_dnn_destroy_tensor_datalayout(self.copy)
        self.case.close()


def counted(xs, call, launches=1):
    """runs call(); asserts its status, the number of launches and, if there was one, that a dnn_copy kernel was the last"""
    L = xs.lib()
    before = L.libxsmm_amd_launch_count()
    assert 0 == call()
    assert before + launches == L.libxsmm_amd_launch_count()
    if 0 < launches:
        assert xs.last_kernel().startswith("dnn_copy"), xs.last_kernel()
        return xs.last_kernel()
    return None


@pytest.mark.parametrize("name", sorted(dc.CASES) + sorted(RESIZED))
def test_copy_in_then_copy_out_on_the_device(xs, torch_gpu, name):
    L = xs.lib()
    lay = Layout(xs, name)
    data = dc.hostile_bytes(lay.nbytes, 17, lay.ts)
    plain = dc.Guarded(torch_gpu, lay.nbytes, "device", content=data)
    buf = dc.Guarded(torch_gpu, lay.nbytes, "device")
    back = dc.Guarded(torch_gpu, lay.nbytes, "device")
    tensor = lay.tensor(buf)
    kin = counted(xs, lambda: L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, lay.fmt))
    want = dc.copy_in(lay.fields, data)
    assert np.array_equal(buf.payload(), want), "the tensor differs from the restatement"
    kout = counted(xs, lambda: L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, lay.fmt))
    assert np.array_equal(back.payload(), data), "the plain buffer does not come back"
    assert np.array_equal(plain.payload(), data) and np.array_equal(buf.payload(), want)  # the sources are untouched
    st, plan = xs.dnn_copy_plan(lay.layout, lay.fmt)
    form = "flat" if 0 == plan[0] else ("tiled" if 0 < plan[5] else "direct")
    assert (kin, kout) == (("dnn_copy_flat",) * 2 if "flat" == form else ("dnn_copy_in_" + form, "dnn_copy_out_" + form))
    L.libxsmm_dnn_destroy_tensor(tensor)
    lay.close()


def test_host_operands_launch_nothing(xs, torch_gpu):
    L = xs.lib()
    for name in ("act_5x13", "fil_c3_k16_7x7", "bias_k40"):
        lay = Layout(xs, name)
        data = dc.hostile_bytes(lay.nbytes, 21, lay.ts)
        for where_t, where_p in (("pageable", "pageable"), ("pageable", "pinned"), ("pinned", "pageable")):
            plain, buf, back = dc.Guarded(torch_gpu, lay.nbytes, where_p, content=data), dc.Guarded(torch_gpu, lay.nbytes, where_t), dc.Guarded(torch_gpu, lay.nbytes, where_p)
            tensor = lay.tensor(buf)
            counted(xs, lambda: L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, lay.fmt), launches=0)
            counted(xs, lambda: L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, lay.fmt), launches=0)
            assert np.array_equal(buf.payload(), dc.copy_in(lay.fields, data)) and np.array_equal(back.payload(), data)
            L.libxsmm_dnn_destroy_tensor(tensor)
        lay.close()


@pytest.mark.parametrize("name", ("act_conv_c24_7x9", "fil_c24_k40_3x3"))
def test_residency_matrix(xs, torch_gpu, name):
    """the same bytes wherever the operands lie; a pageable operand is staged, a pinned one is used in place; complete on return:
    pageable and pinned results are read with no wait after the call"""
    L = xs.lib()
    lay = Layout(xs, name)
    data = dc.hostile_bytes(lay.nbytes, 23, lay.ts)
    want = dc.copy_in(lay.fields, data)
    for where_t, where_p in (("device", "pageable"), ("device", "pinned"), ("device", "device"), ("pageable", "device"), ("pinned", "device")):
        plain, buf = dc.Guarded(torch_gpu, lay.nbytes, where_p, content=data), dc.Guarded(torch_gpu, lay.nbytes, where_t)
        tensor = lay.tensor(buf)
        counted(xs, lambda: L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, lay.fmt))
        if "device" != where_t:  # (no wait: the call is complete on return)
            assert np.array_equal(buf.mem[buf.off:buf.off + lay.nbytes] if "pageable" == where_t else buf.mem.numpy()[buf.off:buf.off + lay.nbytes], want)
        assert np.array_equal(buf.payload(), want), (where_t, where_p)
        back = dc.Guarded(torch_gpu, lay.nbytes, where_p)
        counted(xs, lambda: L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, lay.fmt))
        if "device" != where_p:
            assert np.array_equal(back.mem[back.off:back.off + lay.nbytes] if "pageable" == where_p else back.mem.numpy()[back.off:back.off + lay.nbytes], data)
        assert np.array_equal(back.payload(), data), (where_t, where_p)
        assert np.array_equal(plain.payload(), data)
        L.libxsmm_dnn_destroy_tensor(tensor)
    lay.close()


@pytest.mark.parametrize("name", ("act_8x8", "fil_c24_k40_3x3"))
def test_bases_off_their_16_byte_boundary(xs, torch_gpu, name):
    """the plain base and the tensor base one element past a 16-byte boundary, each alone and both: the bytes of the aligned case"""
    L = xs.lib()
    lay = Layout(xs, name)
    data = dc.hostile_bytes(lay.nbytes, 29, lay.ts)
    want = dc.copy_in(lay.fields, data)
    for shift_t, shift_p in ((0, lay.ts), (lay.ts, 0), (lay.ts, lay.ts)):
        plain = dc.Guarded(torch_gpu, lay.nbytes, "device", content=data, shift=shift_p)
        buf, back = dc.Guarded(torch_gpu, lay.nbytes, "device", shift=shift_t), dc.Guarded(torch_gpu, lay.nbytes, "device", shift=shift_p)
        assert (lay.ts if shift_t else 0) == buf.ptr % 16 and (lay.ts if shift_p else 0) == plain.ptr % 16
        tensor = lay.tensor(buf)
        counted(xs, lambda: L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, lay.fmt))
        assert np.array_equal(buf.payload(), want), (shift_t, shift_p)
        counted(xs, lambda: L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, lay.fmt))
        assert np.array_equal(back.payload(), data), (shift_t, shift_p)
        L.libxsmm_dnn_destroy_tensor(tensor)
    lay.close()


def test_async_chain_with_a_layer(xs, torch_gpu):
    """copy-in of x and w, FC FWD, copy-out of y on one stream with no wait in between, then one libxsmm_amd_synchronize: what the
    synchronous sequence gives"""
    torch = torch_gpu
    L = xs.lib()
    name = "l_5_32_48"
    d = fc.COMPUTE_CASES[name]
    x, w, _ = fc.plain_inputs(name, d)
    N, Cc, K = d["N"], d["C"], d["K"]
    handle, _ = xs.fc_create(*[d[k] for k in fc.DESC_FIELDS])
    size = L.libxsmm_dnn_fullyconnected_get_scratch_size(handle, C.byref(C.c_uint()))
    scratch = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert 0 == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))
    px = dc.Guarded(torch, 4 * N * Cc, "device", content=x.astype(np.float32))
    pw = dc.Guarded(torch, 4 * K * Cc, "device", content=w.astype(np.float32))
    results = []
    stream = torch.cuda.Stream()
    for use_async in (False, True):
        tx, tw, ty = dc.Guarded(torch, 4 * N * Cc, "device"), dc.Guarded(torch, 4 * K * Cc, "device"), dc.Guarded(torch, 4 * N * K, "device")
        py = dc.Guarded(torch, 4 * N * K, "device")
        tensors = [xs.fc_bind_new(handle, t, b.ptr) for t, b in ((fc.REG_IN, tx), (fc.REG_FIL, tw), (fc.REG_OUT, ty))]
        torch.cuda.synchronize()
        if use_async:
            L.libxsmm_amd_set_stream(stream.cuda_stream)
            cin, cout = L.libxsmm_amd_dnn_copyin_tensor_async, L.libxsmm_amd_dnn_copyout_tensor_async
        else:
            cin, cout = L.libxsmm_dnn_copyin_tensor, L.libxsmm_dnn_copyout_tensor
        try:
            assert 0 == cin(tensors[0], px.ptr, dc.FMT_NCHW) == cin(tensors[1], pw.ptr, dc.FMT_KCRS)
            assert 0 == xs.fc_execute(handle, fc.FWD)
            assert 0 == cout(tensors[2], py.ptr, dc.FMT_NCHW)
            assert 0 == L.libxsmm_amd_synchronize()
        finally:
            L.libxsmm_amd_set_stream(None)
        results.append(py.payload())
        for b in (tx, tw, ty):
            b.payload()  # the canaries
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
    y = results[0].view(np.float32).reshape(N, K)
    assert np.array_equal(results[0], results[1])
    assert np.allclose(y, x.astype(np.float64) @ w.astype(np.float64).T, rtol=1e-4, atol=1e-5)  # (the sequence computes the layer at all)
    L.libxsmm_dnn_destroy_fullyconnected(handle)


def test_async_forms_refuse_pageable_operands(xs, torch_gpu):
    L = xs.lib()
    for name in ("act_8x8", "fil_c24_k40_3x3", "bias_k40"):
        lay = Layout(xs, name)
        data = dc.hostile_bytes(lay.nbytes, 31, lay.ts)
        for where_t, where_p in (("device", "pageable"), ("pageable", "device"), ("pageable", "pageable")):
            plain, buf = dc.Guarded(torch_gpu, lay.nbytes, where_p, content=data), dc.Guarded(torch_gpu, lay.nbytes, where_t)
            tensor = lay.tensor(buf)
            before = L.libxsmm_amd_launch_count()
            assert dc.ERR_GENERAL == L.libxsmm_amd_dnn_copyin_tensor_async(tensor, plain.ptr, lay.fmt)
            assert dc.ERR_GENERAL == L.libxsmm_amd_dnn_copyout_tensor_async(tensor, plain.ptr, lay.fmt)
            assert before == L.libxsmm_amd_launch_count()
            assert np.all(buf.payload() == 0x3C) and np.array_equal(plain.payload(), data)
            L.libxsmm_dnn_destroy_tensor(tensor)
        # pinned memory is memory the GPU reaches
        plain, buf = dc.Guarded(torch_gpu, lay.nbytes, "pinned", content=data), dc.Guarded(torch_gpu, lay.nbytes, "device")
        tensor = lay.tensor(buf)
        counted(xs, lambda: L.libxsmm_amd_dnn_copyin_tensor_async(tensor, plain.ptr, lay.fmt))
        assert 0 == L.libxsmm_amd_synchronize()
        assert np.array_equal(buf.payload(), dc.copy_in(lay.fields, data))
        L.libxsmm_dnn_destroy_tensor(tensor)
        lay.close()


def test_call_order_inside_the_defer_bracket(xs, torch_gpu):
    """a recorded libxsmm_gemm_batch call writes C; the copy-out of C as a linked tensor is not recorded: it launches what is open and
    sees the batch's result"""
    torch = torch_gpu
    L = xs.lib()
    lay = Layout(xs, "act_8x8")  # 2048 fp32 elements: the C of eight 16 x 16 products
    m, batch = 16, lay.nbytes // (4 * 16 * 16)
    rng = np.random.default_rng(37)
    a = rng.integers(-4, 5, (batch, m, m)).astype(np.float32)  # (small integers: every sum is exact in any order)
    b = rng.integers(-4, 5, (batch, m, m)).astype(np.float32)
    cwant = np.matmul(b, a)  # column-major C = A * B is, row by row, B^T A^T
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    idx = torch.arange(batch, dtype=torch.int32, device="cuda") * (m * m)
    for bracket in (False, True):
        cbuf = dc.Guarded(torch, lay.nbytes, "device")
        plain = dc.Guarded(torch, lay.nbytes, "device")
        tensor = lay.tensor(cbuf)
        if bracket:
            xs.defer_begin()
        xs.gemm_batch(xs.F32, "N", "N", m, m, m, 1.0, da, m, db, m, 0.0, cbuf.ptr, m, 0, 4, idx, idx, idx, batch)
        assert 0 == L.libxsmm_dnn_copyout_tensor(tensor, plain.ptr, lay.fmt)
        assert xs.last_kernel().startswith("dnn_copy_out")
        got = plain.payload()  # (before the bracket closes)
        if bracket:
            xs.defer_end()
        assert np.array_equal(cbuf.payload().view(np.float32), cwant.reshape(-1)), bracket
        assert np.array_equal(got, dc.copy_out(lay.fields, cwant)), bracket
        L.libxsmm_dnn_destroy_tensor(tensor)
    lay.close()
