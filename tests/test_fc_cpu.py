"""The fully-connected layer without a GPU: the numpy restatement (tests/fc_common.py) against what the reference returned
(tests/golden/fc.npz, captured by tools/golden/fc_capture.*), the built library's host-side functions against the same
values, the blocked composition against the plain one inside the oracle, and the reference's outputs against the oracle's."""
import ctypes as C
import zlib

import numpy as np
import pytest

import fc_common as fc
import quant_common as qc

META_LAYOUT, META_EXEC, META_COPY = 4, 160, 165


@pytest.fixture(scope="module")
def golden():
    return fc.load_golden()


def meta_layout(meta, i):
    m = meta[META_LAYOUT + 26 * i:META_LAYOUT + 26 * (i + 1)]
    if m[1] < 0:
        return int(m[0]), None
    n = int(m[1])
    return int(m[0]), dict(num_dims=n, dim_type=[int(v) for v in m[2:2 + n]], dim_size=[int(v) for v in m[10:10 + n]], datatype=int(m[18]), format=int(m[19]),
                           custom_format=int(m[20]), tensor_type=int(m[21]), size=int(m[22]), elements=int(m[23]), link=int(m[24]), bind=int(m[25]))


def bound_types(name, h):
    return [t for t in fc.TENSOR_TYPES if h.layout(t)[1] is not None and t not in fc.UNBOUND.get(name, ())]


@pytest.mark.parametrize("name", sorted(fc.all_cases()))
def test_restatement_reproduces_the_reference(golden, name):
    d = fc.all_cases()[name]
    meta = golden[name + "/meta"]
    assert list(golden[name + "/desc"]) == [d[k] for k in fc.DESC_FIELDS]
    h = fc.Handle(d)
    assert (h.status, int(h.ok)) == (int(meta[0]), int(meta[1]))
    if not h.ok:
        return
    assert (h.scratch(), 0) == (int(meta[2]), int(meta[3]))
    for i, t in enumerate(fc.TENSOR_TYPES):
        status, ref = meta_layout(meta, i)
        st, mine = h.layout(t)
        assert st == status and (mine is None) == (ref is None)
        if mine is not None:
            assert mine == {k: ref[k] for k in mine}
            assert fc.layout_size(mine) == (ref["size"], ref["elements"])
            assert (ref["link"], ref["bind"]) == (0, -1 if t in fc.UNBOUND.get(name, ()) else 0)
    bound = bound_types(name, h)
    for kind in (fc.FWD, fc.BWD, fc.UPD, fc.BWDUPD, fc.ALL):
        assert h.execute_status(kind, bound) == int(meta[META_EXEC + kind]), kind
    if name in fc.COMPUTE_CASES:
        x, w, dy = fc.plain_inputs(name, d)
        for key, a in (("x", x), ("w", w), ("dy", dy)):
            assert zlib.crc32(np.ascontiguousarray(a).tobytes()) == int(golden[name + "/crc_" + key][0]), "the seeded inputs changed"
            if name + "/in_" + key in golden:
                assert np.array_equal(qc.bf16_widen(golden[name + "/in_" + key]).reshape(a.shape), a)
        if h.custom:
            assert [int(v) for v in meta[META_COPY:META_COPY + 4]] == [0, 0, 0, 0]
            lo = (lambda a: qc.bf16_rne(a).reshape(a.shape)) if h.mixed else (lambda a: a)
            images = {"cin_x": fc.block_act(h, lo(x), "c"), "cin_w": fc.block_fil(h, lo(w)), "cout_x": lo(x), "cout_w": lo(w)}
            for key, image in images.items():  # (the images of the largest tensors are not stored)
                if name + "/" + key in golden:
                    assert golden[name + "/" + key].tobytes() == image.tobytes(), key
            assert name + "/cin_x" in golden and (name + "/cin_w" in golden or w.size > 8192)
        else:
            assert [int(v) for v in meta[META_COPY:META_COPY + 4]] == [fc.ERR_UNSUPPORTED_DST_FORMAT] * 2 + [fc.ERR_UNSUPPORTED_SRC_FORMAT] * 2


@pytest.mark.parametrize("name", sorted(fc.all_cases()))
def test_library_host_side_matches_the_reference(xs, golden, name):
    """create, layouts, sizes, scratch, bind and the statuses execute_st gives before it needs a device"""
    L = xs.lib()
    d = fc.all_cases()[name]
    meta = golden[name + "/meta"]
    handle, status = xs.fc_create(*[d[k] for k in fc.DESC_FIELDS])
    assert (status, int(bool(handle))) == (int(meta[0]), int(meta[1]))
    if not handle:
        return
    st = C.c_uint(7)
    assert L.libxsmm_dnn_fullyconnected_get_scratch_size(handle, C.byref(st)) == int(meta[2]) and 0 == st.value
    tensors, keep = {}, []
    for i, t in enumerate(fc.TENSOR_TYPES):
        status, ref = meta_layout(meta, i)
        layout, st = xs.fc_layout(handle, t)
        assert st == status and (layout is None) == (ref is None)
        if layout is None:
            continue
        n, types, sizes, datatype, fmt, custom, ttype = xs.dnn_layout_fields(layout)
        assert (n, types, sizes, datatype, fmt, custom, ttype) == (ref["num_dims"], ref["dim_type"], ref["dim_size"], ref["datatype"], ref["format"],
                                                                  ref["custom_format"], ref["tensor_type"])
        s2 = C.c_uint(7)
        assert L.libxsmm_dnn_get_tensor_size(layout, C.byref(s2)) == ref["size"] and L.libxsmm_dnn_get_tensor_elements(layout, C.byref(s2)) == ref["elements"]
        buf = np.zeros(ref["size"] + 8, dtype=np.uint8)
        keep.append(buf)
        tensor, st = xs.dnn_link_tensor(layout, buf)
        assert tensor and 0 == st
        assert L.libxsmm_dnn_get_tensor_data_ptr(tensor, C.byref(s2)) == buf.ctypes.data
        copy = L.libxsmm_dnn_get_tensor_datalayout(tensor, C.byref(s2))
        assert 0 == L.libxsmm_dnn_compare_tensor_datalayout(layout, copy, C.byref(s2))
        copy.contents.dim_size[0] += 1
        assert 1 == L.libxsmm_dnn_compare_tensor_datalayout(layout, copy, C.byref(s2))
        wrong, st = xs.dnn_link_tensor(copy, buf)
        assert fc.ERR_MISMATCH_TENSOR == L.libxsmm_dnn_fullyconnected_bind_tensor(handle, wrong, t)
        assert 0 == L.libxsmm_dnn_destroy_tensor(wrong) == L.libxsmm_dnn_destroy_tensor_datalayout(copy) == L.libxsmm_dnn_destroy_tensor_datalayout(layout)
        if t not in fc.UNBOUND.get(name, ()):
            assert 0 == L.libxsmm_dnn_fullyconnected_bind_tensor(handle, tensor, t)
            assert L.libxsmm_dnn_fullyconnected_get_tensor(handle, t, C.byref(s2)) == tensor
        tensors[t] = tensor
    assert fc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_fullyconnected_bind_tensor(handle, None, 7)
    assert fc.ERR_SCRATCH_NOT_ALLOCED == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, None)
    scratch = np.zeros(int(meta[2]), dtype=np.uint8)
    assert 0 == L.libxsmm_dnn_fullyconnected_bind_scratch(handle, xs.dptr(scratch))
    for kind in (fc.FWD, fc.BWD, fc.UPD, fc.BWDUPD, fc.ALL):
        want = int(meta[META_EXEC + kind])
        if 0 != want:  # (a pass that would run needs a device)
            assert want == xs.fc_execute(handle, kind), kind
    for t in tensors.values():
        L.libxsmm_dnn_destroy_tensor(t)
    assert 0 == L.libxsmm_dnn_destroy_fullyconnected(handle)
    assert fc.ERR_INVALID_HANDLE == L.libxsmm_dnn_destroy_fullyconnected(None) == xs.fc_execute(None, fc.FWD)
    assert b"fullyconnected" in L.libxsmm_dnn_get_error(fc.ERR_INVALID_FORMAT_FC)


def test_copies_on_host_memory(xs, golden):
    """copy-in / copy-out / zero of the library on pageable memory: the reference's bytes (needs no device)"""
    L = xs.lib()
    for name in ("l_5_32_48", "lb_5_32_48"):
        d = fc.COMPUTE_CASES[name]
        h = fc.Handle(d)
        handle, _ = xs.fc_create(*[d[k] for k in fc.DESC_FIELDS])
        for t, key, fmt in ((fc.GRAD_IN, "x", fc.FMT_NCHW), (fc.GRAD_FIL, "w", fc.FMT_KCRS)):
            layout, _ = xs.fc_layout(handle, t)
            plain = golden[name + "/cout_" + key].copy()
            buf = np.full(plain.size, 0xff, dtype=np.uint8)
            tensor, _ = xs.dnn_link_tensor(layout, buf)
            assert 0 == L.libxsmm_dnn_copyin_tensor(tensor, xs.dptr(plain), fmt)
            assert np.array_equal(buf, golden[name + "/cin_" + key])
            back = np.zeros_like(plain)
            assert 0 == L.libxsmm_dnn_copyout_tensor(tensor, xs.dptr(back), fmt)
            assert np.array_equal(back, plain)
            assert fc.ERR_UNSUPPORTED_SRC_FORMAT == L.libxsmm_dnn_copyin_tensor(tensor, xs.dptr(plain), fc.FMT_NHWC)
            assert 0 == L.libxsmm_dnn_zero_tensor(tensor) and not buf.any()
            L.libxsmm_dnn_destroy_tensor(tensor)
            L.libxsmm_dnn_destroy_tensor_datalayout(layout)
        L.libxsmm_dnn_destroy_fullyconnected(handle)


def test_blocked_composition_equals_the_plain_one(orc):
    """format B, FWD: one orc.smm_reduce per output block over the C/bc blocks is bit-equal to the single plain orc.smm call"""
    for name in ("b_6_15_14", "b_64_64_96"):
        d = fc.COMPUTE_CASES[name]
        h = fc.Handle(d)
        x, w, dy = fc.plain_inputs(name, d)
        want = fc.tensors(h, x, w, dy)[fc.REG_OUT]
        bn, bc, bk = h.blocks()
        N, Cc, K = d["N"], d["C"], d["K"]
        tx, tw = fc.block_act(h, x, "c").reshape(N // bn, Cc // bc, bn * bc), fc.block_fil(h, w).reshape(K // bk, Cc // bc, bc * bk)
        got = np.full((N // bn, K // bk, bn * bk), np.nan, dtype=np.float32)
        for mb in range(N // bn):
            for ofm in range(K // bk):
                a = [np.ascontiguousarray(tw[ofm, ifm]) for ifm in range(Cc // bc)]
                b = [np.ascontiguousarray(tx[mb, ifm]) for ifm in range(Cc // bc)]
                block = np.full(bn * bk, np.nan, dtype=np.float32)
                orc.smm_reduce(orc.FMA, orc.FLAG_BETA_0, bk, bn, bc, bk, bc, bk, a, b, block)
                got[mb, ofm] = block
        assert np.array_equal(got.reshape(-1).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", sorted(fc.COMPUTE_CASES))
def test_reference_outputs_against_the_oracle(golden, orc, name):
    """The reference's outputs (generic drivers, AVX2 JIT kernels: fma, k ascending, the accumulator kept across the batch-reduce)
    are bit-equal to the oracle's chains in every captured case: asserted as equality."""
    d = fc.COMPUTE_CASES[name]
    h = fc.Handle(d)
    want = fc.tensors(h, *fc.plain_inputs(name, d))
    for key, t in (("y", fc.REG_OUT), ("dx", fc.GRAD_IN), ("dw", fc.GRAD_FIL)):
        got = golden[name + "/" + key]
        assert got.tobytes() == want[t].tobytes(), "%s of %s: %d bytes differ" % (key, name, int(np.sum(got != want[t].view(np.uint8))))
