"""The pooling layer without a GPU: the header as C89 and C++, the exported symbols, the numpy restatement (tests/pool_common.py)
against what the reference returned (tests/golden/pool.npz, captured by tools/golden/pool_capture.* with LIBXSMM_TARGET=hsw),
and the built library's host-side functions against the same values.

One layout is not compared: the mask of a BF16 handle. The reference reports six dimensions for it and sets the sizes of five, so
the sixth and the tensor sizes derived from it are uninitialised memory (recorded as -2); the engine reports the five dimensions
its fp32 branch reports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pool_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META_LAYOUT, META_EXEC = 10, 220
SYMBOLS = ("libxsmm_dnn_create_pooling", "libxsmm_dnn_destroy_pooling", "libxsmm_dnn_pooling_create_tensor_datalayout",
           "libxsmm_dnn_pooling_get_scratch_size", "libxsmm_dnn_pooling_bind_scratch", "libxsmm_dnn_pooling_release_scratch",
           "libxsmm_dnn_pooling_bind_tensor", "libxsmm_dnn_pooling_get_tensor", "libxsmm_dnn_pooling_release_tensor", "libxsmm_dnn_pooling_execute_st")
CASES = sorted(pc.captured_cases())


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def meta_layout(meta, i):
    m = meta[META_LAYOUT + 26 * i:META_LAYOUT + 26 * (i + 1)]
    if m[1] < 0:
        return int(m[0]), None
    n = int(m[1])
    return int(m[0]), dict(num_dims=n, dim_type=[int(v) for v in m[2:2 + n]], dim_size=[int(v) for v in m[10:10 + n]], datatype=int(m[18]), format=int(m[19]),
                           custom_format=int(m[20]), tensor_type=int(m[21]), size=int(m[22]), elements=int(m[23]), link=int(m[24]), bind=int(m[25]))


def uninitialised(ref):
    return ref is not None and ref["size"] == -2


def bound_types(name, h):
    return [t for t in pc.BINDABLE if h.layout(t)[1] is not None and t not in pc.UNBOUND.get(name, ())]


@pytest.mark.parametrize("std", ("c89", "c++11"))
def test_header_compiles(tmp_path, std):
    cxx = std.startswith("c++")
    src = tmp_path / ("t.cpp" if cxx else "t.c")
    src.write_text("#include <libxsmm_dnn_pooling.h>\nint main(void) { libxsmm_dnn_pooling_desc d; d.pooling_type = LIBXSMM_DNN_POOLING_AVG; "
                   "return LIBXSMM_DNN_POOLING_MAX == 1 && LIBXSMM_DNN_POOLING_MASK == 31 && (int)sizeof(d) == 80 ? 0 : 1; }\n")
    subprocess.run(["g++" if cxx else "gcc", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_symbols_are_exported(xs):
    L = xs.lib()
    for name in SYMBOLS:
        assert getattr(L, name)
    for name in ("pool_create", "pool_layout", "pool_bind_new", "pool_execute"):
        assert callable(getattr(xs, name))
    assert b"pooling" in L.libxsmm_dnn_get_error(pc.ERR_UNSUPPORTED_POOLING).lower()


def test_the_golden_file_holds_the_cases(golden):
    assert os.path.getsize(os.path.join(pc.GOLDEN, "pool.npz")) < 1 << 20
    for name, d in pc.captured_cases().items():
        assert list(golden[name + "/desc"]) == [d[k] for k in pc.DESC_FIELDS]
    with_outputs = [n for n in pc.captured_cases() if n + "/crc_out" in golden]
    assert set(with_outputs) >= set(pc.GOLDEN_CASES) | set(pc.SPECIAL_CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_statuses(golden, name):
    d = pc.captured_cases()[name]
    meta = golden[name + "/meta"]
    h = pc.Handle(d)
    assert (h.status, int(h.ok)) == (int(meta[0]), int(meta[1]))
    if not h.ok:
        return
    assert (h.scratch(), 0) == (int(meta[2]), int(meta[3]))
    assert [int(v) for v in meta[4:7]] == [pc.ERR_SCRATCH_NOT_ALLOCED, 0, 0]
    assert int(meta[8]) == pc.ERR_INVALID_HANDLE_TENSOR
    for i, t in enumerate(pc.LAYOUT_TYPES):
        status, ref = meta_layout(meta, i)
        st, mine = h.layout(t)
        assert st == status and (mine is None) == (ref is None), t
        if mine is None or uninitialised(ref):
            continue
        assert mine == {k: ref[k] for k in mine}
        assert pc.layout_size(mine) == (ref["size"], ref["elements"])
        if t in pc.BINDABLE:
            assert (ref["link"], ref["bind"]) == (0, -1 if t in pc.UNBOUND.get(name, ()) else 0)
    if h.layout(pc.REG_IN)[1] is not None:
        assert [int(meta[7]), int(meta[9])] == [pc.ERR_UNKNOWN_TENSOR_TYPE] * 2
    bound = bound_types(name, h)
    for kind in (pc.FWD, pc.BWD, pc.UPD, pc.BWDUPD, pc.ALL):
        if int(meta[META_EXEC + kind]) >= 0:  # (-1: the reference was not run -- NO_RUN, or BWD on a mask with sentinels)
            assert h.execute_status(kind, bound) == int(meta[META_EXEC + kind]), kind
    assert (name in pc.NO_RUN) == (int(meta[META_EXEC]) < 0)
    assert (name in pc.SPECIAL_CASES) == (1 == int(meta[225]))


@pytest.mark.parametrize("name", [n for n in CASES if n in pc.COMPUTE_CASES or n in pc.SPECIAL_CASES or n == "e_avg_nomask"])
def test_restatement_reproduces_the_reference_outputs(golden, name):
    """bit for bit, every case that has outputs: the separate multiply and add of the average BWD included"""
    d = pc.captured_cases()[name]
    e = pc.expected(name, d)
    assert pc.crc(e["x"]) == int(golden[name + "/crc_x"][0]) and pc.crc(e["dout"]) == int(golden[name + "/crc_dout"][0]), "the seeded inputs changed"
    keys = ["out"] + (["mask"] if d["pooling_type"] == pc.MAX else []) + ([] if name in pc.SPECIAL_CASES else ["din"])
    for key in keys:
        assert pc.crc(e[key]) == int(golden[name + "/crc_" + key][0]), key
        if name + "/" + key in golden:
            assert golden[name + "/" + key].tobytes() == e[key].tobytes(), key
        else:
            assert e[key].size > 8192
    if name in pc.SPECIAL_CASES:
        h = pc.Handle(d)
        assert name + "/crc_din" not in golden
        out, mask = pc.as_f32(h, e["out"]), e["mask"]
        lowest = pc.as_f32(h, pc.stored(h, np.array([-pc.FLT_MAX], dtype=np.float32)))[0]
        assert np.all(out[0, 0, 0] == lowest) and np.all(mask[0, 0, 0] == pc.SENTINEL)
        assert np.all(out[1, 1, 2] == lowest) and np.all(mask[1, 1, 2] == pc.SENTINEL)
        assert out[3, 3, 0, 3] == lowest and mask[3, 3, 0, 3] == pc.SENTINEL and np.all(np.delete(mask[3, 3, 0], 3) >= 0)
        assert int(np.sum(mask == pc.SENTINEL)) == 33


def test_fused_or_separate_is_decided_by_the_capture(golden):
    """the average BWD of the reference's build is a multiply and an add: the fused form gives other bits in every captured case
    with more than one covering output, and the same where there is one (one product added to +0.0 is exact either way)"""
    for name in ("a_avg_f32_n", "g_avg_f32_n", "g_avg_bf16_n", "c_avg_f32_n"):
        d = pc.COMPUTE_CASES[name]
        fused = pc.expected(name, d, fused=True)["din"]
        same = pc.crc(fused) == int(golden[name + "/crc_din"][0])
        assert same == name.startswith("c_"), name


@pytest.mark.parametrize("name", CASES)
def test_library_host_side_matches_the_reference(xs, golden, name):
    """create, layouts, sizes, scratch, bind and the statuses execute_st gives before it needs a device"""
    L = xs.lib()
    d = pc.captured_cases()[name]
    meta = golden[name + "/meta"]
    h = pc.Handle(d)
    handle, status = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
    assert (status, int(bool(handle))) == (int(meta[0]), int(meta[1]))
    if not handle:
        return
    st = C.c_uint(7)
    assert L.libxsmm_dnn_pooling_get_scratch_size(handle, C.byref(st)) == int(meta[2]) and 0 == st.value
    tensors, keep = {}, []
    for i, t in enumerate(pc.LAYOUT_TYPES):
        status, ref = meta_layout(meta, i)
        layout, st = xs.pool_layout(handle, t)
        assert st == status and (layout is None) == (ref is None)
        if layout is None:
            continue
        fields = xs.dnn_layout_fields(layout)
        _, mine = h.layout(t)
        assert fields == (mine["num_dims"], mine["dim_type"], mine["dim_size"], mine["datatype"], mine["format"], mine["custom_format"], mine["tensor_type"])
        s2 = C.c_uint(7)
        size, elements = pc.layout_size(mine)
        if not uninitialised(ref):
            assert fields == (ref["num_dims"], ref["dim_type"], ref["dim_size"], ref["datatype"], ref["format"], ref["custom_format"], ref["tensor_type"])
            assert (size, elements) == (ref["size"], ref["elements"])
        assert L.libxsmm_dnn_get_tensor_size(layout, C.byref(s2)) == size and L.libxsmm_dnn_get_tensor_elements(layout, C.byref(s2)) == elements
        if t in pc.BINDABLE:
            buf = np.zeros(size + 8, dtype=np.uint8)
            keep.append(buf)
            tensor, st = xs.dnn_link_tensor(layout, buf)
            assert tensor and 0 == st
            copy = L.libxsmm_dnn_get_tensor_datalayout(tensor, C.byref(s2))
            copy.contents.dim_size[1] += 1
            wrong, st = xs.dnn_link_tensor(copy, buf)
            assert pc.ERR_MISMATCH_TENSOR == L.libxsmm_dnn_pooling_bind_tensor(handle, wrong, t)
            assert 0 == L.libxsmm_dnn_destroy_tensor(wrong) == L.libxsmm_dnn_destroy_tensor_datalayout(copy)
            if t not in pc.UNBOUND.get(name, ()):
                assert 0 == L.libxsmm_dnn_pooling_bind_tensor(handle, tensor, t)
                assert L.libxsmm_dnn_pooling_get_tensor(handle, t, C.byref(s2)) == tensor and 0 == s2.value
            tensors[t] = tensor
        assert 0 == L.libxsmm_dnn_destroy_tensor_datalayout(layout)
    # the tensor type is looked at first, then the pointers
    assert pc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_pooling_bind_tensor(None, None, pc.REG_FIL) == L.libxsmm_dnn_pooling_release_tensor(handle, pc.GEN_IN)
    assert pc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_pooling_bind_tensor(handle, None, pc.REG_IN) == L.libxsmm_dnn_pooling_bind_tensor(None, None, pc.MASK)
    s2 = C.c_uint(7)
    assert not L.libxsmm_dnn_pooling_get_tensor(handle, pc.REG_FIL, C.byref(s2)) and pc.ERR_UNKNOWN_TENSOR_TYPE == s2.value
    bound = bound_types(name, h)
    for with_scratch in (False, True):  # execute_st does not ask for the scratch
        if with_scratch:
            assert pc.ERR_SCRATCH_NOT_ALLOCED == L.libxsmm_dnn_pooling_bind_scratch(handle, None)
            scratch = np.zeros(int(meta[2]), dtype=np.uint8)
            assert 0 == L.libxsmm_dnn_pooling_bind_scratch(handle, xs.dptr(scratch))
        for kind in (pc.FWD, pc.BWD, pc.UPD, pc.BWDUPD, pc.ALL):
            want = h.execute_status(kind, bound)
            if int(meta[META_EXEC + kind]) >= 0:
                assert want == int(meta[META_EXEC + kind])
            if 0 != want:  # (a pass that would run needs a device)
                assert want == xs.pool_execute(handle, kind), kind
            if kind in (pc.FWD, pc.BWD) and want in (0, pc.ERR_UNSUPPORTED_DATATYPE) or (want == pc.ERR_GENERAL):
                assert pc.ERR_GENERAL == xs.pool_execute(handle, kind, 3, 2)  # a negative logical thread
    assert 0 == L.libxsmm_dnn_pooling_release_scratch(handle)
    if pc.REG_IN in tensors and pc.REG_IN in bound:
        assert 0 == L.libxsmm_dnn_pooling_release_tensor(handle, pc.REG_IN)
        assert not L.libxsmm_dnn_pooling_get_tensor(handle, pc.REG_IN, C.byref(s2))
        if d["buffer_format"] == pc.FMT_LIBXSMM:
            assert pc.ERR_DATA_NOT_BOUND == xs.pool_execute(handle, pc.FWD)
    for t in tensors.values():
        L.libxsmm_dnn_destroy_tensor(t)
    assert 0 == L.libxsmm_dnn_destroy_pooling(handle)
    assert pc.ERR_INVALID_HANDLE == L.libxsmm_dnn_destroy_pooling(None) == xs.pool_execute(None, pc.FWD)


def test_statuses_of_this_engine_alone(xs):
    """MAX with a 16-bit mask, a channel block below 16 (no output blocks), and the empty share that needs no device"""
    L = xs.lib()
    for name, want in (("e_mask_i16", pc.ERR_UNSUPPORTED_DATATYPE), ("e_c8", pc.ERR_DATA_NOT_BOUND)):
        d = pc.STATUS_CASES[name]
        handle, status = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
        assert handle and 0 == status
        h = pc.Handle(d)
        keep = []
        for t in pc.BINDABLE:
            _, l = h.layout(t)
            buf = np.zeros(max(pc.layout_size(l)[0], 16), dtype=np.uint8)
            keep.append((buf, xs.pool_bind_new(handle, t, buf)))
        assert h.execute_status(pc.FWD, pc.BINDABLE) == xs.pool_execute(handle, pc.FWD) == xs.pool_execute(handle, pc.BWD)
        assert xs.pool_execute(handle, pc.FWD) == (want if name == "e_mask_i16" else pc.ERR_GENERAL)
        for _, t in keep:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_pooling(handle)
    d = pc.desc(threads=3, pool=pc.AVG, **pc.SHAPES["c"])
    handle, _ = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
    h = pc.Handle(d)
    assert [h.share(t) for t in range(3)] == [(0, 2), (2, 4), (4, 4)]
    bufs = [np.zeros(pc.layout_size(h.layout(t)[1])[0], dtype=np.uint8) for t in (pc.REG_IN, pc.REG_OUT)]
    tensors = [xs.pool_bind_new(handle, t, b) for t, b in zip((pc.REG_IN, pc.REG_OUT), bufs)]
    assert 0 == xs.pool_execute(handle, pc.FWD, 0, 2) == xs.pool_execute(handle, pc.FWD, 2, 4) == xs.pool_execute(handle, pc.FWD, 0, 7)
    for t in tensors:
        L.libxsmm_dnn_destroy_tensor(t)
    L.libxsmm_dnn_destroy_pooling(handle)
