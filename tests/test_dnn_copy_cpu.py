"""libxsmm_dnn_copyin_tensor / _copyout_tensor without a device (include/libxsmm_dnn_tensor.h, libxsmm_amd.h): the numpy restatement
of tests/dnn_copy_common.py against the reference's bytes, the host loop on every layout of the GPU tests, channel tensors, the
statuses and their order, the launch plan of libxsmm_amd_dnn_copy_plan, its clamps against the source, and the async forms'
refusal. Every buffer lies between canaries; comparisons are bitwise."""
import ctypes as C
import os

import numpy as np
import pytest

import dnn_copy_common as dc
import launch_limits as ll

PLAN = "kernels/dnn_copy_plan.h"
KERNELS = "kernels/dnn_copy.hip"
# the clamps of the copy's launches, in the manner of tests/launch_limits.py (ll.check holds them against the sources)
LIMITS = {
    # tiles through LDS: a work-group per tile and trip
    "dnn_copy_tiled": dict(derive=lambda v: v[0], unit="tiles", per_trip=2048, source=[
        (PLAN, r"constexpr int DNN_COPY_MAX_BLOCKS = (\d+);", 2048),
        (PLAN, r"g\.grid = \(int\)\(g\.items < DNN_COPY_MAX_BLOCKS \? g\.items : DNN_COPY_MAX_BLOCKS\);", None),
        (PLAN, r"g\.items = g\.blocks \* g\.jpasses \* g\.ltiles;", None),
        (KERNELS, r"for \(long long item = blockIdx\.x; item < g\.items; item \+= gridDim\.x\)", None)]),
    # the same order on both sides: 16 bytes per lane and trip
    "dnn_copy_flat": dict(derive=lambda v: v[0] * v[1] * v[2], unit="bytes", per_trip=2048 * 256 * 16, source=[
        (PLAN, r"constexpr int DNN_COPY_MAX_BLOCKS = (\d+);", 2048), (PLAN, r"constexpr int DNN_COPY_THREADS = (\d+);", 256),
        (KERNELS, r"template<typename T> struct alignas\(16\) Pack \{ T e\[(\d+) / sizeof\(T\)\]; \};", 16),
        (PLAN, r"wg > DNN_COPY_MAX_BLOCKS \? DNN_COPY_MAX_BLOCKS : wg", None),
        (KERNELS, r"for \(long long q = tid; q < units; q \+= nthreads\)", None)]),
    # a row beyond the LDS budget: an element per lane and trip
    "dnn_copy_direct": dict(derive=lambda v: v[0] * v[1], unit="elements", per_trip=2048 * 256, source=[
        (PLAN, r"constexpr int DNN_COPY_MAX_BLOCKS = (\d+);", 2048), (PLAN, r"constexpr int DNN_COPY_THREADS = (\d+);", 256),
        (PLAN, r"g\.items = \(g\.total \+ DNN_COPY_THREADS - 1\) / DNN_COPY_THREADS;", None),
        (KERNELS, r"i < g\.total; i \+= nthreads", None)]),
}
GEOMETRY = {
    "lds_budget": (PLAN, r"constexpr int DNN_COPY_LDS_BUDGET = (\d+);", 65536),
    "tile_bytes": (PLAN, r"constexpr int DNN_COPY_TILE_BYTES = (\d+);", 16384),
    "pix": (PLAN, r"constexpr int DNN_COPY_PIX = (\d+);", 64),
}
LDS_BUDGET, MAX_BLOCKS = 65536, 2048


@pytest.fixture(scope="module")
def golden_fc():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fc.npz"))


def host_tensor(xs, case, content=None):
    buf = dc.Guarded(None, case.nbytes, content=content)
    tensor, st = xs.dnn_link_tensor(case.layout, buf.ptr)
    assert tensor and 0 == st
    return buf, tensor


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_the_clamps_are_what_the_size_tests_assume(name):
    bad = ll.check(LIMITS[name])
    assert not bad, "\n".join([name] + bad)


def test_the_geometry_constants_are_what_the_tests_assume():
    for name, (path, pattern, value) in GEOMETRY.items():
        assert not ll.check(dict(derive=lambda v: v[0], per_trip=value, source=[(path, pattern, value)])), name
    assert LDS_BUDGET == GEOMETRY["lds_budget"][2] and MAX_BLOCKS == LIMITS["dnn_copy_tiled"]["per_trip"]


def test_the_restatement_equals_the_reference_bytes(xs, golden_fc):
    """tests/golden/fc.npz holds what the unmodified reference's copy-in and copy-out give for two FC layouts"""
    import fc_common as fc
    for name in ("l_5_32_48", "lb_5_32_48"):
        d = fc.COMPUTE_CASES[name]
        handle, _ = xs.fc_create(*[d[k] for k in fc.DESC_FIELDS])
        for t, key in ((fc.GRAD_IN, "x"), (fc.GRAD_FIL, "w")):
            layout, _ = xs.fc_layout(handle, t)
            fields = xs.dnn_layout_fields(layout)
            plain, blocked = golden_fc[name + "/cout_" + key], golden_fc[name + "/cin_" + key]
            assert np.array_equal(dc.copy_in(fields, plain), blocked.view(np.uint8).reshape(-1)), (name, key)
            assert np.array_equal(dc.copy_out(fields, blocked), plain.view(np.uint8).reshape(-1)), (name, key)
            xs.lib().libxsmm_dnn_destroy_tensor_datalayout(layout)
        xs.lib().libxsmm_dnn_destroy_fullyconnected(handle)


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_host_copies_are_the_restatement(xs, name):
    """both operands in pageable memory: the host loop (the only path without a device), nothing is launched"""
    L = xs.lib()
    case = dc.Case(xs, name)
    ts = dc.typesize(case.fields)
    plain = dc.Guarded(None, case.nbytes, content=dc.hostile_bytes(case.nbytes, 3, ts))
    buf, tensor = host_tensor(xs, case)
    launches = L.libxsmm_amd_launch_count()
    assert 0 == L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, case.fmt)
    want = dc.copy_in(case.fields, plain.payload())
    assert np.array_equal(buf.payload(), want)
    if name in dc.CHANNELS:
        assert np.array_equal(want, plain.payload())  # the identity
    back = dc.Guarded(None, case.nbytes)
    assert 0 == L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, case.fmt)
    assert np.array_equal(back.payload(), plain.payload()) and np.array_equal(back.payload(), dc.copy_out(case.fields, want))
    assert launches == L.libxsmm_amd_launch_count()
    L.libxsmm_dnn_destroy_tensor(tensor)
    case.close()


def test_channel_layouts_are_the_handles_own(xs):
    sizes = {name: dc.elements(dc.Case(xs, name).fields) for name in dc.CHANNELS}
    assert 40 == sizes["bias_k40"]
    assert all(0 < sizes[name] <= 24 for name in sizes if name.startswith("bn_"))  # (the reference's blocking of C = 24: one block of 16)


def edited(xs, case, **changes):
    """a tensor on a copy of the case's layout with fields changed"""
    L = xs.lib()
    st = C.c_uint()
    copy = L.libxsmm_dnn_duplicate_tensor_datalayout(case.layout, C.byref(st))
    for key, value in changes.items():
        setattr(copy.contents, key, value)
    buf = dc.Guarded(None, case.nbytes)
    tensor, st = xs.dnn_link_tensor(copy, buf.ptr)
    assert tensor
    return copy, buf, tensor


def statuses(xs, tensor, layout, ptr, fmt):
    """(copy-in, copy-out, async copy-in, async copy-out, plan in, plan out)"""
    L = xs.lib()
    return (L.libxsmm_dnn_copyin_tensor(tensor, ptr, fmt), L.libxsmm_dnn_copyout_tensor(tensor, ptr, fmt),
            L.libxsmm_amd_dnn_copyin_tensor_async(tensor, ptr, fmt), L.libxsmm_amd_dnn_copyout_tensor_async(tensor, ptr, fmt),
            xs.dnn_copy_plan(layout, fmt, True)[0], xs.dnn_copy_plan(layout, fmt, False)[0])


@pytest.mark.parametrize("name", ("bias_k40", "bn_gamma", "act_conv_c24_7x9", "fil_c24_k40_3x3"))
def test_statuses_and_their_order(xs, name):
    """the reference's order (src/libxsmm_dnn.c:1206-1362, :1407-1570): plain format, blocked, data type; then what is not provided.
    Nothing is written by a refused call; the plan answers what the copy answers."""
    L = xs.lib()
    case = dc.Case(xs, name)
    other = dc.Guarded(None, case.nbytes, content=dc.hostile_bytes(case.nbytes, 5))
    pair = lambda a, b: (a, b, a, b, a, b)  # noqa: E731
    bad_plain = pair(dc.ERR_UNSUPPORTED_SRC_FORMAT, dc.ERR_UNSUPPORTED_DST_FORMAT)
    bad_tensor = pair(dc.ERR_UNSUPPORTED_DST_FORMAT, dc.ERR_UNSUPPORTED_SRC_FORMAT)
    wrong_fmt = dc.FMT_KCRS if case.fmt == dc.FMT_NCHW else dc.FMT_NCHW
    checks = [
        (dict(format=dc.FMT_NHWC, datatype=dc.I32), wrong_fmt, bad_plain),                 # the plain format comes first
        (dict(), dc.FMT_NHWC, bad_plain),
        (dict(format=dc.FMT_NHWC, datatype=dc.I32), case.fmt, bad_tensor),               # then a tensor that is not blocked
        (dict(datatype=dc.I32, custom_format=2, num_dims=1), case.fmt, pair(dc.ERR_UNSUPPORTED_DATATYPE, dc.ERR_UNSUPPORTED_DATATYPE)),  # then the type
        (dict(datatype=5), case.fmt, pair(dc.ERR_UNSUPPORTED_DATATYPE, dc.ERR_UNSUPPORTED_DATATYPE)),  # I16
        (dict(tensor_type=31), case.fmt, pair(dc.ERR_INVALID_TENSOR, dc.ERR_INVALID_TENSOR)),          # POOLING_MASK: not a type of the switch
    ]
    if name not in dc.CHANNELS:
        checks += [(dict(custom_format=2, num_dims=1), case.fmt, pair(dc.ERR_NOT_IMPLEMENTED, dc.ERR_NOT_IMPLEMENTED)),
                   (dict(num_dims=case.fields[0] - 2), case.fmt, pair(dc.ERR_INVALID_LAYOUT, dc.ERR_INVALID_LAYOUT))]
    else:
        checks += [(dict(num_dims=1), case.fmt, pair(dc.ERR_INVALID_LAYOUT, dc.ERR_INVALID_LAYOUT))]
    for changes, fmt, want in checks:
        copy, buf, tensor = edited(xs, case, **changes)
        assert want == statuses(xs, tensor, copy, other.ptr, fmt), (changes, fmt)
        assert np.all(buf.payload() == 0x3C) and np.array_equal(other.payload(), dc.hostile_bytes(case.nbytes, 5))
        L.libxsmm_dnn_destroy_tensor(tensor)
        L.libxsmm_dnn_destroy_tensor_datalayout(copy)
    # NULL data: after the layout's checks
    buf, tensor = host_tensor(xs, case)
    assert dc.ERR_INVALID_TENSOR == L.libxsmm_dnn_copyin_tensor(tensor, None, case.fmt) == L.libxsmm_dnn_copyout_tensor(tensor, None, case.fmt)
    assert dc.ERR_INVALID_TENSOR == L.libxsmm_amd_dnn_copyin_tensor_async(tensor, None, case.fmt) == L.libxsmm_amd_dnn_copyout_tensor_async(tensor, None, case.fmt)
    assert dc.ERR_UNSUPPORTED_SRC_FORMAT == L.libxsmm_dnn_copyin_tensor(tensor, None, dc.FMT_RSCK)
    assert dc.ERR_INVALID_TENSOR == L.libxsmm_dnn_copyin_tensor(None, other.ptr, case.fmt) == L.libxsmm_amd_dnn_copyout_tensor_async(None, other.ptr, case.fmt)
    L.libxsmm_dnn_destroy_tensor(tensor)
    # an empty tensor: success, nothing moves
    copy, buf, tensor = edited(xs, case)
    copy.contents.dim_size[0] = 0
    tensor2, _ = xs.dnn_link_tensor(copy, buf.ptr)
    launches = L.libxsmm_amd_launch_count()
    assert 0 == L.libxsmm_dnn_copyin_tensor(tensor2, other.ptr, case.fmt) == L.libxsmm_dnn_copyout_tensor(tensor2, other.ptr, case.fmt)
    assert 0 == L.libxsmm_amd_dnn_copyin_tensor_async(tensor2, other.ptr, case.fmt) == xs.dnn_copy_plan(copy, case.fmt)[0]
    assert launches == L.libxsmm_amd_launch_count() and np.all(buf.payload() == 0x3C)
    for t in (tensor, tensor2):
        L.libxsmm_dnn_destroy_tensor(t)
    L.libxsmm_dnn_destroy_tensor_datalayout(copy)
    case.close()


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_the_plan_of_every_layout(xs, name):
    case = dc.Case(xs, name)
    n, ts = dc.elements(case.fields), dc.typesize(case.fields)
    for copy_in in (True, False):
        st, plan = xs.dnn_copy_plan(case.layout, case.fmt, copy_in)
        assert 0 == st
        form, bytes_, blocks, rows, run, held, items, groups = plan
        assert bytes_ == ts and blocks * rows * run == n
        assert 0 <= held <= rows and held * run * bytes_ <= LDS_BUDGET
        assert 1 <= groups <= MAX_BLOCKS and groups <= max(items, 1)
        sizes = case.fields[2]
        if name in dc.CHANNELS or name.startswith("act_fc"):
            assert (0, 1, 1, n, 0) == (form, blocks, rows, run, held)  # the same order on both sides: no LDS
        elif name in dc.ACTIVATIONS:
            lpb, bfm, W, H, fmb, N = ([1] + sizes) if 5 == len(sizes) else sizes
            assert (1, N * fmb, bfm * lpb, H * W, bfm * lpb) == (form, blocks, rows, run, held)
        else:
            lpb, bofm, bifm, S, R, ifmb, ofmb = ([1] + sizes) if 6 == len(sizes) else sizes
            assert (2, ofmb * ifmb, bofm, bifm * lpb * R * S) == (form, blocks, rows, run)
            assert (held < rows) == (name == "fil_c16_k16_11x11")  # 123 904 bytes per block: cut along its rows
            assert items == blocks * -(-rows // held)
    case.close()


def test_the_plan_of_other_blocks(xs):
    """layouts with extents no handle here returns: an FC filter of 64 x 64 blocks is not cut; a row beyond the LDS budget goes
    without LDS; a wide channel block is cut along its rows and its run"""
    L = xs.lib()
    fil, act = dc.Case(xs, "fil_fc_f32"), dc.Case(xs, "act_8x8")
    for case, sizes, want in ((fil, [64, 64, 1, 1, 2, 2], (2, 4, 4, 64, 64, 64, 4, 4)),
                              (fil, [2, 64, 17, 17, 2, 1], (2, 4, 2, 2, 64 * 289, 0, -(-2 * 2 * 64 * 289 // 256), 289)),
                              (act, [300, 9, 9, 1, 1], (1, 4, 1, 300, 81, 227, 4, 4))):
        layout = dc.resized(xs, case.layout, sizes)
        assert (0, list(want)) == xs.dnn_copy_plan(layout, case.fmt)
        L.libxsmm_dnn_destroy_tensor_datalayout(layout)
    fil.close()
    act.close()


def test_block_sizes_of_the_plan_cases_are_the_librarys(xs):
    want = {"act_conv_c24_7x9": [8, 9, 7, 3, 2], "act_conv_c3": [3, 7, 5, 1, 2], "act_8x8": [16, 8, 8, 1, 2], "act_5x13": [16, 13, 5, 1, 2],
            "fil_c16_k18_1x1": [2, 16, 1, 1, 1, 9], "fil_c16_k16_11x11": [16, 16, 11, 11, 1, 1], "fil_fc_f32": [16, 16, 1, 1, 2, 3]}
    for name, sizes in want.items():
        case = dc.Case(xs, name)
        assert sizes == case.fields[2], name
        case.close()
    bf = dc.Case(xs, "fil_fc_bf16")
    assert 7 == bf.fields[0] and [1, 16, 16, 1, 1, 2, 3] == bf.fields[2]  # (a 7-dimensional layout; its lpb is 1)
    bf.close()
    lp = dc.Case(xs, "act_bn_bf16_6x6")
    assert [2, 8, 6, 6, 2, 2] == lp.fields[2]  # lpb = 2
    lp.close()


def test_async_forms_need_memory_the_gpu_reaches(xs):
    """without a device (or with pageable operands on a machine that has one) the async forms answer ERR_GENERAL once the reference's
    own checks have passed, write nothing and launch nothing"""
    L = xs.lib()
    for name in ("act_8x8", "fil_c24_k40_3x3", "bias_k40"):
        case = dc.Case(xs, name)
        plain = dc.Guarded(None, case.nbytes, content=dc.hostile_bytes(case.nbytes, 9))
        buf, tensor = host_tensor(xs, case)
        launches = L.libxsmm_amd_launch_count()
        assert dc.ERR_GENERAL == L.libxsmm_amd_dnn_copyin_tensor_async(tensor, plain.ptr, case.fmt)
        assert dc.ERR_GENERAL == L.libxsmm_amd_dnn_copyout_tensor_async(tensor, plain.ptr, case.fmt)
        assert dc.ERR_UNSUPPORTED_SRC_FORMAT == L.libxsmm_amd_dnn_copyin_tensor_async(tensor, plain.ptr, dc.FMT_NHWC)  # the checks come first
        assert launches == L.libxsmm_amd_launch_count()
        assert np.all(buf.payload() == 0x3C) and np.array_equal(plain.payload(), dc.hostile_bytes(case.nbytes, 9))
        L.libxsmm_dnn_destroy_tensor(tensor)
        case.close()
