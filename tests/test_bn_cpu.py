"""The fused batch-norm layer without a GPU: the header as C89 and C++, the exported symbols, the numpy restatement
(tests/bn_common.py) against what the reference returned (tests/golden/bn.npz, captured by tools/golden/bn_capture.* with
LIBXSMM_TARGET=hsw and threads = 1), and the built library's host-side functions against the same values.

The reference ran with its scratch bound: without one it answers ERR_DATA_NOT_BOUND for OPS_BN, where this engine does not ask
for the scratch (include/libxsmm_dnn_fusedbatchnorm.h, "ours alone" 1)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bn_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META_LAYOUT, META_EXEC = 10, 480
INPUTS = ("x", "add", "dout", "gamma", "beta", "mean", "rstd", "dgamma", "dbeta")
OUTPUTS = ("out", "mean", "rstd", "var", "din", "dadd", "dout", "dgamma", "dbeta")
SYMBOLS = ("libxsmm_dnn_create_fusedbatchnorm", "libxsmm_dnn_destroy_fusedbatchnorm", "libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout",
           "libxsmm_dnn_fusedbatchnorm_get_scratch_size", "libxsmm_dnn_fusedbatchnorm_bind_scratch", "libxsmm_dnn_fusedbatchnorm_release_scratch",
           "libxsmm_dnn_fusedbatchnorm_bind_tensor", "libxsmm_dnn_fusedbatchnorm_get_tensor", "libxsmm_dnn_fusedbatchnorm_release_tensor",
           "libxsmm_dnn_fusedbatchnorm_execute_st")
CASES = sorted(bc.captured_cases())
WITH_OUTPUTS = [n for n in CASES if n not in bc.STATUS_CASES]


@pytest.fixture(scope="module")
def golden():
    return bc.load_golden()


def meta_layout(meta, i):
    m = meta[META_LAYOUT + 26 * i:META_LAYOUT + 26 * (i + 1)]
    if m[1] < 0:
        return int(m[0]), None
    n = int(m[1])
    return int(m[0]), dict(num_dims=n, dim_type=[int(v) for v in m[2:2 + n]], dim_size=[int(v) for v in m[10:10 + n]], datatype=int(m[18]), format=int(m[19]),
                           custom_format=int(m[20]), tensor_type=int(m[21]), size=int(m[22]), elements=int(m[23]), link=int(m[24]), bind=int(m[25]))


def bound_types(name, h):
    return [t for t in bc.BINDABLE if h.layout(t)[1] is not None and t not in bc.UNBOUND.get(name, ())]


@pytest.mark.parametrize("std", ("c89", "c++11"))
def test_header_compiles(tmp_path, std):
    cxx = std.startswith("c++")
    src = tmp_path / ("t.cpp" if cxx else "t.c")
    src.write_text("#include <libxsmm_dnn_fusedbatchnorm.h>\nint main(void) { libxsmm_dnn_fusedbatchnorm_desc d; d.fuse_ops = LIBXSMM_DNN_FUSEDBN_OPS_BN_ELTWISE_RELU; "
                   "d.fuse_order = LIBXSMM_DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU; return 13 == (int)d.fuse_ops && LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_ELTWISE_RELU == 14 "
                   "&& LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_RELU == 10 && LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE_ELTWISE == 6 && LIBXSMM_DNN_FUSEDBN_OPS_BN_RELU == 9 "
                   "&& LIBXSMM_DNN_FUSEDBN_OPS_BN_ELTWISE == 5 && LIBXSMM_DNN_FUSEDBN_OPS_BN == 1 && LIBXSMM_DNN_FUSEDBN_OPS_BNSCALE == 2 "
                   "&& LIBXSMM_DNN_FUSEDBN_OPS_ELTWISE == 4 && LIBXSMM_DNN_FUSEDBN_OPS_RELU == 8 && LIBXSMM_DNN_CHANNEL_VARIANCE == 25 "
                   "&& (int)sizeof(d) == 68 ? 0 : 1; }\n")
    subprocess.run(["g++" if cxx else "gcc", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_symbols_are_exported(xs):
    L = xs.lib()
    for name in SYMBOLS:
        assert getattr(L, name)
    for name in ("bn_create", "bn_layout", "bn_bind_new", "bn_execute"):
        assert callable(getattr(xs, name))
    assert C.sizeof(xs.FusedBatchnormDesc) == 68 and [f[0] for f in xs.FusedBatchnormDesc._fields_] == list(bc.DESC_FIELDS)


def test_the_golden_file_holds_the_cases(golden):
    assert os.path.getsize(os.path.join(bc.GOLDEN, "bn.npz")) <= os.path.getsize(os.path.join(bc.GOLDEN, "pool.npz"))
    for name, d in bc.captured_cases().items():
        assert list(golden[name + "/desc"]) == [d[k] for k in bc.DESC_FIELDS]
        assert d["H"] % d["u"] == 0 and d["W"] % d["v"] == 0 and d["threads"] == 1
    assert set(n for n in bc.captured_cases() if n + "/crc" in golden) == set(WITH_OUTPUTS)
    # every fuse combination in both element types, and the shapes the cases are for
    for dt in ("f32", "bf16"):
        assert [bc.COMPUTE_CASES["fuse%d_%s_n" % (ops, dt)]["fuse_ops"] for ops in bc.FUSE_COMBINATIONS] == list(bc.FUSE_COMBINATIONS)
    h = bc.Handle(bc.COMPUTE_CASES["c24_f32_n"])
    assert (h.blocksifm, h.blocksofm, h.runnable()) == (1, 1, True)
    h = bc.Handle(bc.STATUS_CASES["e_c8"])
    assert (h.blocksifm, h.blocksofm, h.runnable()) == (1, 0, False)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_statuses(golden, name):
    d = bc.captured_cases()[name]
    meta = golden[name + "/meta"]
    h = bc.Handle(d)
    assert (h.status, int(h.ok)) == (int(meta[0]), int(meta[1]))
    if not h.ok:
        return
    assert (h.scratch(), 0) == (int(meta[2]), int(meta[3]))
    assert [int(v) for v in meta[4:7]] == [bc.ERR_SCRATCH_NOT_ALLOCED, 0, 0]
    assert int(meta[8]) == bc.ERR_INVALID_HANDLE_TENSOR
    for i, t in enumerate(bc.LAYOUT_TYPES):
        status, ref = meta_layout(meta, i)
        st, mine = h.layout(t)
        assert st == status and (mine is None) == (ref is None), t
        if mine is None:
            continue
        assert mine == {k: ref[k] for k in mine}
        assert bc.layout_size(mine) == (ref["size"], ref["elements"])
        if t in bc.BINDABLE:
            assert (ref["link"], ref["bind"]) == (0, -1 if t in bc.UNBOUND.get(name, ()) else 0)
    if h.layout(bc.REG_IN)[1] is not None:
        assert [int(meta[7]), int(meta[9])] == [bc.ERR_UNKNOWN_TENSOR_TYPE] * 2
    bound = bound_types(name, h)
    for kind in (bc.FWD, bc.BWD, bc.UPD, bc.BWDUPD, bc.ALL):
        if int(meta[META_EXEC + kind]) >= 0:  # (-1: the reference was not run -- NO_RUN, or BWD of a FWD-only case)
            assert h.execute_status(kind, bound) == int(meta[META_EXEC + kind]), kind
    assert (name in bc.NO_RUN) == (int(meta[META_EXEC]) < 0)
    assert (name in bc.SPECIAL_CASES) == (int(meta[META_EXEC]) == 0 and int(meta[META_EXEC + 1]) < 0)


def test_every_row_of_the_check_order_is_captured(golden):
    """each status execute_st can answer before it computes was returned by the reference in some case"""
    seen = set()
    for name in bc.STATUS_CASES:
        seen.update(int(v) for v in golden[name + "/meta"][META_EXEC:META_EXEC + 5])
    assert seen >= {bc.SUCCESS, bc.ERR_INVALID_KIND, bc.ERR_INVALID_FORMAT_FUSEDBN, bc.ERR_DATA_NOT_BOUND, bc.ERR_FUSEBN_UNSUPPORTED_ORDER,
                    bc.ERR_FUSEBN_UNSUPPORTED_FUSION}
    assert int(golden["e_un_order/meta"][META_EXEC]) == bc.ERR_DATA_NOT_BOUND and int(golden["e_un_var/meta"][META_EXEC]) == bc.ERR_DATA_NOT_BOUND
    assert int(golden["e_un_regadd_noelt/meta"][META_EXEC]) == 0 == int(golden["e_un_gradadd_noelt/meta"][META_EXEC + 1])


@pytest.mark.parametrize("name", WITH_OUTPUTS)
def test_restatement_reproduces_the_reference_outputs(golden, name):
    """bit for bit, every case that has outputs: each multiply and add its own rounding, rstd through double precision"""
    d = bc.captured_cases()[name]
    bwd = name not in bc.SPECIAL_CASES
    e = bc.expected(name, d, bwd=bwd)
    crcs = golden[name + "/crc"]
    seeded = bc.inputs(name, d)
    for i, key in enumerate(INPUTS):
        assert (bc.crc(seeded[key]) if key in seeded else -1) == int(crcs[i]), "the seeded inputs changed: " + key
    keys = bc.written(d, bc.FWD) + (bc.written(d, bc.BWD) if bwd else [])
    assert [k for k in OUTPUTS if crcs[len(INPUTS) + OUTPUTS.index(k)] >= 0] == [k for k in OUTPUTS if k in keys]
    for key in keys:
        assert bc.crc(e[key]) == int(crcs[len(INPUTS) + OUTPUTS.index(key)]), key
        if name + "/" + key in golden:
            assert golden[name + "/" + key].tobytes() == e[key].tobytes(), key
        else:
            assert e[key].size > 8192


def test_the_cases_hold_what_they_are_for():
    e = bc.expected("zeros_f32_t", bc.COMPUTE_CASES["zeros_f32_t"])
    out = e["out"]
    assert np.all(out[..., 5].view(np.uint32) == 0x80000000), "-0.0 passes the RELU"
    assert np.sum(out.view(np.uint32) == 0) > 50, "the RELU leaves exact zeros"
    assert np.all(e["dout"][..., 5].view(np.uint32) == 0) and np.any(e["dout_in"][..., 5] != 0), "a -0.0 output counts as zero in BWD"
    assert e["dout"].tobytes() != e["dout_in"].tobytes()
    e = bc.expected("const_f32_c", bc.COMPUTE_CASES["const_f32_c"])
    assert np.all(np.abs(e["var"][:, [3, 9]]) < 1e-2) and np.all(np.isfinite(e["rstd"]))
    e = bc.expected("one_f32_n", bc.COMPUTE_CASES["one_f32_n"])
    assert np.all(np.abs(e["var"]) < 1e-6) and np.all(e["rstd"] > 1e3)
    for dt in ("f32", "bf16"):
        name = "nonfinite_" + dt
        e = bc.expected(name, bc.SPECIAL_CASES[name], bwd=False)
        h = bc.Handle(bc.SPECIAL_CASES[name])
        out = bc.as_f32(h, e["out"])
        assert np.isnan(e["mean"][0, 2]) and np.isinf(e["mean"][0, 7]) and np.all(np.isnan(e["var"][0, [2, 7]]))
        assert np.all(np.isfinite(np.delete(e["mean"][0], [2, 7])))
        assert np.all(np.isfinite(np.delete(out, [2, 7], axis=3))), "the other lanes of the pixel are untouched"
    e = bc.expected("stride_bn_f32_n", bc.COMPUTE_CASES["stride_bn_f32_n"])
    din = e["din"].view(np.uint32)
    assert np.all(din[:, 1::2, :, :] == 0xffffffff) and np.all(din[:, :, 1::2, :] == 0xffffffff) and not np.any(din[:, ::2, ::2, :] == 0xffffffff)


def test_fused_or_separate_is_decided_by_the_capture(golden):
    """the reference's build has no fused multiply-add: sumsq += x * x and ... * rstd + beta as one rounding each give other
    bits than the capture, in var and in the output. Read off the fp32 cases: in bf16 x * x is exact in fp32 (8 by 8 bits) and the
    truncation of the output hides a last bit, so those cases cannot tell."""
    for name in ("fuse1_f32_n", "pad_f32_n", "chunk_f32_n", "images_f32_n"):
        d = bc.COMPUTE_CASES[name]
        crcs = golden[name + "/crc"]
        fused = bc.expected(name, d, fused=True, bwd=False)
        separate = bc.expected(name, d, bwd=False)
        for key in ("var", "out"):
            want = int(crcs[len(INPUTS) + OUTPUTS.index(key)])
            assert bc.crc(separate[key]) == want and bc.crc(fused[key]) != want, (name, key)


def bind_all(xs, handle, h, name, keep):
    """every bindable type that has a layout, on host buffers of zeros; returns {type: tensor}"""
    tensors = {}
    for t in bound_types(name, h):
        buf = np.zeros(max(bc.layout_size(h.layout(t)[1])[0], 16), dtype=np.uint8)
        keep.append(buf)
        tensors[t] = xs.bn_bind_new(handle, t, buf)
    return tensors


@pytest.mark.parametrize("name", CASES)
def test_library_host_side_matches_the_reference(xs, golden, name):
    """create, layouts, sizes, scratch, bind and the statuses execute_st gives before it needs a device"""
    L = xs.lib()
    d = bc.captured_cases()[name]
    meta = golden[name + "/meta"]
    h = bc.Handle(d)
    handle, status = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
    assert (status, int(bool(handle))) == (int(meta[0]), int(meta[1]))
    if not handle:
        return
    st = C.c_uint(7)
    assert L.libxsmm_dnn_fusedbatchnorm_get_scratch_size(handle, C.byref(st)) == int(meta[2]) and 0 == st.value
    tensors, keep = {}, []
    for i, t in enumerate(bc.LAYOUT_TYPES):
        status, ref = meta_layout(meta, i)
        layout, st = xs.bn_layout(handle, t)
        assert st == status and (layout is None) == (ref is None)
        if layout is None:
            continue
        fields = xs.dnn_layout_fields(layout)
        assert fields == (ref["num_dims"], ref["dim_type"], ref["dim_size"], ref["datatype"], ref["format"], ref["custom_format"], ref["tensor_type"])
        s2 = C.c_uint(7)
        assert L.libxsmm_dnn_get_tensor_size(layout, C.byref(s2)) == ref["size"] and L.libxsmm_dnn_get_tensor_elements(layout, C.byref(s2)) == ref["elements"]
        if t in bc.BINDABLE:
            buf = np.zeros(ref["size"] + 16, dtype=np.uint8)
            keep.append(buf)
            tensor, st = xs.dnn_link_tensor(layout, buf)
            assert tensor and 0 == st
            copy = L.libxsmm_dnn_get_tensor_datalayout(tensor, C.byref(s2))
            copy.contents.dim_size[0] += 1
            wrong, st = xs.dnn_link_tensor(copy, buf)
            assert bc.ERR_MISMATCH_TENSOR == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, wrong, t)
            assert 0 == L.libxsmm_dnn_destroy_tensor(wrong) == L.libxsmm_dnn_destroy_tensor_datalayout(copy)
            if t not in bc.UNBOUND.get(name, ()):
                assert ref["bind"] == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, tensor, t) == 0
                assert L.libxsmm_dnn_fusedbatchnorm_get_tensor(handle, t, C.byref(s2)) == tensor and 0 == s2.value
            tensors[t] = tensor
        assert 0 == L.libxsmm_dnn_destroy_tensor_datalayout(layout)
    # the tensor type is looked at first, then the pointers
    assert bc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(None, None, bc.REG_FIL) == L.libxsmm_dnn_fusedbatchnorm_release_tensor(handle, bc.GEN_IN)
    assert bc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, None, bc.GEN_BETA)
    assert bc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, None, bc.REG_IN) == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(None, None, bc.VAR)
    assert bc.ERR_INVALID_HANDLE == L.libxsmm_dnn_fusedbatchnorm_release_tensor(None, bc.MEAN)
    s2 = C.c_uint(7)
    assert not L.libxsmm_dnn_fusedbatchnorm_get_tensor(handle, bc.REG_FIL, C.byref(s2)) and bc.ERR_UNKNOWN_TENSOR_TYPE == s2.value
    bound = bound_types(name, h)
    for with_scratch in (False, True):  # execute_st does not ask for the scratch
        if with_scratch:
            assert int(meta[4]) == bc.ERR_SCRATCH_NOT_ALLOCED == L.libxsmm_dnn_fusedbatchnorm_bind_scratch(handle, None)
            scratch = np.zeros(int(meta[2]), dtype=np.uint8)
            assert int(meta[5]) == 0 == L.libxsmm_dnn_fusedbatchnorm_bind_scratch(handle, xs.dptr(scratch))
        for kind in (bc.FWD, bc.BWD, bc.UPD, bc.BWDUPD, bc.ALL):
            want = h.execute_status(kind, bound)
            if int(meta[META_EXEC + kind]) >= 0:
                assert want == int(meta[META_EXEC + kind])
            if 0 != want:  # (a pass that would run needs a device)
                assert want == xs.bn_execute(handle, kind), kind
            if want in (0, bc.ERR_GENERAL):
                assert bc.ERR_GENERAL == xs.bn_execute(handle, kind, 3, 2)  # a negative logical thread
    assert int(meta[6]) == 0 == L.libxsmm_dnn_fusedbatchnorm_release_scratch(handle)
    if bc.REG_IN in tensors and bc.REG_IN in bound:
        assert 0 == L.libxsmm_dnn_fusedbatchnorm_release_tensor(handle, bc.REG_IN)
        assert not L.libxsmm_dnn_fusedbatchnorm_get_tensor(handle, bc.REG_IN, C.byref(s2))
        if d["buffer_format"] == bc.FMT_LIBXSMM:
            assert bc.ERR_DATA_NOT_BOUND == xs.bn_execute(handle, bc.FWD) == xs.bn_execute(handle, bc.BWD)
    for t in tensors.values():
        L.libxsmm_dnn_destroy_tensor(t)
    assert 0 == L.libxsmm_dnn_destroy_fusedbatchnorm(handle)
    assert bc.ERR_INVALID_HANDLE == L.libxsmm_dnn_destroy_fusedbatchnorm(None) == xs.bn_execute(None, bc.FWD)


def test_statuses_of_this_engine_alone(xs):
    """what execute_st refuses with ERR_GENERAL before it needs a device (none of it captured: the reference would write out of
    bounds, trap or walk past its tensors), and the empty share"""
    L = xs.lib()
    refused = {"c8": bc.desc(6, 4, C=8), "h_mod_u": bc.desc(6, 4, u=4), "w_mod_v": bc.desc(6, 4, v=3), "n0": bc.desc(6, 4, N=0), "h0": bc.desc(0, 4),
               "u0": bc.desc(6, 4, u=0), "v_neg": bc.desc(6, 4, v=-1), "pad_neg": bc.desc(6, 4, pin=(0, -1)), "pad_out_neg": bc.desc(6, 4, pout=(-1, 0)),
               "threads0": bc.desc(6, 4, threads=0), "plane": bc.desc(1 << 14, 1 << 13, N=1)}
    for name, d in refused.items():
        handle, status = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
        assert handle and 0 == status, name
        tensors = []
        for t in bc.BINDABLE:   # one small buffer serves: nothing is read before the refusal (and the layouts may be empty or huge)
            layout, st = xs.bn_layout(handle, t)
            assert layout is not None, (name, t)
            tensor, st = xs.dnn_link_tensor(layout, np.zeros(64, dtype=np.uint8))
            assert 0 == L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, tensor, t)
            L.libxsmm_dnn_destroy_tensor_datalayout(layout)
            tensors.append(tensor)
        assert bc.ERR_GENERAL == xs.bn_execute(handle, bc.FWD) == xs.bn_execute(handle, bc.BWD), name
        if name in ("c8", "h_mod_u", "w_mod_v", "plane"):
            assert bc.ERR_GENERAL == bc.Handle(d).execute_status(bc.FWD, bc.BINDABLE)
        for t in tensors:
            L.libxsmm_dnn_destroy_tensor(t)
        L.libxsmm_dnn_destroy_fusedbatchnorm(handle)
    d = bc.desc(6, 4, threads=3, ops=13)
    handle, _ = xs.bn_create(*[d[k] for k in bc.DESC_FIELDS])
    h = bc.Handle(d)
    assert [h.share(t) for t in range(4)] == [(0, 1), (1, 2), (2, 2), (2, 2)]
    keep = []
    tensors = bind_all(xs, handle, h, "", keep)
    for kind in (bc.FWD, bc.BWD):   # the empty share and a logical thread beyond desc.threads need no device
        assert 0 == xs.bn_execute(handle, kind, 0, 2) == xs.bn_execute(handle, kind, 2, 5) == xs.bn_execute(handle, kind, 0, 3) == xs.bn_execute(handle, kind, 0, 70)
        assert bc.ERR_GENERAL == xs.bn_execute(handle, kind, 1, 0)
    for t in tensors.values():
        L.libxsmm_dnn_destroy_tensor(t)
    L.libxsmm_dnn_destroy_fusedbatchnorm(handle)
