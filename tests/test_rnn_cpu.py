"""The RNN cell layer without a GPU: the restatement of tests/rnn_common.py against what the reference returned
(tests/golden/rnn.npz, written by tools/golden/rnn_capture.py from the unmodified reference under LIBXSMM_TARGET=hsw), the host side
of the product (handles, layouts, sizes, bind orders: every row of the capture), the finding about `dst += src0 * src1`, the
reduction blocking against a table read from the templates, the condition on the inputs that lets the GPU tests compare bits, and
the compilation of kernels/rnn.hip for gfx950."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import launch_limits as ll
import rnn_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (rc.FWD, rc.BWD, rc.UPD, rc.BWDUPD, rc.ALL, 5)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(rc.GOLDEN, "rnn.npz"))


def test_the_file_holds_the_cases_of_the_common_module(golden):
    for name, d in rc.captured_cases().items():
        assert list(golden[name + "/desc"]) == [d[k] for k in rc.DESC_FIELDS] + [d["seq"], d["seed"]]
        fb = golden[name + "/forget_bias"][0]
        assert (np.isnan(fb) and d["forget_bias"] is None) or fb == d["forget_bias"]
    assert os.path.getsize(os.path.join(rc.GOLDEN, "rnn.npz")) < 512 * 1024


@pytest.mark.parametrize("name", sorted(rc.COMPUTE_CASES) + sorted(rc.SPECIAL_CASES))
def test_restatement_equals_capture(golden, name):
    """bit for bit, every tensor the pass writes (a large one through its CRC-32); steps beyond the sequence length keep their fill"""
    d = rc.captured_cases()[name]
    t, out = rc.expected(name)
    crcs = golden[name + "/crc"]
    assert 0 == golden[name + "/meta"][704]
    for i, key in enumerate(rc.INPUTS):
        assert crcs[i] == (rc.crc(t[key]) if key in t else -1), "the inputs are not those of the capture"
    for key in rc.OUTPUTS:
        want = crcs[len(rc.INPUTS) + rc.OUTPUTS.index(key)]
        assert (key in out) == (want >= 0)
        if key not in out:
            continue
        if name + "/" + key in golden.files:
            got = golden[name + "/" + key].view(np.uint32)
            assert np.array_equal(out[key].reshape(-1).view(np.uint32), got), key
        assert rc.crc(out[key]) == want, key
        T = rc.Handle(d).T
        assert np.all(out[key][T:].view(np.uint32) == 0xffffffff) and not np.any(out[key][:T].view(np.uint32) == 0xffffffff)


@pytest.mark.parametrize("name", ("blk_lstm", "blk_gru", "k72_lstm", "seq_gru"))
def test_the_fused_form_gives_other_bits(golden, name):
    """`dst += src0 * src1` (eltwise_fma_ld) is a multiply and an add in the reference's build: the fused form misses the capture"""
    d = rc.COMPUTE_CASES[name]
    out = rc.forward(rc.Handle(d), rc.inputs(name, d), fused=True)
    key = "cs" if d["cell"] == rc.LSTM else "h"
    assert rc.crc(out[key]) != golden[name + "/crc"][len(rc.INPUTS) + rc.OUTPUTS.index(key)]


def layout_row(meta, i):
    m = meta[80 + 26 * i:106 + 26 * i]
    return m


@pytest.mark.parametrize("name", sorted(rc.captured_cases()))
def test_statuses_layouts_and_sizes(xs, golden, name):
    """every status, layout and size row of the capture, from the restatement's Handle and from the product's host side"""
    L = xs.lib()
    d = rc.captured_cases()[name]
    meta = golden[name + "/meta"]
    h = rc.Handle(d)
    st = C.c_uint(0xdead)
    desc = xs.RnncellDesc(d["threads"], d["K"], d["N"], d["C"], d["max_T"], d["bk"], d["bn"], d["bc"], d["cell"], d["datatype_in"], d["datatype_out"],
                          d["buffer_format"], d["filter_format"])
    handle = L.libxsmm_dnn_create_rnncell(desc, C.byref(st))
    assert meta[0] == h.status == st.value and meta[1] == int(h.ok) == int(bool(handle))
    assert meta[69] == rc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_rnncell_allocate_forget_bias(None, 1.0)
    (L.libxsmm_dnn_rnncell_get_sequence_length(None, C.byref(st)))
    assert meta[74] == rc.ERR_INVALID_HANDLE == st.value
    assert meta[75] == rc.ERR_INVALID_HANDLE == L.libxsmm_dnn_rnncell_set_sequence_length(None, 1)
    assert meta[79] == rc.ERR_INVALID_HANDLE == L.libxsmm_dnn_destroy_rnncell(None)
    if not h.ok:
        return
    for kind in KINDS:
        size = L.libxsmm_dnn_rnncell_get_scratch_size(handle, kind, C.byref(st))
        assert (meta[2 + 2 * kind], meta[3 + 2 * kind]) == h.scratch_size(kind) == (size, st.value), kind
        size = L.libxsmm_dnn_rnncell_get_internalstate_size(handle, kind, C.byref(st))
        assert (meta[14 + 2 * kind], meta[15 + 2 * kind]) == h.internalstate_size(kind) == (size, st.value), kind
    # layouts of the 23 types and of one the layer does not know; every tensor is linked and bound
    buf = np.zeros(int(max(meta[80 + 26 * i + 22] for i in range(24))) + 256, dtype=np.uint8)
    tensors = {}
    for i, t in enumerate(rc.RNN_TYPES + (0,)):
        m = layout_row(meta, i)
        want_st, want = h.layout(t)
        l, got_st = xs.rnn_layout(handle, t)
        assert m[0] == want_st == got_st, t
        assert (m[1] < 0) == (want is None) == (l is None)
        if want is None:
            continue
        n = int(m[1])
        fields = (n, list(m[2:2 + n]), list(m[10:10 + n]), int(m[18]), int(m[19]), int(m[20]), int(m[21]))
        assert fields == (want["num_dims"], want["dim_type"], want["dim_size"], want["datatype"], want["format"], want["custom_format"], want["tensor_type"])
        assert fields == xs.dnn_layout_fields(l), t
        assert (m[22], m[23]) == rc.layout_size(want)
        tensors[t], link = xs.dnn_link_tensor(l, buf)
        L.libxsmm_dnn_destroy_tensor_datalayout(l)
        assert m[24] == 0 == link and m[25] == 0 == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensors[t], t)
        assert tensors[t] == L.libxsmm_dnn_rnncell_get_tensor(handle, t, C.byref(st))
    # the orders of bind, get and release
    assert meta[62] == rc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_rnncell_bind_tensor(handle, None, rc.X)
    if rc.X in tensors:  # (a format without activation layouts has no tensor to try with)
        assert meta[63] == rc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensors[rc.X], 0)
        assert meta[64] == rc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_rnncell_bind_tensor(None, tensors[rc.X], rc.X)
        # (the input as the hidden state: a C dimension is no K dimension, whatever the sizes)
        assert meta[76] == rc.ERR_MISMATCH_TENSOR == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensors[rc.X], rc.H)
    else:
        assert meta[63] == meta[64] == meta[76] == -1
    assert meta[65] == rc.ERR_UNKNOWN_TENSOR_TYPE == L.libxsmm_dnn_rnncell_release_tensor(handle, 0)
    assert meta[66] == rc.ERR_INVALID_HANDLE_TENSOR == L.libxsmm_dnn_rnncell_release_tensor(None, rc.X)
    for hd, t in ((handle, 0), (None, rc.X)):  # get_tensor never writes the status
        st.value = 0xdead
        assert not L.libxsmm_dnn_rnncell_get_tensor(hd, t, C.byref(st))
        assert meta[67] == meta[68] == 0xdead == st.value
    scratch = np.zeros(256, dtype=np.uint8)
    base = scratch.ctypes.data + 4
    for kind in KINDS:
        assert meta[26 + kind] == h.bind_scratch(kind, True) == L.libxsmm_dnn_rnncell_bind_scratch(handle, kind, None), kind
        assert meta[32 + kind] == h.bind_scratch(kind, False) == L.libxsmm_dnn_rnncell_bind_scratch(handle, kind, C.c_void_p(base)), kind
        if kind != 5 and meta[32 + kind] == 0 and meta[2 + 2 * kind] > 0:
            assert meta[77] == 1 and base == L.libxsmm_dnn_rnncell_get_scratch_ptr(handle, C.byref(st))
        assert meta[38 + kind] == h.release(kind) == L.libxsmm_dnn_rnncell_release_scratch(handle, kind), kind
        assert meta[44 + kind] == h.bind_internalstate(kind, True) == L.libxsmm_dnn_rnncell_bind_internalstate(handle, kind, None), kind
        assert meta[50 + kind] == h.bind_internalstate(kind, False) == L.libxsmm_dnn_rnncell_bind_internalstate(handle, kind, C.c_void_p(base)), kind
        if kind != 5 and meta[14 + 2 * kind] > 0:
            assert meta[78] == 1 and (base + 63) // 64 * 64 == L.libxsmm_dnn_rnncell_get_internalstate_ptr(handle, C.byref(st))
        assert meta[56 + kind] == h.release(kind) == L.libxsmm_dnn_rnncell_release_internalstate(handle, kind), kind
    assert meta[70] == rc.ERR_RNN_INVALID_SEQ_LEN == L.libxsmm_dnn_rnncell_set_sequence_length(handle, d["max_T"] + 1)
    assert meta[71] == d["max_T"] == L.libxsmm_dnn_rnncell_get_sequence_length(handle, C.byref(st)) and meta[72] == 0 == st.value
    if d["seq"] >= 0:
        assert meta[73] == 0 == L.libxsmm_dnn_rnncell_set_sequence_length(handle, d["seq"])
        assert d["seq"] == L.libxsmm_dnn_rnncell_get_sequence_length(handle, C.byref(st))
    for t in tensors.values():
        L.libxsmm_dnn_destroy_tensor(t)
    assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)


def test_host_checks_answer_before_any_device_probe(xs):
    """this machine may have no GPU at all: every refusal of execute_st, and the call of a thread without a share, must answer"""
    L = xs.lib()
    assert rc.ERR_INVALID_HANDLE == xs.rnn_execute(None, rc.FWD)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    for cell in rc.CELLS:
        for change, status in ((dict(), None), (dict(buffer_format=rc.FMT_NCPACKED, filter_format=rc.FMT_CKPACKED), rc.ERR_INVALID_FORMAT_GENERAL),
                               (dict(filter_format=rc.FMT_CKPACKED), rc.ERR_INVALID_FORMAT_GENERAL)):
            d = dict(rc.desc(4, 8, 8, 2, cell, bn=2, bc=4, bk=4, threads=2), **change)
            handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], cell, d["bn"], d["bc"], d["bk"], d["threads"],
                                       buffer_format=d["buffer_format"], filter_format=d["filter_format"])
            assert handle and 0 == st
            for kind in (rc.BWD, rc.UPD, rc.BWDUPD, rc.ALL, 7):
                assert rc.ERR_INVALID_KIND == xs.rnn_execute(handle, kind)
            if status is not None:
                assert status == xs.rnn_execute(handle, rc.FWD)
                continue
            types = [rc.IN_TYPE.get(k, rc.OUT_TYPE.get(k)) for k in rc.read(cell) + rc.written(cell) if k != "z"]
            assert rc.ERR_DATA_NOT_BOUND == xs.rnn_execute(handle, rc.FWD)
            tensors = [xs.rnn_bind_new(handle, t, buf) for t in types]
            if cell in (rc.RELU, rc.SIGMOID, rc.TANH):
                assert rc.ERR_DATA_NOT_BOUND == xs.rnn_execute(handle, rc.FWD)  # z: the internal state
                assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, rc.FWD, xs.dptr(buf))
            for t in types:
                assert 0 == L.libxsmm_dnn_rnncell_release_tensor(handle, t)
                assert rc.ERR_DATA_NOT_BOUND == xs.rnn_execute(handle, rc.FWD), t
            for t, tensor in zip(types, tensors):
                assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensor, t)
            assert rc.ERR_GENERAL == xs.rnn_execute(handle, rc.FWD, 1, 0)                                # logical thread -1
            before = L.libxsmm_amd_launch_count()
            assert 0 == xs.rnn_execute(handle, rc.FWD, 0, 2) == xs.rnn_execute(handle, rc.FWD, 3, 40)  # beyond desc.threads: nothing to do
            assert 0 == L.libxsmm_dnn_rnncell_set_sequence_length(handle, 0)
            assert 0 == xs.rnn_execute(handle, rc.FWD)                                                    # no step: nothing to do
            assert before == L.libxsmm_amd_launch_count() and not buf.any()
            for tensor in tensors:
                L.libxsmm_dnn_destroy_tensor(tensor)
            assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)
    for change in (dict(N=0), dict(C=0), dict(K=0), dict(threads=0), dict(N=1 << 16, K=1 << 14, max_T=4)):
        d = dict(rc.desc(4, 8, 8, 2, rc.LSTM), **change)
        handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], rc.LSTM, threads=d["threads"])
        assert handle
        for t in (rc.IN_TYPE[k] for k in rc.read(rc.LSTM)):  # (bound to a small buffer: nothing is ever read)
            l, _ = xs.rnn_layout(handle, t)
            tensor, _ = xs.dnn_link_tensor(l, buf)
            assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensor, t)
            L.libxsmm_dnn_destroy_tensor_datalayout(l)
        for t in (rc.OUT_TYPE[k] for k in rc.written(rc.LSTM)):
            l, _ = xs.rnn_layout(handle, t)
            tensor, _ = xs.dnn_link_tensor(l, buf)
            assert 0 == L.libxsmm_dnn_rnncell_bind_tensor(handle, tensor, t)
            L.libxsmm_dnn_destroy_tensor_datalayout(l)
        assert rc.ERR_GENERAL == xs.rnn_execute(handle, rc.FWD), change


# The reduction blocking, read from the templates (lstm :156-176, gru :134-154, and which body walks which order): C, K in
# {1024, 1040, 2048, 2064} with bc = bk = 16, and the special case C == 2048 && K == 1024. Per (C, K): BF.
BF_TABLE = {(1024, 1024): 1, (1024, 1040): 1, (1024, 2048): 8, (1024, 2064): 1,
            (1040, 1024): 1, (1040, 1040): 5, (1040, 2048): 1, (1040, 2064): 1,
            (2048, 1024): 2, (2048, 1040): 1, (2048, 2048): 8, (2048, 2064): 1,
            (2064, 1024): 1, (2064, 1040): 1, (2064, 2048): 1, (2064, 2064): 3}


def test_segment_list_against_the_table(xs):
    for (Cc, K), bf in BF_TABLE.items():
        assert bf == rc.blocking_factor(Cc, K, Cc // 16, K // 16), (Cc, K)
        wl, rl = Cc // 16 // bf * 16, K // 16 // bf * 16
        alternating = [s for cb in range(bf) for s in ((0, cb * wl, wl), (1, cb * rl, rl))]
        plain = [(0, 0, bf * wl), (1, 0, bf * rl)]
        for cell in (rc.RELU, rc.SIGMOID, rc.TANH):
            assert [(0, 0, Cc), (1, 0, K)] == xs.rnn_segments(cell, Cc, K, 16, 16)              # no BF
        assert (alternating if (Cc, K) == (2048, 2048) else plain) == xs.rnn_segments(rc.LSTM, Cc, K, 16, 16)  # the fused body
        for phase in (0, 1):
            assert (alternating if bf > 1 else plain) == xs.rnn_segments(rc.GRU, Cc, K, 16, 16, phase)
    # 2064 = 129 blocks of 16 = 3 * 43: above 2048 the search starts at 16
    assert 3 == rc.blocking_factor(2064, 2064, 129, 129)
    # the forced BF = 2 with an odd block count (2048 and 1024 have no odd divisor but 1: it is always one block): no block per chunk,
    # so nothing of that operand is computed. The reference cannot be asked: it ends with a segmentation fault there
    # (rnn_common.UNCAPTURED_CASES), so this is the template's arithmetic taken at its word, not a captured behaviour
    assert [(1, 0, 1024)] == xs.rnn_segments(rc.LSTM, 2048, 1024, 2048, 512)
    assert [(0, 0, 2048)] == xs.rnn_segments(rc.LSTM, 2048, 1024, 512, 1024)
    assert [] == xs.rnn_segments(rc.LSTM, 30, 30, 7, 5)


def exact_distance_ulps(kind, arg, mid):
    """|exp(arg) or tanh(arg) - mid| in fp64 ulps of the value, to more than fp64 precision: mpmath if it is there, else long double"""
    try:
        import mpmath
        mpmath.mp.prec = 200
        exact = mpmath.exp(mpmath.mpf(arg)) if kind == "exp" else mpmath.tanh(mpmath.mpf(arg))
        ulp = mpmath.mpf(2) ** (int(mpmath.floor(mpmath.log(abs(exact), 2))) - 52)
        return float(abs(exact - mpmath.mpf(mid)) / ulp)
    except ImportError:
        x = np.longdouble(arg)
        exact = np.exp(x) if kind == "exp" else np.tanh(x)
        return float(abs(exact - np.longdouble(mid)) / np.longdouble(np.spacing(np.float64(exact))))


def test_no_transcendental_is_a_hard_case():
    """A condition on the inputs (met by choosing seeds), not a tolerance: of every exp and tanh evaluated in every captured, uncaptured,
    swept, threads and limit case (all steps of steps_tanh, the one period of the wide case), none lies within 64 fp64 ulps of a float rounding boundary (the midpoint of two neighbouring floats), so a
    device exp / tanh that differs from the host libm's by a few fp64 ulps still rounds to the same float. Flushed or saturated
    results (0, +-1, Inf) are exempt. All values are screened in float64 first (numpy's exp and tanh, good to an ulp or two: whatever
    lies within 1024 ulps of a boundary goes on); what is left is evaluated to more than fp64 precision."""
    cases = list(rc.GPU_COMPUTE_CASES.items()) + list(rc.SPECIAL_CASES.items()) + list(rc.SWEEP.items()) + list(rc.THREAD_CASES.items())
    cases += [("steps_tanh", None), ("manyrows_small", None), ("wide_relu", None)]
    count, worst = 0, (np.inf, None)
    for name, d in cases:
        log = []
        if name == "steps_tanh":    # all 65537 steps
            log = rc.limit_expected(name)[2]
        elif name == "manyrows_small":  # (a ReLU cell has none; the rows of manyrows_relu beyond these go the same way)
            d = dict(rc.LIMIT_CASES["manyrows_relu"], N=640, bn=320)
            rc.forward(rc.Handle(d), rc.inputs("manyrows_relu", d), log=log)
        elif name == "wide_relu":   # the one period of the wide case
            d = dict(rc.WIDE_CASE, N=rc.WIDE_PERIOD, threads=1)
            rc.forward(rc.Handle(d), rc.inputs(name, d), log=log)
        else:
            rc.forward(rc.Handle(dict(d, threads=1)), rc.inputs(name, d), log=log)
        for kind in ("exp", "tanh"):
            arg = np.array([a for k, a in log if k == kind], dtype=np.float64)
            count += arg.size
            with np.errstate(all="ignore"):
                v = np.exp(arg) if kind == "exp" else np.tanh(arg)
                f = v.astype(np.float32)
                live = np.isfinite(f) & (f != 0) & (np.abs(f) != 1) & np.isfinite(arg)
                arg, v, f = arg[live], v[live], f[live]
                f64 = f.astype(np.float64)
                mids = [(f64 + np.nextafter(f, np.float32(side)).astype(np.float64)) / 2 for side in (-np.inf, np.inf)]
                ulps = [np.abs(v - m) / np.spacing(np.abs(v)) for m in mids]
            for m, u in zip(mids, ulps):
                for idx in np.nonzero(u < 1024)[0]:
                    dist = exact_distance_ulps(kind, float(arg[idx]), float(m[idx]))
                    if dist < worst[0]:
                        worst = (dist, (name, kind, float(arg[idx])))
    assert count > 2000000
    assert worst[0] >= 64, worst


def tiles(n, tile):
    return (n + tile - 1) // tile


def test_the_limit_cases_are_what_they_are_for(xs, golden):
    """what each case past one tile, past a grid limit or near 2^31 is there for, from its descriptor and the constants the launch
    limits table reads out of the sources: an edit that shrinks a case out of its purpose fails here, without a GPU"""
    rows, steps = ll.THRESHOLDS["rnn_rows_per_share"], ll.LIMITS["rnn_steps"]
    assert not ll.check(rows) and not ll.check(steps)
    BT, BK, max_tiles, max_steps = rows["tile"], rows["chunk"], rows["tiles"], steps["per_trip"]
    for cell in rc.CELLS:
        d = rc.COMPUTE_CASES["rows_" + rc.CELL_NAMES[cell]]
        assert d["cell"] == cell and d["max_T"] >= 2
        for extent in (d["K"], d["N"]):                      # two tiles and more both ways, the last one partial
            assert tiles(extent, BT) >= 2 and extent % BT != 0
        assert d["C"] > BK and d["C"] % BK != 0 and d["K"] > BK and d["K"] % BK != 0   # whole chunks and a k tail in both reductions
        h = rc.Handle(d)
        assert h.status == rc.SUCCESS and (h.bn, h.bc, h.bk) == (d["bn"], d["bc"], d["bk"])
    for cell in (rc.TANH, rc.LSTM, rc.GRU):
        d = rc.THREAD_CASES["rowshares_" + rc.CELL_NAMES[cell]]
        shares = rc.Handle(d).shares()
        assert shares == [(0, 91), (91, 182), (182, 260)] and d["cell"] == cell
        assert all(n0 // BT != (n1 - 1) // BT and tiles(n1 - n0, BT) >= 2 for n0, n1 in shares) and sum(n0 % BT != 0 for n0, _ in shares) >= 2
    # the special rows: what was planted beyond the first tile stays in its row
    d = rc.SPECIAL_CASES["special_rows_lstm"]
    t, out = rc.expected("special_rows_lstm")
    (rn, cn), (ri, ci) = rc.SPECIAL_ROWS_PLANTED["nan"], rc.SPECIAL_ROWS_PLANTED["inf"]
    assert min(rn, ri) >= BT and min(cn, ci) >= 2 * BT and np.isnan(t["hp"][0, rn, cn]) and np.isposinf(t["hp"][0, ri, ci])
    poisoned = sorted(set(np.nonzero(~np.isfinite(t["x"]).all(axis=(0, 2)) | ~np.isfinite(t["hp"][0]).all(axis=1))[0]))
    assert poisoned == sorted([0, 1, 2, ri, rn])
    clean = np.setdiff1d(np.arange(d["N"]), poisoned)
    for key in rc.written(rc.LSTM):
        assert np.isfinite(out[key][:, clean]).all(), key
        assert np.isnan(out[key][0, rn]).all(), key             # every output of the row depends on the NaN (r has no zero)
    # the orders held by a capture
    d = rc.COMPUTE_CASES["odd_gru"]
    h = rc.Handle(d)
    bf = rc.blocking_factor(d["C"], d["K"], d["C"] // h.bc, d["K"] // h.bk)
    seg = xs.rnn_segments(rc.GRU, d["C"], d["K"], h.bc, h.bk)
    assert bf == 3 and len(seg) == 2 * bf and [s[0] for s in seg] == [0, 1] * bf
    assert all(s[2] % 2 == 1 and s[2] % BK != 0 and s[2] > BK for s in seg) and seg[0][2] == 351
    d = rc.COMPUTE_CASES["fused_lstm"]
    h = rc.Handle(d)
    seg = xs.rnn_segments(rc.LSTM, d["C"], d["K"], h.bc, h.bk)
    assert 8 == rc.blocking_factor(d["C"], d["K"], d["C"] // h.bc, d["K"] // h.bk) and [s[0] for s in seg] == [0, 1] * 8
    assert seg == [s for cb in range(8) for s in ((0, 256 * cb, 256), (1, 256 * cb, 256))]
    assert "fused_lstm/crc" in golden.files and "odd_gru/crc" in golden.files
    # no w segment at all, and the restatement agrees: x does not enter. The reference gave no capture (it faults)
    d = rc.UNCAPTURED_CASES["rem_lstm"]
    h = rc.Handle(d)
    assert h.status == rc.SUCCESS and [(1, 0, d["K"])] == xs.rnn_segments(rc.LSTM, d["C"], d["K"], h.bc, h.bk)
    assert not any(name.startswith("rem_lstm/") for name in golden.files)
    t, out = rc.expected("rem_lstm")
    other = rc.forward(h, dict(t, x=t["x"] * np.float32(-3) + np.float32(1)))
    assert all(rc.same_bits(other[key], out[key]) for key in out)
    # one pre-activation, naively in float64, where w.x would be largest: sigmoid^-1 of the i gate is b + r.h alone
    k0 = int(np.argmax(np.abs(t["x"].astype(np.float64)[0, 1] @ t["w"].astype(np.float64)[:, :d["K"]])))
    rk, h1 = t["r"].astype(np.float64)[:, k0], t["hp"].astype(np.float64)[0, 1]
    pre, mag = t["b"][k0] + rk @ h1, abs(t["b"][k0]) + np.abs(rk) @ np.abs(h1)
    assert abs(1 / (1 + np.exp(-pre)) - out["i"][0, 1, k0]) <= (d["K"] + 1) * 2.0 ** -24 * mag / 4 + 3 * 2.0 ** -24  # (as in the sweep)
    assert abs(t["w"].astype(np.float64)[:, k0] @ t["x"].astype(np.float64)[0, 1]) > 64 * ((d["K"] + 1) * 2.0 ** -24 * mag)  # w.x would show
    # the step clamp: two trips, and the recurrence still alive where the second trip writes
    d = rc.LIMIT_CASES["steps_tanh"]
    h = rc.Handle(d)
    assert max_steps < h.T <= 2 * max_steps and h.simple() and (h.bn, h.bc, h.bk) == (d["N"], d["C"], d["K"])
    t, out, _ = rc.limit_expected("steps_tanh")
    last = out["h"][-1]
    assert np.all(np.isfinite(last)) and np.all((np.abs(last) > 0) & (np.abs(last) < 1))
    assert not np.array_equal(out["h"][max_steps], out["h"][max_steps - 1])
    # the row-tile limit: refused by exactly that rule at one thread, admitted at two
    d = rc.LIMIT_CASES["manyrows_relu"]
    h1, h2 = rc.Handle(d), rc.Handle(dict(d, threads=2))
    assert h1.status == rc.SUCCESS and d["max_T"] * d["N"] * max(d["C"], d["K"]) < 1 << 31  # (no other refusal of execute_st applies)
    assert [tiles(n1 - n0, BT) for n0, n1 in h1.shares()] == [max_tiles + 3]
    assert [tiles(n1 - n0, BT) for n0, n1 in h2.shares()] == [(max_tiles + 3) // 2] * 2 and (max_tiles + 3) // 2 > 1 << 15
    assert h1.shares()[0][1] - h1.shares()[0][0] > rows["threshold"] >= max(n1 - n0 for n0, n1 in h2.shares())
    small = dict(d, N=640, bn=320)
    ts = rc.inputs("manyrows_relu", small)
    want = rc.forward(rc.Handle(small), ts)
    got_h, got_z = rc.forward_c1k1(ts)
    assert rc.same_bits(got_h, want["h"]) and rc.same_bits(got_z, want["z"]) and np.any(want["h"] == 0) and np.any(want["h"] > 0)
    # the wide case: just below 2^31 elements, step 1 begins within 2^20 bytes of byte 2^32 and ends near byte 2^33
    d = rc.WIDE_CASE
    h = rc.Handle(d)
    total = d["max_T"] * d["N"] * d["K"]
    assert (1 << 31) - (1 << 20) <= total < 1 << 31 and total + d["max_T"] * rc.WIDE_PERIOD * d["K"] >= 1 << 31
    assert (1 << 32) - (1 << 20) < d["N"] * d["K"] * 4 < 1 << 32 < (d["N"] + rc.WIDE_PERIOD) * d["K"] * 4 and total * 4 > (1 << 33) - (1 << 22)
    assert d["N"] % rc.WIDE_PERIOD == 0 and rc.WIDE_PERIOD % h.bn == 0 and rc.WIDE_PERIOD % BT != 0 and h.status == rc.SUCCESS
    shares = h.shares()
    assert len(shares) == 4 and shares[0][0] == 0 and shares[-1][1] == d["N"] and all(0 < n1 - n0 <= rows["threshold"] for n0, n1 in shares)
    assert all(n0 % rc.WIDE_PERIOD != 0 and n0 % BT != 0 for n0, _ in shares[1:])  # a share boundary falls inside a period and a tile


def test_rnn_kernel_compiles_for_gfx950(tmp_path):
    """the device code alone, to assembly: it compiles, and the fp32 divide of the sigmoid is the correctly rounded sequence"""
    out = tmp_path / "rnn.s"
    src = os.path.join(ROOT, "libxsmm-1_amd", "csrc", "kernels", "rnn.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                    src, "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    for g in range(1, 5):
        assert "rnn_stepILi%dEE" % g in text
    assert "v_mfma_f32_32x32x2" in text and "v_div_fixup_f32" in text and "v_div_fmas_f32" in text
