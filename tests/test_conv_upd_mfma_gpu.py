"""UPD of the convolution layer on the matrix cores (kernels/conv_upd_mfma.hip, LIBXSMM_AMD_CONV_UPD=mfma): both forms
of UPD go to conv_upd_mfma_gemm / conv_upd_mfma_image in one launch per call, and dfilter -- the canary bands included -- keeps the
bits of the restatement of tests/conv_common.py."""
import functools

import numpy as np
import pytest

import conv_common as cc
from test_conv_gpu import Layer

pytestmark = pytest.mark.gpu


def run_upd(xs, layer, tids, kernel=None):
    """UPD of the shares tids in turn: one launch each, on the kernel of the form (or on the one named)"""
    for tid in tids:
        launches = layer.L.libxsmm_amd_launch_count()
        assert 0 == layer.run(cc.UPD, 0, tid)
        assert 1 == layer.L.libxsmm_amd_launch_count() - launches
        assert xs.last_kernel() == (kernel or ("conv_upd_mfma_image" if layer.h.upd_per_image() else "conv_upd_mfma_gemm"))


@pytest.mark.parametrize("name", sorted(cc.COMPUTE_CASES))
def test_named_cases_bit_equal(xs, torch_gpu, monkeypatch, name):
    monkeypatch.setenv("LIBXSMM_AMD_CONV_UPD", "mfma")
    want = cc.expected(name)
    layer = Layer(xs, torch_gpu, cc.COMPUTE_CASES[name], want)
    run_upd(xs, layer, (0,))
    layer.check(cc.GRAD_FIL, want["dw"], name.startswith("special_"))
    for t, key in ((cc.REG_IN, "x"), (cc.GRAD_OUT, "dout")):
        layer.check(t, want[key])
    layer.close()


A = cc.desc(H=7, W=9, R=3, S=3, pad=(1, 1), pin=cc.LOGICAL, N=3, C=16, K=16)
SHAPES = {
    "a_odd_189_terms": A,                                                                         # 189 = 2 * 64 + 61 terms, 144 columns
    "b_ragged_k136": cc.desc(11, 10, 3, 3, pad=(1, 1), N=2, C=5, K=136, options=0),               # 2 tiles + 8 rows, blocks of 8 and 5
    "c_q_tiles_block2": cc.desc(6, 6, 3, 3, pad=(1, 1), pin=cc.LOGICAL, N=2, C=24, K=18),         # ofmblock 2, 27 items in a tile row
    "d_2x3_rim_outpad": cc.desc(6, 8, 2, 3, pad=(0, 1), pout=(1, 2), N=2, C=8, K=16),
    "e_1x1_s2_zero_row": cc.desc(5, 7, 1, 1, 2, 2, N=3, C=24, K=16),                              # GEMM form at stride 2
    "f_three_shares": cc.desc(7, 7, 3, 3, pad=(1, 1), N=2, C=24, K=40, threads=3),                # 15 items, tiles across shares
    "g_image_odd_plane": cc.desc(21, 25, 3, 3, 2, 2, pad=(1, 1), pin=cc.LOGICAL, N=3, C=16, K=16, options=0),  # 143 terms per image
    "h_image_physical_c72": cc.desc(7, 9, 2, 2, 2, 1, pad=(1, 1), N=2, C=72, K=8),                # 288 columns, nine items
    "i_one_term": cc.desc(1, 1, 1, 1, N=1, C=3, K=3),                                             # the tail alone
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """the inputs of a shape, dfilter after each share (the last first) and the float64 contract: computed once, read only"""
    h = cc.Handle(SHAPES[name])
    t = cc.inputs(name, SHAPES[name])
    steps = [t["dw0"]]
    for tid in reversed(range(h.d["threads"])):
        steps.append(cc.upd(h, t["x"], t["dout"], steps[-1], tid))
    return h, t, steps, cc.contract64(h, t)["dw"]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_bit_equal_and_within_the_float64_bound(xs, torch_gpu, monkeypatch, name):
    monkeypatch.setenv("LIBXSMM_AMD_CONV_UPD", "mfma")
    h, t, steps, (value, bound, _) = shape_case(name)
    assert h.upd_per_image() == (name[0] in "gh")
    layer = Layer(xs, torch_gpu, SHAPES[name], t)
    last = h.d["threads"] - 1
    run_upd(xs, layer, (last,))
    layer.check(cc.GRAD_FIL, steps[1])
    if last > 0:  # after the first share only that share's items have changed
        lo, hi = h.share(cc.UPD, last)
        untouched = np.ones(h.work(cc.UPD), dtype=bool)
        untouched[lo:hi] = False
        assert lo < hi and cc.same_bits(steps[1].reshape(len(untouched), -1)[untouched], t["dw0"].reshape(len(untouched), -1)[untouched])
    run_upd(xs, layer, reversed(range(last)))
    layer.check(cc.GRAD_FIL, steps[-1])
    got = cc.interior(h, "dw", layer.result(cc.GRAD_FIL)).astype(np.float64)
    assert np.all(np.abs(got - value) <= bound), "beyond terms * 2^-24 * (sum|a*b| + |start|) in %d elements" % np.sum(np.abs(got - value) > bound)
    layer.close()


def test_matrix_cores_switched_off(xs, torch_gpu, monkeypatch):
    """libxsmm_amd_set_mfma(0) takes the path away although the variable is set: conv_upd_gemm, the same bits"""
    monkeypatch.setenv("LIBXSMM_AMD_CONV_UPD", "mfma")
    h, t, steps, _ = shape_case("a_odd_189_terms")
    layer = Layer(xs, torch_gpu, A, t)
    before = layer.L.libxsmm_amd_get_mfma()
    layer.L.libxsmm_amd_set_mfma(0)
    try:
        run_upd(xs, layer, (0,), "conv_upd_gemm")
    finally:
        layer.L.libxsmm_amd_set_mfma(before)
    layer.check(cc.GRAD_FIL, steps[-1])
    layer.close()
