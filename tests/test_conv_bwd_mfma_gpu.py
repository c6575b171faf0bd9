"""BWD of the convolution layer on the matrix cores (kernels/conv_bwd_mfma.hip, LIBXSMM_AMD_CONV_BWD=mfma): the
pixels of dinput that have all their terms go to conv_bwd_mfma_t64 / _t128, the frame around them to conv_bwd, and dinput --
its physical padding and the canary bands included -- keeps the bits of the restatement of tests/conv_common.py."""
import functools

import numpy as np
import pytest

import conv_common as cc
from test_conv_gpu import Layer, with_tile

pytestmark = pytest.mark.gpu


def full_rect(h):
    """(rows, columns, whether it is the whole buffer plane) of the full rectangle; rows or columns <= 0: empty"""
    d = h.d
    rows = min(h.ofh, d["pad_h"] + d["H"]) - max(d["R"] - 1, d["pad_h"])
    cols = min(h.ofw, d["pad_w"] + d["W"]) - max(d["S"] - 1, d["pad_w"])
    return rows, cols, (rows, cols) == (h.ifhp, h.ifwp)


def run_bwd(xs, layer, tile=None):
    """BWD of every share, the last first; returns the launches and checks the kernel's name against the rectangle"""
    def shares():
        for tid in reversed(range(layer.h.d["threads"])):
            assert 0 == layer.run(cc.BWD, 0, tid)
    rows, cols, whole = full_rect(layer.h)
    mfma = layer.h.d["u"] == layer.h.d["v"] == 1 and rows > 0 and cols > 0
    launches = layer.L.libxsmm_amd_launch_count()
    shares() if tile is None else with_tile(tile, shares)
    launches = layer.L.libxsmm_amd_launch_count() - launches
    if mfma:
        assert xs.last_kernel().startswith("conv_bwd_mfma_t") and (tile is None or xs.last_kernel() == "conv_bwd_mfma_t%d" % tile)
    else:
        assert xs.last_kernel() == "conv_bwd"
    return launches, mfma, whole


@pytest.mark.parametrize("name", sorted(n for n, d in cc.COMPUTE_CASES.items() if d["u"] == d["v"] == 1))
def test_named_cases_bit_equal(xs, torch_gpu, monkeypatch, name):
    monkeypatch.setenv("LIBXSMM_AMD_CONV_BWD", "mfma")
    want = cc.expected(name)
    layer = Layer(xs, torch_gpu, cc.COMPUTE_CASES[name], want)
    assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)  # (BWD of the notrans case reads it)
    launches, mfma, whole = run_bwd(xs, layer)
    assert launches == (1 + (not whole) if mfma else 1)  # [frame] + one slab
    layer.check(cc.GRAD_IN, want["din"], name.startswith("special_"))
    layer.close()


A = dict(H=7, W=9, R=3, S=3, pad=(1, 1), pin=cc.LOGICAL, N=3, C=16, K=16)
SHAPES = {
    "a_tile_ends_in_image_1": cc.desc(**A),                                                   # 35 pixels per image
    "b_ragged_c_and_k_tail": cc.desc(11, 10, 3, 3, pad=(1, 1), N=2, C=136, K=5, options=0),  # reduction 45 = 32 + 13
    "c_1x1_whole_plane": cc.desc(6, 6, 1, 1, N=2, C=24, K=18),
    "d_2x3_window_rim_outpad": cc.desc(6, 8, 2, 3, pad=(0, 1), pout=(1, 2), N=2, C=8, K=16),
    "e_filter_trans": cc.desc(options=cc.OVERWRITE | cc.NO_FILTER_TRANSPOSE, **A),
    "f_three_shares": cc.desc(7, 7, 3, 3, pad=(1, 1), N=2, C=24, K=16, threads=3),
    "g_stride_2": cc.desc(5, 5, 3, 3, 2, 2, pad=(1, 1), N=1, C=16, K=16),
    "h_no_full_pixel": cc.desc(1, 5, 3, 3, pad=(1, 1), N=1, C=8, K=8),
}
SLAB_DESC = cc.desc(2047, 4099, 1, 1, N=1, C=1, K=1)  # 131104 pixel tiles of 64: three launches of at most 65535


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """the inputs of a shape, dinput after each share (the last first) and the float64 contract: computed once, read only"""
    h = cc.Handle(SHAPES[name])
    t = cc.inputs(name, SHAPES[name])
    steps = [t["din0"]]
    for tid in reversed(range(h.d["threads"])):
        steps.append(cc.bwd(h, t["dout"], t["w"], steps[-1], tid))
    return h, t, steps, cc.contract64(h, t)["din"]


@pytest.mark.parametrize("tile", (64, 128))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_bit_equal_and_within_the_float64_bound(xs, torch_gpu, monkeypatch, name, tile):
    monkeypatch.setenv("LIBXSMM_AMD_CONV_BWD", "mfma")
    h, t, steps, (value, bound, _) = shape_case(name)
    layer = Layer(xs, torch_gpu, SHAPES[name], t)
    assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)
    if h.d["threads"] > 1:  # after the first share only that share's items have changed
        assert 0 == with_tile(tile, lambda: layer.run(cc.BWD, 0, h.d["threads"] - 1))
        layer.check(cc.GRAD_IN, steps[1])
        lo, hi = h.share(cc.BWD, h.d["threads"] - 1)
        untouched = np.ones(h.work(cc.BWD), dtype=bool)
        untouched[lo:hi] = False
        assert lo < hi and cc.same_bits(steps[1].reshape(len(untouched), -1)[untouched], t["din0"].reshape(len(untouched), -1)[untouched])
        layer.close()
        layer = Layer(xs, torch_gpu, SHAPES[name], t)
    launches, mfma, whole = run_bwd(xs, layer, tile)
    assert launches == h.d["threads"] * (1 + (not whole) if mfma else 1) and mfma == (name[0] not in "gh") and whole == (name[0] == "c")
    layer.check(cc.GRAD_IN, steps[-1])
    got = cc.interior(h, "din", layer.result(cc.GRAD_IN)).astype(np.float64)
    assert np.all(np.abs(got - value) <= bound), "beyond K*R*S * 2^-24 * (sum|a*b| + |start|) in %d elements" % np.sum(np.abs(got - value) > bound)
    layer.close()


@functools.lru_cache(maxsize=None)
def slab_case():
    h = cc.Handle(SLAB_DESC)
    rng = np.random.default_rng(7)
    t = dict(dout=rng.standard_normal(h.out_shape(), dtype=np.float32), w=rng.standard_normal(h.fil_shape(), dtype=np.float32),
             din0=np.full(h.in_shape(), cc.POISON, dtype=np.float32))
    return t, cc.bwd(h, t["dout"], t["w"], t["din0"])


@pytest.mark.parametrize("tile,slabs", [(64, 3), (128, 2)])
def test_pixel_tiles_in_several_slabs(xs, torch_gpu, monkeypatch, tile, slabs):
    """1 x 1 on 2047 x 4099 pixels: the whole plane, no frame, one launch per slab of 65535 pixel tiles (jtile0 > 0)"""
    monkeypatch.setenv("LIBXSMM_AMD_CONV_BWD", "mfma")
    t, want = slab_case()
    part = type("Part", (Layer,), {"SLOTS": {k: Layer.SLOTS[k] for k in (cc.GRAD_OUT, cc.REG_FIL, cc.GRAD_IN)}})
    layer = part(xs, torch_gpu, SLAB_DESC, t)
    launches, mfma, whole = run_bwd(xs, layer, tile)
    assert mfma and whole and launches == slabs == -(-(-(-2047 * 4099 // tile)) // 65535)
    layer.check(cc.GRAD_IN, want)
    layer.close()
