"""The convolution layer past its launch limits (kernels/conv.hip; the limits are those of tests/launch_limits.py, which
tests/test_launch_limits_cpu.py holds against the source): FWD over more than two slabs of 65535 pixel tiles (jtile0 > 0, tiles
that straddle images, a share that starts at a later image), BWD and UPD over more than two slabs of 32768 items (blockIdx.z > 0),
and the filter transposition wrapped into a second row of work-groups (blockIdx.y > 0).

Bit for bit against tests/conv_common.py with the oracle's fused chain, every tensor between canary bands; a destination starts
from ones bits where the pass overwrites and from seeded values where it accumulates, and what a pass reads is compared
afterwards. Only the tensors a pass touches exist. Each restatement is computed once and shared by the tests that need it."""
import time

import numpy as np
import pytest

import conv_common as cc
import launch_limits as ll
import oracle_binding as orc
from test_conv_gpu import FWD_KERNELS, Layer, with_tile

pytestmark = pytest.mark.gpu

_data = {}


def cached(key, make):
    if key not in _data:
        t0 = time.time()
        _data[key] = make()
        print("restatement %s: %.1f s" % (key, time.time() - t0))
    return _data[key]


def normal(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def poison(shape):
    return np.full(shape, cc.POISON, dtype=np.float32)


def layer_of(xs, torch, d, data, types):
    """a Layer with the tensors `types` alone"""
    part = type("Part", (Layer,), {"SLOTS": {t: Layer.SLOTS[t] for t in types}})
    return part(xs, torch, d, data)


def in_reverse(layer, kind, threads):
    for tid in reversed(range(threads)):
        assert 0 == layer.run(kind, 0, tid)


# ---- FWD: three slabs of pixel tiles at tile 64, two at tile 128 -----------------------------------------------------------------
FWD_DESC = cc.desc(H=1, W=4099, R=1, S=5, pad=(0, 2), pin=cc.LOGICAL, N=2047, C=8, K=2)
FWD_TYPES = (cc.REG_IN, cc.REG_FIL, cc.REG_OUT)
SLAB = ll.per_trip("conv_fwd_slab")


def fwd_case(options, fuse):
    def make():
        h = cc.Handle(dict(FWD_DESC, options=options, fuse_ops=fuse))
        x, w = cached("fwd inputs", lambda: (normal(11, h.in_shape()), normal(12, h.fil_shape())))
        t = dict(x=x, w=w, out0=poison(h.out_shape()) if h.overwrite else normal(13, h.out_shape()))
        t["out"] = cc.fwd(h, x, w, t["out0"], None, arith=orc.FMA)
        return t
    return cached(("fwd", options, fuse), make)


def slabs(pixels, tile):
    tiles = -(-pixels // tile)
    return -(-tiles // SLAB)


def test_the_fwd_case_is_what_it_is_for():
    h = cc.Handle(FWD_DESC)
    pixels = h.d["N"] * h.ofh * h.ofw
    assert (h.ofh, h.ofw, h.ifmblock, h.ofmblock, h.blocksifm, h.blocksofm) == (1, 4099, 8, 2, 1, 1) and not h.physical
    assert h.d["C"] * h.d["R"] * h.d["S"] == 40  # a chunk of 32 and a tail
    assert pixels == 2 * SLAB * 64 + 2173 == SLAB * 128 + 2173 and (slabs(pixels, 64), slabs(pixels, 128)) == (3, 2)
    assert (h.ofh * h.ofw) % 64 and (SLAB * 64) % (h.ofh * h.ofw) and (SLAB * 128) % (h.ofh * h.ofw)  # tiles and slabs straddle images
    h2 = cc.Handle(dict(FWD_DESC, threads=2))
    assert [h2.share(cc.FWD, t) for t in (0, 1)] == [(0, 1024), (1024, 2047)]
    assert 1024 * 4099 > SLAB * 64 > 1023 * 4099  # share 0 crosses the slab of tile 64, share 1 does not


@pytest.mark.parametrize("options,fuse", [(cc.OVERWRITE, 0), (0, cc.FUSE_RELU)])
@pytest.mark.parametrize("tile", [64, 128])
def test_fwd_pixel_tiles_in_several_slabs(xs, torch_gpu, tile, options, fuse):
    """threads = 1: one launch per slab; the accumulating variant reads its start value and stores through the ReLU past the slab"""
    d = dict(FWD_DESC, options=options, fuse_ops=fuse)
    want = fwd_case(options, fuse)
    assert not fuse or (np.any(want["out"] == 0) and np.any(want["out"] > 0))
    layer = layer_of(xs, torch_gpu, d, want, FWD_TYPES)
    launches = layer.L.libxsmm_amd_launch_count()
    assert 0 == with_tile(tile, lambda: layer.run(cc.FWD))
    assert layer.L.libxsmm_amd_launch_count() - launches == {64: 3, 128: 2}[tile] == slabs(layer.h.d["N"] * layer.h.ofw, tile)
    assert xs.last_kernel() == FWD_KERNELS[tile]
    print("kernel %s, %d launches" % (xs.last_kernel(), layer.L.libxsmm_amd_launch_count() - launches))
    layer.check(cc.REG_OUT, want["out"])
    layer.check(cc.REG_IN, want["x"])
    layer.check(cc.REG_FIL, want["w"])
    layer.close()


def test_fwd_shares_on_either_side_of_a_slab(xs, torch_gpu):
    """threads = 2 at tile 64, share 1 first: it starts at image 1024 (img0 > 0) and fits one slab, share 0 needs a second"""
    d = dict(FWD_DESC, threads=2)
    want = fwd_case(cc.OVERWRITE, 0)
    layer = layer_of(xs, torch_gpu, d, want, FWD_TYPES)
    for tid, count in ((1, 1), (0, 2)):
        launches = layer.L.libxsmm_amd_launch_count()
        assert 0 == with_tile(64, lambda: layer.run(cc.FWD, 0, tid))
        assert layer.L.libxsmm_amd_launch_count() - launches == count and xs.last_kernel() == FWD_KERNELS[64]
        if tid == 1:  # everything outside the share still holds its start bits
            got = layer.result(cc.REG_OUT).reshape(2047, -1)
            assert cc.same_bits(got[1024:], want["out"].reshape(2047, -1)[1024:]) and cc.same_bits(got[:1024], want["out0"].reshape(2047, -1)[:1024])
    layer.check(cc.REG_OUT, want["out"])
    layer.check(cc.REG_IN, want["x"])
    layer.close()


# ---- BWD: items in three slabs along gridDim.z ----------------------------------------------------------------------------------------
ITEMS = ll.per_trip("conv_items")
BWD_DESC = cc.desc(H=1, W=3, R=1, S=3, pad=(0, 1), N=ll.sized("conv_items", 41), C=1, K=2)
BWD_TYPES = (cc.GRAD_OUT, cc.REG_FIL, cc.REG_FIL_TR, cc.GRAD_IN)


def bwd_case():
    def make():
        h = cc.Handle(BWD_DESC)
        t = dict(dout=normal(21, h.out_shape()), w=normal(22, h.fil_shape()), din0=poison(h.in_shape()))
        t["din"] = cc.bwd(h, t["dout"], t["w"], t["din0"], arith=orc.FMA)
        t["wtr"] = cc.trans_filter(h, t["w"])
        return t
    return cached("bwd", make)


@pytest.mark.parametrize("threads,options", [(1, cc.OVERWRITE), (2, cc.OVERWRITE), (1, cc.OVERWRITE | cc.NO_FILTER_TRANSPOSE)])
def test_bwd_items_in_three_slabs(xs, torch_gpu, threads, options):
    """physical padding: the kernel zeroes the rim columns, which are compared. threads = 2 in reverse: share 1 starts past the
    first slab. NO_FILTER_TRANSPOSE reads the filter that libxsmm_dnn_trans_reg_filter wrote."""
    d = dict(BWD_DESC, threads=threads, options=options)
    want = bwd_case()
    layer = layer_of(xs, torch_gpu, d, want, BWD_TYPES)
    h = layer.h
    assert h.work(cc.BWD) == 65577 == 2 * ITEMS + 41 and h.physical and (h.ifwp, h.ifmblock, h.blocksifm) == (5, 1, 1)
    assert threads == 1 or h.share(cc.BWD, 1)[0] == 32789 > ITEMS
    if options & cc.NO_FILTER_TRANSPOSE:
        assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)
        layer.check(cc.REG_FIL_TR, want["wtr"])
    in_reverse(layer, cc.BWD, threads)
    assert xs.last_kernel() == "conv_bwd"
    print("kernel %s, %d items" % (xs.last_kernel(), h.work(cc.BWD)))
    layer.check(cc.GRAD_IN, want["din"])
    assert np.all(cc.bits(want["din"][..., 0, :]) == 0) and np.all(cc.bits(want["din"][..., 4, :]) == 0)  # the rim, zeroed
    layer.check(cc.GRAD_OUT, want["dout"])
    layer.check(cc.REG_FIL, want["w"])
    layer.close()


# ---- UPD: items in three slabs, both kernels ------------------------------------------------------------------------------------------
UPD_DESC = {"conv_upd_gemm": cc.desc(H=1, W=3, R=1, S=1, N=2, C=257, K=257),
            "conv_upd_image": cc.desc(H=1, W=5, R=1, S=3, u=1, v=2, pad=(0, 1), pin=cc.LOGICAL, N=1, C=257, K=257)}  # (N = 1: the restatement of N = 2 takes 6 s)
UPD_TYPES = (cc.REG_IN, cc.GRAD_OUT, cc.GRAD_FIL)


def upd_case(kernel, options):
    def make():
        h = cc.Handle(dict(UPD_DESC[kernel], options=options))
        t = dict(x=normal(31, h.in_shape()), dout=normal(32, h.out_shape()), dw0=poison(h.fil_shape()) if h.overwrite else normal(33, h.fil_shape()))
        t["dw"] = cc.upd(h, t["x"], t["dout"], t["dw0"], arith=orc.FMA)
        return t
    return cached((kernel, options), make)


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("options", [cc.OVERWRITE, 0])
@pytest.mark.parametrize("kernel", sorted(UPD_DESC))
def test_upd_items_in_three_slabs(xs, torch_gpu, kernel, options, threads):
    """blocks of one channel on both sides: 257 * 257 items. threads = 3 in reverse: the last share starts at item
    44034, inside what one launch takes as its second slab"""
    d = dict(UPD_DESC[kernel], options=options, threads=threads)
    want = upd_case(kernel, options)
    layer = layer_of(xs, torch_gpu, d, want, UPD_TYPES)
    h = layer.h
    assert (h.ifmblock, h.ofmblock) == (1, 1) and h.work(cc.UPD) == 66049 == ll.sized("conv_items", 513)
    assert h.upd_per_image() == (kernel == "conv_upd_image")
    assert threads == 1 or 2 * ITEMS > h.share(cc.UPD, 2)[0] > ITEMS
    in_reverse(layer, cc.UPD, threads)
    assert xs.last_kernel() == kernel
    print("kernel %s, %d items" % (xs.last_kernel(), h.work(cc.UPD)))
    layer.check(cc.GRAD_FIL, want["dw"])
    layer.check(cc.REG_IN, want["x"])
    layer.check(cc.GRAD_OUT, want["dout"])
    layer.close()


# ---- the filter transposition in two rows of work-groups --------------------------------------------------------------------------------
def test_trans_filter_in_two_rows_of_work_groups(xs, torch_gpu):
    d = cc.desc(H=3, W=3, R=3, S=3, pad=(1, 1), N=1, C=1376, K=1380)
    h = cc.Handle(d)
    total = int(np.prod(h.fil_shape()))
    assert (h.ifmblock, h.ofmblock) == (16, 4) and total == 17089920 > ll.per_trip("conv_trans_filter")
    w = normal(41, h.fil_shape())
    layer = layer_of(xs, torch_gpu, d, dict(w=w), (cc.REG_FIL, cc.REG_FIL_TR))
    assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)
    assert xs.last_kernel() == "conv_trans_filter"
    print("kernel %s, %d elements" % (xs.last_kernel(), total))
    layer.check(cc.REG_FIL_TR, cc.trans_filter(h, w))
    layer.check(cc.REG_FIL, w)
    layer.close()
