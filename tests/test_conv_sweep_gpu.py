"""The seeded descriptor sweep of tests/conv_common.py (sweep_cases) on the GPU: what test_conv_gpu.py does for the named cases --
the filter transposition, FWD with both tiles, BWD and UPD, bit for bit against the restatement, with the kernel names and the
inputs compared afterwards -- on 48 drawn descriptors that combine strides, windows, paddings on either side, block sizes,
accumulation, fusions and NO_FILTER_TRANSPOSE. tests/test_conv_sweep_cpu.py holds the restatement of the same cases against a
float64 convolution and counts what the set holds. Where a case has more than one logical thread the shares run in reverse order."""
import pytest

import conv_common as cc
from test_conv_gpu import DEST, FWD_KERNELS, Layer, with_tile

pytestmark = pytest.mark.gpu


def shares_in_reverse(layer, kind):
    for tid in reversed(range(layer.h.d["threads"])):
        assert 0 == layer.run(kind, 0, tid)


@pytest.mark.parametrize("name", sorted(cc.sweep_cases()))
def test_three_passes_bit_equal(xs, torch_gpu, name):
    d = cc.sweep_cases()[name]
    want = cc.sweep_expected(name)
    layer = Layer(xs, torch_gpu, d, want)
    assert 0 == layer.L.libxsmm_dnn_trans_reg_filter(layer.handle)  # (BWD with NO_FILTER_TRANSPOSE reads it)
    assert xs.last_kernel() == "conv_trans_filter"
    layer.check(cc.REG_FIL_TR, want["wtr"])
    kernels = {cc.FWD: FWD_KERNELS[64], cc.BWD: "conv_bwd", cc.UPD: "conv_upd_image" if layer.h.upd_per_image() else "conv_upd_gemm"}
    for kind, (dest, key) in DEST.items():
        with_tile(64, lambda: shares_in_reverse(layer, kind))
        assert xs.last_kernel() == kernels[kind]
        layer.check(dest, want[key])  # the physical padding and every element no term reaches are part of the comparison
    for t, key in ((cc.REG_IN, "x"), (cc.REG_FIL, "w"), (cc.GRAD_OUT, "dout"), (cc.REG_BIAS, "bias"), (cc.REG_FIL_TR, "wtr")):
        layer.check(t, want[key])
    layer.close()
    layer = Layer(xs, torch_gpu, d, want)
    with_tile(128, lambda: shares_in_reverse(layer, cc.FWD))
    assert xs.last_kernel() == FWD_KERNELS[128]
    layer.check(cc.REG_OUT, want["out"])
    layer.close()
