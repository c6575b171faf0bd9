"""The seeded descriptor sweep of tests/pool_common.py (sweep_cases) on the GPU: what test_pool_gpu.py does for the named cases --
FWD then BWD, bit for bit against the restatement, destinations pre-filled with ones bits between canary bands, the kernel's name
and the inputs compared afterwards -- on 48 drawn descriptors that combine strides, windows, logical paddings up to and beyond the
window's extent (windows wholly in the padding), physical paddings on either side, channel counts, image counts and both element
types. tests/test_pool_sweep_cpu.py holds the restatement of the same cases against a float64 definition and counts what the set
holds. The shares of the logical threads run in reverse order, each is one launch, and an empty share launches nothing."""
import pytest

import pool_common as pc
from test_pool_gpu import Layer

pytestmark = pytest.mark.gpu


def shares_in_reverse(layer, kind):
    d = layer.h.d
    for tid in reversed(range(d["threads"])):
        b0, b1 = layer.h.share(tid)
        launches = layer.L.libxsmm_amd_launch_count()
        assert 0 == layer.run(kind, 0, tid)
        assert (1 if b1 > b0 else 0) == layer.L.libxsmm_amd_launch_count() - launches, "a share is one launch, an empty one none"


@pytest.mark.parametrize("name", sorted(pc.sweep_cases()))
def test_fwd_and_bwd_bit_equal(xs, torch_gpu, name):
    d = pc.sweep_cases()[name]
    want = pc.sweep_expected(name)
    layer = Layer(xs, torch_gpu, d, want)
    is_max = d["pooling_type"] == pc.MAX
    kernel = "%s_%s" % ("max" if is_max else "avg", "f32" if layer.h.f32 else "bf16")
    shares_in_reverse(layer, pc.FWD)
    assert xs.last_kernel() == "pool_fwd_" + kernel
    layer.check(pc.REG_OUT)     # the physical padding keeps its fill: it is part of the comparison
    if is_max:
        layer.check(pc.MASK)    # ... and so does the mask where a window holds no element
    shares_in_reverse(layer, pc.BWD)
    assert xs.last_kernel() == "pool_bwd_" + kernel
    for t in (pc.GRAD_IN, pc.REG_IN, pc.GRAD_OUT, pc.REG_OUT) + ((pc.MASK,) if is_max else ()):
        layer.check(t)
    layer.close()
