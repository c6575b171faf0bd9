"""The seeded descriptor sweep of tests/bn_common.py (sweep_cases) on the GPU: what test_bn_gpu.py does for the named cases -- FWD
then BWD, all thirteen tensors compared whole and bit for bit against the restatement after either pass, destinations pre-filled
with ones bits between canary bands, the kernel's name asserted -- on 40 drawn descriptors that combine the eight fuse combinations
with strides, physical paddings on either side, channel and image counts, both element types and one to five logical threads.
tests/test_bn_sweep_cpu.py holds the restatement of the same cases against a float64 definition and counts what the set holds,
the share patterns among them: a run of channel blocks that wraps, a share as long as an image, more shares than items. The shares
run in reverse order; a share is three launches with statistics (partial sums, finish, apply) and one without, an empty share none."""
import pytest

import bn_common as bc
from test_bn_gpu import ALL_KEYS, Layer, after_fwd

pytestmark = pytest.mark.gpu


def shares_in_reverse(layer, kind):
    d = layer.d
    per_share = 3 if d["fuse_ops"] & bc.OPS_BN else 1
    for tid in reversed(range(d["threads"])):
        b0, b1 = layer.h.share(tid)
        launches = layer.L.libxsmm_amd_launch_count()
        assert 0 == layer.run(kind, 0, tid)
        assert (per_share if b1 > b0 else 0) == layer.L.libxsmm_amd_launch_count() - launches


@pytest.mark.parametrize("name", sorted(bc.sweep_cases()))
def test_fwd_and_bwd_bit_equal(xs, torch_gpu, name):
    d = bc.sweep_cases()[name]
    want = bc.sweep_expected(name)
    layer = Layer(xs, torch_gpu, d, want)
    dname = "f32" if layer.h.f32 else "bf16"
    shares_in_reverse(layer, bc.FWD)
    assert xs.last_kernel() == "bn_fwd_apply_" + dname
    layer.check(ALL_KEYS, after_fwd(want))  # padding, skipped pixels and every tensor FWD does not write keep their bytes
    shares_in_reverse(layer, bc.BWD)
    assert xs.last_kernel() == "bn_bwd_apply_" + dname
    layer.check(ALL_KEYS)                   # ... the inputs among them
    layer.close()
