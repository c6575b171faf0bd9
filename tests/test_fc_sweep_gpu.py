"""The seeded descriptor sweep of tests/fc_common.py (sweep_cases) on the GPU: what test_fc_gpu.py does for the named cases -- the
three passes bit for bit against the oracle's fma chains in the tensors' layouts, destinations pre-filled with NaN between canary
bands -- on 32 drawn descriptors, with both values of LIBXSMM_AMD_FC_TILE: the packed format with block factors that divide their
dimension or do not (create answers WARN_*, takes the whole dimension, and the passes run), the custom format in fp32 and
bf16-in / fp32-out, N on either side of both tile sizes, K = 1000. tests/test_fc_sweep_cpu.py holds the expectation of the same
cases against float64 products and counts what the set holds. The shares of the logical threads run in reverse order, each is one
launch, and an empty share launches nothing; the inputs and the scratch are compared afterwards."""
import os

import numpy as np
import pytest

import fc_common as fc
from test_fc_gpu import DEST, Layer, tile_env  # noqa: F401 (tile_env: a fixture)

pytestmark = pytest.mark.gpu

KERNEL = {fc.FWD: "fwd", fc.BWD: "bwd", fc.UPD: "upd"}


@pytest.mark.parametrize("tile", ("64", "128"))
@pytest.mark.parametrize("name", sorted(fc.sweep_cases()))
def test_three_passes_bit_equal(xs, orc, torch_gpu, tile_env, name, tile):
    os.environ["LIBXSMM_AMD_FC_TILE"] = tile
    layer = Layer(xs, torch_gpu, name, sweep=True)
    h = layer.h
    for kind in (fc.FWD, fc.BWD, fc.UPD):
        for tid in reversed(range(h.d["threads"])):
            b0, b1 = h.share(kind, tid)
            launches = layer.L.libxsmm_amd_launch_count()
            assert 0 == xs.fc_execute(layer.handle, kind, 0, tid)
            assert (1 if b1 > b0 else 0) == layer.L.libxsmm_amd_launch_count() - launches, "a share is one launch, an empty one none"
        assert xs.last_kernel() == ("fc_f32_t" + tile if h.f32 else "fc_bf16_%s_t%s" % (KERNEL[kind], tile))
        layer.check(kind)
    for t in (fc.REG_IN, fc.REG_FIL, fc.GRAD_OUT):
        got, want = layer.result(t), layer.want[t].astype(fc.dtype_of(h, t))
        assert got.tobytes() == want.tobytes(), "input tensor %d was written" % t
    assert np.all(layer.scratch.cpu().numpy() == 0x5a), "the scratch is never written"
    layer.close()
