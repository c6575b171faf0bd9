"""The fused batch-norm layer past its launch limits (kernels/bn.hip): the apply kernel takes its items along gridDim.y in slabs
of 32768 along gridDim.z, and the partial-sum and finish kernels take one work-group per (channel block, image) and per channel
block along gridDim.x. Planes of one pixel and 2 * 32768 + 41 items (N = 3, so a multiple of 3) cross the slab twice with a rest;
bit for bit against tests/bn_common.py, every tensor between canaries."""
import os
import re

import pytest

import bn_common as bc
from test_bn_gpu import ALL_KEYS, Layer, after_fwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SLAB = 32768
ITEMS = 2 * SLAB + 41
_data = {}


def test_the_slab_is_what_the_source_says():
    with open(os.path.join(ROOT, "libxsmm-1_amd", "csrc", "kernels", "bn.hip")) as f:
        src = f.read()
    m = re.search(r"gy = items < (\d+) \? items : \1, gz = \(items \+ gy - 1\) / gy", src)
    assert m and int(m.group(1)) == SLAB
    assert "(long long)g.w0 + blockIdx.y + (long long)blockIdx.z * gridDim.y" in src
    assert ITEMS % 3 == 0 and ITEMS > 2 * SLAB


@pytest.mark.parametrize("dt", [bc.F32, bc.BF16])
@pytest.mark.parametrize("threads", [1, 2])
def test_items_in_three_slabs(xs, torch_gpu, dt, threads):
    """threads = 2: each share is a slab and a bit of its own, and the second starts past the first slab"""
    d = bc.desc(1, 1, N=3, C=16 * (ITEMS // 3), ops=13, dt=dt, threads=threads)
    name = "limits_%s_n" % ("f32" if dt == bc.F32 else "bf16")
    if name not in _data:
        _data[name] = bc.expected(name, d)
    want = _data[name]
    layer = Layer(xs, torch_gpu, d, want)
    assert layer.h.work() == ITEMS and (threads == 1 or layer.h.share(1)[0] > SLAB)
    for kind in (bc.FWD, bc.BWD):
        for tid in reversed(range(threads)):
            assert 0 == layer.run(kind, 0, tid)
        layer.check(ALL_KEYS, after_fwd(want) if kind == bc.FWD else want)
    layer.close()
