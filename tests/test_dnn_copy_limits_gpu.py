"""The DNN tensor copy past its grid clamps and past 2^32 bytes (kernels/dnn_copy.hip). Sizes come from the clamp table of
tests/test_dnn_copy_cpu.py, which holds it against the sources: two full trips of a grid-stride loop and an odd rest that is no
multiple of 64. The layouts are copies of real ones with other extents and tiny blocks; results are checked on the device with
torch (view / permute / equal), canaries included."""
import numpy as np
import pytest

import dnn_copy_common as dc
from test_dnn_copy_cpu import LIMITS

pytestmark = pytest.mark.gpu


def sized(name, rest):
    per_trip = LIMITS[name]["per_trip"]
    assert rest % 2 == 1 and rest % 64 != 0 and 0 < rest < per_trip
    return 2 * per_trip + rest


class DeviceBuffer:
    """n 4-byte elements on the device between two bands of canary bytes"""

    def __init__(self, torch, n, fill=None):
        self.torch = torch
        self.raw = torch.full((4 * n + 2 * dc.BAND,), dc.CANARY, dtype=torch.uint8, device="cuda")
        self.data = self.raw[dc.BAND:dc.BAND + 4 * n].view(torch.int32)
        if fill is not None:
            self.data.copy_(fill)
        self.ptr = self.raw.data_ptr() + dc.BAND

    def intact(self):
        return bool((self.raw[:dc.BAND] == dc.CANARY).all()) and bool((self.raw[-dc.BAND:] == dc.CANARY).all())


def round_trip(xs, torch, base, sizes, blocked_of, kernel):
    """copy-in and copy-out of a resized layout; blocked_of(plain int32 tensor) is the tensor the reference's loops give"""
    L = xs.lib()
    case = dc.Case(xs, base)
    layout = dc.resized(xs, case.layout, sizes)
    n = int(np.prod(sizes, dtype=np.int64))
    plain = DeviceBuffer(torch, n, torch.arange(n, dtype=torch.int32, device="cuda"))
    buf, back = DeviceBuffer(torch, n), DeviceBuffer(torch, n)
    tensor, st = xs.dnn_link_tensor(layout, buf.ptr)
    assert tensor and 0 == st
    before = L.libxsmm_amd_launch_count()
    assert 0 == L.libxsmm_dnn_copyin_tensor(tensor, plain.ptr, case.fmt)
    assert xs.last_kernel() == kernel.replace("*", "in") and before + 1 == L.libxsmm_amd_launch_count()
    assert torch.equal(buf.data, blocked_of(plain.data).reshape(-1)), "copy-in differs"
    assert 0 == L.libxsmm_dnn_copyout_tensor(tensor, back.ptr, case.fmt)
    assert xs.last_kernel() == kernel.replace("*", "out") and before + 2 == L.libxsmm_amd_launch_count()
    assert torch.equal(back.data, plain.data), "copy-out differs"
    assert plain.intact() and buf.intact() and back.intact(), "a canary was overwritten"
    st, plan = xs.dnn_copy_plan(layout, case.fmt)
    L.libxsmm_dnn_destroy_tensor(tensor)
    L.libxsmm_dnn_destroy_tensor_datalayout(layout)
    case.close()
    return plan


def act_blocked(sizes):
    bfm, W, H, fmb, N = sizes
    return lambda p: p.view(N, fmb, bfm, H, W).permute(0, 1, 3, 4, 2).contiguous()


def fil_blocked(sizes):
    bofm, bifm, S, R, ifmb, ofmb = sizes
    return lambda p: p.view(ofmb, bofm, ifmb, bifm, R, S).permute(0, 2, 4, 5, 3, 1).contiguous()


def test_tiles_past_the_grid(xs, torch_gpu):
    tiles = sized("dnn_copy_tiled", 39)  # 4135 = 5 * 827
    sizes = [4, 3, 3, tiles, 1]  # a block of 4 channels x 9 pixels is one tile
    plan = round_trip(xs, torch_gpu, "act_8x8", sizes, act_blocked(sizes), "dnn_copy_*_tiled")
    assert (tiles, LIMITS["dnn_copy_tiled"]["per_trip"]) == (plan[6], plan[7])
    sizes = [2, 3, 3, 1, 5, tiles // 5]  # blocks of 2 rows of 9 elements, five to a row of blocks
    plan = round_trip(xs, torch_gpu, "fil_fc_f32", sizes, fil_blocked(sizes), "dnn_copy_*_tiled")
    assert (tiles, LIMITS["dnn_copy_tiled"]["per_trip"]) == (plan[6], plan[7])


def test_flat_and_direct_past_the_grid(xs, torch_gpu):
    n = 2 * LIMITS["dnn_copy_flat"]["per_trip"] // 4 + 37  # bytes -> fp32 elements: two trips and 37 elements
    plan = round_trip(xs, torch_gpu, "bias_k40", [1, n], lambda p: p, "dnn_copy_flat")
    assert 0 == plan[0] and 2048 == plan[7]
    sizes = [1, 63, 17, 17, 59, 1]  # rows of 63 * 289 elements exceed the LDS budget; 59 of them are two trips and an odd rest
    n = int(np.prod(sizes))
    rest = n - 2 * LIMITS["dnn_copy_direct"]["per_trip"]
    assert 0 < rest < LIMITS["dnn_copy_direct"]["per_trip"] and 1 == rest % 2
    plan = round_trip(xs, torch_gpu, "fil_fc_f32", sizes, fil_blocked(sizes), "dnn_copy_*_direct")
    assert 0 == plan[5] and 2048 == plan[7]


def test_byte_offsets_past_2_to_the_32(xs, torch_gpu):
    """one fp32 activation of just over 2^30 elements: 16 channels of 8193 x 8192 pixels, both directions"""
    sizes = [16, 8192, 8193, 1, 1]
    assert 2 ** 30 < int(np.prod(sizes, dtype=np.int64)) < 2 ** 31
    plan = round_trip(xs, torch_gpu, "act_8x8", sizes, act_blocked(sizes), "dnn_copy_*_tiled")
    assert (1, 4, 1, 16, 8192 * 8193) == tuple(plan[:5]) and 2048 == plan[7]
    torch_gpu.cuda.empty_cache()
