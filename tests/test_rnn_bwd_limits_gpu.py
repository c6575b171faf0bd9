"""The backward pass of the RNN cell layer past the grid limits of kernels/rnn_bwd.hip: more steps than one dx launch takes
(gridDim.z, 65535) and a share of more row tiles than a grid has (gridDim.y, 65535 tiles of 64 rows). Bit for bit against the
restatement of tests/rnn_bwd_common.py, as everywhere."""
import functools

import numpy as np
import pytest

import rnn_common as rc
import rnn_bwd_common as rb

pytestmark = pytest.mark.gpu

PERIOD = 2979  # rows of the seeded block the many-rows case repeats: 4194432 = 1408 * 2979, and no multiple of 64


@functools.lru_cache(maxsize=None)
def steps_expected():
    d = rb.LIMIT_CASES["steps_relu"]
    t = rb.inputs("steps_relu", d)
    return t, rb.backward(rc.Handle(d), t, rb.BWD)


def bind(xs, handle, torch, arrays):
    """the tensors of a simple cell's BWD on the device; returns (device tensors by key, tensor handles)"""
    L = xs.lib()
    dev = {key: torch.from_numpy(a).cuda() for key, a in arrays.items()}
    tensors = [xs.rnn_bind_new(handle, dict(rc.IN_TYPE, **rb.GRAD_TYPE)[key], m) for key, m in dev.items() if key != "z"]
    assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, rb.BWD, xs.dptr(dev["z"]))
    return dev, tensors


def test_more_steps_than_one_dx_launch(xs, torch_gpu):
    """T = 65537 on a ReLU cell of 2 x 3 x 5: the recurrence is 65537 launches, dx of all steps two (65535 steps and 2)"""
    L = xs.lib()
    d = rb.LIMIT_CASES["steps_relu"]
    t, out = steps_expected()
    handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], 1)
    assert handle and 0 == st
    dev, tensors = bind(xs, handle, torch_gpu, dict(r=t["r"], w=t["w"], dh=t["dh"], z=t["z"], dx=rc.filled(out["dx"].shape)))
    before = L.libxsmm_amd_launch_count()
    assert 0 == xs.rnn_execute(handle, rb.BWD)
    assert 65537 + 2 == rb.launches(d["cell"], rb.BWD, d["max_T"]) == L.libxsmm_amd_launch_count() - before
    torch_gpu.cuda.synchronize()
    got = dev["dx"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), out["dx"].view(np.uint32))
    assert np.any(got[65535:] != 0) and np.any(got[:65535] != 0)
    for key in ("r", "w", "dh", "z"):
        assert dev[key].cpu().numpy().tobytes() == t[key].tobytes(), key
    for tensor in tensors:
        L.libxsmm_dnn_destroy_tensor(tensor)
    assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)


def test_a_share_of_too_many_row_tiles_is_refused_whole_and_two_shares_pass(xs, torch_gpu):
    """N = 4194432 = 65538 tiles of 64 rows, C = K = 8, one step: with threads = 1 BWD is refused before anything is launched or
    written; with threads = 2 each share is 32769 tiles and both run. The rows repeat a seeded block of 2979 rows (rows are independent
    in BWD), whose gradient is the restatement's."""
    L = xs.lib()
    d = rb.LIMIT_CASES["manyrows_relu"]
    assert d["N"] % PERIOD == 0 and PERIOD % 64 != 0 and d["N"] // 64 == 65538 and d["N"] // d["bn"] == 2
    dp = dict(d, N=PERIOD, bn=PERIOD)
    tp = rb.inputs("manyrows_relu", dp)
    want = rb.backward(rc.Handle(dp), tp, rb.BWD)["dx"]
    reps = d["N"] // PERIOD
    rows = lambda a: np.ascontiguousarray(np.tile(a, (1, reps, 1)))  # noqa: E731
    arrays = dict(r=tp["r"], w=tp["w"], dh=rows(tp["dh"]), z=rows(tp["z"]))
    for threads in (1, 2):
        handle, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], threads)
        assert handle and 0 == st
        dev, tensors = bind(xs, handle, torch_gpu, dict(arrays, dx=rc.filled((1, d["N"], d["C"]))))
        before = L.libxsmm_amd_launch_count()
        if threads == 1:
            assert rc.ERR_GENERAL == xs.rnn_execute(handle, rb.BWD)
            assert before == L.libxsmm_amd_launch_count()
            torch_gpu.cuda.synchronize()
            assert bool((dev["dx"].view(torch_gpu.int32) == -1).all())
        else:
            assert 0 == xs.rnn_execute(handle, rb.BWD, 0, 1) == xs.rnn_execute(handle, rb.BWD, 0, 0)
            assert 2 * rb.launches(d["cell"], rb.BWD, 1) == L.libxsmm_amd_launch_count() - before
            torch_gpu.cuda.synchronize()
            got = dev["dx"].cpu().numpy().reshape(reps, PERIOD, d["C"])
            assert np.array_equal(got.view(np.uint32), np.broadcast_to(want.reshape(1, PERIOD, d["C"]).view(np.uint32), got.shape))
            for key in ("dh", "z"):
                assert bool((dev[key] == torch_gpu.from_numpy(arrays[key]).cuda()).all()), key
        for tensor in tensors:
            L.libxsmm_dnn_destroy_tensor(tensor)
        assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)
        del dev
