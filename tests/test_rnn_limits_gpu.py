"""The RNN cell layer past the grid limits of kernels/rnn.hip (tests/launch_limits.py: rnn_steps, rnn_rows_per_share): more steps
than one launch of the split plan's bias + w.x takes, and more tiles of rows than one share may have. Bit for bit through
test_rnn_gpu.Layer.check like every other case: canary bands, inputs and scratch unchanged. tests/test_rnn_cpu.py
(test_the_limit_cases_are_what_they_are_for) holds the cases to their purpose."""
import os
import time

import numpy as np
import pytest

import launch_limits as ll
import rnn_common as rc
from test_rnn_gpu import Layer, clean_env, launches_of  # noqa: F401 (clean_env: the autouse fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("plan", ("split", "whole"))
def test_more_steps_than_one_launch_takes(xs, torch_gpu, plan):
    """steps_tanh, T = 65537: under split the launch of bias + w.x runs twice, the second time with two steps, x and the chains moved
    along by 65535 steps (T + 2 launches); under whole there are T launches. Every step of h and z against the restatement."""
    d = rc.LIMIT_CASES["steps_tanh"]
    t, out, _ = rc.limit_expected("steps_tanh")
    trip = ll.per_trip("rnn_steps")
    os.environ["LIBXSMM_AMD_RNN_PLAN"] = plan
    layer = Layer(xs, torch_gpu, d, t)
    assert trip < layer.h.T <= 2 * trip
    before, t0 = layer.count(), time.time()
    assert 0 == layer.run()
    torch_gpu.cuda.synchronize()
    print("steps_tanh, %s: %d launches in %.2f s" % (plan, layer.count() - before, time.time() - t0))
    assert layer.h.T + (2 if plan == "split" else 0) == launches_of(d, layer.h, plan == "split") == layer.count() - before
    layer.check(t, out)
    layer.close()


def test_more_row_tiles_than_one_share_may_have(xs, torch_gpu):
    """manyrows_relu, 65538 tiles of 64 rows, C = K = 1, one step. A handle with threads = 1 on the tensors answers _ERR_GENERAL under
    either plan, and every destination byte keeps its fill. A handle with threads = 2 on the same tensors runs its two shares of 32769
    tiles (blockIdx.y beyond 2^15) and gives the restatement's bits: z = fma(r, hp, fma(w, x, b)) row by row."""
    torch, L = torch_gpu, xs.lib()
    d = dict(rc.LIMIT_CASES["manyrows_relu"], threads=2)
    limit = ll.threshold("rnn_rows_per_share")
    t = rc.inputs("manyrows_relu", d)
    h, z = rc.forward_c1k1(t)
    layer = Layer(xs, torch, d, t)
    assert [n1 - n0 > limit for n0, n1 in rc.Handle(dict(d, threads=1)).shares()] == [True]
    assert [n1 - n0 > limit for n0, n1 in layer.h.shares()] == [False, False]
    # one share of all rows: refused
    single, st = xs.rnn_create(d["N"], d["C"], d["K"], d["max_T"], d["cell"], d["bn"], d["bc"], d["bk"], 1)
    assert single and st == 0
    tensors = [xs.rnn_bind_new(single, rc.IN_TYPE.get(key, rc.OUT_TYPE.get(key)), layer.view[key]) for key in rc.read(d["cell"]) + ("h",)]
    assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(single, rc.FWD, xs.dptr(layer.view["z"]))
    fill = {key: rc.filled(z.shape) for key in ("h", "z")}
    for plan in ("split", "whole"):
        os.environ["LIBXSMM_AMD_RNN_PLAN"] = plan
        assert rc.ERR_GENERAL == xs.rnn_execute(single, rc.FWD), plan
        layer.check(t, fill)
    os.environ.pop("LIBXSMM_AMD_RNN_PLAN")
    for tensor in tensors:
        L.libxsmm_dnn_destroy_tensor(tensor)
    assert 0 == L.libxsmm_dnn_destroy_rnncell(single)
    # two shares
    t0 = time.time()
    assert 0 == layer.run(rc.FWD, 0, 1)
    got = layer.result("h").reshape(-1)
    n0 = layer.h.shares()[1][0]
    assert np.all(got[:n0].view(np.uint32) == 0xffffffff) and got[n0:].tobytes() == h.reshape(-1)[n0:].tobytes()
    assert 0 == layer.run(rc.FWD, 0, 0)
    torch.cuda.synchronize()
    print("manyrows_relu: two shares in %.2f s" % (time.time() - t0))
    layer.check(t, {"h": h, "z": z})
    layer.close()
