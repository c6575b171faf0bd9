"""Packed kernels on hostile values: three packs of the benign matrices of tests/packed_common.py in which lanes 1, VLEN / 2 and VLEN - 1
of every pack hold matrices of NaN, Inf, zero pivots and signed zeros (specials), subnormal pivots and results (underflow), chains that
pass the largest finite number (overflow) -- tests/hostile_operands.py:packed_hostile. Padding and guards hold a NaN with a payload.

A lane owns a matrix: the benign lanes must come out bit for bit as the oracle (oracle/xsmm_oracle.c, xo_packed_*) has them, whatever
their neighbours hold. The hostile lanes are held to same_values(): NaN exactly where the oracle has NaN, its bits everywhere else,
signed zeros and subnormals included (the sign and payload of a NaN are not compared). Every case runs in both forms
(LIBXSMM_AMD_PACKED_FORM), with and without the register-resident text (LIBXSMM_AMD_PACKED_RESIDENT), and once with neither set.
tests/test_packed_chain_cpu.py holds every case against its conditions on the oracle alone, so that each comparison compares something."""
import numpy as np
import pytest

import hostile_operands as ho
import packed_common as pc

pytestmark = pytest.mark.gpu

VARIANTS = [{"LIBXSMM_AMD_PACKED_FORM": f, "LIBXSMM_AMD_PACKED_RESIDENT": r} for f in ("1", "2") for r in ("1", "0")] + [{}]


def execute(xs, torch, case, fn):
    """the case through libxsmm_amd_packed_execute_batch -> (buffers before, buffers after)"""
    before = case.buffers(xs)
    dev = {name: torch.from_numpy(x).cuda() for name, x in before.items()}
    a, b, c, sa, sb, sc = pc.call_args(case, {name: t.data_ptr() for name, t in dev.items()})
    torch.cuda.synchronize()
    assert 0 == xs.lib().libxsmm_amd_packed_execute_batch(fn, a, b, c, case.nmat // pc.width(case.dtype))
    assert 0 == xs.lib().libxsmm_amd_synchronize()
    return before, {name: t.cpu().numpy() for name, t in dev.items()}


@pytest.mark.parametrize("op,fmt,size", ho.packed_cases())
def test_hostile_lanes_stay_in_their_lanes(xs, orc, torch_gpu, monkeypatch, op, fmt, size):
    ho.assert_environment(orc)
    base = ho.packed_case(op, fmt, size)
    fn = base.dispatch(xs)
    lanes = ho.packed_hostile_lanes(base)
    benign = np.ones(base.nmat, bool)
    benign[lanes] = False
    bits = np.uint32 if base.dtype == np.float32 else np.uint64
    for kind in ho.KINDS:
        case = ho.packed_hostile(base, kind)
        want_buf = case.chain(xs, orc)[case.written]
        want = case.result(xs, want_buf)
        valid = case.valid_mask(xs, case.written)
        for env in VARIANTS:
            for name in ("LIBXSMM_AMD_PACKED_FORM", "LIBXSMM_AMD_PACKED_RESIDENT"):
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            before, after = execute(xs, torch_gpu, case, fn)
            if "LIBXSMM_AMD_PACKED_FORM" in env:
                # (the three operands of a pack of pgemm 16 x 16 x 16 take 48 KiB and their padding: beyond the LDS budget, form 2 serves them
                # whatever is asked for)
                lds = env["LIBXSMM_AMD_PACKED_FORM"] == "1" and not (op == pc.PGEMM and size == 16)
                assert xs.last_kernel().endswith("_lds" if lds else "_direct"), xs.last_kernel()
            what = (case, kind, env)
            msg = case.untouched(xs, before, after)
            assert msg is None, (what, msg)
            got = case.result(xs, after[case.written])
            same = got[benign].view(bits) == want[benign].view(bits)
            assert same.all(), (what, "%d elements of the benign lanes differ from the oracle" % int(np.count_nonzero(~same)))
            assert ho.same_values(got[lanes], want[lanes]), (what, "hostile lanes: (NaN positions, other bits) that differ: %r" % (ho.differences(got[lanes], want[lanes]),))
            # no element is left out: the two groups are all matrices, and the matrices are all of the buffer that is not canary
            assert benign.sum() + len(lanes) == case.nmat and got.size == int(valid.sum())
            assert ho.same_values(after[case.written][valid], want_buf[valid])
    for name in ("LIBXSMM_AMD_PACKED_FORM", "LIBXSMM_AMD_PACKED_RESIDENT"):
        monkeypatch.delenv(name, raising=False)
