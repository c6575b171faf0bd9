"""The seeded descriptor sweep of tests/conv_common.py (sweep_cases) without a GPU: the restatement of the three templates, which
tests/test_conv_cpu.py holds against captured reference output on the named cases only, against a float64 convolution on 48 drawn
descriptors that combine what the named cases take one at a time; and a census of what the drawn set holds.

The bound is derived, not measured: a chain of n fused multiply-adds in fp32 from a start value s ends within
n * 2^-24 * (sum|a * b| + |s|) of the exact sum (first order in 2^-24; n is the longest chain of the pass). UPD's per-image form
rounds ofh * ofw + N times per term instead, which is no more than n = N * ofh * ofw wherever N and the plane are above 1; with
N = 1 and overwrite its one add per image is exact. Where the pass ends in a ReLU the float64 side applies it too, and an
element whose float64 argument lies within the bound of 0 is left out (the two sides may fall on either side of it): fewer
than 2 % of any case's outputs, or sweep_cases would have drawn again. One deviation from a plain convolution is part of the
contract and of conv_common.naive64(gemm_form_copy=True): UPD's GEMM form with a stride."""
import numpy as np
import pytest

import conv_common as cc

CASES = cc.sweep_cases()


def census(cases):
    """what the sweep is for -> the number of cases that have it"""
    n = dict.fromkeys(("logical pad", "physical pad", "upd per image", "no filter transpose", "u != v", "R != S", "window leaves a rest",
                       "block other than 16", "uneven shares", "more than one tile"), 0)
    for d in cases.values():
        h = cc.Handle(d)
        padded = d["pad_h"] > 0 or d["pad_w"] > 0
        n["logical pad"] += padded and not h.physical
        n["physical pad"] += padded and h.physical
        n["upd per image"] += h.upd_per_image()
        n["no filter transpose"] += bool(d["options"] & cc.NO_FILTER_TRANSPOSE)
        n["u != v"] += d["u"] != d["v"]
        n["R != S"] += d["R"] != d["S"]
        n["window leaves a rest"] += (h.hp - d["R"]) % d["u"] != 0 or (h.wp - d["S"]) % d["v"] != 0
        n["block other than 16"] += h.ifmblock != 16 or h.ofmblock != 16
        n["uneven shares"] += d["threads"] > 1 and any(h.work(kind) % d["threads"] != 0 for kind in (cc.FWD, cc.BWD, cc.UPD))
        n["more than one tile"] += d["K"] > 128 or d["N"] * h.ofh * h.ofw > 128
    return n


def test_the_drawn_set_is_worth_running():
    assert len(CASES) == 48 == len({tuple(d.items()) for d in CASES.values()}) and sorted(CASES) == ["sweep_%02d" % i for i in range(48)]
    assert all(cc.Handle(d).status == cc.SUCCESS for d in CASES.values())
    counted = census(CASES)
    assert min(counted.values()) >= 6, counted
    # every value of every drawn field occurs
    for key, values in (("H", range(1, 10)), ("R", range(1, 5)), ("S", range(1, 5)), ("u", (1, 2, 3)), ("v", (1, 2, 3)), ("pad_h", (0, 1, 2)),
                        ("pad_w_out", (0, 1, 2)), ("N", (1, 2, 3)), ("C", cc.SWEEP_FEATURES), ("K", cc.SWEEP_FEATURES),
                        ("options", (0, 1, 8, 9)), ("fuse_ops", range(8)), ("threads", (1, 2, 3))):
        assert {d[key] for d in CASES.values()} == set(values), key


def test_the_drawing_is_reproducible():
    cc.sweep_cases.cache_clear()
    try:
        assert cc.sweep_cases() == CASES
    finally:
        cc.sweep_cases.cache_clear()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_float64_convolution(name):
    d = CASES[name]
    h = cc.Handle(d)
    t = cc.sweep_expected(name)
    want = cc.contract64(h, t)
    for key in ("out", "din", "dw"):
        value, bound, compared = want[key]
        got = cc.interior(h, key, t[key]).astype(np.float64)
        assert np.all(np.isfinite(got))
        err = np.abs(got - value)
        worst = float(np.max(err[compared] / np.where(bound[compared] > 0, bound[compared], 1), initial=0))
        print("%s %s: worst error / bound %.3g, left out %d of %d" % (name, key, worst, int(np.sum(~compared)), compared.size))
        assert np.mean(~compared) < cc.RELU_NEAR_ZERO
        assert np.all(err[compared] <= bound[compared]), (key, int(np.sum(err[compared] > bound[compared])))
        if key == "out" and d["fuse_ops"] & cc.FUSE_RELU:
            assert np.all(got[~compared] >= 0)
    # what no term of BWD reaches keeps its start bits: the seeded value, or +0.0 with overwrite
    idle = want["unreached"]
    start = np.zeros_like(t["din0"]) if h.overwrite else t["din0"]
    assert cc.same_bits(cc.interior(h, "din", t["din"])[idle], cc.interior(h, "din", start)[idle])
    # ... and the padding of the output, which no pass writes, and that of dinput, which physical BWD zeroes
    rim = np.ones(h.out_shape(), dtype=bool)
    rim[:, :, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :] = False
    assert cc.same_bits(np.asarray(t["out"])[rim], np.asarray(t["out0"])[rim])
    rim = np.ones(h.in_shape(), dtype=bool)
    rim[:, :, d["pad_h_in"]:d["pad_h_in"] + d["H"], d["pad_w_in"]:d["pad_w_in"] + d["W"], :] = False
    assert np.all(cc.bits(np.asarray(t["din"])[rim]) == 0)
