"""The seeded descriptor sweep of tests/pool_common.py (sweep_cases) without a GPU: the restatement of the pooling layer, which
tests/test_pool_cpu.py holds against captured reference output on the named cases only, against a float64 definition of the
contract (pool_common.contract64, whose docstring derives the bounds) on 48 drawn descriptors that combine what the named cases
take one at a time -- among them paddings that reach the window's extent, so that whole windows lie in the padding; a census of
what the drawn set holds; torch's own pooling and its autograd as a second opinion on the float64 side; and a list of mistakes
that the comparison must reject.

The assertion is error <= bound with bounds that are derived, not measured: MAX FWD and the mask are equalities, the sums carry
gamma(roundings) * sum|terms| (every rounding of relative size 2^-24, compounded, so the bound is no first-order estimate), a bf16
store adds its cut of below 2^-7. Each test prints the worst error / bound per tensor; DESIGN.md 8t records them."""
import numpy as np
import pytest

import pool_common as pc

CASES = pc.sweep_cases()
GROUP = {True: 64, False: 128}  # pixels of a work-group: 256 threads, a 16-byte piece each (kernels/pool.hip)


def census(cases):
    """what the sweep is for -> the number of cases that have it"""
    n = dict.fromkeys(("max f32", "max bf16", "avg f32", "avg bf16", "logical pad", "empty window", "clipped window", "holes", "u != v", "R != S",
                       "physical pad in", "physical pad out", "C = 24", "uneven shares", "more shares than items", "more than one work-group"), 0)
    for d in cases.values():
        h = pc.Handle(d)
        counts = pc.window_counts(h)
        n["%s %s" % ("max" if d["pooling_type"] == pc.MAX else "avg", "f32" if h.f32 else "bf16")] += 1
        n["logical pad"] += d["pad_h"] > 0 or d["pad_w"] > 0
        n["empty window"] += bool(np.any(counts == 0))
        n["clipped window"] += bool(np.any((counts > 0) & (counts < d["R"] * d["S"])))
        n["holes"] += d["u"] > d["R"] or d["v"] > d["S"]
        n["u != v"] += d["u"] != d["v"]
        n["R != S"] += d["R"] != d["S"]
        n["physical pad in"] += d["pad_h_in"] > 0 or d["pad_w_in"] > 0
        n["physical pad out"] += d["pad_h_out"] > 0 or d["pad_w_out"] > 0
        n["C = 24"] += d["C"] == 24
        n["uneven shares"] += d["threads"] > 1 and h.work() % d["threads"] != 0
        n["more shares than items"] += d["threads"] > h.work()
        n["more than one work-group"] += any(p > GROUP[h.f32] and p % GROUP[h.f32] != 0 for p in (h.ofh * h.ofw, d["H"] * d["W"]))
    return n


def every_value_occurs(cases):
    """every value of every drawn field (H and W: of the range most draws use; the wide range 17..40 is drawn about six times,
    and "more than one work-group" counts what it is for)"""
    fields = (("H", range(1, 13)), ("W", range(1, 13)), ("R", range(1, 5)), ("S", range(1, 5)), ("u", range(1, 5)), ("v", range(1, 5)),
              ("pad_h", range(4)), ("pad_w", range(4)), ("pad_h_in", range(3)), ("pad_w_in", range(3)), ("pad_h_out", range(3)),
              ("pad_w_out", range(3)), ("N", range(1, 6)), ("C", pc.SWEEP_CHANNELS), ("pooling_type", (pc.MAX, pc.AVG)),
              ("datatype_in", (pc.F32, pc.BF16)), ("threads", range(1, 6)))
    return all({d[key] for d in cases.values()} - set(range(17, 41) if key in "HW" else ()) == set(values) for key, values in fields)


def census_passes(cases):
    counted = census(cases)
    return all(v >= (8 if k[:3] in ("max", "avg") else 6) for k, v in counted.items()) and every_value_occurs(cases)


def test_the_drawn_set_is_worth_running():
    assert len(CASES) == 48 == len({tuple(d.items()) for d in CASES.values()}) and sorted(CASES) == ["sweep_%02d" % i for i in range(48)]
    bound = {pc.MAX: pc.BINDABLE, pc.AVG: pc.BINDABLE[:4]}
    assert all(pc.Handle(d).status == pc.SUCCESS == pc.Handle(d).execute_status(pc.BWD, bound[d["pooling_type"]]) for d in CASES.values())
    assert all(pc.window_counts(pc.Handle(d)).any() for d in CASES.values())
    counted = census(CASES)
    print(counted)
    assert census_passes(CASES), counted
    assert any(d["H"] >= 17 for d in CASES.values())
    # a padding at or above the window's extent is what leaves a window empty
    assert sum(d["pad_h"] >= d["R"] or d["pad_w"] >= d["S"] for d in CASES.values()) >= 6


def test_the_drawing_is_reproducible_and_the_seed_is_the_first_that_passes():
    pc.sweep_cases.cache_clear()
    try:
        assert pc.sweep_cases() == CASES
    finally:
        pc.sweep_cases.cache_clear()
    assert not any(census_passes(pc.sweep_cases_from(seed)) for seed in range(pc.SWEEP_SEED))


def compare(h, t, want, label):
    """None, or what differs: every tensor of t that a pass writes against contract64, and the bytes that no pass writes"""
    d = h.d
    for key in ("out", "mask", "din"):
        if key not in want:
            continue
        value, bound, compared = want[key]
        got = pc.interior(h, key, t[key]).astype(np.float64)
        if not np.all(np.isfinite(got)):
            return "%s is not finite" % key
        err = np.abs(got - value)
        if label:
            scale = float(np.max(np.abs(value)))
            print("%s %s: worst error / bound %.3g, worst error %.3g (%.3g of max|tensor|)" % (
                label, key, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), initial=0)), float(err.max()),
                float(err.max()) / scale if scale else 0))
        if not np.all(err[compared] <= bound[compared]):
            return "%s: %d elements beyond their bound" % (key, int(np.sum(err > bound)))
    if np.any(pc.interior(h, "din", t["din"])[want["unreached"]].view(np.uint32) != 0):
        return "an element of dinput that no term reaches is not +0.0"
    # what no pass writes keeps its start bytes: the physical padding of either destination (the mask's sentinels are compared above)
    rim = np.ones(h.out_shape(), dtype=bool)
    rim[:, d["pad_h_out"]:d["pad_h_out"] + h.ofh, d["pad_w_out"]:d["pad_w_out"] + h.ofw, :] = False
    if not np.all(np.asarray(t["out"])[rim].view(np.uint8) == 0xff):
        return "the padding of the output was written"
    rim = np.ones(h.in_shape(), dtype=bool)
    rim[:, d["pad_h_in"]:d["pad_h_in"] + d["H"], d["pad_w_in"]:d["pad_w_in"] + d["W"], :] = False
    if not np.all(np.asarray(t["din"])[rim].view(np.uint8) == 0xff):
        return "the padding of dinput was written"
    return None


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_the_float64_contract(name):
    h = pc.Handle(CASES[name])
    t = pc.sweep_expected(name)
    want = pc.contract64(h, t)
    if not h.f32:  # a bf16 store cuts towards zero: the magnitude stays within the fp32 part of the bound
        for key in ("din",) if CASES[name]["pooling_type"] == pc.MAX else ("out", "din"):  # (MAX FWD is an equality)
            value, bound, _ = want[key]
            fp32_part = (bound - pc.BF16_CUT * np.abs(value)) / (1 + pc.BF16_CUT)
            assert np.all(np.abs(pc.interior(h, key, t[key]).astype(np.float64)) <= np.abs(value) + fp32_part * (1 + 2.0 ** -40))
    assert compare(h, t, want, name) is None
    if CASES[name]["pooling_type"] == pc.MAX:
        empty = np.broadcast_to((pc.window_counts(h) == 0)[None, :, :, None], t["mask"].shape)
        assert np.all(t["mask"][empty] == pc.SENTINEL) and np.all(t["mask"][~empty] >= 0)
        lowest = np.float32(-pc.FLT_MAX) if h.f32 else pc.widen(np.uint16(0xff7f))
        assert np.all(pc.interior(h, "out", t["out"])[empty] == lowest)


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_the_bounds_bite(wrong):
    """a restatement with one mistake is rejected by at least one drawn case"""
    caught = []
    for name in sorted(CASES):
        d = CASES[name]
        h = pc.Handle(d)
        good = pc.sweep_expected(name)
        t = dict(good, out=good["out"].copy(), mask=None if good["mask"] is None else np.full_like(good["mask"], pc.SENTINEL))
        t["out"].view(np.uint8)[...] = 0xff
        pc.forward(h, good["x"], t["out"], t["mask"], wrong=wrong)
        if compare(h, t, pc.contract64(h, good), None) is not None:
            caught.append(name)
    print("%s: rejected by %d cases: %s" % (wrong, len(caught), " ".join(caught)))
    assert caught


def torch_accepts(d):
    """torch's own argument checks: a padding of at most half the window"""
    return d["pad_h"] <= d["R"] // 2 and d["pad_w"] <= d["S"] // 2


def test_torch_accepts_enough_of_the_set():
    assert sum(torch_accepts(d) for d in CASES.values()) >= 12


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if torch_accepts(CASES[n])])
def test_float64_contract_agrees_with_torch(name):
    """max_pool2d / avg_pool2d(count_include_pad=True) in float64 on the CPU, and their gradients from autograd, against
    contract64's values. MAX FWD and the winning index are equalities. The sums agree to float64 rounding: both sides add the
    same at most 16 terms, in another order, so they differ by at most 2 * 16 * 2^-53 * sum|terms| <= 2^-48 * sum|terms|; the
    tolerance is 2^-44 * max|tensor| (sum|terms| <= 16 * max|tensor|)."""
    import torch
    import torch.nn.functional as F
    d = CASES[name]
    h = pc.Handle(d)
    t = pc.sweep_expected(name)
    want = pc.contract64(h, t)
    plain = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))  # noqa: E731 ([item][16][rows][columns])
    x = plain(pc.interior(h, "din", t["x"]).astype(np.float64)).requires_grad_(True)
    g = plain(pc.interior(h, "out", t["dout"]).astype(np.float64))
    window, stride, pad = (d["R"], d["S"]), (d["u"], d["v"]), (d["pad_h"], d["pad_w"])
    if d["pooling_type"] == pc.MAX:
        out, index = F.max_pool2d(x, window, stride, pad, return_indices=True)
    else:
        out = F.avg_pool2d(x, window, stride, pad, count_include_pad=True)
    assert tuple(out.shape[2:]) == (h.ofh, h.ofw)
    out.backward(g)
    back = lambda a: a.detach().numpy().transpose(0, 2, 3, 1)  # noqa: E731
    tol = lambda a: 2.0 ** -44 * float(np.max(np.abs(a)))  # noqa: E731
    if d["pooling_type"] == pc.MAX:
        assert np.array_equal(back(out), want["out"][0])
        assert np.array_equal(back(index), want["mask"][0] // 16)
    else:
        assert np.max(np.abs(back(out) - want["out"][0])) <= tol(want["out"][0])
    assert np.max(np.abs(back(x.grad) - want["din"][0])) <= tol(want["din"][0])
