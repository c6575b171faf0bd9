"""The seeded descriptor sweep of tests/fc_common.py (sweep_cases) without a GPU: the expected tensors of the fully-connected
layer -- the CPU oracle's fma chains on the plain matrices, put into the tensors' layouts by fc_common's blocking -- against three
float64 matrix products (fc_common.contract64, whose docstring derives the bounds) on 32 drawn descriptors: half in the packed
format with block factors that divide their dimension or do not (the handle then answers WARN_* and takes the whole dimension, and
the case runs all the same: on the named cases that arithmetic is a status only), half in the custom format in fp32 and bf16-in /
fp32-out, with N on either side of both tile sizes. The tensors are taken apart here by the index formula of each layout
(DESIGN.md 8g), not by fc_common's reshapes, so the blocking is held to an independent definition too. With a census of what the
drawn set holds and a list of mistakes that the comparison must reject.

The assertion is error <= bound, derived and not measured. Each test prints the worst error / bound per tensor; DESIGN.md 8t
records them."""
import numpy as np
import pytest

import fc_common as fc
import quant_common as qc

CASES = fc.sweep_cases()
KINDS = (fc.FWD, fc.BWD, fc.UPD)


def misfit(block, n):
    return block <= 0 or n % block != 0


def census(cases):
    """what the sweep is for -> the number of cases that have it"""
    n = dict.fromkeys(("non-dividing bn", "non-dividing bc", "non-dividing bk", "N above 64", "N above 128", "K = 1000", "mixed type", "uneven shares",
                       "more shares than work"), 0)
    for d in cases.values():
        h = fc.Handle(d)
        n["non-dividing bn"] += h.packed and misfit(d["bn"], d["N"])
        n["non-dividing bc"] += h.packed and misfit(d["bc"], d["C"])
        n["non-dividing bk"] += h.packed and misfit(d["bk"], d["K"])
        n["N above 64"] += d["N"] > 64
        n["N above 128"] += d["N"] > 128
        n["K = 1000"] += d["K"] == 1000
        n["mixed type"] += h.mixed
        n["uneven shares"] += d["threads"] > 1 and any(h.work(kind) % d["threads"] != 0 for kind in KINDS)
        n["more shares than work"] += any(d["threads"] > h.work(kind) for kind in KINDS)
    return n


def every_value_occurs(cases):
    """every value of every drawn field with few values (N, and C, K and the block factors of the packed format, have more values
    than there are cases: the census counts what they are drawn for)"""
    custom = [d for d in cases.values() if d["buffer_format"] == fc.FMT_LIBXSMM]
    return {d["C"] for d in custom} == set(fc.SWEEP_C) and {d["K"] for d in custom} == set(fc.SWEEP_K) \
        and {d["datatype_in"] for d in custom} == {fc.F32, fc.BF16} and {d["threads"] for d in cases.values()} == set(range(1, 6))


def census_passes(cases):
    return min(census(cases).values()) >= 3 and every_value_occurs(cases)


def test_the_drawn_set_is_worth_running():
    assert len(CASES) == 32 == len({tuple(d.items()) for d in CASES.values()}) and sorted(CASES) == ["sweep_%02d" % i for i in range(32)]
    assert [fc.Handle(CASES[n]).packed for n in sorted(CASES)] == [True, False] * 16
    assert all(fc.Handle(d).f32 for d in CASES.values() if d["buffer_format"] != fc.FMT_LIBXSMM)
    counted = census(CASES)
    print(counted)
    assert census_passes(CASES), counted
    # each of the three warnings is what some handle answers, and a zero block occurs
    assert {fc.Handle(d).status for d in CASES.values()} >= {fc.SUCCESS, fc.WARN_N, fc.WARN_C, fc.WARN_K}
    assert any(0 in (d["bn"], d["bc"], d["bk"]) for d in CASES.values() if d["buffer_format"] != fc.FMT_LIBXSMM)


def test_the_drawing_is_reproducible_and_the_seed_is_the_first_that_passes():
    fc.sweep_cases.cache_clear()
    try:
        assert fc.sweep_cases() == CASES
    finally:
        fc.sweep_cases.cache_clear()
    assert not any(census_passes(fc.sweep_cases_from(seed)) for seed in range(fc.SWEEP_SEED))


def plain_of(d, flat, rows, cols):
    """a tensor's flat contents as the plain matrix [rows][cols] (rows, cols: two of 'n', 'c', 'k'), by the index formula of its
    layout: packed activations [N/bn][F/b][bn][b], custom ones [N][F], filters [K/bk][C/bc][bc][bk] in either format (custom: bc =
    16, bk = 16, or 10 where K = 1000); a block factor that does not divide its dimension is the whole dimension"""
    size = {"n": d["N"], "c": d["C"], "k": d["K"]}
    if d["buffer_format"] == fc.FMT_LIBXSMM:
        block = {"n": 1, "c": 16, "k": 10 if d["K"] == 1000 else 16}
    else:
        block = {key: (size[key] if misfit(d["b" + key], size[key]) else d["b" + key]) for key in "nck"}
    i, j = np.arange(size[rows])[:, None], np.arange(size[cols])[None, :]
    if rows == "k":  # a filter: (k, c)
        bk, bc = block["k"], block["c"]
        at = ((i // bk * (d["C"] // bc) + j // bc) * bc + j % bc) * bk + i % bk
    elif d["buffer_format"] == fc.FMT_LIBXSMM:
        at = i * size[cols] + j
    else:            # a packed activation: (n, f)
        bn, b = block["n"], block[cols]
        at = ((i // bn * (size[cols] // b) + j // b) * bn + i % bn) * b + j % b
    assert np.array_equal(np.sort(at.reshape(-1)), np.arange(flat.size)), "the layout is no permutation of the matrix"
    return np.asarray(flat)[at]


def compare(d, want, tensors, label):
    """None, or what differs: y, dx and dw against contract64; the inputs against what was seeded"""
    x, w, dy = want["inputs"]
    mixed = d["datatype_in"] == fc.BF16
    f32 = lambda a: qc.bf16_widen(a).reshape(a.shape) if a.dtype == np.uint16 else a  # noqa: E731
    for t, rows, cols, plain in ((fc.REG_IN, "n", "c", x), (fc.REG_FIL, "k", "c", w), (fc.GRAD_OUT, "n", "k", dy)):
        if not np.array_equal(f32(plain_of(d, tensors[t], rows, cols)), plain):
            return "input tensor %d is not the seeded matrix" % t
    for key, t, rows, cols in (("y", fc.REG_OUT, "n", "k"), ("dx", fc.GRAD_IN, "n", "c"), ("dw", fc.GRAD_FIL, "k", "c")):
        value, bound, compared = want[key]
        got = f32(plain_of(d, tensors[t], rows, cols)).astype(np.float64)
        if got.dtype != np.float64 or not np.all(np.isfinite(got)) or (mixed and key != "y") != (tensors[t].dtype == np.uint16):
            return "%s is not finite, or of the wrong type" % key
        err = np.abs(got - value)
        if label:
            print("%s %s: worst error / bound %.3g" % (label, key, float(np.max((err / np.where(bound > 0, bound, 1))[bound > 0], initial=0))))
        if not np.all(err[compared] <= bound[compared]):
            return "%s: %d elements beyond their bound" % (key, int(np.sum(err > bound)))
    return None


def contract_of(name):
    d = CASES[name]
    x, w, dy = fc.plain_inputs(name, d)
    return dict(fc.contract64(d, x, w, dy), inputs=(x, w, dy))


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_tensors_agree_with_float64_products(orc, name):
    h, _, tensors = fc.sweep_expected(name)
    assert compare(CASES[name], contract_of(name), tensors, name) is None


@pytest.mark.parametrize("wrong", fc.WRONG)
def test_the_bounds_bite(orc, wrong):
    """a handle restatement with one mistake is rejected by at least one drawn case (a blocking that no longer fits its tensor makes
    numpy refuse the reshape, or divide by a zero block: that counts as rejected)"""
    caught = []
    for name in sorted(CASES):
        d = CASES[name]
        want = contract_of(name)
        try:
            tensors = fc.tensors(fc.Handle(d, wrong=wrong), *want["inputs"])
            rejected = compare(d, want, tensors, None) is not None
        except (ValueError, ZeroDivisionError, AssertionError):
            rejected = True
        if rejected:
            caught.append(name)
    print("%s: rejected by %d cases: %s" % (wrong, len(caught), " ".join(caught)))
    assert caught
    assert all(fc.Handle(CASES[name]).packed for name in caught)
