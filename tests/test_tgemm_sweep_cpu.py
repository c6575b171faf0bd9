"""The seeded sweep of tests/tgemm_sweep_common.py (sweep_cases) without a GPU: the expected bits of the tiled GEMM and of the GEMM
with 16-bit inputs -- the oracle's fma chains and lowp_gemm_common.reference, what the GPU tests of both families trust -- against
a float64 product whose bounds are derived in tgemm_sweep_common.contract64, on 72 cases over six kinds: fp32, fp64, i16 -> i32,
i16 -> f32, bf16 exact and bf16 fast. The operands are taken apart here by the column-major index formula with each case's own
leading dimensions and offsets, not by lowp_gemm_common.op or the reshapes of test_tgemm_gpu.Case, so for odd k and the three
transposed forms, where the oracle of the 16-bit kinds computes nothing, lowp_gemm_common.reference is held to an independent
definition. With a census of what the dealt and drawn set holds, the partition rule on the drawn extents, and a list of mistakes
that the comparison must reject.

The assertion is error <= bound, derived and not measured. The tests print the worst error / bound per kind, the census and
which cases reject each mistake; DESIGN.md 8v records them."""
import numpy as np
import pytest

import tgemm_sweep_common as ts

CASES = ts.sweep_cases()
FAST = sorted(name for name, c in CASES.items() if c["kind"] == "bf16fast")


def census(cases):
    """what the sweep is for -> the number of cases that have it"""
    geo = ts.geometry()
    count = {}

    def add(key, hit):
        count[key] = count.get(key, 0) + (1 if hit else 0)
    for c in cases.values():
        kind, m, n, k = c["kind"], c["m"], c["n"], c["k"]
        D, BK, TS = geo[kind]
        add(kind + ": k below D", k < D)
        add(kind + ": k = BK", k == BK)
        add(kind + ": k = 2 BK", k == 2 * BK)
        if kind == "f64":
            for t in range(1, D):
                add("f64: chunk multiple plus tail %d" % t, ts.tail_of(kind, k) == t)
        else:
            add(kind + ": chunk multiple plus tail", ts.tail_of(kind, k) > 0)
        for v in (() if TS is None else (TS - 1, TS, TS + 1)):
            add("%s: m or n = %d" % (kind, v), v in (m, n))
        for v in (63, 64, 65):
            add("m or n = %d" % v, v in (m, n))
        add("m or n above 128", max(m, n) > 128)
        add("m or n above 256", max(m, n) > 256)
        add("three different pads", 3 == len(set(c["pads"])))
        for w, x in enumerate("ABC"):
            add("odd offset of " + x, 1 == c["offs"][w] % 2)
        mt, nt = ts.task_grid(m, n, c["nthreads"])
        add("more tasks than tiles", c["nthreads"] > -(-m // ts.TILE) * -(-n // ts.TILE))
        add("task grid cut both ways", mt > 1 and nt > 1)
        add("pageable C, more than one task with work", c["mem"][2] == "pageable" and mt * nt > 1)
        for t in ("TN", "NT", "TT"):
            add("bf16fast %s, k above one chunk" % t, kind == "bf16fast" and c["trans"] == t and k > BK)
    return count


def every_value_occurs(cases):
    """12 cases of each kind; every pair of kind and transposes three times, with both betas; every memory kind for every operand,
    and at least half of the cases with all operands on the device; every pad, offset and number of tasks"""
    per = len(cases) // len(ts.KINDS)
    for kind in ts.KINDS:
        mine = [c for c in cases.values() if c["kind"] == kind]
        if len(mine) != per:
            return False
        for t in ts.TRANS:
            if sorted({c["beta"] for c in mine if c["trans"] == t}) != [0, 1] or sum(c["trans"] == t for c in mine) != per // 4:
                return False
    return all({c["mem"][w] for c in cases.values()} == set(ts.MEMS) and {c["pads"][w] for c in cases.values()} == set(ts.PADS)
               and {c["offs"][w] for c in cases.values()} == set(range(8)) for w in range(3)) \
        and 2 * sum(c["mem"] == ("device",) * 3 for c in cases.values()) >= len(cases) \
        and {c["nthreads"] for c in cases.values()} == set(range(1, 8))


def census_passes(cases):
    return min(census(cases).values()) >= 2 and every_value_occurs(cases)


def test_the_drawn_set_is_worth_running(xs):
    assert len(CASES) == ts.SWEEP_CASES == 72 and [CASES[n]["kind"] for n in sorted(CASES)] == list(ts.KINDS) * 12
    assert all(1 <= c["m"] <= ts.MAX_MN and 1 <= c["n"] <= ts.MAX_MN and 1 <= c["k"] <= ts.MAX_K for c in CASES.values())
    assert all(sorted(c["order"]) == list(range(c["nthreads"])) for c in CASES.values())
    # the constants the drawing reads from the kernel files are those the library answers and DESIGN.md 8c / 8d state
    assert ts.TILE == xs.lib().libxsmm_amd_gemm_tile()
    assert ts.geometry() == {"f32": (2, 32, 32), "f64": (4, 16, 16), "i16i32": (2, 32, None), "i16f32": (2, 32, None), "bf16": (2, 64, 32), "bf16fast": (16, 64, 32)}
    counted = census(CASES)
    for key in sorted(counted):
        print("%-50s %d" % (key, counted[key]))
    assert census_passes(CASES), counted


def test_the_drawing_is_reproducible_and_the_seed_is_the_first_that_passes():
    ts.sweep_cases.cache_clear()
    try:
        assert ts.sweep_cases() == CASES
    finally:
        ts.sweep_cases.cache_clear()
    assert not any(census_passes(ts.sweep_cases_from(seed)) for seed in range(ts.SWEEP_SEED))


def test_partition_of_the_drawn_extents(xs):
    """libxsmm_amd_gemm_task on every drawn (m, n, nthreads): the rectangles are disjoint, cover C, lie on tile multiples, and are
    those of the restated rule that the census and the mistakes use (no device is needed)"""
    for c in CASES.values():
        m, n, nthreads = c["m"], c["n"], c["nthreads"]
        keep, h = xs.gemm_handle(xs.F32, xs.F32, "N", "N", m, n, 1)
        assert h
        cover = np.zeros((m, n), dtype=np.int32)
        for tid in range(nthreads):
            rc, rect = xs.gemm_task(h, tid, nthreads)
            assert rc == 0 and rect == ts.task_rect(m, n, tid, nthreads), (m, n, tid, nthreads)
            m0, m1, n0, n1 = rect
            if m0 == m1:
                assert rect == (0, 0, 0, 0)
                continue
            assert m0 < m1 <= m and n0 < n1 <= n and m0 % ts.TILE == 0 and n0 % ts.TILE == 0
            assert (m1 % ts.TILE == 0 or m1 == m) and (n1 % ts.TILE == 0 or n1 == n)
            cover[m0:m1, n0:n1] += 1
        assert (cover == 1).all(), (m, n, nthreads)


def held(name, ints=False):
    want = ts.expected(name, ints)
    assert ts.compare(name, want, ints) is None, ts.compare(name, want, ints)
    # the same bits from the operands taken apart by the index formula, multiplied tight and written back task by task
    assert ts.restated(name, ints).tobytes() == want.tobytes()
    if CASES[name]["kind"] == "bf16fast" and not ints:  # the exact chain lies inside the fast mode's wider bound as well
        assert ts.compare(name, want, ints, fast=True) is None


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_bits_meet_the_float64_contract(orc, name):
    held(name)


@pytest.mark.parametrize("name", FAST)
def test_expected_bits_of_the_integer_operands_are_exact(orc, name):
    a, b, c = ts.operands(name, True)
    assert not any(np.any(x.view(np.uint16 if x.dtype == np.uint16 else np.uint32) == (0x8000 if x.dtype == np.uint16 else 0x80000000)) for x in (a, b, c)), "-0.0"
    held(name, True)


def test_worst_ratios(orc):
    """the worst error / bound of the expected bits per kind"""
    worst = {}
    for name in sorted(CASES):
        kind = CASES[name]["kind"]
        worst[kind] = max(worst.get(kind, 0.0), ts.ratio_of(name, ts.expected(name)))
    for kind in ts.KINDS:
        print("%-10s worst error / bound %.3g" % (kind, worst[kind]))
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("wrong", ts.WRONG)
def test_the_bounds_bite(orc, wrong):
    """the restated product with one mistake is rejected by at least one drawn case"""
    caught = [name for name in sorted(CASES) if ts.compare(name, ts.restated(name, wrong=wrong)) is not None]
    print("%s: rejected by %d cases: %s" % (wrong, len(caught), " ".join(n.split("_")[1] for n in caught)))
    assert caught
