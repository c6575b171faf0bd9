"""Batch calls recorded inside a libxsmm_amd_defer_begin/end bracket leave in segments of independent calls (include/libxsmm_amd.h).
The rule that cuts them is a pure function, libxsmm_amd_merge_segments, and is checked here without a GPU: on hand-made tables of
address hulls, and against a restatement of the rule in Python on random tables.

hulls: per call (a_lo, a_hi, b_lo, b_hi, c_lo, c_hi), half-open byte ranges. A call joins the open segment unless its C meets the
A, B or C of a member, or its A or B meets the C of a member (the rule of the grouped pointer batches as well,
csrc/xsmm_batch.hpp: merge_segments, used by csrc/xsmm_gemm.cpp: try_grouped_pointer_batches); otherwise it opens a new segment.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(a, b, c):
    """hull entry from three (lo, hi) ranges"""
    return (a[0], a[1], b[0], b[1], c[0], c[1])


def restated(hulls):
    """the rule, restated"""
    meet = lambda x, y: x[0] < y[1] and y[0] < x[1]
    abc = lambda h: ((h[0], h[1]), (h[2], h[3]), (h[4], h[5]))
    first, seg, out = 0, 0, []
    for i, h in enumerate(hulls):
        ai, bi, ci = abc(h)
        for j in range(first, i):
            aj, bj, cj = abc(hulls[j])
            if meet(ci, aj) or meet(ci, bj) or meet(ci, cj) or meet(cj, ai) or meet(cj, bi):
                first, seg = i, seg + 1
                break
        out.append(seg)
    return (seg + 1 if hulls else 0), out


def test_all_disjoint_is_one_segment(xs):
    hulls = [call((1000 * i, 1000 * i + 100), (1000 * i + 100, 1000 * i + 300), (1000 * i + 300, 1000 * i + 900)) for i in range(27)]
    assert xs.merge_segments(hulls) == (1, [0] * 27)


def test_c_of_a_later_call_meets_a_of_an_earlier_one(xs):
    hulls = [call((0, 100), (100, 200), (200, 300)), call((400, 500), (500, 600), (50, 60))]
    assert xs.merge_segments(hulls) == (2, [0, 1])
    # ... and the other way round: a later call reads (as A, as B) what an earlier one writes
    hulls = [call((0, 100), (100, 200), (200, 300)), call((250, 260), (500, 600), (700, 800))]
    assert xs.merge_segments(hulls) == (2, [0, 1])
    hulls = [call((0, 100), (100, 200), (200, 300)), call((400, 500), (299, 600), (700, 800))]
    assert xs.merge_segments(hulls) == (2, [0, 1])


def test_cut_is_made_before_the_conflicting_call_not_earlier(xs):
    """C(2) meets C(0), an independent call 1 sits between: calls 0 and 1 stay together, call 2 opens the next segment"""
    hulls = [call((0, 100), (100, 200), (200, 300)), call((1000, 1100), (1100, 1200), (1200, 1300)), call((2000, 2100), (2100, 2200), (250, 350)),
             call((3000, 3100), (3100, 3200), (3200, 3300))]
    assert xs.merge_segments(hulls) == (2, [0, 0, 1, 1])
    # a call is compared with the members of the open segment only: call 3 may meet call 0 again without a further cut
    hulls[3] = call((3000, 3100), (3100, 3200), (0, 50))
    assert xs.merge_segments(hulls) == (2, [0, 0, 1, 1])
    # ... but not call 2
    hulls[3] = call((3000, 3100), (260, 270), (3200, 3300))
    assert xs.merge_segments(hulls) == (3, [0, 0, 1, 2])


def test_ranges_that_only_touch_do_not_meet(xs):
    hulls = [call((0, 100), (100, 200), (200, 300)), call((300, 400), (400, 500), (500, 600)), call((600, 700), (700, 800), (800, 900))]
    assert xs.merge_segments(hulls) == (1, [0, 0, 0])
    hulls[1] = call((300, 400), (400, 500), (299, 600))  # one byte into C(0)
    assert xs.merge_segments(hulls) == (2, [0, 1, 1])
    # addresses in the upper half of the 64-bit range are compared unsigned
    top = 0xFFFF800000000000
    hulls = [call((top, top + 100), (top + 100, top + 200), (top + 200, top + 300)), call((0, 100), (100, 200), (200, 300)),
             call((top + 250, top + 260), (500, 600), (700, 800))]
    assert xs.merge_segments(hulls) == (2, [0, 0, 1])


def test_one_call_no_call_and_bad_arguments(xs):
    assert xs.merge_segments([call((0, 1), (1, 2), (2, 3))]) == (1, [0])
    assert xs.merge_segments([]) == (0, [])
    L = xs.lib()
    assert 0 == L.libxsmm_amd_merge_segments(0, None, None)
    assert -1 == L.libxsmm_amd_merge_segments(-1, None, None)
    assert -1 == L.libxsmm_amd_merge_segments(2, None, None)


def test_random_tables_against_the_restated_rule(xs):
    rng = np.random.default_rng(20240)
    cuts = 0
    for trial in range(400):
        n = int(rng.integers(1, 70))
        space = int(rng.choice([2000, 20000, 400000]))  # dense, mixed, sparse: many cuts ... hardly any
        hulls = []
        for _ in range(n):
            ranges = []
            for _ in range(3):
                lo = int(rng.integers(0, space)); ranges.append((lo, lo + int(rng.integers(1, 200))))
            hulls.append(call(*ranges))
        want = restated(hulls)
        assert xs.merge_segments(hulls) == want, (trial, hulls)
        assert want[1] == sorted(want[1]) and want[1][0] == 0 and want[1][-1] == want[0] - 1
        cuts += want[0] - 1
    assert cuts > 400  # (the tables do exercise the rule)


def no_pair_meets(hulls):
    """the rule the grouped pointer batches used to state on their own: the groups may be fused if no group's C meets another
    group's A or B, or the C of a later group"""
    meet = lambda x, y: x[0] < y[1] and y[0] < x[1]
    a = lambda h: (h[0], h[1]); b = lambda h: (h[2], h[3]); c = lambda h: (h[4], h[5])
    for x, hx in enumerate(hulls):
        for y, hy in enumerate(hulls):
            if x != y and (meet(c(hx), a(hy)) or meet(c(hx), b(hy)) or (x < y and meet(c(hx), c(hy)))):
                return False
    return True


def test_one_segment_says_no_pair_meets(xs):
    """the groups of ?gemm_batch are fused on "one segment"; that must be the old "no pair of groups meets", on every table"""
    rng = np.random.default_rng(7051)
    fused = split = 0
    for trial in range(600):
        n = int(rng.integers(2, 9))
        space = int(rng.choice([600, 3000, 40000]))  # most tables conflict ... hardly any does
        hulls = []
        for _ in range(n):
            ranges = []
            for _ in range(3):
                lo = int(rng.integers(0, space)); ranges.append((lo, lo + int(rng.integers(1, 120))))
            hulls.append(call(*ranges))
        want = no_pair_meets(hulls)
        assert (1 == xs.merge_segments(hulls)[0]) == want, (trial, hulls)
        fused += want; split += not want
    assert fused > 100 and split > 100  # (both answers are exercised)


def test_a_plan_without_a_flush_is_empty(xs):
    """the plan is kept per thread: a thread that has never flushed a record (a fresh one) reports an empty plan"""
    import threading
    got = []
    t = threading.Thread(target=lambda: got.append(xs.merge_last_plan()))
    t.start(); t.join()
    plan = got[0]
    assert plan["calls"] == 0 and plan["segments"] == 0 and plan["hulls"] == []


def test_exports_and_no_oracle_in_the_product(xs):
    out = subprocess.run(["nm", "-D", "--defined-only", xs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"libxsmm_amd_merge_segments", "libxsmm_amd_merge_last_plan", "libxsmm_amd_defer_begin", "libxsmm_amd_defer_end", "libxsmm_amd_flush"} <= exported
    everything = subprocess.run(["nm", "-D", xs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " xo_" not in everything
    assert callable(xs.defer_begin) and callable(xs.defer_end) and callable(xs.flush)
    header = open(os.path.join(ROOT, "include", "libxsmm_amd.h")).read()
    assert "libxsmm_amd_merge_segments" in header and "libxsmm_amd_merge_last_plan" in header


def test_bracket_without_a_device_records_nothing(xs):
    """the bracket itself needs no device: begin / end nest and an empty bracket does nothing"""
    L = xs.lib()
    before = L.libxsmm_amd_launch_count()
    xs.defer_begin(); xs.defer_begin()
    assert 1 == L.libxsmm_amd_defer_active()
    xs.defer_end()
    assert 1 == L.libxsmm_amd_defer_active()
    xs.defer_end()
    assert L.libxsmm_amd_launch_count() == before
    assert int(os.environ.get("LIBXSMM_AMD_DEFER", "0") or 0) != 0 or 0 == L.libxsmm_amd_defer_active()
    assert C.sizeof(C.c_ulonglong) == 8
