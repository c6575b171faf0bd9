"""tests/spmdm_batch_cases.py against the sources and against float64: the lines of sparse.hip that plan() restates are still
there with the numbers the cases assume; every kernel form the source compiles for the spmdm batch family -- each XSMM_SPW(n),
each XSMM_SPM(n, true|false), the element kernel, the two create kernels and the wave kernel's two sub-paths -- is made to do the
work by at least one case of CASES (who removes the last case of a class, or adds an instantiation, meets this test first); and
the oracle, the reference of tests/test_spmdm_batch_shapes_gpu.py, agrees with a float64 product at every one of those shapes."""
import numpy as np
import pytest

import spmdm_batch_cases as sc


def test_the_source_still_says_what_plan_restates():
    bad = sc.check_source()
    assert not bad, "\n".join(bad)


def test_a_changed_number_and_a_lost_line_are_noticed():
    path, line, values = sc.SOURCE[1]
    assert sc.check_source([(path, line, (values[0] + 1,))])
    assert sc.check_source([(path, "constexpr int SPW_METADATA = <N>;", values)])
    path, line, values = next(s for s in sc.SOURCE if "XSMM_SPW(<N>)" in s[1])
    assert not sc.check_source([(path, line, values)])
    assert sc.check_source([(path, line, values[:-1] + (16,))])


def test_the_source_compiles_the_classes_the_issue_names():
    want = set(("wg", n) for n in sc.NB_LADDER) | set(("mfma", nt, full) for nt in (1, 2, 3, 4) for full in (True, False))
    want |= set([("elem",), ("create", "staged"), ("create", "wave", "rows8"), ("create", "wave", "chunks")])
    assert sc.compiled_classes() == want


def test_every_compiled_class_has_a_case_that_makes_it_work():
    bad = sc.missing()
    assert not bad, "\n".join(bad)


def test_a_class_that_loses_its_cases_is_named():
    """for every class: without the cases that cover it the census complains, and about that class only"""
    reached = sc.census()
    for cls, ids in reached.items():
        left = [c for c in sc.CASES if c.id not in ids]
        bad = sc.missing(left)
        assert bad and any(repr(cls) in line for line in bad), (cls, bad)


def test_the_plan_of_the_shapes_the_issue_lists():
    P = sc.plan
    assert P(255, 4, 160).inst == ("wg", 1) and P(64, 32, 64, mfma=0).inst == ("wg", 2) and P(64, 48, 64, mfma=0).inst == ("wg", 3)
    assert P(64, 64, 64, mfma=0).inst == ("wg", 4) and P(30, 36, 114).inst == ("wg", 6) and P(65, 64, 96).inst == ("wg", 6)
    assert P(100, 64, 128).inst == ("wg", 8) and P(255, 64, 160).inst == ("wg", 12) and P(97, 60, 140).inst == ("wg", 12)
    for nt, n in enumerate((16, 32, 48, 64), 1):
        assert P(64, n, 64).inst == ("mfma|wg", nt, True, nt) and P(64, n, 64).compute == "spmdm_compute_mfma|wg_lds"
    assert [P(*s).inst[1:3] for s in ((16, 16, 4), (32, 32, 60), (48, 48, 32), (48, 64, 64), (64, 64, 60))] == [(1, False), (2, False), (3, False), (4, False), (4, False)]
    for shape in ((64, 68, 64), (64, 63, 64), (5, 1, 7), (256, 64, 64), (64, 64, 161), (300, 20, 200)):
        assert P(*shape).inst == ("elem",) and P(*shape).compute == "spmdm_compute_elem"
    assert P(64, 48, 64, transb=True).inst == ("elem",) and P(64, 48, 64, transc=True).inst == ("elem",)
    assert [P(m, 4, k).create_path for m, k in ((255, 64), (255, 63), (65, 1))] == ["staged"] * 3
    assert [P(m, 4, k).create_path for m, k in ((259, 64), (256, 8), (65535, 1))] == ["rows8"] * 3
    assert [P(m, 4, k).create_path for m, k in ((1, 65), (40, 128), (255, 160), (7, 200), (1, 65535))] == ["chunks"] * 5
    assert P(1, 4, 65).inst == ("wg", 1) and P(1, 4, 65).create == "spmdm_create_slices_wave"


def test_the_two_sides_of_the_device_choice():
    def dense(id):
        case = sc.BY_ID[id]
        counts = (sc.logical_a(case) != 0).reshape(case.batch, -1).sum(axis=1)
        return int(counts.sum()), sc.batch_is_dense(counts, case.M, case.K)
    assert dense("choice-1146") == (1146, False) and dense("choice-1147") == (1147, True)
    assert dense("choice-even-dense")[1] and not dense("choice-odd-dense")[1]
    assert sc.covered(sc.BY_ID["choice-even-dense"]) >= set([("mfma", 3, True)])
    assert sc.covered(sc.BY_ID["choice-odd-dense"]) >= set([("wg", 3)])
    # 100 % is past what the matrix-core kernel stages through LDS, 2 % goes to the gather kernel of the pair
    assert 64 * 64 > sc.SPM_META and sc.covered(sc.BY_ID["pair-64x64x64-d2"]) >= set([("wg", 4)])


def test_hostile_operands_hold_what_they_promise():
    seen = dict(nan=0, tiny=0, negzero=0)
    for case in sc.CASES:
        if case.pattern[0] != "hostile":
            continue
        A = sc.logical_a(case)
        seen["nan"] += int(np.isnan(A).sum())
        seen["tiny"] += int(((A != 0) & (np.abs(A) < 2.0 ** -126)).sum())
        seen["negzero"] += int(((A == 0) & np.signbit(A)).sum())
        assert not A[0, 0].any() and not A[-1, -1].any(), case.id
        assert case.batch < 4 or not A[case.batch // 2].any(), case.id
        assert (A != 0).any(), case.id
    assert all(seen.values()), seen
    assert set(c.trans[0] for c in sc.CASES if "create" in repr(sc.covered(c)) and c.pattern[0] == "hostile") == set("NT")


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_the_oracle_agrees_with_float64(orc, case):
    """per element |oracle - float64| <= K * 2^-24 * (|A||B| + |beta * C|): a chain of at most K fused multiply-adds, each
    rounded once (beta is 0, 1 or 0.5: beta * C is exact); NaN exactly where float64 has NaN. The slices of the numpy row scan
    rebuild A."""
    a, b = sc.operands(case)
    for beta in case.betas:
        c = sc.c_operand(case, beta)
        ref = sc.reference(orc, case, a, b, c, beta)
        A, B, Cm = sc.views(case, a, b, c)
        R = sc.views(case, a, b, ref)[2]
        A64, B64 = np.where(A == 0, 0.0, A.astype(np.float64)), B.astype(np.float64)
        C64 = np.zeros(Cm.shape) if beta == 0.0 else beta * Cm.astype(np.float64)
        with np.errstate(invalid="ignore"):
            gold = A64 @ B64 + C64
            bound = case.K * 2.0 ** -24 * (np.abs(A64) @ np.abs(B64) + np.abs(C64))
        nan = np.isnan(gold)
        assert np.array_equal(np.isnan(R), nan), (case.id, beta)
        err = np.abs(R.astype(np.float64) - gold)
        worst = float(np.max(np.where(nan, 0.0, err - bound)))
        print("%s beta %g: max error %.3g, max bound %.3g" % (case.id, beta, float(np.max(np.where(nan, 0.0, err))), float(np.max(np.where(nan, 0.0, bound)))))
        assert worst <= 0.0, (case.id, beta, worst)
    for item in (0, case.batch - 1):
        ri, ci, va = sc.slice_of(A[item])
        back = np.zeros((case.M, case.K), dtype=np.float32)
        rows = np.repeat(np.arange(case.M), np.diff(ri.astype(np.int64)))
        back[rows, ci] = va
        assert np.array_equal(np.where(A[item] == 0, np.float32(0), A[item]).view(np.uint32), back.view(np.uint32)), (case.id, item)
