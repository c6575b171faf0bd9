"""The launch plans of dense batches against tests/launch_plans.py, without a GPU: every chain of the table is what the planner
offers (libxsmm_amd_smm_plan_describe), every class of alternative the planner offers anywhere on a grid of batches is reached by a
case of the table -- a planner change that adds an alternative fails here until a case runs it --, and every kernel text the
cases need compiles for gfx950."""
import ctypes as C
import itertools

import pytest

import launch_plans as lp


@pytest.fixture(scope="module")
def planner(xs):
    with lp.environment(LIBXSMM_AMD_JIT_MINBATCH=1, LIBXSMM_AMD_JIT=None, XSMM_SMMJIT_GAPS_MFMA=None, XSMM_SMMJIT_TILESPLIT=None,
                        XSMM_SMMJIT_LOWP_PACK=None):
        yield xs


@pytest.mark.parametrize("name", sorted(lp.CASES))
def test_chain_of_the_table_is_the_planners(planner, name):
    case = lp.CASES[name]
    plan = lp.describe(planner, case)
    got = [(a["pos"], a["name"], lp.launches_of(a)) for a in plan]
    want = [link for link in case["chain"] if isinstance(link[0], int)]
    assert got == want, (name, plan)
    # the order of the chain: matrix-core tier, hand-written kernels, specialised tier, pre-compiled kernel
    rank = {"mfma": 0, "special": 1, "jit": 2, "generic": 3, "lowp": 3}
    tiers = [rank[plan[link[0]]["tier"]] if isinstance(link[0], int) else rank[link[0]] for link in case["chain"]]
    assert tiers == sorted(tiers) and tiers[-1] == 3 and 1 == tiers.count(3), (name, tiers)
    if case["cpat"] == "nines":
        assert 8 * (case["batch"] - len(lp.run_lengths(case))) >= 7 * case["batch"]  # the hand-over of the two-part alternative: the work-group side
    if case["cpat"] == "mixed":
        assert 8 * (case["batch"] - len(lp.run_lengths(case))) < 7 * case["batch"]   # ... the wave side


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("geom", lp.BLOCKED_GEOMETRIES)
def test_blocked_chain_of_the_table_is_the_planners(planner, geom, prec, mfma):
    xs = planner
    items, kb = lp.blocked_items(geom)
    assert kb < 16  # (from 16 k blocks on a relaxed batch of few runs is cut into segments: no defined order)
    blob, d = xs.descriptor(xs.F64 if prec == "f64" else xs.F32, *geom[3:])
    plan = xs.smm_plan(d, mode=lp.INDEX, sync=lp.SYNC_DEVICE, batch=items, relaxed=True, uniform_run=kb, mfma=mfma)
    got = [(a["pos"], a["name"], lp.launches_of(a)) for a in plan if a["tier"] == "jit"]  # (blocked GEMM does not ask the matrix-core tier)
    assert got == [link for link in lp.blocked_chain(prec, geom, mfma) if isinstance(link[0], int)], plan


SIZES = (1, 8, 13, 16, 23, 32, 33, 40, 56, 64)


def _grid(xs):
    """(descriptor arguments, plan arguments) over the grid of the issue: shapes, leading dimensions, TRANS_B, addressing and sync modes,
    relaxed, alignment, batches below and above the pack, matrix cores on and off, the low-precision kinds"""
    for prec, m, n, k, gaps, transb in itertools.product((xs.F32, xs.F64), SIZES, SIZES, SIZES + (70,), (0, 3), (False, True)):
        ts = 8 if prec == xs.F64 else 4
        lda, ldb, ldc = m + gaps, (n if transb else k) + gaps, m + gaps
        desc = (prec, m, n, k, lda, ldb, ldc, xs.FLAG_TRANS_B if transb else 0)
        sizes = (lda * k, ldb * (k if transb else n), ldc * n)
        for mfma in (1, 0):
            for batch, bits in itertools.product((3, 37), (0, ts)):
                yield desc, dict(mode=lp.STRIDED, sync=lp.SYNC_NONE, batch=batch, strides=sizes, address_bits=bits, mfma=mfma)
            yield desc, dict(mode=lp.STRIDED, sync=lp.SYNC_RUNS, batch=37, strides=(sizes[0], sizes[1], 0), mfma=mfma)
            for mode in (lp.INDEX, lp.POINTER):
                strides = (8, 8, 8) if mode == lp.POINTER else (0, 0, 0)
                for sync in (lp.SYNC_NONE, lp.SYNC_RUNS, lp.SYNC_ATOMIC):
                    yield desc, dict(mode=mode, sync=sync, batch=37, strides=strides, mfma=mfma)
                for relaxed in (False, True):
                    yield desc, dict(mode=mode, sync=lp.SYNC_DEVICE, batch=37, strides=strides, relaxed=relaxed, mfma=mfma)
            yield desc, dict(mode=lp.INDEX, sync=lp.SYNC_DEVICE, batch=36, relaxed=True, uniform_run=4, mfma=mfma)  # a blocked GEMM work list
    for lowp, m, n, k, gaps in itertools.product((1, 3, 4), SIZES, SIZES, SIZES, (0, 3)):
        desc = (xs.F32, m, n, k, m + gaps, k + gaps, m + gaps, 0)
        sizes = ((m + gaps) * k, (k + gaps) * n, (m + gaps) * n)
        for mfma, batch, bits in itertools.product((1, 0), (3, 37), (0, 2)):
            yield desc, dict(mode=lp.STRIDED, sync=lp.SYNC_NONE, batch=batch, strides=sizes, address_bits=bits, mfma=mfma, lowp=lowp)
            yield desc, dict(mode=lp.STRIDED, sync=lp.SYNC_NONE, batch=batch, strides=tuple(s + 8 for s in sizes), address_bits=bits, mfma=mfma, lowp=lowp)
        for mode in (lp.INDEX, lp.POINTER):
            yield desc, dict(mode=mode, sync=lp.SYNC_NONE, batch=37, strides=(8, 8, 8) if mode == lp.POINTER else (0, 0, 0), lowp=lowp)


def test_every_class_of_alternative_is_reached_by_a_case(planner):
    xs = planner
    reached = {}
    for name, case in lp.CASES.items():
        for alt in lp.describe(xs, case):
            reached.setdefault(lp.alt_class(alt), name)
    found, descs = {}, {}
    for desc, query in _grid(xs):
        if desc not in descs:
            descs[desc] = xs.descriptor(desc[0], desc[1], desc[2], desc[3], desc[4], desc[5], desc[6], flags=desc[7])
        for alt in xs.smm_plan(descs[desc][1], **query):
            found.setdefault(lp.alt_class(alt), (desc, query))
    missing = {cls: where for cls, where in found.items() if cls not in reached}
    assert not missing, "classes of alternatives no case of tests/launch_plans.py runs:\n" + "\n".join("%r first at %r" % kv for kv in sorted(missing.items(), key=repr))
    assert len(found) >= 30  # (the grid does reach the planner)
    # no entry point sets runs of a uniform length on the matrix-core tier: the plan must not offer such an alternative
    assert not [cls for cls in found if "wg_runs_jit" in cls[1]]


def test_kernel_texts_of_the_cases_compile_for_gfx950(planner):
    xs = planner
    L = xs.lib()
    buf = C.create_string_buffer(1 << 18)
    seen = set()
    for name, case in sorted(lp.CASES.items()):
        lda, ldb, ldc = lp.leading_dimensions(case)
        flags = xs.FLAG_TRANS_B if case["transb"] else 0
        prec = xs.F64 if case["prec"] == "f64" else xs.F32  # (16-bit inputs: the generated kernel is an fp32 kernel that widens on load)
        blob, d = xs.descriptor(prec, case["m"], case["n"], case["k"], lda, ldb, ldc, flags=flags)
        for alt in lp.describe(xs, case):
            for variant, _ in alt["parts"]:
                key = (prec, case["m"], case["n"], case["k"], lda, ldb, ldc, flags, variant)
                if key in seen:
                    continue
                seen.add(key)
                rc = L.libxsmm_amd_smm_kernel_source(d, variant, buf, len(buf), 1)
                if rc == -1:
                    pytest.skip("libhiprtc is not available here")
                assert rc == 0, (name, alt["name"], variant)
        if any(alt["tiles"] for alt in lp.describe(xs, case)):  # the tiles of C as one grouped kernel: compiled by the diagnostic itself
            query = dict(lp.plan_query(case), compile_tiles=True)
            assert xs.smm_plan(d, **query), name
    assert len(seen) >= 60
