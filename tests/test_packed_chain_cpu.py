"""The oracle of the packed kernels (oracle/xsmm_oracle.c: xo_packed_pgemm / getrf / trmm / trsm), held to what does not depend on it,
without a GPU: exact arithmetic on operands where every step is exact (its flag and index logic), a planted triple on which a fused
and a separate multiply-add differ (it is fused), the derived bounds of tests/packed_common.py on every case the GPU sweeps run, memory it
must leave alone, and the conditions every hostile case of tests/test_packed_hostile_gpu.py has to meet on the oracle alone. The
GPU tests then compare the kernels with this oracle bit for bit."""
import itertools

import numpy as np
import pytest

import hostile_operands as ho
import packed_common as pc
from packed_common import PGEMM, GETRF, TRMM, TRSM, COL, ROW, Case

DTYPES = [np.float32, np.float64]
LAYOUTS = [COL, ROW]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def oracle_result(xs, orc, case):
    """-> the written operand's matrices after the oracle's call; the canaries and the operands that are only read keep their bits"""
    before, after = case.buffers(xs), case.chain(xs, orc)
    msg = case.untouched(xs, before, after)
    assert msg is None, (case, msg)
    return case.result(xs, after[case.written])


# ---- exact cases -------------------------------------------------------------------------------------------------------------------
def exact_case(kind, dtype, m, n, k=0, seed=0, **kw):
    """a case whose operands make every step of the operation exact in float32 (hence in float64): small integers, diagonals of +-1, +-2,
    +-0.5, alpha in 1, -1, 0.5, 0.75; getrf: A = L U from such factors (-> the case, and for getrf the factors as one matrix)"""
    case = Case(kind, dtype, m, n, k, nmat=pc.width(dtype), seed=seed, **kw)
    rng = np.random.default_rng(1000 + seed)
    nmat = case.nmat
    ints = lambda *shape: rng.integers(-2, 3, (nmat,) + shape).astype(np.float64)
    diag = lambda d: rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], (nmat, d))
    factors = None
    if kind == PGEMM:
        ops = {name: ints(*x.shape[1:]) for name, x in case.ops.items()}
    elif kind == GETRF:
        d = min(m, n)
        low = np.tril(rng.integers(-1, 3, (nmat, m, d)).astype(np.float64), -1)
        up = np.triu(rng.integers(-2, 3, (nmat, d, n)).astype(np.float64), 1)
        idx = np.arange(d)
        up[:, idx, idx] = diag(d)
        factors = np.zeros((nmat, m, n))
        factors[:, :, :d] += low
        factors[:, :d, :] += up
        low[:, idx, idx] = 1.0
        ops = {"a": np.matmul(low, up)}
    else:
        nt = case.ops["a"].shape[1]
        t = rng.integers(-1, 2, (nmat, nt, nt)).astype(np.float64)
        idx = np.arange(nt)
        t[:, idx, idx] = diag(nt)
        t[np.isnan(case.ops["a"])] = np.nan  # what is never read keeps its NaN
        # (no zero in B: a sum whose terms are all zeros has the sign of its first term in the oracle's chain, and numpy's matmul, which
        # Case.reference() uses for trmm, starts from +0; with the diagonal term nonzero no such sum occurs)
        ops = {"a": t, "b": rng.choice([-2.0, -1.0, 1.0, 2.0], (nmat, m, n))}
    case.ops = {name: x.astype(case.dtype) for name, x in ops.items()}
    for name, x in ops.items():
        assert np.array_equal(case.ops[name].astype(np.float64), x, equal_nan=True)
    return case, factors


def assert_exact(xs, orc, case, factors=None):
    got = oracle_result(xs, orc, case)
    with np.errstate(invalid="ignore"):
        want = case.reference()
    # every step was exact: the same operation in the other type gives the same numbers
    other = Case.__new__(Case)
    other.__dict__.update(case.__dict__)
    other.dtype = np.dtype(np.float64 if case.dtype == np.float32 else np.float32)
    other.ops = {name: x.astype(other.dtype) for name, x in case.ops.items()}
    with np.errstate(invalid="ignore"):
        assert np.array_equal(other.reference().astype(np.float64), want.astype(np.float64)), case
    assert np.all(np.isfinite(want)) and np.array_equal(bits(got), bits(want.astype(case.dtype))), (case, int(np.sum(bits(got) != bits(want.astype(case.dtype)))))
    if factors is not None:
        assert np.array_equal(got.astype(np.float64), factors), case


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [TRSM, TRMM])
def test_exact_triangles_every_side_uplo_trans_diag(xs, orc, kind, dtype, layout):
    """all 16 flag combinations, tight and padded: the oracle equals plain numpy arithmetic (multiply, then add) bit for bit where no step
    rounds"""
    for i, (side, uplo, trans, diag) in enumerate(pc.FLAGS):
        for j, pad in enumerate((0, 3)):
            m, n = ((5, 4), (4, 6), (6, 3), (3, 5))[(i + j) % 4]
            case, _ = exact_case(kind, dtype, m, n, seed=2 * i + j, layout=layout, side=side, uplo=uplo, transa=trans, diag=diag,
                                 alpha=(1.0, -1.0, 0.5, 0.75)[(i + j) % 4], pad=pad)
            assert_exact(xs, orc, case)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_getrf_returns_its_factors(xs, orc, dtype, layout):
    for i, (m, n) in enumerate(((5, 5), (6, 4), (4, 6), (1, 3), (3, 1), (8, 8))):
        for pad in (0, 3):
            case, factors = exact_case(GETRF, dtype, m, n, seed=i, layout=layout, pad=pad)
            assert_exact(xs, orc, case, factors)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_pgemm_every_trans_and_alpha(xs, orc, dtype, layout):
    for i, (ta, tb, alpha) in enumerate(itertools.product("NT", "NT", (1.0, -1.0))):
        for j, pad in enumerate((0, 2)):
            m, n, k = ((5, 4, 3), (3, 6, 4), (4, 3, 6), (1, 2, 7))[(i + j) % 4]
            case, _ = exact_case(PGEMM, dtype, m, n, k, seed=i, layout=layout, transa=ta, transb=tb, alpha=alpha, pad=pad)
            assert_exact(xs, orc, case)


# ---- fused, not separate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [PGEMM, TRSM, TRMM, GETRF])
def test_the_oracle_is_fused(xs, orc, kind, dtype, layout):
    """a = 1 + 2^-e with 2 e >= p: a * a = 1 + 2^(1 - e) + 2^(-2 e) rounds to 1 + 2^(1 - e), so a * a - (1 + 2^(1 - e)) is 0 with two roundings
    and 2^(-2 e) with one. The triple goes through the chain of pgemm, the update of trsm, the row of trmm and the update of getrf"""
    e = 12 if np.dtype(dtype) == np.float32 else 27
    a, c, fused = 1.0 + 2.0 ** -e, -(1.0 + 2.0 ** (1 - e)), 2.0 ** (-2 * e)
    t = np.dtype(dtype).type
    assert t(a) * t(a) + t(c) == 0 and float(t(a)) == a and float(t(c)) == c
    v = pc.width(dtype)
    if kind == PGEMM:
        case = Case(kind, dtype, 1, 1, 1, layout=layout, nmat=v)
        ops, at = {"a": [[a]], "b": [[a]], "c": [[c]]}, (0, 0)
    elif kind == GETRF:   # l = -a / 1, then w(1,1) = fma(-l, w(0,1), w(1,1))
        case = Case(kind, dtype, 2, 2, layout=layout, nmat=v)
        ops, at = {"a": [[1.0, a], [-a, c]]}, (1, 1)
    elif kind == TRSM:    # x[1] = fma(-E(1,0), x[0], x[1]) under a unit diagonal
        case = Case(kind, dtype, 2, 1, layout=layout, nmat=v, diag="U")
        ops, at = {"a": [[np.nan, np.nan], [-a, np.nan]], "b": [[a], [c]]}, (1, 0)
    else:                 # s = x[1], then s = fma(E(1,0), x[0], s)
        case = Case(kind, dtype, 2, 1, layout=layout, nmat=v, diag="U")
        ops, at = {"a": [[np.nan, np.nan], [a, np.nan]], "b": [[a], [c]]}, (1, 0)
    case.ops = {name: np.broadcast_to(np.array(x, dtype=dtype), (v,) + np.shape(x)).copy() for name, x in ops.items()}
    got = oracle_result(xs, orc, case)
    assert np.all(got[:, at[0], at[1]] == t(fused)), (case, got[:, at[0], at[1]])
    if kind != TRMM:  # (multiply, then add: the triple does tell the two apart; numpy's matmul, the reference of trmm, may fuse on its own)
        with np.errstate(all="ignore"):
            assert np.all(case.reference()[:, at[0], at[1]] == 0)


# ---- the bounds, on the table the GPU sweeps walk ---------------------------------------------------------------------------------------
def assert_bound(xs, orc, case):
    ratio, msg = case.check(oracle_result(xs, orc, case))
    assert msg is None, (case, msg)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_oracle_meets_the_bounds_of_every_sweep(xs, orc, dtype, layout):
    cases = pc.pgemm_sweep(dtype, layout)
    for kind in (TRSM, TRMM):
        cases += pc.flag_sweep(kind, dtype, layout)
    for kind in (TRSM, TRMM, GETRF):
        cases += pc.shape_sweep(kind, dtype, layout)
    for kind, m, n, k, kw in pc.RESIDENT_CASES:
        cases.append(pc.resident_case(kind, m, n, k, kw, dtype, layout))
    for case in cases:
        assert_bound(xs, orc, case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_oracle_meets_the_bounds_of_the_other_gpu_cases(xs, orc, dtype):
    for kind, m, n, k, kw in pc.ONE_ANSWER:
        assert_bound(xs, orc, pc.one_answer_case(kind, m, n, k, kw, dtype))
    for kind, m, n, k, kw in pc.UNALIGNED_CASES:
        assert_bound(xs, orc, pc.unaligned_case(kind, m, n, k, kw, dtype))
    if np.dtype(dtype) == np.float32:
        for kind in (PGEMM, GETRF, TRMM, TRSM):
            assert_bound(xs, orc, pc.redispatch_case(kind))


def test_the_oracle_refuses_what_is_outside_its_domain(orc):
    x = np.zeros(4096, np.float32)
    assert orc.packed_pgemm(16, COL, 2, 2, 2, 2, 2, 2, "N", "N", 0.75, x, x, x, 1) == -1   # alpha is 1 or -1
    assert orc.packed_pgemm(16, COL, 2, 2, 2, 1, 2, 2, "N", "N", 1.0, x, x, x, 1) == -1    # lda < m
    assert orc.packed_getrf(16, 100, 2, 2, 2, x, 1) == -1                                  # layout
    assert orc.packed_trsm(16, ROW, 2, 3, 2, 2, "L", "L", "N", "N", 1.0, x, x, 1) == -1    # ldb < n, row major
    assert orc.packed_trmm(16, COL, 2, 3, 2, 2, "X", "L", "N", "N", 1.0, x, x, 1) == -1
    assert not x.any()


# ---- the hostile cases of tests/test_packed_hostile_gpu.py ---------------------------------------------------------------------------------
@pytest.mark.parametrize("op,fmt,size", ho.packed_cases())
def test_hostile_cases_meet_their_conditions_on_the_oracle(xs, orc, op, fmt, size):
    """per kind of values: the conditions on the hostile lanes' results, nothing else touched, the benign lanes the results of the benign
    case (a lane owns its matrix), and for the overflow kind the planted triple: finite, where multiply-then-add gives Inf"""
    ho.assert_environment(orc)
    base = ho.packed_case(op, fmt, size)
    lanes = ho.packed_hostile_lanes(base)
    assert len(lanes) == 3 * ho.PACKED_PACKS and base.diag == "N"
    benign = np.ones(base.nmat, bool)
    benign[lanes] = False
    plain = oracle_result(xs, orc, base)
    for kind in ho.KINDS:
        case = ho.packed_hostile(base, kind)
        got = oracle_result(xs, orc, case)
        ho.packed_conditions(kind, got[lanes])
        assert np.array_equal(bits(got[benign]), bits(plain[benign])), (case, kind)
        if kind == "overflow":
            t, i, j = ho.packed_fused_spot(case)
            with np.errstate(all="ignore"):
                separate = case.reference()
            assert np.isfinite(got[t, i, j]) and got[t, i, j] != 0, (case, got[t, i, j])
            assert op == TRMM or np.isinf(separate[t, i, j]), (case, separate[t, i, j])  # (numpy's matmul, trmm's reference, may fuse on its own)


def test_hostile_cases_cover_both_layouts_and_every_alpha():
    cases = [ho.packed_case(*c) for c in ho.packed_cases()]
    for op in (PGEMM, GETRF, TRMM, TRSM):
        mine = [c for c in cases if c.kind == op]
        assert {c.layout for c in mine} == {COL, ROW} and {(c.dtype.name, c.m) for c in mine} == {(d, s) for d in ("float32", "float64") for s in (8, 16)}
        want = {PGEMM: {1.0, -1.0}, GETRF: {1.0}}.get(op, {1.0, -1.0, 0.75})
        assert {c.alpha for c in mine} == want, (op, {c.alpha for c in mine})


# ---- the wide cases of tests/test_wide_offsets_gpu.py --------------------------------------------------------------------------------------
def test_the_wide_packed_cases_pass_2_31_elements_and_2_32_bytes():
    """(npacks - 1) * ld * lines * VLEN, the offset of the last pack of the wide operand, as the kernel text and the host form it: beyond what
    32 bits hold"""
    for name, kind, dtype, m, n, k, wide, npacks, kw in pc.WIDE_CASES:
        v, ts = pc.width(dtype), np.dtype(dtype).itemsize
        case = Case(kind, dtype, m, n, k, nmat=v, **kw)
        assert case.ops[wide].shape[2] == pc.WIDE_LINES and case.layout == COL, name
        last = (npacks - 1) * pc.WIDE_LD * pc.WIDE_LINES * v
        if ts == 4:
            assert last >= 2 ** 31 and last * ts >= 2 ** 33, name
            assert np.int64(last).astype(np.int32) != last  # (what narrowing the offset to int would make of it)
        else:
            assert last * ts >= 2 ** 32, name
        assert (last + pc.WIDE_LD * pc.WIDE_LINES * v) * ts <= 10 * 2 ** 30  # the operand fits the memory the file allows a case
