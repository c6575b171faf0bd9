"""The references, the generated inputs and the comparison of tests/test_hostile_operands_gpu.py, checked without a GPU:

  * known answers of the oracle's fma chain and of the numpy gold loops at the edges of the number line (hand-computed
    chains of one to three terms);
  * the conditions on the generated inputs, on the reference result of every shape the GPU file uses;
  * six deliberately wrong restatements of a kernel, each of which hostile_operands.same_values has to reject on at least
    one of the three generators."""
import numpy as np
import pytest

import fc_common as fc
import hostile_operands as ho
import lowp_gemm_common as lg
import quant_common as qc

F32_MAX = float(np.finfo(np.float32).max)
F64_MAX = float(np.finfo(np.float64).max)


def chain1(orc, dtype, terms, c0, beta=1):
    """the oracle's fma chain of one element: c0 + sum a_i * b_i, k ascending"""
    a = np.array([[[t[0] for t in terms]]], dtype=dtype)
    b = np.array([[[t[1]] for t in terms]], dtype=dtype)
    return ho.chain(orc, a, b, np.array([[[c0]]], dtype=dtype), beta)[0, 0, 0]


def bits(x):
    return int(np.asarray(x).view({4: np.uint32, 8: np.uint64}[np.asarray(x).dtype.itemsize]))


# ---- known answers -------------------------------------------------------------------------------------------------------------
def test_oracle_chain_known_answers_fp32(orc):
    ho.assert_environment(orc)
    f = np.float32
    # a subnormal result: 2^-126 * 0.5 = 2^-127
    assert bits(chain1(orc, f, [(2.0 ** -126, 0.5)], 0.0)) == 0x00400000
    # rounding at the subnormal boundary. 3 * 2^-150 = 1.5 units of 2^-149, a tie: to even, 2 units; (2^-149 + 2^-150) + 2^-150
    # is exact in the fma (one rounding of 2.5 units: a tie again, to even: 2 units), while rounding the product alone first gives
    # 2 + 1 = 3 units
    assert bits(chain1(orc, f, [(3 * 2.0 ** -75, 2.0 ** -75)], 0.0)) == 0x00000002
    assert bits(chain1(orc, f, [(2.0 ** -75, 2.0 ** -74 * 1.5)], f(2.0 ** -149))) == 0x00000002   # 1 + 1.5 units -> 2.5 -> 2
    assert bits(chain1(orc, f, [(2.0 ** -75, 2.0 ** -74 * 1.5)], f(3 * 2.0 ** -149))) == 0x00000004  # 3 + 1.5 -> 4.5 -> 4 (product alone: 2, sum 5)
    # the smallest subnormal times one half is a tie between 0 and 2^-149: to even, zero, with the sign of the exact sum
    assert bits(chain1(orc, f, [(-(2.0 ** -149), 0.5)], 0.0)) == 0x80000000
    # overflow to Inf: FLT_MAX * 2, and FLT_MAX + FLT_MAX * 2^-24 (half a unit in the last place: a tie, to even: up to Inf)
    assert bits(chain1(orc, f, [(F32_MAX, 2.0)], 0.0)) == 0x7f800000
    assert bits(chain1(orc, f, [(F32_MAX, 2.0 ** -24)], f(F32_MAX))) == 0x7f800000
    assert bits(chain1(orc, f, [(F32_MAX, 2.0 ** -26)], f(F32_MAX))) == 0x7f7fffff   # a quarter of a unit: stays finite
    assert bits(chain1(orc, f, [(-F32_MAX, 2.0)], 0.0)) == 0xff800000
    # Inf - Inf and 0 * Inf
    assert np.isnan(chain1(orc, f, [(F32_MAX, 2.0), (-np.inf, 1.0)], 0.0))
    assert bits(chain1(orc, f, [(F32_MAX, 2.0), (-F32_MAX, 2.0)], 0.0)) == 0x7f800000   # (the fma's product does not overflow on its own: Inf - finite)
    assert np.isnan(chain1(orc, f, [(0.0, np.inf)], 1.0))
    assert np.isnan(chain1(orc, f, [(1.0, 1.0), (np.inf, 0.0), (1.0, 1.0)], 1.0))
    assert bits(chain1(orc, f, [(2.0, 3.0), (np.inf, -1.0)], 1.0)) == 0xff800000
    # -0.0 kept: -0 + (-0 * 1), and lost to +0 by a chain that starts from +0 (beta = 0)
    assert bits(chain1(orc, f, [(-0.0, 1.0), (1.0, -0.0)], f(-0.0))) == 0x80000000
    assert bits(chain1(orc, f, [(-0.0, 1.0)], f(-0.0), beta=0)) == 0x00000000
    assert bits(chain1(orc, f, [(1.0, -1.0)], 1.0)) == 0x00000000   # x - x is +0 in round-to-nearest


def test_oracle_chain_known_answers_fp64(orc):
    ho.assert_environment(orc)
    f = np.float64
    assert bits(chain1(orc, f, [(2.0 ** -1022, 0.5)], 0.0)) == 0x0008000000000000
    assert bits(chain1(orc, f, [(3 * 2.0 ** -537, 2.0 ** -538)], 0.0)) == 0x0000000000000002
    assert bits(chain1(orc, f, [(2.0 ** -537, 2.0 ** -537 * 1.5)], f(2.0 ** -1074))) == 0x0000000000000002
    assert bits(chain1(orc, f, [(2.0 ** -537, 2.0 ** -537 * 1.5)], f(3 * 2.0 ** -1074))) == 0x0000000000000004
    assert bits(chain1(orc, f, [(F64_MAX, 2.0)], 0.0)) == 0x7ff0000000000000
    assert bits(chain1(orc, f, [(F64_MAX, 2.0 ** -53)], f(F64_MAX))) == 0x7ff0000000000000
    assert bits(chain1(orc, f, [(F64_MAX, 2.0 ** -55)], f(F64_MAX))) == 0x7fefffffffffffff
    assert np.isnan(chain1(orc, f, [(F64_MAX, 2.0), (-np.inf, 1.0)], 0.0))
    assert bits(chain1(orc, f, [(F64_MAX, 2.0), (-F64_MAX, 2.0)], 0.0)) == 0x7ff0000000000000
    assert np.isnan(chain1(orc, f, [(0.0, np.inf)], 1.0))
    assert bits(chain1(orc, f, [(-0.0, 1.0), (1.0, -0.0)], f(-0.0))) == 0x8000000000000000
    assert bits(chain1(orc, f, [(-0.0, 1.0)], f(-0.0), beta=0)) == 0


def test_muladd_differs_from_fma_exactly_where_it_should(orc):
    """the oracle's other flavour rounds the product on its own: 1.5 units of the smallest subnormal become 2 before the sum"""
    ho.assert_environment(orc)
    a, b, c = (np.array([[[v]]], dtype=np.float32) for v in (2.0 ** -75, 2.0 ** -74 * 1.5, 3 * 2.0 ** -149))
    assert bits(ho.chain(orc, a, b, c, 1, arith=orc.MULADD)[0, 0, 0]) == 0x00000005
    assert bits(ho.chain(orc, a, b, c, 1)[0, 0, 0]) == 0x00000004


def gold1(terms, c0, beta=1):
    """hostile_operands.gold_bf16 and lowp_gemm_common.reference (kind 2) on one element; they must agree"""
    a = np.array([[[t[0] for t in terms]]], dtype=np.float32)
    b = np.array([[[t[1]] for t in terms]], dtype=np.float32)
    c = np.array([[[c0]]], dtype=np.float32)
    assert np.array_equal(ho.bf16_widen(ho.bf16_bits(a)), a) and np.array_equal(ho.bf16_widen(ho.bf16_bits(b)), b), "operands must be bf16 numbers"
    with np.errstate(all="ignore"):
        g = ho.gold_bf16(a, b, c, beta)[0, 0, 0]
        k = len(terms)
        r = lg.reference(2, False, False, 1, 1, k, ho.bf16_bits(a).ravel(), 1, ho.bf16_bits(b).ravel(), k, beta, c.ravel().copy(), 1)[0]
    assert bits(g) == bits(r) or (np.isnan(g) and np.isnan(r))
    return g


def test_gold_loop_known_answers_bf16(orc):
    """the gold loop of the bf16 kinds: product and sum rounded separately, in float32"""
    ho.assert_environment(orc)
    assert bits(gold1([(2.0 ** -126, 0.5)], 0.0)) == 0x00400000                       # a subnormal result
    assert bits(gold1([(2.0 ** -75, 2.0 ** -74 * 1.5)], 3 * 2.0 ** -149)) == 0x00000005   # the product alone rounds 1.5 -> 2 units; the fma chain gives 4
    assert bits(chain1(orc, np.float32, [(2.0 ** -75, 2.0 ** -74 * 1.5)], np.float32(3 * 2.0 ** -149))) == 0x00000004
    big = float(ho.bf16_widen(np.array([0x7f7f], np.uint16))[0])                     # the largest bf16 number
    assert bits(gold1([(big, 2.0)], 0.0)) == 0x7f800000                              # overflow to Inf
    assert np.isnan(gold1([(big, 2.0), (-big, 2.0)], 0.0))                           # Inf - Inf
    assert np.isnan(gold1([(0.0, np.inf)], 1.0))                                     # 0 * Inf
    assert bits(gold1([(-0.0, 1.0), (1.0, -0.0)], -0.0)) == 0x80000000               # -0.0 kept
    assert bits(gold1([(-0.0, 1.0)], -0.0, beta=0)) == 0x00000000
    # the numpy loop of tests/test_lowp.py (pairs of k, the dispatched kernels' reading of A) on the same two-term chain
    a = ho.bf16_bits(np.array([2.0 ** -75, 1.0], np.float32)); b = ho.bf16_bits(np.array([2.0 ** -74 * 1.5, 0.0], np.float32))
    c = np.array([3 * 2.0 ** -149], np.float32)
    assert bits(lg.pairs_gold(2, 0, 1, 1, 2, 1, 2, 1, a, b, c, 1.0)[0]) == 0x00000005
    ref = c.copy()
    assert 0 == orc.gemm_lowp(2, 0, 1, 1, 2, 1, 2, 1, a, b, ref, 1.0) and bits(ref[0]) == 0x00000005


def test_bf16_output_rounding_known_answers(orc):
    """what becomes of a float32 sum that leaves as bf16: the fully-connected layer rounds to nearest even (overflow to Inf, NaN
    stays NaN and quiet), the bf16 -> bf16 kernels truncate"""
    ho.assert_environment(orc)
    x = np.array([0x7f7f8000, 0x7f7f7fff, 0x7fc00001, 0x7f800001, 0xff7f8000, 0x80000000, 0x00008000, 0x00018000], dtype=np.uint32).view(np.float32)
    r = qc.bf16_rne(x)
    assert r[0] == 0x7f80 and r[1] == 0x7f7f and r[4] == 0xff80           # 0x7f7f8000 is a tie: to even, which is Inf
    assert (r[2] & 0x7fff) > 0x7f80                                       # a quiet NaN stays NaN: it is not rounded up into the sign bit
    assert r[3] == 0x7f80                                                 # (the reference's converter only drops the lower half of a non-finite number)
    assert r[5] == 0x8000 and r[6] == 0x0000 and r[7] == 0x0002           # -0 kept; ties at the bottom of the subnormals: to even
    # the oracle's bf16 -> bf16 gold loop (kind 3) truncates: 0x7f7f8000 stays the largest finite number
    big = ho.bf16_bits(np.array([ho.bf16_widen(np.array([0x7f7f], np.uint16))[0], 1.0], np.float32))
    b = ho.bf16_bits(np.array([1.0, 0.0], np.float32)); c = np.array([0x7b00], dtype=np.uint16)  # 0x7f7f0000 + 0x7b000000 (2^119) = 0x7f7f8000 exactly
    assert 0 == orc.gemm_lowp(3, 0, 1, 1, 2, 1, 2, 1, big, b, c, 1.0) and c[0] == 0x7f7f
    # the fully-connected expectation rounds dx through the same converter
    h = fc.Handle(fc.desc(5, 32, 48, dt="bf16"))
    x0, w, dy = (np.zeros(s, np.float32) for s in ((5, 32), (48, 32), (5, 48)))
    w[0, 0], w[1, 0], dy[0, 0], dy[0, 1] = x[0] * 0 + ho.bf16_widen(np.array([0x7f7f], np.uint16))[0], 2.0 ** 119, 1.0, 1.0
    y, dx, dw = fc.expected(h, x0, w, dy)
    assert dx[0, 0] == 0x7f80   # 0x7f7f0000 + 0x7b000000 = 0x7f7f8000 -> Inf


# ---- the generated inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ho.KINDS)
def test_conditions_on_the_smm_cases(orc, kind):
    ho.assert_environment(orc)
    for case, fmt, beta in ho.smm_variants() + ho.smm_variants(ho.GROUPED):
        a, b, c = case.operands(kind, fmt, beta)
        want = case.reference(orc, a, b, c, beta)
        try:
            ho.conditions(kind, want, beta)
        except AssertionError as e:
            raise AssertionError((case.id, fmt, beta) + e.args)


@pytest.mark.parametrize("kind", ho.KINDS)
def test_conditions_on_the_tiled_gemm_cases(xs, orc, kind):
    ho.assert_environment(orc)
    T = xs.lib().libxsmm_amd_gemm_tile()
    for beta in (1, 0):
        for fmt in ("f32", "f64"):
            a, b, c = ho.operands(kind, fmt, ho.seed_of("tgemm", fmt, kind, beta), 1, T + 1, 33, 35)
            ho.conditions(kind, ho.chain(orc, a, b, c, beta), beta)
        for k in (35, 34):
            a, b, c = ho.operands(kind, "bf16", ho.seed_of("tgemm_bf16", kind, beta, k), 1, T + 1, 33, k)
            with np.errstate(all="ignore"):
                gold = ho.gold_bf16(a, b, c, beta)
            ho.conditions(kind, gold, beta)
            if kind == "underflow":
                sub = ho.inexact_product(a, b)
                assert sub.any() and not sub.all()
                assert not ho.same_values(gold[sub], ho.chain(orc, a, b, c, beta)[sub])  # the divergence DESIGN.md 8j pins is in the data


@pytest.mark.parametrize("kind", ho.KINDS)
def test_conditions_on_the_fsspmdm_fc_and_low_precision_cases(orc, kind):
    ho.assert_environment(orc)
    for fmt in ("f32", "f64"):
        a = ho.fsspmdm_operator(orc, fmt, True)
        info = np.finfo(a.dtype)
        assert (a == info.smallest_subnormal).sum() == 1 and (a == -info.max).sum() == 1 and np.sum((a == 0) & np.signbit(a)) == 1
        for beta in (1, 0):
            b, c = ho.fsspmdm_operands(kind, fmt, ho.seed_of("fsspmdm", fmt, kind, beta), a, beta)
            ho.conditions(kind, ho.fsspmdm_reference(orc, a, b, c, beta), beta)
    assert all(name in ho.FC_CASES and gen in ho.KINDS and which in (ho.FC_FWD, ho.FC_BWD, ho.FC_UPD) for name, gen, which in ho.FC_SHIFT)
    for name in ho.FC_CASES:  # every pass on its own
        for which, (plain, result) in enumerate(ho.fc_chains(orc, name, kind)):
            try:
                ho.conditions(kind, result, 0)
            except AssertionError as e:
                raise AssertionError((name, which) + e.args)
    for case in ho.LOWP_CASES:
        for beta in case.betas:
            if case.kind != 0:
                a, b, c = case.operands(kind, beta)
                ho.conditions(kind, case.sums(a, b, c, beta), beta)
                if kind != "specials":  # products that float32 cannot hold exactly are in the data, and they matter
                    hit = case.inexact(a, b)
                    assert hit.any() and not ho.same_values(case.sums(a, b, c, beta)[hit], case.sums(a, b, c, beta, fma=orc)[hit])


def test_fc_chains_are_the_expectation_of_fc_common(orc):
    """the chain whose result the conditions are asked of is what tests/fc_common.py expects of the pass"""
    ho.assert_environment(orc)
    for name in ho.FC_CASES:
        d = fc.COMPUTE_CASES[name]
        h = fc.Handle(d)
        for kind in (None,) + ho.KINDS:
            for which, ((x, w, dy), result) in enumerate(ho.fc_chains(orc, name, kind)):
                with np.errstate(all="ignore"):
                    out = fc.expected(h, x, w, dy)[which]
                mine = np.ascontiguousarray(result.T if which != ho.FC_UPD else result)
                mine = qc.bf16_rne(mine).reshape(mine.shape) if out.dtype == np.uint16 else mine
                assert ho.same_values(np.ascontiguousarray(out), mine), (name, kind, which)


def test_surround_and_same_values(orc):
    ho.assert_environment(orc)
    lay = ho.Layout(3, 5, batch=2, extra=1)
    assert (lay.ld, lay.size, lay.stride, lay.total) == (6, 30, 31, 2 * 64 + 62)
    x = np.arange(30, dtype=np.float32).reshape(2, 3, 5)
    flat = ho.surround(x, lay, np.float32(np.inf))
    assert np.array_equal(ho.peel(flat, lay), x) and np.isinf(flat[~lay.mask()]).all() and lay.mask().sum() == 30
    assert flat[64] == 0 and flat[64 + 1] == 5 and flat[64 + 6] == 1 and flat[64 + 31] == 15   # column major, ld 6, stride 31
    assert np.isinf(flat[:64]).all() and np.isinf(flat[-64:]).all()
    a = np.array([0.0, -0.0, np.nan, np.inf, 1e-45], np.float32)
    b = a.copy(); b[2] = -np.float32(np.nan)
    assert ho.same_values(a, b)                                # sign and payload of a NaN are not compared
    for i, v in ((0, -0.0), (1, 0.0), (2, 1.0), (3, -np.inf), (4, 0.0), (0, np.nan)):
        b = a.copy(); b[i] = v
        assert not ho.same_values(a, b), (i, v)
    h = np.array([0x7fc0, 0x7f80, 0x8000], np.uint16)
    assert ho.same_values(h, np.array([0xffc1, 0x7f80, 0x8000], np.uint16)) and not ho.same_values(h, np.array([0x7fc0, 0x7f80, 0x0000], np.uint16))


# ---- the comparison rejects the mistakes it is meant for ---------------------------------------------------------------------------
def flush(x):
    out = x.copy()
    out[(np.abs(out) < np.finfo(x.dtype).tiny)] *= 0  # keeps the sign: what a flushing unit gives
    return out


def wrong_inputs_flushed(orc, a, b, c, fill):
    return ho.chain(orc, flush(a), flush(b), flush(c), 1)


def wrong_outputs_flushed(orc, a, b, c, fill):
    return flush(ho.chain(orc, a, b, c, 1))


def wrong_mul_then_add(orc, a, b, c, fill):
    return ho.chain(orc, a, b, c, 1, arith=orc.MULADD)


def wrong_zero_padded_step(orc, a, b, c, fill):
    return ho.chain(orc, a, b, c, 1) + a.dtype.type(0)  # fma(0, 0, acc) = acc + 0


def wrong_zeros_skipped(orc, a, b, c, fill):
    """terms whose element of A is zero are left out: rows of A that hold zeros are redone on the entries that remain"""
    out = ho.chain(orc, a, b, c, 1)
    for t, i in zip(*np.nonzero((a == 0).any(axis=2))):
        keep = a[t, i] != 0
        if keep.any():
            out[t, i] = ho.chain(orc, a[t:t + 1, i:i + 1][:, :, keep], b[t:t + 1][:, keep, :], c[t:t + 1, i:i + 1], 1)[0, 0]
        else:
            out[t, i] = c[t, i]
    return out


def wrong_gap_times_zero(orc, a, b, c, fill):
    """one more step: a gap element of B against a padded zero of A"""
    a2 = np.concatenate([a, np.zeros_like(a[:, :, :1])], axis=2)
    b2 = np.concatenate([b, np.full_like(b[:, :1, :], fill)], axis=1)
    return ho.chain(orc, a2, b2, c, 1)


WRONG = [wrong_inputs_flushed, wrong_outputs_flushed, wrong_mul_then_add, wrong_zero_padded_step, wrong_zeros_skipped, wrong_gap_times_zero]


@pytest.mark.parametrize("fmt", ["f32", "f64"])
@pytest.mark.parametrize("wrong", WRONG, ids=[w.__name__ for w in WRONG])
def test_same_values_rejects_a_wrong_kernel(orc, wrong, fmt):
    ho.assert_environment(orc)
    rejected = []
    for kind in ho.KINDS:
        a, b, c = ho.operands(kind, fmt, ho.seed_of("wrong", fmt, kind), 5, 23, 29, 31)
        want = ho.chain(orc, a, b, c, 1)
        ho.conditions(kind, want, 1)
        assert ho.same_values(want, ho.chain(orc, a, b, c, 1))
        for fill in ho.fills(fmt):
            with np.errstate(all="ignore"):
                got = wrong(orc, a, b, c, fill)
            if not ho.same_values(got, want):
                rejected.append(kind)
    assert rejected, "no generator tells this kernel from a correct one"
    print(wrong.__name__, fmt, "rejected on", sorted(set(rejected)))


def test_same_values_rejects_a_wrong_bf16_kernel(orc):
    """for the gold loop of the bf16 kinds (product and sum rounded separately) the same mistakes, fma in place of multiply-add among them"""
    ho.assert_environment(orc)
    with np.errstate(all="ignore"):
        hits = {}
        for kind in ho.KINDS:
            a, b, c = ho.operands(kind, "bf16", ho.seed_of("wrong", "bf16", kind), 5, 23, 23, 22)
            want = ho.gold_bf16(a, b, c, 1)
            ho.conditions(kind, want, 1)
            wrongs = {"inputs flushed": ho.gold_bf16(flush(a), flush(b), flush(c), 1), "outputs flushed": flush(want),
                      "fma": ho.chain(orc, a, b, c, 1), "zero-padded step": want + np.float32(0),
                      "gap times zero": want + np.float32(0) * np.float32(np.inf)}
            for name, got in wrongs.items():
                if not ho.same_values(got, want):
                    hits.setdefault(name, []).append(kind)
    assert sorted(hits) == ["fma", "gap times zero", "inputs flushed", "outputs flushed", "zero-padded step"], hits
