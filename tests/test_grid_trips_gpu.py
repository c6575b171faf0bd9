"""Every launcher that caps its grid, or cuts the work into slabs or bands, driven past the cap: two full trips of the
grid-stride loop (or two slabs, or a band and a bit) and an odd rest, so that a third, partial trip falls on other work-groups
than the first. The sizes come from tests/launch_limits.py, which tests/test_launch_limits_cpu.py holds against the sources.

References and comparisons are those of each family's own tests: bit for bit against tests/quant_common.py,
tests/pool_common.py, tests/lowp_gemm_common.py, tests/xcopy_common.py and the oracle; tests/matdiff_common.py with its bounds
for matdiff. Outputs lie between canaries. Every dimension that does not help to cross a limit is as small as the routing to
the intended kernel allows; the kernel is named by xs.last_kernel() wherever the family's tests do so.

What the layout of an operation rules out is said where it happens: a quantised tensor has an even number of elements (its
channel block is even), so the rest of the layout kernels is odd in the pairs a lane takes, not in elements; pooling with
N = 3 has a multiple of 3 items, 2 * 32768 + 41 here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import launch_limits as ll
import lowp_gemm_common as lg
import matdiff_common as mc
import pool_common as pc
import quant_common as qc
import xcopy_common as xc
from test_pool_gpu import Layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD16, GUARD32 = 0x7b7b, 0x7b7b7b7b
REST = 37  # odd, no multiple of 2, 4 or 64


def bits32(x):
    return x.view(np.uint32)


def rel_err(ref, tst):
    """as tests/test_smm_gpu.py has it"""
    den = np.max(np.abs(ref))
    return float(np.max(np.abs(ref.astype(np.float64) - tst.astype(np.float64))) / (den if den > 0 else 1.0))


# ---- quantise and convert, flat ------------------------------------------------------------------------------------------------
class Flat:
    """device input and output with 16 guard elements around the output; off: elements past a 16-byte boundary on both sides, so
    that quad_plan takes a head of 4 - off elements one by one (fp32 input) and the quads start at the boundary"""
    def __init__(self, torch, x, off, out_dtype, in_dtype):
        n = x.size
        self.n, self.o0 = n, 16 + off
        self.guard = GUARD32 if out_dtype is torch.int32 else GUARD16
        self.din = torch.zeros(n + 8, dtype=in_dtype, device="cuda")
        self.dout = torch.full((n + 48,), self.guard, dtype=out_dtype, device="cuda")
        assert self.din.data_ptr() % 16 == 0 and self.dout.data_ptr() % 16 == 0
        self.vin, self.vout = self.din[off:off + n], self.dout[self.o0:self.o0 + n]
        self.vin.copy_(torch.from_numpy(x))

    def result(self):
        out = self.dout.cpu().numpy()
        assert (out[:self.o0] == self.guard).all() and (out[self.o0 + self.n:] == self.guard).all(), "guard elements were overwritten"
        return out[self.o0:self.o0 + self.n]


def flat_floats(n, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(0.9)).astype(np.float32)
    x[::97] = 0.0
    return x


@pytest.mark.parametrize("mode", qc.DETERMINISTIC)
def test_quant_flat(xs, torch_gpu, mode):
    """libxsmm_dnn_quantize: the largest magnitude once in the last, partial trip of quant_absmax and once in its first; the
    scaling factor and every element of quant_flat depend on it"""
    torch = torch_gpu
    n = ll.sized("quant_flat", REST)
    x = flat_floats(n, mode)
    assert np.abs(x).max() < 0.5
    for off, pos, shift in ((0, n - 9, 2), (1, 5, 0)):  # n - 9: a quad of the third trip; 5: the first quad behind the head
        y = x.copy()
        y[pos] = np.float32(-1.25)
        b = Flat(torch, y, off, torch.int16, torch.float32)
        scf = xs.dnn_quantize(b.vin, b.vout, n, shift, mode)
        assert xs.last_kernel() == "quant_flat"
        gq, gscf = qc.quantize(y, shift, mode)
        assert gscf != qc.quantize(x, shift, mode)[1]  # (without the planted element the scale would be another)
        got = b.result()
        assert scf == gscf and np.array_equal(got, gq), (mode, off, pos, scf, gscf, int(np.argmax(got != gq)))


def test_dequantize_and_converters(xs, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(5)
    n = ll.sized("quant_flat", REST)
    q = rng.integers(-32768, 32768, n).astype(np.int16)
    for off in (0, 1):
        b = Flat(torch, q, off, torch.int32, torch.int16)
        xs.dnn_dequantize(b.vin, b.vout, n, 12)
        assert xs.last_kernel() == "dequant_flat"
        assert np.array_equal(bits32(b.result()), bits32(qc.dequantize(q, 12))), off
    u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[-qc.BF16_SPECIALS.size:] = qc.BF16_SPECIALS  # ties, NaN and Inf in the last, partial trip
    x = qc.from_bits(u)
    for off, (rounding, gold_fn) in zip((0, 1, 0), (("truncate", qc.bf16_truncate), ("rnaz", qc.bf16_rnaz), ("rne", qc.bf16_rne))):
        b = Flat(torch, u.view(np.int32), off, torch.int16, torch.int32)
        xs.convert_f32_bf16(b.vin, b.vout, n, rounding)
        assert xs.last_kernel() == "bf16_" + rounding
        assert np.array_equal(b.result().view(np.uint16), gold_fn(x)), rounding
    n = ll.sized("bf16_widen", REST)
    h = rng.integers(0, 2 ** 16, n, dtype=np.uint64).astype(np.uint16)
    for off in (0, 1):
        b = Flat(torch, h.view(np.int16), off, torch.int32, torch.int16)
        xs.convert_bf16_f32(b.vin, b.vout, n)
        assert xs.last_kernel() == "bf16_widen"
        assert np.array_equal(bits32(b.result()), bits32(qc.bf16_widen(h))), off


# ---- quantise, layouts ---------------------------------------------------------------------------------------------------------
# 2 * 1048576 + 2 * 41 outputs each: with `pair` two trips of 2048 * 256 pairs and 41 pairs, without four trips and 82 outputs
ACT_CASE = (3, 6, 37, 3149, 3, 1, 2)         # N, C, H, W, cb32, cb16, lp: cb32 = 3 is neither cb16 * lp nor 1 -> quant_act
FIL_CASE = (3, 6, 37, 3149, 3, 1, 3, 1, 2)   # K, C, R, S, cb32, cb16, kb32, kb16, lp
# plain input (cb32 = 1): 27 * 17 channel blocks of 130 channels (chunks of 64, 64 and 2) over 130 pixels (tiles of 64, 64 and 2)
TILED_CASE = (27, 2210, 2, 65, 1, 65, 2)


def run_layout(xs, torch, fn, gold_fn, case, mode, kernel):
    n = int(np.prod(case[:4]))
    x = flat_floats(n, n % 1000)
    x[n - 3] = np.float32(1.75)  # the largest magnitude: the last trip of quant_absmax
    dx = torch.from_numpy(x).cuda()
    gq, gscf = gold_fn(x, case, 2, mode)
    for off in ((0, 1) if kernel != "quant_act_tiled" else (0,)):  # off 1: out only 2-byte aligned, no pairs
        dq = torch.full((n + 32,), GUARD16, dtype=torch.int16, device="cuda")
        assert dq.data_ptr() % 16 == 0
        scf = fn(dx, dq[16 + off:16 + off + n], *case, 2, mode)
        assert xs.last_kernel() == kernel
        out = dq.cpu().numpy()
        assert (out[:16 + off] == GUARD16).all() and (out[16 + off + n:] == GUARD16).all()
        got = out[16 + off:16 + off + n]
        assert scf == gscf and np.array_equal(got, gq), (case, off, scf, gscf, int(np.argmax(got != gq)))


def test_quant_act_layout(xs, torch_gpu):
    n = int(np.prod(ACT_CASE[:4]))
    assert n == 2 * ll.per_trip("quant_layout_pair") + 2 * 41 and n > 4 * ll.per_trip("quant_layout_single")
    run_layout(xs, torch_gpu, xs.dnn_quantize_act, qc.quantize_act, ACT_CASE, qc.NEAREST_ROUND, "quant_act")


def test_quant_fil_layout(xs, torch_gpu):
    assert int(np.prod(FIL_CASE[:4])) == 2 * ll.per_trip("quant_layout_pair") + 2 * 41
    run_layout(xs, torch_gpu, xs.dnn_quantize_fil, qc.quantize_fil, FIL_CASE, qc.BIAS_ROUND, "quant_fil")


def test_quant_act_tiled(xs, torch_gpu, monkeypatch):
    """one LDS tile per work-group, reused trip after trip: 2 * 2048 + 35 tiles, the last ones of 2 pixels x 2 channels"""
    N, Cc, H, W, cb32, cb16, lp = TILED_CASE
    lim = ll.LIMITS["quant_act_tiled"]
    CB, P = cb16 * lp, H * W
    chunks, ptiles = -(-CB // lim["channels"]), -(-P // lim["pixels"])
    assert CB > lim["channels"] and CB % lim["channels"] and P % lim["pixels"]
    assert N * (Cc // CB) * chunks * ptiles == ll.sized("quant_act_tiled", 35)
    monkeypatch.setenv("LIBXSMM_AMD_QUANT_TILED", "1")
    run_layout(xs, torch_gpu, xs.dnn_quantize_act, qc.quantize_act, TILED_CASE, qc.FPHW_ROUND, "quant_act_tiled")


# ---- matdiff, tiled --------------------------------------------------------------------------------------------------------------
def matdiff_call(xs, torch, dt, m, n, ref, tst, ld):
    info = xs.MatdiffInfo()
    dref, dtst = torch.from_numpy(ref).cuda(), torch.from_numpy(tst).cuda()
    rc = xs.lib().libxsmm_matdiff(C.byref(info), dt, m, n, xs.dptr(dref), xs.dptr(dtst), xs.iptr(ld), xs.iptr(ld))
    assert 0 == rc and xs.last_kernel().startswith("matdiff_")
    return mc.fields_of(info)


@pytest.mark.parametrize("lines", [32, 48])
@pytest.mark.parametrize("dt", [mc.F32, mc.I8])
def test_matdiff_tiles_of_more_lines(xs, torch_gpu, dt, lines):
    """m = 300 is two strips; from 2048 * 16 / 2 lines on a tile has 32 of them, from twice that 48. The largest difference, the
    extremes of both operands and (floats, a second call) a NaN lie in the last tile row, which is partial, in the second strip"""
    lim = ll.LIMITS["matdiff_tiles"]
    m = 300
    nstrips = -(-m // lim["strip"])
    n = (lines // lim["lines"] - 1) * lim["per_trip"] // nstrips + REST
    assert lines == -(-(-(-n * nstrips // 2048)) // lim["lines"]) * lim["lines"] and n % lines
    ld = m + 4
    ref, tst = mc.operand(lines + dt, dt, n, ld, m), mc.operand(lines + dt + 1, dt, n, ld, m)
    last = (n // lines) * lines + 2  # a line of the partial tile row
    at = lambda i, j: i * ld + j
    if dt == mc.F32:
        ref[at(last, 290)], tst[at(last, 290)] = 40.0, -40.0    # linf_abs = 80, max_ref, min_tst
        ref[at(last + 1, 299)], tst[at(last + 1, 257)] = -50.0, 45.0  # min_ref, max_tst
    else:
        ref[at(last, 290)], tst[at(last, 290)] = 127, -128
        ref[at(last + 1, 299)], tst[at(last + 1, 257)] = -128, 127
    rc, want = mc.matdiff(m, n, ref, tst, ld, ld)
    assert 0 == rc and (want["m"], want["n"]) == (290, last)
    got = matdiff_call(xs, torch_gpu, dt, m, n, ref, tst, ld)
    mc.compare(got, want, m * n, (dt, lines))
    if dt == mc.F32:
        tst[at(n - 1, 298)] = np.nan
        rc, want = mc.matdiff(m, n, ref, tst, ld, ld)
        assert (want["m"], want["n"]) == (298, n - 1)
        assert matdiff_call(xs, torch_gpu, dt, m, n, ref, tst, ld) == want


@pytest.mark.parametrize("dt", [mc.F32, mc.I8])
def test_matdiff_norms_over_more_lines_than_lanes(xs, torch_gpu, dt):
    """m = 3: matdiff_norms has a lane per line and per column, 2 * 2048 * 256 + 37 of them; the line with the largest sums
    (normi_*) is one of the last trip"""
    m = 3
    n = ll.sized("matdiff_norms", REST) - m
    ref, tst = mc.operand(7 + dt, dt, n, m, m), mc.operand(8 + dt, dt, n, m, m)
    big = (120, -120) if dt == mc.I8 else (30.0, -30.0)
    for j in range(m):
        ref[(n - 2) * m + j], tst[(n - 2) * m + j] = big
    rc, want = mc.matdiff(m, n, ref, tst, m, m)
    assert 0 == rc and want["normi_abs"] == 3.0 * (big[0] - big[1]) and (want["m"], want["n"]) == (0, n - 2)
    got = matdiff_call(xs, torch_gpu, dt, m, n, ref, tst, m)
    assert xs.last_kernel().startswith("matdiff_")
    mc.compare(got, want, m * n, (dt, "norms"))


# ---- pooling -----------------------------------------------------------------------------------------------------------------------
POOL_ITEMS = ll.sized("pool", 41)  # N = 3: the items are a multiple of 3
_pool = {}


def pool_case(kind, dt, threads=1):
    assert POOL_ITEMS % 3 == 0
    d = pc.desc(H=3, W=3, R=2, S=2, u=1, v=1, pad_h=1, pad_w=1, N=3, C=16 * (POOL_ITEMS // 3), pool=kind, dt=dt, threads=threads)
    name = "trips_%s_%s_%s" % ("max" if kind == pc.MAX else "avg", "f32" if dt == pc.F32 else "bf16", "t" if kind == pc.MAX else "n")
    if name not in _pool:
        _pool[name] = pc.expected(name, d)
    return d, _pool[name]


@pytest.mark.parametrize("dt", [pc.F32, pc.BF16])
@pytest.mark.parametrize("kind", [pc.MAX, pc.AVG])
def test_pool_items_in_three_slabs(xs, torch_gpu, kind, dt):
    d, want = pool_case(kind, dt)
    layer = Layer(xs, torch_gpu, d, want)
    assert layer.h.work() == POOL_ITEMS
    assert 0 == layer.run(pc.FWD)
    assert xs.last_kernel() == "pool_fwd_%s_%s" % ("max" if kind == pc.MAX else "avg", "f32" if dt == pc.F32 else "bf16")
    layer.check(pc.REG_OUT)
    if kind == pc.MAX:
        layer.check(pc.MASK)
    assert 0 == layer.run(pc.BWD)
    assert xs.last_kernel().startswith("pool_bwd_")
    layer.check(pc.GRAD_IN)
    layer.check(pc.REG_IN)
    layer.check(pc.GRAD_OUT)
    layer.close()


@pytest.mark.parametrize("threads", [3, 2])
def test_pool_shares_that_start_past_a_slab(xs, torch_gpu, threads):
    """threads = 3: the last share starts at item 43718, inside what one launch would take as its second slab;
    threads = 2: each share is a slab and a bit of its own, counted from the share's first item"""
    d, want = pool_case(pc.MAX, pc.F32, threads)
    layer = Layer(xs, torch_gpu, d, want)
    shares = [layer.h.share(t) for t in range(threads)]
    assert shares[-1][0] > ll.per_trip("pool") and (threads != 2 or shares[0][1] > ll.per_trip("pool"))
    for kind, dest in ((pc.FWD, pc.REG_OUT), (pc.BWD, pc.GRAD_IN)):
        for tid in reversed(range(threads)):
            assert 0 == layer.run(kind, 0, tid)
        layer.check(dest)
    layer.check(pc.MASK)
    layer.close()


# ---- tiled GEMM: a band of 65535 tiles of columns and one tile and a column more ---------------------------------------------------
def band_columns(xs):
    T = xs.lib().libxsmm_amd_gemm_tile()
    assert T == ll.LIMITS["tgemm_band"]["tile_cross_check"]
    return ll.per_trip("tgemm_band") * T + T + 1


@pytest.mark.parametrize("trans", ["NN", "NT"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tgemm_second_band(xs, orc, torch_gpu, dtype, trans):
    torch = torch_gpu
    m, k, n = 3, 3, band_columns(xs)
    tb = trans[1] == "T"
    lda, ldb, ldc = m, (n if tb else k), m + 3
    rng = np.random.default_rng(n % 1000 + tb)
    a = rng.uniform(-1, 1, lda * k).astype(dtype)
    b = rng.uniform(-1, 1, ldb * (k if tb else n)).astype(dtype)
    c = rng.uniform(-1, 1, ldc * n).astype(dtype)
    gold = c.copy()
    orc.smm(orc.FMA, orc.FLAG_TRANS_B if tb else 0, m, n, k, lda, ldb, ldc, a, b, gold)
    prec = xs.F64 if dtype == np.float64 else xs.F32
    keep, h = xs.gemm_handle(prec, prec, "N", trans[1], m, n, k, lda, ldb, ldc, 1.0, 1.0)
    assert h
    da, db, dc = (torch.from_numpy(v).cuda() for v in (a, b, c))
    xs.gemm_thread(h, da, db, dc)
    torch.cuda.synchronize()
    assert xs.last_kernel() == "tgemm_f%d_%s" % (64 if dtype == np.float64 else 32, trans.lower())
    got = dc.cpu().numpy()
    u = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(got.view(u), gold.view(u)), int(np.argmax(got.view(u) != gold.view(u))) // ldc  # (the padding is part of it)
    tail = gold.reshape(n, ldc)[ll.per_trip("tgemm_band") * xs.lib().libxsmm_amd_gemm_tile():, :m]
    assert not np.array_equal(tail, c.reshape(n, ldc)[-tail.shape[0]:, :m])  # the second band holds a product


def test_tgemm_lowp_second_band(xs, torch_gpu):
    m, k, n = 3, 3, band_columns(xs)
    case = lg.Case(2, "NN", m, n, k, 1, pad=3, seed=3)
    got = case.run_device(xs, torch_gpu)
    assert xs.last_kernel() == lg.NAMES[2] + "nn"
    assert lg.same_bits(got, case.gold), int(np.argmax(lg.bits(got) != lg.bits(case.gold))) // case.ldc


# ---- spmdm batch -----------------------------------------------------------------------------------------------------------------
def spmdm_operands(M, N, K, batch, density, seed):
    """items that differ strongly in their number of non-zeros: of every 7 consecutive items one is empty, the next one full,
    the rest at `density`, so an image of the previous item left in LDS changes the result"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (batch, M * K)).astype(np.float32)
    a[rng.random((batch, M * K)) >= density] = 0.0
    a[3::7] = 0.0
    a[4::7] = rng.uniform(0.5, 1.5, a[4::7].shape).astype(np.float32)
    a[batch - 1] = np.float32(1.25)  # the last item of the last trip is full
    b = rng.uniform(-1, 1, batch * K * N).astype(np.float32)
    return a.reshape(-1), b


def slices_of(a, M, K):
    """row starts, column indices and values of every item, by numpy: the entries that are not zero (-0 is zero), row by row"""
    A = a.reshape(-1, M, K)
    keep = A != 0
    rowidx = np.concatenate([np.zeros((A.shape[0], 1), np.int64), np.cumsum(keep.sum(axis=2), axis=1)], axis=1).astype(np.uint16)
    return rowidx, keep


def spmdm_create_past_its_grid(xs, orc, torch, M, N, K, create_kernel, compute_kernels):
    """2 * 32768 + 5 items: every item's row starts and entries against numpy, by way of libxsmm_amd_spmdm_batch_get_slice for items
    at both ends and around the trips, and for all items through the product computed from the slices, between canaries"""
    L = xs.lib()
    batch = ll.sized("spmdm_create", 5)
    a, b = spmdm_operands(M, N, K, batch, 0.15, 1)
    a[7 * M * K + 3] = -0.0
    sb = L.libxsmm_amd_spmdm_batch_create(M, N, K, batch)
    assert sb
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert 0 == L.libxsmm_amd_spmdm_batch_create_slices(sb, b"N", xs.dptr(da))
    assert xs.last_kernel() == create_kernel, xs.last_kernel()
    rowidx, keep = slices_of(a, M, K)
    per = ll.per_trip("spmdm_create")
    ri = np.zeros(M + 1, dtype=np.uint16); ci = np.zeros(M * K, dtype=np.uint16); va = np.zeros(M * K, dtype=np.float32)
    cols = np.broadcast_to(np.arange(K, dtype=np.uint16), (M, K))
    for item in (0, 3, 4, 7, per - 1, per, per + 3, per + 4, 2 * per - 1, 2 * per, 2 * per + 1, batch - 2, batch - 1):
        assert 0 == L.libxsmm_amd_spmdm_batch_get_slice(sb, item, xs.dptr(ri), xs.dptr(ci), xs.dptr(va), M * K)
        nnz = int(rowidx[item, M])
        assert np.array_equal(ri, rowidx[item]), item
        assert np.array_equal(ci[:nnz], cols[keep[item]]) and np.array_equal(bits32(va[:nnz]), bits32(a.reshape(batch, M, K)[item][keep[item]])), item
    ref = np.full(batch * M * N, np.nan, dtype=np.float32)
    orc.spmdm_exec_batch(orc.FMA, M, N, K, 48, "N", "N", "N", 0.0, a, b, ref, batch, 4)
    dc = torch.full((batch * M * N + 64,), float("nan"), dtype=torch.float32, device="cuda")
    be = C.c_float(0.0)
    assert 0 == L.libxsmm_amd_spmdm_batch_compute(sb, b"N", xs.dptr(db), b"N", C.byref(be), xs.dptr(dc[32:]))
    torch.cuda.synchronize()
    assert xs.last_kernel() in compute_kernels, xs.last_kernel()
    got = dc.cpu().numpy()
    L.libxsmm_amd_spmdm_batch_destroy(sb)
    assert np.isnan(got[:32]).all() and np.isnan(got[-32:]).all()
    assert np.array_equal(bits32(got[32:-32]), bits32(ref))


def test_spmdm_batch_create_past_its_grid(xs, orc, torch_gpu):
    """items of 16 x 16 x 16: spmdm_create_staged_kernel (entries collected in LDS), then the pair of compute kernels"""
    spmdm_create_past_its_grid(xs, orc, torch_gpu, 16, 16, 16, "spmdm_create_slices_staged", ("spmdm_compute_mfma|wg_lds", "spmdm_compute_wg_lds"))


def test_spmdm_batch_create_wave_kernel_past_its_grid(xs, orc, torch_gpu):
    """items of 1 x 4 x 65: more than 64 columns, so spmdm_create_kernel (a wavefront per slice, the loop over chunks of 64 columns)
    walks its grid-stride loop over the items; the product comes from spmdm_compute_wg_kernel<1> alone (M is no multiple of 16)"""
    spmdm_create_past_its_grid(xs, orc, torch_gpu, 1, 4, 65, "spmdm_create_slices_wave", ("spmdm_compute_wg_lds",))


def spmdm_compute_case(xs, orc, torch, mfma, M, N, K, batch, tb, betas, kernels):
    L = xs.lib()
    a, b = spmdm_operands(M, N, K, batch, 0.15, 2)
    rng = np.random.default_rng(9)
    old = L.libxsmm_amd_set_mfma(mfma)
    try:
        sb = L.libxsmm_amd_spmdm_batch_create(M, N, K, batch)
        assert sb
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        assert 0 == L.libxsmm_amd_spmdm_batch_create_slices(sb, b"N", xs.dptr(da))
        for beta in betas:
            c = rng.uniform(-1, 1, batch * M * N).astype(np.float32)
            if beta == 0.0:
                c[:] = np.nan
            ref = c.copy()
            orc.spmdm_exec_batch(orc.FMA, M, N, K, 48, "N", tb, "N", beta, a, b, ref, batch, 4)
            dc = torch.full((batch * M * N + 64,), -7.25e11, dtype=torch.float32, device="cuda")
            dc[32:-32].copy_(torch.from_numpy(c))
            be = C.c_float(beta)
            assert 0 == L.libxsmm_amd_spmdm_batch_compute(sb, tb.encode(), xs.dptr(db), b"N", C.byref(be), xs.dptr(dc[32:]))
            torch.cuda.synchronize()
            assert xs.last_kernel() in kernels, xs.last_kernel()
            got = dc.cpu().numpy()
            assert (got[:32] == np.float32(-7.25e11)).all() and (got[-32:] == np.float32(-7.25e11)).all()
            bad = np.flatnonzero(bits32(got[32:-32]) != bits32(ref))
            assert bad.size == 0, (mfma, beta, bad.size, int(bad[0]) // (M * N))
        L.libxsmm_amd_spmdm_batch_destroy(sb)
    finally:
        L.libxsmm_amd_set_mfma(old)


@pytest.mark.parametrize("mfma", [1, 0])
def test_spmdm_batch_compute_many_items_per_work_group(xs, orc, torch_gpu, mfma):
    """16 x 16 x 16, 2 * 2048 + 37 items on at most 2048 (wg_lds) and 768 (mfma) work-groups: matrix cores on -- both kernels share
    the batch, which one takes an item is decided on the device -- and off (wg_lds alone)"""
    batch = ll.sized("spmdm_wg_lds", REST)
    assert batch > 2 * ll.per_trip("spmdm_mfma")
    kernels = ("spmdm_compute_mfma|wg_lds",) if mfma else ("spmdm_compute_wg_lds",)
    spmdm_compute_case(xs, orc, torch_gpu, mfma, 16, 16, 16, batch, "N", (0.0, 1.0, 0.5), kernels)


SPMDM_MFMA_ONLY = r"""
import ctypes as C, importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
xs = importlib.import_module("libxsmm-1_amd")
L = xs.lib()
M, N, K, batch = (int(v) for v in sys.argv[3:7])
a, b, c = np.load(sys.argv[2] + "_a.npy"), np.load(sys.argv[2] + "_b.npy"), np.load(sys.argv[2] + "_c.npy")
dev = []
for x in (a, b, c):
    p = L.libxsmm_amd_device_malloc(x.nbytes)
    assert p and 0 == L.libxsmm_amd_memcpy_h2d(p, xs.dptr(x), x.nbytes)
    dev.append(p)
sb = L.libxsmm_amd_spmdm_batch_create(M, N, K, batch)
assert sb and 0 == L.libxsmm_amd_spmdm_batch_create_slices(sb, b"N", dev[0])
be = C.c_float(float(sys.argv[7]))
assert 0 == L.libxsmm_amd_spmdm_batch_compute(sb, b"N", dev[1], b"N", C.byref(be), dev[2])
assert 0 == L.libxsmm_amd_synchronize() and 0 == L.libxsmm_amd_memcpy_d2h(xs.dptr(c), dev[2], c.nbytes)
np.save(sys.argv[2] + "_out.npy", c)
print("kernel:", xs.last_kernel())
"""


def test_spmdm_batch_compute_matrix_cores_alone(xs, orc, torch_gpu, tmp_path):
    """XSMM_SPMDM_MFMA=1 gives the whole batch to the matrix-core kernel; the setting is read once per process, so this one
    case runs in a process of its own (operands through the library's own allocator)"""
    M = N = K = 16
    batch = ll.sized("spmdm_wg_lds", REST)
    a, b = spmdm_operands(M, N, K, batch, 0.15, 2)
    c = np.random.default_rng(4).uniform(-1, 1, batch * M * N).astype(np.float32)
    ref = c.copy()
    orc.spmdm_exec_batch(orc.FMA, M, N, K, 48, "N", "N", "N", 0.5, a, b, ref, batch, 4)
    base = str(tmp_path / "mfma")
    for name, x in (("a", a), ("b", b), ("c", c)):
        np.save(base + "_%s.npy" % name, x)
    env = dict(os.environ, XSMM_SPMDM_MFMA="1")
    res = subprocess.run([sys.executable, "-c", SPMDM_MFMA_ONLY, ROOT, base, str(M), str(N), str(K), str(batch), "0.5"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "kernel: spmdm_compute_mfma\n" in res.stdout, res.stdout
    assert np.array_equal(bits32(np.load(base + "_out.npy")), bits32(ref))


SPMDM_TILED16 = r"""
import ctypes as C, importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
xs = importlib.import_module("libxsmm-1_amd")
L = xs.lib()
base, M, K = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
a = np.load(base + "_a.npy")
alpha, be = C.c_float(1.0), C.c_float(0.5)
for tag in sys.argv[5:]:
    N, tb = int(tag[:-1]), tag[-1]
    b, c = np.load(base + "_b%s.npy" % tag), np.load(base + "_c%s.npy" % tag)
    h = xs.SpmdmHandle(); slices = C.POINTER(xs.CSRSlice)()
    L.libxsmm_spmdm_init(M, N, K, 1, C.byref(h), C.byref(slices))
    assert 0 == L.libxsmm_amd_spmdm_createSparseSlice_all(C.byref(h), b"N", xs.dptr(a), slices)
    assert 0 == L.libxsmm_amd_spmdm_compute_all(C.byref(h), b"N", tb.encode(), C.byref(alpha), slices, xs.dptr(b), b"N", C.byref(be), xs.dptr(c))
    assert 0 == L.libxsmm_amd_synchronize()
    print("kernel %s: %s" % (tag, xs.last_kernel()))
    L.libxsmm_spmdm_destroy(C.byref(h))
    np.save(base + "_out%s.npy" % tag, c)
"""


def test_spmdm_tiled_kernel_sixteen_row_tiles(xs, orc, torch_gpu, tmp_path):
    """XSMM_SPMDM_TILE_ROWS=16 gives the whole-problem calls to spmdm_tiled_kernel<*, *, 4> (tiles of 16 rows, four waves): the
    setting is read once per process, so the four instantiations run in one process of their own, on pageable host operands.
    130 x N x 200 at 15 %, beta = 0.5: N = 516 takes 16-byte accesses, N = 515 element-wide ones, each with B plain and transposed;
    ragged tiles in every direction (130 = 8 * 16 + 2 rows, 516 = 2 * 256 + 4 columns, 200 = 3 * 64 + 8)."""
    M, K = 130, 200
    rng = np.random.default_rng(16)
    a = rng.uniform(-1, 1, M * K).astype(np.float32)
    a[rng.random(M * K) >= 0.15] = 0.0
    a[5 * K:6 * K] = 0.0                      # an empty row
    a[17 * K:18 * K] = np.float32(0.75)       # a full one
    base = str(tmp_path / "tiled16")
    np.save(base + "_a.npy", a)
    tags, refs = [], {}
    for N in (516, 515):
        for tb in "NT":
            tag = "%d%s" % (N, tb)
            b = rng.uniform(-1, 1, K * N).astype(np.float32)
            c = rng.uniform(-1, 1, M * N).astype(np.float32)
            ref = c.copy()
            orc.spmdm_exec(orc.FMA, M, N, K, 48, "N", tb, "N", 0.5, a, b, ref)
            np.save(base + "_b%s.npy" % tag, b); np.save(base + "_c%s.npy" % tag, c)
            tags.append(tag); refs[tag] = ref
    env = dict(os.environ, XSMM_SPMDM_TILE_ROWS="16")
    res = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", SPMDM_TILED16, ROOT, base, str(M), str(K)] + tags,
                         capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    for tag in tags:
        assert "kernel %s: spmdm_compute_tiled16\n" % tag in res.stdout, res.stdout
        got = np.load(base + "_out%s.npy" % tag)
        bad = np.flatnonzero(bits32(got) != bits32(refs[tag]))
        assert bad.size == 0, (tag, bad.size, int(bad[0]))


def test_spmdm_batch_compute_element_kernel(xs, orc, torch_gpu):
    """TRANS_B goes to the kernel with a lane per element of C: 3 x 3 x 5 items, 2 * 2097152 + 29 elements"""
    total = ll.sized("spmdm_generic", 29)
    assert total % 9 == 0
    spmdm_compute_case(xs, orc, torch_gpu, 1, 3, 3, 5, total // 9, "T", (0.5,), ("spmdm_compute_elem",))


# ---- fsspmdm without its operator kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fsspmdm_csr_columns(xs, orc, torch_gpu, dtype, monkeypatch):
    """LIBXSMM_AMD_JIT=0: the CSR kernel with a lane per column of C, 2 * 2097152 + 16 columns in panels of 16"""
    torch, L = torch_gpu, xs.lib()
    monkeypatch.setenv("LIBXSMM_AMD_JIT", "0")
    M, K, N = 5, 5, 16
    ncols = 2 * ll.per_trip("fsspmdm_csr") + N
    panels = ncols // N
    rng = np.random.default_rng(11)
    pal = np.array([0.25, -0.5, 0.75, 1.0, -1.25, 1.5, -2.0])
    A = np.where(rng.random((M, K)) < 0.5, pal[rng.integers(0, 7, (M, K))], 0.0)
    A[np.arange(M), np.arange(M)] = 3.0  # no row without entries (the reference's two paths disagree there for beta = 0)
    A = np.ascontiguousarray(A.astype(dtype))
    B = rng.uniform(-1, 1, (K, ncols)).astype(dtype)
    suffix = "d" if dtype == np.float64 else "s"
    dB = torch.from_numpy(B).cuda()
    u = np.uint64 if dtype == np.float64 else np.uint32
    for beta in (0.0, 1.0):
        Cin = np.full((M, ncols), np.nan, dtype=dtype) if beta == 0.0 else rng.uniform(-1, 1, (M, ncols)).astype(dtype)
        ref = Cin.copy()
        h = orc.Fsspmdm(A, M, ncols, K, K, ncols, ncols, 1.0, beta, have_avx512=True)  # (the oracle walks its N in chunks of 16 / 8 itself)
        assert h.sparse() == 1
        h.execute(B, ref); h.close()
        hd = getattr(L, "libxsmm_%sfsspmdm_create" % suffix)(M, N, K, K, ncols, ncols, 1.0, beta, xs.dptr(A))
        assert hd
        dC = torch.from_numpy(Cin).cuda()
        assert 0 == getattr(L, "libxsmm_amd_%sfsspmdm_execute_batch" % suffix)(hd, xs.dptr(dB), xs.dptr(dC), panels)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "fsspmdm_f%d_csr_cols" % (64 if dtype == np.float64 else 32)
        got = dC.cpu().numpy()
        getattr(L, "libxsmm_%sfsspmdm_destroy" % suffix)(hd)
        bad = np.flatnonzero((got.view(u) != ref.view(u)).any(axis=0))
        assert bad.size == 0, (beta, bad.size, int(bad[0]))


# ---- low-precision SMM -----------------------------------------------------------------------------------------------------------
def bf16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def widen(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def lowp_batch_gold(kind, m, n, k, a, b, c):
    """the gold loops of the reference's harness (samples/xgemm/kernel.c; tests/test_lowp.py restates them for one item) over a
    batch of tight items, beta = 1: A in pairs of k, terms in ascending k, every float operation rounded on its own"""
    batch = c.size // (m * n)
    A = a.reshape(batch, k // 2, m, 2)
    B = b.reshape(batch, n, k)
    C2 = c.reshape(batch, n, m)
    if kind == 0:
        acc = C2.astype(np.int64)
        for kk in range(k):
            acc += B[:, :, kk, None].view(np.int16).astype(np.int64) * A[:, kk // 2, None, :, kk % 2].view(np.int16).astype(np.int64)
        return (acc & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(-1)
    acc = widen(C2) if kind == 3 else C2.copy()
    for kk in range(k):
        acc = acc + widen(B[:, :, kk, None]) * widen(A[:, kk // 2, None, :, kk % 2])
    return (bf16(acc) if kind == 3 else acc).reshape(-1)


@pytest.mark.parametrize("kind", [0, 2, 3])
def test_smm_lowp_more_items_than_work_groups(xs, orc, torch_gpu, kind, monkeypatch):
    """2 * 2048 + 3 items on 2048 work-groups that park A and B of an item in LDS: kinds i16 -> i32, bf16 -> f32, bf16 -> bf16.
    (i16 -> f32 takes its scaling factor as an argument of the single call: no entry point gives it a batch.)"""
    torch, L = torch_gpu, xs.lib()
    monkeypatch.setenv("LIBXSMM_AMD_JIT_MINBATCH", "1000000")  # the pre-compiled kernel, not the specialised streaming form
    m, n, k = 16, 3, 4
    batch = ll.sized("smm_lowp", 3)
    rng = np.random.default_rng(kind)
    if kind == 0:
        a = rng.integers(-32768, 32768, batch * m * k).astype(np.int16).view(np.uint16)
        b = rng.integers(-32768, 32768, batch * k * n).astype(np.int16).view(np.uint16)
        c = rng.integers(-2 ** 31, 2 ** 31, batch * m * n).astype(np.int32)
    else:
        a, b = lg.rand_bf16(rng, batch * m * k), lg.rand_bf16(rng, batch * k * n)
        c = rng.uniform(-1, 1, batch * m * n).astype(np.float32) if kind == 2 else bf16(rng.uniform(-1, 1, batch * m * n))
    ref = lowp_batch_gold(kind, m, n, k, a, b, c)
    for i in (0, 2047, 2048, 4096, batch - 1):  # the batched restatement against the oracle's gold loop
        one = c[i * m * n:(i + 1) * m * n].copy()
        assert 0 == orc.gemm_lowp(kind, 0, m, n, k, m, k, m, a[i * m * k:(i + 1) * m * k], b[i * k * n:(i + 1) * k * n], one, 1.0)
        assert np.array_equal(one.view(np.uint8), ref[i * m * n:(i + 1) * m * n].view(np.uint8)), i
    blob = xs.DescriptorBlob()
    L.libxsmm_gemm_descriptor_dinit2.restype = C.c_void_p
    L.libxsmm_gemm_descriptor_dinit2.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_double, C.c_double, C.c_int, C.c_int]
    ip, op = {0: (xs.I16, xs.I32), 2: (xs.BF16, xs.F32), 3: (xs.BF16, xs.BF16)}[kind]
    desc = L.libxsmm_gemm_descriptor_dinit2(C.byref(blob), ip, op, m, n, k, m, k, m, 1.0, 1.0, 0, 0)
    assert desc
    da, db = (torch.from_numpy(x.view(np.int16)).cuda() for x in (a, b))
    pad = 64
    guard = np.full(pad, 0x7b7b if kind == 3 else 0x7b7b7b7b, dtype=np.uint16 if kind == 3 else np.uint32)
    host = np.concatenate([guard, c.view(guard.dtype), guard])
    dc = torch.from_numpy(host.view(np.int16 if kind == 3 else np.int32)).cuda()
    assert 0 == L.libxsmm_amd_gemm_batch_strided(C.c_void_p(desc), da.data_ptr(), db.data_ptr(), dc.data_ptr() + pad * guard.itemsize, m * k, k * n, m * n, batch)
    torch.cuda.synchronize()
    assert xs.last_kernel() == {0: "smm_i16i32_lowp", 2: "smm_bf16f32_lowp", 3: "smm_bf16_lowp"}[kind]
    got = dc.cpu().numpy().view(guard.dtype)
    assert np.array_equal(got[:pad], guard) and np.array_equal(got[-pad:], guard)
    bad = np.flatnonzero(got[pad:-pad] != ref.view(guard.dtype))
    assert bad.size == 0, (bad.size, int(bad[0]) // (m * n))


@pytest.mark.parametrize("kind", [2, 3])
def test_smm_lowp_batch_reduce_of_many_products(xs, orc, torch_gpu, kind):
    """the bf16 batch-reduce kernels over 2 * 2048 + 3 products: one chain of fp32 sums through all of them (the chain is the
    operation: the oracle's gold loop is called product after product, as tests/test_lowp.py does)"""
    torch, L = torch_gpu, xs.lib()
    m, n, k = 16, 3, 4
    cnt = ll.sized("smm_lowp", 3)
    for name in ("libxsmm_bsmmdispatch_reducebatch", "libxsmm_bmmdispatch_reducebatch"):
        f = getattr(L, name); f.restype = C.c_void_p
        f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 7
    disp = L.libxsmm_bsmmdispatch_reducebatch if kind == 2 else L.libxsmm_bmmdispatch_reducebatch
    rng = np.random.default_rng(kind)
    beta = C.c_float(1.0)
    fn = disp(m, n, k, None, None, None, None, C.addressof(beta), None, None)
    assert fn
    a, b = bf16(rng.uniform(-1, 1, cnt * m * k)), bf16(rng.uniform(-1, 1, cnt * k * n))
    c = rng.uniform(-1, 1, m * n).astype(np.float32) if kind == 2 else bf16(rng.uniform(-1, 1, m * n))
    chain = c.copy() if kind == 2 else widen(c)
    for i in range(cnt):
        assert 0 == orc.gemm_lowp(2, 0, m, n, k, m, k, m, a[i * m * k:(i + 1) * m * k], b[i * k * n:(i + 1) * k * n], chain, 1.0)
    ref = chain if kind == 2 else bf16(chain)
    da, db = (torch.from_numpy(x.view(np.int16)).cuda() for x in (a, b))
    qa = torch.from_numpy(da.data_ptr() + np.arange(cnt, dtype=np.int64) * m * k * 2).cuda()
    qb = torch.from_numpy(db.data_ptr() + np.arange(cnt, dtype=np.int64) * k * n * 2).cuda()
    dc = torch.from_numpy(c.view(np.int16) if kind == 3 else c).cuda()
    xs.call_kernel(fn, qa, qb, dc, np.array([cnt], dtype=np.uint64))
    torch.cuda.synchronize()
    assert xs.last_kernel() == ("smm_bf16f32_reduce_lowp" if kind == 2 else "smm_bf16_reduce_lowp")
    got = dc.cpu().numpy()
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8))


# ---- dense generic kernel and the check of the order of C ------------------------------------------------------------------------
def test_smm_generic_and_c_order(xs, orc, torch_gpu, monkeypatch):
    """LIBXSMM_AMD_JIT=0 leaves a 3 x 3 x 3 fp64 batch to the pre-compiled generic kernel (four items per work-group, 4096
    work-groups): a strided batch of 2 * 4 * 4096 + rest items with a C each, an index batch of as many whose C come in runs of
    three, and an index batch past the 512 * 256 items one pass of the order check covers, whose last trip alone holds a C block
    that comes back out of order sixteen times."""
    torch, L = torch_gpu, xs.lib()
    monkeypatch.setenv("LIBXSMM_AMD_JIT", "0")
    m = n = k = 3
    sz = m * n
    ppb = 256 // ll.LIMITS["smm_generic"]["lanes_small"]
    batch = ppb * ll.sized("smm_generic", REST) - 1
    rng = np.random.default_rng(21)
    a, b = rng.uniform(-1, 1, batch * sz), rng.uniform(-1, 1, batch * sz)
    c = rng.uniform(-1, 1, batch * sz)
    # strided, a C per item
    ref = c.copy()
    orc.gemm_batch_strided(orc.FMA, 0, m, n, k, m, k, m, a, b, ref, sz, sz, sz, batch, 4)
    blob, desc = xs.descriptor(xs.F64, m, n, k, m, k, m, 1.0, 1.0)
    assert desc
    da, db, dc = (torch.from_numpy(v).cuda() for v in (a, b, c))
    assert 0 == L.libxsmm_amd_gemm_batch_strided(desc, xs.dptr(da), xs.dptr(db), xs.dptr(dc), sz, sz, sz, batch)
    torch.cuda.synchronize()
    assert xs.last_kernel() == "smm_f64_generic_w8", xs.last_kernel()
    assert np.array_equal(dc.cpu().numpy(), ref)
    # index batch, runs of three items per C
    ia = (np.arange(batch) * sz).astype(np.int32)
    ic = ((np.arange(batch) // 3) * sz).astype(np.int32)
    ref = c.copy()
    assert 0 == orc.gemm_batch_idx(orc.FMA, 0, m, n, k, m, k, m, a, b, ref, 0, ia, ia, ic, batch)
    dc = torch.from_numpy(c).cuda()
    xs.gemm_batch(xs.F64, "N", "N", m, n, k, 1.0, da, m, db, k, 1.0, dc, m, 0, 4, ia, ia, ic, batch)
    torch.cuda.synchronize()
    assert xs.last_kernel() == "smm_f64_generic_w8", xs.last_kernel()
    assert np.array_equal(dc.cpu().numpy(), ref)
    # the order check: ascending C, but for 16 items of the last trip, every other one, that return to one and the same C
    big = ll.sized("c_order", REST)
    ia = (np.arange(big) % batch * sz).astype(np.int32)  # (A and B of the first batch, over and over)
    ic = np.arange(big, dtype=np.int64)
    cbig = rng.uniform(-1, 1, big * sz)
    first = 2 * ll.per_trip("c_order") + 3
    for j in range(first, first + 32, 2):
        ic[j] = ic[j - 2]
    ic = (ic * sz).astype(np.int32)
    assert (np.diff(ic[:2 * ll.per_trip("c_order")]) > 0).all() and (np.diff(ic) < 0).sum() == 16
    ref = cbig.copy()
    assert 0 == orc.gemm_batch_idx(orc.FMA, 0, m, n, k, m, k, m, a, b, ref, 0, ia, ia, ic, big)
    dc = torch.from_numpy(cbig).cuda()
    xs.gemm_batch(xs.F64, "N", "N", m, n, k, 1.0, da, m, db, k, 1.0, dc, m, 0, 4, ia, ia, ic, big)
    torch.cuda.synchronize()
    # C blocks that repeat out of order are summed with atomic adds of whole products: the comparison and
    # the bound of tests/test_smm_gpu.py::test_unsorted_duplicate_c_uses_atomics_within_tolerance. A check that misses the
    # repeats lets 17 items update one C side by side without atomics: products of order 1 get lost.
    err = rel_err(ref, dc.cpu().numpy())
    print("out-of-order C past the order check: relative deviation %.3g" % err)
    assert err <= 1e-12


# ---- xcopy -------------------------------------------------------------------------------------------------------------------------
def test_matcopy_more_column_slabs_than_the_grid(xs, torch_gpu):
    """rows of one 2-byte element, 256 columns per work-group: 2 * 65535 + 37 slabs of columns, the last one partial"""
    lim = ll.LIMITS["xcopy_rows"]
    n = lim["threads"] * ll.sized("xcopy_rows", REST) - 91
    src = xc.Stack(2, 1, n, ld=1, rng=np.random.default_rng(1))
    dst = xc.Stack(2, 1, n, ld=2, fill=False)
    want = xc.expected_copy(dst, src)
    di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
    xs.matcopy(do.ptr(), di.ptr(), 2, 1, n, src.ld, dst.ld)
    torch_gpu.cuda.synchronize()
    assert xs.last_kernel() == "xcopy_copy"
    assert xc.first_difference(do.get(), want) is None and xc.first_difference(di.get(), src.host) is None


def test_stack_copy_past_the_generic_grid(xs, torch_gpu):
    """3 x 3 items of 2-byte elements with padded columns: 2 * 65536 * 256 + 43 elements on the kernel with a lane per element"""
    total = ll.sized("xcopy_generic", 43)
    assert total % 9 == 0
    batch = total // 9
    src = xc.Stack(2, 3, 3, ld=4, batch=batch, rng=np.random.default_rng(2))
    dst = xc.Stack(2, 3, 3, ld=5, batch=batch, fill=False)
    want = xc.expected_copy(dst, src)
    di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
    assert 0 == xs.matcopy_batch(do.ptr(), di.ptr(), 2, 3, 3, src.ld, dst.ld, src.stride, dst.stride, batch)
    torch_gpu.cuda.synchronize()
    assert xs.last_kernel() == "xcopy_generic_copy"
    assert xc.first_difference(do.get(), want) is None and xc.first_difference(di.get(), src.host) is None


def test_stack_transpose_more_chunks_than_work_groups(xs, torch_gpu):
    """27 x 27 items of 8 bytes: two of them make a chunk of the LDS kernel (an image has 27 columns of 27 units, 5832 bytes);
    2 * 16384 + 37 chunks, the last one of a single item"""
    lim = ll.LIMITS["xcopy_stack_trans"]
    ts, m = 8, 27
    G = lim["lds_chunk"] // (m * (m | 1) * ts)
    assert G == 2
    batch = G * ll.sized("xcopy_stack_trans", REST) - 1
    src = xc.Stack(ts, m, m, batch=batch, rng=np.random.default_rng(3))
    dst = xc.Stack(ts, m, m, batch=batch, fill=False)
    want = xc.expected_trans(dst, src)
    di, do = xc.Device(torch_gpu, src), xc.Device(torch_gpu, dst)
    assert 0 == xs.otrans_batch(do.ptr(), di.ptr(), ts, m, m, m, m, src.stride, dst.stride, batch)
    torch_gpu.cuda.synchronize()
    assert xs.last_kernel() == "xcopy_stack_trans"
    assert xc.first_difference(do.get(), want) is None and xc.first_difference(di.get(), src.host) is None
