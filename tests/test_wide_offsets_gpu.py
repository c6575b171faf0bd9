"""Operands whose element offsets pass 2^31 (and whose byte offsets pass 2^32): the 64-bit instantiation of the quantise layout
kernel, leading dimensions of 2^30 + 7 in the tiled GEMMs, a strided batch with a C stride of 2^20 elements, fsspmdm at the
leading dimension of BASELINE config 3, pooling over more than 2^31 elements, and packed operands whose packs lie 2^21 elements apart. The convolution layer refuses tensors of 2^31
elements (its offsets are 32-bit): it runs on the largest ones it accepts, an input and a filter just below 2^31 elements.

The operands are built on the device and never travel whole. Each case checks (i) a sample gathered to the host against the
family's host reference -- everywhere the call writes where that is small, otherwise at least 256 places that include the
first and the last element and the neighbours of offset 2^31 --, (ii) canaries: what the call must not touch, compared on the
device in slabs, and (iii) a property of the whole array where there is one. A case needs up to 20 GiB (the RNN cell layer with its
three state tensors of 8 GiB: 26 GiB) and skips only where torch.cuda.mem_get_info() shows less free memory than it needs; on an
MI355X none does.

The RNN cell layer refuses tensors of 2^31 elements as well; its case has states just below that, whose second step begins just below
byte 2^32 and ends near byte 2^33. Its rows are independent recurrences, so the tensors repeat one seeded block of rows and every
period of what the pass writes is compared on the device with the restatement of that block."""
import ctypes as C
import glob
import os
import time

import numpy as np
import pytest

import conv_common as cc
import launch_limits as ll
import lowp_gemm_common as lg
import packed_common as pk
import pool_common as pc
import quant_common as qc
import rnn_common as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GiB = 1 << 30
W31 = 1 << 31
SLAB = 1 << 28  # elements compared at once on the device


def need(torch, nbytes, most=20 * GiB):
    assert nbytes <= most
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + GiB:
        pytest.skip("%.1f GiB free, the case needs %.1f" % (free / GiB, nbytes / GiB + 1))


def all_equal(torch, t, value, lo, hi):
    """t[lo:hi] == value everywhere, slab by slab"""
    for s in range(lo, hi, SLAB):
        if not bool((t[s:min(hi, s + SLAB)] == value).all()):
            return False
    return True


def none_is(torch, t, pred):
    for s in range(0, t.numel(), SLAB):
        if bool(pred(t[s:s + SLAB]).any()):
            return False
    return True


# ---- quantise: the layout kernel with 64-bit indices ------------------------------------------------------------------------------
def act_source_at(o, N, Cc, H, W, cb32, cb16, lp):
    """tests/quant_common.py:act_source for single output positions (int64 arrays)"""
    cb = cb16 * lp
    cin = o % cb; o = o // cb
    i4 = o % W; o = o // W
    i3 = o % H; o = o // H
    i2 = o % (Cc // cb); i1 = o // (Cc // cb)
    c = i2 * cb + cin
    return (((i1 * (Cc // cb32) + c // cb32) * H + i3) * W + i4) * cb32 + c % cb32


def act_dest_at(s, N, Cc, H, W, cb32, cb16, lp):
    """the output position that reads input position s"""
    cb = cb16 * lp
    fi5 = s % cb32; s = s // cb32
    i4 = s % W; s = s // W
    i3 = s % H; s = s // H
    fi2 = s % (Cc // cb32); i1 = s // (Cc // cb32)
    c = fi2 * cb32 + fi5
    return (((i1 * (Cc // cb) + c // cb) * H + i3) * W + i4) * cb + c % cb


def fil_source_at(o, K, Cc, R, S, cb32, cb16, kb32, kb16, lp):
    i7 = o % lp; o = o // lp
    i6 = o % kb16; o = o // kb16
    i5 = o % cb16; o = o // cb16
    i4 = o % S; o = o // S
    i3 = o % R; o = o // R
    cblk = Cc // (cb16 * lp)
    i2 = o % cblk; i1 = o // cblk
    k = i1 * kb16 + i6
    c = (i2 * cb16 + i5) * lp + i7
    return ((((k // kb32 * (Cc // cb32) + c // cb32) * R + i3) * S + i4) * cb32 + c % cb32) * kb32 + k % kb32


def fil_dest_at(s, K, Cc, R, S, cb32, cb16, kb32, kb16, lp):
    fi6 = s % kb32; s = s // kb32
    fi5 = s % cb32; s = s // cb32
    i4 = s % S; s = s // S
    i3 = s % R; s = s // R
    fi2 = s % (Cc // cb32); fi1 = s // (Cc // cb32)
    k, c = fi1 * kb32 + fi6, fi2 * cb32 + fi5
    cb = cb16 * lp
    return (((((k // kb16 * (Cc // cb) + c // cb) * R + i3) * S + i4) * cb16 + (c % cb) // lp) * kb16 + k % kb16) * lp + c % lp


def test_the_index_maps_of_this_file():
    """single positions against the whole maps of tests/quant_common.py, both directions (no GPU involved)"""
    for case in qc.ACT_CASES:
        n = int(np.prod(case[:4]))
        o = np.arange(n, dtype=np.int64)
        assert np.array_equal(act_source_at(o, *case), qc.act_source(*case)) and np.array_equal(act_dest_at(act_source_at(o, *case), *case), o)
    for case in qc.FIL_CASES:
        n = int(np.prod(case[:4]))
        o = np.arange(n, dtype=np.int64)
        assert np.array_equal(fil_source_at(o, *case), qc.fil_source(*case)) and np.array_equal(fil_dest_at(fil_source_at(o, *case), *case), o)


WIDE_ACT = (33, 64, 1024, 1024, 16, 4, 2)        # N, C, H, W, cb32, cb16, lp: 2^31 + 2^26 elements
WIDE_FIL = (2048, 2048, 23, 23, 16, 4, 16, 16, 2)  # K, C, R, S, cb32, cb16, kb32, kb16, lp: 529 * 2^22 elements


@pytest.mark.parametrize("layout", ["act", "fil"])
def test_quant_layout_past_2_31_outputs(xs, torch_gpu, layout):
    """quant_layout_kernel<MODE, unsigned long long>: the largest magnitude sits three elements before the end of the input; 4096
    and some output positions on the host -- both ends, the neighbours of output 2^31 (byte 2^32 of the output), and the
    outputs that read the neighbours of input 2^30 (byte 2^32) and 2^31. No output keeps the fill, none exceeds what the scale
    allows: every position was written."""
    torch = torch_gpu
    case = WIDE_ACT if layout == "act" else WIDE_FIL
    src_at, dest_at = (act_source_at, act_dest_at) if layout == "act" else (fil_source_at, fil_dest_at)
    fn = xs.dnn_quantize_act if layout == "act" else xs.dnn_quantize_fil
    total = int(np.prod([int(v) for v in case[:4]]))
    assert total >= ll.threshold("quant_layout_wide") and total % 2 == 0
    guard, fill = 64, 0x7b7b
    need(torch, total * 6)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    x = torch.rand(total, device="cuda", generator=g)
    x.sub_(0.5).mul_(0.9)
    x[total - 3] = 1.75
    x[5] = 0.0
    dq = torch.full((total + 2 * guard,), fill, dtype=torch.int16, device="cuda")
    assert dq.data_ptr() % 16 == 0
    mode, shift = qc.NEAREST_ROUND, 2
    scf = fn(x, dq[guard:guard + total], *case, shift, mode)
    torch.cuda.synchronize()
    assert xs.last_kernel() == "quant_" + layout
    rng = np.random.default_rng(3)
    near = np.array([-2, -1, 0, 1, 2], dtype=np.int64)
    o = np.concatenate([[0, 1, total - 2, total - 1], W31 + near, dest_at(W31 + near, *case), dest_at((1 << 30) + near, *case),
                        dest_at(np.array([total - 3, total - 1, 0, 5], dtype=np.int64), *case), rng.integers(0, total, 4096)]).astype(np.int64)
    o = np.unique(o)
    s = src_at(o, *case)
    assert o.size >= 256 and s.min() == 0 and s.max() == total - 1 and (s > W31).any() and (o > W31).any()
    xin = x[torch.from_numpy(s).cuda()].cpu().numpy()
    gq, gscf = qc.quantize(np.concatenate([xin, [np.float32(1.75)]]), shift, mode)  # (the maximum is part of the sample anyway)
    got = dq[guard:guard + total][torch.from_numpy(o).cuda()].cpu().numpy()
    assert scf == gscf and np.array_equal(got, gq[:-1]), (scf, gscf, o[got != gq[:-1]][:8])
    assert all_equal(torch, dq, fill, 0, guard) and all_equal(torch, dq, fill, guard + total, total + 2 * guard)
    limit = int(np.abs(qc.quantize(np.array([1.75], dtype=np.float32), shift, mode)[0].astype(np.int64)).max()) + 1
    assert limit < fill and none_is(torch, dq[guard:guard + total], lambda t: (t > limit) | (t < -limit))


# ---- tiled GEMM: a leading dimension of 2^30 + 7 -----------------------------------------------------------------------------------
WIDE_LD = (1 << 30) + 7
CANARY = -7.25e11


def strided_columns(t, ld, rows, cols):
    return t.as_strided((cols, rows), (ld, 1))


@pytest.mark.parametrize("wide", ["ldc", "ldb"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_tgemm_leading_dimension_past_2_30(xs, orc, torch_gpu, kind, wide):
    """m = T + 1, n = 3, k = 35, NN: column 2 of C (of B) starts at element 2^31 + 14. Every element of the product against the
    reference on tight copies (the leading dimension only places the columns); all that lies between the columns keeps its bits"""
    torch = torch_gpu
    T = xs.lib().libxsmm_amd_gemm_tile()
    m, n, k = T + 1, 3, 35
    ldb, ldc = (WIDE_LD, m + 3) if wide == "ldb" else (k, WIDE_LD)
    assert 2 * WIDE_LD > W31
    rng = np.random.default_rng(5)
    if kind == "f32":
        a, b = rng.uniform(-1, 1, m * k).astype(np.float32), rng.uniform(-1, 1, k * n).astype(np.float32)
    else:
        a, b = lg.rand_bf16(rng, m * k), lg.rand_bf16(rng, k * n)
    c = rng.uniform(-1, 1, m * n).astype(np.float32)
    if kind == "f32":
        gold = c.copy()
        orc.smm(orc.FMA, 0, m, n, k, m, k, m, a, b, gold)
    else:
        gold = lg.reference(2, False, False, m, n, k, a, m, b, k, 1, c, m)
    in_t = torch.float32 if kind == "f32" else torch.int16
    nb, nc = (n - 1) * ldb + k, (n - 1) * ldc + m
    need(torch, nb * (4 if kind == "f32" else 2) + nc * 4)
    bfill = 0.0 if kind == "f32" else 0
    db = torch.full((nb,), bfill, dtype=in_t, device="cuda")
    dc = torch.full((nc,), CANARY, dtype=torch.float32, device="cuda")
    da = torch.from_numpy(a if kind == "f32" else a.view(np.int16)).cuda()
    strided_columns(db, ldb, k, n).copy_(torch.from_numpy((b if kind == "f32" else b.view(np.int16)).reshape(n, k)))
    strided_columns(dc, ldc, m, n).copy_(torch.from_numpy(c.reshape(n, m)))
    if kind == "f32":
        keep, h = xs.gemm_handle(xs.F32, xs.F32, "N", "N", m, n, k, m, ldb, ldc, 1.0, 1.0)
        assert h
        xs.gemm_thread(h, da, db, dc)
    else:
        assert 0 == xs.gemm_lowp(xs.BF16, xs.F32, "N", "N", m, n, k, da, m, db, ldb, 1, dc, ldc)
    torch.cuda.synchronize()
    assert xs.last_kernel() == ("tgemm_f32_nn" if kind == "f32" else lg.NAMES[2] + "nn")
    got = strided_columns(dc, ldc, m, n).cpu().numpy().reshape(-1)
    assert lg.same_bits(got, gold), int(np.argmax(lg.bits(got) != lg.bits(gold)))
    for j in range(n - 1):  # between the columns
        assert all_equal(torch, dc, CANARY, j * ldc + m, (j + 1) * ldc), j
        assert all_equal(torch, db, bfill, j * ldb + k, (j + 1) * ldb), j
    hb = strided_columns(db, ldb, k, n).cpu().numpy().reshape(-1)
    assert np.array_equal(hb if kind == "f32" else hb.view(np.uint16), b)


# ---- strided dense batch: the items of C 2^20 elements apart ----------------------------------------------------------------------
@pytest.mark.parametrize("config", [("f32", 32, 1), ("f32", 32, 0), ("f64", 23, 0)])
def test_strided_batch_with_c_items_2_20_apart(xs, orc, torch_gpu, config):
    """2049 items, A and B tight: the last C starts at element 2^31. All items against the oracle (fp32 32^3 on the matrix cores within
    the bound tests/test_edge_gpu.py uses for them, the scalar kernels bit for bit); the gaps between the items keep their bits"""
    torch, L = torch_gpu, xs.lib()
    name, m, mfma = config
    dtype, tt, prec = (np.float32, torch.float32, xs.F32) if name == "f32" else (np.float64, torch.float64, xs.F64)
    stride, batch, sz = 1 << 20, 2049, m * m
    assert (batch - 1) * stride >= W31
    need(torch, ((batch - 1) * stride + sz) * np.dtype(dtype).itemsize)
    rng = np.random.default_rng(m)
    a, b, c = (rng.uniform(-1, 1, batch * sz).astype(dtype) for _ in range(3))
    ref = c.copy()
    orc.gemm_batch_strided(orc.FMA, 0, m, m, m, m, m, m, a, b, ref, sz, sz, sz, batch, 4)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dc = torch.full(((batch - 1) * stride + sz,), CANARY, dtype=tt, device="cuda")
    items = dc.as_strided((batch, sz), (stride, 1))
    items.copy_(torch.from_numpy(c.reshape(batch, sz)))
    blob, desc = xs.descriptor(prec, m, m, m, m, m, m, 1.0, 1.0)
    assert desc
    old = L.libxsmm_amd_set_mfma(mfma)
    try:
        assert 0 == L.libxsmm_amd_gemm_batch_strided(desc, xs.dptr(da), xs.dptr(db), xs.dptr(dc), sz, sz, stride, batch)
        torch.cuda.synchronize()
    finally:
        L.libxsmm_amd_set_mfma(old)
    kernel = xs.last_kernel()
    assert kernel == {("f32", 1): "smm_f32_32x32x32_mfma", ("f32", 0): "smm_f32_32x32x32_fma", ("f64", 0): "smm_f64_jit_shape"}[(name, mfma)], kernel
    got = items.cpu().numpy().reshape(-1)
    if mfma:
        assert np.max(np.abs(got - ref)) <= 1e-6 * np.max(np.abs(ref))
    else:
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (bad.size, int(bad[0]) // sz)
    gaps = dc[:(batch - 1) * stride].view(batch - 1, stride)[:, sz:]
    for i in range(0, batch - 1, 256):
        assert bool((gaps[i:i + 256] == CANARY).all()), i


# ---- fsspmdm at the leading dimension of BASELINE config 3 ------------------------------------------------------------------------
def test_fsspmdm_at_the_leading_dimension_of_config_3(xs, orc, torch_gpu):
    """ldb = ldc = 25 165 824 (262 144 panels of 96 columns), fp32, the PyFR operator p4_pri_m3 (75 x 105: the largest of
    tests/golden/mtx/pyfr whose B and C fit 20 GiB together). 64 panels each at the start, in the middle and at the end of the
    row; rows 86 and up of B start past element 2^31, rows 43 and up of C past byte 2^32. The rest of C is canary."""
    torch, L = torch_gpu, xs.lib()
    ld, N, npan = 25165824, 96, 64
    path = os.path.join(GOLDEN, "mtx", "pyfr", "p4_pri_m3-sp.mtx")
    assert path in glob.glob(os.path.join(GOLDEN, "mtx", "pyfr", "*-sp.mtx"))
    rowptr, colidx, vals, M, K, nnz = orc.read_csr(path)
    A = np.zeros((M, K), dtype=np.float32)
    A[np.repeat(np.arange(M), np.diff(rowptr)), colidx] = vals.astype(np.float32)
    assert (K - 1) * ld > W31 and (M - 1) * ld * 4 > (1 << 32)
    need(torch, (M + K) * ld * 4)
    width = npan * N
    starts = [0, (ld // N // 2) * N, ld - width]
    rng = np.random.default_rng(9)
    dB = torch.zeros((K, ld), dtype=torch.float32, device="cuda")
    dC = torch.full((M, ld), CANARY, dtype=torch.float32, device="cuda")
    hd = L.libxsmm_sfsspmdm_create(M, N, K, K, ld, ld, 1.0, 1.0, xs.dptr(A))
    assert hd
    want = []
    for s in starts:
        B, Cin = rng.uniform(-1, 1, (K, width)).astype(np.float32), rng.uniform(-1, 1, (M, width)).astype(np.float32)
        dB[:, s:s + width].copy_(torch.from_numpy(B))
        dC[:, s:s + width].copy_(torch.from_numpy(Cin))
        ref = Cin.copy()
        h = orc.Fsspmdm(A, M, width, K, K, width, width, 1.0, 1.0, have_avx512=False)
        h.execute(B, ref); h.close()
        want.append(ref)
    for s in starts:
        assert 0 == L.libxsmm_amd_sfsspmdm_execute_batch(hd, C.c_void_p(dB.data_ptr() + 4 * s), C.c_void_p(dC.data_ptr() + 4 * s), npan)
    torch.cuda.synchronize()
    assert xs.last_kernel().startswith("fsspmdm_")
    L.libxsmm_sfsspmdm_destroy(hd)
    for s, ref in zip(starts, want):
        got = dC[:, s:s + width].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), s
    for lo, hi in ((starts[0] + width, starts[1]), (starts[1] + width, starts[2])):
        for r in range(M):
            assert bool((dC[r, lo:hi] == CANARY).all()), (r, lo)


# ---- pooling over more than 2^31 elements ------------------------------------------------------------------------------------------
POOL_WIDE = dict(H=64, W=64, R=2, S=2, u=2, v=2, N=33, C=16 * 1000)  # 33000 items of 64 x 64 x 16: items 32768 and up start past 2^31
BAND = 256


def banded(torch, n, dtype, fill):
    t = torch.full((n + 2 * BAND,), -77, dtype=dtype, device="cuda")
    t[BAND:BAND + n] = fill
    return t, t[BAND:BAND + n]


def bands_intact(t):
    return bool((t[:BAND] == -77).all()) and bool((t[-BAND:] == -77).all())


def pool_sample(items):
    rng = np.random.default_rng(1)
    return np.unique(np.concatenate([[0, 1, 32767, 32768, 32769, items - 1], rng.integers(0, items, 18)]))


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_pool_past_2_31_elements(xs, torch_gpu, kind):
    """max pooling, fp32: 24 items against tests/pool_common.py (a layer of those items alone: items do not meet), among them the
    first, the last and the two on either side of element 2^31; destinations pre-filled with NaN and -1 hold neither afterwards"""
    torch, L = torch_gpu, xs.lib()
    d = pc.desc(**POOL_WIDE)
    h = pc.Handle(d)
    items, plane_in, plane_out = h.work(), 64 * 64 * 16, 32 * 32 * 16
    assert items * plane_in >= W31 and h.in_shape() == (items, 64, 64, 16) and h.out_shape() == (items, 32, 32, 16)
    need(torch, items * (plane_in + 2 * plane_out) * 4)
    handle, st = xs.pool_create(*[d[k] for k in pc.DESC_FIELDS])
    assert handle and 0 == st
    sel = pool_sample(items)
    dsel = torch.from_numpy(sel).cuda()
    small = pc.Handle(pc.desc(**dict(POOL_WIDE, N=1, C=16 * sel.size)))
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    if kind == "fwd":
        bx, x = banded(torch, items * plane_in, torch.float32, 0.0)
        x.normal_(generator=g)
        bo, out = banded(torch, items * plane_out, torch.float32, float("nan"))
        bm, mask = banded(torch, items * plane_out, torch.int32, pc.SENTINEL)
        bound = [xs.pool_bind_new(handle, t, v) for t, v in ((pc.REG_IN, x), (pc.REG_OUT, out), (pc.MASK, mask))]
        assert 0 == xs.pool_execute(handle, pc.FWD)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "pool_fwd_max_f32"
        hx = x.view(items, 64, 64, 16)[dsel].cpu().numpy()
        wout = np.full(small.out_shape(), np.nan, dtype=np.float32)
        wmask = np.full(small.mask_shape(), pc.SENTINEL, dtype=np.int32)
        pc.forward(small, hx, wout, wmask)
        assert out.view(items, -1)[dsel].cpu().numpy().tobytes() == wout.tobytes()
        assert mask.view(items, -1)[dsel].cpu().numpy().tobytes() == wmask.tobytes()
        assert none_is(torch, out, torch.isnan) and none_is(torch, mask, lambda t: t < 0)
        assert bands_intact(bx) and bands_intact(bo) and bands_intact(bm)
    else:
        bi, din = banded(torch, items * plane_in, torch.float32, float("nan"))
        bo, dout = banded(torch, items * plane_out, torch.float32, 0.0)
        dout.normal_(generator=g)
        bm, mask = banded(torch, items * plane_out, torch.int32, 0)
        # a mask FWD could have written: per output and lane one of the four elements of its window
        ho = torch.arange(32, device="cuda", dtype=torch.int32).view(1, 32, 1, 1)
        wo = torch.arange(32, device="cuda", dtype=torch.int32).view(1, 1, 32, 1)
        lane = torch.arange(16, device="cuda", dtype=torch.int32).view(1, 1, 1, 16)
        for i0 in range(0, items, 3000):  # (in parts: the temporaries stay small)
            part = mask.view(items, 32, 32, 16)[i0:i0 + 3000]
            pick = torch.randint(0, 4, part.shape, device="cuda", generator=g, dtype=torch.int32)
            part.copy_(((2 * ho + pick // 2) * 64 + 2 * wo + pick % 2) * 16 + lane)
        del pick, part
        bound = [xs.pool_bind_new(handle, t, v) for t, v in ((pc.GRAD_IN, din), (pc.GRAD_OUT, dout), (pc.MASK, mask))]
        assert 0 == xs.pool_execute(handle, pc.BWD)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "pool_bwd_max_f32"
        hd = dout.view(items, 32, 32, 16)[dsel].cpu().numpy()
        hm = mask.view(items, 32, 32, 16)[dsel].cpu().numpy()
        wdin = np.full(small.in_shape(), np.nan, dtype=np.float32)
        pc.backward(small, hd, hm, wdin)
        assert din.view(items, -1)[dsel].cpu().numpy().tobytes() == wdin.tobytes()
        assert none_is(torch, din, torch.isnan)
        assert bands_intact(bi) and bands_intact(bo) and bands_intact(bm)
    for t in bound:
        L.libxsmm_dnn_destroy_tensor(t)
    assert 0 == L.libxsmm_dnn_destroy_pooling(handle)


# ---- convolution: tensors one image (one block) short of 2^31 elements --------------------------------------------------------------
CONV_ACT = cc.desc(H=128, W=128, R=1, S=1, N=2047, C=64, K=1)      # the input: 2^31 elements less one image
CONV_FIL = cc.desc(H=1, W=1, R=1, S=1, N=1, C=46336, K=46336)      # the filter: 2896 * 2896 items of 16 x 16
POISON_BITS = -1  # conv_common.POISON as int32


def poisoned(torch, n):
    """n float32 elements of ones bits between bands: (whole tensor as int32, the elements as int32, the elements as float32)"""
    whole, inner = banded(torch, n, torch.int32, POISON_BITS)
    return whole, inner, inner.view(torch.float32)


def seeded(torch, n, seed):
    whole, inner = banded(torch, n, torch.float32, 0.0)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    inner.normal_(generator=g)
    return whole, inner


def bit_sum(torch, t):
    """the sum of the elements' bits, exact: what a tensor that must not be written is held against"""
    total = 0
    for s in range(0, t.numel(), SLAB):
        total += int(t[s:s + SLAB].view(torch.int32).sum(dtype=torch.int64))
    return total


def only_these_written(torch, dest_i32, per_item, items):
    """everything outside the given items (of per_item elements each) still holds ones bits"""
    lo = 0
    for i in sorted(items):
        if not all_equal(torch, dest_i32, POISON_BITS, lo, i * per_item):
            return False
        lo = (i + 1) * per_item
    return all_equal(torch, dest_i32, POISON_BITS, lo, dest_i32.numel())


def conv_layer(xs, d, bind):
    handle, st = xs.conv_create(*[d[k] for k in cc.DESC_FIELDS])
    assert handle and 0 == st
    scratch = np.zeros(64, dtype=np.uint8)  # (never read or written: host memory will do)
    assert 0 == xs.lib().libxsmm_dnn_bind_scratch(handle, cc.ALL, xs.dptr(scratch))
    return handle, [xs.conv_bind_new(handle, t, v) for t, v in bind], scratch


def conv_close(xs, handle, tensors):
    for t in tensors:
        xs.lib().libxsmm_dnn_destroy_tensor(t)
    assert 0 == xs.lib().libxsmm_dnn_destroy_conv_layer(handle)


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_conv_activations_below_2_31_elements(xs, torch_gpu, kind):
    """FWD reads and BWD writes an input of 2^31 - 2^20 elements: as many logical threads as items, and only the shares of three
    items run -- the first, the last (whose offsets end at 2^31 - 2^20 - 1, above 2^30) and one in the upper half. Each against
    tests/conv_common.py on a layer of those three images alone (C and the blocks kept: the chain order depends on them)."""
    torch = torch_gpu
    h = cc.Handle(CONV_ACT)
    n_in, n_out = int(np.prod(h.in_shape())), int(np.prod(h.out_shape()))
    plane_in = 128 * 128 * 16
    assert n_in == W31 - 64 * 128 * 128 == 2146435072 and n_out == 2047 * 128 * 128 and (h.ifmblock, h.blocksifm, h.ofmblock, h.blocksofm) == (16, 4, 1, 1)
    need(torch, (n_in + n_out) * 4)
    images = (0, 1024, 2046)
    small = cc.Handle(dict(CONV_ACT, N=len(images)))
    w = np.random.default_rng(5).standard_normal(h.fil_shape(), dtype=np.float32)
    dw = torch.from_numpy(w).cuda()
    dsel = torch.tensor(images, device="cuda")
    if kind == "fwd":
        d = dict(CONV_ACT, threads=h.work(cc.FWD))
        assert d["threads"] == 2047 and [cc.Handle(d).share(cc.FWD, i) for i in images] == [(i, i + 1) for i in images]
        bx, x = seeded(torch, n_in, 17)
        bo, out_bits, out = poisoned(torch, n_out)
        before = bit_sum(torch, x)
        handle, tensors, scratch = conv_layer(xs, d, ((cc.REG_IN, x), (cc.REG_FIL, dw), (cc.REG_OUT, out)))
        for i in reversed(images):
            assert 0 == xs.conv_execute(handle, cc.FWD, 0, i)
        torch.cuda.synchronize()
        assert xs.last_kernel().startswith("conv_fwd_t")
        hx = x.view(2047, -1)[dsel].cpu().numpy()
        want = cc.fwd(small, hx, w, np.full(small.out_shape(), cc.POISON, dtype=np.float32), None)
        got = out.view(2047, -1)[dsel].cpu().numpy()
        assert cc.same_bits(got, want), int(np.sum(cc.bits(got) != cc.bits(want)))
        assert only_these_written(torch, out_bits, 128 * 128, images)
        assert bit_sum(torch, x) == before and np.array_equal(dw.cpu().numpy(), w)
        assert bands_intact(bx) and bands_intact(bo)
    else:
        items = (0, 4 * 1500 + 1, 4 * 2047 - 1)  # (image, block): the first, one in the upper half, the last
        d = dict(CONV_ACT, threads=h.work(cc.BWD))
        assert d["threads"] == 8188 and [cc.Handle(d).share(cc.BWD, i) for i in items] == [(i, i + 1) for i in items]
        assert items[1] * plane_in > W31 // 2 and (items[2] + 1) * plane_in == n_in
        bi, din_bits, din = poisoned(torch, n_in)
        bo, dout = seeded(torch, n_out, 19)
        before = bit_sum(torch, dout)
        handle, tensors, scratch = conv_layer(xs, d, ((cc.GRAD_IN, din), (cc.REG_FIL, dw), (cc.GRAD_OUT, dout)))
        for i in reversed(items):
            assert 0 == xs.conv_execute(handle, cc.BWD, 0, i)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "conv_bwd"
        of_images = torch.tensor([i // 4 for i in items], device="cuda")
        hd = dout.view(2047, -1)[of_images].cpu().numpy()
        want = cc.bwd(small, hd, w, np.full(small.in_shape(), cc.POISON, dtype=np.float32))  # all four blocks of the three images
        got = din.view(2047 * 4, -1)[torch.tensor(items, device="cuda")].cpu().numpy()
        for n, i in enumerate(items):
            assert cc.same_bits(got[n], want[n, i % 4]), (i, int(np.sum(cc.bits(got[n]) != cc.bits(want[n, i % 4]))))
        assert only_these_written(torch, din_bits, plane_in, items)
        assert bit_sum(torch, dout) == before and np.array_equal(dw.cpu().numpy(), w)
        assert bands_intact(bi) and bands_intact(bo)
    assert np.all(scratch == 0)
    conv_close(xs, handle, tensors)


@pytest.mark.parametrize("part", ["upd", "trans"])
def test_conv_filter_below_2_31_elements(xs, torch_gpu, part):
    """a filter of 2896 * 2896 blocks of 16 x 16: 2^31 - 458752 elements. upd: the shares of the first item, the last (its offsets
    end above 2^30, at the last element) and one in the middle, each against tests/conv_common.py on a layer of one block on either
    side. trans: libxsmm_dnn_trans_reg_filter into a second tensor of that size, compared on the device with the permuted view of
    the source (1 x 1: nothing to flip), 256 rows of blocks at a time."""
    torch = torch_gpu
    h = cc.Handle(CONV_FIL)
    nb, total = 2896, int(np.prod(h.fil_shape()))
    assert total == 2147024896 < W31 and (h.ifmblock, h.ofmblock, h.blocksifm, h.blocksofm) == (16, 16, nb, nb) and h.work(cc.UPD) == nb * nb
    if part == "upd":
        need(torch, total * 4)
        items = (0, 1450 * nb + 77, nb * nb - 1)
        d = dict(CONV_FIL, threads=h.work(cc.UPD))
        assert [cc.Handle(d).share(cc.UPD, i) for i in items] == [(i, i + 1) for i in items] and (items[2] + 1) * 256 == total
        rng = np.random.default_rng(23)
        x, dout = rng.standard_normal(h.in_shape(), dtype=np.float32), rng.standard_normal(h.out_shape(), dtype=np.float32)
        dx, ddout = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
        bw, dw_bits, dw = poisoned(torch, total)
        handle, tensors, scratch = conv_layer(xs, d, ((cc.REG_IN, dx), (cc.GRAD_OUT, ddout), (cc.GRAD_FIL, dw)))
        for i in reversed(items):
            assert 0 == xs.conv_execute(handle, cc.UPD, 0, i)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "conv_upd_gemm"
        got = dw.view(nb * nb, 256)[torch.tensor(items, device="cuda")].cpu().numpy()
        small = cc.Handle(dict(CONV_FIL, C=16, K=16))
        for n, i in enumerate(items):
            ofm1, ifm1 = divmod(i, nb)
            want = cc.upd(small, x[:, ifm1:ifm1 + 1], dout[:, ofm1:ofm1 + 1], np.full(small.fil_shape(), cc.POISON, dtype=np.float32))
            assert cc.same_bits(got[n], want), i
        assert only_these_written(torch, dw_bits, 256, items) and bands_intact(bw)
        assert np.array_equal(dx.cpu().numpy(), x) and np.array_equal(ddout.cpu().numpy(), dout)
    else:
        if torch.cuda.mem_get_info()[0] < 2 * total * 4 + GiB:
            pytest.skip("the transposition needs a second tensor of 8 GiB: %.1f GiB free, it needs %.1f" % (torch.cuda.mem_get_info()[0] / GiB, 2 * total * 4 / GiB + 1))
        need(torch, 2 * total * 4)
        bw, w = seeded(torch, total, 29)
        bt, wtr_bits, wtr = poisoned(torch, total)
        before = bit_sum(torch, w)
        handle, tensors, scratch = conv_layer(xs, CONV_FIL, ((cc.REG_FIL, w), (cc.REG_FIL_TR, wtr)))
        assert 0 == xs.lib().libxsmm_dnn_trans_reg_filter(handle)
        torch.cuda.synchronize()
        assert xs.last_kernel() == "conv_trans_filter"
        src, dst = w.view(nb, nb, 16, 16), wtr.view(nb, nb, 16, 16)  # [ofm1][ifm1][ifm2][ofm2] -> [ifm1][ofm1][ofm2][ifm2]
        for i0 in range(0, nb, 256):
            assert bool((dst[i0:i0 + 256] == src[:, i0:i0 + 256].permute(1, 0, 3, 2)).all()), i0
        assert bit_sum(torch, w) == before and bands_intact(bw) and bands_intact(bt)
    assert np.all(scratch == 0)
    conv_close(xs, handle, tensors)


# ---- RNN cell: hidden state, internal state and previous state just below 2^31 elements ------------------------------------------------
def periods_that_differ(torch, bits, want, steps, reps):
    """bits: [steps][reps][period] as int32, want: [steps][1][period]; the indices of the periods that are not want, slab by slab"""
    v, bad = bits.view(steps, reps, -1), []
    step = max(1, SLAB // (steps * v.shape[2]))
    for r0 in range(0, reps, step):
        ok = (v[:, r0:r0 + step] == want).all(dim=2).all(dim=0)
        bad += (r0 + torch.nonzero(~ok).view(-1)).tolist()
    return bad


def test_rnn_state_below_2_31_elements(xs, torch_gpu):
    """A ReLU cell with two steps, C = 8, K = 72 and as many rows as max_T * N * K < 2^31 allows in whole periods of 1240: step 1 of h,
    of z and of the chains the launch of bias + w.x leaves begins 242176 bytes below byte 2^32 (more the layer does not accept: it
    refuses 2^31 elements) and ends near byte 2^33. Four logical threads, all run, in reverse order: every share stays below the
    row-tile limit. x and hp repeat one seeded block of 1240 rows; every period of h and z is compared with the restatement of that
    block as uint32, the last one, the ones across the share boundaries and the one that holds byte 2^32 by name."""
    torch, L = torch_gpu, xs.lib()
    d = rc.WIDE_CASE
    N, Cc, K, T, P = d["N"], d["C"], d["K"], d["max_T"], rc.WIDE_PERIOD
    reps, n_state, n_x = N // P, T * N * K, T * N * Cc
    assert W31 - (1 << 20) <= n_state < W31 and reps * P == N and (1 << 32) - (1 << 20) < N * K * 4 < 1 << 32 and n_state * 4 > (1 << 33) - (1 << 22)
    need(torch, (3 * n_state + n_x) * 4 + GiB, most=27 * GiB)
    t0 = time.time()
    dp, tp, op = rc.wide_period()
    handle, st = xs.rnn_create(N, Cc, K, T, d["cell"], d["bn"], d["bc"], d["bk"], d["threads"])
    shares = rc.Handle(d).shares()
    assert handle and 0 == st and len(shares) == 4 and all(n1 - n0 <= ll.threshold("rnn_rows_per_share") for n0, n1 in shares)
    on_device = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()  # noqa: E731
    want = {key: on_device(a).view(T, 1, -1) for key, a in (("x", tp["x"]), ("hp", tp["hp"]), ("h", op["h"]), ("z", op["z"]))}
    bx, x = banded(torch, n_x, torch.float32, 0.0)
    bhp, hp = banded(torch, n_state, torch.float32, 0.0)
    x.view(torch.int32).view(T, reps, -1).copy_(want["x"])
    hp.view(torch.int32).view(T, reps, -1).copy_(want["hp"])
    bh, h_bits, h = poisoned(torch, n_state)
    bz, z_bits, z = poisoned(torch, n_state)
    assert z.data_ptr() % 64 == 0
    small = {key: torch.from_numpy(tp[key]).cuda() for key in ("w", "r", "b")}
    tensors = [xs.rnn_bind_new(handle, rc.IN_TYPE.get(key, rc.OUT_TYPE.get(key)), v)
               for key, v in (("x", x), ("hp", hp), ("w", small["w"]), ("r", small["r"]), ("b", small["b"]), ("h", h))]
    assert 0 == L.libxsmm_dnn_rnncell_bind_internalstate(handle, rc.FWD, xs.dptr(z))
    before = L.libxsmm_amd_launch_count()
    torch.cuda.synchronize()
    t1 = time.time()
    for tid in (3, 2, 1, 0):
        assert 0 == xs.rnn_execute(handle, rc.FWD, 0, tid), tid
    torch.cuda.synchronize()
    t2 = time.time()
    assert xs.last_kernel() == "rnn_g1" and 4 * (T + 1) == L.libxsmm_amd_launch_count() - before
    named = {"the last period": reps - 1, "the period of step 1 that holds byte 2^32": ((1 << 30) - N * K) // K // P}
    named.update({"the period across the boundary of shares %d and %d (row %d)" % (i, i + 1, shares[i][1]): shares[i][1] // P for i in range(3)})
    assert all(0 <= p < reps for p in named.values()) and all(shares[i][1] % P for i in range(3))
    for key, bits in (("h", h_bits), ("z", z_bits)):
        for what, p in named.items():
            assert bool((bits.view(T, reps, -1)[:, p] == want[key][:, 0]).all()), "%s: %s (period %d of %d) differs" % (key, what, p, reps)
        bad = periods_that_differ(torch, bits, want[key], T, reps)
        assert not bad, "%s: %d of %d periods differ, the first ones %r (named: %r)" % (key, len(bad), reps, bad[:8], named)
    for key, v in (("x", x), ("hp", hp)):  # what the pass reads
        assert not periods_that_differ(torch, v.view(torch.int32), want[key], T, reps), key
    assert all(np.array_equal(small[key].cpu().numpy().view(np.uint32), tp[key].view(np.uint32)) for key in small)
    assert bands_intact(bx) and bands_intact(bhp) and bands_intact(bh) and bands_intact(bz)
    for tensor in tensors:
        L.libxsmm_dnn_destroy_tensor(tensor)
    assert 0 == L.libxsmm_dnn_destroy_rnncell(handle)
    print("rnn wide: fill %.2f s, four shares %.2f s, compare %.2f s" % (t1 - t0, t2 - t1, time.time() - t2))


# ---- packed kernels: a pack of 2^21 elements, a thousand packs -----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("name,kind,dtype,m,n,k,wide,npacks,kw", pk.WIDE_CASES, ids=[c[0] for c in pk.WIDE_CASES])
def test_packed_operand_past_2_31_elements(xs, orc, torch_gpu, monkeypatch, name, kind, dtype, m, n, k, wide, npacks, kw, form):
    """one operand with ld = 4096, column major, 32 columns: its packs lie 2^21 (fp64: 2^20) elements apart, the last one starts past
    element 2^31 and byte 2^33 (fp64: byte 2^32) -- p * (long long)LD * (NL * VLEN) in the kernel text, once per operand slot and form. The
    other operands are tight. All valid elements of all packs, gathered through the index tensor that scattered them, against the oracle
    on tight copies of the same matrices, bit for bit; the padding between the extent of a column and ld keeps the canary everywhere."""
    torch, L = torch_gpu, xs.lib()
    v, ts = pk.width(dtype), np.dtype(dtype).itemsize
    tight = pk.Case(kind, dtype, m, n, k, nmat=npacks * v, seed=41, **kw)
    rows, cols = tight.ops[wide].shape[1:]
    ld, nl, guard = pk.WIDE_LD, pk.WIDE_LINES, pk.GUARD
    assert cols == nl and tight.layout == pk.COL and tight.ld[wide] == rows
    ps = ld * nl * v
    assert (npacks - 1) * ps * ts >= 1 << 32 and (ts == 8 or ((npacks - 1) * ps >= W31 and (npacks - 1) * ps * ts >= 1 << 33))
    need(torch, (npacks * ps + 2 * guard) * ts)
    want = tight.chain(xs, orc)  # the oracle on the tight layout: the leading dimension only places the columns
    host = tight.buffers(xs)
    body = lambda buf: buf[guard:-guard]
    # where element (i, j) of matrix lane of pack p lies in the wide operand, in the order of the tight packed buffer [p][j][i][lane]
    p_, j_, i_, l_ = np.meshgrid(np.arange(npacks, dtype=np.int64), np.arange(nl, dtype=np.int64), np.arange(rows, dtype=np.int64),
                                 np.arange(v, dtype=np.int64), indexing="ij")
    index = (guard + ((p_ * nl + j_) * ld + i_) * v + l_).reshape(-1)
    assert index.size == body(host[wide]).size and index[-1] == guard + (npacks - 1) * ps + ((nl - 1) * ld + rows) * v - 1 and int(index.max()) * ts >= 1 << 32
    dindex = torch.from_numpy(index).cuda()
    tt = torch.float32 if ts == 4 else torch.float64
    dwide = torch.full((npacks * ps + 2 * guard,), CANARY, dtype=tt, device="cuda")
    assert dwide.data_ptr() % 16 == 0
    dwide[dindex] = torch.from_numpy(body(host[wide])).cuda()
    dev = {nm: torch.from_numpy(x).cuda() for nm, x in host.items() if nm != wide}
    ptr = {nm: t.data_ptr() + guard * ts for nm, t in dev.items()}
    ptr[wide] = dwide.data_ptr() + guard * ts
    a, b, c = (ptr["a"], ptr["b"], ptr["c"]) if kind == pk.PGEMM else ((ptr["a"], ptr["a"], None) if kind == pk.GETRF else (ptr["a"], ptr["b"], None))
    case = pk.Case(kind, dtype, m, n, k, nmat=v, seed=41, **kw)  # (the descriptor: one pack will do)
    case.ld[wide] = ld
    fn = case.dispatch(xs)
    monkeypatch.setenv("LIBXSMM_AMD_PACKED_FORM", form)
    torch.cuda.synchronize()
    assert 0 == L.libxsmm_amd_packed_execute_batch(fn, a, b, c, npacks)
    assert 0 == L.libxsmm_amd_synchronize()
    assert xs.last_kernel().endswith("_lds" if form == "1" else "_direct"), xs.last_kernel()
    bits = np.uint32 if ts == 4 else np.uint64
    got = {nm: t.cpu().numpy() for nm, t in dev.items()}
    got_wide = dwide[dindex].cpu().numpy()
    diff = np.flatnonzero(got_wide.view(bits) != body(want[wide]).view(bits))
    assert diff.size == 0, (diff.size, "first in pack %d" % (int(diff[0]) // (nl * rows * v)))
    for nm in got:  # the tight operands, canaries included
        assert np.array_equal(got[nm].view(bits), want[nm].view(bits)), nm
    per = nl * rows * v if tight.written == wide else tight.pack_elems(tight.written)
    out, was = (got_wide, body(host[wide])) if tight.written == wide else (body(got[tight.written]), body(host[tight.written]))
    assert np.any(out[:per].view(bits) != was[:per].view(bits)) and np.any(out[-per:].view(bits) != was[-per:].view(bits))  # first and last pack written
    # the canaries of the wide operand: both guards, and of every column what lies between its extent and ld
    assert all_equal(torch, dwide, CANARY, 0, guard) and all_equal(torch, dwide, CANARY, guard + (npacks * nl - 1) * ld * v + rows * v, dwide.numel())
    columns = dwide[guard:guard + npacks * ps].view(npacks * nl, ld * v)
    step = max(1, SLAB // (ld * v))
    for r0 in range(0, npacks * nl, step):
        assert bool((columns[r0:r0 + step, rows * v:] == CANARY).all()), r0
