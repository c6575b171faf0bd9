"""Quantisation and bf16 conversion on the GPU (include/libxsmm_dnn.h): every result is compared bit for bit (np.array_equal,
scf byte included) with tests/quant_common.py, the numpy restatement that tests/test_quant_cpu.py holds against the
reference's own outputs.

Reference: src/libxsmm_dnn.c:2394-2907; the flow of samples/deeplearning/cnnlayer/layer_example_qi16f32.c:509-525."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quant_common as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1023, 4099, 262147)  # the last one spans many work-groups: the maximum crosses them
GUARD16, GUARD32 = 0x7b7b, 0x7b7b7b7b


def flat_input(n, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.random(n) - 0.5) * 1.9).astype(np.float32)
    x[rng.random(n) < 0.03] = 0.0
    return x


class Buffers:
    """device in / out with guard elements around them; in_off / out_off: elements from a 16-byte boundary"""
    def __init__(self, torch, x, in_off, out_off, out_dtype=None, in_dtype=None):
        n = x.size
        self.n, self.o0 = n, 16 + out_off
        self.guard = GUARD32 if out_dtype is torch.int32 else GUARD16
        self.din = torch.zeros(n + 32, dtype=in_dtype or torch.float32, device="cuda")
        assert self.din.data_ptr() % 16 == 0
        self.din[in_off:in_off + n] = torch.from_numpy(x).cuda()
        self.vin = self.din[in_off:in_off + n]
        self.dout = torch.full((n + 48,), self.guard, dtype=out_dtype or torch.int16, device="cuda")
        assert self.dout.data_ptr() % 16 == 0
        self.vout = self.dout[self.o0:self.o0 + n]

    def result(self):
        out = self.dout.cpu().numpy()
        assert (out[:self.o0] == self.guard).all() and (out[self.o0 + self.n:] == self.guard).all(), "guard elements were overwritten"
        return out[self.o0:self.o0 + self.n]


def check_flat(xs, torch, x, shift, mode, in_off=0, out_off=0, note=""):
    b = Buffers(torch, x, in_off, out_off)
    scf = xs.dnn_quantize(b.vin, b.vout, x.size, shift, mode)
    gq, gscf = qc.quantize(x, shift, mode)
    assert scf == gscf, (note, x.size, shift, mode, in_off, out_off, scf, gscf)
    got = b.result()
    assert np.array_equal(got, gq), (note, x.size, shift, mode, in_off, out_off, int(np.argmax(got != gq)))
    return got, scf


@pytest.mark.parametrize("mode", qc.DETERMINISTIC)
def test_flat_lengths_and_alignments(xs, torch_gpu, mode):
    for n in LENGTHS:
        x = flat_input(n, n)
        for shift in (0, 2):
            for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 1)) if n < 5000 else ((0, 0), (1, 1)):
                check_flat(xs, torch_gpu, x, shift, mode, in_off, out_off)
    assert xs.last_kernel() == "quant_flat"


@pytest.mark.parametrize("mode", qc.DETERMINISTIC)
def test_flat_where_the_maximum_sits_and_how_large_it_is(xs, torch_gpu, mode):
    n = 4099
    for in_off in (0, 1):  # in_off 1: a scalar head of three elements; 4099 - 3 leaves no tail, 4099 - 0 a tail of three
        for pos, sign in ((0, 1), (n - 1, 1), (1, -1), (n - 2, -1), (n // 2, -1)):
            for mag in (2.0 ** -20, 1.0, 2.0 ** 20):
                x = (flat_input(n, pos + 7) * np.float32(mag * 0.5)).astype(np.float32)
                x[pos] = np.float32(sign * mag * 1.25)
                check_flat(xs, torch_gpu, x, 2, mode, in_off, in_off, note="max at %d" % pos)


@pytest.mark.parametrize("mode", qc.DETERMINISTIC)
def test_flat_special_values(xs, torch_gpu, mode):
    for shift in (0, 2):
        for n in (1, 7, 300):
            got, scf = check_flat(xs, torch_gpu, np.zeros(n, dtype=np.float32), shift, mode, note="zeros")
            assert not got.any() and scf == (15 if mode == qc.FPHW_ROUND else 141) - shift
    # ties after scaling: with a maximum of 4096 and add_shift 2 the FPHW scale is 1
    ties = np.array([4096.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3.0], dtype=np.float32)
    got, scf = check_flat(xs, torch_gpu, ties, 2, mode, note="ties")
    if mode == qc.FPHW_ROUND:
        assert scf == 0 and list(got[:9]) == [4096, 1, -1, 2, -2, 3, -3, 0, 0]
    check_flat(xs, torch_gpu, ties, 0, mode, 1, 1, note="ties")
    den = np.array([1e-40, -3e-39, 0.0, 1.4e-45, -0.0, 5.9e-39], dtype=np.float32)  # a denormal maximum: frexpf on the device
    check_flat(xs, torch_gpu, den, 2, mode, note="denormals")
    check_flat(xs, torch_gpu, np.array([1.0, -0.3, 0.0], dtype=np.float32), 2 if mode == qc.FPHW_ROUND else 0, mode, note="known answers")


def test_known_answers(xs, torch_gpu):
    x = np.array([1.0, -0.3, 0.0], dtype=np.float32)
    got, scf = check_flat(xs, torch_gpu, x, 2, qc.FPHW_ROUND)
    assert list(got) == [4096, -1229, 0] and scf == 12
    for mode in (qc.NO_ROUND, qc.BIAS_ROUND, qc.NEAREST_ROUND):
        got, scf = check_flat(xs, torch_gpu, x, 0, mode)
        assert list(got) == [16384, -4915, 0] and scf == 14


def test_flat_golden_captures(xs, torch_gpu):
    """the reference's own outputs, straight against the device"""
    g = qc.load_golden("quant_flat.npz")
    for name, mode in (("no", qc.NO_ROUND), ("bias", qc.BIAS_ROUND), ("nearest", qc.NEAREST_ROUND), ("fphw", qc.FPHW_ROUND)):
        for n in qc.FLAT_GOLDEN_LENGTHS:
            for shift in (0, 2):
                got, scf = check_flat(xs, torch_gpu, g["in_%d" % n], shift, mode)
                assert scf == int(g["scf_%s_%d_%d" % (name, shift, n)]) and np.array_equal(got, g["out_%s_%d_%d" % (name, shift, n)])


def test_dequantize(xs, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(5)
    for n in LENGTHS:
        q = rng.integers(-32768, 32768, n).astype(np.int16)
        for scf in qc.DEQUANT_SCF if n < 5000 else (12,):
            for in_off, out_off in ((0, 0), (1, 1), (1, 0)):
                b = Buffers(torch, q, in_off, out_off, out_dtype=torch.int32, in_dtype=torch.int16)
                xs.dnn_dequantize(b.vin, b.vout, n, scf)
                assert np.array_equal(b.result().view(np.uint32), qc.dequantize(q, scf).view(np.uint32)), (n, scf, in_off, out_off)
    assert xs.last_kernel() == "dequant_flat"
    g = qc.load_golden("quant_misc.npz")
    for scf in qc.DEQUANT_SCF:
        b = Buffers(torch, g["deq_in"], 0, 0, out_dtype=torch.int32, in_dtype=torch.int16)
        xs.dnn_dequantize(b.vin, b.vout, g["deq_in"].size, scf)
        assert np.array_equal(b.result().view(np.uint32), g["deq_%d" % scf])


def test_async_forms_leave_scf_on_the_device(xs, torch_gpu):
    """the scf byte lands in device memory and a consumer queued behind the call sees it without a host wait in between"""
    torch = torch_gpu
    x = flat_input(262147, 11) * np.float32(37.0)
    dx = torch.from_numpy(x).cuda()
    dq = torch.zeros(x.size, dtype=torch.int16, device="cuda")
    dscf = torch.full((4,), 0xa5, dtype=torch.uint8, device="cuda")
    seen = torch.zeros(4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert 0 == xs.dnn_quantize(dx, dq, x.size, 2, qc.FPHW_ROUND, scf=dscf[1:])
    seen.copy_(dscf)  # the stream-ordered consumer (the library's default stream is the one torch queues on)
    torch.cuda.synchronize()
    gq, gscf = qc.quantize(x, 2, qc.FPHW_ROUND)
    assert list(seen.cpu().numpy()) == [0xa5, gscf, 0xa5, 0xa5] and np.array_equal(dq.cpu().numpy(), gq)
    case = qc.ACT_CASES[0]
    xa = flat_input(int(np.prod(case[:4])), 12)
    da, dqa = torch.from_numpy(xa).cuda(), torch.zeros(xa.size, dtype=torch.int16, device="cuda")
    assert 0 == xs.dnn_quantize_act(da, dqa, *case, 0, qc.NEAREST_ROUND, scf=dscf[2:])
    cf = qc.FIL_CASES[2]
    xf = flat_input(int(np.prod(cf[:4])), 13)
    df, dqf = torch.from_numpy(xf).cuda(), torch.zeros(xf.size, dtype=torch.int16, device="cuda")
    assert 0 == xs.dnn_quantize_fil(df, dqf, *cf, 0, qc.BIAS_ROUND, scf=dscf[3:])
    torch.cuda.synchronize()
    ga, sa = qc.quantize_act(xa, case, 0, qc.NEAREST_ROUND)
    gf, sf = qc.quantize_fil(xf, cf, 0, qc.BIAS_ROUND)
    assert list(dscf.cpu().numpy()) == [0xa5, gscf, sa, sf]
    assert np.array_equal(dqa.cpu().numpy(), ga) and np.array_equal(dqf.cpu().numpy(), gf)
    host_byte = np.zeros(1, dtype=np.uint8)  # a byte the GPU does not reach is refused
    assert 0 != xs.dnn_quantize(dx, dq, 8, 2, qc.FPHW_ROUND, scf=host_byte)


@pytest.mark.parametrize("case", qc.ACT_CASES)
def test_act_layouts(xs, torch_gpu, case, monkeypatch):
    torch = torch_gpu
    n = int(np.prod(case[:4]))
    g = qc.load_golden("quant_act.npz")
    ci = qc.ACT_CASES.index(case)
    x = g["in_%d" % ci]
    dx = torch.from_numpy(x).cuda()
    names = {mode: name for name, mode in qc.GOLDEN_MODES.items()}
    expect = "quant_flat" if case[4] == case[5] * case[6] else ("quant_act_tiled" if case[4] == 1 else "quant_act")
    for mode in qc.DETERMINISTIC:
        for shift in (0, 2):
            gq, gscf = qc.quantize_act(x, case, shift, mode)
            rq, rscf = qc.golden_layout(g, names[mode], shift, ci)  # the reference's own output
            assert gscf == rscf and np.array_equal(gq, rq)
            outs = []
            for tiled in ("1", "0"):
                monkeypatch.setenv("LIBXSMM_AMD_QUANT_TILED", tiled)
                dq = torch.full((n + 16,), GUARD16, dtype=torch.int16, device="cuda")
                scf = xs.dnn_quantize_act(dx, dq[8:8 + n], *case, shift, mode)
                assert xs.last_kernel() == (expect if tiled == "1" or expect != "quant_act_tiled" else "quant_act")
                out = dq.cpu().numpy()
                assert (out[:8] == GUARD16).all() and (out[8 + n:] == GUARD16).all()
                assert scf == gscf and np.array_equal(out[8:8 + n], gq), (case, mode, shift, tiled)
                outs.append(out)
            assert np.array_equal(outs[0], outs[1])
    monkeypatch.setenv("LIBXSMM_AMD_QUANT_TILED", "1")
    dq = torch.zeros(n + 1, dtype=torch.int16, device="cuda")  # out only 2-byte aligned: element by element
    scf = xs.dnn_quantize_act(dx, dq[1:], *case, 2, qc.FPHW_ROUND)
    gq, gscf = qc.quantize_act(x, case, 2, qc.FPHW_ROUND)
    assert xs.last_kernel() == ("quant_flat" if expect == "quant_flat" else "quant_act")
    assert scf == gscf and np.array_equal(dq[1:].cpu().numpy(), gq)


@pytest.mark.parametrize("case", qc.FIL_CASES)
def test_fil_layouts(xs, torch_gpu, case):
    torch = torch_gpu
    n = int(np.prod(case[:4]))
    g = qc.load_golden("quant_fil.npz")
    ci = qc.FIL_CASES.index(case)
    x = g["in_%d" % ci]
    dx = torch.from_numpy(x).cuda()
    names = {mode: name for name, mode in qc.GOLDEN_MODES.items()}
    for mode in qc.DETERMINISTIC:
        for shift in (0, 2):
            rq, rscf = qc.golden_layout(g, names[mode], shift, ci)  # the reference's own output
            for off in (0, 1):
                dq = torch.full((n + 16,), GUARD16, dtype=torch.int16, device="cuda")
                scf = xs.dnn_quantize_fil(dx, dq[8 + off:8 + off + n], *case, shift, mode)
                gq, gscf = qc.quantize_fil(x, case, shift, mode)
                out = dq.cpu().numpy()
                assert (out[:8 + off] == GUARD16).all() and (out[8 + off + n:] == GUARD16).all()
                assert scf == gscf == rscf and np.array_equal(out[8 + off:8 + off + n], gq) and np.array_equal(gq, rq), (case, mode, shift, off)
    assert xs.last_kernel() == "quant_fil"


def test_converters(xs, torch_gpu):
    torch = torch_gpu
    g = qc.load_golden("quant_misc.npz")
    rng = np.random.default_rng(17)
    u = np.concatenate([qc.BF16_SPECIALS, rng.integers(0, 2 ** 32, 4099, dtype=np.uint64).astype(np.uint32)])
    x = qc.from_bits(u)
    n = x.size
    for rounding, gold_fn in (("truncate", qc.bf16_truncate), ("rnaz", qc.bf16_rnaz), ("rne", qc.bf16_rne)):
        gold = gold_fn(x)
        assert np.array_equal(gold[:qc.BF16_SPECIALS.size], g[rounding])
        for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 3)):
            b = Buffers(torch, u.view(np.int32), in_off, out_off, in_dtype=torch.int32)
            xs.convert_f32_bf16(b.vin, b.vout, n, rounding)
            assert np.array_equal(b.result().view(np.uint16), gold), (rounding, in_off, out_off)
        assert xs.last_kernel() == "bf16_" + rounding
    finite = np.isfinite(x)
    t = torch.from_numpy(x[finite].copy()).cuda().to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(qc.bf16_rne(x)[finite], t)  # torch's own fp32 -> bf16 on the finite subset
    h = rng.integers(0, 2 ** 16, 4099, dtype=np.uint64).astype(np.uint16)
    for in_off, out_off in ((0, 0), (1, 1)):
        b = Buffers(torch, h.view(np.int16), in_off, out_off, out_dtype=torch.int32, in_dtype=torch.int16)
        xs.convert_bf16_f32(b.vin, b.vout, h.size)
        assert np.array_equal(b.result().view(np.uint32), qc.bf16_widen(h).view(np.uint32))


def test_stochastic_rounding(xs, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(23)
    n = 20000
    x = ((rng.random(n) - 0.5) * 2).astype(np.float32)
    x[0] = 1.0  # max_exp 127, add_shift 0: rhs = 9 + exp_off, the quantum of the maximum's binade is 2^-14
    # 4096 elements whose discarded part is at most 2^-24 = 2^-9 * 2^-15 (|q| < 0.01): multiples of the quantum in [0.5, 1),
    # half of them one ulp above
    lo = np.float32(0.5) + rng.integers(0, 2 ** 13, 4096).astype(np.float32) * np.float32(2.0 ** -14) + rng.integers(0, 2, 4096).astype(np.float32) * np.float32(2.0 ** -24)
    x[1:4097] = lo.astype(np.float32)
    base, scf0 = qc.quantize(x, 0, qc.NO_ROUND)
    _, q = qc.no_scf_parts(x, 127, 0, qc.STOCH_ROUND)
    assert (np.abs(q[1:4097]) < 0.01).all() and (q > 0.5).any() and (q < -0.5).any()
    dx = torch.from_numpy(x).cuda()

    def run(seed):
        xs.dnn_quantize_set_seed(seed)
        dq = torch.zeros(n, dtype=torch.int16, device="cuda")
        scf = xs.dnn_quantize(dx, dq, n, 0, qc.STOCH_ROUND)
        assert scf == scf0
        return dq.cpu().numpy()
    try:
        a, a2, b = run(1234), run(1234), run(99)
        free = run(0)  # a seed per call: still the base or the base plus one
    finally:
        xs.dnn_quantize_set_seed(0)
    assert np.array_equal(a, a2) and not np.array_equal(a, b)
    for out in (a, b, free):
        inc = (out.view(np.uint16).astype(np.int64) - base.view(np.uint16).astype(np.int64)) & 0xffff
        assert np.isin(inc, (0, 1)).all()
        nz = x != 0
        assert (inc[(q > 0.5) & nz] == 1).all() and (inc[(q < -0.5) & nz] == 0).all()
        share = inc[1:4097].mean()
        assert 0.4 <= share <= 0.6, share  # a fair coin over 4096 draws: sigma 0.0078


def test_memory_kinds(xs, torch_gpu):
    torch = torch_gpu
    L = xs.lib()
    n = 4099
    x = flat_input(n, 31)
    gq, gscf = qc.quantize(x, 2, qc.FPHW_ROUND)
    # pageable numpy memory, misaligned on both sides
    hin, hout = np.zeros(n + 4, dtype=np.float32), np.full(n + 8, GUARD16, dtype=np.int16)
    hin[1:n + 1] = x
    assert xs.dnn_quantize(hin[1:], hout[3:], n, 2, qc.FPHW_ROUND) == gscf
    assert np.array_equal(hout[3:3 + n], gq) and (hout[:3] == GUARD16).all() and (hout[3 + n:] == GUARD16).all()
    hb = np.zeros(n, dtype=np.uint16)
    xs.convert_f32_bf16(x, hb, n, "rne")
    assert np.array_equal(hb, qc.bf16_rne(x))
    hf = np.zeros(n, dtype=np.float32)
    xs.dnn_dequantize(gq, hf, n, gscf)
    assert np.array_equal(hf.view(np.uint32), qc.dequantize(gq, gscf).view(np.uint32))
    # pinned memory of libxsmm_malloc: in place, complete on return
    pin, pout = L.libxsmm_malloc(x.nbytes), L.libxsmm_malloc(2 * n)
    assert pin and pout
    try:
        C.memmove(pin, x.ctypes.data, x.nbytes)
        C.memset(pout, 0, 2 * n)
        assert xs.dnn_quantize(pin, pout, n, 2, qc.FPHW_ROUND) == gscf
        assert np.array_equal(np.frombuffer((C.c_char * (2 * n)).from_address(pout), dtype=np.int16), gq)
        C.memset(pout, 0, 2 * n)
        dscf = torch.zeros(1, dtype=torch.uint8, device="cuda")
        assert 0 == xs.dnn_quantize(pin, pout, n, 2, qc.FPHW_ROUND, scf=dscf)  # host-visible out: complete on return
        assert np.array_equal(np.frombuffer((C.c_char * (2 * n)).from_address(pout), dtype=np.int16), gq)
    finally:
        L.libxsmm_free(pin); L.libxsmm_free(pout)
    # device memory
    dx, dq = torch.from_numpy(x).cuda(), torch.zeros(n, dtype=torch.int16, device="cuda")
    assert xs.dnn_quantize(dx, dq, n, 2, qc.FPHW_ROUND) == gscf and np.array_equal(dq.cpu().numpy(), gq)


def test_call_order_inside_the_defer_bracket(xs, orc, torch_gpu):
    """dispatched kernel writes X -> quantise X -> dispatched kernel updates X again: inside libxsmm_amd_defer_begin/end the
    quantise call seals the open burst, so it sees the X of the first call and not that of the third"""
    torch = torch_gpu
    L = xs.lib()
    m = 32
    rng = np.random.default_rng(3)
    p, q, x = (rng.uniform(-1, 1, m * m).astype(np.float32) for _ in range(3))
    fn = L.libxsmm_smmdispatch(m, m, m, None, None, None, None, None, None, None)
    assert fn
    dp, dq_, dx = (torch.from_numpy(v.copy()).cuda() for v in (p, q, x))
    xs.call_kernel(fn, dp, dq_, dx)                    # X += P * Q
    torch.cuda.synchronize()
    x1 = dx.cpu().numpy()
    gx = x.copy()
    orc.smm(orc.FMA, 0, m, m, m, m, m, m, p, q, gx)
    assert np.allclose(x1, gx, rtol=1e-5, atol=1e-5) and not np.array_equal(x1, x)
    gq, gscf = qc.quantize(x1, 2, qc.FPHW_ROUND)
    xs.call_kernel(fn, dq_, dp, dx)                    # X += Q * P
    torch.cuda.synchronize()
    x2 = dx.cpu().numpy()
    assert not np.array_equal(qc.quantize(x2, 2, qc.FPHW_ROUND)[0], gq)
    for bracket in (False, True):
        dx = torch.from_numpy(x.copy()).cuda()
        out = torch.zeros(m * m, dtype=torch.int16, device="cuda")
        dscf = torch.zeros(1, dtype=torch.uint8, device="cuda")
        if bracket:
            xs.defer_begin()
        xs.call_kernel(fn, dp, dq_, dx)
        assert 0 == xs.dnn_quantize(dx, out, m * m, 2, qc.FPHW_ROUND, scf=dscf)
        xs.call_kernel(fn, dq_, dp, dx)
        if bracket:
            xs.defer_end()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), gq) and int(dscf.cpu()[0]) == gscf, bracket
        assert np.array_equal(dx.cpu().numpy(), x2), bracket


def test_chain_quantise_multiply_dequantise(xs, torch_gpu):
    """fp32 A (70 x 40), B (40 x 50) -> FPHW int16 -> libxsmm_amd_lowp_gemm I16 -> I32: exactly the integer product of the
    restated operands; scaled back it lies within half a quantum per operand of the fp64 product"""
    torch = torch_gpu
    m, k, n = 70, 40, 50
    rng = np.random.default_rng(41)
    a, b = rng.uniform(-1, 1, m * k).astype(np.float32), rng.uniform(-1, 1, k * n).astype(np.float32)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    qa, qb = torch.zeros(m * k, dtype=torch.int16, device="cuda"), torch.zeros(k * n, dtype=torch.int16, device="cuda")
    dscf = torch.zeros(2, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(m * n, dtype=torch.int32, device="cuda")
    assert 0 == xs.dnn_quantize(da, qa, m * k, 2, qc.FPHW_ROUND, scf=dscf[0:])
    assert 0 == xs.dnn_quantize(db, qb, k * n, 2, qc.FPHW_ROUND, scf=dscf[1:])
    assert 0 == xs.gemm_lowp(xs.I16, xs.I32, "N", "N", m, n, k, qa, m, qb, k, 0, dc, m)
    torch.cuda.synchronize()
    (ga, sa), (gb, sb) = qc.quantize(a, 2, qc.FPHW_ROUND), qc.quantize(b, 2, qc.FPHW_ROUND)
    assert list(dscf.cpu().numpy()) == [sa, sb]
    A, B = ga.astype(np.int64).reshape(k, m).T, gb.astype(np.int64).reshape(n, k).T  # column-major
    got = dc.cpu().numpy().astype(np.int64).reshape(n, m).T
    assert np.array_equal(got, A @ B)
    exact = a.astype(np.float64).reshape(k, m).T @ b.astype(np.float64).reshape(n, k).T
    fa, fb = 2.0 ** sa, 2.0 ** sb
    bound = k * (0.5 / fa * np.abs(b).max() + 0.5 / fb * np.abs(a).max() + 0.25 / (fa * fb))
    assert np.abs(got * 2.0 ** -(sa + sb) - exact).max() <= bound


def test_example_runs_on_the_gpu(xs, torch_gpu, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    exe = tmp_path / "quant_caller"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "quant_caller.c"),
                    "-o", str(exe), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "quant_caller" in res.stdout
