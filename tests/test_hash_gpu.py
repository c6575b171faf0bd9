"""libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n on operands in device memory, and libxsmm_amd_hash_async /
_hash_batch / _memcmp_async / _memcmp_batch, against the restatement of tests/hash_common.py, which tests/test_hash_cpu.py holds
against what the reference returns. Every comparison is integer equality. The sizes are those at which the kernels take another
path (tests/hash_common.py reads them from kernels/hash_plan.h): a lane's word, a wave's step, the least span of a wave and of a
work-group, the size that fills the grid and twice that, where the span of a wave grows; every test also checks that its
inputs are unchanged and that the words around its results are intact.

One random buffer of a little over twice the grid-filling size serves all tests that read large ranges: the expected value of
a range comes from the buffer's prefix values (hash_common.Prefix), computed once."""
import ctypes as C

import numpy as np
import pytest

import hash_common as hc

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def feature(xs):
    """before any device pointer reaches libxsmm_hash: a library without the feature fails here, by assertion"""
    assert all(hasattr(xs.lib(), n) for n in ("libxsmm_hash", "libxsmm_memcmp", "libxsmm_diff", "libxsmm_diff_n", "libxsmm_amd_hash_async",
                                              "libxsmm_amd_hash_batch", "libxsmm_amd_memcmp_async", "libxsmm_amd_memcmp_batch"))


class Big:
    def __init__(self, torch):
        self.host = hc.seeded(2024, 2 * hc.FILL + 1 + 32)
        self.prefix = hc.Prefix(self.host)
        self.dev = torch.from_numpy(self.host).cuda()
        self.base = self.dev.data_ptr()
        assert 0 == self.base % 16

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


@pytest.fixture(scope="module")
def big(torch_gpu):
    return Big(torch_gpu)


class Results:
    """`count` 32-bit results in device memory between two canary words"""
    def __init__(self, torch, count=1, dtype=None):
        self.t = torch.full((count + 2,), CANARY, dtype=torch.int32 if dtype is None else dtype, device="cuda")
        self.ptr = self.t.data_ptr() + self.t.element_size()
        self.count = count

    def take(self):
        v = self.t.cpu().numpy()
        assert CANARY == int(v[0]) and CANARY == int(v[-1]), "a word next to the results was written"
        return v[1:-1].view(np.uint32 if 4 == v.itemsize else np.int64)


def hash_both_ways(xs, torch, ptr, size, seed):
    """libxsmm_hash (waits, returns the value) and libxsmm_amd_hash_async (device result, nobody waits) must agree"""
    L = xs.lib()
    out = Results(torch)
    assert 0 == L.libxsmm_amd_hash_async(out.ptr, ptr, size, seed)
    sync = L.libxsmm_hash(ptr, size, seed) if size < 1 << 32 else None
    torch.cuda.synchronize()
    value = int(out.take()[0])
    assert sync is None or sync == value, (size, seed, sync, value)
    return value


# ---- single buffers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", hc.OFFSETS)
def test_single_buffers(xs, torch_gpu, big, offset):
    L = xs.lib()
    n0 = L.libxsmm_amd_launch_count()
    for k, size in enumerate(hc.single_sizes()):
        seed = hc.SEEDS[(k + offset) % len(hc.SEEDS)]
        got = hash_both_ways(xs, torch_gpu, big.base + offset, size, seed)
        assert got == big.prefix.crc(offset, offset + size, seed), (size, offset, seed)
    assert L.libxsmm_amd_launch_count() > n0 and xs.last_kernel().startswith("hash_")
    assert big.unchanged()


def test_zeros_with_each_seed(xs, torch_gpu):
    """all zeros: the value is adv(seed, size) alone"""
    zeros = torch_gpu.zeros(3 * hc.GROUP_SPAN + 64, dtype=torch_gpu.uint8, device="cuda")
    for size in (1, 17, hc.PASS + 1, hc.WAVE_SPAN + 1, 3 * hc.GROUP_SPAN + 5):
        for offset in (0, 9):
            for seed in hc.SEEDS:
                assert hash_both_ways(xs, torch_gpu, zeros.data_ptr() + offset, size, seed) == hc.adv(seed, size), (size, offset, seed)
    assert 0 == int(zeros.max())


def probe_positions(size, offset):
    """the first byte, the last byte and both sides of every boundary between two waves' spans"""
    return sorted({0, size - 1} | {p for b in hc.span_boundaries(size, offset) for p in (b - 1, b)})


@pytest.mark.parametrize("offset", [0, 9])
def test_single_set_bits(xs, torch_gpu, offset):
    """seed 0, one set bit: the value is that bit advanced over what follows it"""
    size = 3 * hc.WAVE_SPAN + 100
    buf = torch_gpu.zeros(size + 32, dtype=torch_gpu.uint8, device="cuda")
    positions = probe_positions(size, offset)
    assert len(positions) >= 2 + 2 * 3
    for k, pos in enumerate(positions):
        bit = 1 << (k % 8)
        buf[offset + pos] = bit
        assert hash_both_ways(xs, torch_gpu, buf.data_ptr() + offset, size, 0) == hc.sparse(size, {pos: bit}), (pos, bit)
        buf[offset + pos] = 0
    assert 0 == int(buf.max())


@pytest.mark.parametrize("offset", [0, 7])
def test_no_byte_is_dropped(xs, torch_gpu, big, offset):
    """CRC-32 detects every burst of at most 32 bits: flipping one byte must change the hash, to the value the algebra gives"""
    L = xs.lib()
    for size in hc.around(hc.WAVE_SPAN) + hc.around(hc.GROUP_SPAN) + [8 * hc.GROUP_SPAN + 5]:
        base = L.libxsmm_hash(big.base + offset, size, 7)
        assert base == big.prefix.crc(offset, offset + size, 7)
        for pos in probe_positions(size, offset):
            big.dev[offset + pos] ^= 0x10
            got = L.libxsmm_hash(big.base + offset, size, 7)
            big.dev[offset + pos] ^= 0x10
            assert got != base and got == base ^ hc.adv(hc.TABLE[0x10], size - 1 - pos), (size, pos)
    assert big.unchanged()


def test_past_four_gib(xs, torch_gpu):
    """2^32 + 17 bytes, all zero but for six: the expected value needs no walk; the same buffer against a copy that differs in its last byte"""
    torch, L = torch_gpu, xs.lib()
    size = (1 << 32) + 17
    marks = {0: 0x01, (1 << 31) - 1: 0x80, 1 << 31: 0x7F, (1 << 32) - 1: 0xFF, 1 << 32: 0x10, size - 1: 0x02}
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    for pos, value in marks.items():
        buf[pos] = value
    for seed in (0, 0xFFFFFFFF):
        assert hash_both_ways(xs, torch, buf.data_ptr(), size, seed) == hc.sparse(size, marks, seed)
    other = buf.clone()
    out = Results(torch, 2)
    assert 0 == L.libxsmm_amd_memcmp_async(out.ptr, buf.data_ptr(), other.data_ptr(), size)
    other[size - 1] = 0x03
    assert 0 == L.libxsmm_amd_memcmp_async(out.ptr + 4, buf.data_ptr(), other.data_ptr(), size)
    torch.cuda.synchronize()
    assert out.take().tolist() == [0, 1]
    assert 1 == L.libxsmm_memcmp(buf.data_ptr(), other.data_ptr(), size) and 0 == L.libxsmm_memcmp(buf.data_ptr(), other.data_ptr(), size - 1)
    # an item beyond 2^31 bytes from the first: two items 2^31 + 5 bytes apart
    stride, item = (1 << 31) + 5, 64
    want = [hc.sparse(item, {0: 0x01}, 3), hc.sparse(item, {}, 3)]
    buf[stride + 9] = 0x33
    want[1] = hc.sparse(item, {9: 0x33}, 3)
    out = Results(torch, 2)
    assert 0 == L.libxsmm_amd_hash_batch(out.ptr, buf.data_ptr(), item, 1, 0, stride, 2, 3)
    host = np.full(4, CANARY, dtype=np.uint32)
    assert 0 == L.libxsmm_amd_hash_batch(host[1:].ctypes.data, buf.data_ptr(), item, 1, 0, stride, 2, 3)
    torch.cuda.synchronize()
    assert out.take().tolist() == want == host[1:3].tolist() and CANARY == host[0] == host[3]
    zero = torch.zeros(item, dtype=torch.uint8, device="cuda")
    flags, first = Results(torch, 2), Results(torch, 1, torch.int64)
    buf[0] = 0
    assert 0 == L.libxsmm_amd_memcmp_batch(flags.ptr, first.ptr, buf.data_ptr(), zero.data_ptr(), item, 1, 0, 0, stride, 0, 2)
    torch.cuda.synchronize()
    assert flags.take().tolist() == [0, 1] and 1 == int(first.take()[0])


# ---- batches -------------------------------------------------------------------------------------------------------------------
ITEMS_PER_PASS = hc.GRID * hc.K["HASH_WAVES"]


def run_hash_batch(xs, torch, ptr, line_bytes, lines, ld, stride, batch, seed):
    """results in device memory and in host memory: both must be the same"""
    L = xs.lib()
    out = Results(torch, batch)
    assert 0 == L.libxsmm_amd_hash_batch(out.ptr, ptr, line_bytes, lines, ld, stride, batch, seed)
    host = np.full(batch + 2, CANARY, dtype=np.uint32)
    assert 0 == L.libxsmm_amd_hash_batch(host[1:].ctypes.data, ptr, line_bytes, lines, ld, stride, batch, seed)  # complete on return
    got = host[1:-1].copy()
    assert CANARY == host[0] == host[-1]
    torch.cuda.synchronize()
    assert np.array_equal(out.take(), got)
    return got


@pytest.mark.parametrize("item,stride", [(1, 1), (5, 7), (16, 16), (16, 19), (64, 67), (4096, 2040)])
def test_batch_past_the_grid(xs, torch_gpu, big, item, stride):
    """4 passes of the grid and a remainder of 3 items; strides that put the items at every alignment; overlapping items"""
    batch = 4 * ITEMS_PER_PASS + 3
    got = run_hash_batch(xs, torch_gpu, big.base + 3, item, 1, 0, stride, batch, 0x9E3779B9)
    want = hc.crc_rows(hc.items_of(big.host, 3, item, 1, 0, stride, batch), 0x9E3779B9)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert xs.last_kernel() == "hash_items" and big.unchanged()


def test_batch_of_items_past_the_wave_form(xs, torch_gpu, big):
    """the first size a wave does not take: the items go through the units one after the other"""
    item, stride, batch = hc.ITEM_MAX + 1, hc.ITEM_MAX + 1 + 7, 3
    got = run_hash_batch(xs, torch_gpu, big.base + 5, item, 1, 0, stride, batch, 1)
    assert got.tolist() == [big.prefix.crc(5 + i * stride, 5 + i * stride + item, 1) for i in range(batch)]
    assert xs.last_kernel() == "hash_units"
    got = run_hash_batch(xs, torch_gpu, big.base + 5, hc.ITEM_MAX, 1, 0, stride, batch, 1)
    assert got.tolist() == [big.prefix.crc(5 + i * stride, 5 + i * stride + hc.ITEM_MAX, 1) for i in range(batch)]
    assert xs.last_kernel() == "hash_items" and big.unchanged()


@pytest.mark.parametrize("line_bytes,lines,ld,stride,batch", [(24, 5, 37, 200, 1000), (5000, 4, 5003, 20011, 2), (1, 300, 3, 1000, 9)])
def test_items_with_gaps(xs, torch_gpu, line_bytes, lines, ld, stride, batch):
    """two copies whose gap bytes are poisoned differently hash equal and compare equal: nothing between line_bytes and ld is read"""
    torch, L = torch_gpu, xs.lib()
    extent = (batch - 1) * stride + (lines - 1) * ld + line_bytes
    data = hc.seeded(77, extent + 16)
    rows = hc.items_of(data, 2, line_bytes, lines, ld, stride, batch)
    want = hc.crc_rows(rows, 5)
    copies = []
    for poison in (0x00, 0xFF):
        c = np.full(extent + 16, poison, dtype=np.uint8)
        for i in range(batch):
            for j in range(lines):
                lo = 2 + i * stride + j * ld
                c[lo:lo + line_bytes] = data[lo:lo + line_bytes]
        copies.append(c)
    devs = [torch.from_numpy(c).cuda() for c in copies]
    for d in devs:
        got = run_hash_batch(xs, torch, d.data_ptr() + 2, line_bytes, lines, ld, stride, batch, 5)
        assert np.array_equal(got, want)
    assert xs.last_kernel() == ("hash_items" if line_bytes * lines <= hc.ITEM_MAX else "hash_units")
    flags, first = Results(torch, batch), Results(torch, 1, torch.int64)
    assert 0 == L.libxsmm_amd_memcmp_batch(flags.ptr, first.ptr, devs[0].data_ptr() + 2, devs[1].data_ptr() + 2, line_bytes, lines, ld, ld, stride, stride, batch)
    torch.cuda.synchronize()
    assert not flags.take().any() and -1 == int(first.take()[0])
    devs[1][2 + (batch - 1) * stride + (lines - 1) * ld + line_bytes - 1] ^= 1  # the last byte of the last line of the last item
    assert 0 == L.libxsmm_amd_memcmp_batch(flags.ptr, first.ptr, devs[0].data_ptr() + 2, devs[1].data_ptr() + 2, line_bytes, lines, ld, ld, stride, stride, batch)
    torch.cuda.synchronize()
    assert flags.take().tolist() == [0] * (batch - 1) + [1] and batch - 1 == int(first.take()[0])
    assert np.array_equal(devs[0].cpu().numpy(), copies[0])


def test_stride_zero(xs, torch_gpu, big):
    got = run_hash_batch(xs, torch_gpu, big.base + 1, 100, 1, 0, 0, 50, 2)
    assert got.tolist() == [big.prefix.crc(1, 101, 2)] * 50


@pytest.mark.parametrize("differing", [(0,), (-1,), (4097, 20000), ()])
@pytest.mark.parametrize("host_results", [False, True])
def test_first_diff(xs, torch_gpu, big, differing, host_results):
    torch, L = torch_gpu, xs.lib()
    item, batch = 16, 4 * ITEMS_PER_PASS + 3
    other = big.dev[:batch * item + 16].clone()
    differing = [d % batch for d in differing]
    for d in differing:
        other[7 + d * item + d % item] ^= 0x80
    if host_results:
        flags, first = np.full(batch + 2, CANARY, dtype=np.int32), np.full(3, -2, dtype=np.int64)
        assert 0 == L.libxsmm_amd_memcmp_batch(flags[1:].ctypes.data, first[1:].ctypes.data, big.base + 7, other.data_ptr() + 7, item, 1, 0, 0, item, item, batch)
        assert CANARY == flags[0] == flags[-1] and -2 == first[0] == first[2]
        got, where = flags[1:-1], int(first[1])
    else:
        flags, first = Results(torch, batch), Results(torch, 1, torch.int64)
        assert 0 == L.libxsmm_amd_memcmp_batch(flags.ptr, first.ptr, big.base + 7, other.data_ptr() + 7, item, 1, 0, 0, item, item, batch)
        torch.cuda.synchronize()
        got, where = flags.take(), int(first.take()[0])
    assert np.flatnonzero(got).tolist() == sorted(differing) and set(np.unique(got).tolist()) <= {0, 1}
    assert where == (min(differing) if differing else -1)
    assert xs.last_kernel() == "hash_first"
    none = Results(torch, batch)  # first_diff may be NULL
    assert 0 == L.libxsmm_amd_memcmp_batch(none.ptr, None, big.base + 7, other.data_ptr() + 7, item, 1, 0, 0, item, item, batch)
    torch.cuda.synchronize()
    assert np.flatnonzero(none.take()).tolist() == sorted(differing)


# ---- compare -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_a,off_b", [(0, 0), (0, 1), (7, 0), (15, 8), (3, 3)])
def test_compare(xs, torch_gpu, big, off_a, off_b):
    """equal buffers; a difference in the first byte, the last byte and at every boundary between two spans; different alignments"""
    torch, L = torch_gpu, xs.lib()
    other = torch.zeros(2 * hc.FILL + 64, dtype=torch.uint8, device="cuda")
    other[off_b:off_b + hc.FILL + 17] = big.dev[off_a:off_a + hc.FILL + 17]
    pa, pb = big.base + off_a, other.data_ptr() + off_b
    out = Results(torch)
    for size in [0, 1, 15, 16, 17, 130] + hc.around(hc.PASS) + hc.around(hc.WAVE_SPAN) + hc.around(hc.GROUP_SPAN) + [3 * hc.WAVE_SPAN + 100, hc.FILL + 1]:
        assert 0 == L.libxsmm_memcmp(pa, pb, size), size
        assert 0 == L.libxsmm_amd_memcmp_async(out.ptr, pa, pb, size)
        torch.cuda.synchronize()
        assert 0 == int(out.take()[0])
        if 0 < size <= 255:
            assert 0 == L.libxsmm_diff(pa, pb, size)
        positions = probe_positions(size, off_a) if size else []
        if 200 < len(positions):  # (thousands of spans: the two ends and the first and the last of the boundaries)
            positions = positions[:3] + positions[-3:]
        for pos in positions:
            other[off_b + pos] ^= 0x04
            got = L.libxsmm_memcmp(pa, pb, size)
            assert 0 == L.libxsmm_amd_memcmp_async(out.ptr, pa, pb, size)
            short = L.libxsmm_diff(pa, pb, size) if size <= 255 else 1
            other[off_b + pos] ^= 0x04
            assert 1 == got == int(out.take()[0]) and 0 != short, (size, pos)
        if size:  # a difference just outside the range is none
            other[off_b + size] ^= 0x04
            assert 0 == L.libxsmm_memcmp(pa, pb, size)
            other[off_b + size] ^= 0x04
    assert xs.last_kernel() == "memcmp_units" and big.unchanged()


def test_compare_with_a_pageable_partner(xs, torch_gpu, big):
    L = xs.lib()
    size = 3 * hc.GROUP_SPAN + 11
    host = big.host[5:5 + size].copy()
    n0 = L.libxsmm_amd_launch_count()
    assert 0 == L.libxsmm_memcmp(host.ctypes.data, big.base + 5, size) == L.libxsmm_memcmp(big.base + 5, host.ctypes.data, size)
    host[size - 1] ^= 1
    assert 1 == L.libxsmm_memcmp(host.ctypes.data, big.base + 5, size) == L.libxsmm_memcmp(big.base + 5, host.ctypes.data, size)
    assert 0 == L.libxsmm_memcmp(host.ctypes.data, big.base + 5, size - 1)
    assert 1 == L.libxsmm_diff(host[size - 200:].ctypes.data, big.base + 5 + size - 200, 200) and 0 == L.libxsmm_diff(host.ctypes.data, big.base + 5, 255)
    assert L.libxsmm_amd_launch_count() > n0
    n1 = L.libxsmm_amd_launch_count()  # two host operands launch nothing
    assert 1 == L.libxsmm_memcmp(host.ctypes.data, big.host[5:].ctypes.data, size) and L.libxsmm_hash(host.ctypes.data, size, 1) == hc.crc(host, 1)
    assert n1 == L.libxsmm_amd_launch_count() and big.unchanged()


# ---- diff_n ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(hc.DIFF_N_CASES)))
@pytest.mark.parametrize("a_on_device", [False, True])
def test_diff_n_cases(xs, torch_gpu, index, a_on_device):
    torch, L = torch_gpu, xs.lib()
    size, stride, hint, n, equal = hc.DIFF_N_CASES[index]
    a, bn = hc.diff_n_case_input(index)
    da, dbn = torch.from_numpy(a).cuda(), torch.from_numpy(bn).cuda()
    pa = da.data_ptr() if a_on_device else a.ctypes.data
    for h in sorted({hint, 0, n - 1, n // 2, n, 2 * n + 1}):
        assert L.libxsmm_diff_n(pa, dbn.data_ptr(), size, stride, h, n) == hc.diff_n(a, bn, size, stride, h % n, n), h
    assert xs.last_kernel() == "diff_n"
    assert 0 == L.libxsmm_diff_n(pa, dbn.data_ptr(), size, stride, hint, 0)
    if a_on_device:  # a on the device, the items pageable
        assert L.libxsmm_diff_n(pa, bn.ctypes.data, size, stride, hint, n) == hc.diff_n(a, bn, size, stride, hint, n)
    assert np.array_equal(dbn.cpu().numpy(), bn) and np.array_equal(da.cpu().numpy(), a)


@pytest.mark.parametrize("a_on_device", [False, True])
def test_diff_n_past_one_pass_of_the_grid(xs, torch_gpu, a_on_device):
    """300 000 items of 16 bytes, the only match at the start, at the end, just before the hint; then two matches and none"""
    torch, L = torch_gpu, xs.lib()
    n, size, hint = 300000, 16, 123457
    bn = hc.seeded(41, n * size)
    a = np.arange(0xE0, 0xF0, dtype=np.uint8)
    dbn, da = torch.from_numpy(bn).cuda(), torch.from_numpy(a).cuda()
    pa = da.data_ptr() if a_on_device else a.ctypes.data
    assert n == L.libxsmm_diff_n(pa, dbn.data_ptr(), size, size, hint, n)
    for where in (0, n - 1, hint - 1, hint):
        dbn[where * size:(where + 1) * size] = da
        for h in (0, hint, n - 1):
            assert where == L.libxsmm_diff_n(pa, dbn.data_ptr(), size, size, h, n), (where, h)
        dbn[where * size] ^= 1
    dbn[5 * size:6 * size] = da
    dbn[(n - 7) * size:(n - 6) * size] = da
    assert [5, n - 7, n - 7, 5] == [L.libxsmm_diff_n(pa, dbn.data_ptr(), size, size, h, n) for h in (0, 6, n - 7, n - 6)]
    assert 1 == L.libxsmm_diff(pa, dbn.data_ptr(), size) and 0 == L.libxsmm_diff(pa, dbn.data_ptr() + 5 * size, size)


# ---- stream order ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bracket", [False, True])
def test_hash_sees_the_product_queued_before_it(xs, torch_gpu, bracket):
    torch, L = torch_gpu, xs.lib()
    m, batch = 8, 64
    rng = np.random.default_rng(11)
    a = rng.integers(-4, 5, batch * m * m).astype(np.float64)
    b = rng.integers(-4, 5, batch * m * m).astype(np.float64)
    want = np.concatenate([(b[i * 64:(i + 1) * 64].reshape(m, m) @ a[i * 64:(i + 1) * 64].reshape(m, m)).reshape(-1) for i in range(batch)])  # column-major A * B
    idx = (np.arange(batch) * m * m).astype(np.int32)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dc = torch.full((batch * m * m,), 12345.0, dtype=torch.float64, device="cuda")
    out = Results(torch, 2)
    size = batch * m * m * 8
    torch.cuda.synchronize()
    n0 = L.libxsmm_amd_launch_count()
    if bracket:
        L.libxsmm_amd_defer_begin()
    xs.gemm_batch(xs.F64, "N", "N", m, m, m, 1.0, da, m, db, m, 0.0, dc, m, 0, 4, idx, idx, idx, batch)
    rc = L.libxsmm_amd_hash_async(out.ptr, dc.data_ptr(), size, 0x1234)  # queued behind the product, nobody waits in between
    if bracket:
        L.libxsmm_amd_defer_end()
    assert 0 == rc
    torch.cuda.synchronize()
    assert L.libxsmm_amd_launch_count() >= n0 + 2
    assert 0 == L.libxsmm_amd_hash_async(out.ptr + 4, dc.data_ptr(), size, 0x1234)
    torch.cuda.synchronize()
    got = out.take().tolist()
    assert got[0] == got[1] == hc.crc(want.tobytes(), 0x1234)  # the product (small integers: exact), not the 12345s
    assert np.array_equal(dc.cpu().numpy(), want)
