"""The restatement of libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n that the hash tests compare against, their
case lists and their seeded inputs.

Reference: src/libxsmm_math.c:260-263 with src/libxsmm_hash.c (libxsmm_hash is libxsmm_crc32(seed, data, size): CRC-32C, reflected
polynomial 0x82F63B78, the register starts at the seed, nothing is inverted), src/libxsmm_diff.c:131-146, src/libxsmm_diff.h:76-98.

CRC is linear over GF(2). adv(c, n) is the register after n zero bytes, the n-th power of the 32 x 32 bit matrix of one zero
byte applied to c, and crc(s, A + B) = adv(crc(s, A), len(B)) ^ crc(0, B). Nothing here walks more bytes than it has to: a range
of a large buffer comes from the prefix values of the buffer (Prefix), a mostly-zero buffer from its few non-zero bytes (sparse)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
POLY = 0x82F63B78
SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF, 0x9E3779B9, 0x01234567)
OFFSETS = (0, 1, 7, 15)


# ---- the definition ------------------------------------------------------------------------------------------------------------
def make_table():
    table = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
        table.append(c)
    return table


TABLE = make_table()
TABLE_NP = np.array(TABLE, dtype=np.uint32)


def crc(data, seed=0):
    """byte by byte: crc = T[(crc ^ byte) & 0xFF] ^ (crc >> 8)"""
    c = seed
    for b in bytes(data):
        c = TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c


# ---- adv by matrix powers (the operator of one zero byte, squared k times, is the operator of 2^k zero bytes) ---------------
def matrix_times(mat, vec):
    out, i = 0, 0
    while vec:
        if vec & 1:
            out ^= mat[i]
        vec >>= 1
        i += 1
    return out


def matrix_square(mat):
    return [matrix_times(mat, mat[i]) for i in range(32)]


def byte_matrix():
    """column i: what one zero byte makes of the register 1 << i"""
    return [crc(b"\0", 1 << i) for i in range(32)]


_POWERS = [byte_matrix()]


def adv(c, n):
    """the register c after n zero bytes, O(log n)"""
    k = 0
    while n:
        if k == len(_POWERS):
            _POWERS.append(matrix_square(_POWERS[-1]))
        if n & 1:
            c = matrix_times(_POWERS[k], c)
        n >>= 1
        k += 1
    return c


def crc_rows(rows, seed=0):
    """the crc of every row of a 2-d array of bytes, the rows side by side in numpy"""
    c = np.full(rows.shape[0], seed, dtype=np.uint32)
    for j in range(rows.shape[1]):
        c = TABLE_NP[(c ^ rows[:, j]) & 0xFF] ^ (c >> 8)
    return c


def items_of(buf, start, line_bytes, lines, ld, stride, batch):
    """the items of a batch as rows: item i is the concatenation of its lines (a view where that can be one)"""
    view = np.lib.stride_tricks.as_strided(buf[start:], shape=(batch, lines, line_bytes), strides=(stride, ld, 1), writeable=False)
    return view.reshape(batch, lines * line_bytes) if 1 != lines else view[:, 0, :]


def sparse(size, bytes_at, seed=0):
    """crc of `size` zero bytes but for {position: value}: adv(seed, size) ^ XOR adv(crc(0, [value]), bytes after it)"""
    c = adv(seed, size)
    for pos, value in bytes_at.items():
        assert 0 <= pos < size
        c ^= adv(TABLE[value & 0xFF], size - 1 - pos)
    return c


class Prefix:
    """crc of any range of one large buffer: the values crc(0, buf[:i * CHUNK]) once (the chunks side by side in numpy, then
    one pass over them), a range from two of them and at most 2 * CHUNK bytes walked"""
    CHUNK = 4096

    def __init__(self, buf):
        self.buf = buf
        k = len(buf) // self.CHUNK
        cols = np.ascontiguousarray(buf[:k * self.CHUNK].reshape(k, self.CHUNK).T)
        c = np.zeros(k, dtype=np.uint32)
        for j in range(self.CHUNK):
            c = TABLE_NP[(c ^ cols[j]) & 0xFF] ^ (c >> 8)
        step = [[adv(b << (8 * byte), self.CHUNK) for b in range(256)] for byte in range(4)]
        self.at = [0]
        acc = 0
        for x in c.tolist():
            acc = step[0][acc & 0xFF] ^ step[1][(acc >> 8) & 0xFF] ^ step[2][(acc >> 16) & 0xFF] ^ step[3][acc >> 24] ^ x
            self.at.append(acc)

    def upto(self, end):
        i = min(end // self.CHUNK, len(self.at) - 1)
        return crc(self.buf[i * self.CHUNK:end].tobytes(), self.at[i])

    def crc(self, start, end, seed=0):
        return adv(seed, end - start) ^ adv(self.upto(start), end - start) ^ self.upto(end)


# ---- the compare functions -------------------------------------------------------------------------------------------------------
def memcmp(a, b):
    return 0 if bytes(a) == bytes(b) else 1


def diff_n(a, bn, size, stride, hint, n):
    """the first item equal to a in the order hint, hint + 1, ..., n - 1, 0, ..., hint - 1 (hint taken modulo n), n if none, 0 for n == 0"""
    if 0 == n:
        return 0
    a, bn = bytes(a)[:size], bytes(bn)
    for k in range(n):
        i = (hint + k) % n
        if bn[i * stride:i * stride + size] == a:
            return i
    return n


def item_bytes(buf, start, line_bytes, lines, ld):
    """an item as the batch forms see it: the concatenation of its lines"""
    return b"".join(bytes(buf[start + j * ld:start + j * ld + line_bytes]) for j in range(lines))


# ---- the geometry of the kernels (kernels/hash_plan.h) --------------------------------------------------------------------------
def plan_constants():
    text = open(os.path.join(ROOT, "libxsmm-1_amd", "csrc", "kernels", "hash_plan.h")).read()
    names = {}
    for m in re.finditer(r"constexpr int (HASH_\w+) = ([^;]+);", text):
        names[m.group(1)] = int(eval(m.group(2), {}, names))
    return names


K = plan_constants()
PASS = K["HASH_PASS"]                                   # one step of a wave
WAVE_SPAN = K["HASH_SPAN_MIN"]                          # the least a wave is given
GROUP_SPAN = WAVE_SPAN * K["HASH_WAVES"]                # ... and a work-group
GRID = K["HASH_MAX_BLOCKS"]
FILL = GROUP_SPAN * GRID                                # the size that first fills the grid; past it the span of a wave grows
ITEM_MAX = K["HASH_ITEM_MAX"]                           # the largest item of the wave-per-item form


def around(x):
    return [x - 1, x, x + 1]


def single_sizes():
    """every size up to 130, then one either side of every size at which the kernels take another path"""
    sizes = set(range(0, 131))
    for edge in (16, PASS, WAVE_SPAN, GROUP_SPAN, FILL, 2 * FILL):
        sizes.update(around(edge))
    return sorted(sizes)


def span_boundaries(size, offset):
    """the byte positions of a buffer of `size` bytes at address offset (mod 16) where one wave's unit ends and the next begins"""
    waves = GRID * K["HASH_WAVES"]
    span = max(WAVE_SPAN, -(-(-(-size // waves)) // PASS) * PASS)  # the share of a wave, rounded up to whole steps
    head = min(size, -offset % 16)
    return [head + s * span for s in range(1, -(-size // span)) if head + s * span < size]


def seeded(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


# ---- the cases of the capture (tools/golden/hash_capture.py -> tests/golden/hash.npz) ---------------------------------------
HASH_CASES = [(size, offset, seed) for size in (0, 1, 3, 4, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 4095, 4096, 4097, 70001)
              for offset, seed in ((0, 0), (1, 0xFFFFFFFF), (7, 0x80000000), (15, 0x9E3779B9))]
DIFF_N_CASES = [  # size, stride, hint, n, the items equal to a
    (16, 16, 0, 7, (3,)), (16, 16, 4, 7, (3, 5)), (16, 16, 6, 7, (1, 2)), (16, 16, 2, 7, ()), (5, 9, 0, 40, (39,)), (5, 9, 39, 40, (0, 38)),
    (255, 255, 1, 3, (0,)), (1, 1, 100, 200, (99, 101)), (32, 40, 0, 1, (0,)), (32, 40, 0, 1, ())]


def hash_case_input(size, offset, seed):
    """the bytes of a capture case: `size` bytes, `offset` past the start of a seeded buffer"""
    return seeded(1000 + size, size + 16)[offset:offset + size]


def diff_n_case_input(index):
    size, stride, hint, n, equal = DIFF_N_CASES[index]
    bn = seeded(2000 + index, n * stride)
    a = seeded(3000 + index, size)
    for i in equal:
        bn[i * stride:i * stride + size] = a
    return a, bn


def load_golden():
    return np.load(os.path.join(GOLDEN, "hash.npz"))
