"""Hash and byte compare, without a GPU: the new symbols are exported and declared, the headers compile as C89 and as C++, the
restatement of tests/hash_common.py -- the gold of the GPU tests -- equals what the reference returns (tests/golden/hash.npz), the
published check value and the reference's table, the host paths of all four functions equal the restatement through the C-ABI,
wrong calls of the extensions fail quietly and write nothing, the partition of kernels/hash_plan.h covers every byte once
(tools/hash_walk.cpp under the sanitizers), and the kernels compile for gfx950 without scratch memory or spills.

Reference: src/libxsmm_math.c:260-263, src/libxsmm_hash.c, src/libxsmm_diff.c:131-146, src/libxsmm_diff.h:76-98."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hash_common as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FUNCTIONS = ["libxsmm_hash", "libxsmm_memcmp", "libxsmm_diff", "libxsmm_diff_n"]
AMD_FUNCTIONS = ["libxsmm_amd_hash_async", "libxsmm_amd_hash_batch", "libxsmm_amd_memcmp_async", "libxsmm_amd_memcmp_batch"]
SIZES = list(range(0, 66)) + [255, 256, 257, 4095, 4096, 4097]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_symbols_are_exported_and_declared(xs):
    out = subprocess.run(["nm", "-D", "--defined-only", xs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in REFERENCE_FUNCTIONS + AMD_FUNCTIONS if n not in exported]
    for header, names in (("libxsmm.h", REFERENCE_FUNCTIONS), ("libxsmm_amd.h", AMD_FUNCTIONS)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = {m.group(1) for m in re.finditer(r"LIBXSMM_API(?:EXT)?\s+[^;{]*?\b(libxsmm_\w+)\s*\(", text)}
        assert set(names) <= declared, header
    for n in REFERENCE_FUNCTIONS + AMD_FUNCTIONS:
        assert getattr(xs.lib(), n) is not None


def test_headers_compile_as_c89_and_cxx_and_link(xs, tmp_path):
    src = tmp_path / "t.c"
    src.write_text("#include <libxsmm.h>\n#include <libxsmm_math.h>\n#include <libxsmm_amd.h>\ntypedef void (*fn)(void);\n"
                   "int main(void) { const fn f[] = { (fn)libxsmm_amd_hash_async, (fn)libxsmm_amd_hash_batch, (fn)libxsmm_amd_memcmp_async, (fn)libxsmm_amd_memcmp_batch };\n"
                   "  const char a[] = \"123456789\", b[] = \"123456780\";\n"
                   "  return (int)(0 == f[0] || 0 == f[1] || 0 == f[2] || 0 == f[3] || 0x1CF96D7Cu != libxsmm_hash(a, 9, 0xFFFFFFFFu) || 0 != libxsmm_memcmp(a, b, 8)\n"
                   "    || 1 != libxsmm_memcmp(a, b, 9) || 0 != libxsmm_diff(a, b, 8) || 0 == libxsmm_diff(a, b, 9) || 4 != libxsmm_diff_n(a + 4, a, 1, 1, 2, 9)); }\n")
    libdir = os.path.dirname(xs.LIB_PATH)
    for cc, std in (("gcc", "-std=c89"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c" if cc == "gcc" else "c++", str(src), "-o", str(exe),
                        "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        assert subprocess.run([str(exe)]).returncode == 0


def test_example_compiles(xs, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    res = subprocess.run(["gcc", "-std=c89", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "hash_caller.c"),
                          "-o", str(tmp_path / "hash_caller"), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_known_values_and_the_table():
    assert hc.TABLE[:3] == [0x00000000, 0xF26B8303, 0xE13B70F7]              # src/libxsmm_hash.c:313
    assert hc.crc(b"123456789", 0xFFFFFFFF) == 0x1CF96D7C == 0xE3069283 ^ 0xFFFFFFFF  # the published check value of CRC-32C
    assert hc.crc(b"123456789", 0) == 0x58E3FA20
    assert all(hc.crc(b"abc"[:0], s) == s for s in hc.SEEDS)
    assert all(hc.crc(bytes(n), 0) == 0 for n in (1, 16, 1000))


def test_the_algebra_of_the_restatement():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 5, 255, 256, 1000, 4097):
        for c in (1, 0x80000000, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))):
            assert hc.adv(c, n) == hc.crc(bytes(n), c), (c, n)
    data = hc.seeded(6, 9000)
    for cut in (0, 1, 16, 4096, 8999, 9000):
        for s in hc.SEEDS:
            assert hc.crc(data, s) == hc.adv(hc.crc(data[:cut], s), 9000 - cut) ^ hc.crc(data[cut:], 0)
    pieces = (0, 7, 1024, 1031, 5000, 9000)  # any split: adv(seed, n) ^ XOR of the pieces, each advanced over what follows it
    for s in hc.SEEDS:
        total = hc.adv(s, 9000)
        for lo, hi in zip(pieces[:-1], pieces[1:]):
            total ^= hc.adv(hc.crc(data[lo:hi], 0), 9000 - hi)
        assert total == hc.crc(data, s)
    prefix = hc.Prefix(data)
    for lo, hi in ((0, 9000), (1, 8999), (4095, 4097), (4096, 8192), (17, 17), (8999, 9000)):
        assert prefix.crc(lo, hi, 0x1234) == hc.crc(data[lo:hi], 0x1234)
    assert hc.sparse(5000, {0: 0x80, 4096: 1, 4999: 0xFF}, 7) == hc.crc(bytes([0x80]) + bytes(4095) + b"\x01" + bytes(902) + b"\xff", 7)


def test_restatement_equals_the_capture():
    g = hc.load_golden()
    assert len(g["hash"]) == len(hc.HASH_CASES) and len(g["diff_n"]) == len(hc.DIFF_N_CASES)
    for (size, offset, seed), want, cmp in zip(hc.HASH_CASES, g["hash"], g["compare"]):
        a = hc.hash_case_input(size, offset, seed)
        assert hc.crc(a, seed) == int(want), (size, offset, seed)
        b = a.copy()
        if 0 < size:
            b[-1] ^= 0x40
        diff = lambda v: -1 if 255 < size else v  # (libxsmm_diff takes sizes up to 255)
        assert [int(v) for v in cmp] == [hc.memcmp(a, a), diff(hc.memcmp(a, a)), hc.memcmp(a, b), diff(hc.memcmp(a, b))]
    for index, (size, stride, hint, n, _) in enumerate(hc.DIFF_N_CASES):
        a, bn = hc.diff_n_case_input(index)
        assert hc.diff_n(a, bn, size, stride, hint, n) == int(g["diff_n"][index]), index


# ---- the host paths through the C-ABI -------------------------------------------------------------------------------------------
def test_host_hash_is_the_restatement(xs):
    L = xs.lib()
    n0 = L.libxsmm_amd_launch_count()
    rng = np.random.default_rng(11)
    buf = hc.seeded(12, 4097 + 16)
    seeds = list(hc.SEEDS[:4]) + [int(v) for v in rng.integers(0, 1 << 32, size=2)]
    for offset in range(16):
        for k, size in enumerate(SIZES):
            seed = seeds[(k + offset) % len(seeds)]
            data = buf[offset:offset + size]
            assert L.libxsmm_hash(xs.dptr(data) if size else xs.dptr(buf), size, seed) == hc.crc(data, seed), (size, offset, seed)
    for seed in seeds:
        assert L.libxsmm_hash(xs.dptr(buf), 4097, seed) == hc.crc(buf[:4097], seed)
        assert L.libxsmm_hash(None, 0, seed) == seed and L.libxsmm_hash(xs.dptr(buf), 0, seed) == seed
    assert L.libxsmm_hash(xs.dptr(np.frombuffer(b"123456789", dtype=np.uint8)), 9, 0xFFFFFFFF) == 0x1CF96D7C
    assert n0 == L.libxsmm_amd_launch_count()


def test_host_compares_are_the_restatement(xs):
    L = xs.lib()
    n0 = L.libxsmm_amd_launch_count()
    buf = hc.seeded(13, 4097 + 16)
    for offset in range(16):
        for size in SIZES:
            a = buf[offset:offset + size].copy()
            assert 0 == L.libxsmm_memcmp(xs.dptr(a), xs.dptr(buf[offset:]), size)
            if size <= 255:
                assert 0 == L.libxsmm_diff(xs.dptr(a), xs.dptr(buf[offset:]), size)
            for pos in {0, size // 2, size - 1} if size else ():
                b = a.copy()
                b[pos] ^= 1 << (pos % 8)
                assert 1 == L.libxsmm_memcmp(xs.dptr(a), xs.dptr(b), size) == hc.memcmp(a, b)
                if size <= 255:
                    assert 0 != L.libxsmm_diff(xs.dptr(a), xs.dptr(b), size)
    assert 0 == L.libxsmm_memcmp(None, None, 0) and 0 == L.libxsmm_diff(None, None, 0)
    assert n0 == L.libxsmm_amd_launch_count()


@pytest.mark.parametrize("index", range(len(hc.DIFF_N_CASES)))
def test_host_diff_n_is_the_restatement(xs, index):
    """hint 0 and above; matches on both sides of the hint, only before it, none; stride > size"""
    L = xs.lib()
    size, stride, hint, n, equal = hc.DIFF_N_CASES[index]
    a, bn = hc.diff_n_case_input(index)
    want = hc.diff_n(a, bn, size, stride, hint, n)
    assert want == int(hc.load_golden()["diff_n"][index])
    assert L.libxsmm_diff_n(xs.dptr(a), xs.dptr(bn), size, stride, hint, n) == want
    for h in range(n):  # every hint: the first match from there on, going round
        assert L.libxsmm_diff_n(xs.dptr(a), xs.dptr(bn), size, stride, h, n) == hc.diff_n(a, bn, size, stride, h, n)
    for h in (n, n + 1, 3 * n + 2):  # the stated deviation: hint >= n is taken modulo n (the reference reads out of bounds)
        assert L.libxsmm_diff_n(xs.dptr(a), xs.dptr(bn), size, stride, h, n) == hc.diff_n(a, bn, size, stride, h % n, n)
    assert 0 == L.libxsmm_diff_n(xs.dptr(a), xs.dptr(bn), size, stride, hint, 0)


def test_null_operands_give_the_neutral_answer(xs, capfd):
    L = xs.lib()
    x = np.ones(64, dtype=np.uint8)
    L.libxsmm_set_verbosity(0)
    for _ in range(2):
        assert 0x1234 == L.libxsmm_hash(None, 16, 0x1234)
        assert 0 == L.libxsmm_memcmp(None, xs.dptr(x), 16) == L.libxsmm_memcmp(xs.dptr(x), None, 16)
        assert 0 == L.libxsmm_diff(None, xs.dptr(x), 16) == L.libxsmm_diff_n(None, xs.dptr(x), 4, 4, 0, 8) == L.libxsmm_diff_n(xs.dptr(x), None, 4, 4, 0, 8)
    cap = capfd.readouterr()
    assert cap.err == "" and cap.out == ""
    L.libxsmm_set_verbosity(1)
    try:
        for _ in range(2):
            assert 7 == L.libxsmm_hash(None, 16, 7)
        assert 1 == capfd.readouterr().err.count("libxsmm_hash")  # one line, once
    finally:
        L.libxsmm_set_verbosity(0)


# ---- the extensions without a device ---------------------------------------------------------------------------------------------
def test_wrong_calls_fail_quietly_and_write_nothing(xs, capfd):
    L = xs.lib()
    L.libxsmm_set_verbosity(0)
    n0 = L.libxsmm_amd_launch_count()
    x = np.ones(4096, dtype=np.uint8)
    px = xs.dptr(x)
    res = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    guard = res.copy()
    first = C.c_longlong(-2)
    pr, pf = xs.dptr(res), C.byref(first)
    for _ in range(2):
        # a NULL result, a NULL operand with bytes to read, negative counts and strides, a line beyond its leading dimension
        assert 0 != L.libxsmm_amd_hash_async(None, px, 16, 0)
        assert 0 != L.libxsmm_amd_hash_async(pr, None, 16, 0)
        assert 0 != L.libxsmm_amd_memcmp_async(None, px, px, 16)
        assert 0 != L.libxsmm_amd_memcmp_async(pr, None, px, 16) and 0 != L.libxsmm_amd_memcmp_async(pr, px, None, 16)
        for args in ((None, px, 16, 2, 32, 64, 4, 0), (pr, None, 16, 2, 32, 64, 4, 0), (pr, px, 16, -1, 32, 64, 4, 0), (pr, px, 16, 2, 32, 64, -1, 0),
                     (pr, px, 16, 2, 32, -64, 4, 0), (pr, px, 16, 2, 15, 64, 4, 0), (pr, px, 16, 2, -32, 64, 4, 0)):
            assert 0 != L.libxsmm_amd_hash_batch(*args), args
        for args in ((None, pf, px, px, 16, 2, 32, 32, 64, 64, 4), (pr, pf, None, px, 16, 2, 32, 32, 64, 64, 4), (pr, pf, px, None, 16, 2, 32, 32, 64, 64, 4),
                     (pr, pf, px, px, 16, -2, 32, 32, 64, 64, 4), (pr, pf, px, px, 16, 2, 32, 32, 64, 64, -4), (pr, pf, px, px, 16, 2, 32, 32, -64, 64, 4),
                     (pr, pf, px, px, 16, 2, 32, 32, 64, -64, 4), (pr, pf, px, px, 16, 2, 15, 32, 64, 64, 4), (pr, pf, px, px, 16, 2, 32, 15, 64, 64, 4)):
            assert 0 != L.libxsmm_amd_memcmp_batch(*args), args
        # the _async forms need a result the GPU reaches: plain host memory is refused (with or without a device)
        assert 0 != L.libxsmm_amd_hash_async(pr, px, 16, 0) and 0 != L.libxsmm_amd_memcmp_async(pr, px, px, 16)
    assert np.array_equal(res, guard) and -2 == first.value and n0 == L.libxsmm_amd_launch_count()
    cap = capfd.readouterr()
    assert cap.out == "" and ("" == cap.err or 0 == L.libxsmm_amd_device_count())  # (without a device the refusal of the last pair is the loud one)


def test_empty_calls_give_the_neutral_answer_and_launch_nothing(xs):
    L = xs.lib()
    n0 = L.libxsmm_amd_launch_count()
    x = np.ones(64, dtype=np.uint8)
    res = np.full(6, 0x5A5A5A5A, dtype=np.uint32)
    first = C.c_longlong(-2)
    assert 0 == L.libxsmm_amd_hash_async(xs.dptr(res), None, 0, 0xABCD) and 0xABCD == res[0] and 0x5A5A5A5A == res[1]
    assert 0 == L.libxsmm_amd_memcmp_async(xs.dptr(res), None, None, 0) and 0 == res[0] and 0x5A5A5A5A == res[1]
    for line_bytes, lines in ((0, 3), (16, 0)):  # an empty item: the seed per item, or "equal"
        res[:] = 0x5A5A5A5A
        assert 0 == L.libxsmm_amd_hash_batch(xs.dptr(res), xs.dptr(x), line_bytes, lines, 16, 16, 4, 0x77)
        assert res.tolist() == [0x77] * 4 + [0x5A5A5A5A] * 2
        assert 0 == L.libxsmm_amd_memcmp_batch(xs.dptr(res), C.byref(first), xs.dptr(x), xs.dptr(x), line_bytes, lines, 16, 16, 16, 16, 4)
        assert res.tolist() == [0] * 4 + [0x5A5A5A5A] * 2 and -1 == first.value
        first.value = -2
    res[:] = 0x5A5A5A5A  # batch == 0: nothing per item, no item differs
    assert 0 == L.libxsmm_amd_hash_batch(xs.dptr(res), xs.dptr(x), 16, 1, 16, 16, 0, 0x77)
    assert 0 == L.libxsmm_amd_memcmp_batch(xs.dptr(res), C.byref(first), xs.dptr(x), xs.dptr(x), 16, 1, 16, 16, 16, 16, 0)
    assert res.tolist() == [0x5A5A5A5A] * 6 and -1 == first.value and n0 == L.libxsmm_amd_launch_count()


# ---- the partition and the kernels -------------------------------------------------------------------------------------------------
def test_the_geometry_the_size_lists_follow():
    assert (hc.PASS, hc.WAVE_SPAN, hc.GROUP_SPAN, hc.GRID) == (1024, 4096, 16384, 2048) and hc.FILL == 32 << 20 and hc.ITEM_MAX == 16384
    sizes = hc.single_sizes()
    assert all(s in sizes for s in (0, 130, 15, 17, 1023, 1025, 4095, 4097, 16383, 16385, hc.FILL - 1, hc.FILL + 1, 2 * hc.FILL - 1, 2 * hc.FILL + 1))
    assert hc.span_boundaries(3 * 4096, 0) == [4096, 8192] and hc.span_boundaries(3 * 4096, 9) == [7 + 4096, 7 + 8192]
    assert hc.span_boundaries(2 * hc.FILL + 1, 0)[0] == 9 * 1024  # past twice the fill the span of a wave has grown


def test_walk_of_the_partition_under_the_sanitizers(tmp_path):
    """tools/hash_walk.cpp: every byte covered once, the combined value is the bytewise CRC, sizes 0...5000 at offsets 0...31 and the boundaries"""
    exe = tmp_path / "hash_walk"
    subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "hash_walk.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert 0 == res.returncode and " 0 failures" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])


def test_kernels_compile_for_gfx950_without_scratch_or_spills(tmp_path):
    """read from the compiler's metadata of every kernel of kernels/hash.hip"""
    out = tmp_path / "hash.s"
    csrc = os.path.join(ROOT, "libxsmm-1_amd", "csrc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
                    os.path.join(csrc, "kernels", "hash.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*(?:hash_\w+_kernel|diff_n_kernel)\S*)", asm)
    assert 8 == len(set(kernels)), kernels  # items, units and close for hash and compare, first, diff_n
    for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        values = re.findall(r"\.%s:\s*(\d+)" % field, asm)
        assert len(values) == len(set(kernels)) and all("0" == v for v in values), (field, values)
    assert not re.findall(r"\bscratch_\w+", asm)
