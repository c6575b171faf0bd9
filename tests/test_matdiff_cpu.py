"""matdiff on device operands, without a GPU: the new symbols are exported and declared, the headers still compile as C89 and
as C++, the numpy restatement of tests/matdiff_common.py -- the gold of the GPU tests -- reproduces what the reference returns
(tests/golden/matdiff.npz, all three calls of the reference's tests/matdiff.c among them) within the derived bound, plain host
operands go the old way without a launch, and wrong calls of the new entry points fail quietly without a device.

Reference: src/libxsmm_math.c:48-238, src/template/libxsmm_matdiff.tpl.c, tests/matdiff.c."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import matdiff_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD_FUNCTIONS = ["libxsmm_amd_matdiff_async", "libxsmm_amd_matdiff_batch"]
CASES = mc.cases()


def test_symbols_are_exported_and_declared(xs):
    out = subprocess.run(["nm", "-D", "--defined-only", xs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in AMD_FUNCTIONS if n not in exported]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libxsmm_amd.h")).read(), flags=re.S)
    declared = {m.group(1) for m in re.finditer(r"LIBXSMM_API(?:EXT)?\s+[^;{]*?\b(libxsmm_\w+)\s*\(", text)}
    assert set(AMD_FUNCTIONS) <= declared
    for n in AMD_FUNCTIONS:
        assert getattr(xs.lib(), n) is not None


def test_headers_compile_as_c89_and_cxx_and_link(xs, tmp_path):
    src = tmp_path / "t.c"
    src.write_text("#include <libxsmm.h>\n#include <libxsmm_amd.h>\ntypedef void (*fn)(void);\n"
                   "int main(void) { const fn f[] = { (fn)libxsmm_matdiff, (fn)libxsmm_amd_matdiff_async, (fn)libxsmm_amd_matdiff_batch };\n"
                   "  libxsmm_matdiff_info info; libxsmm_matdiff_clear(&info);\n"
                   "  return (int)(0 == f[0] || 0 == f[1] || 0 == f[2] || -1 != info.m || 160 != sizeof(info)); }\n")
    libdir = os.path.dirname(xs.LIB_PATH)
    for cc, std in (("gcc", "-std=c89"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c" if cc == "gcc" else "c++", str(src), "-o", str(exe),
                        "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        assert subprocess.run([str(exe)]).returncode == 0


def test_example_compiles(xs, tmp_path):
    libdir = os.path.dirname(xs.LIB_PATH)
    res = subprocess.run(["gcc", "-std=c89", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "matdiff_caller.c"),
                          "-o", str(tmp_path / "matdiff_caller"), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_captures(name):
    """the reference's compensated sums are within a few ulp of exact: the bound of the GPU tests holds here as well"""
    dt, m, n, ldr, ldt, ref, tst = mc.case_operands(CASES[name])
    rc, got = mc.matdiff(m, n, ref, tst, ldr, ldt)
    grc, want = mc.golden_fields(mc.load_golden(), name)
    assert rc == grc == 0
    special = name.rsplit("_", 1)[0]
    if special in mc.NONFINITE:  # the location always; the nine +inf where ref is finite there (the two deviations of DESIGN.md 8f)
        assert (got["m"], got["n"]) == (want["m"], want["n"])
        if "nan_both" != special:
            assert all(got[f] == want[f] == mc.INF for f in mc.NINE)
        assert all(got[f] == mc.cleared()[f] for f in mc.FIELDS if f not in mc.NINE)
    else:
        mc.compare(got, want, m * n, name, skip=mc.skipped(name))


def test_known_answers_of_the_reference_test():
    """the numbers the reference's tests/matdiff.c states for its three calls (its own program only looks at the last)"""
    g = mc.load_golden()
    for name, known in (("known_3x3_f64", dict(norm1_abs=1.83, norm1_rel=0.0963158, normi_abs=2.44, normi_rel=0.0976, normf_rel=0.1074954, l2_abs=1.8742465,
                                               l2_rel=0.6726295, l1_ref=46.0, l1_tst=45.66, linf_abs=0.93, linf_rel=0.56, m=2, n=2)),
                        ("known_1x3_f64", dict(norm1_abs=3.1, norm1_rel=0.0281818, normi_abs=2.0, normi_rel=0.02, normf_rel=0.0222918, l2_abs=2.2383029,
                                               l2_rel=0.2438908, l1_ref=110.0, l1_tst=111.1, linf_abs=2.0, linf_rel=0.2222222, m=0, n=2)),
                        ("known_3x1_f64", dict(norm1_abs=3.1, norm1_rel=0.0281818, normi_abs=2.0, normi_rel=0.02, normf_rel=0.0222918, l2_abs=2.2383029,
                                               l2_rel=0.2438908, l1_ref=110.0, l1_tst=111.1, linf_abs=2.0, linf_rel=0.2222222, m=2, n=0))):
        dt, m, n, ldr, ldt, ref, tst = mc.case_operands(CASES[name])
        for fields in (mc.matdiff(m, n, ref, tst, ldr, ldt)[1], mc.golden_fields(g, name)[1]):
            for f, v in known.items():
                assert abs(fields[f] - v) < 1e-6, (name, f, fields[f], v)


@pytest.mark.parametrize("name", sorted(mc.BATCHES))
def test_restatement_reproduces_the_batch_captures(name):
    case = mc.BATCHES[name]
    dt, m, n, ldr, ldt, sr, st, batch = case[:8]
    infos, total, item = mc.batch_expected(case)
    g = mc.load_golden()["batch_" + name]
    row = lambda v: (dict(zip(mc.FIELDS, (float(x) for x in v[:19])), m=int(v[19]), n=int(v[20])), int(v[21]))
    if "nan" == case[9]:
        assert 2 == item and (total["m"], total["n"]) == (infos[2]["m"], infos[2]["n"]) == (row(g[2])[0]["m"], row(g[2])[0]["n"])
        assert all(total[f] == mc.INF for f in mc.NINE)
        return
    for b in range(batch):
        want, rc = row(g[b])
        assert 0 == rc
        mc.compare(infos[b], want, m * n, (name, b))
    want, _ = row(g[batch])
    # the averages are the one stated deviation: the mean over the batch here, a running half-sum in the reference
    mc.compare(total, want, m * n, name, count_l1=m * n * batch, skip=("avg_ref", "avg_tst"))
    assert total["avg_ref"] == total["l1_ref"] / (m * n * batch)
    assert item == [i for i, x in enumerate(infos) if x["linf_abs"] == total["linf_abs"]][0]


def host_call(xs, dt, m, n, ref, tst, ldr=None, ldt=None):
    info = xs.MatdiffInfo()
    rc = xs.lib().libxsmm_matdiff(C.byref(info), dt, m, n, xs.dptr(ref), xs.dptr(tst), xs.iptr(ldr), xs.iptr(ldt))
    return rc, info


def test_host_operands_go_the_old_way(xs):
    """not a line of the host loop changed: its known results, its known differences from the reference, and no launch"""
    L = xs.lib()
    n0 = L.libxsmm_amd_launch_count()
    ref, tst = np.array(mc.REF3X3), np.array(mc.TST3X3)
    rc, info = host_call(xs, mc.F64, 3, 3, ref, tst)
    assert 0 == rc and (info.m, info.n) == (2, 2) and abs(info.linf_abs - 0.93) < 1e-12 and abs(info.l1_ref - 46.0) < 1e-12
    assert abs(info.norm1_abs - 2.44) < 1e-12 and abs(info.normi_abs - 1.83) < 1e-12  # the host path's assignment of the two norms
    assert 0 == host_call(xs, mc.F64, 3, 3, ref, tst, 2, 2)[0]                        # it accepts m > ld
    assert 0 != host_call(xs, mc.I32, 3, 3, ref.astype(np.int32), tst.astype(np.int32))[0]  # and refuses the integer types
    assert 0 != host_call(xs, mc.F64, -1, 3, ref, tst)[0] and 0 != host_call(xs, mc.F64, 3, 3, None, None)[0]
    rc, info = host_call(xs, mc.F32, 3, 1, np.array(mc.REFVEC, dtype=np.float32), np.array(mc.TSTVEC, dtype=np.float32))
    assert 0 == rc and abs(info.linf_abs - 2.0) < 1e-6
    assert n0 == L.libxsmm_amd_launch_count()


def test_wrong_calls_fail_quietly_without_a_device(xs, capfd):
    L = xs.lib()
    L.libxsmm_set_verbosity(0)
    n0 = L.libxsmm_amd_launch_count()
    x = np.ones(64)
    info = xs.MatdiffInfo()
    guard = bytes(info)
    p, pi, px = C.byref(info), xs.iptr, xs.dptr(x)
    which = C.c_longlong(-2)
    for _ in range(2):
        for args in ((None, mc.F64, 4, 4, px, px, None, None), (p, mc.F64, 4, 4, None, None, None, None), (p, mc.F64, 4, 4, px, px, pi(3), None),
                     (p, mc.F64, 4, 4, px, px, None, pi(3)), (p, mc.F64, -1, 4, px, px, None, None), (p, mc.F64, 4, -1, px, px, None, None),
                     (p, 2, 4, 4, px, px, None, None), (p, 7, 4, 4, px, px, None, None)):
            assert 0 != L.libxsmm_amd_matdiff_async(*args), args
            assert 0 != L.libxsmm_amd_matdiff_batch(args[0], None, C.byref(which), *args[1:], 16, 16, 2), args
        assert 0 != L.libxsmm_amd_matdiff_batch(p, None, None, mc.F64, 4, 4, px, px, None, None, 16, 16, -1)
        assert 0 != L.libxsmm_amd_matdiff_batch(p, None, None, mc.F64, 4, 4, px, px, None, None, -16, 16, 2)
    assert bytes(info) == guard and -2 == which.value and n0 == L.libxsmm_amd_launch_count()
    cap = capfd.readouterr()
    assert cap.err == "" and cap.out == ""


def test_empty_calls_return_a_cleared_info(xs):
    L = xs.lib()
    x = np.ones(64)
    for m, n in ((0, 4), (4, 0)):
        info = xs.MatdiffInfo()
        C.memset(C.byref(info), 0x5a, C.sizeof(info))
        assert 0 == L.libxsmm_amd_matdiff_async(C.byref(info), mc.F64, m, n, xs.dptr(x), xs.dptr(x), None, None)
        assert mc.fields_of(info) == mc.cleared()
    items = (xs.MatdiffInfo * 2)()
    which = C.c_longlong(-2)
    assert 0 == L.libxsmm_amd_matdiff_batch(C.byref(info), items, C.byref(which), mc.F32, 0, 4, xs.dptr(x), xs.dptr(x), None, None, 16, 16, 2)
    assert -1 == which.value and all(mc.fields_of(i) == mc.cleared() for i in items)
    which = C.c_longlong(-2)
    assert 0 == L.libxsmm_amd_matdiff_batch(C.byref(info), None, C.byref(which), mc.F32, 4, 4, xs.dptr(x), xs.dptr(x), None, None, 16, 16, 0)
    assert -1 == which.value and mc.fields_of(info) == mc.cleared()


def test_the_tile_cases_follow_the_kernel_constants():
    strip, lines, item_max = mc.kernel_constants()
    c = CASES["tile_f32"]
    assert (c[2], c[3]) == (strip + 1, lines + 1) and c[2] * c[3] > item_max  # one past the tile both ways, on the tiled path
    assert 33 * 5 <= item_max < 1000 * 70 and 1000 > 3 * strip and 70 > 4 * lines
