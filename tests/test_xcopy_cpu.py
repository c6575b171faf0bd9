"""Matrix copy and transposition, the part that needs no GPU: exported symbols, descriptor layouts and rules
(src/libxsmm_main.h:171-190, src/libxsmm_generator.c:339-381), dispatch / info / kind / release, the header as C89 and C++,
a C caller of every entry point, and the argument checks of src/libxsmm_xcopy.c:174-177,295-298,386-421 -- which return before
any device probe, write nothing and print one line per entry point only if the verbosity is not zero."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import xcopy_common as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
NEW_SYMBOLS = ["libxsmm_matcopy", "libxsmm_matcopy_thread", "libxsmm_matcopy_omp", "libxsmm_otrans", "libxsmm_otrans_thread", "libxsmm_otrans_omp",
               "libxsmm_itrans", "libxsmm_dispatch_mcopy", "libxsmm_dispatch_trans", "libxsmm_mcopy_descriptor_init", "libxsmm_trans_descriptor_init",
               "libxsmm_get_mcopykernel_info", "libxsmm_get_transkernel_info", "libxsmm_amd_matcopy_batch", "libxsmm_amd_otrans_batch",
               "libxsmm_amd_matcopy_batch_ptr", "libxsmm_amd_otrans_batch_ptr"]


def test_new_symbols_are_exported_and_declared(xs):
    out = subprocess.run(["nm", "-D", "--defined-only", xs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    text = open(os.path.join(ROOT, "include", "libxsmm.h")).read() + open(os.path.join(ROOT, "include", "libxsmm_amd.h")).read()
    assert not [s for s in NEW_SYMBOLS if s + "(" not in text]
    assert "LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE = 1" in text


def u32(raw, at):
    return int.from_bytes(raw[at:at + 4], "little")


def test_descriptor_layouts_and_rules(xs):
    L = xs.lib()
    blob, d = xs.trans_descriptor(8, 5, 7, 9)
    assert d and d == C.addressof(blob)
    raw = C.string_at(C.byref(blob), 64)
    assert (u32(raw, 0), u32(raw, 4), u32(raw, 8), raw[12]) == (5, 7, 9, 8) and not any(raw[13:])  # m, n, ldo, typesize: 13 packed bytes
    # mcopy: only multiples of four bytes; normalised to typesize 4 with m, ldi, ldo scaled; unroll default 2, at most 64
    for ts in (1, 2, 3, 6, 255):
        assert not xs.mcopy_descriptor(ts, 4, 4, 4, 4)[1]
    blob, d = xs.mcopy_descriptor(8, 5, 7, 11, 9, flags=xs.MATCOPY_FLAG_ZERO_SOURCE, prefetch=1)
    raw = C.string_at(C.byref(blob), 64)
    assert d and (u32(raw, 0), u32(raw, 4), u32(raw, 8), u32(raw, 12)) == (10, 7, 18, 22)  # m, n, ldi, ldo
    assert tuple(raw[16:20]) == (4, 2, 1, 1) and not any(raw[20:])                        # typesize, unroll_level, prefetch, flags
    for unroll, want in ((0, 2), (-3, 2), (5, 5), (64, 64), (1000, 64)):
        blob, d = xs.mcopy_descriptor(4, 3, 3, 3, 3, unroll=unroll)
        assert C.string_at(C.byref(blob), 20)[17] == want
    blob, d = xs.mcopy_descriptor(12, 2, 3, 4, 5)
    raw = C.string_at(C.byref(blob), 20)
    assert (u32(raw, 0), u32(raw, 4), u32(raw, 8), u32(raw, 12), raw[16]) == (6, 3, 15, 12, 4)
    # NULL rules
    assert not L.libxsmm_dispatch_mcopy(None) and not L.libxsmm_dispatch_trans(None)
    assert not L.libxsmm_trans_descriptor_init(None, 4, 1, 1, 1)


def test_dispatch_info_kind_release(xs):
    L = xs.lib()
    keep = []  # (a descriptor lives in its blob)

    def tdesc(*args):
        keep.append(xs.trans_descriptor(*args))
        return keep[-1][1]

    def mdesc(*args, **kwargs):
        keep.append(xs.mcopy_descriptor(*args, **kwargs))
        return keep[-1][1]
    d = tdesc(4, 13, 17, 20)
    f = xs.trans_dispatch(d)
    assert f and f == xs.trans_dispatch(tdesc(4, 13, 17, 20))
    assert xs.trans_dispatch(tdesc(4, 13, 17, 21)) != f
    assert not xs.trans_dispatch(tdesc(4, 13, 17, 16))  # ldo < n
    assert not xs.trans_dispatch(tdesc(4, 0, 17, 17))
    dm = mdesc(8, 6, 9, 8, 7, prefetch=1)
    g = xs.mcopy_dispatch(dm)
    assert g and g != f and g == xs.mcopy_dispatch(mdesc(8, 6, 9, 8, 7, prefetch=1))
    gz = xs.mcopy_dispatch(mdesc(8, 6, 9, 8, 0, flags=1))  # zero source: ldi does not matter
    assert gz and gz != g
    assert not xs.mcopy_dispatch(mdesc(8, 6, 9, 5, 7))   # ldo < m
    assert not xs.mcopy_dispatch(mdesc(8, 6, 9, 8, 5))   # ldi < m
    kind = C.c_int(-1)
    assert 0 == L.libxsmm_get_kernel_kind(g, C.byref(kind)) and kind.value == 1 == xs.KIND_MCOPY
    assert 0 == L.libxsmm_get_kernel_kind(f, C.byref(kind)) and kind.value == 2 == xs.KIND_TRANS
    ti, mi, size = xs.TransKernelInfo(), xs.McopyKernelInfo(), C.c_size_t(0)
    assert 0 == L.libxsmm_get_transkernel_info(f, C.byref(ti), C.byref(size)) and size.value > 0
    assert (ti.typesize, ti.m, ti.n, ti.ldo) == (4, 13, 17, 20)
    assert 0 == L.libxsmm_get_mcopykernel_info(g, C.byref(mi), None)
    assert (mi.typesize, mi.m, mi.n, mi.ldi, mi.ldo, mi.prefetch, mi.flags) == (4, 12, 9, 14, 16, 1, 0)  # the normalised values
    assert 0 == L.libxsmm_get_mcopykernel_info(gz, C.byref(mi), None) and mi.flags == 1
    # the wrong kind of kernel, and nothing to fill
    assert 0 != L.libxsmm_get_transkernel_info(g, C.byref(ti), None) and 0 != L.libxsmm_get_mcopykernel_info(f, C.byref(mi), None)
    assert 0 != L.libxsmm_get_transkernel_info(f, None, None)
    mm = xs.MMKernelInfo()
    assert 0 != L.libxsmm_get_mmkernel_info(f, C.byref(mm), None)
    smm = L.libxsmm_smmdispatch(8, 8, 8, None, None, None, None, None, None, None)
    assert 0 != L.libxsmm_get_transkernel_info(smm, C.byref(ti), None)
    L.libxsmm_release_kernel(f); L.libxsmm_release_kernel(g)  # registered kernels: a fresh dispatch finds them (reference: warning only)
    assert xs.trans_dispatch(d) == f and xs.mcopy_dispatch(dm) == g
    assert 0 == L.libxsmm_get_kernel_kind(f, C.byref(kind)) and kind.value == 2


CALLER = r'''
#include <libxsmm.h>
#include <libxsmm_amd.h>
int main(int argc, char* argv[]) {
  libxsmm_descriptor_blob blob; libxsmm_transkernel_info ti; libxsmm_mcopykernel_info mi; libxsmm_kernel_kind kind;
  const libxsmm_trans_descriptor* td; const libxsmm_mcopy_descriptor* md;
  libxsmm_xtransfunction tf; libxsmm_xmcopyfunction mf;
  double a[6], b[6]; void* po[1]; const void* pi[1]; int r = 0; const int unroll = 4;
  (void)argv;
  td = libxsmm_trans_descriptor_init(&blob, 8, 2, 3, 3); tf = libxsmm_dispatch_trans(td);
  md = libxsmm_mcopy_descriptor_init(&blob, 8, 2, 3, 2, 2, LIBXSMM_MATCOPY_FLAG_ZERO_SOURCE, 0, &unroll); mf = libxsmm_dispatch_mcopy(md);
  if (NULL == tf || NULL == mf) return 1;
  if (EXIT_SUCCESS != libxsmm_get_transkernel_info(tf, &ti, NULL) || 2 != ti.m || 3 != ti.n || 3 != ti.ldo || 8 != ti.typesize) return 2;
  if (EXIT_SUCCESS != libxsmm_get_mcopykernel_info(mf, &mi, NULL) || 4 != mi.m || 4 != mi.typesize || 1 != mi.flags) return 3;
  if (EXIT_SUCCESS != libxsmm_get_kernel_kind((const void*)mf, &kind) || LIBXSMM_KERNEL_KIND_MCOPY != kind) return 4;
  if (EXIT_SUCCESS != libxsmm_get_kernel_kind((const void*)tf, &kind) || LIBXSMM_KERNEL_KIND_TRANS != kind) return 5;
  if (1 < argc) { /* never taken by the test: the calls only have to link */
    po[0] = b; pi[0] = a;
    libxsmm_matcopy(b, a, 8, 2, 3, 2, 2, NULL); libxsmm_matcopy_thread(b, a, 8, 2, 3, 2, 2, NULL, 0, 1); libxsmm_matcopy_omp(b, a, 8, 2, 3, 2, 2, NULL);
    libxsmm_otrans(b, a, 8, 2, 3, 2, 3); libxsmm_otrans_thread(b, a, 8, 2, 3, 2, 3, 0, 1); libxsmm_otrans_omp(b, a, 8, 2, 3, 2, 3);
    libxsmm_itrans(a, 8, 2, 2, 2);
    r += libxsmm_amd_matcopy_batch(b, a, 8, 2, 3, 2, 2, 6, 6, 1) + libxsmm_amd_otrans_batch(b, a, 8, 2, 3, 2, 3, 6, 6, 1);
    r += libxsmm_amd_matcopy_batch_ptr(po, pi, 8, 2, 3, 2, 2, 1) + libxsmm_amd_otrans_batch_ptr(po, pi, 8, 2, 3, 2, 3, 1);
    { const unsigned int ldi = 2, ldo = 3; tf(a, &ldi, b, &ldo); mf(NULL, &ldi, b, &ldo, a); }
  }
  libxsmm_release_kernel((const void*)tf);
  return r;
}
'''


def test_header_is_c89_and_cxx_and_a_c_caller_links(xs, tmp_path):
    src = tmp_path / "xcopy_abi.c"
    src.write_text(CALLER)
    libdir = os.path.dirname(xs.LIB_PATH)
    link = ["-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, lang in (("gcc", "-std=c89", "c"), ("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        exe = tmp_path / ("xcopy_abi_%s_%s" % (cc, std[5:]))
        res = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic" if lang == "c++" else "-Wno-long-long", "-I", os.path.join(ROOT, "include"), "-x", lang, str(src),
                              "-o", str(exe)] + link, capture_output=True, text=True)
        assert res.returncode == 0, (cc, std, res.stderr[-3000:])
        assert subprocess.run([str(exe)]).returncode == 0


def invalid_calls(xs):
    """(entry point, call) for every invalid-argument case; every buffer a canary-filled Stack the call must leave alone"""
    a, b = xc.Stack(4, 8, 8, ld=10), xc.Stack(4, 8, 8, ld=10)
    pa, pb = a.ptr(), b.ptr()
    cases = []
    for name, extra in (("matcopy", {}), ("matcopy_omp", {"omp": True}), ("matcopy_thread", {"tid": 0, "nthreads": 1})):
        mc = lambda out, inp, ts, m, n, ldi, ldo, extra=extra: xs.matcopy(out, inp, ts, m, n, ldi, ldo, **extra)
        cases += [(name, lambda mc=mc: mc(pb, pa, 0, 8, 8, 10, 10)),     # typesize
                  (name, lambda mc=mc: mc(pb, pa, 4, 8, 8, 7, 10)),      # m > ldi
                  (name, lambda mc=mc: mc(pb, pa, 4, 8, 8, 10, 7)),      # m > ldo
                  (name, lambda mc=mc: mc(pb, pb, 4, 8, 8, 10, 10)),     # out == in
                  (name, lambda mc=mc: mc(None, pa, 4, 8, 8, 10, 10)),   # out NULL
                  (name, lambda mc=mc: mc(pb, pa, 4, 8, 0, 10, 10)),     # one extent zero
                  (name, lambda mc=mc: mc(pb, pa, 4, -1, 8, 10, 10))]
    cases += [("matcopy_thread", lambda: xs.matcopy(pb, pa, 4, 8, 8, 10, 10, tid=-1, nthreads=2)),
              ("matcopy_thread", lambda: xs.matcopy(pb, pa, 4, 8, 8, 10, 10, tid=2, nthreads=2)),
              ("matcopy_thread", lambda: xs.matcopy(pb, pa, 4, 8, 8, 10, 10, tid=0, nthreads=0))]
    for name, extra in (("otrans", {}), ("otrans_omp", {"omp": True}), ("otrans_thread", {"tid": 0, "nthreads": 1})):
        ot = lambda out, inp, ts, m, n, ldi, ldo, extra=extra: xs.otrans(out, inp, ts, m, n, ldi, ldo, **extra)
        cases += [(name, lambda ot=ot: ot(pb, pa, 0, 8, 8, 10, 10)),
                  (name, lambda ot=ot: ot(pb, pa, 4, 8, 6, 7, 10)),      # m > ldi
                  (name, lambda ot=ot: ot(pb, pa, 4, 6, 8, 10, 7)),      # n > ldo (m <= ldo would pass a wrong check)
                  (name, lambda ot=ot: ot(None, pa, 4, 8, 8, 10, 10)),
                  (name, lambda ot=ot: ot(pb, None, 4, 8, 8, 10, 10)),
                  (name, lambda ot=ot: ot(pb, pa, 4, 0, 8, 10, 10)),
                  (name, lambda ot=ot: ot(pb, pb, 4, 8, 8, 10, 9)),      # in place with ldi != ldo
                  (name, lambda ot=ot: ot(pb, pb, 4, 8, 6, 10, 10))]     # in place, not square
    cases += [("otrans_thread", lambda: xs.otrans(pb, pa, 4, 8, 8, 10, 10, tid=3, nthreads=3)),
              ("otrans_thread", lambda: xs.otrans(pb, pa, 4, 8, 8, 10, 10, tid=-1, nthreads=3))]
    cases += [("itrans", lambda: xs.itrans(None, 4, 8, 8, 10)), ("itrans", lambda: xs.itrans(pb, 4, 8, 6, 10)), ("itrans", lambda: xs.itrans(pb, 4, 6, 8, 10))]
    return a, b, cases


def silent_calls(xs, a, b):
    """valid calls that move nothing: m == n == 0 (also with NULL operands); none may probe the device or print"""
    pa, pb = a.ptr(), b.ptr()
    xs.matcopy(pb, pa, 4, 0, 0, 10, 10); xs.matcopy(None, None, 4, 0, 0, 0, 0); xs.matcopy(None, pa, 4, 0, 0, 0, 0, tid=1, nthreads=2)
    xs.otrans(pb, pa, 4, 0, 0, 10, 10); xs.otrans(None, None, 4, 0, 0, 0, 0); xs.otrans(None, None, 4, 0, 0, 0, 0, omp=True)
    xs.itrans(pb, 4, 0, 0, 10); xs.itrans(pb, 4, 1, 1, 10)


def run_invalid(xs):
    a, b, cases = invalid_calls(xs)
    a0, b0 = a.host.copy(), b.host.copy()
    for _ in range(2):  # (a second round must not print again)
        for name, call in cases:
            call()
            assert np.array_equal(a.host, a0) and np.array_equal(b.host, b0), name
    silent_calls(xs, a, b)
    L = xs.lib()
    assert L.libxsmm_amd_matcopy_batch(b.ptr(), a.ptr(), 4, 8, 8, 10, 10, 80, 80, -1) != 0      # negative batch
    assert L.libxsmm_amd_matcopy_batch(b.ptr(), a.ptr(), 4, 8, 8, 7, 10, 80, 80, 1) != 0       # m > ldi
    assert L.libxsmm_amd_otrans_batch(b.ptr(), a.ptr(), 4, 6, 8, 10, 7, 80, 80, 1) != 0        # n > ldo
    assert L.libxsmm_amd_otrans_batch(b.ptr(), a.ptr(), 4, 8, 8, 10, 10, 80, 77, 2) != 0       # items of out would overlap
    assert L.libxsmm_amd_otrans_batch(b.ptr(), b.ptr(), 4, 8, 6, 10, 10, 80, 80, 1) != 0       # in place, not square
    assert L.libxsmm_amd_otrans_batch(None, a.ptr(), 4, 8, 8, 10, 10, 80, 80, 1) != 0
    assert L.libxsmm_amd_otrans_batch_ptr(None, None, 4, 8, 8, 10, 10, 1) != 0
    assert L.libxsmm_amd_matcopy_batch_ptr(None, None, 0, 8, 8, 10, 10, 1) != 0
    assert L.libxsmm_amd_matcopy_batch(b.ptr(), a.ptr(), 4, 8, 8, 10, 10, 80, 80, 0) == 0       # batch == 0: nothing to do
    assert L.libxsmm_amd_otrans_batch_ptr(None, None, 4, 8, 8, 10, 10, 0) == 0
    assert np.array_equal(a.host, a0) and np.array_equal(b.host, b0)
    return sorted({name for name, _ in cases})


def test_invalid_arguments_write_nothing_and_are_quiet(xs, capfd):
    xs.lib().libxsmm_set_verbosity(0)
    run_invalid(xs)
    cap = capfd.readouterr()
    assert cap.err == "" and cap.out == ""


def test_invalid_arguments_print_one_line_per_entry_point_when_verbose(xs):
    """in a child process (the once-per-process flags are fresh there): LIBXSMM_VERBOSE=1, every invalid case twice"""
    code = ("import sys, importlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_xcopy_cpu as t\n"
            "xs = importlib.import_module('libxsmm-1_amd'); xs.lib()\n"
            "assert xs.lib().libxsmm_get_verbosity() == 1\n"
            "names = t.run_invalid(xs)\n"
            "sys.stderr.flush(); print('ENTRY_POINTS', len(names))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, LIBXSMM_VERBOSE="1")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ENTRY_POINTS 7" in res.stdout
    lines = [l for l in res.stderr.splitlines() if l.startswith("LIBXSMM ERROR")]
    assert len(lines) == 7, res.stderr
    assert "requires a HIP device" not in res.stderr and "FATAL" not in res.stderr  # the checks come before any device probe
    assert sum("matrix-copy" in l for l in lines) == 3 and sum("transpose" in l for l in lines) == 4


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "samples")), reason="the reference tree is only mounted in the build container")
def test_reference_xcopy_sources_compile_and_link_unchanged(xs, tmp_path):
    """The reference's own tests/matcopy.c, tests/otrans.c, samples/transpose and samples/matcopy, read in place (never copied,
    never run here: they need the GPU), compile against include/libxsmm.h and link against libxsmm.so."""
    libdir = os.path.dirname(xs.LIB_PATH)
    link = ["-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    jobs = [(["gcc", "-std=gnu99"], "tests/matcopy.c"), (["gcc", "-std=gnu99"], "tests/otrans.c"),
            (["gcc", "-std=gnu99"], "samples/transpose/transpose.c"), (["gcc", "-std=gnu99"], "samples/matcopy/matcopy.c")]
    for cc, rel in jobs:
        path = os.path.join(REFERENCE, rel)
        assert os.path.exists(path), path
        out = tmp_path / os.path.basename(rel).split(".")[0]
        res = subprocess.run(cc + ["-O0", "-fopenmp", "-Werror=implicit-function-declaration", "-I", os.path.join(ROOT, "include"), path, "-o", str(out)] + link,
                             capture_output=True, text=True)
        assert res.returncode == 0, (rel, res.stderr[-3000:])


def test_example_compiles(xs, tmp_path):
    """examples/xcopy_caller.c is written against the reference API only and compiles warning-free (it runs in the GPU suite)"""
    text = open(os.path.join(ROOT, "examples", "xcopy_caller.c")).read()
    assert "libxsmm_amd" not in text
    libdir = os.path.dirname(xs.LIB_PATH)
    res = subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "xcopy_caller.c"),
                          "-o", str(tmp_path / "xcopy_caller"), "-L", libdir, "-lxsmm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
