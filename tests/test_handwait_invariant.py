"""Hand-counted waits of the matrix-core run form: an invariant of the code objects, checked without a GPU.

The run form (csrc/kernels/smm_jit_mfma_runs.inc, XHANDWAIT 1) issues its operand loads as inline assembly and waits for them with
`s_waitcnt vmcnt(N)`, N a constant of the pipeline. Those counts hold only while the body's vector-memory traffic is exactly
the loads the pipeline accounts for: no FLAT access (FLAT instructions retire out of order with the others), no scratch
(spills, or a table entry kept in the private segment and read through a generic pointer). So: whenever the text the
library actually builds (compile == 2 of the *_kernel_source functions: after the library's own check of the code object)
holds `XHANDWAIT 1`, its code object has no private segment, no spilled VGPRs and no flat or scratch instruction.
SGPR spills are allowed: they go to VGPR lanes, not to memory.
"""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TRANS_B = 2  # LIBXSMM_GEMM_FLAG_TRANS_B

CP2K = [[m, n, k] for m in (13, 23, 32) for n in (13, 23, 32) for k in (13, 23, 32)]
# a group: [m, n, k, flags, ldb] (ldb 0: tight)
SETS = {
    "eligible": [[13, 13, 13, 0, 0], [32, 32, 32, 0, 0]],
    "nn_nt": [[13, 13, 13, 0, 0], [32, 32, 32, 0, 0], [23, 23, 23, TRANS_B, 0]],
    "nn_wide_ldb": [[13, 13, 13, 0, 0], [32, 32, 32, 0, 100]],  # B span 100 * 31 + 32 > 2560: not the run form
    "cp2k": [s + [0, 0] for s in CP2K],
    "cp2k_nt": [s + [0, 0] for s in CP2K] + [[23, 23, 23, TRANS_B, 0]],
}
# sha256 of the generated text of the all-eligible sets (the fast path of the CP2K configuration): must not change silently
ELIGIBLE_TEXT = {
    ("eligible", 8): "e0ceebacd680c2ae54a123da2ed236b0420d64943e4b05813965a70f98f6379c",
    ("eligible", 4): "fa2c7ca01e814b49e11b1ded4796df2d97da4f662bb1cb05d60026eb89ac03ac",
    ("cp2k", 8): "0ccb1517e726b5ec8a2f1b6bc7a3af051542c3fb1e19d9ed7ec6d09740b6df1d",
    ("cp2k", 4): "069b804152ac4dbc91c8a873dc7cfea89f47765db96e38ed4f026f5aa4511d01",
}
# single-shape run / streaming forms (variant 1|2|65536 resp. 1|65536): [typesize, m, n, k, ldb]
SINGLE = [[8, 32, 32, 64, 0], [8, 32, 32, 32, 0], [8, 32, 32, 64, 80], [8, 13, 13, 13, 0], [8, 32, 16, 64, 0], [8, 5, 7, 3, 0],
          [4, 32, 32, 64, 0], [4, 32, 32, 64, 80]]

# the library's side of a case, in this process or in a child (the knobs are read once into statics)
_CHILD = r"""
import ctypes as C, importlib, json, sys
sys.path[:0] = [%(root)r]
xs = importlib.import_module("libxsmm-1_amd")
from test_handwait_invariant import built_texts
json.dump(built_texts(xs, json.loads(sys.argv[1])), open(sys.argv[2], "w"))
"""


def _descriptors(xs, typesize, groups):
    prec = xs.F64 if typesize == 8 else xs.F32
    keep, arr = [], (C.c_void_p * len(groups))()
    for i, (m, n, k, flags, ldb) in enumerate(groups):
        blob, d = xs.descriptor(prec, m, n, k, ldb=(ldb or None), flags=flags)
        assert d, (m, n, k, flags, ldb)
        keep.append(blob)
        arr[i] = C.cast(d, C.c_void_p)
    return keep, arr


def built_texts(xs, cases):
    """cases: [[kind, typesize, groups]] -> [[rc, generated text, text the library builds]] (kind "grouped" or "runs"/"stream")"""
    L = xs.lib()
    out = []
    for kind, typesize, groups in cases:
        buf = C.create_string_buffer(1 << 23)
        if kind == "grouped":
            keep, arr = _descriptors(xs, typesize, groups)
            call = lambda compile: L.libxsmm_amd_smm_grouped_kernel_source(arr, len(groups), buf, len(buf), compile)
        else:
            keep, arr = _descriptors(xs, typesize, groups)
            variant = 65536 | 1 | (2 if kind == "runs" else 0)
            call = lambda compile: L.libxsmm_amd_smm_kernel_source(C.c_void_p(arr[0]), variant, buf, len(buf), compile)
        n = call(0)
        gen = buf.value.decode()
        assert n == len(gen), (kind, typesize, groups, n)
        rc = call(2)
        out.append([rc, gen, buf.value.decode()])
    return out


def _code_object_facts(src, work, name):
    """compile `src` as hiprtc would (hip_runtime.h included) for gfx950 -> private segment, spills, flat/scratch counts"""
    hip, asm = os.path.join(work, name + ".hip"), os.path.join(work, name + ".s")
    with open(hip, "w") as f:
        f.write("#include <hip/hip_runtime.h>\n" + src)
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", hip, "-o", asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(asm) as f:
        s = f.read()
    ints = lambda key: [int(x) for x in re.findall(r"\.%s:\s*(\d+)" % key, s)]
    facts = {"private_segment": ints("private_segment_fixed_size"), "vgpr_spill": ints("vgpr_spill_count"),
             "flat": len(re.findall(r"^\s*flat_(?:load|store)", s, re.M)), "scratch": len(re.findall(r"^\s*scratch_", s, re.M))}
    assert facts["private_segment"] and facts["vgpr_spill"], "no kernel metadata in the assembly"
    return facts


def _check_invariant(results, labels, tmp_path):
    """every built text with hand-counted waits compiles to a code object without memory traffic the counts do not know"""
    todo = [(label, built) for label, (rc, gen, built) in zip(labels, results) if "#define XHANDWAIT 1\n" in built]
    for label, (rc, gen, built) in zip(labels, results):
        if rc == -1:
            pytest.skip("libhiprtc is not available here")
        assert rc == 0, label
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        facts = list(pool.map(lambda x: _code_object_facts(x[1], str(tmp_path), re.sub(r"\W+", "_", x[0])), todo))
    bad = [(label, f) for (label, _), f in zip(todo, facts)
           if max(f["private_segment"]) or max(f["vgpr_spill"]) or f["flat"] or f["scratch"]]
    assert not bad, "hand-counted waits next to memory traffic they do not count: %s" % bad
    return len(todo)


def _cases():
    cases, labels = [], []
    for name, groups in SETS.items():
        for typesize in (8, 4):
            cases.append(["grouped", typesize, groups])
            labels.append("%s_f%d" % (name, 8 * typesize))
    return cases, labels


@pytest.fixture(scope="module")
def default_texts(xs):
    cases, labels = _cases()
    return cases, labels, built_texts(xs, cases)


def test_eligible_sets_keep_the_inlined_handwaited_bodies(default_texts):
    """all-eligible sets (every body on the run form): the bodies are force-inlined into a dispatcher without calls and keep
    the hand-counted waits -- the generated text is the one the fast path of the CP2K configuration was measured with, and the
    library builds it unchanged (its code object passes the library's check)"""
    cases, labels, results = default_texts
    for (kind, typesize, groups), label, (rc, gen, built) in zip(cases, labels, results):
        name = label.rsplit("_", 1)[0]
        if (name, typesize) not in ELIGIBLE_TEXT:
            continue
        if rc == -1:
            pytest.skip("libhiprtc is not available here")
        assert "#define XENTRY_ATTR __forceinline__\n" in gen, label
        assert gen.count("#define XHANDWAIT 1\n") == len(groups), label
        assert hashlib.sha256(gen.encode()).hexdigest() == ELIGIBLE_TEXT[(name, typesize)], label
        assert built == gen, label + ": the library's check of the code object dropped the hand-counted waits"


def test_mixed_sets_never_handwait_in_called_bodies(default_texts):
    """one group off the run form (TRANS_B, a B span beyond 2560 elements) turns every body into a called function: none of
    them may keep the hand-counted waits"""
    cases, labels, results = default_texts
    for label, (rc, gen, built) in zip(labels, results):
        if "noinline" in gen:
            handwait, compilers = ("#define XHANDWAIT 1\n" in gen), ("#define XHANDWAIT 0\n" in gen)
            assert not handwait and compilers, label  # (the matrix-core bodies are still there, with the compiler's waits)


def test_grouped_handwait_code_objects(default_texts, tmp_path):
    """the invariant over all sets, fp64 and fp32, default settings"""
    cases, labels, results = default_texts
    assert _check_invariant(results, labels, tmp_path) >= 4  # (at least the all-eligible sets are checked)


def test_single_shape_handwait_code_objects(xs, tmp_path):
    """the run form and the streaming form of one shape (smm_*_mfma_runs_jit, smm_*_mfma_stream_jit)"""
    cases, labels = [], []
    for typesize, m, n, k, ldb in SINGLE:
        for kind in ("runs", "stream"):
            cases.append([kind, typesize, [[m, n, k, 0, ldb]]])
            labels.append("%s_f%d_%dx%dx%d_ldb%d" % (kind, 8 * typesize, m, n, k, ldb))
    results = built_texts(xs, cases)
    assert _check_invariant(results, labels, tmp_path) == len(cases)  # (all of them keep the hand-counted waits)


@pytest.mark.parametrize("knob", ["XSMM_SMMJIT_GROUPED_INLINE=0", "XSMM_SMMJIT_GROUPED_WPE=3", "XSMM_SMMJIT_GROUPED_WPE=4"])
def test_grouped_handwait_code_objects_under_knobs(xs, tmp_path, knob):
    """the developer knobs of the grouped kernel, each in a child process (read once): bodies called instead of inlined, and
    the register bounds of three and four waves per SIMD (the 32^3 fp64 bodies spill there)"""
    cases, labels = _cases()
    key, value = knob.split("=")
    env = dict(os.environ, **{key: value})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = tmp_path / "texts.json"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": os.path.join(ROOT, "tests")}, json.dumps(cases), str(out)],
                       env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-4000:]
    results = json.loads(out.read_text())
    if key == "XSMM_SMMJIT_GROUPED_INLINE":
        assert not any("#define XHANDWAIT 1\n" in gen for rc, gen, built in results)
    _check_invariant(results, labels, tmp_path)
