"""Every link of every launch chain of tests/launch_plans.py, run alone on the GPU.

In the product's default configuration the compiler works on a helper thread, so a descriptor is served by whichever alternative
of its plan happens to be ready -- the second, third or fourth included; the rest of the suite compiles in the calling thread and
only ever runs the first. Here XSMM_SMMJIT_SKIP masks the links in front of the one under test (LIBXSMM_AMD_JIT=0 leaves the
generic kernel). Each run asserts the kernel's name, the number of generated kernels launched, and the whole C array -- results,
gaps of the leading dimensions, untouched blocks and 64 canary elements on either side -- bit for bit against the oracle's fma
chain (16-bit inputs: the gold loops); A and B must come back untouched. Every batch here has a defined order of its sums (runs
are walked in batch order; relaxed batches are only cut into segments from 16 items per run on), so nothing is held to a bound."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import launch_plans as lp
from lowp_gemm_common import pairs_gold
from test_lowp import _bf16

pytestmark = pytest.mark.gpu

CANARY = 64
DURATIONS = {}


def _bits(x):
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


class Batch:
    """the operands of a case in host memory, the expected C (computed once per case), and the call"""
    def __init__(self, xs, orc, name):
        c = self.case = lp.CASES[name]
        self.xs = xs
        m, n, k, batch = c["m"], c["n"], c["k"], c["batch"]
        lda, ldb, ldc = lp.leading_dimensions(c)
        sa, sb, sc = lp.item_sizes(c)
        rng = np.random.default_rng(sum(map(ord, name)))
        lens = lp.run_lengths(c) if (c["kind"] == "index" or c["cpat"] == "one") else [1] * batch
        nblocks = len(lens) + 2  # (two blocks of C that no item names stay as they are)
        owners = np.sort(rng.choice(np.arange(nblocks), size=len(lens), replace=False))
        self.cidx = np.repeat(owners, lens) if c["kind"] == "index" else None
        if c["kind"] != "index":
            nblocks = 1 if c["cpat"] == "one" else batch
        if c["lowp"]:
            if c["lowp"] == 1:
                self.a = rng.integers(-300, 300, batch * sa).astype(np.int16).view(np.uint16); self.b = rng.integers(-300, 300, batch * sb).astype(np.int16).view(np.uint16)
                cin = rng.integers(-1000, 1000, nblocks * sc).astype(np.int32)
            else:
                self.a = _bf16(rng.uniform(-1, 1, batch * sa)); self.b = _bf16(rng.uniform(-1, 1, batch * sb))
                cin = rng.uniform(-1, 1, nblocks * sc).astype(np.float32) if c["lowp"] == 3 else _bf16(rng.uniform(-1, 1, nblocks * sc))
        else:
            dtype = np.float64 if c["prec"] == "f64" else np.float32
            self.a = rng.uniform(-1, 1, batch * sa).astype(dtype); self.b = rng.uniform(-1, 1, batch * sb).astype(dtype)
            cin = rng.uniform(-1, 1, nblocks * sc).astype(dtype)
        self.c = np.concatenate([np.full(CANARY, 3, cin.dtype), cin, np.full(CANARY, 5, cin.dtype)])
        self.ref = self.c.copy()
        inner = self.ref[CANARY:CANARY + len(cin)]
        flags = orc.FLAG_TRANS_B if c["transb"] else 0
        if c["lowp"]:
            for i in range(batch):
                inner[i * sc:i * sc + m * n] = pairs_gold(lp.LOWP_GOLD[c["lowp"]], 0, m, n, k, m, k, m, self.a[i * sa:i * sa + m * k], self.b[i * sb:i * sb + k * n],
                                                          inner[i * sc:i * sc + m * n], 1.0)
        elif c["kind"] == "index":
            self.ia = (rng.permutation(batch) * sa).astype(np.int32); self.ib = (rng.permutation(batch) * sb).astype(np.int32)
            self.ic = None if c["cpat"] == "one" else (self.cidx * sc).astype(np.int32)
            assert 0 == orc.gemm_batch_idx(orc.FMA, flags, m, n, k, lda, ldb, ldc, self.a, self.b, inner, 0, self.ia, self.ib, self.ic, batch)
        else:
            orc.gemm_batch_strided(orc.FMA, flags, m, n, k, lda, ldb, ldc, self.a, self.b, inner, sa, sb, 0 if c["cpat"] == "one" else sc, batch, 1)
        assert not np.array_equal(_bits(self.ref), _bits(self.c))
        L = xs.lib()
        self.blob = xs.DescriptorBlob()
        if c["lowp"]:
            L.libxsmm_gemm_descriptor_dinit2.restype = C.c_void_p
            L.libxsmm_gemm_descriptor_dinit2.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_double, C.c_double, C.c_int, C.c_int]
            ip, op = {1: (xs.I16, xs.I32), 3: (xs.BF16, xs.F32), 4: (xs.BF16, xs.BF16)}[c["lowp"]]
            self.desc = L.libxsmm_gemm_descriptor_dinit2(C.byref(self.blob), ip, op, m, n, k, m, k, m, 1.0, 1.0, 0, 0)
        else:
            self.prec = xs.F64 if c["prec"] == "f64" else xs.F32
            self.desc = L.libxsmm_gemm_descriptor_dinit(C.byref(self.blob), self.prec, m, n, k, lda, ldb, ldc, 1.0, 1.0, xs.FLAG_TRANS_B if c["transb"] else 0, 0)
        assert self.desc
        self.dev = None

    def call(self, torch):
        """one batch call on a fresh copy of C; returns (kernel name, generated kernels launched, C from the device, A and B untouched)"""
        xs, c, L = self.xs, self.case, self.xs.lib()

        def up(x):
            return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda()
        if self.dev is None:
            self.dev = (up(self.a), up(self.b))
        da, db = self.dev
        dc = up(self.c)
        pc = dc.data_ptr() + CANARY * self.c.dtype.itemsize
        assert 0 == pc % 16 and 0 == da.data_ptr() % 16 and 0 == db.data_ptr() % 16  # (the plans of the table are those of aligned operands)
        sa, sb, sc = lp.item_sizes(c)
        lda, ldb, ldc = lp.leading_dimensions(c)
        torch.cuda.synchronize()
        before = L.libxsmm_amd_jit_launch_count(), L.libxsmm_amd_launch_count()
        if c["kind"] == "index":
            xs.gemm_batch(self.prec, "N", "T" if c["transb"] else "N", c["m"], c["n"], c["k"], 1.0, da, lda, db, ldb, 1.0, pc, ldc, 0, 4, self.ia, self.ib, self.ic,
                          c["batch"], omp=c["relaxed"])
        else:
            assert 0 == L.libxsmm_amd_gemm_batch_strided(C.c_void_p(self.desc), da.data_ptr(), db.data_ptr(), pc, sa, sb, 0 if c["cpat"] == "one" else sc, c["batch"])
        name = xs.last_kernel()
        torch.cuda.synchronize()
        assert 1 == L.libxsmm_amd_launch_count() - before[1]
        got = dc.cpu().numpy()
        got = got.view(np.uint16) if self.c.dtype == np.uint16 else got
        clean = np.array_equal(_bits(da.cpu().numpy()), _bits(self.a)) and np.array_equal(_bits(db.cpu().numpy()), _bits(self.b))
        return name, L.libxsmm_amd_jit_launch_count() - before[0], got, clean


_batches = {}


def _batch(xs, orc, name):
    if name not in _batches:
        _batches.clear()  # (the cases come one after the other: one set of operands at a time)
        _batches[name] = Batch(xs, orc, name)
    return _batches[name]


LINKS = [(name, i) for name in sorted(lp.CASES) for i in range(len(lp.CASES[name]["chain"]))]


@pytest.mark.parametrize("name,index", LINKS, ids=["%s-%s" % (name, lp.CASES[name]["chain"][i][0]) for name, i in LINKS])
def test_link_alone(xs, orc, torch_gpu, name, index):
    case = lp.CASES[name]
    link, kernel, launches = case["chain"][index]
    mask = 0
    for before, _, _ in case["chain"][:index]:
        mask |= lp.SKIP_SPECIAL if before == "special" else (1 << before if isinstance(before, int) else 0)
    if link == "generic":
        mask = lp.SKIP_SPECIAL  # (no plan at all: the hand-written kernels are the only link in front)
    batch = _batch(xs, orc, name)
    old = xs.lib().libxsmm_amd_set_mfma(case["mfma"])
    t0 = time.perf_counter()
    try:
        with lp.environment(LIBXSMM_AMD_JIT_MINBATCH=1, XSMM_SMMJIT_SKIP=mask, LIBXSMM_AMD_JIT=0 if link == "generic" else None):
            got_name, got_launches, got, clean = batch.call(torch_gpu)
    finally:
        xs.lib().libxsmm_amd_set_mfma(old)
    DURATIONS[(name, link)] = time.perf_counter() - t0
    print("%s %s: %s, %d generated kernels, %.2f s" % (name, link, got_name, got_launches, DURATIONS[(name, link)]))
    assert got_name == kernel, (got_name, kernel, mask)
    assert got_launches == launches, (got_launches, launches)
    wrong = np.flatnonzero(_bits(got) != _bits(batch.ref))
    assert 0 == len(wrong), (name, link, got_name, len(wrong), wrong[:8] - CANARY)
    assert clean, "A or B was written"


def test_mask_unset_or_zero_changes_nothing(xs, orc, torch_gpu):
    """XSMM_SMMJIT_SKIP unset and 0: the first link serves; a bit beyond the plan's length masks nothing"""
    name = "device_wg_nines_strict_f64"
    batch = _batch(xs, orc, name)
    first = lp.CASES[name]["chain"][0]
    old = xs.lib().libxsmm_amd_set_mfma(1)
    try:
        for mask in (None, 0, 1 << 7):
            with lp.environment(LIBXSMM_AMD_JIT_MINBATCH=1, XSMM_SMMJIT_SKIP=mask, LIBXSMM_AMD_JIT=None):
                got_name, got_launches, got, clean = batch.call(torch_gpu)
            assert (got_name, got_launches) == first[1:], (mask, got_name)
            assert np.array_equal(_bits(got), _bits(batch.ref)) and clean
    finally:
        xs.lib().libxsmm_amd_set_mfma(old)


CHILD = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import oracle_binding as orc
import launch_plans as lp
xs = importlib.import_module("libxsmm-1_amd")
L = xs.lib()
torch.cuda.set_device(0)
L.libxsmm_amd_set_mfma(1)
case = lp.CASES["device_wg_nines_strict_f64"]
m, n, k, batch = case["m"], case["n"], case["k"], case["batch"]
rng = np.random.default_rng(40)
lens = lp.run_lengths(case)
a = rng.uniform(-1, 1, batch * m * k); b = rng.uniform(-1, 1, batch * k * n); c = rng.uniform(-1, 1, len(lens) * m * n)
sa = (rng.permutation(batch) * m * k).astype(np.int32); sb = (rng.permutation(batch) * k * n).astype(np.int32)
sc = (np.repeat(np.arange(len(lens)), lens) * m * n).astype(np.int32)
ref = c.copy(); assert 0 == orc.gemm_batch_idx(orc.FMA, 0, m, n, k, m, k, m, a, b, ref, 0, sa, sb, sc, batch)
da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
outs, names = [], []
def call():
    before = L.libxsmm_amd_jit_launch_count()
    dc = torch.from_numpy(c).cuda()
    xs.gemm_batch(xs.F64, "N", "N", m, n, k, 1.0, da, m, db, k, 1.0, dc, m, 0, 4, sa, sb, sc, batch)
    names.append("%s:%d" % (xs.last_kernel(), L.libxsmm_amd_jit_launch_count() - before)); outs.append(dc)
for it in range(40):
    call()
L.libxsmm_amd_jit_wait()
call()
torch.cuda.synchronize()
bad = [i for i, dc in enumerate(outs) if not np.array_equal(dc.cpu().numpy().view(np.uint64), ref.view(np.uint64))]
print("RESULT", len(bad), " ".join(names))
'''


def test_product_defaults_serve_from_later_alternatives_meanwhile(xs, torch_gpu, tmp_path):
    """A fresh process with the product's defaults (the compiler on its helper thread, an empty code-object cache) makes the fp64 32^3
    index-batch call with runs 40 times without waiting: every result is the oracle's, the kernels that serve never move back in the
    chain, and after libxsmm_amd_jit_wait the first alternative serves."""
    case = lp.CASES["device_wg_nines_strict_f64"]
    position = {(kernel, launches): i for i, (link, kernel, launches) in enumerate(case["chain"])}
    env = dict(os.environ)
    for key in ("LIBXSMM_AMD_JIT_ASYNC", "LIBXSMM_AMD_JIT_MINBATCH", "LIBXSMM_AMD_JIT", "XSMM_SMMJIT_SKIP"):
        env.pop(key, None)
    env["LIBXSMM_AMD_CACHE"] = str(tmp_path / "cold_cache")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, root], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    words = [l for l in res.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert "0" == words[1], words
    served = [position[(w.rsplit(":", 1)[0], int(w.rsplit(":", 1)[1]))] for w in words[2:]]
    print("positions in the chain:", served)
    assert 41 == len(served)
    assert all(x >= y for x, y in zip(served[:40], served[1:40])), served  # towards the front of the plan only
    assert 0 == served[40], served
