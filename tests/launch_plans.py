"""The launch chains of dense batches, as the tests of the alternatives assume them.

A batch call walks a chain (csrc/xsmm_batch.cpp:run_smm): the alternatives of the matrix-core tier of its plan, the hand-written
kernels (kernels/smm_special.hip), the alternatives of the specialised tier, the generic kernel; 16-bit inputs: the alternatives of
their plan, then the pre-compiled kernel (kernels/smm_lowp.hip). The first link that is ready serves, "with the same bits". CASES
names batches and, for each, the whole chain: per link which kernel libxsmm_amd_last_kernel names and how many generated kernels
it launches (libxsmm_amd_jit_launch_count; a pre-compiled kernel: 0). A link is an index into the plan (SmmPlan::alts, both tiers
counted), "special", "generic" or "lowp". tests/test_launch_plans_cpu.py holds every chain against the planner
(libxsmm_amd_smm_plan_describe) and fails when the planner offers a class of alternative no case here reaches;
tests/test_plan_alternatives_gpu.py runs every link alone (XSMM_SMMJIT_SKIP masks the links in front of it)."""
import os

SKIP_SPECIAL = 256  # bit of XSMM_SMMJIT_SKIP for the hand-written kernels; bits 0-7: the alternatives by position
PACK_BITS = 7 << 8  # variant bits that hold log2 of the items per wave pass

STRIDED, INDEX, POINTER = 0, 1, 2
SYNC_NONE, SYNC_RUNS, SYNC_ATOMIC, SYNC_DEVICE = 0, 1, 2, 3
LOWP_NAME = {1: "i16i32", 3: "bf16f32", 4: "bf16"}  # the planner's kinds (the oracle's gold loops: 0, 2, 3)
LOWP_GOLD = {1: 0, 3: 2, 4: 3}


def generic_name(prec, m, n):
    mx = max(m, n)
    return "smm_%s_generic_%s" % (prec, "w8" if mx <= 8 else "w16" if mx <= 16 else "w24" if mx <= 24 else "w32" if mx <= 32 else "g48" if mx <= 48 else "g64")


def _case(prec, shape, chain, kind="strided", ld=None, transb=False, batch=37, cpat="distinct", relaxed=False, mfma=1, lowp=0, layout="b2b"):
    m, n, k = shape
    p = "smm_" + prec
    full = []
    for link, kernel, launches in chain:
        if link == "generic":
            kernel = generic_name(prec, m, n)
        elif link == "lowp":
            kernel = "smm_%s_lowp" % LOWP_NAME[lowp]
        elif lowp:
            kernel = "smm_%s_%s" % (LOWP_NAME[lowp], kernel)
        else:
            kernel = p + "_" + kernel
        full.append((link, kernel, launches))
    return dict(prec=prec, m=m, n=n, k=k, ld=ld, transb=transb, kind=kind, batch=batch, cpat=cpat, relaxed=relaxed, mfma=mfma, lowp=lowp,
                layout=layout, chain=full)


def _build():
    cases = {}
    for prec in ("f32", "f64"):
        # matrix-core tier: tight strided aligned items beyond 32 (wide one-wave-per-item form first)
        cases["beyond32_tight_" + prec] = _case(prec, (36, 33, 12), [(0, "mfma_wave_jit", 1), (1, "mfma_wg_jit", 1), ("special", "mfma_wg", 0),
                                                                     (2, "jit_shape_wg", 1), ("generic", None, 0)])
        # ... leading dimensions with gaps: the element-wise wave form; the specialised tier does not take gaps beyond 32
        cases["beyond32_gaps_" + prec] = _case(prec, (43, 9, 27), [(0, "mfma_wave_jit", 1), (1, "mfma_wg_jit", 1), ("special", "mfma_wg", 0), ("generic", None, 0)],
                                               ld=(48, 32, 48))
        # ... B transposed in memory: the wave form alone in its tier, no hand-written kernel
        cases["beyond32_transb_" + prec] = _case(prec, (40, 36, 20), [(0, "mfma_wave_jit", 1), (1, "jit_shape_wg", 1), ("generic", None, 0)], transb=True)
        # long K with small M and N
        cases["long_k_" + prec] = _case(prec, (23, 23, 70), [(0, "mfma_stream_jit", 1), (1, "jit_shape_wg", 1), ("generic", None, 0)])
        # every item its own C: pack * 5 + 3 items, the packed part and the rest as two launches, then one item per wave
        cases["own_c_13_" + prec] = _case(prec, (13, 13, 13), [(0, "jit_shape", 2), (1, "jit_shape", 1), ("generic", None, 0)], batch=(8 if prec == "f32" else 4) * 5 + 3)
        cases["own_c_13_few_" + prec] = _case(prec, (13, 13, 13), [(0, "jit_shape", 1), (1, "jit_shape", 1), ("generic", None, 0)], batch=3)  # fewer than a pack: the rest alone
        cases["own_c_13_gaps_" + prec] = _case(prec, (13, 13, 13), [(0, "mfma_stream_jit", 1), (1, "jit_shape", 1), ("generic", None, 0)], ld=(16, 16, 16), batch=43)
        # one C for the whole batch (the host knows: no index array for C)
        cases["one_c_23_" + prec] = _case(prec, (23, 23, 23), [(0, "mfma_runs_jit", 1), (1, "jit_shape_runs", 1), ("generic", None, 0)], kind="index", cpat="one", batch=40)
        big = (32, 32, 32) if prec == "f64" else (32, 32, 64)  # the smallest shapes whose operands make the work-group form worth it
        cases["one_c_wg_" + prec] = _case(prec, big, [(0, "mfma_runs_jit", 1), (1, "jit_shape_wgruns", 1), (2, "jit_shape_runs", 1), ("generic", None, 0)],
                                          kind="index", cpat="one", batch=40)
        cases["one_c_wg_strided_" + prec] = _case(prec, big, [(0, "mfma_runs_jit", 1), (1, "jit_shape_wgruns", 1), (2, "jit_shape_runs", 1), ("generic", None, 0)],
                                                  cpat="one", batch=40)  # a strided batch whose C does not move: 16-byte accesses
        cases["one_c_wg_nomfma_" + prec] = _case(prec, big, [(0, "jit_shape_wgruns", 1), (1, "jit_shape_runs", 1), ("generic", None, 0)],
                                                 kind="index", cpat="one", batch=40, mfma=0)
        # index batches, the verdict on the device: mixed short runs / runs of 9 / strictly increasing C, strict and relaxed
        for cpat in ("mixed", "nines", "increasing"):
            for relaxed in (False, True):
                if prec == "f32" and cpat != "nines":
                    continue  # (fp32: one pattern per class is enough, the kernel text is the fp64 one)
                tag = "%s_%s_%s" % (cpat, "relaxed" if relaxed else "strict", prec)
                cases["device_wg_" + tag] = _case(prec, big, [(0, "mfma_runs_tiles_jit", 1), (1, "mfma_runs_jit", 1), (2, "jit_shape_runs", 2), (3, "jit_shape_runs", 1),
                                                              ("generic", None, 0)], kind="index", cpat=cpat, relaxed=relaxed, batch=135)
                cases["device_13_" + tag] = _case(prec, (13, 13, 13), [(0, "mfma_runs_jit", 1), (1, "jit_shape_runs", 1), ("generic", None, 0)],
                                                  kind="index", cpat=cpat, relaxed=relaxed, batch=135)
    # fp32 beyond 32: the generated work-group kernel with A and B in 16-byte chunks only, and with the image of C only
    for name, shape in (("beyond32_chunks_f32", (34, 33, 12)), ("beyond32_c_image_f32", (36, 33, 11))):
        cases[name] = _case("f32", shape, [(0, "mfma_wave_jit", 1), (1, "mfma_wg_jit", 1), ("special", "mfma_wg", 0), (2, "jit_shape_wg", 1), ("generic", None, 0)])
    # fp64 items whose images leave no room for four waves per CU: the columns of C in two halves
    cases["beyond32_two_halves_f64"] = _case("f64", (16, 64, 64), [(0, "mfma_wave2_jit", 1), (1, "mfma_wg_jit", 1), ("special", "mfma_wg", 0),
                                                                   (2, "jit_shape_wg", 1), ("generic", None, 0)])
    # 16-bit inputs: back to back (16-byte accesses, small items several per wave pass) and with a stride of their own
    for lowp in (1, 3, 4):
        wave = [(0, "mfma_wave_jit_lowp", 1)] if lowp != 1 else []
        for layout in ("b2b", "strided"):
            cases["lowp_%s_32_%s" % (LOWP_NAME[lowp], layout)] = _case("f32", (32, 32, 32), wave + [(len(wave), "jit_shape_lowp", 1), ("lowp", None, 0)],
                                                                       kind="lowp", lowp=lowp, layout=layout, batch=43)
        cases["lowp_%s_16_b2b" % LOWP_NAME[lowp]] = _case("f32", (16, 16, 16), [(0, "jit_shape_lowp", 2), (1, "jit_shape_lowp", 1), ("lowp", None, 0)],
                                                          kind="lowp", lowp=lowp, batch=43)
        cases["lowp_%s_16_strided" % LOWP_NAME[lowp]] = _case("f32", (16, 16, 16), [(0, "jit_shape_lowp", 1), ("lowp", None, 0)], kind="lowp", lowp=lowp,
                                                              layout="strided", batch=43)
    return cases


CASES = _build()

# Blocked GEMM (csrc/xsmm_blocked.cpp:bgemm_run): the hand-written run kernels, then the specialised tier of the plan of an index batch
# with the verdict on the device, a relaxed order and runs of k / bk items, then the generic kernel. (m, n, k, bm, bn, bk); every
# geometry has fewer than 16 k blocks per C block, so no run is cut into segments: each element of C is one ascending-k fma chain.
BLOCKED_GEOMETRIES = [(256, 192, 320, 32, 32, 32), (256, 128, 384, 64, 64, 64), (192, 192, 192, 48, 24, 16)]


def blocked_chain(prec, geom, mfma):
    bm, bn, bk = geom[3:]
    p = "smm_" + prec + "_"
    last = [("generic", generic_name(prec, bm, bn), 0)]
    if max(bm, bn) > 32:  # the work-group-per-item form with uniform runs; matrix cores: the pre-compiled run form beyond 32
        return ([("special", p + "mfma_wg_runs", 0)] if mfma else []) + [(0, p + "jit_shape_wg", 1)] + last
    assert (bm, bn, bk) == (32, 32, 32)
    runs = [(p + "jit_shape_runs", 2), (p + "jit_shape_runs", 1)] if prec == "f64" else [(p + "jit_shape_runs", 1)]  # (fp32 32^3: too small for the work-group part)
    if mfma:
        runs = [(p + "mfma_runs_tiles_jit", 1), (p + "mfma_runs_jit", 1)] + runs
    head = [("special", "smm_f32_32x32x32_mfma_runs", 0)] if (mfma and prec == "f32") else []
    return head + [(i, kernel, launches) for i, (kernel, launches) in enumerate(runs)] + last


def blocked_items(geom):
    m, n, k, bm, bn, bk = geom
    return (m // bm) * (n // bn) * (k // bk), k // bk


def leading_dimensions(c):
    if c["ld"] is not None:
        return c["ld"]
    return (c["m"], c["n"] if c["transb"] else c["k"], c["m"])


def item_sizes(c):
    """elements from one item to the next (A, B, C)"""
    lda, ldb, ldc = leading_dimensions(c)
    sizes = (lda * c["k"], ldb * (c["k"] if c["transb"] else c["n"]), ldc * c["n"])
    return tuple(s + 8 for s in sizes) if c["layout"] == "strided" else sizes


def run_lengths(c):
    """the lengths of the runs of equal C of an index batch"""
    batch, cpat = c["batch"], c["cpat"]
    if cpat == "one":
        return [batch]
    if cpat == "nines":  # 9 on average: the work-group part of a two-part alternative does the work
        assert 0 == batch % 9
        return [9] * (batch // 9)
    if cpat == "mixed":  # 2 on average: the wave part does the work
        out = []
        while sum(out) < batch:
            out.append(min((1, 2, 3)[len(out) % 3], batch - sum(out)))
        return out
    return [1] * batch


def plan_query(c):
    """keyword arguments of the binding's smm_plan() for the batch of case c (descriptor aside)"""
    if c["kind"] == "index":
        return dict(mode=INDEX, sync=SYNC_RUNS if c["cpat"] == "one" else SYNC_DEVICE, batch=c["batch"], relaxed=c["relaxed"], mfma=c["mfma"])
    sizes = item_sizes(c)
    if c["cpat"] == "one":  # a strided batch whose C does not move
        return dict(mode=STRIDED, sync=SYNC_RUNS, batch=c["batch"], strides=(sizes[0], sizes[1], 0), mfma=c["mfma"])
    return dict(mode=STRIDED, sync=SYNC_NONE, batch=c["batch"], strides=sizes, mfma=c["mfma"], lowp=c["lowp"])


def describe(xs, c):
    lda, ldb, ldc = leading_dimensions(c)
    prec = xs.F64 if c["prec"] == "f64" else xs.F32
    blob, d = xs.descriptor(prec, c["m"], c["n"], c["k"], lda, ldb, ldc, flags=xs.FLAG_TRANS_B if c["transb"] else 0)
    return xs.smm_plan(d, **plan_query(c))


def alt_class(alt):
    """what kind of alternative this is, whatever the shape: tier, name, the variant bits of its parts without the pack count, and
    their slices (the number of parts with them); the tiles of C: their variant bits"""
    return (alt["tier"], alt["name"], tuple((v & ~PACK_BITS, s) for v, s in alt["parts"]), tuple(sorted(set(t[2] for t in alt["tiles"]))))


def launches_of(alt):
    return 1 if alt["tiles"] else len(alt["parts"])


class environment:
    """environment variables for the length of a with block (the knobs of the launch chains are read on every call)"""
    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.values}
        for k, v in self.values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
