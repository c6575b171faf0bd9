"""The grid clamps, slab splits and index-width switches of the launchers in libxsmm-1_amd/csrc, as size tests assume them.

Every entry names the source file, the expressions the threshold comes from (regular expressions; a group is the number a
test assumes, an expression without a group only has to be there), and `per_trip`: the work one full trip of the grid-stride
loop (or one slab, band or launch) covers, in the unit given. tests/test_launch_limits_cpu.py holds every expression against
the sources, so a raised clamp fails there instead of quietly keeping a size test below the second trip. A test that wants to
pass a clamp takes its size from here: sized(name, r) is two full trips and an odd rest that is no multiple of the wave (64)
or of a vector (2, 4), so the third trip is partial and falls on other work-groups than the first."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libxsmm-1_amd", "csrc")

QUANT, MATDIFF, POOL, TILE, SPARSE, GENERIC, LOWP, XCOPY = ("kernels/quant.hip", "kernels/matdiff.hip", "kernels/pool.hip",
    "kernels/tile_gemm.cuh", "kernels/sparse.hip", "kernels/smm_generic.hip", "kernels/smm_lowp.hip", "kernels/xcopy.hip")
CONV = "kernels/conv.hip"
RNN, RNN_HOST = "kernels/rnn.hip", "xsmm_dnn_rnn.cpp"
GRID_FOR = (SPARSE, r"if \(blocks > 256LL \* (\d+)\) blocks = 256LL \* \1;", 32)

LIMITS = {
    # quantise and convert, flat: blocks_for caps the grid; a lane takes four elements per trip
    "quant_flat": dict(derive=lambda v: v[0] * v[1] * v[2], unit="elements", per_trip=2048 * 256 * 4, source=[
        (QUANT, r"constexpr int QUANT_MAX_BLOCKS = (\d+);", 2048), (QUANT, r"constexpr int QUANT_THREADS = (\d+);", 256),
        (QUANT, r"b > QUANT_MAX_BLOCKS \? QUANT_MAX_BLOCKS : b", None), (QUANT, r"blocks_for\(\(n \+ 3\) / (\d+)\)", 4),
        (QUANT, r"for \(long long q = tid; q < nquads; q \+= nthreads\)", None)]),
    # the widening converter lives with the sparse kernels: grid_for(count, 256), one element per lane and trip
    "bf16_widen": dict(derive=lambda v: 256 * v[0] * v[1], unit="elements", per_trip=256 * 32 * 256, source=[
        GRID_FOR, (SPARSE, r"bf16_widen_kernel, dim3\(grid_for\(count, (\d+)\)\), dim3\(256\)", 256)]),
    # quantise, layout kernels: one output per lane and trip, two with `pair`
    "quant_layout_pair": dict(derive=lambda v: v[0] * v[1] * v[2], unit="outputs", per_trip=2048 * 256 * 2, source=[
        (QUANT, r"constexpr int QUANT_MAX_BLOCKS = (\d+);", 2048), (QUANT, r"constexpr int QUANT_THREADS = (\d+);", 256),
        (QUANT, r"blocks_for\(0 != pair \? g\.total / (\d+) : g\.total\)", 2),
        (QUANT, r"width = \(0 != pair \? (\d+) : 1\), step = \(IDX\)gridDim\.x \* QUANT_THREADS \* width", 2)]),
    "quant_layout_single": dict(derive=lambda v: v[0] * v[1] * v[2], unit="outputs", per_trip=2048 * 256, source=[
        (QUANT, r"constexpr int QUANT_MAX_BLOCKS = (\d+);", 2048), (QUANT, r"constexpr int QUANT_THREADS = (\d+);", 256),
        (QUANT, r"blocks_for\(0 != pair \? g\.total / 2 : g\.total\)", None),
        (QUANT, r"width = \(0 != pair \? 2 : (\d+)\), step = \(IDX\)gridDim\.x \* QUANT_THREADS \* width", 1)]),
    # quantise, plain input through LDS: a work-group per tile of 64 pixels x up to 64 channels, the tile reused per trip
    "quant_act_tiled": dict(derive=lambda v: v[0], unit="tiles", per_trip=2048, pixels=64, channels=64, source=[
        (QUANT, r"constexpr int QUANT_MAX_BLOCKS = (\d+);", 2048),
        (QUANT, r"g\.ntiles < QUANT_MAX_BLOCKS \? g\.ntiles : QUANT_MAX_BLOCKS", None),
        (QUANT, r"constexpr int QT_PIX = (\d+), QT_CH = \d+", 64), (QUANT, r"constexpr int QT_PIX = \d+, QT_CH = (\d+)", 64),
        (QUANT, r"for \(long long t = blockIdx\.x; t < g\.ntiles; t \+= gridDim\.x\)", None)]),
    # matdiff, tiled: a tile has 16 lines until nn * nstrips passes 2048 * 16, then 32, 48, ...
    "matdiff_tiles": dict(derive=lambda v: v[0] * v[1], unit="lines x strips", per_trip=2048 * 16, lines=16, strip=256, source=[
        (MATDIFF, r"constexpr int MATDIFF_MAX_BLOCKS = (\d+);", 2048), (MATDIFF, r"constexpr int MATDIFF_LINES = (\d+);", 16),
        (MATDIFF, r"constexpr int MATDIFF_VEC = (\d+);", 4), (MATDIFF, r"constexpr int MATDIFF_STRIP = (\d+) \* MATDIFF_VEC;", 64),
        (MATDIFF, r"long long lines = \(a\.nn \* p\.nstrips \+ MATDIFF_MAX_BLOCKS - 1\) / MATDIFF_MAX_BLOCKS;", None),
        (MATDIFF, r"lines = \(lines \+ MATDIFF_LINES - 1\) / MATDIFF_LINES \* MATDIFF_LINES;", None)]),
    "matdiff_norms": dict(derive=lambda v: v[0] * v[1], unit="lines + columns", per_trip=2048 * 256, source=[
        (MATDIFF, r"constexpr int MATDIFF_MAX_BLOCKS = (\d+);", 2048),
        (MATDIFF, r"constexpr int MATDIFF_THREADS = (\d+);", 256), (MATDIFF, r"const long long lanes = a\.nn \+ a\.mm;", None),
        (MATDIFF, r"matdiff_norms_kernel, dim3\(\(unsigned\)\(nb > MATDIFF_MAX_BLOCKS \? MATDIFF_MAX_BLOCKS : nb\)\)", None)]),
    # pooling: items along gridDim.y, slabs of 32768 of them along gridDim.z
    "pool": dict(derive=lambda v: v[0], unit="items", per_trip=32768, source=[
        (POOL, r"gy = items < (\d+) \? items : \1, gz = \(items \+ gy - 1\) / gy", 32768),
        (POOL, r"\(long long\)g\.w0 \+ blockIdx\.y \+ \(long long\)blockIdx\.z \* gridDim\.y", None)]),
    # convolution: FWD takes 65535 tiles of pixels per launch (gridDim.y) and hands the kernel the first tile of the slab; BWD and
    # UPD take their items as pooling does; the filter transposition wraps its work-groups into rows of 65536
    "conv_fwd_slab": dict(derive=lambda v: v[0], unit="tiles of pixels", per_trip=65535, tiles=(64, 128), source=[
        (CONV, r"constexpr long long SLAB = (\d+);", 65535), (CONV, r"for \(long long j0 = 0; j0 < tiles_j; j0 \+= SLAB\)", None),
        (CONV, r"\(long long\)BT \* \(\(long long\)jtile0 \+ blockIdx\.y\)", None)]),
    "conv_items": dict(derive=lambda v: v[0], unit="items", per_trip=32768, source=[
        (CONV, r"gy = items < (\d+) \? items : \1, gz = \(items \+ gy - 1\) / gy", 32768),
        (CONV, r"void conv_bwd\(const ConvArgs g\)\s*\{\s*const long long item = \(long long\)g\.w0 \+ blockIdx\.y \+ \(long long\)blockIdx\.z \* gridDim\.y;", None),
        (CONV, r"void conv_upd\(const ConvArgs g\)\s*\{\s*const long long item = \(long long\)g\.w0 \+ blockIdx\.y \+ \(long long\)blockIdx\.z \* gridDim\.y;", None)]),
    "conv_trans_filter": dict(derive=lambda v: v[0] * v[1], unit="elements", per_trip=65536 * 256, source=[
        (CONV, r"gx = blocks < (\d+) \? blocks : \1, gy = \(blocks \+ gx - 1\) / gx", 65536), (TILE, r"constexpr int NTHREADS = (\d+);", 256),
        (CONV, r"blocks = \(total \+ NTHREADS - 1\) / NTHREADS", None),
        (CONV, r"\(\(long long\)blockIdx\.x \+ \(long long\)blockIdx\.y \* gridDim\.x\) \* NTHREADS \+ threadIdx\.x", None)]),
    # RNN cell: the split plan's launch of bias + w.x takes 65535 steps at a time (gridDim.z) and moves x and the chains along
    "rnn_steps": dict(derive=lambda v: v[0], unit="steps", per_trip=65535, source=[
        (RNN_HOST, r"for \(int t0 = 0; t0 < T; t0 \+= (\d+)\)", 65535),
        (RNN_HOST, r"a\.nz = \(T - t0 < (\d+)\) \? \(T - t0\) : \1;", 65535), (RNN, r"\|\| g\.nz > (\d+)\) return \(int\)hipErrorInvalidValue;", 65535),
        (RNN_HOST, r"a\.pre\[q\] = chain\[q\] \+ t0 \* nk;", None), (RNN_HOST, r"a\.x = f32\(ox\) \+ t0 \* nc;", None),
        (RNN, r"zx = \(long long\)blockIdx\.z \* g\.zx, zo = \(long long\)blockIdx\.z \* g\.zo;", None)]),
    # tiled GEMM: one grid covers 65535 tiles of columns. A test asks libxsmm_amd_gemm_tile() for the tile; tile_cross_check is
    # only what that answer is held against
    "tgemm_band": dict(derive=lambda v: v[0], unit="tiles of columns", per_trip=65535, tile_cross_check=128, source=[
        (TILE, r"constexpr int BAND = (\d+) \* BT;", 65535), ("xsmm_internal.hpp", r"constexpr int TGEMM_TILE = (\d+);", 128),
        (TILE, r"for \(long long n0 = 0; n0 < g\.n; n0 \+= BAND\)", None)]),
    # spmdm batch
    "spmdm_create": dict(derive=lambda v: 256 * v[0] * v[1], unit="items", per_trip=256 * 32 * 4, source=[
        GRID_FOR, (SPARSE, r"spmdm_create_staged_kernel, dim3\(grid_for\(g\.batch, (\d+)\)\)", 4),
        (SPARSE, r"spmdm_create_kernel, dim3\(grid_for\(g\.batch, (\d+)\)\)", 4)]),
    "spmdm_wg_lds": dict(derive=lambda v: 256 * v[0], unit="items", per_trip=256 * 8, source=[
        (SPARSE, r"if \(per_cu > (\d+)\) per_cu = \1; if \(per_cu < 1\) per_cu = 1;\s*const long long want", 8)]),
    "spmdm_mfma": dict(derive=lambda v: 256 * v[0], unit="items", per_trip=256 * 3, source=[
        (SPARSE, r"if \(per_cu > (\d+)\) per_cu = \1; if \(per_cu < 1\) per_cu = 1;\s*static const int bpc_env", 3)]),
    "spmdm_generic": dict(derive=lambda v: 256 * v[0] * v[1], unit="elements of C", per_trip=256 * 32 * 256, source=[
        GRID_FOR, (SPARSE, r"spmdm_compute_kernel, dim3\(grid_for\(total, (\d+)\)\), dim3\(256\)", 256)]),
    # fsspmdm without its operator kernel: a column of C per lane and trip
    "fsspmdm_csr": dict(derive=lambda v: 256 * v[0] * v[1], unit="columns", per_trip=256 * 32 * 256, source=[
        GRID_FOR, (SPARSE, r"csr_panels_kernel<double, 1>\), dim3\(grid_for\(ncols, (\d+)\)\), dim3\(256\)", 256),
        (SPARSE, r"csr_panels_kernel<float, 1>\), dim3\(grid_for\(ncols, (\d+)\)\), dim3\(256\)", 256)]),
    # dense generic kernel: PPB = 256 / G units per work-group (G = 64 lanes per unit up to 32 x 32), 4096 work-groups
    "smm_generic": dict(derive=lambda v: 256 * v[0], unit="work-groups", per_trip=256 * 16, lanes_small=64, source=[
        (GENERIC, r"const long long maxblocks = 256LL \* (\d+);", 16), (GENERIC, r"constexpr int G = TGM \* TGM, PPB = 256 / G", None),
        (GENERIC, r"if \(mx <= 8\) \{ \*name = names\[0\]; return launch_generic_t<T, 1, (\d+), GENERAL>", 8)]),
    "c_order": dict(derive=lambda v: v[0] * v[1], unit="items", per_trip=512 * 256, source=[
        ("xsmm_internal.hpp", r"constexpr int FLAG_SLOT_BLOCKS = (\d+);", 512),
        (GENERIC, r"long long blocks = \(s\.batch \+ 255\) / (\d+);\s*if \(blocks > FLAG_SLOT_BLOCKS\) blocks = FLAG_SLOT_BLOCKS;", 256)]),
    # low-precision SMM: a work-group per item
    "smm_lowp": dict(derive=lambda v: 256 * v[0], unit="items", per_trip=256 * 8, source=[
        (LOWP, r"if \(blocks > 256 \* (\d+)\) blocks = 256 \* \1;", 8),
        (LOWP, r"for \(long long item = blockIdx\.x; item < batch; item \+= gridDim\.x\)", None)]),
    # xcopy
    "xcopy_rows": dict(derive=lambda v: v[0], unit="slabs of columns", per_trip=65535, threads=256, source=[
        (XCOPY, r"\(unsigned\)\(by < (\d+) \? by : \1\)\), dim3\(256\)", 65535),
        (XCOPY, r"const int TX = 1 << lx, TY = (\d+) >> lx;", 256),
        (XCOPY, r"while \(lx < 8 && \(1LL << lx\) \* 4 < per\) \+\+lx;", None)]),
    "xcopy_generic": dict(derive=lambda v: v[0] * v[1], unit="units", per_trip=65536 * 256, source=[
        (XCOPY, r"long long blocks = \(total \+ 255\) / (\d+);\s*if \(blocks > 65536\) blocks = 65536;", 256),
        (XCOPY, r"if \(blocks > (\d+)\) blocks = \1;\s*decompose\(blocks \* 256", 65536)]),
    "xcopy_stack_trans": dict(derive=lambda v: v[0], unit="chunks", per_trip=16384, lds_chunk=16 * 1024, source=[
        (XCOPY, r"const unsigned blocks = \(unsigned\)\(nchunks < (\d+) \? nchunks : \1\);", 16384),
        ("xsmm_xcopy.cpp", r"constexpr size_t STACK_LDS_CHUNK = (\d+) \* 1024;", 16)]),
}


# switches between two instantiations of a kernel: a size, not a trip (sized() knows nothing of them)
THRESHOLDS = {
    "quant_layout_wide": dict(derive=lambda v: 1 << v[0], unit="outputs", threshold=1 << 31, source=[
        (QUANT, r"if \(g\.total < \(1LL << (\d+)\)\) hipLaunchKernelGGL\(\(quant_layout_kernel<MODE, unsigned int>\)", 31),
        (QUANT, r"else hipLaunchKernelGGL\(\(quant_layout_kernel<MODE, unsigned long long>\)", None)]),
    # RNN cell: a share of more than 65535 tiles of 64 rows (gridDim.y) is refused, not split: the rows go to more logical threads.
    # chunk: the rows of w or r per trip through LDS (a segment's rest below it ends on the vector ALU)
    "rnn_rows_per_share": dict(derive=lambda v: v[0] * v[1], unit="rows", threshold=65535 * 64, tiles=65535, tile=64, chunk=32, source=[
        (RNN, r"if \(tk > 0x7fffffffLL \|\| tn > (\d+) \|\|", 65535), (RNN, r"constexpr int BT = (\d+);", 64),
        (RNN, r"tn = \(\(long long\)\(g\.n1 - g\.n0\) \+ BT - 1\) / BT;", None), (RNN, r"jt0 = g\.n0 \+ BT \* \(int\)blockIdx\.y;", None),
        (RNN, r"constexpr int BK = (\d+);", 32)]),
}


def threshold(name):
    return THRESHOLDS[name]["threshold"]


def per_trip(name):
    return LIMITS[name]["per_trip"]


def sized(name, rest, trips=2):
    """`trips` full trips and `rest` more"""
    assert rest % 2 == 1 and rest % 64 != 0 and 0 < rest < per_trip(name), rest
    return trips * per_trip(name) + rest


def check(entry):
    """every (file, expression, value) of an entry against the sources, and per_trip against the numbers found (derive takes
    them in the order of the entry); returns the list of complaints"""
    bad, numbers = [], []
    for path, pattern, value in entry["source"]:
        text = open(os.path.join(CSRC, path)).read()
        found = re.search(pattern.replace(" ", r"\s*"), text)  # (however the source is spaced and broken into lines)
        if found is None:
            bad.append("%s: no match for %r" % (path, pattern))
        elif value is not None:
            numbers.append(int(found.group(1)))
            if numbers[-1] != value:
                bad.append("%s: %r gives %s, the tests assume %d" % (path, pattern, found.group(1), value))
    size = entry["per_trip"] if "per_trip" in entry else entry["threshold"]
    if not bad and entry["derive"](numbers) != size:
        bad.append("%d does not follow from %r" % (size, numbers))
    return bad
