"""What the numpy restatements of the DNN layers share (tests/pool_common.py, tests/bn_common.py and, for the constants, the split
and layout_size, tests/fc_common.py): the constants of include/libxsmm_dnn.h, the feature-map blocking with the activation
layouts built on it, the split of a pass over logical threads, and the 16-bit element helpers. The layer modules re-export
these names."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

F32, BF16, I32, I16 = 1, 2, 4, 5
FMT_LIBXSMM, FMT_NHWC, FMT_NCHW = 1, 2, 4
FWD, BWD, UPD, BWDUPD, ALL = 0, 1, 2, 3, 4
REG_IN, GRAD_IN, REG_OUT, GRAD_OUT, GEN_IN, GEN_OUT, REG_FIL = 0, 3, 5, 6, 7, 8, 10
DIM_N, DIM_H, DIM_W, DIM_C = 0, 1, 2, 3

SUCCESS = 0
ERR_GENERAL, ERR_UNSUPPORTED_DATATYPE, ERR_INVALID_HANDLE, ERR_DATA_NOT_BOUND = 100000, 100002, 100004, 100005
ERR_MISMATCH_TENSOR, ERR_INVALID_HANDLE_TENSOR, ERR_INVALID_KIND, ERR_INVALID_FORMAT_GENERAL = 100008, 100009, 100010, 100016
ERR_SCRATCH_NOT_ALLOCED, ERR_UNKNOWN_TENSOR_TYPE, ERR_INVALID_FORMAT_FUSEDBN = 100020, 100021, 100032


def share(work, threads, ltid):
    """the items [b0, b1) of logical thread ltid (the templates' chunksize, thr_begin, thr_end)"""
    chunk = work // threads if work % threads == 0 else work // threads + 1
    return min(ltid * chunk, work), min((ltid + 1) * chunk, work)


def made(types, sizes, datatype, fmt, tensor_type=0):
    return SUCCESS, dict(num_dims=len(types), dim_type=list(types), dim_size=[int(s) for s in sizes], datatype=datatype, format=fmt,
                         custom_format=1, tensor_type=tensor_type)


def layout_size(l):
    n = 1
    for s in l["dim_size"]:
        n *= s
    return n * {F32: 4, BF16: 2, I32: 4, I16: 2}[l["datatype"]], n


# ---- handle rules of the layers on blocked activations (src/libxsmm_dnn_setup.c:197-252) ------------------------------------------
class FmHandle:
    """the data types and the feature-map blocking of a desc with N, C, H, W and the physical paddings; a layer's Handle adds its
    output plane (set_output), its scratch_size, its other layouts and its statuses, and sets ok"""

    def __init__(self, d):
        self.d = d
        self.ok = False
        pair = (d["datatype_in"], d["datatype_out"])
        if pair not in ((F32, F32), (BF16, BF16)):
            self.status = ERR_UNSUPPORTED_DATATYPE
            return
        self.status = SUCCESS
        self.f32 = pair == (F32, F32)
        Cc = d["C"]
        if self.f32:
            self.ifmblock, self.fm_lp_block = (16 if Cc >= 16 else Cc), 1
        else:
            self.ifmblock, self.fm_lp_block = (8 if Cc >= 16 else Cc // 2), 2
            if Cc == 3:
                self.ifmblock, self.fm_lp_block = 3, 1
        self.ofmblock = 16
        self.ifmblock_hp, self.ofmblock_lp = self.ifmblock * self.fm_lp_block, self.ofmblock // self.fm_lp_block
        self.blocksifm = Cc // (self.ifmblock if self.f32 else self.ifmblock_hp)
        self.blocksofm = Cc // self.ofmblock

    def set_output(self, ofh, ofw):
        d = self.d
        self.ofh, self.ofw = ofh, ofw
        self.ifhp, self.ifwp = d["H"] + 2 * d["pad_h_in"], d["W"] + 2 * d["pad_w_in"]
        self.ofhp, self.ofwp = ofh + 2 * d["pad_h_out"], ofw + 2 * d["pad_w_out"]

    def scratch(self):
        return self.scratch_size + 64

    def activation_layout(self, inp):
        """the layout of an input-side (inp) or output-side activation tensor"""
        d = self.d
        fmt = d["buffer_format"]
        if fmt & FMT_LIBXSMM:
            if self.f32:
                sizes = (self.ifmblock, self.ifwp, self.ifhp, self.blocksifm, d["N"]) if inp else (self.ofmblock, self.ofwp, self.ofhp, self.blocksofm, d["N"])
                return made((DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), sizes, F32, fmt)
            sizes = (self.fm_lp_block, self.ifmblock, self.ifwp, self.ifhp, self.blocksifm, d["N"]) if inp \
                else (self.fm_lp_block, self.ofmblock_lp, self.ofwp, self.ofhp, self.blocksofm, d["N"])
            return made((DIM_C, DIM_C, DIM_W, DIM_H, DIM_C, DIM_N), sizes, BF16, fmt)
        if fmt & FMT_NHWC:
            sizes = (d["C"], self.ifwp, self.ifhp, d["N"]) if inp else (d["C"], self.ofwp, self.ofhp, d["N"])
            return made((DIM_C, DIM_W, DIM_H, DIM_N), sizes, d["datatype_in"], fmt)
        return ERR_INVALID_FORMAT_GENERAL, None

    def runnable(self):
        """the channel block is the 16 the kernels are written for, on both sides"""
        return self.ifmblock_hp == 16 and self.blocksifm == self.blocksofm

    def work(self):
        return self.d["N"] * self.blocksifm

    def share(self, ltid):
        return share(self.work(), self.d["threads"], ltid)

    # shapes of the blocked activations as arrays [item][row][column][16]
    def in_shape(self):
        return (self.work(), self.ifhp, self.ifwp, 16)

    def out_shape(self):
        return (self.work(), self.ofhp, self.ofwp, 16)


# ---- 16-bit elements: widened by a shift, stored by truncation (the generic templates' union) -------------------------------------
def widen(a):
    return (np.asarray(a, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def truncate(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def as_f32(h, a):
    return a if h.f32 else widen(a)


def stored(h, a):
    return a.astype(np.float32) if h.f32 else truncate(a)


def elem_dtype(h):
    return np.float32 if h.f32 else np.uint16


def fma(a, b, c):
    """fp32 fma of arrays through float64: the product is exact there; the sum is rounded twice (to 53, then 24 bits), which
    differs from one rounding only in rare halfway cases -- good enough to tell the fused form from the separate one"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def check_mixed_residency(torch, roles, host_written, bind, run):
    """One pass with its tensors split over pageable host memory and the device. roles: key -> (contents before the pass,
    contents after it, whether the pass writes the tensor); host_written: the written tensors are pageable numpy arrays and the
    others lie on the device, else the reverse. bind(key, memory) binds a tensor, run() executes the pass. Every tensor is compared
    byte for byte, the pageable ones first and with no wait after the call. Returns what bind returned."""
    mem, tensors = {}, []
    for key, (before, _, written) in roles.items():
        a = np.ascontiguousarray(before).copy()
        # (torch has no uint16 arithmetic: the bytes travel as int16)
        mem[key] = a if written == host_written else torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        tensors.append(bind(key, mem[key]))
    assert 0 == run()
    for key, (_, after, _) in roles.items():
        if isinstance(mem[key], np.ndarray):
            assert mem[key].tobytes() == after.tobytes(), "pageable tensor %s differs" % (key,)
    torch.cuda.synchronize()
    for key, (_, after, _) in roles.items():
        if not isinstance(mem[key], np.ndarray):
            assert mem[key].cpu().numpy().tobytes() == after.tobytes(), "device tensor %s differs" % (key,)
    return tensors
