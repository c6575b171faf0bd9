"""What the tests of libxsmm_dnn_copyin_tensor / _copyout_tensor share: the reference's copies restated in numpy, the layouts the
tests walk (taken from real handles, so the block sizes are the library's own), and buffers between canaries.

The reference's copies are pure permutations (src/template/libxsmm_dnn_tensor_buffer_copy_{in,out}_nchw.tpl.c,
libxsmm_dnn_tensor_filter_copy_{in,out}_kcrs.tpl.c, libxsmm_dnn_tensor_bias_copy_{in,out}_nchw.tpl.c). source_index(fields) is the
index formula of the copy-in templates: element i of the tensor is element source_index[i] of the plain buffer; the copy-out
templates are the same assignment the other way round. Channel tensors are a plain copy."""
import numpy as np

from dnn_common import F32, BF16, I32, FMT_LIBXSMM, FMT_NHWC, FMT_NCHW, REG_IN, REG_FIL, GRAD_IN  # noqa: F401

FMT_RSCK, FMT_KCRS = 8, 16
GRAD_FIL = 12
ACTIVATION_TYPES, FILTER_TYPES = (0, 3, 5, 6, 7, 8, 9), (10, 12, 13)
CHANNEL_TYPES = tuple(range(14, 27))  # REGULAR_CHANNEL_BIAS ... CHANNEL_SCALAR: the thirteen of src/libxsmm_dnn.c:1300-1312
CHANNEL_BIAS, CHANNEL_BETA, CHANNEL_GAMMA, CHANNEL_EXPECTVAL, CHANNEL_RCPSTDDEV, CHANNEL_VARIANCE = 14, 17, 20, 23, 24, 25

SUCCESS = 0
ERR_GENERAL, ERR_UNSUPPORTED_DATATYPE, ERR_INVALID_TENSOR = 100000, 100002, 100007
ERR_UNSUPPORTED_DST_FORMAT, ERR_UNSUPPORTED_SRC_FORMAT, ERR_INVALID_LAYOUT, ERR_NOT_IMPLEMENTED = 100012, 100013, 100018, 100029

CANARY, BAND = 0xA5, 64  # bytes on both sides of every buffer


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def kind_of(fields):
    t = fields[6]
    return "act" if t in ACTIVATION_TYPES else "fil" if t in FILTER_TYPES else "chan" if t in CHANNEL_TYPES else None


def typesize(fields):
    return {F32: 4, BF16: 2}[fields[3]]


def elements(fields):
    n = 1
    for s in fields[2]:
        n *= s
    return n


def source_index(fields):
    """tensor[i] = plain[source_index[i]]: the loops of the copy-in templates, every index variable an axis"""
    sizes, kind = fields[2], kind_of(fields)
    if kind == "chan":
        return np.arange(elements(fields), dtype=np.int64)
    if kind == "act":  # [N][fmb][H][W][bfm][lpb]; dimension 0 of a layout is the fastest, 16-bit layouts carry lpb first
        lpb, bfm, W, H, fmb, N = ([1] + sizes) if len(sizes) == 5 else sizes
        i1, i2, i3, i4, i5, i6 = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in (N, fmb, H, W, bfm, lpb)], indexing="ij", sparse=True)
        Cc = fmb * bfm * lpb
        return (((i1 * Cc + (i2 * bfm * lpb + i5 * lpb + i6)) * H + i3) * W + i4).reshape(-1)
    lpb, bofm, bifm, S, R, ifmb, ofmb = ([1] + sizes) if len(sizes) == 6 else sizes  # [ofmb][ifmb][R][S][bifm][bofm][lpb]
    i1, i2, i3, i4, i5, i6, i7 = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in (ofmb, ifmb, R, S, bifm, bofm, lpb)], indexing="ij", sparse=True)
    Cc = ifmb * bifm * lpb
    return ((((i1 * bofm + i6) * Cc + (i2 * bifm * lpb + i5 * lpb + i7)) * R + i3) * S + i4).reshape(-1)


def elems(fields, raw):
    """bytes as the layout's elements (unsigned integers: nothing here is arithmetic)"""
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view(np.uint32 if 4 == typesize(fields) else np.uint16)


def copy_in(fields, plain):
    """the tensor's bytes after copy-in of the plain bytes"""
    return elems(fields, plain)[source_index(fields)].view(np.uint8)


def copy_out(fields, tensor):
    """the plain bytes after copy-out of the tensor's bytes"""
    out = np.empty_like(elems(fields, tensor))
    out[source_index(fields)] = elems(fields, tensor)
    return out.view(np.uint8)


def hostile_bytes(nbytes, seed, ts=4):
    """arbitrary bits, with the patterns a float copy could mangle planted in front: NaN payloads (quiet and signalling), +-0, +-Inf,
    subnormals"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0, 0x7f800000, 0xff800000, 1, 0x807fffff], dtype=np.uint32) if 4 == ts else \
        np.array([0x7fc1, 0xffc5, 0x7f81, 0x8000, 0, 0x7f80, 0xff80, 1, 0x807f], dtype=np.uint16)
    sb = special.view(np.uint8)[:nbytes]
    raw[:sb.size] = sb
    return raw


# ---- layouts from real handles ---------------------------------------------------------------------------------------------------------
CONV_C24 = dict(N=2, Cc=24, H=5, W=7, K=40, R=3, S=3, pad_h=1, pad_w=1, pad_h_in=1, pad_w_in=1)
CONV_C3 = dict(N=2, Cc=3, H=5, W=7, K=16, R=7, S=7, pad_h=3, pad_w=3)
CONV_8X8 = dict(N=2, Cc=16, H=8, W=8, K=16, R=1, S=1)
CONV_5X13 = dict(N=2, Cc=16, H=5, W=13, K=18, R=1, S=1)
CONV_11 = dict(N=1, Cc=16, H=11, W=11, K=16, R=11, S=11)
FC_F32 = dict(N=5, Cc=32, K=48)                     # tests/fc_common.py l_5_32_48
FC_BF16 = dict(N=5, Cc=32, K=48, datatype_in=BF16)   # lb_5_32_48 (fp32 outputs)
BN_BF16 = dict(N=2, Cc=32, H=6, W=6, datatype_in=BF16, datatype_out=BF16)
BN_C24 = dict(N=2, Cc=24, H=4, W=4)

# name -> (layer, desc, tensor type, plain format)
ACTIVATIONS = {
    "act_conv_c24_7x9": ("conv", CONV_C24, REG_IN, FMT_NCHW),   # 63 pixels: odd, below one tile; the block is 8
    "act_conv_c3": ("conv", CONV_C3, REG_IN, FMT_NCHW),         # the block is 3
    "act_8x8": ("conv", CONV_8X8, REG_IN, FMT_NCHW),            # 64 pixels: vectorised throughout
    "act_5x13": ("conv", CONV_5X13, REG_IN, FMT_NCHW),          # 65 pixels
    "act_fc_f32": ("fc", FC_F32, REG_IN, FMT_NCHW),
    "act_fc_bf16": ("fc", FC_BF16, REG_IN, FMT_NCHW),           # lpb = 2
    "act_bn_bf16_6x6": ("bn", BN_BF16, REG_IN, FMT_NCHW),
}
FILTERS = {
    "fil_c24_k40_3x3": ("conv", CONV_C24, REG_FIL, FMT_KCRS),
    "fil_c3_k16_7x7": ("conv", CONV_C3, REG_FIL, FMT_KCRS),
    "fil_c16_k18_1x1": ("conv", CONV_5X13, REG_FIL, FMT_KCRS),  # bofm is 2
    "fil_c16_k16_11x11": ("conv", CONV_11, REG_FIL, FMT_KCRS),  # the block is cut
    "fil_fc_f32": ("fc", FC_F32, REG_FIL, FMT_KCRS),
    "fil_fc_bf16": ("fc", FC_BF16, REG_FIL, FMT_KCRS),          # 7 dimensions
}
CHANNELS = {
    "bias_k40": ("conv", CONV_C24, CHANNEL_BIAS, FMT_NCHW),
    "bn_beta": ("bn", BN_C24, CHANNEL_BETA, FMT_NCHW),
    "bn_gamma": ("bn", BN_C24, CHANNEL_GAMMA, FMT_NCHW),
    "bn_expectval": ("bn", BN_C24, CHANNEL_EXPECTVAL, FMT_NCHW),
    "bn_rcpstddev": ("bn", BN_C24, CHANNEL_RCPSTDDEV, FMT_NCHW),
    "bn_variance": ("bn", BN_C24, CHANNEL_VARIANCE, FMT_NCHW),
}
CASES = dict(ACTIVATIONS, **FILTERS, **CHANNELS)


class Case:
    """the layout of a case from a handle of its layer; close() destroys both"""

    def __init__(self, xs, name):
        layer, desc, self.ttype, self.fmt = CASES[name]
        self.xs, self.L, self.name = xs, xs.lib(), name
        create, layout, self.destroy = {
            "conv": (xs.conv_create, xs.conv_layout, self.L.libxsmm_dnn_destroy_conv_layer),
            "fc": (xs.fc_create, xs.fc_layout, self.L.libxsmm_dnn_destroy_fullyconnected),
            "bn": (xs.bn_create, xs.bn_layout, self.L.libxsmm_dnn_destroy_fusedbatchnorm)}[layer]
        self.handle, st = create(**desc)
        assert self.handle and st < 100000, (name, st)
        self.layout, st = layout(self.handle, self.ttype)
        assert self.layout is not None and 0 == st, (name, st)
        self.fields = xs.dnn_layout_fields(self.layout)
        self.nbytes = elements(self.fields) * typesize(self.fields)

    def close(self):
        self.L.libxsmm_dnn_destroy_tensor_datalayout(self.layout)
        self.destroy(self.handle)


def resized(xs, layout, sizes):
    """a copy of a layout with other extents (the caller destroys it): what a handle with those blocks would return"""
    import ctypes
    st = ctypes.c_uint()
    copy = xs.lib().libxsmm_dnn_duplicate_tensor_datalayout(layout, ctypes.byref(st))
    assert copy and 0 == st.value and len(sizes) == copy.contents.num_dims
    for j, n in enumerate(sizes):
        copy.contents.dim_size[j] = n
    return copy


class Guarded:
    """nbytes of memory between two bands of canary bytes; where: "pageable" (numpy), "pinned" or "device" (torch). shift moves the
    payload off its 16-byte boundary. content: the payload's bytes (default: 0x3c)."""

    def __init__(self, torch, nbytes, where="pageable", content=None, shift=0):
        self.torch, self.nbytes, self.where, self.off = torch, nbytes, where, BAND + shift
        host = np.full(self.off + nbytes + BAND + 16, CANARY, dtype=np.uint8)
        host[self.off:self.off + nbytes] = 0x3C if content is None else np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        if "pageable" == where:
            self.mem, base = host, host.ctypes.data
        else:
            self.mem = torch.from_numpy(host).cuda() if "device" == where else torch.from_numpy(host).pin_memory()
            base = self.mem.data_ptr()
            assert 0 == base % 16
        self.ptr = base + self.off

    def payload(self):
        """the payload's bytes; asserts the canaries (device memory: after waiting for every stream)"""
        if "pageable" == self.where:
            host = self.mem
        else:
            self.torch.cuda.synchronize()
            host = self.mem.cpu().numpy()
        assert np.all(host[:self.off] == CANARY) and np.all(host[self.off + self.nbytes:] == CANARY), "a canary was overwritten"
        return host[self.off:self.off + self.nbytes].copy()
