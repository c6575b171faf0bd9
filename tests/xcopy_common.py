"""Shared by tests/test_xcopy_cpu.py and tests/test_xcopy_gpu.py: byte-exact buffers for the copy / transposition entry points
(libxsmm_matcopy, libxsmm_otrans, libxsmm_itrans, the dispatched mcopy / trans kernels and the stack forms of libxsmm_amd.h).

A buffer is, in elements of `typesize` bytes: GUARD canaries, `off` more canaries (so the matrix can start one element past a
16-byte boundary), the operand as it is stored (every padding element a canary), GUARD canaries. The first byte of the buffer
is 16-byte aligned (GUARD * typesize is a multiple of 16 for every typesize). Expected results are whole buffers built with
numpy: the bytes the call may write are replaced, everything else -- guards, padding, gaps between items -- must keep its bits,
so one array_equal checks the result and every canary at once. Data are random bytes with a NaN payload and a -0 planted."""
import ctypes as C

import numpy as np

GUARD = 96
CANARY = 0xCD


def aligned_bytes(nbytes, fill=CANARY):
    """uint8 array whose first byte is 16-byte aligned"""
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16
    return raw[start:start + nbytes]


class Stack:
    """`batch` items of rows x cols elements (column major, columns ld apart, items stride apart), off elements past alignment"""

    def __init__(self, ts, rows, cols, ld=None, stride=None, batch=1, off=0, rng=None, fill=True):
        self.ts, self.rows, self.cols, self.batch, self.off = ts, rows, cols, batch, off
        self.ld = rows if ld is None else ld
        self.extent = (cols - 1) * self.ld + rows if rows and cols else 0
        self.stride = self.extent if stride is None else stride
        self.span = ((batch - 1) * self.stride + self.extent) if batch else 0
        self.base = (GUARD + off) * ts
        self.host = aligned_bytes((GUARD + off + self.span + GUARD) * ts)
        if fill and self.span:
            rng = rng or np.random.default_rng(0)
            v = self.view()
            v[...] = rng.integers(0, 256, size=v.shape, dtype=np.uint8)
            if ts in (4, 8):  # a NaN with a payload and -0, bit patterns a floating-point move could alter
                v[0, 0, 0] = np.frombuffer((0x7FA0DEAD if ts == 4 else 0x7FF4DEADBEEF0BAD).to_bytes(ts, "little"), np.uint8)
                if rows * cols * batch > 1:
                    v[-1, -1, -1] = np.frombuffer((1 << (8 * ts - 1)).to_bytes(ts, "little"), np.uint8)

    def view(self, buf=None):
        """(batch, cols, rows, ts) view of the elements of the items inside buf (default: the host buffer)"""
        buf = self.host if buf is None else buf
        ts = self.ts
        return np.lib.stride_tricks.as_strided(buf[self.base:], shape=(self.batch, self.cols, self.rows, ts),
                                               strides=(self.stride * ts, self.ld * ts, ts, 1), writeable=True)

    def ptr(self, origin=None):
        """address of element (0, 0) of item 0 (origin: the address of the buffer's first byte, default the host buffer's)"""
        return (self.host.ctypes.data if origin is None else origin) + self.base

    def item_ptrs(self, origin=None):
        return np.array([self.ptr(origin) + g * self.stride * self.ts for g in range(self.batch)], dtype=np.uint64)


def expected_copy(dst, src):
    """the destination buffer after matcopy (src None: zero fill)"""
    out = dst.host.copy()
    dst.view(out)[...] = 0 if src is None else src.view()
    return out


def expected_trans(dst, src):
    """the destination buffer after otrans: dst is cols x rows of src"""
    out = dst.host.copy()
    dst.view(out)[...] = src.view().transpose(0, 2, 1, 3)
    return out


def expected_itrans(mat):
    out = mat.host.copy()
    mat.view(out)[...] = mat.view().transpose(0, 2, 1, 3)
    return out


class Device:
    """a Stack's buffer in device memory (torch uint8 tensor; torch allocations are at least 256-byte aligned)"""

    def __init__(self, torch, stack):
        self.stack = stack
        self.t = torch.from_numpy(stack.host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.stack.ptr(self.t.data_ptr())

    def item_ptrs(self):
        return self.stack.item_ptrs(self.t.data_ptr())

    def get(self):
        return self.t.cpu().numpy()


class Pinned:
    """a Stack's buffer in memory of libxsmm_malloc (the CPU and the GPU address it)"""

    def __init__(self, xs, stack):
        self.stack, self.L = stack, xs.lib()
        n = stack.host.size
        self.p = self.L.libxsmm_aligned_malloc(n, 16)
        assert self.p and self.p % 16 == 0
        self.arr = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_ubyte)), shape=(n,))
        self.arr[...] = stack.host

    def ptr(self):
        return self.stack.ptr(self.p)

    def get(self):
        return self.arr.copy()

    def free(self):
        self.L.libxsmm_free(self.p)


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else "%d bytes differ, first at byte %d (got 0x%02x, expected 0x%02x)" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
