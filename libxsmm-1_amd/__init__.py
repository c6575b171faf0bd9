"""libxsmm-1_amd -- Python-side plumbing for the MI355X-native LIBXSMM engine.

The product is the C-ABI shared library ``lib/libxsmm.so`` (sources in ``csrc/``, interface in
``/include/libxsmm.h``). This module only loads it through ``ctypes`` and declares argument
types, so that tests and ``bench.py`` can call the *same* entry points a C caller binds
(reference interface: ``src/template/libxsmm.h:73-414``). There is no Python or CPU compute path
here: if the library is missing, or no HIP device is usable, calls fail loudly.

Import with ``importlib.import_module("libxsmm-1_amd")`` (the directory name is not an identifier).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LIBXSMM_AMD_LIBRARY", os.path.join(_HERE, "lib", "libxsmm.so"))  # override: A/B builds in tools/
CSRC = os.path.join(_HERE, "csrc")

# enum values (include/libxsmm.h; reference include/libxsmm_typedefs.h:158-213)
F64, F32, BF16, I32, I16 = 0, 1, 2, 4, 5  # libxsmm_gemm_precision (include/libxsmm.h)
FLAG_TRANS_A, FLAG_TRANS_B, FLAG_BETA_0, FLAG_BATCH_REDUCE = 1, 2, 16, 256

c_int_p = C.POINTER(C.c_int)


class DescriptorBlob(C.Structure):
    _fields_ = [("data", C.c_char * 64)]


class MMKernelInfo(C.Structure):  # libxsmm_mmkernel_info
    _fields_ = [("iprecision", C.c_int), ("oprecision", C.c_int), ("prefetch", C.c_int),
                ("lda", C.c_uint), ("ldb", C.c_uint), ("ldc", C.c_uint),
                ("m", C.c_uint), ("n", C.c_uint), ("k", C.c_uint), ("flags", C.c_int)]


class TransKernelInfo(C.Structure):  # libxsmm_transkernel_info
    _fields_ = [("ldo", C.c_uint), ("m", C.c_uint), ("n", C.c_uint), ("typesize", C.c_uint)]


class McopyKernelInfo(C.Structure):  # libxsmm_mcopykernel_info
    _fields_ = [("ldi", C.c_uint), ("ldo", C.c_uint), ("m", C.c_uint), ("n", C.c_uint), ("typesize", C.c_uint),
                ("prefetch", C.c_int), ("flags", C.c_int)]


class RegistryInfo(C.Structure):
    _fields_ = [("capacity", C.c_size_t), ("size", C.c_size_t), ("nbytes", C.c_size_t),
                ("nstatic", C.c_size_t), ("ncache", C.c_size_t)]


class SpmdmHandle(C.Structure):  # libxsmm_spmdm_handle (reference include/libxsmm_spmdm.h:42-61)
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("k", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("bk", C.c_int),
                ("mb", C.c_int), ("nb", C.c_int), ("kb", C.c_int), ("datatype", C.c_int),
                ("base_ptr_scratch_A", C.c_void_p), ("base_ptr_scratch_B_scratch_C", C.c_void_p),
                ("memory_for_scratch_per_thread", C.c_int)]


class CSRSlice(C.Structure):  # libxsmm_CSR_sparseslice
    _fields_ = [("rowidx", C.c_void_p), ("colidx", C.c_void_p), ("values", C.c_void_p)]


class GeneratedCode(C.Structure):  # libxsmm_generated_code
    _fields_ = [("generated_code", C.c_void_p), ("buffer_size", C.c_uint), ("code_size", C.c_uint), ("code_type", C.c_uint),
                ("last_error", C.c_uint)]

    def text(self):
        return C.string_at(self.generated_code, self.code_size).decode() if self.generated_code else ""

    def release(self):
        if self.generated_code:
            C.CDLL(None).free(C.c_void_p(self.generated_code))
            self.generated_code = None


class MatdiffInfo(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "norm1_abs", "norm1_rel", "normi_abs", "normi_rel", "normf_rel", "linf_abs", "linf_rel", "l2_abs", "l2_rel",
        "l1_ref", "min_ref", "max_ref", "avg_ref", "var_ref", "l1_tst", "min_tst", "max_tst", "avg_tst", "var_tst")] + \
        [("m", C.c_int), ("n", C.c_int)]


class TensorDatalayout(C.Structure):  # libxsmm_dnn_tensor_datalayout
    _fields_ = [("dim_type", C.POINTER(C.c_int)), ("dim_size", C.POINTER(C.c_uint)), ("num_dims", C.c_uint), ("format", C.c_int),
                ("custom_format", C.c_int), ("datatype", C.c_int), ("tensor_type", C.c_int)]


class FullyconnectedDesc(C.Structure):  # libxsmm_dnn_fullyconnected_desc
    _fields_ = [(n, C.c_int) for n in ("N", "C", "K", "bn", "bk", "bc", "threads", "datatype_in", "datatype_out", "buffer_format",
                                       "filter_format", "fuse_ops")]


class PoolingDesc(C.Structure):  # libxsmm_dnn_pooling_desc
    _fields_ = [(n, C.c_int) for n in ("N", "C", "H", "W", "R", "S", "u", "v", "pad_h", "pad_w", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out",
                                       "threads", "datatype_in", "datatype_out", "datatype_mask", "buffer_format", "pooling_type")]


class FusedBatchnormDesc(C.Structure):  # libxsmm_dnn_fusedbatchnorm_desc
    _fields_ = [(n, C.c_int) for n in ("N", "C", "H", "W", "u", "v", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out", "threads", "datatype_in",
                                       "datatype_out", "datatype_stats", "buffer_format", "fuse_order", "fuse_ops")]


class ConvDesc(C.Structure):  # libxsmm_dnn_conv_desc
    _fields_ = [(n, C.c_int) for n in ("N", "C", "H", "W", "K", "R", "S", "u", "v", "pad_h", "pad_w", "pad_h_in", "pad_w_in", "pad_h_out", "pad_w_out",
                                       "threads", "datatype_in", "datatype_out", "buffer_format", "filter_format", "algo", "options", "fuse_ops")] \
        + [("pre_bn", C.c_void_p), ("post_bn", C.c_void_p)]


class RnncellDesc(C.Structure):  # libxsmm_dnn_rnncell_desc
    _fields_ = [(n, C.c_int) for n in ("threads", "K", "N", "C", "max_T", "bk", "bn", "bc", "cell_type", "datatype_in", "datatype_out",
                                       "buffer_format", "filter_format")]


def build(verbose=False):
    """Compile csrc/ into lib/libxsmm.so for gfx950 (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("building libxsmm.so failed")
    return LIB_PATH


# shapes whose code objects build() leaves in lib/jit_cache (they travel with the library): the BASELINE configurations
PREBUILD_F64 = [(m, n, k) for m in (13, 23, 32) for n in (13, 23, 32) for k in (13, 23, 32)]  # config 1 and 5 (CP2K stacks: also grouped)
PREBUILD_F64 += [(40, 40, 40), (48, 48, 48), (56, 56, 56), (64, 64, 64)]  # shapes beyond 32: matrix-core forms
PREBUILD_F32 = [(32, 32, 32), (23, 23, 23), (13, 13, 13), (40, 40, 40), (48, 48, 48), (56, 56, 56), (64, 64, 32)]


def prebuild_kernels(verbose=False):
    """hiprtc ahead of time (no device needed): see libxsmm_amd_jit_prebuild"""
    L = lib()
    total = 0
    for prec, shapes, grouped in ((F64, PREBUILD_F64, 1), (F32, PREBUILD_F32, 0)):
        keep, arr = [], (C.c_void_p * len(shapes))()
        for idx, (m, n, k) in enumerate(shapes):
            blob, d = descriptor(prec, m, n, k)
            keep.append(blob); arr[idx] = C.cast(d, C.c_void_p)
        rc = L.libxsmm_amd_jit_prebuild(arr, len(shapes), grouped)
        if verbose:
            print("prebuild: precision %d, %d shapes -> %d" % (prec, len(shapes), rc))
        if rc < 0:
            raise RuntimeError("libxsmm_amd_jit_prebuild failed for %d code objects" % -rc)
        total += rc
    return total


_lib = None


def lib():
    """The loaded C-ABI library (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run __graft_entry__.build() (there is no non-HIP fallback)" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's). If
        # libxsmm.so were loaded first, a later `import torch` would map a second runtime and neither would see the
        # GPU reliably. Importing torch first makes libxsmm.so bind to the runtime torch already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
        import atexit
        atexit.register(L.libxsmm_amd_jit_drain)  # before the interpreter goes: see include/libxsmm_amd.h
    return _lib


def _declare(L):
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)
    sig("libxsmm_init", None)
    sig("libxsmm_finalize", None)
    sig("libxsmm_get_verbosity", i)
    sig("libxsmm_set_verbosity", None, i)
    sig("libxsmm_get_target_arch", C.c_char_p)
    sig("libxsmm_set_target_arch", None, C.c_char_p)
    sig("libxsmm_get_target_archid", i)
    sig("libxsmm_set_target_archid", None, i)
    sig("libxsmm_dgemm_descriptor_init", vp, C.POINTER(DescriptorBlob), i, i, i, i, i, i, C.c_double, C.c_double, i, i)
    sig("libxsmm_sgemm_descriptor_init", vp, C.POINTER(DescriptorBlob), i, i, i, i, i, i, C.c_float, C.c_float, i, i)
    sig("libxsmm_gemm_descriptor_dinit", vp, C.POINTER(DescriptorBlob), i, i, i, i, i, i, i, C.c_double, C.c_double, i, i)
    sig("libxsmm_gemm_descriptor_init", vp, C.POINTER(DescriptorBlob), i, i, i, i, i, i, i, vp, vp, i, i)
    sig("libxsmm_xmmdispatch", vp, vp)
    sig("libxsmm_dmmdispatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_double), C.POINTER(C.c_double), c_int_p, c_int_p)
    sig("libxsmm_smmdispatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_float), C.POINTER(C.c_float), c_int_p, c_int_p)
    sig("libxsmm_wimmdispatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p)
    for name in ("libxsmm_wsmmdispatch", "libxsmm_bsmmdispatch", "libxsmm_bmmdispatch"):
        sig(name, vp, i, i, i, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_float), C.POINTER(C.c_float), c_int_p, c_int_p)
    sig("libxsmm_dmmdispatch_reducebatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_double), C.POINTER(C.c_double), c_int_p, c_int_p)
    sig("libxsmm_smmdispatch_reducebatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_float), C.POINTER(C.c_float), c_int_p, c_int_p)
    sig("libxsmm_wimmdispatch", vp, i, i, i, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p)
    sig("libxsmm_release_kernel", None, vp)
    sig("libxsmm_get_kernel_kind", i, vp, c_int_p)
    sig("libxsmm_get_mmkernel_info", i, vp, C.POINTER(MMKernelInfo), C.POINTER(C.c_size_t))
    sig("libxsmm_get_registry_info", i, C.POINTER(RegistryInfo))
    sig("libxsmm_create_dcsr_reg", vp, vp, vp, vp, vp)
    sig("libxsmm_create_scsr_reg", vp, vp, vp, vp, vp)
    batch_args = [i, i, vp, vp, i, i, i, vp, vp, c_int_p, vp, c_int_p, vp, vp, c_int_p, i, i, vp, vp, vp, i]
    sig("libxsmm_gemm_batch", None, *batch_args)
    sig("libxsmm_gemm_batch_omp", None, *batch_args)
    sig("libxsmm_mmbatch", None, *(batch_args + [i, i]))
    sig("libxsmm_mmbatch_kernel", i, vp, i, i, vp, vp, vp, vp, vp, vp, i, i, i, C.c_ubyte, C.c_ubyte, i)
    sig("libxsmm_mmbatch_blas", i, *batch_args)
    grp = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    sig("libxsmm_dgemm_batch", None, *grp)
    sig("libxsmm_sgemm_batch", None, *grp)
    sig("libxsmm_mmbatch_begin", None, i, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, vp, vp)
    sig("libxsmm_mmbatch_end", None)
    gemm = [C.c_char_p, C.c_char_p, c_int_p, c_int_p, c_int_p, vp, vp, c_int_p, vp, c_int_p, vp, vp, c_int_p]
    sig("libxsmm_dgemm", None, *gemm)
    sig("libxsmm_sgemm", None, *gemm)
    sig("libxsmm_blas_dgemm", None, *gemm)
    sig("libxsmm_blas_sgemm", None, *gemm)
    sig("libxsmm_dfsspmdm_create", vp, i, i, i, i, i, i, C.c_double, C.c_double, vp)
    sig("libxsmm_dfsspmdm_execute", None, vp, vp, vp)
    sig("libxsmm_dfsspmdm_destroy", None, vp)
    sig("libxsmm_sfsspmdm_create", vp, i, i, i, i, i, i, C.c_float, C.c_float, vp)
    sig("libxsmm_sfsspmdm_execute", None, vp, vp, vp)
    sig("libxsmm_sfsspmdm_destroy", None, vp)
    sig("libxsmm_amd_dfsspmdm_execute_batch", i, vp, vp, vp, ll)
    sig("libxsmm_amd_sfsspmdm_execute_batch", i, vp, vp, vp, ll)
    sig("libxsmm_spmdm_init", None, i, i, i, i, C.POINTER(SpmdmHandle), C.POINTER(C.POINTER(CSRSlice)))
    sig("libxsmm_spmdm_destroy", None, C.POINTER(SpmdmHandle))
    sig("libxsmm_spmdm_get_num_createSparseSlice_blocks", i, C.POINTER(SpmdmHandle))
    sig("libxsmm_spmdm_get_num_compute_blocks", i, C.POINTER(SpmdmHandle))
    sig("libxsmm_spmdm_createSparseSlice_fp32_thread", None, C.POINTER(SpmdmHandle), C.c_char, vp, C.POINTER(CSRSlice), i, i, i)
    sig("libxsmm_spmdm_compute_fp32_thread", None, C.POINTER(SpmdmHandle), C.c_char, C.c_char, vp, C.POINTER(CSRSlice), vp,
        C.c_char, vp, vp, i, i, i)
    sig("libxsmm_spmdm_createSparseSlice_bfloat16_thread", None, C.POINTER(SpmdmHandle), C.c_char, vp, C.POINTER(CSRSlice), i, i, i)
    sig("libxsmm_spmdm_compute_bfloat16_thread", None, C.POINTER(SpmdmHandle), C.c_char, C.c_char, vp, C.POINTER(CSRSlice), vp,
        C.c_char, vp, vp, i, i, i)
    sig("libxsmm_amd_memcpy_h2d", i, vp, vp, C.c_size_t)
    sig("libxsmm_amd_memcpy_d2h", i, vp, vp, C.c_size_t)
    sig("libxsmm_amd_spmdm_createSparseSlice_all", i, C.POINTER(SpmdmHandle), C.c_char, vp, C.POINTER(CSRSlice))
    sig("libxsmm_amd_spmdm_compute_all", i, C.POINTER(SpmdmHandle), C.c_char, C.c_char, vp, C.POINTER(CSRSlice), vp, C.c_char, vp, vp)
    sig("libxsmm_amd_spmdm_createSparseSlice_bfloat16_all", i, C.POINTER(SpmdmHandle), C.c_char, vp, C.POINTER(CSRSlice))
    sig("libxsmm_amd_spmdm_compute_bfloat16_all", i, C.POINTER(SpmdmHandle), C.c_char, C.c_char, vp, C.POINTER(CSRSlice), vp, C.c_char, vp, vp)
    sig("libxsmm_amd_spmdm_batch_create", vp, i, i, i, ll)
    sig("libxsmm_amd_spmdm_batch_destroy", None, vp)
    sig("libxsmm_amd_spmdm_batch_create_slices", i, vp, C.c_char, vp)
    sig("libxsmm_amd_spmdm_batch_compute", i, vp, C.c_char, vp, C.c_char, vp, vp)
    sig("libxsmm_amd_spmdm_batch_get_slice", i, vp, ll, vp, vp, vp, i)
    sig("libxsmm_blocked_gemm_handle_create", vp, i, i, i, i, i, i, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p,
        vp, vp, c_int_p, c_int_p, c_int_p)
    sig("libxsmm_blocked_gemm_handle_destroy", None, vp)
    for nm in ("copyin_a", "copyin_b", "copyin_c", "copyout_c", "convert_b_to_a", "transpose_b"):
        sig("libxsmm_blocked_gemm_" + nm, i, vp, vp, c_int_p, vp)
    sig("libxsmm_blocked_gemm_st", None, vp, vp, vp, vp, i, i)
    sig("libxsmm_blocked_gemm_omp", None, vp, vp, vp, vp, i)
    sig("libxsmm_malloc", vp, C.c_size_t)
    sig("libxsmm_aligned_malloc", vp, C.c_size_t, C.c_size_t)
    sig("libxsmm_free", None, vp)
    sig("libxsmm_typesize", C.c_ubyte, i)
    sig("libxsmm_timer_tick", C.c_ulonglong)
    sig("libxsmm_timer_duration", C.c_double, C.c_ulonglong, C.c_ulonglong)
    sig("libxsmm_rng_set_seed", None, C.c_uint)
    sig("libxsmm_rng_f64", C.c_double)
    sig("libxsmm_rng_u32", C.c_uint, C.c_uint)
    sig("libxsmm_isqrt_u64", C.c_uint, C.c_ulonglong)
    sig("libxsmm_shuffle", C.c_size_t, C.c_uint)
    sig("libxsmm_matdiff", i, C.POINTER(MatdiffInfo), i, i, i, vp, vp, c_int_p, c_int_p)
    sig("libxsmm_matdiff_clear", None, C.POINTER(MatdiffInfo))
    sig("libxsmm_matdiff_reduce", None, C.POINTER(MatdiffInfo), C.POINTER(MatdiffInfo))
    sig("libxsmm_amd_device_count", i)
    sig("libxsmm_amd_set_stream", None, vp)
    sig("libxsmm_amd_get_stream", vp)
    sig("libxsmm_amd_synchronize", i)
    sig("libxsmm_amd_set_mfma", i, i)
    sig("libxsmm_amd_get_mfma", i)
    sig("libxsmm_amd_last_kernel", C.c_char_p)
    sig("libxsmm_amd_launch_count", C.c_ulonglong)
    sig("libxsmm_amd_jit_launch_count", C.c_ulonglong)
    sig("libxsmm_amd_flush", None)
    sig("libxsmm_amd_defer_begin", None)
    sig("libxsmm_amd_defer_end", None)
    sig("libxsmm_amd_defer_active", i)
    ull_p = C.POINTER(C.c_ulonglong)
    sig("libxsmm_amd_merge_segments", i, i, ull_p, c_int_p)
    sig("libxsmm_amd_merge_last_plan", i, c_int_p, c_int_p, c_int_p, ull_p, c_int_p, i)
    sig("libxsmm_amd_smm_plan_describe", i, vp, i, i, ll, ll, ll, ll, C.c_uint, i, ll, i, i, vp, C.c_size_t, i)
    sig("libxsmm_amd_is_device_pointer", i, vp)
    sig("libxsmm_amd_gemm_batch_strided", i, vp, vp, vp, vp, ll, ll, ll, ll)
    sig("libxsmm_amd_stream_probe", i, vp, vp, vp, ll)
    sig("libxsmm_amd_csr_kernel_source", i, i, i, i, vp, vp, vp, i, i, vp, C.c_size_t, i)
    gc = C.POINTER(GeneratedCode)
    sig("libxsmm_strerror", C.c_char_p, C.c_uint)
    sig("libxsmm_generator_gemm_kernel", None, gc, vp, C.c_char_p)
    sig("libxsmm_generator_gemm_inlineasm", None, C.c_char_p, C.c_char_p, vp, C.c_char_p)
    sig("libxsmm_generator_gemm_directasm", None, C.c_char_p, C.c_char_p, vp, C.c_char_p)
    sig("libxsmm_generator_spgemm", None, C.c_char_p, C.c_char_p, vp, C.c_char_p, C.c_char_p, i)
    for nm in ("csr", "csc", "csr_reg"):
        sig("libxsmm_generator_spgemm_%s_kernel" % nm, None, gc, vp, C.c_char_p, vp, vp, vp)
    for nm in ("csr_soa", "csc_soa"):
        sig("libxsmm_generator_spgemm_%s_kernel" % nm, None, gc, vp, C.c_char_p, vp, vp, vp)
    sig("libxsmm_create_xcsr_soa", vp, vp, vp, vp, vp)
    sig("libxsmm_create_xcsc_soa", vp, vp, vp, vp, vp)
    sig("libxsmm_create_rm_ac_soa", vp, vp)
    sig("libxsmm_create_rm_bc_soa", vp, vp)
    sig("libxsmm_amd_soa_width", i, i)
    sig("libxsmm_amd_sparse_reader", i, C.c_char_p, i, C.POINTER(C.POINTER(C.c_uint)), C.POINTER(C.POINTER(C.c_uint)), C.POINTER(C.POINTER(C.c_double)),
        C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint))
    sig("libxsmm_amd_kernel_execute_batch", i, vp, vp, vp, vp, ll, ll, ll)
    sig("libxsmm_amd_spgemm_create", vp, vp, i, vp, vp, i)
    sig("libxsmm_amd_spgemm_execute_batch", i, vp, vp, vp, vp, ll, ll, ll)
    sig("libxsmm_amd_spgemm_destroy", None, vp)
    sig("libxsmm_amd_spgemm_source", i, vp, i, vp, vp, i, vp, C.c_size_t, i)
    sig("libxsmm_amd_soa_source", i, vp, i, vp, vp, i, vp, C.c_size_t, i)
    sig("libxsmm_amd_smm_kernel_source", i, vp, i, vp, C.c_size_t, i)
    sig("libxsmm_amd_device_malloc", vp, C.c_size_t)
    sig("libxsmm_amd_device_free", None, vp)
    sig("libxsmm_amd_smm_grouped_kernel_source", i, C.POINTER(vp), i, vp, C.c_size_t, i)
    sig("libxsmm_amd_jit_prebuild", i, C.POINTER(vp), i, i)
    sig("libxsmm_amd_jit_wait", None)
    sig("libxsmm_amd_jit_drain", None)
    u = C.c_uint
    for nm in ("trsm", "trmm"):
        sig("libxsmm_%s_descriptor_init" % nm, vp, C.POINTER(DescriptorBlob), u, i, i, i, i, vp, C.c_char, C.c_char, C.c_char, C.c_char, i)
    sig("libxsmm_pgemm_descriptor_init", vp, C.POINTER(DescriptorBlob), u, i, i, i, i, i, i, vp, C.c_char, C.c_char, i)
    sig("libxsmm_getrf_descriptor_init", vp, C.POINTER(DescriptorBlob), u, i, i, i, i)
    for nm in ("pgemm", "getrf", "trmm", "trsm"):
        sig("libxsmm_dispatch_" + nm, vp, vp)
    sig("libxsmm_amd_packed_width", i, u)
    sig("libxsmm_amd_packed_execute_batch", i, vp, vp, vp, vp, ll)
    sig("libxsmm_amd_packed_kernel_source", i, vp, i, vp, C.c_size_t, i)
    sig("libxsmm_trans_descriptor_init", vp, C.POINTER(DescriptorBlob), u, u, u, u)
    sig("libxsmm_mcopy_descriptor_init", vp, C.POINTER(DescriptorBlob), u, u, u, u, u, i, i, c_int_p)
    sig("libxsmm_dispatch_mcopy", vp, vp)
    sig("libxsmm_dispatch_trans", vp, vp)
    sig("libxsmm_get_transkernel_info", i, vp, C.POINTER(TransKernelInfo), C.POINTER(C.c_size_t))
    sig("libxsmm_get_mcopykernel_info", i, vp, C.POINTER(McopyKernelInfo), C.POINTER(C.c_size_t))
    for nm in ("libxsmm_matcopy", "libxsmm_matcopy_omp"):
        sig(nm, None, vp, vp, u, i, i, i, i, c_int_p)
    sig("libxsmm_matcopy_thread", None, vp, vp, u, i, i, i, i, c_int_p, i, i)
    for nm in ("libxsmm_otrans", "libxsmm_otrans_omp"):
        sig(nm, None, vp, vp, u, i, i, i, i)
    sig("libxsmm_otrans_thread", None, vp, vp, u, i, i, i, i, i, i)
    sig("libxsmm_itrans", None, vp, u, i, i, i)
    for nm in ("libxsmm_amd_matcopy_batch", "libxsmm_amd_otrans_batch"):
        sig(nm, i, vp, vp, u, i, i, i, i, ll, ll, ll)
    for nm in ("libxsmm_amd_matcopy_batch_ptr", "libxsmm_amd_otrans_batch_ptr"):
        sig(nm, i, vp, vp, u, i, i, i, i, ll)
    # tiled GEMM (include/libxsmm.h; the partition query and the tile extent in include/libxsmm_amd.h)
    sig("libxsmm_gemm_handle_init", vp, vp, i, i, C.c_char_p, C.c_char_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, vp, vp, i, i)
    sig("libxsmm_gemm_handle_get_scratch_size", C.c_size_t, vp)
    sig("libxsmm_gemm_thread", None, vp, vp, vp, vp, vp, i, i)
    sig("libxsmm_xgemm_omp", None, i, i, C.c_char_p, C.c_char_p, c_int_p, c_int_p, c_int_p, vp, vp, c_int_p, vp, c_int_p, vp, vp, c_int_p)
    sig("libxsmm_amd_gemm_task", i, vp, i, i, C.POINTER(C.c_uint))
    sig("libxsmm_amd_gemm_tile", i)
    # GEMM with 16-bit inputs (front ends in include/libxsmm.h, the one-layout entry in include/libxsmm_amd.h)
    for nm in ("libxsmm_wigemm", "libxsmm_wsgemm", "libxsmm_bsgemm"):
        sig(nm, None, *gemm)
    lowp = [i, i, C.c_char, C.c_char, i, i, i, vp, i, vp, i, i, vp, i]
    sig("libxsmm_amd_lowp_gemm", i, *lowp)
    sig("libxsmm_amd_lowp_gemm_thread", i, *(lowp + [i, i]))
    sig("libxsmm_amd_set_lowp_fast", i, i)
    sig("libxsmm_amd_get_lowp_fast", i)
    sig("libxsmm_amd_lowp_gemm_chunk", i, i)
    # quantisation and bf16 conversion (include/libxsmm_dnn.h; the stream-ordered forms in include/libxsmm_amd.h)
    ub = C.c_ubyte
    sig("libxsmm_sexp2_u8", C.c_float, ub)
    sig("libxsmm_sexp2_i8", C.c_float, C.c_byte)
    sig("libxsmm_sexp2_i8i", C.c_float, i)
    sig("libxsmm_dnn_quantize", None, vp, vp, i, ub, vp, i)
    sig("libxsmm_dnn_quantize_act", None, vp, vp, u, u, u, u, u, u, u, ub, vp, i)
    sig("libxsmm_dnn_quantize_fil", None, vp, vp, u, u, u, u, u, u, u, u, u, ub, vp, i)
    sig("libxsmm_amd_dnn_quantize_async", i, vp, vp, i, ub, vp, i)
    sig("libxsmm_amd_dnn_quantize_act_async", i, vp, vp, u, u, u, u, u, u, u, ub, vp, i)
    sig("libxsmm_amd_dnn_quantize_fil_async", i, vp, vp, u, u, u, u, u, u, u, u, u, ub, vp, i)
    sig("libxsmm_amd_dnn_quantize_set_seed", None, u)
    sig("libxsmm_dnn_dequantize", None, vp, vp, i, ub)
    for nm in ("libxsmm_truncate_convert_f32_bf16", "libxsmm_rnaz_convert_fp32_bfp16", "libxsmm_rne_convert_fp32_bfp16", "libxsmm_convert_bf16_f32"):
        sig(nm, None, vp, vp, u)
    # DNN tensors and the fully-connected layer (include/libxsmm_dnn.h, include/libxsmm_dnn_fullyconnected.h)
    up = C.POINTER(C.c_uint)
    lp = C.POINTER(TensorDatalayout)
    sig("libxsmm_dnn_get_error", C.c_char_p, u)
    sig("libxsmm_dnn_typesize", C.c_size_t, i)
    sig("libxsmm_dnn_link_tensor", vp, lp, vp, up)
    sig("libxsmm_dnn_link_qtensor", vp, lp, vp, ub, up)
    sig("libxsmm_dnn_destroy_tensor", u, vp)
    sig("libxsmm_dnn_destroy_tensor_datalayout", u, lp)
    sig("libxsmm_dnn_duplicate_tensor_datalayout", lp, lp, up)
    sig("libxsmm_dnn_compare_tensor_datalayout", u, lp, lp, up)
    sig("libxsmm_dnn_get_tensor_size", u, lp, up)
    sig("libxsmm_dnn_get_tensor_elements", u, lp, up)
    sig("libxsmm_dnn_set_tensor_data_ptr", u, vp, vp)
    sig("libxsmm_dnn_get_tensor_data_ptr", vp, vp, up)
    sig("libxsmm_dnn_get_tensor_datalayout", lp, vp, up)
    sig("libxsmm_dnn_get_qtensor_scf", ub, vp, up)
    sig("libxsmm_dnn_set_qtensor_scf", u, vp, ub)
    sig("libxsmm_dnn_zero_tensor", u, vp)
    sig("libxsmm_dnn_copyin_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_copyout_tensor", u, vp, vp, i)
    sig("libxsmm_amd_dnn_copyin_tensor_async", u, vp, vp, i)
    sig("libxsmm_amd_dnn_copyout_tensor_async", u, vp, vp, i)
    sig("libxsmm_amd_dnn_copy_plan", u, lp, i, i, C.POINTER(C.c_longlong))
    sig("libxsmm_dnn_create_fullyconnected", vp, FullyconnectedDesc, up)
    sig("libxsmm_dnn_destroy_fullyconnected", u, vp)
    sig("libxsmm_dnn_fullyconnected_create_tensor_datalayout", lp, vp, i, up)
    sig("libxsmm_dnn_fullyconnected_get_scratch_size", C.c_size_t, vp, up)
    sig("libxsmm_dnn_fullyconnected_bind_scratch", u, vp, vp)
    sig("libxsmm_dnn_fullyconnected_release_scratch", u, vp)
    sig("libxsmm_dnn_fullyconnected_bind_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_fullyconnected_get_tensor", vp, vp, i, up)
    sig("libxsmm_dnn_fullyconnected_release_tensor", u, vp, i)
    sig("libxsmm_dnn_fullyconnected_execute_st", u, vp, i, i, i)
    # the pooling layer (include/libxsmm_dnn_pooling.h)
    sig("libxsmm_dnn_create_pooling", vp, PoolingDesc, up)
    sig("libxsmm_dnn_destroy_pooling", u, vp)
    sig("libxsmm_dnn_pooling_create_tensor_datalayout", lp, vp, i, up)
    sig("libxsmm_dnn_pooling_get_scratch_size", C.c_size_t, vp, up)
    sig("libxsmm_dnn_pooling_bind_scratch", u, vp, vp)
    sig("libxsmm_dnn_pooling_release_scratch", u, vp)
    sig("libxsmm_dnn_pooling_bind_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_pooling_get_tensor", vp, vp, i, up)
    sig("libxsmm_dnn_pooling_release_tensor", u, vp, i)
    sig("libxsmm_dnn_pooling_execute_st", u, vp, i, i, i)
    # the fused batch-norm layer (include/libxsmm_dnn_fusedbatchnorm.h)
    sig("libxsmm_dnn_create_fusedbatchnorm", vp, FusedBatchnormDesc, up)
    sig("libxsmm_dnn_destroy_fusedbatchnorm", u, vp)
    sig("libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout", lp, vp, i, up)
    sig("libxsmm_dnn_fusedbatchnorm_get_scratch_size", C.c_size_t, vp, up)
    sig("libxsmm_dnn_fusedbatchnorm_bind_scratch", u, vp, vp)
    sig("libxsmm_dnn_fusedbatchnorm_release_scratch", u, vp)
    sig("libxsmm_dnn_fusedbatchnorm_bind_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_fusedbatchnorm_get_tensor", vp, vp, i, up)
    sig("libxsmm_dnn_fusedbatchnorm_release_tensor", u, vp, i)
    sig("libxsmm_dnn_fusedbatchnorm_execute_st", u, vp, i, i, i)
    # the convolution layer (include/libxsmm_dnn_convolution.h)
    sig("libxsmm_dnn_create_conv_layer", vp, ConvDesc, up)
    sig("libxsmm_dnn_destroy_conv_layer", u, vp)
    sig("libxsmm_dnn_create_tensor_datalayout", lp, vp, i, up)
    sig("libxsmm_dnn_trans_reg_filter", u, vp)
    sig("libxsmm_dnn_get_scratch_size", C.c_size_t, vp, i, up)
    sig("libxsmm_dnn_bind_scratch", u, vp, i, vp)
    sig("libxsmm_dnn_release_scratch", u, vp, i)
    sig("libxsmm_dnn_bind_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_get_tensor", vp, vp, i, up)
    sig("libxsmm_dnn_release_tensor", u, vp, i)
    sig("libxsmm_dnn_execute", None, vp, i)
    sig("libxsmm_dnn_execute_st", u, vp, i, i, i)
    sig("libxsmm_dnn_transpose_filter", u, vp, i)
    sig("libxsmm_dnn_reduce_wu_filters", u, vp, i)
    sig("libxsmm_dnn_get_codegen_success", u, vp, i)
    sig("libxsmm_dnn_get_parallel_tasks", u, vp, i, up)
    # the RNN cell layer (include/libxsmm_dnn_rnncell.h)
    sig("libxsmm_dnn_create_rnncell", vp, RnncellDesc, up)
    sig("libxsmm_dnn_destroy_rnncell", u, vp)
    sig("libxsmm_dnn_rnncell_create_tensor_datalayout", lp, vp, i, up)
    sig("libxsmm_dnn_rnncell_get_scratch_size", C.c_size_t, vp, i, up)
    sig("libxsmm_dnn_rnncell_get_scratch_ptr", vp, vp, up)
    sig("libxsmm_dnn_rnncell_bind_scratch", u, vp, i, vp)
    sig("libxsmm_dnn_rnncell_release_scratch", u, vp, i)
    sig("libxsmm_dnn_rnncell_get_internalstate_size", C.c_size_t, vp, i, up)
    sig("libxsmm_dnn_rnncell_get_internalstate_ptr", vp, vp, up)
    sig("libxsmm_dnn_rnncell_bind_internalstate", u, vp, i, vp)
    sig("libxsmm_dnn_rnncell_release_internalstate", u, vp, i)
    sig("libxsmm_dnn_rnncell_allocate_forget_bias", u, vp, C.c_float)
    sig("libxsmm_dnn_rnncell_bind_tensor", u, vp, vp, i)
    sig("libxsmm_dnn_rnncell_get_tensor", vp, vp, i, up)
    sig("libxsmm_dnn_rnncell_release_tensor", u, vp, i)
    sig("libxsmm_dnn_rnncell_set_sequence_length", u, vp, i)
    sig("libxsmm_dnn_rnncell_get_sequence_length", i, vp, up)
    sig("libxsmm_dnn_rnncell_execute_st", u, vp, i, i, i)
    sig("libxsmm_amd_rnn_segments", i, i, i, i, i, i, i, c_int_p, i)
    sig("libxsmm_amd_rnn_bwd_segments", i, i, i, i, c_int_p, i)
    # matdiff on device operands
    sig("libxsmm_amd_matdiff_async", i, C.POINTER(MatdiffInfo), i, i, i, vp, vp, c_int_p, c_int_p)
    sig("libxsmm_amd_matdiff_batch", i, C.POINTER(MatdiffInfo), C.POINTER(MatdiffInfo), C.POINTER(ll), i, i, i, vp, vp, c_int_p, c_int_p, ll, ll, ll)
    # hash and byte compare
    sig("libxsmm_hash", u, vp, u, u)
    sig("libxsmm_memcmp", i, vp, vp, C.c_size_t)
    sig("libxsmm_diff", C.c_ubyte, vp, vp, C.c_ubyte)
    sig("libxsmm_diff_n", u, vp, vp, C.c_ubyte, C.c_ubyte, u, u)
    sig("libxsmm_amd_hash_async", i, vp, vp, C.c_size_t, u)
    sig("libxsmm_amd_hash_batch", i, vp, vp, C.c_size_t, ll, ll, ll, ll, u)
    sig("libxsmm_amd_memcmp_async", i, vp, vp, vp, C.c_size_t)
    sig("libxsmm_amd_memcmp_batch", i, vp, vp, vp, vp, C.c_size_t, ll, ll, ll, ll, ll, ll)
    sig("libxsmm_amd_gemm_batch_groups", i, i, i, i, C.c_char_p, C.c_char_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, vp, vp,
        C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), c_int_p, i)


# ---- thin helpers used by tests and bench (argument marshalling only) -------------------------------------------------
def iptr(v):
    """pointer to a C int holding v (or NULL)"""
    return None if v is None else C.byref(C.c_int(int(v)))


def dptr(t):
    """raw pointer of a torch tensor / numpy array / int"""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    if hasattr(t, "ctypes"):
        return C.c_void_p(t.ctypes.data)
    return C.c_void_p(int(t))


def descriptor(prec, m, n, k, lda=None, ldb=None, ldc=None, alpha=1.0, beta=1.0, flags=0, prefetch=0):
    """libxsmm_gemm_descriptor_dinit -> (blob, pointer); pointer is None when the reference would return NULL."""
    blob = DescriptorBlob()
    lda = m if lda is None else lda
    ldb = (n if (flags & FLAG_TRANS_B) else k) if ldb is None else ldb
    ldc = m if ldc is None else ldc
    p = lib().libxsmm_gemm_descriptor_dinit(C.byref(blob), prec, m, n, k, lda, ldb, ldc, alpha, beta, flags, prefetch)
    return blob, p


def gemm_batch(prec, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, index_base, index_stride,
               stride_a, stride_b, stride_c, batchsize, omp=False):
    """libxsmm_gemm_batch[_omp]; alpha/beta are Python floats (or None), a/b/c/stride_* tensors, arrays or addresses."""
    ct = C.c_double if prec == F64 else C.c_float
    al = None if alpha is None else C.byref(ct(alpha))
    be = None if beta is None else C.byref(ct(beta))
    f = lib().libxsmm_gemm_batch_omp if omp else lib().libxsmm_gemm_batch
    f(prec, prec, C.c_char_p(transa.encode()) if transa else None, C.c_char_p(transb.encode()) if transb else None,
      m, n, k, al, dptr(a), iptr(lda), dptr(b), iptr(ldb), be, dptr(c), iptr(ldc), index_base, index_stride,
      dptr(stride_a), dptr(stride_b), dptr(stride_c), batchsize)


def read_mtx(path, is_csr):
    """libxsmm_amd_sparse_reader -> (error code, ptr, idx, values, rows, cols, nnz) as numpy arrays (None on error)"""
    import numpy as np
    ptr, idx, val = C.POINTER(C.c_uint)(), C.POINTER(C.c_uint)(), C.POINTER(C.c_double)()
    r, c, z = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    rc = lib().libxsmm_amd_sparse_reader(str(path).encode(), 1 if is_csr else 0, C.byref(ptr), C.byref(idx), C.byref(val), C.byref(r), C.byref(c), C.byref(z))
    if 0 != rc:
        assert not ptr and not idx and not val
        return rc, None, None, None, 0, 0, 0
    nmajor = r.value if is_csr else c.value
    out = (rc, np.ctypeslib.as_array(ptr, (nmajor + 1,)).copy(), np.ctypeslib.as_array(idx, (z.value,)).copy(),
           np.ctypeslib.as_array(val, (z.value,)).copy(), r.value, c.value, z.value)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for p in (ptr, idx, val):
        libc.free(C.cast(p, C.c_void_p))
    return out


def gemm_batch_groups(prec, shapes, a, b, c, stride_a, stride_b, stride_c, sizes, index_base=0, index_stride=4, beta=1.0, relaxed=False,
                      transa=None, transb=None, lda=None, ldb=None, ldc=None):
    """libxsmm_amd_gemm_batch_groups: shapes = [(m, n, k)], a/b/c/stride_* = per-group tensors / arrays, sizes = per-group batch sizes;
    transa/transb = per-group 'N'/'T' (a string or a list), lda/ldb/ldc = per-group leading dimensions (None: the library's default)"""
    n = len(shapes)
    ints = lambda v: (C.c_int * n)(*[int(x) for x in v])
    ptrs = lambda v: (C.c_void_p * n)(*[dptr(x).value if x is not None else None for x in v])
    chars = lambda v: None if v is None else C.c_char_p("".join(v).encode())
    lds = lambda v: None if v is None else ints(v)
    assert all(v is None or len(v) == n for v in (transa, transb, lda, ldb, ldc)), "one entry per group"
    ct = C.c_double if prec == F64 else C.c_float
    be = ct(beta)
    return lib().libxsmm_amd_gemm_batch_groups(prec, prec, n, chars(transa), chars(transb), ints(s[0] for s in shapes), ints(s[1] for s in shapes),
                                               ints(s[2] for s in shapes), lds(lda), lds(ldb), lds(ldc), None, C.byref(be), ptrs(a), ptrs(b), ptrs(c),
                                               index_base, index_stride, ptrs(stride_a), ptrs(stride_b), ptrs(stride_c), ints(sizes), 1 if relaxed else 0)


def defer_begin():
    """libxsmm_amd_defer_begin: per-product kernel calls, spmdm block calls and batch calls of this thread are recorded (brackets nest)"""
    lib().libxsmm_amd_defer_begin()


def defer_end():
    """libxsmm_amd_defer_end: the outermost one launches what was recorded"""
    lib().libxsmm_amd_defer_end()


def flush():
    """libxsmm_amd_flush: launches what was recorded, the bracket stays open"""
    lib().libxsmm_amd_flush()


def merge_segments(hulls):
    """libxsmm_amd_merge_segments: hulls = per call (a_lo, a_hi, b_lo, b_hi, c_lo, c_hi), half-open byte ranges -> (number of segments,
    [segment of call i])"""
    n = len(hulls)
    flat = (C.c_ulonglong * max(1, 6 * n))(*[int(v) for h in hulls for v in h])
    seg = (C.c_int * max(1, n))()
    count = lib().libxsmm_amd_merge_segments(n, flat, seg)
    return count, [seg[j] for j in range(n)]


def merge_last_plan(capacity=64):
    """libxsmm_amd_merge_last_plan -> dict(calls, segments, device_hulls, hulls=[6-tuples], segment_of=[...]) of this thread's last flush"""
    nc, ns, nd = C.c_int(0), C.c_int(0), C.c_int(0)
    flat = (C.c_ulonglong * (6 * capacity))()
    seg = (C.c_int * capacity)()
    m = lib().libxsmm_amd_merge_last_plan(C.byref(nc), C.byref(ns), C.byref(nd), flat, seg, capacity)
    return dict(calls=nc.value, segments=ns.value, device_hulls=nd.value, hulls=[tuple(flat[6 * j + o] for o in range(6)) for j in range(m)],
                segment_of=[seg[j] for j in range(m)])


ADDR_STRIDED, ADDR_INDEX, ADDR_POINTER = 0, 1, 2  # how a batch addresses its items
SYNC_NONE, SYNC_RUNS, SYNC_DEVICE = 0, 1, 3       # every item its own C; C in runs the host knows of; the verdict on the device


def smm_plan(desc, mode, sync, batch, strides=(0, 0, 0), address_bits=0, relaxed=False, uniform_run=0, mfma=1, lowp=0, compile_tiles=False):
    """libxsmm_amd_smm_plan_describe -> [dict(pos, tier, name, parts=[(variant bits, slice)], tiles=[(m, n, variant bits)])], one per
    alternative in the order a batch call tries them (diagnostic: no device needed)"""
    buf = C.create_string_buffer(1 << 12)
    rc = lib().libxsmm_amd_smm_plan_describe(desc, mode, sync, batch, strides[0], strides[1], strides[2], address_bits, 1 if relaxed else 0,
                                             uniform_run, mfma, lowp, buf, len(buf), 1 if compile_tiles else 0)
    if rc < 0:
        raise RuntimeError("libxsmm_amd_smm_plan_describe: %d" % rc)
    plan = []
    for line in buf.value.decode().splitlines():
        w = line.split()
        nparts = int(w[3].split("=")[1])
        parts = [(int(x.split(":")[0]), x.split(":")[1]) for x in w[4:4 + nparts]]
        ntiles = int(w[4 + nparts].split("=")[1])
        tiles = [(int(x.split(":")[0].split("x")[0]), int(x.split(":")[0].split("x")[1]), int(x.split(":")[1])) for x in w[5 + nparts:5 + nparts + ntiles]]
        plan.append(dict(pos=int(w[0]), tier=w[1], name=w[2], parts=parts, tiles=tiles))
    return plan


# ---- packed kernels (libxsmm_dispatch_pgemm / getrf / trmm / trsm) ------------------------------------------------------
KIND_PGEMM, KIND_GETRF, KIND_TRMM, KIND_TRSM = 3, 4, 5, 6  # libxsmm_kernel_kind
COL_MAJOR, ROW_MAJOR = 102, 101


def packed_width(typesize):
    """libxsmm_amd_packed_width: matrices per pack (8 for fp64, 16 for fp32)"""
    return lib().libxsmm_amd_packed_width(typesize)


def packed_descriptor(kind, typesize, m, n, k=0, lda=None, ldb=None, ldc=None, alpha=1.0, transa="N", transb="N", side="L", uplo="L",
                      diag="N", layout=COL_MAJOR):
    """libxsmm_{pgemm,getrf,trmm,trsm}_descriptor_init -> (blob, pointer); leading dimensions default to the tight ones"""
    blob = DescriptorBlob()
    ct = C.c_double if typesize == 8 else C.c_float
    al = C.byref(ct(alpha)) if alpha is not None else None
    lead = lambda rows, cols: rows if layout == COL_MAJOR else cols
    ch = lambda c: c.encode()
    L = lib()
    if kind == KIND_PGEMM:
        ar, ac = (k, m) if transa in "Tt" else (m, k)
        br, bc = (n, k) if transb in "Tt" else (k, n)
        p = L.libxsmm_pgemm_descriptor_init(C.byref(blob), typesize, m, n, k, lead(ar, ac) if lda is None else lda,
                                            lead(br, bc) if ldb is None else ldb, lead(m, n) if ldc is None else ldc, al, ch(transa), ch(transb), layout)
    elif kind == KIND_GETRF:
        p = L.libxsmm_getrf_descriptor_init(C.byref(blob), typesize, m, n, lead(m, n) if lda is None else lda, layout)
    else:
        nt = n if side in "Rr" else m
        init = L.libxsmm_trmm_descriptor_init if kind == KIND_TRMM else L.libxsmm_trsm_descriptor_init
        p = init(C.byref(blob), typesize, m, n, nt if lda is None else lda, lead(m, n) if ldb is None else ldb, al, ch(transa), ch(diag), ch(side),
                 ch(uplo), layout)
    return blob, p


def packed_dispatch(kind, desc):
    """libxsmm_dispatch_{pgemm,getrf,trmm,trsm}: the kernel's function pointer, None outside the supported domain"""
    L = lib()
    return {KIND_PGEMM: L.libxsmm_dispatch_pgemm, KIND_GETRF: L.libxsmm_dispatch_getrf, KIND_TRMM: L.libxsmm_dispatch_trmm,
            KIND_TRSM: L.libxsmm_dispatch_trsm}[kind](desc)


def packed_execute_batch(fn_ptr, a, b, c, npacks):
    """libxsmm_amd_packed_execute_batch: npacks packs back to back, one launch"""
    return lib().libxsmm_amd_packed_execute_batch(fn_ptr, dptr(a), dptr(b), dptr(c), npacks)


def packed_kernel_source(kind, desc, compile=0, capacity=1 << 16):
    """libxsmm_amd_packed_kernel_source -> (return code, text)"""
    buf = C.create_string_buffer(capacity)
    rc = lib().libxsmm_amd_packed_kernel_source(desc, kind, buf, capacity, compile)
    return rc, buf.value.decode()


def pack(mats, ld, layout=COL_MAJOR, vlen=None, fill=0):
    """(nmat, rows, cols) array -> packed layout: element (i, j) of matrix v of pack p at [p][line][i or j][v] with `ld` elements per line
    (layout 102: a line is a column); nmat is rounded up to whole packs (the added matrices and the padding hold `fill`)"""
    import numpy as np
    mats = np.asarray(mats)
    nmat, rows, cols = mats.shape
    vlen = packed_width(mats.dtype.itemsize) if vlen is None else vlen
    npacks = (nmat + vlen - 1) // vlen
    nl, cd = (cols, rows) if layout == COL_MAJOR else (rows, cols)
    assert ld >= cd
    out = np.full((npacks, nl, ld, vlen), fill, dtype=mats.dtype)
    full = np.full((npacks * vlen, rows, cols), fill, dtype=mats.dtype)
    full[:nmat] = mats
    lines = full.transpose(0, 2, 1) if layout == COL_MAJOR else full  # (matrix, line, position in the line)
    out[:, :, :cd, :] = lines.reshape(npacks, vlen, nl, cd).transpose(0, 2, 3, 1)
    return out.reshape(-1)


def unpack(packed, nmat, rows, cols, ld, layout=COL_MAJOR, vlen=None):
    """the inverse of pack: -> (nmat, rows, cols)"""
    import numpy as np
    packed = np.asarray(packed)
    vlen = packed_width(packed.dtype.itemsize) if vlen is None else vlen
    npacks = (nmat + vlen - 1) // vlen
    nl, cd = (cols, rows) if layout == COL_MAJOR else (rows, cols)
    lines = packed.reshape(npacks, nl, ld, vlen)[:, :, :cd, :].transpose(0, 3, 1, 2).reshape(npacks * vlen, nl, cd)
    mats = lines.transpose(0, 2, 1) if layout == COL_MAJOR else lines
    return np.ascontiguousarray(mats[:nmat])


# ---- matrix copy and transposition (libxsmm_matcopy / otrans / itrans, libxsmm_dispatch_mcopy / _trans, stack forms) ------
KIND_MCOPY, KIND_TRANS = 1, 2  # libxsmm_kernel_kind
MATCOPY_FLAG_ZERO_SOURCE = 1


def matcopy(out, inp, typesize, m, n, ldi, ldo, prefetch=None, tid=None, nthreads=None, omp=False):
    """libxsmm_matcopy[_thread|_omp]: out[j*ldo+i] = in[j*ldi+i]; inp None zeroes the destination (tid given: the _thread form)"""
    L = lib()
    if tid is not None:
        L.libxsmm_matcopy_thread(dptr(out), dptr(inp), typesize, m, n, ldi, ldo, iptr(prefetch), tid, nthreads)
    else:
        (L.libxsmm_matcopy_omp if omp else L.libxsmm_matcopy)(dptr(out), dptr(inp), typesize, m, n, ldi, ldo, iptr(prefetch))


def otrans(out, inp, typesize, m, n, ldi, ldo, tid=None, nthreads=None, omp=False):
    """libxsmm_otrans[_thread|_omp]: out[i*ldo+j] = in[j*ldi+i] (tid given: the _thread form)"""
    L = lib()
    if tid is not None:
        L.libxsmm_otrans_thread(dptr(out), dptr(inp), typesize, m, n, ldi, ldo, tid, nthreads)
    else:
        (L.libxsmm_otrans_omp if omp else L.libxsmm_otrans)(dptr(out), dptr(inp), typesize, m, n, ldi, ldo)


def itrans(inout, typesize, m, n, ld):
    """libxsmm_itrans: in place, m == n"""
    lib().libxsmm_itrans(dptr(inout), typesize, m, n, ld)


def trans_descriptor(typesize, m, n, ldo):
    """libxsmm_trans_descriptor_init -> (blob, pointer)"""
    blob = DescriptorBlob()
    return blob, lib().libxsmm_trans_descriptor_init(C.byref(blob), typesize, m, n, ldo)


def mcopy_descriptor(typesize, m, n, ldo, ldi, flags=0, prefetch=0, unroll=None):
    """libxsmm_mcopy_descriptor_init -> (blob, pointer); pointer is None unless typesize is a multiple of 4"""
    blob = DescriptorBlob()
    return blob, lib().libxsmm_mcopy_descriptor_init(C.byref(blob), typesize, m, n, ldo, ldi, flags, prefetch, iptr(unroll))


def trans_dispatch(desc):
    """libxsmm_dispatch_trans: kernel(in, &ldi, out, &ldo), None for a NULL or unusable descriptor"""
    return lib().libxsmm_dispatch_trans(desc)


def mcopy_dispatch(desc):
    """libxsmm_dispatch_mcopy: kernel(in, &ldi, out, &ldo[, prefetch])"""
    return lib().libxsmm_dispatch_mcopy(desc)


def call_xcopy_kernel(fn_ptr, inp, ldi, out, ldo, prefetch=False):
    """Call a dispatched mcopy / trans kernel through its bare pointer (prefetch: pass a fifth argument, as matcopy callers may)."""
    li, lo = C.c_uint(ldi), C.c_uint(ldo)
    if prefetch:
        C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn_ptr)(dptr(inp), C.addressof(li), dptr(out), C.addressof(lo), dptr(inp))
    else:
        C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn_ptr)(dptr(inp), C.addressof(li), dptr(out), C.addressof(lo))


def matcopy_batch(out, inp, typesize, m, n, ldi, ldo, stride_in, stride_out, batch):
    """libxsmm_amd_matcopy_batch: `batch` items, strides in elements, one launch; inp None zeroes the items"""
    return lib().libxsmm_amd_matcopy_batch(dptr(out), dptr(inp), typesize, m, n, ldi, ldo, stride_in, stride_out, batch)


def otrans_batch(out, inp, typesize, m, n, ldi, ldo, stride_in, stride_out, batch):
    """libxsmm_amd_otrans_batch (out == inp with equal strides, ldi == ldo and m == n: every item in place)"""
    return lib().libxsmm_amd_otrans_batch(dptr(out), dptr(inp), typesize, m, n, ldi, ldo, stride_in, stride_out, batch)


def matcopy_batch_ptr(out_ptrs, in_ptrs, typesize, m, n, ldi, ldo, batch):
    """libxsmm_amd_matcopy_batch_ptr: arrays of item pointers (int64 numpy arrays or device tensors); in_ptrs None zeroes the items"""
    return lib().libxsmm_amd_matcopy_batch_ptr(dptr(out_ptrs), dptr(in_ptrs), typesize, m, n, ldi, ldo, batch)


def otrans_batch_ptr(out_ptrs, in_ptrs, typesize, m, n, ldi, ldo, batch):
    """libxsmm_amd_otrans_batch_ptr"""
    return lib().libxsmm_amd_otrans_batch_ptr(dptr(out_ptrs), dptr(in_ptrs), typesize, m, n, ldi, ldo, batch)


class GemmBlob(C.Structure):  # libxsmm_gemm_blob
    _fields_ = [("data", C.c_char * 128)]


def _scalar(prec, v):
    return None if v is None else C.byref(C.c_double(v) if prec == F64 else C.c_float(v))


def _trans(t):
    return None if t is None else t.encode()


def gemm_handle(iprec, oprec, transa, transb, m, n, k, lda=None, ldb=None, ldc=None, alpha=None, beta=None, flags=0, ntasks=1):
    """libxsmm_gemm_handle_init -> (blob, handle); handle is None where the call returns NULL. m, n, k, ld*: int or None."""
    blob = GemmBlob()
    h = lib().libxsmm_gemm_handle_init(C.byref(blob), iprec, oprec, _trans(transa), _trans(transb), iptr(m), iptr(n), iptr(k),
                                       iptr(lda), iptr(ldb), iptr(ldc), _scalar(iprec, alpha), _scalar(oprec, beta), flags, ntasks)
    return blob, h


def gemm_thread(handle, a, b, c, tid=0, nthreads=1, scratch=None):
    """libxsmm_gemm_thread"""
    lib().libxsmm_gemm_thread(handle, dptr(scratch), dptr(a), dptr(b), dptr(c), tid, nthreads)


def gemm_task(handle, tid, nthreads):
    """libxsmm_amd_gemm_task -> (return code, (m0, m1, n0, n1))"""
    rect = (C.c_uint * 4)()
    rc = lib().libxsmm_amd_gemm_task(handle, tid, nthreads, rect)
    return rc, tuple(rect)


def xgemm_omp(prec, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, oprec=None):
    """libxsmm_xgemm_omp (libxsmm_dgemm_omp / libxsmm_sgemm_omp are macros over it)"""
    oprec = prec if oprec is None else oprec
    lib().libxsmm_xgemm_omp(prec, oprec, _trans(transa), _trans(transb), iptr(m), iptr(n), iptr(k), _scalar(prec, alpha), dptr(a), iptr(lda),
                            dptr(b), iptr(ldb), _scalar(oprec, beta), dptr(c), iptr(ldc))


def call_kernel(fn_ptr, a, b, c, x3=None):
    """Call a dispatched kernel (bare function pointer) with three (or four) pointer arguments."""
    proto = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    proto(fn_ptr)(dptr(a), dptr(b), dptr(c), dptr(x3))


def last_kernel():
    return lib().libxsmm_amd_last_kernel().decode()


def gemm_lowp_thread(iprec, oprec, transa, transb, m, n, k, a, lda, b, ldb, beta, c, ldc, tid=0, nthreads=1):
    """libxsmm_amd_lowp_gemm_thread: plain column-major operands, (iprec, oprec) in (I16, I32), (I16, F32), (BF16, F32), beta 0 or 1"""
    return lib().libxsmm_amd_lowp_gemm_thread(iprec, oprec, transa.encode(), transb.encode(), m, n, k, dptr(a), lda, dptr(b), ldb, beta, dptr(c), ldc,
                                              tid, nthreads)


def gemm_lowp(iprec, oprec, transa, transb, m, n, k, a, lda, b, ldb, beta, c, ldc):
    """libxsmm_amd_lowp_gemm"""
    return lib().libxsmm_amd_lowp_gemm(iprec, oprec, transa.encode(), transb.encode(), m, n, k, dptr(a), lda, dptr(b), ldb, beta, dptr(c), ldc)


def set_lowp_fast(on):
    """libxsmm_amd_set_lowp_fast -> the previous value"""
    return lib().libxsmm_amd_set_lowp_fast(1 if on else 0)


def _lowp_front_end(name, ctype, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    sc = lambda v: None if v is None else C.byref(ctype(v))
    getattr(lib(), name)(_trans(transa), _trans(transb), iptr(m), iptr(n), iptr(k), sc(alpha), dptr(a), iptr(lda), dptr(b), iptr(ldb), sc(beta),
                         dptr(c), iptr(ldc))


def wigemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """libxsmm_wigemm (alpha, beta: Python ints or None)"""
    _lowp_front_end("libxsmm_wigemm", C.c_int, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)


def wsgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """libxsmm_wsgemm (alpha, beta: Python floats or None)"""
    _lowp_front_end("libxsmm_wsgemm", C.c_float, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)


def bsgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """libxsmm_bsgemm (alpha, beta: Python floats or None)"""
    _lowp_front_end("libxsmm_bsgemm", C.c_float, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc)


# ---- quantisation and bf16 conversion (include/libxsmm_dnn.h) ----------------------------------------------------------------
QUANT_NO_ROUND, QUANT_BIAS_ROUND, QUANT_STOCH_ROUND, QUANT_NEAREST_ROUND, QUANT_FPHW_ROUND = 80000, 80001, 80002, 80003, 80004


def _quantize(name, args, scf):
    """the reference form (scf None: the byte is returned) or the _async form (scf: one byte the GPU reaches; returns the status)"""
    if scf is not None:
        return getattr(lib(), "libxsmm_amd_" + name + "_async")(*(args[:-1] + [dptr(scf), args[-1]]))
    byte = C.c_ubyte(0xa5)
    getattr(lib(), "libxsmm_" + name)(*(args[:-1] + [C.cast(C.byref(byte), C.c_void_p), args[-1]]))
    return byte.value


def dnn_quantize(inp, out, length, add_shift, round_mode, scf=None):
    """libxsmm_dnn_quantize / libxsmm_amd_dnn_quantize_async"""
    return _quantize("dnn_quantize", [dptr(inp), dptr(out), length, add_shift, round_mode], scf)


def dnn_quantize_act(inp, out, N, Cc, H, W, cblk_f32, cblk_i16, lp_blk, add_shift, round_mode, scf=None):
    """libxsmm_dnn_quantize_act / libxsmm_amd_dnn_quantize_act_async"""
    return _quantize("dnn_quantize_act", [dptr(inp), dptr(out), N, Cc, H, W, cblk_f32, cblk_i16, lp_blk, add_shift, round_mode], scf)


def dnn_quantize_fil(inp, out, K, Cc, R, S, cblk_f32, cblk_i16, kblk_f32, kblk_i16, lp_blk, add_shift, round_mode, scf=None):
    """libxsmm_dnn_quantize_fil / libxsmm_amd_dnn_quantize_fil_async"""
    return _quantize("dnn_quantize_fil", [dptr(inp), dptr(out), K, Cc, R, S, cblk_f32, cblk_i16, kblk_f32, kblk_i16, lp_blk, add_shift, round_mode], scf)


def dnn_quantize_set_seed(seed):
    """libxsmm_amd_dnn_quantize_set_seed: 0 draws a seed per call"""
    lib().libxsmm_amd_dnn_quantize_set_seed(seed)


def dnn_dequantize(inp, out, length, scf):
    """libxsmm_dnn_dequantize"""
    lib().libxsmm_dnn_dequantize(dptr(inp), dptr(out), length, scf)


def convert_f32_bf16(inp, out, length, rounding="rne"):
    """libxsmm_truncate_convert_f32_bf16 / libxsmm_rnaz_convert_fp32_bfp16 / libxsmm_rne_convert_fp32_bfp16"""
    name = {"truncate": "libxsmm_truncate_convert_f32_bf16", "rnaz": "libxsmm_rnaz_convert_fp32_bfp16", "rne": "libxsmm_rne_convert_fp32_bfp16"}[rounding]
    getattr(lib(), name)(dptr(inp), dptr(out), length)


def convert_bf16_f32(inp, out, length):
    """libxsmm_convert_bf16_f32"""
    lib().libxsmm_convert_bf16_f32(dptr(inp), dptr(out), length)


# ---- matdiff on device operands (include/libxsmm_amd.h) --------------------------------------------------------------------------
MATDIFF_DATATYPES = {"torch.float64": F64, "torch.float32": F32, "torch.int32": 4, "torch.int16": 5, "torch.int8": 6,
                     "float64": F64, "float32": F32, "int32": 4, "int16": 5, "int8": 6}


def matdiff(ref, tst, m=None, n=None, ldref=None, ldtst=None, info=None):
    """libxsmm_matdiff on torch tensors (or numpy arrays) holding n lines of m elements, ld apart; returns the filled MatdiffInfo.
    m, n default to a 2-d operand's shape (n lines of m), or to a vector. info: memory the GPU reaches (a tensor of
    sizeof(MatdiffInfo) bytes) -- the call is libxsmm_amd_matdiff_async then and its status is returned instead."""
    x = ref if ref is not None else tst
    if m is None:
        m, n = (int(x.shape[-1]), int(x.shape[0])) if 2 == len(x.shape) else (int(x.numel() if hasattr(x, "numel") else x.size), 1)
    dt = MATDIFF_DATATYPES[str(x.dtype)]
    if info is not None:
        return lib().libxsmm_amd_matdiff_async(C.cast(dptr(info), C.POINTER(MatdiffInfo)), dt, m, n, dptr(ref), dptr(tst), iptr(ldref), iptr(ldtst))
    out = MatdiffInfo()
    rc = lib().libxsmm_matdiff(C.byref(out), dt, m, n, dptr(ref), dptr(tst), iptr(ldref), iptr(ldtst))
    if 0 != rc:
        raise RuntimeError("libxsmm_matdiff failed")
    return out


def matdiff_batch(ref, tst, dt, m, n, ldref, ldtst, stride_ref, stride_tst, batch, items=False, info=None):
    """libxsmm_amd_matdiff_batch; returns (status, info, list of item infos or None, item index)"""
    out = MatdiffInfo() if info is None else None
    arr = (MatdiffInfo * max(1, batch))() if items is True else None
    which = C.c_longlong(-2)
    pinfo = C.byref(out) if info is None else C.cast(dptr(info), C.POINTER(MatdiffInfo))
    pitems = arr if items is True else (None if items is None or items is False else C.cast(dptr(items), C.POINTER(MatdiffInfo)))
    rc = lib().libxsmm_amd_matdiff_batch(pinfo, pitems, C.byref(which), dt, m, n, dptr(ref), dptr(tst), iptr(ldref), iptr(ldtst),
                                         stride_ref, stride_tst, batch)
    return rc, out, (list(arr)[:batch] if arr is not None else None), which.value


# ---- hash and byte compare (include/libxsmm.h, include/libxsmm_amd.h) -----------------------------------------------------------
def hash(data, size, seed=0, result=None):
    """libxsmm_hash of `size` bytes at data (tensor, array or address); result: memory the GPU reaches (a tensor of 4 bytes) --
    the call is libxsmm_amd_hash_async then (any size_t size) and its status is returned instead"""
    if result is not None:
        return lib().libxsmm_amd_hash_async(dptr(result), dptr(data), size, seed)
    return lib().libxsmm_hash(dptr(data), size, seed)


def hash_batch(results, data, line_bytes, lines, ld, stride, batch, seed=0):
    """libxsmm_amd_hash_batch; results: `batch` uint32 in host or device memory; returns the status"""
    return lib().libxsmm_amd_hash_batch(dptr(results), dptr(data), line_bytes, lines, ld, stride, batch, seed)


def memcmp(a, b, size, result=None):
    """libxsmm_memcmp (0: equal, 1: not); result: memory the GPU reaches -- libxsmm_amd_memcmp_async, returns the status"""
    if result is not None:
        return lib().libxsmm_amd_memcmp_async(dptr(result), dptr(a), dptr(b), size)
    return lib().libxsmm_memcmp(dptr(a), dptr(b), size)


def memcmp_batch(results, a, b, line_bytes, lines, lda, ldb, stride_a, stride_b, batch, first_diff=None):
    """libxsmm_amd_memcmp_batch; results: `batch` int32, first_diff: None or one int64, host or device memory; returns the status"""
    return lib().libxsmm_amd_memcmp_batch(dptr(results), dptr(first_diff), dptr(a), dptr(b), line_bytes, lines, lda, ldb, stride_a, stride_b, batch)


def diff(a, b, size):
    """libxsmm_diff (size <= 255)"""
    return lib().libxsmm_diff(dptr(a), dptr(b), size)


def diff_n(a, bn, size, stride, hint, n):
    """libxsmm_diff_n: the first item of bn equal to a in the order hint, ..., n - 1, 0, ..., hint - 1, or n"""
    return lib().libxsmm_diff_n(dptr(a), dptr(bn), size, stride, hint, n)


# ---- DNN tensors and the fully-connected layer (include/libxsmm_dnn.h, include/libxsmm_dnn_fullyconnected.h) ------------------
DNN_F32, DNN_BF16 = F32, 2
DNN_FORMAT_LIBXSMM, DNN_FORMAT_NHWC, DNN_FORMAT_NCHW, DNN_FORMAT_RSCK, DNN_FORMAT_KCRS = 1, 2, 4, 8, 16
DNN_FORMAT_CKPACKED, DNN_FORMAT_NCPACKED = 64, 128
DNN_FWD, DNN_BWD, DNN_UPD, DNN_BWDUPD, DNN_ALL = 0, 1, 2, 3, 4
DNN_REGULAR_INPUT, DNN_GRADIENT_INPUT, DNN_REGULAR_OUTPUT, DNN_GRADIENT_OUTPUT, DNN_REGULAR_FILTER, DNN_GRADIENT_FILTER = 0, 3, 5, 6, 10, 12
DNN_TENSOR_TYPES = (DNN_REGULAR_INPUT, DNN_GRADIENT_INPUT, DNN_REGULAR_OUTPUT, DNN_GRADIENT_OUTPUT, DNN_REGULAR_FILTER, DNN_GRADIENT_FILTER)


def fc_create(N, Cc, K, bn=0, bk=0, bc=0, threads=1, datatype_in=DNN_F32, datatype_out=DNN_F32, buffer_format=DNN_FORMAT_LIBXSMM,
              filter_format=DNN_FORMAT_LIBXSMM, fuse_ops=0):
    """libxsmm_dnn_create_fullyconnected; returns (handle or None, status)"""
    st = C.c_uint(0xdead)
    desc = FullyconnectedDesc(N, Cc, K, bn, bk, bc, threads, datatype_in, datatype_out, buffer_format, filter_format, fuse_ops)
    h = lib().libxsmm_dnn_create_fullyconnected(desc, C.byref(st))
    return h, st.value


def fc_layout(handle, ttype):
    """libxsmm_dnn_fullyconnected_create_tensor_datalayout; returns (pointer or None, status). The caller destroys the layout."""
    st = C.c_uint(0xdead)
    l = lib().libxsmm_dnn_fullyconnected_create_tensor_datalayout(handle, ttype, C.byref(st))
    return (l if l else None), st.value


def dnn_layout_fields(l):
    """what a layout says: (num_dims, dim_type list, dim_size list, datatype, format, custom_format, tensor_type)"""
    c = l.contents
    n = int(c.num_dims)
    return n, [int(c.dim_type[j]) for j in range(n)], [int(c.dim_size[j]) for j in range(n)], int(c.datatype), int(c.format), int(c.custom_format), int(c.tensor_type)


def dnn_link_tensor(layout, data):
    """libxsmm_dnn_link_tensor on a torch tensor / numpy array / address; returns (tensor handle or None, status)"""
    st = C.c_uint(0xdead)
    t = lib().libxsmm_dnn_link_tensor(layout, dptr(data), C.byref(st))
    return t, st.value


def dnn_copy_plan(layout, plain_format, copy_in=True):
    """libxsmm_amd_dnn_copy_plan; returns (status, the eight slots or None)"""
    plan = (C.c_longlong * 8)()
    st = lib().libxsmm_amd_dnn_copy_plan(layout, plain_format, 1 if copy_in else 0, plan)
    return st, ([int(x) for x in plan] if 0 == st else None)


def fc_bind_new(handle, ttype, data):
    """layout of ttype, a tensor linked to data, bound to the handle; returns the tensor handle (the caller destroys it)"""
    L = lib()
    l, st = fc_layout(handle, ttype)
    if l is None:
        raise RuntimeError("no layout: status %d" % st)
    t, st = dnn_link_tensor(l, data)
    L.libxsmm_dnn_destroy_tensor_datalayout(l)
    if not t:
        raise RuntimeError("link failed: status %d" % st)
    st = L.libxsmm_dnn_fullyconnected_bind_tensor(handle, t, ttype)
    if 0 != st:
        raise RuntimeError("bind failed: status %d" % st)
    return t


def fc_execute(handle, kind, start_thread=0, tid=0):
    """libxsmm_dnn_fullyconnected_execute_st; returns the status"""
    return lib().libxsmm_dnn_fullyconnected_execute_st(handle, kind, start_thread, tid)


# ---- the pooling layer (include/libxsmm_dnn_pooling.h) ---------------------------------------------------------------------------
DNN_I32, DNN_I16 = 4, 5
DNN_POOLING_MAX, DNN_POOLING_AVG = 1, 2
DNN_POOLING_MASK = 31


def pool_create(N, Cc, H, W, R, S, u, v, pad_h=0, pad_w=0, pad_h_in=0, pad_w_in=0, pad_h_out=0, pad_w_out=0, threads=1, datatype_in=DNN_F32,
                datatype_out=DNN_F32, datatype_mask=DNN_I32, buffer_format=DNN_FORMAT_LIBXSMM, pooling_type=DNN_POOLING_MAX):
    """libxsmm_dnn_create_pooling; returns (handle or None, status)"""
    st = C.c_uint(0xdead)
    desc = PoolingDesc(N, Cc, H, W, R, S, u, v, pad_h, pad_w, pad_h_in, pad_w_in, pad_h_out, pad_w_out, threads, datatype_in, datatype_out,
                       datatype_mask, buffer_format, pooling_type)
    h = lib().libxsmm_dnn_create_pooling(desc, C.byref(st))
    return h, st.value


def pool_layout(handle, ttype):
    """libxsmm_dnn_pooling_create_tensor_datalayout; returns (pointer or None, status). The caller destroys the layout."""
    st = C.c_uint(0xdead)
    l = lib().libxsmm_dnn_pooling_create_tensor_datalayout(handle, ttype, C.byref(st))
    return (l if l else None), st.value


def pool_bind_new(handle, ttype, data):
    """layout of ttype, a tensor linked to data, bound to the handle; returns the tensor handle (the caller destroys it)"""
    L = lib()
    l, st = pool_layout(handle, ttype)
    if l is None:
        raise RuntimeError("no layout: status %d" % st)
    t, st = dnn_link_tensor(l, data)
    L.libxsmm_dnn_destroy_tensor_datalayout(l)
    if not t:
        raise RuntimeError("link failed: status %d" % st)
    st = L.libxsmm_dnn_pooling_bind_tensor(handle, t, ttype)
    if 0 != st:
        raise RuntimeError("bind failed: status %d" % st)
    return t


def pool_execute(handle, kind, start_thread=0, tid=0):
    """libxsmm_dnn_pooling_execute_st; returns the status"""
    return lib().libxsmm_dnn_pooling_execute_st(handle, kind, start_thread, tid)


# ---- the fused batch-norm layer (include/libxsmm_dnn_fusedbatchnorm.h) -------------------------------------------------------------
DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU = 0
DNN_FUSEDBN_OPS_BN, DNN_FUSEDBN_OPS_BNSCALE, DNN_FUSEDBN_OPS_ELTWISE, DNN_FUSEDBN_OPS_RELU = 1, 2, 4, 8


def bn_create(N, Cc, H, W, u=1, v=1, pad_h_in=0, pad_w_in=0, pad_h_out=0, pad_w_out=0, threads=1, datatype_in=DNN_F32, datatype_out=DNN_F32,
              datatype_stats=DNN_F32, buffer_format=DNN_FORMAT_LIBXSMM, fuse_order=DNN_FUSEDBN_ORDER_BN_ELTWISE_RELU, fuse_ops=DNN_FUSEDBN_OPS_BN):
    """libxsmm_dnn_create_fusedbatchnorm; returns (handle or None, status)"""
    st = C.c_uint(0xdead)
    desc = FusedBatchnormDesc(N, Cc, H, W, u, v, pad_h_in, pad_w_in, pad_h_out, pad_w_out, threads, datatype_in, datatype_out, datatype_stats,
                              buffer_format, fuse_order, fuse_ops)
    h = lib().libxsmm_dnn_create_fusedbatchnorm(desc, C.byref(st))
    return h, st.value


def bn_layout(handle, ttype):
    """libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout; returns (pointer or None, status). The caller destroys the layout."""
    st = C.c_uint(0xdead)
    l = lib().libxsmm_dnn_fusedbatchnorm_create_tensor_datalayout(handle, ttype, C.byref(st))
    return (l if l else None), st.value


def bn_bind_new(handle, ttype, data):
    """layout of ttype, a tensor linked to data, bound to the handle; returns the tensor handle (the caller destroys it)"""
    L = lib()
    l, st = bn_layout(handle, ttype)
    if l is None:
        raise RuntimeError("no layout: status %d" % st)
    t, st = dnn_link_tensor(l, data)
    L.libxsmm_dnn_destroy_tensor_datalayout(l)
    if not t:
        raise RuntimeError("link failed: status %d" % st)
    st = L.libxsmm_dnn_fusedbatchnorm_bind_tensor(handle, t, ttype)
    if 0 != st:
        raise RuntimeError("bind failed: status %d" % st)
    return t


def bn_execute(handle, kind, start_thread=0, tid=0):
    """libxsmm_dnn_fusedbatchnorm_execute_st; returns the status"""
    return lib().libxsmm_dnn_fusedbatchnorm_execute_st(handle, kind, start_thread, tid)


# ---- the convolution layer (include/libxsmm_dnn_convolution.h) ---------------------------------------------------------------------
DNN_REGULAR_FILTER_TRANS, DNN_REGULAR_CHANNEL_BIAS, DNN_GRADIENT_CHANNEL_BIAS = 11, 14, 15
DNN_CONV_FUSE_BIAS, DNN_CONV_FUSE_RELU_FWD, DNN_CONV_FUSE_RELU_BWD, DNN_CONV_FUSE_RELU = 1, 2, 4, 6
DNN_CONV_OPTION_OVERWRITE, DNN_CONV_OPTION_BWD_NO_FILTER_TRANSPOSE = 1, 8
DNN_CONV_ALGO_AUTO, DNN_CONV_ALGO_DIRECT = 0, 1


def conv_create(N, Cc, H, W, K, R, S, u=1, v=1, pad_h=0, pad_w=0, pad_h_in=0, pad_w_in=0, pad_h_out=0, pad_w_out=0, threads=1, datatype_in=DNN_F32,
                datatype_out=DNN_F32, buffer_format=DNN_FORMAT_LIBXSMM, filter_format=DNN_FORMAT_LIBXSMM, algo=DNN_CONV_ALGO_DIRECT, options=0,
                fuse_ops=0, pre_bn=None, post_bn=None):
    """libxsmm_dnn_create_conv_layer; returns (handle or None, status)"""
    st = C.c_uint(0xdead)
    desc = ConvDesc(N, Cc, H, W, K, R, S, u, v, pad_h, pad_w, pad_h_in, pad_w_in, pad_h_out, pad_w_out, threads, datatype_in, datatype_out,
                    buffer_format, filter_format, algo, options, fuse_ops, pre_bn, post_bn)
    h = lib().libxsmm_dnn_create_conv_layer(desc, C.byref(st))
    return h, st.value


def conv_layout(handle, ttype):
    """libxsmm_dnn_create_tensor_datalayout; returns (pointer or None, status). The caller destroys the layout."""
    st = C.c_uint(0xdead)
    l = lib().libxsmm_dnn_create_tensor_datalayout(handle, ttype, C.byref(st))
    return (l if l else None), st.value


def conv_bind_new(handle, ttype, data):
    """layout of ttype, a tensor linked to data, bound to the handle; returns the tensor handle (the caller destroys it)"""
    L = lib()
    l, st = conv_layout(handle, ttype)
    if l is None:
        raise RuntimeError("no layout: status %d" % st)
    t, st = dnn_link_tensor(l, data)
    L.libxsmm_dnn_destroy_tensor_datalayout(l)
    if not t:
        raise RuntimeError("link failed: status %d" % st)
    st = L.libxsmm_dnn_bind_tensor(handle, t, ttype)
    if 0 != st:
        raise RuntimeError("bind failed: status %d" % st)
    return t


def conv_execute(handle, kind, start_thread=0, tid=0):
    """libxsmm_dnn_execute_st; returns the status"""
    return lib().libxsmm_dnn_execute_st(handle, kind, start_thread, tid)


# ---- the RNN cell layer (include/libxsmm_dnn_rnncell.h) -----------------------------------------------------------------------------
DNN_FORMAT_CK, DNN_FORMAT_CKPACKED, DNN_FORMAT_NCPACKED, DNN_FORMAT_NC = 32, 64, 128, 256
DNN_RNNCELL_RNN_RELU, DNN_RNNCELL_RNN_SIGMOID, DNN_RNNCELL_RNN_TANH, DNN_RNNCELL_LSTM, DNN_RNNCELL_GRU = 0, 1, 2, 3, 4
DNN_RNN_FIRST_TYPE = 33  # LIBXSMM_DNN_RNN_REGULAR_INPUT; the 23 RNN tensor types follow each other


def rnn_create(N, Cc, K, max_T, cell_type, bn=0, bc=0, bk=0, threads=1, datatype_in=DNN_F32, datatype_out=DNN_F32,
               buffer_format=DNN_FORMAT_NC, filter_format=DNN_FORMAT_CK):
    """libxsmm_dnn_create_rnncell; returns (handle or None, status)"""
    st = C.c_uint(0xdead)
    desc = RnncellDesc(threads, K, N, Cc, max_T, bk, bn, bc, cell_type, datatype_in, datatype_out, buffer_format, filter_format)
    h = lib().libxsmm_dnn_create_rnncell(desc, C.byref(st))
    return h, st.value


def rnn_layout(handle, ttype):
    """libxsmm_dnn_rnncell_create_tensor_datalayout; returns (pointer or None, status). The caller destroys the layout."""
    st = C.c_uint(0xdead)
    l = lib().libxsmm_dnn_rnncell_create_tensor_datalayout(handle, ttype, C.byref(st))
    return (l if l else None), st.value


def rnn_bind_new(handle, ttype, data):
    """layout of ttype, a tensor linked to data, bound to the handle; returns the tensor handle (the caller destroys it)"""
    L = lib()
    l, st = rnn_layout(handle, ttype)
    if l is None:
        raise RuntimeError("no layout: status %d" % st)
    t, st = dnn_link_tensor(l, data)
    L.libxsmm_dnn_destroy_tensor_datalayout(l)
    if not t:
        raise RuntimeError("link failed: status %d" % st)
    st = L.libxsmm_dnn_rnncell_bind_tensor(handle, t, ttype)
    if 0 != st:
        raise RuntimeError("bind failed: status %d" % st)
    return t


def rnn_execute(handle, kind, start_thread=0, tid=0):
    """libxsmm_dnn_rnncell_execute_st; returns the status"""
    return lib().libxsmm_dnn_rnncell_execute_st(handle, kind, start_thread, tid)


def rnn_segments(cell_type, Cc, K, bc, bk, phase=0):
    """libxsmm_amd_rnn_segments; returns the list of (operand pair, first row, rows)"""
    buf = (C.c_int * (3 * 64))()
    n = lib().libxsmm_amd_rnn_segments(cell_type, Cc, K, bc, bk, phase, buf, 64)
    return [(buf[3 * j], buf[3 * j + 1], buf[3 * j + 2]) for j in range(n)]


def rnn_bwd_segments(cell_type, K, bk):
    """libxsmm_amd_rnn_bwd_segments; returns the list of (first column, columns)"""
    buf = (C.c_int * (2 * 64))()
    n = lib().libxsmm_amd_rnn_bwd_segments(cell_type, K, bk, buf, 64)
    return [(buf[2 * j], buf[2 * j + 1]) for j in range(n)]
