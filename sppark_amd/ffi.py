"""ctypes binding of the sppark_amd C ABI (include/sppark_amd.h).

What a maintainer of the reference's callers would write:
  * Rust  `#[repr(C)] struct Error { code: i32, str: Option<NonNull<c_char>> }`
    returned by value (rust/src/lib.rs:9-23)               -> class _Error below
  * Go    dlopen the library next to the executable and dlsym each entry point
    (go/sppark.go:83-96,165-214)                           -> load() below
Errors surface as SpparkError (the Rust wrappers `panic!(String::from(err))`,
poc/msm-cuda/src/lib.rs:76-78).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}

CURVES = ("bls12_381", "bn254", "bls12_377", "pallas", "vesta")
POLY_ONLY = ("m31", "bb31x4")                        # field types without NTT parameters: polynomial primitives only
NO_G2 = ("pallas", "vesta")                          # no pairing: no mult_pippenger_fp2_inf / sppark_g2_*
NTT_FIELDS = ("gl64", "bb31", "gl64_plonky2", "bb31_canonical")      # the last two: root-convention variants


class _Error(ctypes.Structure):                 # util/rusterror.h:18-36
    _fields_ = [("code", ctypes.c_int), ("message", ctypes.c_void_p)]


class SpparkError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("sppark error %d: %s" % (code, message))
        self.code = code
        self.message = message


def lib_path(name):
    # (SPPARK_LIBDIR: a second build with other flags for an A/B job of tools/, see sppark_amd/build.py)
    return os.path.join(_HERE, os.environ.get("SPPARK_LIBDIR", "lib"), "libsppark_%s.so" % name)


def load(name):
    """dlopen libsppark_<name>.so and declare its entry points.  Fails loudly
    when the HIP library has not been built -- there is no fallback."""
    if name in _LIBS:
        return _LIBS[name]
    # torch wheels bundle their own HIP runtime; if /opt/rocm's copy gets loaded
    # first (as a dependency of our library) torch later reports no GPU.  Import
    # torch first so that one runtime serves both.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path(name)
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s is missing: build the HIP libraries first (python -m sppark_amd.build)" % path)
    L = ctypes.CDLL(path)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    L.cuda_available.restype = ctypes.c_bool
    L.drop_error_message.argtypes = [vp]
    L.cuda_func.argtypes = [vp]
    L.cuda_func.restype = _Error
    L.drop_gpu_ptr_t.argtypes = [ctypes.POINTER(vp)]
    L.clone_gpu_ptr_t.argtypes = [ctypes.POINTER(vp)]
    L.clone_gpu_ptr_t.restype = vp
    if name in CURVES:
        L.mult_pippenger_inf.argtypes = [vp, vp, sz, vp, sz]
        L.mult_pippenger_inf.restype = _Error
        if name not in NO_G2:
            L.mult_pippenger_fp2_inf.argtypes = [vp, vp, sz, vp, sz]
            L.mult_pippenger_fp2_inf.restype = _Error
            L.sppark_msm_g2_path.argtypes = [ctypes.c_uint]
            L.sppark_msm_g2_path.restype = _Error
            L.sppark_g2_jacobian_sum.argtypes = [vp, vp, sz]
            L.sppark_g2_jacobian_sum.restype = None
            L.sppark_g2_to_affine.argtypes = [vp, vp]
            L.sppark_g2_to_affine.restype = None
        L.mult_pippenger.argtypes = [vp, vp, sz, vp]
        L.mult_pippenger.restype = _Error
        L.sppark_msm_create.argtypes = [ctypes.POINTER(vp), ci, vp]
        L.sppark_msm_create.restype = _Error
        L.sppark_msm_destroy.argtypes = [vp]
        L.sppark_msm_set_stream.argtypes = [vp, vp]
        L.sppark_msm_set_stream.restype = _Error
        L.sppark_msm_tune.argtypes = [vp, cu, cu, cu, cu, cu]
        L.sppark_msm_tune.restype = _Error
        L.sppark_msm_release_cached.argtypes = []
        L.sppark_msm_release_cached.restype = None
        L.sppark_msm_tune_split.argtypes = [vp, cu]
        L.sppark_msm_tune_split.restype = _Error
        L.sppark_msm_tune_sums.argtypes = [vp, cu]
        L.sppark_msm_tune_sums.restype = _Error
        L.sppark_msm_tune_sort.argtypes = [vp, cu]
        L.sppark_msm_tune_sort.restype = _Error
        L.sppark_msm_tune_tail.argtypes = [vp, cu, cu]
        L.sppark_msm_tune_tail.restype = _Error
        L.sppark_msm_tune_pipeline.argtypes = [vp, cu, sz, sz]
        L.sppark_msm_tune_pipeline.restype = _Error
        L.sppark_msm_last_chunks.argtypes = [vp]
        L.sppark_msm_last_chunks.restype = cu
        L.sppark_msm_plan_sort.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint * 8)]
        L.sppark_msm_tune_records.argtypes = [vp, cu]
        L.sppark_msm_tune_records.restype = _Error
        L.sppark_msm_tail_redone.argtypes = [vp]
        L.sppark_msm_tail_redone.restype = cu
        L.sppark_msm_plan_groups.argtypes = [vp, sz]
        L.sppark_msm_plan_groups.restype = cu
        L.sppark_batch_addition.argtypes = [vp, vp, sz, vp, vp, sz]
        L.sppark_batch_addition.restype = _Error
        L.sppark_ngpus.argtypes = []
        L.sppark_ngpus.restype = sz
        L.sppark_msm_multi.argtypes = [vp, vp, sz, vp, ci, sz, cu]
        L.sppark_msm_multi.restype = _Error
        L.sppark_msm_multi_shards.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ci, sz, cu,
                                              ctypes.POINTER(ci)]
        L.sppark_msm_multi_shards.restype = _Error
        L.sppark_msm_multi_ms.argtypes = [vp, vp, sz, vp, ci, sz, cu, ctypes.POINTER(ctypes.c_float)]
        L.sppark_msm_multi_ms.restype = _Error
        L.sppark_msm_multi_shards_ms.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ci, sz, cu,
                                                 ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_float)]
        L.sppark_msm_multi_shards_ms.restype = _Error
        L.sppark_msm_rccl_sum.argtypes = [vp, vp, ci, vp, vp]
        L.sppark_msm_rccl_sum.restype = _Error
        L.sppark_msm_rccl.argtypes = [vp, vp, sz, vp, ci, sz, vp, vp]
        L.sppark_msm_rccl.restype = _Error
        L.sppark_msm_reserve.argtypes = [vp, sz, sz, ci, ci]
        L.sppark_msm_reserve.restype = _Error
        L.sppark_msm_invoke.argtypes = [vp, vp, vp, sz, vp, ci, sz]
        L.sppark_msm_invoke.restype = _Error
        L.sppark_msm_set_points.argtypes = [vp, vp, sz, sz]
        L.sppark_msm_set_points.restype = _Error
        L.sppark_msm_set_points_fixed_base.argtypes = [vp, vp, sz, sz]
        L.sppark_msm_set_points_fixed_base.restype = _Error
        L.sppark_msm_fixed_base_windows.argtypes = [vp]
        L.sppark_msm_fixed_base_windows.restype = cu
        L.sppark_msm_preloaded.argtypes = [vp]
        L.sppark_msm_preloaded.restype = sz
        L.sppark_msm_enable_timing.argtypes = [vp, ci]
        L.sppark_msm_enable_timing.restype = _Error
        L.sppark_msm_kernel_ms.argtypes = [vp, ci]
        L.sppark_msm_kernel_ms.restype = ctypes.c_float
        L.sppark_msm_scratch_bytes.argtypes = [vp]
        L.sppark_msm_scratch_bytes.restype = sz
        L.sppark_msm_plan.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint * 8)]
        # include/sppark_amd_short.h: scalars of a declared bit length
        L.sppark_msm_invoke_bits.argtypes = [vp, vp, vp, sz, vp, cu, sz, sz]
        L.sppark_msm_invoke_bits.restype = _Error
        L.sppark_msm_reserve_bits.argtypes = [vp, sz, sz, ci, ci, cu, sz]
        L.sppark_msm_reserve_bits.restype = _Error
        L.sppark_msm_plan_bits.argtypes = [vp, sz, cu, ctypes.POINTER(ctypes.c_uint * 8)]
        L.mult_pippenger_inf_bits.argtypes = [vp, vp, sz, vp, cu, sz, sz]
        L.mult_pippenger_inf_bits.restype = _Error
        if name not in NO_G2:
            L.mult_pippenger_fp2_inf_bits.argtypes = [vp, vp, sz, vp, cu, sz, sz]
            L.mult_pippenger_fp2_inf_bits.restype = _Error
        L.sppark_g1_jacobian_sum.argtypes = [vp, vp, sz]
        L.sppark_g1_to_affine.argtypes = [vp, vp]
        L.sppark_g1_generate.argtypes = [vp, sz, sz, ctypes.c_uint64]
        L.sppark_g1_generate.restype = _Error
        L.sppark_g1_generate_progression.argtypes = [vp, sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.sppark_g1_generate_progression.restype = _Error
    if name in NTT_FIELDS or name in CURVES:
        L.compute_ntt.argtypes = [sz, vp, ctypes.c_uint32, ci, ci, ci]
        L.compute_ntt.restype = _Error
        L.sppark_ntt.argtypes = [sz, vp, ctypes.c_uint32, ci, ci, ci, vp]
        L.sppark_ntt.restype = _Error
        u32 = ctypes.c_uint32
        L.sppark_lde.argtypes = [sz, vp, u32, u32, vp, vp]
        L.sppark_lde.restype = _Error
        L.sppark_lde_powers.argtypes = [sz, vp, u32, vp]
        L.sppark_lde_powers.restype = _Error
        L.sppark_lde_expand.argtypes = [sz, vp, vp, u32, u32, vp]
        L.sppark_lde_expand.restype = _Error
        L.sppark_ntt_release_cached.argtypes = []
        L.sppark_ntt_release_cached.restype = None
        L.sppark_ntt_cached_scratch_bytes.argtypes = []
        L.sppark_ntt_cached_scratch_bytes.restype = sz
        L.sppark_ntt_cached_tables.argtypes = []
        L.sppark_ntt_cached_tables.restype = sz
        L.sppark_ntt_batch.argtypes = [sz, vp, u32, sz, sz, ci, ci, ci, vp]       # include/sppark_amd_batch.h
        L.sppark_ntt_batch.restype = _Error
        L.sppark_lde_batch.argtypes = [sz, vp, u32, u32, sz, vp, vp]
        L.sppark_lde_batch.restype = _Error
        L.sppark_ntt_batch_launch_cols.argtypes = [sz, u32]
        L.sppark_ntt_batch_launch_cols.restype = sz

    if name in NTT_FIELDS or name in CURVES or name in POLY_ONLY:
        L.sppark_prefix_op.argtypes = [sz, vp, vp, sz, ci, vp]
        L.sppark_prefix_op.restype = _Error
        L.sppark_poly_evaluate.argtypes = [sz, vp, vp, sz, vp, sz, vp]
        L.sppark_poly_evaluate.restype = _Error
        L.sppark_div_by_x_minus_z.argtypes = [sz, vp, sz, vp, ci, vp]
        L.sppark_div_by_x_minus_z.restype = _Error
        L.sppark_field_inverse.argtypes = [sz, vp, vp, sz, vp]                   # include/sppark_amd_field.h
        L.sppark_field_inverse.restype = _Error
        L.sppark_field_divide.argtypes = [sz, vp, vp, vp, sz, vp]
        L.sppark_field_divide.restype = _Error
        for fn in (L.sppark_field_add, L.sppark_field_sub, L.sppark_field_mul, L.sppark_field_scale):     # include/sppark_amd_arith.h
            fn.argtypes = [sz, vp, vp, vp, sz, vp]
            fn.restype = _Error
        L.sppark_field_mul_sub.argtypes = [sz, vp, vp, vp, vp, vp, sz, vp]
        L.sppark_field_mul_sub.restype = _Error
        u32 = ctypes.c_uint32                                                    # include/sppark_amd_mle.h
        L.sppark_mle_fold.argtypes = [sz, vp, vp, u32, vp, ci, vp]
        L.sppark_mle_fold.restype = _Error
        L.sppark_mle_evaluate.argtypes = [sz, vp, vp, u32, vp, vp]
        L.sppark_mle_evaluate.restype = _Error
        L.sppark_mle_eq.argtypes = [sz, vp, vp, u32, vp]
        L.sppark_mle_eq.restype = _Error
        L.sppark_sumcheck_round.argtypes = [sz, vp, ctypes.POINTER(vp), sz, ci, u32, ci, vp]
        L.sppark_sumcheck_round.restype = _Error
        # include/sppark_amd_merkle.h (indices: a host array of uint64, passed by address)
        L.sppark_merkle_commit.argtypes = [sz, vp, vp, vp, u32, sz, sz, sz, ci, vp]
        L.sppark_merkle_commit.restype = _Error
        L.sppark_merkle_open.argtypes = [sz, vp, vp, u32, vp, sz, vp]
        L.sppark_merkle_open.restype = _Error
        L.sppark_merkle_gather.argtypes = [sz, vp, vp, u32, sz, sz, sz, vp, sz, vp]
        L.sppark_merkle_gather.restype = _Error
        # include/sppark_amd_fri.h (fold and domain: the libraries with a 2-adic domain, i.e. all but m31)
        L.sppark_fri_reduce.argtypes = [sz, vp, vp, ci, u32, sz, sz, sz, vp, vp, ci, vp]
        L.sppark_fri_reduce.restype = _Error
        if name != "m31":
            L.sppark_fri_fold.argtypes = [sz, vp, vp, u32, u32, vp, vp, ci, vp]
            L.sppark_fri_fold.restype = _Error
            L.sppark_fri_domain.argtypes = [sz, vp, u32, vp, ci, vp, vp]
            L.sppark_fri_domain.restype = _Error
    if name in NTT_FIELDS:                                                       # include/sppark_amd_poseidon2.h
        u32 = ctypes.c_uint32
        L.sppark_poseidon2_permute.argtypes = [sz, vp, vp, sz, vp, u32, u32, vp]
        L.sppark_poseidon2_permute.restype = _Error
        L.sppark_poseidon2_commit.argtypes = [sz, vp, vp, vp, u32, sz, sz, sz, vp, u32, u32, vp]
        L.sppark_poseidon2_commit.restype = _Error
    if name in NTT_FIELDS or name in CURVES:
        L.sppark_poly_product.argtypes = [sz, vp, vp, sz, vp, sz, vp]
        L.sppark_poly_product.restype = _Error
        L.sppark_poly_vanishing_quotient.argtypes = [sz, vp, vp, vp, vp, ctypes.c_uint32, vp]
        L.sppark_poly_vanishing_quotient.restype = _Error
    if name == "m31":                                                            # include/sppark_amd_circle.h
        u32 = ctypes.c_uint32
        L.sppark_circle_ntt.argtypes = [sz, vp, u32, sz, sz, ci, ci, vp]
        L.sppark_circle_ntt.restype = _Error
        L.sppark_circle_lde.argtypes = [sz, vp, u32, u32, sz, ci, vp, vp]
        L.sppark_circle_lde.restype = _Error
        L.sppark_circle_cached_bytes.argtypes = [sz]
        L.sppark_circle_cached_bytes.restype = sz
        L.sppark_circle_release_cached.argtypes = [sz]
        L.sppark_circle_release_cached.restype = _Error
    _LIBS[name] = L
    return L


def load_devtest(name):
    """dlopen libsppark_<name>_devtest.so: the device test hooks (sppark_devtest_*), a TEST-only
    library built next to the product ones by sppark_amd.build."""
    key = name + "_devtest"
    if key in _LIBS:
        return _LIBS[key]
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path(key)
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: python -m sppark_amd.build" % path)
    L = ctypes.CDLL(path)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.drop_error_message.argtypes = [vp]
    if name in CURVES:
        L.sppark_devtest_field_op.argtypes = [ci, ci, vp, vp, vp, sz]
        L.sppark_devtest_field_op.restype = _Error
        L.sppark_devtest_bucket_field_op.argtypes = [ci, vp, vp, vp, sz]
        L.sppark_devtest_bucket_field_op.restype = _Error
        L.sppark_devtest_bucket_field_limbs.argtypes = []
        L.sppark_devtest_bucket_field_limbs.restype = ci
        L.sppark_devtest_bucket_xyzz_op.argtypes = [ci, vp, vp, vp, sz]
        L.sppark_devtest_bucket_xyzz_op.restype = _Error
        L.sppark_devtest_xyzz_op.argtypes = [ci, vp, vp, vp, sz]
        L.sppark_devtest_xyzz_op.restype = _Error
        # api/devtest_g2_api.hip: every product form of the bucket field on raw limbs; on the curves with a G2, Fp2 and the
        # G2 point classes operation by operation
        L.sppark_devtest_blocks_info.argtypes = [ci, vp]
        L.sppark_devtest_blocks_info.restype = ci
        L.sppark_devtest_blocks_run.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, sz]
        L.sppark_devtest_blocks_run.restype = _Error
        if name not in NO_G2:
            L.sppark_devtest_fp2x_op.argtypes = [ci, ci, vp, vp, vp, sz]
            L.sppark_devtest_fp2x_op.restype = _Error
            L.sppark_devtest_fp2_wire_op.argtypes = [ci, vp, vp, vp, sz]
            L.sppark_devtest_fp2_wire_op.restype = _Error
            L.sppark_devtest_g2_xyzz_op.argtypes = [ci, ci, vp, vp, vp, sz]
            L.sppark_devtest_g2_xyzz_op.restype = _Error
            L.sppark_devtest_g2_chain.argtypes = [ci, vp, vp, vp, sz, sz, vp, sz, ctypes.c_uint]
            L.sppark_devtest_g2_chain.restype = _Error
    else:
        L.sppark_devtest_small_field_op.argtypes = [ci, vp, vp, vp, sz]
        L.sppark_devtest_small_field_op.restype = _Error
    _LIBS[key] = L
    return L


def check(L, err):
    """Raise SpparkError for a non-zero code; take ownership of the message."""
    if err.code != 0:
        msg = ""
        if err.message:
            msg = ctypes.string_at(err.message).decode(errors="replace")
            L.drop_error_message(err.message)
        raise SpparkError(err.code, msg)


def cuda_available(name="bls12_381"):
    """util/all_gpus.cpp:65-66 via go/sppark.go:475-477 IsCudaAvailable()."""
    return bool(load(name).cuda_available())


def as_pointer(x):
    """(address, keepalive) of a numpy array, torch tensor (host or device) or int."""
    if isinstance(x, int):
        return x, None
    if hasattr(x, "data_ptr"):                      # torch tensor
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr(), x
    if hasattr(x, "ctypes"):                        # numpy
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data, x
    raise TypeError("unsupported buffer type %r" % type(x))
