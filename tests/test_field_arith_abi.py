"""CPU: include/sppark_amd_arith.h -- field-vector arithmetic, polynomial product, vanishing quotient -- compiles as plain
C and C++; every product library exports the five pointwise calls and exactly the nine with compute_ntt the two polynomial
ones; the calls fail loudly without a device, reject bad arguments before a device is looked up, the Python wrappers
reject bad shapes before they reach the library, and the pointwise kernels use neither scratch nor LDS."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
POINTWISE = ("sppark_field_add", "sppark_field_sub", "sppark_field_mul", "sppark_field_scale", "sppark_field_mul_sub")
POLY = ("sppark_poly_product", "sppark_poly_vanishing_quotient")
NO_NTT = ("m31", "bb31x4")
ELEM = (("gl64", 8), ("bls12_381", 32), ("m31", 4), ("bb31x4", 16), ("bb31", 4))


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def test_arith_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_arith.h"\n'
            'int main(void) {\n'
            '  SppError (*f3[3])(size_t, void *, const void *, const void *, size_t, void *) = {sppark_field_add, sppark_field_sub, sppark_field_mul};\n'
            '  SppError (*fs)(size_t, void *, const void *, const void *, size_t, void *) = sppark_field_scale;\n'
            '  SppError (*fm)(size_t, void *, const void *, const void *, const void *, const void *, size_t, void *) = sppark_field_mul_sub;\n'
            '  SppError (*pp)(size_t, void *, const void *, size_t, const void *, size_t, void *) = sppark_poly_product;\n'
            '  SppError (*vq)(size_t, void *, const void *, const void *, const void *, uint32_t, void *) = sppark_poly_vanishing_quotient;\n'
            '  return (f3[0] == 0) + (f3[1] == 0) + (f3[2] == 0) + (fs == 0) + (fm == 0) + (pp == 0) + (vq == 0); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_arith_symbols_exported(libs):
    assert len(libs) == 11
    with_poly = []
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        for fn in POINTWISE:
            assert hasattr(L, fn), (name, fn)
        has = [hasattr(L, fn) for fn in POLY]
        assert all(has) or not any(has), name
        if all(has):
            with_poly.append(name)
        assert all(has) == (name not in NO_NTT), name
    assert len(with_poly) == 9


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_arith_calls_fail_loudly_without_a_device(libs):
    from sppark_amd import ffi
    for name in ("gl64", "bls12_381", "m31"):
        L = ffi.load(name)
        o, a, b, c, k = (np.ones(64, dtype=np.uint64) for _ in range(5))
        p = [x.ctypes.data for x in (o, a, b, c, k)]
        for fn in (L.sppark_field_add, L.sppark_field_sub, L.sppark_field_mul, L.sppark_field_scale):
            err = fn(0, p[0], p[1], p[2], 8, None)
            assert err.code < 0 and _message(L, err), name
        for kk in (None, p[4]):
            err = L.sppark_field_mul_sub(0, p[0], p[1], p[2], p[3], kk, 8, None)
            assert err.code < 0 and _message(L, err), name
        if name not in NO_NTT:
            err = L.sppark_poly_product(0, p[0], p[1], 4, p[2], 4, None)
            assert err.code < 0 and _message(L, err), name
            err = L.sppark_poly_vanishing_quotient(0, p[0], p[1], p[2], p[3], 2, None)
            assert err.code < 0 and _message(L, err), name
        assert all((x == 1).all() for x in (o, a, b, c, k))


def _calls(L, bufs, k, n):
    """every pointwise call as (name, buffer positions it takes, a function of those buffers)"""
    return (
        ("add", 3, lambda o, a, b: L.sppark_field_add(0, o, a, b, n, None)),
        ("sub", 3, lambda o, a, b: L.sppark_field_sub(0, o, a, b, n, None)),
        ("mul", 3, lambda o, a, b: L.sppark_field_mul(0, o, a, b, n, None)),
        ("scale", 2, lambda o, a: L.sppark_field_scale(0, o, a, k, n, None)),
        ("mul_sub", 4, lambda o, a, b, c: L.sppark_field_mul_sub(0, o, a, b, c, None, n, None)),
        ("mul_sub_k", 4, lambda o, a, b, c: L.sppark_field_mul_sub(0, o, a, b, c, k, n, None)),
    )


def test_arith_calls_reject_bad_arguments_before_the_device(libs):
    """the partial-overlap matrix for every pair of buffers of every call, NULL buffers, byte-extent overflow, len == 0:
    the same error protocol with or without a device"""
    from sppark_amd import ffi
    for name, eb in ELEM:
        L = ffi.load(name)
        n = 16
        pool = [np.ones(64 * eb, dtype=np.uint8) for _ in range(4)]
        base = [x.ctypes.data for x in pool]
        kbuf = np.ones(eb, dtype=np.uint8)
        k = kbuf.ctypes.data
        for call, nbuf, fn in _calls(L, base, k, n):
            for i in range(nbuf):
                for j in range(nbuf):
                    if i == j:
                        continue
                    for shift in (eb, 3 * eb, 15 * eb):               # buffer i starts inside buffer j
                        args = list(base[:nbuf])
                        args[i] = base[j] + shift
                        err = fn(*args)
                        assert err.code < 0 and b"overlap" in _message(L, err), (name, call, i, j, shift)
            for i in range(nbuf):                                      # NULL buffers
                args = list(base[:nbuf])
                args[i] = None
                err = fn(*args)
                assert err.code < 0 and _message(L, err), (name, call, i)
        err = L.sppark_field_scale(0, base[0], base[1], None, n, None)                 # scale needs its k
        assert err.code < 0 and _message(L, err), name
        err = L.sppark_field_scale(0, base[0], base[1], base[0] + 2 * eb, n, None)     # k inside out
        assert err.code < 0 and b"overlap" in _message(L, err), name
        # len * sizeof(element) past size_t
        big = (1 << 64) // eb
        for call, nbuf, fn in _calls(L, base, k, big):
            err = fn(*base[:nbuf])
            assert err.code < 0 and _message(L, err), (name, call)
        # len == 0 succeeds and touches nothing, NULL pointers included
        for call, nbuf, fn in _calls(L, base, None, 0):
            err = fn(*([None] * nbuf))
            assert err.code == 0 and not err.message, (name, call)
        assert all((x == 1).all() for x in pool) and (kbuf == 1).all()


def test_poly_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    two_adicity = {"gl64": 32, "bb31": 27, "bls12_381": 32, "bn254": 28}
    for name, eb in (("gl64", 8), ("bb31", 4), ("bls12_381", 32), ("bn254", 32)):
        L = ffi.load(name)
        pool = [np.ones(64 * eb, dtype=np.uint8) for _ in range(4)]
        h, a, b, c = (x.ctypes.data for x in pool)
        # product: out must be disjoint from a and b -- identical included; a and b may be anything
        for args in ((a, a, 8, b, 8), (b, a, 8, b, 8), (a + 7 * eb, a, 8, b, 8), (b - eb, a, 8, b + 13 * eb, 8), (a + eb, a, 8, a, 8)):
            err = L.sppark_poly_product(0, args[0], args[1], args[2], args[3], args[4], None)
            assert err.code < 0 and b"overlap" in _message(L, err), (name, args)
        for args in ((None, a, b), (h, None, b), (h, a, None)):
            err = L.sppark_poly_product(0, args[0], args[1], 8, args[2], 8, None)
            assert err.code < 0 and _message(L, err), (name, args)
        for la, lb in ((0, 8), (8, 0), (0, 0)):                           # nothing to do: succeeds, NULL pointers included
            err = L.sppark_poly_product(0, None, None, la, None, lb, None)
            assert err.code == 0 and not err.message, (name, la, lb)
        err = L.sppark_poly_product(0, h, a, (1 << 64) // eb, b, 8, None)
        assert err.code < 0 and _message(L, err), name
        # the vanishing quotient: h identical to an input or disjoint from all
        for i in range(3):
            for shift in (eb, 3 * eb, -eb):
                ins = [a, b, c]
                hh = ins[i] + shift
                err = L.sppark_poly_vanishing_quotient(0, hh, ins[0], ins[1], ins[2], 2, None)
                assert err.code < 0 and b"overlap" in _message(L, err), (name, i, shift)
        for args in ((None, a, b, c), (h, None, b, c), (h, a, None, c), (h, a, b, None)):
            err = L.sppark_poly_vanishing_quotient(0, args[0], args[1], args[2], args[3], 2, None)
            assert err.code < 0 and _message(L, err), (name, args)
        # above the 2-adicity: rejected whatever the pointers are (never dereferenced)
        err = L.sppark_poly_vanishing_quotient(0, 0x10000000, 0x20000000, 0x30000000, 0x40000000, two_adicity[name] + 1, None)
        msg = _message(L, err)
        assert err.code < 0 and b"2-adicity" in msg and str(two_adicity[name]).encode() in msg, (name, msg)
        assert all((x == 1).all() for x in pool)
    # BabyBear, la = lb = 2^27: la + lb - 1 needs 2^28 > 2^27
    L = ffi.load("bb31")
    err = L.sppark_poly_product(0, 0x7000000000, 0x1000000000, 1 << 27, 0x3000000000, 1 << 27, None)
    msg = _message(L, err)
    assert err.code < 0 and b"2-adicity" in msg and b"27" in msg, msg


def test_arith_wrappers_reject_bad_shapes(libs):
    from sppark_amd import poly
    x8, y8, z8 = (np.ones(8, dtype=np.uint64) for _ in range(3))
    x9 = np.ones(9, dtype=np.uint64)
    k1, k2 = np.ones(1, dtype=np.uint64), np.ones(2, dtype=np.uint64)
    for fn in (poly.vec_add, poly.vec_sub, poly.vec_mul):
        for args in ((x9, y8, z8), (x8, x9, z8), (x8, y8, x9)):
            with pytest.raises(ValueError):
                fn(*args, field="gl64")
    for args in ((x9, y8, k1), (x8, x9, k1), (x8, y8, k2)):
        with pytest.raises(ValueError):
            poly.vec_scale(*args, field="gl64")
    w8 = np.ones(8, dtype=np.uint64)
    for args in ((x9, y8, z8, w8), (x8, x9, z8, w8), (x8, y8, x9, w8), (x8, y8, z8, x9)):
        with pytest.raises(ValueError):
            poly.vec_mul_sub(*args, field="gl64")
    with pytest.raises(ValueError):
        poly.vec_mul_sub(x8, y8, z8, w8, k=k2, field="gl64")
    w3 = np.ones(3, dtype=np.uint64)                                # 24 bytes of a 32-byte field
    with pytest.raises(ValueError):
        poly.vec_add(w3, w3, w3, field="bls12_381")
    with pytest.raises(ValueError):
        poly.vec_scale(x8, y8, w3, field="bls12_381")               # k: not one element
    with pytest.raises(ValueError):
        poly.vec_mul_sub(x8, y8, z8, w8, k=k1, field="bls12_381")   # k: 8 bytes of 32
    with pytest.raises(ValueError):
        poly.product(np.ones(14, dtype=np.uint64), x8, y8, field="gl64")       # 8 + 8 - 1 = 15
    with pytest.raises(ValueError):
        poly.product(w3, w3, w3, field="bls12_381")
    for n in (3, 6, 12):
        v = [np.ones(n, dtype=np.uint64) for _ in range(4)]
        with pytest.raises(ValueError):
            poly.vanishing_quotient(*v, field="gl64")
    with pytest.raises(ValueError):
        poly.vanishing_quotient(x8, y8, z8, x9, field="gl64")
    with pytest.raises(ValueError):
        poly.vanishing_quotient(w3, w3, w3, w3, field="bls12_381")


@pytest.mark.parametrize("obj,count", [("gl64__api_ntt_api.hip.o", 16), ("bb31__api_ntt_api.hip.o", 16),
                                       ("m31__api_poly_only_api.hip.o", 16), ("bb31x4__api_poly_only_api.hip.o", 8),
                                       ("bls12_381__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o", 8),
                                       ("bn254__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o", 8)])
def test_pointwise_kernels_use_no_scratch_and_no_lds(libs, obj, count):
    """k_vec (poly/vec_kernels.hpp) streams: no private segment, no LDS, and at most 128 registers (four waves per SIMD)
    -- except the 256-bit products, which keep the operands of two elements per lane in registers.
    Instances: six operations, k by value and by pointer for the two that take one (8), times the 16-byte and the
    element-wise form for the single-word fields."""
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    hit = {k: v for k, v in meta.items() if "k_vec" in k and "vgpr_count" in v}
    vec = {k: v for k, v in hit.items() if "k_vec_pad" not in k}
    assert len(vec) == count, sorted(vec)
    assert len(hit) - len(vec) == (0 if "poly_only" in obj else 1)
    for name, md in hit.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("group_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, (name, md)
        if "WITH_MSM" not in obj:
            assert int(md.get("vgpr_count") or 0) + int(md.get("agpr_count") or 0) <= 128, (name, md)
