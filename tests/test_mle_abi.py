"""CPU: include/sppark_amd_mle.h -- multilinear tables and sumcheck rounds -- compiles as plain C and C++; all eleven
product libraries export the four calls; every rejection arrives before a device is looked up (the same error protocol with
or without one); the Python wrappers reject bad shapes before they reach the library; and the new kernels' resources, from
the code objects' metadata: fold streams (no LDS, no private segment), no kernel has a private segment, every work-group is
256 lanes."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
CALLS = ("sppark_mle_fold", "sppark_mle_evaluate", "sppark_mle_eq", "sppark_sumcheck_round")
ELEM = (("gl64", 8), ("bls12_381", 32), ("m31", 4), ("bb31x4", 16), ("bb31", 4))
INVALID = -1                                               # negated hipErrorInvalidValue
LOW, HIGH, PRODUCT, EQ_MUL_SUB = 0, 1, 0, 1


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def _rejected(L, err, word=None):
    msg = _message(L, err)
    assert err.code == INVALID and msg, (err.code, msg)
    if word is not None:
        assert word in msg, msg


def test_mle_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_mle.h"\n'
            'int main(void) {\n'
            '  SppError (*fo)(size_t, void *, const void *, uint32_t, const void *, int, void *) = sppark_mle_fold;\n'
            '  SppError (*ev)(size_t, void *, const void *, uint32_t, const void *, void *) = sppark_mle_evaluate;\n'
            '  SppError (*eq)(size_t, void *, const void *, uint32_t, void *) = sppark_mle_eq;\n'
            '  SppError (*ro)(size_t, void *, const void *const *, size_t, int, uint32_t, int, void *) = sppark_sumcheck_round;\n'
            '  int k = SPPARK_MLE_LOW + SPPARK_MLE_HIGH + SPPARK_SUMCHECK_PRODUCT + SPPARK_SUMCHECK_EQ_MUL_SUB;\n'
            '  return (fo == 0) + (ev == 0) + (eq == 0) + (ro == 0) + (k == 2); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_mle_symbols_exported(libs):
    assert len(libs) == 11
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        for fn in CALLS:
            assert hasattr(L, fn), (name, fn)


def test_mle_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    for name, eb in ELEM:
        L = ffi.load(name)
        lg = 4
        n = 1 << lg
        pool = [np.ones(2 * n * eb, dtype=np.uint8) for _ in range(5)]
        a, b, c, d, o = (x.ctypes.data for x in pool)
        small = np.ones(8 * eb, dtype=np.uint8)
        r = small.ctypes.data
        tabs = lambda *p: (ctypes.c_void_p * len(p))(*p)                                   # noqa: E731

        # fold
        for order in (LOW, HIGH):
            for args in ((None, a, r), (o, None, r), (o, a, None)):
                _rejected(L, L.sppark_mle_fold(0, args[0], args[1], lg, args[2], order, None))
            _rejected(L, L.sppark_mle_fold(0, o, a, 0, r, order, None), b"lg_n")               # nothing to bind
            _rejected(L, L.sppark_mle_fold(0, o, a, 33, r, order, None), b"lg_n")
            for shift in (eb, (n // 2 - 1) * eb, (n - 1) * eb, -eb, -(n // 2 - 1) * eb):    # out partly over in
                _rejected(L, L.sppark_mle_fold(0, a + shift, a, lg, r, order, None), b"overlap")
            _rejected(L, L.sppark_mle_fold(0, o, a, lg, o + 3 * eb, order, None), b"overlap")  # r inside out
        _rejected(L, L.sppark_mle_fold(0, a, a, lg, r, LOW, None), b"overlap")                # in place: HIGH only
        for order in (-1, 2, 7):
            _rejected(L, L.sppark_mle_fold(0, o, a, lg, r, order, None), b"order")

        # evaluate
        for args in ((None, a, r), (o, None, r), (o, a, None)):
            _rejected(L, L.sppark_mle_evaluate(0, args[0], args[1], lg, args[2], None))
        _rejected(L, L.sppark_mle_evaluate(0, o, a, 33, r, None), b"lg_n")
        _rejected(L, L.sppark_mle_evaluate(0, a + 5 * eb, a, lg, r, None), b"overlap")         # ret inside in
        _rejected(L, L.sppark_mle_evaluate(0, r + 2 * eb, a, lg, r, None), b"overlap")         # ret inside point
        _rejected(L, L.sppark_mle_evaluate(0, None, a, 0, None, None))

        # eq
        for args in ((None, r), (o, None)):
            _rejected(L, L.sppark_mle_eq(0, args[0], args[1], lg, None))
        _rejected(L, L.sppark_mle_eq(0, o, r, 33, None), b"lg_n")
        _rejected(L, L.sppark_mle_eq(0, o, o + 2 * eb, lg, None), b"overlap")                  # point inside out
        _rejected(L, L.sppark_mle_eq(0, None, None, 0, None))

        # round
        res = o
        for form, nt in ((PRODUCT, 0), (PRODUCT, 5), (EQ_MUL_SUB, 3), (EQ_MUL_SUB, 5), (EQ_MUL_SUB, 1)):
            _rejected(L, L.sppark_sumcheck_round(0, res, tabs(a, b, c, d, a), nt, form, lg, LOW, None), b"ntables")
        for form in (-1, 2):
            _rejected(L, L.sppark_sumcheck_round(0, res, tabs(a, b, c, d), 4, form, lg, LOW, None), b"form")
        for order in (-1, 2):
            _rejected(L, L.sppark_sumcheck_round(0, res, tabs(a, b, c, d), 4, PRODUCT, lg, order, None), b"order")
        for form in (PRODUCT, EQ_MUL_SUB):
            _rejected(L, L.sppark_sumcheck_round(0, res, tabs(a, b, c, d), 4, form, 0, LOW, None), b"lg_n")
            _rejected(L, L.sppark_sumcheck_round(0, res, tabs(a, b, c, d), 4, form, 33, LOW, None), b"lg_n")
            _rejected(L, L.sppark_sumcheck_round(0, None, tabs(a, b, c, d), 4, form, lg, LOW, None))
            _rejected(L, L.sppark_sumcheck_round(0, res, None, 4, form, lg, LOW, None))
            for i in range(4):
                p = [a, b, c, d]
                p[i] = None
                _rejected(L, L.sppark_sumcheck_round(0, res, tabs(*p), 4, form, lg, LOW, None))
                p = [a, b, c, d]
                p[i] = p[(i + 1) % 4] + 3 * eb                                              # a table partly over its neighbour
                _rejected(L, L.sppark_sumcheck_round(0, res, tabs(*p), 4, form, lg, LOW, None), b"overlap")
            _rejected(L, L.sppark_sumcheck_round(0, b + 2 * eb, tabs(a, b, c, d), 4, form, lg, LOW, None), b"overlap")    # out in a table
        assert all((x == 1).all() for x in pool) and (small == 1).all()


def test_mle_wrappers_reject_bad_shapes(libs):
    from sppark_amd import mle
    x8, y8, x4, x6, x16 = (np.ones(k, dtype=np.uint64) for k in (8, 8, 4, 6, 16))
    k1, k2, k3 = (np.ones(k, dtype=np.uint64) for k in (1, 2, 3))
    for args in ((x8, x8, k1), (x4, x6, k1), (x4, x8, k2), (x6, x8, k1), (k1, k1, k1)):   # out n/2; a power of two; one r; lg_n >= 1
        with pytest.raises(ValueError):
            mle.fold(*args, order=mle.HIGH if args[0] is not args[1] else mle.LOW, field="gl64")
    with pytest.raises(ValueError):
        mle.fold(x4, x8, k1, order=2, field="gl64")
    with pytest.raises(ValueError):
        mle.fold(np.ones(6, dtype=np.uint64), np.ones(12, dtype=np.uint64), k1, field="bls12_381")    # 1.5 elements
    for args in ((x8, k2), (x6, k3), (x8, x4)):                                            # lg_n elements; a power of two
        with pytest.raises(ValueError):
            mle.evaluate(*args, field="gl64")
        with pytest.raises(ValueError):
            mle.eq(*args, field="gl64")
    with pytest.raises(ValueError):
        mle.evaluate(x8, k1, field="bls12_381")                                            # two elements, a point of a quarter
    for tables, form in (([], "product"), ([x8] * 5, "product"), ([x8] * 3, "eq_mul_sub"), ([x8, x16], "product"), ([x6, x6], "product"),
                         ([k1], "product"), ([x8, y8], "sum")):
        with pytest.raises(ValueError):
            mle.round(tables, form=form, field="gl64")
    with pytest.raises(ValueError):
        mle.round([x8, y8], order=3, field="gl64")


KERNEL_OBJECTS = ["gl64__api_ntt_api.hip.o", "bb31__api_ntt_api.hip.o", "m31__api_poly_only_api.hip.o", "bb31x4__api_poly_only_api.hip.o",
                  "bls12_381__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o", "bn254__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o"]


@pytest.mark.parametrize("obj", KERNEL_OBJECTS)
def test_mle_kernels_resources(libs, obj):
    """Instances: fold 2 orders x r by value / by pointer (4), bind 1, eq 1, round 5 shapes x 2 orders (10), sum 1 -- and, for
    the single-word fields, all but the sum twice: with 16-byte accesses and element-wise."""
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    hit = {k: v for k, v in meta.items() if ("k_mle_" in k or "k_sumcheck_" in k) and "vgpr_count" in v}
    assert not any("k_vec" in k for k in hit)
    single_word = not ("bb31x4" in obj or "WITH_MSM" in obj)
    count = lambda word: len([k for k in hit if word in k])                                 # noqa: E731
    two = 2 if single_word else 1
    assert count("k_mle_fold") == 4 * two and count("k_mle_bind") == two and count("k_mle_eq") == two, sorted(hit)
    assert count("k_sumcheck_round") == 10 * two and count("k_sumcheck_sum") == 1, sorted(hit)
    for name, md in hit.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, (name, md)
        if "k_mle_fold" in name:
            assert int(md.get("group_segment_fixed_size") or 0) == 0, (name, md)
