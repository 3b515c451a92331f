"""CPU: include/sppark_amd_circle.h compiles as plain C and C++; libsppark_m31 alone exports its four entry points; the
calls fail loudly without a device and leave the buffers alone, reject bad arguments before a device is looked up, the
Python wrappers raise ValueError before any native call, and circle.domain equals the host model's."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu
import circle_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SYMBOLS = ("sppark_circle_ntt", "sppark_circle_lde", "sppark_circle_cached_bytes", "sppark_circle_release_cached")
INVALID = -1                                            # -(int)hipErrorInvalidValue


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def test_circle_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_circle.h"\n'
            'int main(void) {\n'
            '  SppError (*t)(size_t, void *, uint32_t, size_t, size_t, int, int, void *) = sppark_circle_ntt;\n'
            '  SppError (*l)(size_t, void *, uint32_t, uint32_t, size_t, int, void *, void *) = sppark_circle_lde;\n'
            '  size_t (*c)(size_t) = sppark_circle_cached_bytes;\n'
            '  SppError (*r)(size_t) = sppark_circle_release_cached;\n'
            '  size_t cap = SPPARK_CIRCLE_CACHE_CAP_BYTES;\n'
            '  return (t == 0) + (l == 0) + (c == 0) + (r == 0) + (cap == 0) + SPPARK_CIRCLE_EVALS_BITREV + SPPARK_CIRCLE_FORWARD\n'
            '         + (SPPARK_CIRCLE_EVALS_NATURAL != 1) + (SPPARK_CIRCLE_INVERSE != 1) + (SPPARK_CIRCLE_MAX_LG != 30); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_circle_symbols_in_m31_only(libs):
    assert len(libs) == 11
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        for fn in SYMBOLS:
            assert hasattr(L, fn) == (name == "m31"), (name, fn)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_circle_calls_fail_loudly_without_a_device(libs):
    from sppark_amd import ffi, circle, SpparkError
    L = ffi.load("m31")
    x = np.arange(64, dtype=np.uint32)
    a = np.full(16, 7, dtype=np.uint32)
    for direction in (0, 1):
        for order in (0, 1):
            err = L.sppark_circle_ntt(0, x.ctypes.data, 6, 1, 0, order, direction, None)
            assert err.code < 0 and err.code != INVALID and _message(L, err)
    err = L.sppark_circle_lde(0, x.ctypes.data, 4, 2, 1, 0, a.ctypes.data, None)
    assert err.code < 0 and err.code != INVALID and _message(L, err)
    err = L.sppark_circle_release_cached(0)
    assert err.code < 0 and _message(L, err)
    assert L.sppark_circle_cached_bytes(0) == 0
    with pytest.raises(SpparkError):
        circle.evaluate(0, x)
    assert (x == np.arange(64)).all() and (a == 7).all()


def test_circle_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    L = ffi.load("m31")
    x = np.arange(64, dtype=np.uint32)
    p = x.ctypes.data
    huge = (1 << 64) - 1
    bad = [
        ("lg above 30", lambda: L.sppark_circle_ntt(0, p, 31, 1, 0, 0, 0, None)),
        ("order", lambda: L.sppark_circle_ntt(0, p, 4, 1, 0, 2, 0, None)),
        ("order", lambda: L.sppark_circle_ntt(0, p, 4, 1, 0, -1, 0, None)),
        ("direction", lambda: L.sppark_circle_ntt(0, p, 4, 1, 0, 0, 2, None)),
        ("stride", lambda: L.sppark_circle_ntt(0, p, 4, 2, 15, 0, 0, None)),
        ("stride", lambda: L.sppark_circle_ntt(0, p, 4, 1, 1, 0, 0, None)),
        ("overflow", lambda: L.sppark_circle_ntt(0, p, 4, huge, 16, 0, 0, None)),
        ("overflow", lambda: L.sppark_circle_ntt(0, p, 4, 3, huge // 2, 0, 0, None)),
        ("NULL", lambda: L.sppark_circle_ntt(0, None, 4, 1, 0, 0, 0, None)),
        ("lg + lg_blowup above 30", lambda: L.sppark_circle_lde(0, p, 20, 11, 1, 0, None, None)),
        ("lg + lg_blowup above 30", lambda: L.sppark_circle_lde(0, p, 31, 0, 1, 0, None, None)),
        ("lg + lg_blowup above 30", lambda: L.sppark_circle_lde(0, p, 1, (1 << 32) - 1, 1, 0, None, None)),
        ("order", lambda: L.sppark_circle_lde(0, p, 2, 2, 1, 5, None, None)),
        ("overflow", lambda: L.sppark_circle_lde(0, p, 2, 2, huge // 4, 0, None, None)),
        ("NULL", lambda: L.sppark_circle_lde(0, None, 2, 2, 1, 0, None, None)),
    ]
    for what, call in bad:
        err = call()
        msg = _message(L, err)
        assert err.code == INVALID and b"sppark_circle_" in msg and b"invalid argument" in msg, (what, err.code, msg)
    assert (x == np.arange(64)).all()
    # no-ops succeed with or without a device, whatever the pointer
    for call in (lambda: L.sppark_circle_ntt(0, p, 4, 0, 0, 0, 0, None), lambda: L.sppark_circle_ntt(0, None, 0, 5, 0, 1, 1, None),
                 lambda: L.sppark_circle_ntt(0, p, 0, 64, 1, 0, 0, None), lambda: L.sppark_circle_lde(0, None, 3, 1, 0, 0, None, None)):
        err = call()
        assert err.code == 0 and not err.message
    assert (x == np.arange(64)).all()


def test_circle_wrappers_reject_bad_input():
    from sppark_amd import circle
    for bad in (np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.float32), np.zeros(12, dtype=np.uint32),
                np.zeros(0, dtype=np.uint32), np.zeros((2, 2, 4), dtype=np.uint32), np.zeros((4, 24), dtype=np.uint32),
                np.zeros((4, 32), dtype=np.uint32)[:, ::2], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            circle.ntt(0, bad, circle.FORWARD)
    x = np.zeros(16, dtype=np.uint32)
    with pytest.raises(ValueError):
        circle.ntt(0, x, 2)
    with pytest.raises(ValueError):
        circle.ntt(0, x, circle.FORWARD, 3)
    ext = np.zeros((2, 64), dtype=np.uint32)
    for aux in (np.zeros((2, 8), dtype=np.uint32), np.zeros((1, 16), dtype=np.uint32), np.zeros((2, 16), dtype=np.uint64),
                np.zeros(32, dtype=np.uint32), np.zeros((2, 32), dtype=np.uint32)[:, :16]):
        with pytest.raises(ValueError):
            circle.lde(0, ext, 4, 2, aux_out=aux)
    with pytest.raises(ValueError):
        circle.lde(0, ext, 4, 3)
    with pytest.raises(ValueError):
        circle.lde(0, ext, 28, 3)
    with pytest.raises(ValueError):
        circle.lde(0, np.zeros((2, 128), dtype=np.uint32)[:, :64], 4, 2)
    with pytest.raises(ValueError):
        circle.domain(31)
    assert (ext == 0).all()


@pytest.mark.parametrize("k", range(0, 15))
def test_circle_domain_equals_the_model(k):
    from sppark_amd import circle
    for order in (M.BITREV, M.NATURAL):
        d = circle.domain(k, order)
        assert d.dtype == np.uint32 and d.shape == (1 << k, 2)
        assert (d == M.domain(k, order)).all()
    # the definition itself, point by point in Python integers (circle.domain and the model's share their table scheme)
    direct = M.domain_direct(k)
    assert circle.domain(k, M.NATURAL).tolist() == [list(p) for p in direct]
    assert circle.domain(k, M.BITREV).tolist() == [list(direct[M.bitrev(q, k)]) for q in range(1 << k)]
