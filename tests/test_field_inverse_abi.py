"""CPU: include/sppark_amd_field.h -- the field-vector inverse and quotient -- compiles as plain C and C++, every product
library exports both calls, they fail loudly without a device, reject bad arguments before a device is looked up, and the
Python wrappers reject bad shapes before they reach the library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def test_field_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_field.h"\n'
            'int main(void) { SppError (*f)(size_t, void *, const void *, size_t, void *) = sppark_field_inverse;\n'
            '  SppError (*g)(size_t, void *, const void *, const void *, size_t, void *) = sppark_field_divide;\n'
            '  return (f == 0) + (g == 0); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_field_symbols_exported_by_every_library(libs):
    assert len(libs) == 11
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        assert hasattr(L, "sppark_field_inverse"), name
        assert hasattr(L, "sppark_field_divide"), name


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_field_calls_fail_loudly_without_a_device(libs):
    from sppark_amd import ffi
    for name in ("gl64", "bls12_381", "m31"):
        L = ffi.load(name)
        a = np.ones(64, dtype=np.uint64); b = np.ones(64, dtype=np.uint64); c = np.ones(64, dtype=np.uint64)
        err = L.sppark_field_inverse(0, a.ctypes.data, b.ctypes.data, 8, None)
        assert err.code < 0 and _message(L, err), name
        err = L.sppark_field_divide(0, a.ctypes.data, b.ctypes.data, c.ctypes.data, 8, None)
        assert err.code < 0 and _message(L, err), name


def test_field_calls_reject_bad_arguments_before_the_device(libs):
    """partial overlaps and NULL buffers: the same error protocol with or without a device"""
    from sppark_amd import ffi
    for name, eb in (("gl64", 8), ("bls12_381", 32), ("m31", 4), ("bb31x4", 16)):
        L = ffi.load(name)
        buf = np.ones(64 * eb, dtype=np.uint8)
        other = np.ones(64 * eb, dtype=np.uint8)
        p, q = buf.ctypes.data, other.ctypes.data
        for shift in (eb, 3 * eb, -eb + 16 * eb):                  # out starts inside inp / inp starts inside out
            err = L.sppark_field_inverse(0, p + shift, p, 16, None)
            assert err.code < 0 and b"overlap" in _message(L, err), (name, shift)
            err = L.sppark_field_inverse(0, p, p + shift, 16, None)
            assert err.code < 0 and b"overlap" in _message(L, err), (name, shift)
        for args in ((p + eb, p, q), (p, p + eb, q), (p, q, p + eb), (q, p, p + eb), (q, p + 15 * eb, p)):
            err = L.sppark_field_divide(0, args[0], args[1], args[2], 16, None)
            assert err.code < 0 and b"overlap" in _message(L, err), (name, args)
        for args in ((None, p), (p, None)):
            err = L.sppark_field_inverse(0, args[0], args[1], 16, None)
            assert err.code < 0 and _message(L, err), (name, args)
        for args in ((None, p, q), (p, None, q), (p, q, None)):
            err = L.sppark_field_divide(0, args[0], args[1], args[2], 16, None)
            assert err.code < 0 and _message(L, err), (name, args)
        # len * sizeof(element) past size_t
        err = L.sppark_field_inverse(0, p, q, (1 << 64) // eb, None)
        assert err.code < 0 and _message(L, err), name
        # len == 0 succeeds and touches nothing, NULL pointers included
        err = L.sppark_field_inverse(0, None, None, 0, None)
        assert err.code == 0 and not err.message, name
        err = L.sppark_field_divide(0, None, None, None, 0, None)
        assert err.code == 0 and not err.message, name
        assert (buf == 1).all() and (other == 1).all()


def test_field_wrappers_reject_bad_shapes(libs):
    from sppark_amd import poly
    x8, x9 = np.ones(8, dtype=np.uint64), np.ones(9, dtype=np.uint64)
    with pytest.raises(ValueError):
        poly.inverse(x8, x9, field="gl64")
    with pytest.raises(ValueError):
        poly.divide(x8, x9, x8.copy(), field="gl64")
    with pytest.raises(ValueError):
        poly.divide(x8, x8.copy(), x9, field="gl64")
    w3 = np.ones(3, dtype=np.uint64)                                # 24 bytes of a 32-byte field
    with pytest.raises(ValueError):
        poly.inverse(w3, w3, field="bls12_381")
    with pytest.raises(ValueError):
        poly.divide(w3, w3, w3, field="bls12_381")
    with pytest.raises(ValueError):
        poly.inverse(np.ones(4, dtype=np.uint64), w3, field="bls12_381")
