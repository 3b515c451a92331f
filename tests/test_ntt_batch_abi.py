"""CPU: include/sppark_amd_batch.h -- the batched NTT / LDE -- compiles as plain C and C++, every library with an NTT exports
exactly what it declares (m31 / bb31x4 none of it), the calls fail loudly without a device, and the Python wrappers reject
bad shapes before they reach the library."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NTT_LIBS = ("gl64", "bb31", "gl64_plonky2", "bb31_canonical", "bls12_381", "bn254", "bls12_377", "pallas", "vesta")


def batch_symbols():
    hdr = open(os.path.join(INC, "sppark_amd_batch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"^#.*$", "", hdr, flags=re.M)
    return sorted(set(re.findall(r"\b(\w+)\s*\([^;{}]*\)\s*;", hdr)) - {"defined"})


def test_batch_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_batch.h"\n'
            'int main(void) { SppError (*f)(size_t, void *, uint32_t, size_t, size_t, int, int, int, void *) = sppark_ntt_batch;\n'
            '  SppError (*g)(size_t, void *, uint32_t, uint32_t, size_t, void *, void *) = sppark_lde_batch;\n'
            '  return (f == 0) + (g == 0) + (SPPARK_BATCH_CHUNK_BYTES != ((size_t)256 << 20)); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_batch_symbols_exported_exactly(libs):
    syms = batch_symbols()
    assert syms == ["sppark_lde_batch", "sppark_ntt_batch", "sppark_ntt_batch_launch_cols"]
    for name, path in libs.items():
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        have = {s for s in re.findall(r"\b(sppark_\w*batch\w*)\b", exported)} - {"sppark_batch_addition"}   # (an MSM helper)
        if name in ("m31", "bb31x4"):
            assert have == set(), (name, have)
        else:
            assert name in NTT_LIBS
            assert have == set(syms), (name, have)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_batch_calls_fail_loudly_without_a_device(libs):
    from sppark_amd import ffi
    for name in ("gl64", "bls12_381"):
        L = ffi.load(name)
        buf = np.zeros(64, dtype=np.uint64)
        err = L.sppark_ntt_batch(0, buf.ctypes.data, 2, 4, 0, 1, 0, 0, None)
        assert err.code < 0 and ctypes.string_at(err.message)
        L.drop_error_message(err.message)
        err = L.sppark_lde_batch(0, buf.ctypes.data, 1, 1, 4, None, None)
        assert err.code < 0 and ctypes.string_at(err.message)
        L.drop_error_message(err.message)
        assert L.sppark_ntt_batch_launch_cols(0, 12) == 0
        # rejected arguments: the same error protocol, before any device is looked for
        err = L.sppark_ntt_batch(0, buf.ctypes.data, 2, 4, 0, 7, 0, 0, None)
        assert err.code < 0 and b"ntt_order" in ctypes.string_at(err.message)
        L.drop_error_message(err.message)
        err = L.sppark_ntt_batch(0, buf.ctypes.data, 3, 4, 5, 1, 0, 0, None)
        assert err.code < 0 and b"stride" in ctypes.string_at(err.message)
        L.drop_error_message(err.message)


def test_batch_wrappers_reject_bad_shapes():
    import sppark_amd
    bad = [np.zeros(16, dtype=np.uint64),                          # 1-D
           np.zeros((2, 3, 4), dtype=np.uint64),                   # 3-D
           np.zeros((4, 6), dtype=np.uint64),                      # rows of 6 elements
           np.zeros((4, 16), dtype=np.uint64)[:, ::2],             # inner stride 2
           np.zeros((4, 16), dtype=np.uint64)[::-1],               # rows backwards
           np.zeros((4, 0), dtype=np.uint64)]                      # empty rows
    for x in bad:
        with pytest.raises(ValueError):
            sppark_amd.compute_ntt_batch(0, x, 1, 0, 0, "gl64")
    with pytest.raises(ValueError):                                # 24-byte rows of a 32-byte field
        sppark_amd.compute_ntt_batch(0, np.zeros((4, 3), dtype=np.uint64), 1, 0, 0, "bls12_381")
    with pytest.raises(ValueError):                                # overlapping rows (as_strided view)
        x = np.lib.stride_tricks.as_strided(np.zeros(64, dtype=np.uint64), shape=(4, 16), strides=(8 * 8, 8))
        sppark_amd.compute_ntt_batch(0, x, 1, 0, 0, "gl64")
    with pytest.raises(ValueError):                                # LDE: rows must be 2^(lg+lgb)
        sppark_amd.LDE_batch(0, np.zeros((4, 8), dtype=np.uint64), 2, 2, "gl64")
    with pytest.raises(ValueError):                                # LDE: packed rows only
        sppark_amd.LDE_batch(0, np.zeros((4, 32), dtype=np.uint64)[:, :16], 2, 2, "gl64")
    with pytest.raises(ValueError):                                # LDE: aux_out shape
        sppark_amd.LDE_batch(0, np.zeros((4, 16), dtype=np.uint64), 2, 2, "gl64", aux_out=np.zeros((3, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        sppark_amd.compute_ntt_batch(0, np.zeros((4, 16), dtype=np.uint32), 1, 0, 0, "m31")
    try:
        import torch
    except ImportError:
        return
    with pytest.raises(ValueError):                                # torch column view: inner stride != 1
        sppark_amd.compute_ntt_batch(0, torch.zeros(16, 4, dtype=torch.int64).t(), 1, 0, 0, "gl64")
