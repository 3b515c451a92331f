"""CPU: k_ntt_small_packed, the batched NTT's kernel for columns of 2^1 ... 2^6 elements (256 / (n/2) of them per work-group
of 256 lanes), on the host (tests/emu/emu_ntt_batch.cpp: the kernel's own lane function ntt_packed_lane, its lanes as host
threads) against the oracle, column by column: every size it takes, all 16 modes, batches that fill one segment, leave a
partial wave and a partial work-group, and span several work-groups; columns |stride| elements apart with untouched gaps.
The other sizes (one column per grid row of the single-transform kernels) are held against sppark_ntt on the GPU,
tests/test_ntt_batch_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import recipe

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = [("gl64", "GOLDILOCKS"), ("bb31", "BABY_BEAR"), ("bls12_381", "BLS12_381"), ("bn254", "BN254")]
WIDE = ("bls12_381", "bn254")


def _emu(feature):
    so = os.path.join(HERE, "emu", "libemu_ntt_batch_%s.so" % feature)
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_ntt_batch.cpp", "emu_ntt.cpp")]
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max([os.stat(s).st_mtime for s in srcs] + [os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs])
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread",
                               "-DFEATURE_" + feature, "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    L.emu_ntt_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.emu_ntt_batch.restype = ctypes.c_int
    return L


def _oracle_ntt(O, field):
    if field in WIDE:
        curve = O.BLS12_381 if field == "bls12_381" else O.BN254
        return lambda x, order, direction, typ: O.ntt_fr(curve, x, order, direction, typ)
    return O.ntt_gl64 if field == "gl64" else O.ntt_bb31


def _columns(field, lg, batch, stride, seed):
    """(buffer of batch columns |stride| apart, gaps filled with a sentinel; the columns as a list)"""
    cols = [recipe.ntt_input(field, lg, seed + j) for j in range(batch)]
    shape = (batch, stride) + cols[0].shape[1:]
    buf = np.full(shape, 0x5A, dtype=cols[0].dtype)
    for j, c in enumerate(cols):
        buf[j, :1 << lg] = c
    return buf, cols


@pytest.mark.parametrize("field,feature", FIELDS)
def test_packed_small_columns_on_host(oracle, field, feature):
    L = _emu(feature)
    f = _oracle_ntt(oracle, field)
    for lg in range(1, 7):
        nh = 1 << (lg - 1)
        # one column; a partial wave; a partial work-group; several work-groups with a partial last one
        batches = sorted({2, 3, 64 // nh + 1, 256 // nh - 1, 256 // nh + 5} if field not in WIDE else {2, 64 // nh + 1, 256 // nh + 5})
        for batch in batches:
            for stride in ((1 << lg), (1 << lg) + 3):
                buf, cols = _columns(field, lg, batch, stride, 1000 * lg + batch)
                for mode in range(16):
                    order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
                    if field in WIDE and batch > 2 and mode not in (1, 6, 11, 12):
                        continue                                # (256-bit fields: every mode on two columns, four at the larger batches)
                    y = buf.copy()
                    assert L.emu_ntt_batch(y.ctypes.data, lg, batch, stride, order, direction, typ) == 1
                    for j, c in enumerate(cols):
                        assert (y[j, :1 << lg] == f(c, order, direction, typ)).all(), (field, lg, batch, stride, mode, j)
                    assert (y[:, 1 << lg:] == buf[:, 1 << lg:]).all(), "gap written"
