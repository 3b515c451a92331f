"""CPU: the multilinear-table kernels' phase functions run on the host (tests/emu/emu_mle.cpp), over the steps of the
driver's own route, bit for bit against the host model (tests/mle_model.py): every lg_n from 0 (1 for fold and round) to
T + 2, both orders, every table count, both forms, the 16-byte and the element-wise instance."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import mle_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FEATURE = {"gl64": "GOLDILOCKS", "bb31": "BABY_BEAR", "bb31x4": "BABY_BEAR_X4", "bls12_381": "BLS12_381"}
# csrc/mle/mle_route.hpp mle_tile_lg: log2 elements of a tile (64 bytes per lane, 256 lanes)
MLE_T = {"gl64": 11, "bb31": 12, "bb31x4": 10, "bls12_381": 9}
CUS = 3                                                     # a small device: 24 work-groups, so that work-groups loop
FORMS = [(M.PRODUCT, 1), (M.PRODUCT, 2), (M.PRODUCT, 3), (M.PRODUCT, 4), (M.EQ_MUL_SUB, 4)]


@functools.lru_cache(maxsize=None)
def emu(field):
    so = os.path.join(HERE, "emu", "libemu_mle_%s.so" % field)
    src = os.path.join(HERE, "emu", "emu_mle.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max([os.stat(src).st_mtime] + [os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs])
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-DFEATURE_" + FEATURE[field], "-o", so, src])
    L = ctypes.CDLL(so)
    vp, cu, ci = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int
    L.emu_mle_fold.argtypes = [vp, vp, cu, vp, ci, cu, ci]
    L.emu_mle_evaluate.argtypes = [vp, vp, cu, vp, cu, ci]
    L.emu_mle_eq.argtypes = [vp, vp, cu, cu, ci]
    L.emu_mle_round.argtypes = [vp, ctypes.POINTER(vp), cu, ci, cu, ci, cu, ci]
    L.emu_mle_route.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), cu]
    L.emu_mle_route.restype = cu
    L.emu_mle_elem_bytes.restype = cu
    L.emu_mle_tile_lg.restype = cu
    return L


@functools.lru_cache(maxsize=None)
def _case(field, lg):
    """(model, four tables as wire rows with the edge values planted, their values, a point) -- never modified"""
    m = M.Model(field)
    n = 1 << lg
    rows = [m.random_rows(n, 1000 * lg + k) for k in range(4)]
    for k, x in enumerate(rows):
        for j, edge in enumerate((0, m.f.one, m.f.pm1)):
            x[(j + k) % n] = edge
        assert m.f.canonical(x).all()
        x.setflags(write=False)
    point = m.random_rows(max(lg, 1), 77 + lg)
    point.setflags(write=False)
    return m, rows, [m.vals(x) for x in rows], point


def _variants(field):
    return (0, 1) if field in ("gl64", "bb31") else (0,)          # (elements of 16 bytes and more have one instance)


@pytest.mark.parametrize("field", list(FEATURE))
def test_geometry(field):
    L = emu(field)
    assert L.emu_mle_tile_lg() == MLE_T[field]
    assert L.emu_mle_elem_bytes() == M.Model(field).f.w * np.dtype(M.Model(field).f.dtype).itemsize


@pytest.mark.parametrize("field", list(FEATURE))
def test_fold(oracle, field):
    L = emu(field)
    for lg in range(1, MLE_T[field] + 3):
        m, rows, vals, point = _case(field, lg)
        r = point[:1].copy()
        for order in (M.LOW, M.HIGH):
            want = m.rows(m.fold(vals[0], m.vals(r)[0], order))
            for unaligned in _variants(field):
                src = rows[0].copy()
                out = np.full((1 << (lg - 1), m.f.w), 5, dtype=m.f.dtype)
                assert L.emu_mle_fold(out.ctypes.data, src.ctypes.data, lg, r.ctypes.data, order, CUS, unaligned) == 0
                assert (out == want).all(), (field, lg, order, unaligned)
                assert (src == rows[0]).all()
            src = rows[0].copy()                                # HIGH in place: the first half is overwritten, the second kept
            if order == M.HIGH:
                assert L.emu_mle_fold(src.ctypes.data, src.ctypes.data, lg, r.ctypes.data, order, CUS, 0) == 0
                h = 1 << (lg - 1)
                assert (src[:h] == want).all() and (src[h:] == rows[0][h:]).all(), (field, lg)


@pytest.mark.parametrize("field", list(FEATURE))
def test_evaluate_and_eq(oracle, field):
    L = emu(field)
    for lg in range(0, MLE_T[field] + 3):
        m, rows, vals, point = _case(field, lg)
        pv = m.vals(point)[:lg]
        want_eq = m.rows(m.eq(pv))
        want_ev = m.row(m.evaluate(vals[0], pv))
        for unaligned in _variants(field):
            out = np.full((1 << lg, m.f.w), 5, dtype=m.f.dtype)
            assert L.emu_mle_eq(out.ctypes.data, point.ctypes.data, lg, CUS, unaligned) == 0
            assert (out == want_eq).all(), (field, lg, unaligned)
            ret = np.full(m.f.w, 5, dtype=m.f.dtype)
            src = rows[0].copy()
            assert L.emu_mle_evaluate(ret.ctypes.data, src.ctypes.data, lg, point.ctypes.data, CUS, unaligned) == 0
            assert (ret == want_ev).all(), (field, lg, unaligned)
            assert (src == rows[0]).all()


@pytest.mark.parametrize("field", list(FEATURE))
def test_round(oracle, field):
    L = emu(field)
    for lg in range(1, MLE_T[field] + 3):
        m, rows, vals, point = _case(field, lg)
        for form, nt in FORMS:
            ptrs = (ctypes.c_void_p * 4)(*[rows[k].ctypes.data for k in range(4)])
            for order in (M.LOW, M.HIGH):
                want = m.rows(m.round(vals[:nt], form, order))
                for unaligned in _variants(field):
                    out = np.full((len(want), m.f.w), 5, dtype=m.f.dtype)
                    assert L.emu_mle_round(out.ctypes.data, ptrs, nt, 1 if form == M.EQ_MUL_SUB else 0, lg, order, CUS, unaligned) == 0
                    assert (out == want).all(), (field, lg, form, nt, order, unaligned)
