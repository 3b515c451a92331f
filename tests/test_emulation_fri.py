"""CPU: the FRI kernels' per-lane functions run on the host (tests/emu/emu_fri.cpp) under the driver's own route, bit for
bit against the host model (tests/fri_model.py).  One CU and one or two work-groups per CU, so that a work-group walks many
tiles and the tile part of the twiddles advances at small sizes: lg_n in {a, a+1, T-1, T, T+1, T+3}, every arity and order,
misaligned pointers (the element-wise instance), and the reduce chunk boundary."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import fri_model as FM

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FEATURE = {"gl64": "GOLDILOCKS", "bb31": "BABY_BEAR", "bb31x4": "BABY_BEAR_X4", "bls12_381": "BLS12_381", "m31": "MERSENNE31"}
FOLD_FIELDS = ["gl64", "bb31", "bb31x4", "bls12_381"]
# csrc/fri/fri_route.hpp fri_tile_lg: log2 elements that 64 bytes per lane make
FRI_T = {"gl64": 11, "bb31": 12, "bb31x4": 10, "bls12_381": 9, "m31": 12}
CHUNK = 512                                                 # FRI_RED_CHUNK
CUS = 1


@functools.lru_cache(maxsize=None)
def emu(field):
    so = os.path.join(HERE, "emu", "libemu_fri_%s.so" % field)
    src = os.path.join(HERE, "emu", "emu_fri.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max([os.stat(src).st_mtime] + [os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs])
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-DFEATURE_" + FEATURE[field], "-o", so, src])
    L = ctypes.CDLL(so)
    vp, cu, ci, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t
    if field != "m31":
        L.emu_fri_fold.argtypes = [vp, vp, cu, cu, vp, vp, ci, cu, ci]
        L.emu_fri_domain.argtypes = [vp, cu, vp, ci, vp, cu, ci]
    L.emu_fri_reduce.argtypes = [vp, vp, ci, cu, sz, sz, sz, vp, vp, ci, cu, ci]
    L.emu_fri_route.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.emu_fri_route.restype = None
    L.emu_fri_set_wg_per_cu.argtypes = [cu]
    for fn in (L.emu_fri_elem_bytes, L.emu_fri_tile_lg, L.emu_fri_red_chunk, L.emu_fri_lazy_terms):
        fn.restype = cu
    return L


def _variants(field):
    return (0, 1) if field in ("gl64", "bb31", "m31") else (0,)      # (elements of 16 bytes and more have one instance)


@functools.lru_cache(maxsize=None)
def _case(field, lg):
    """(model, wire rows with the edge values planted, their values, beta rows, a shift row of the base field)"""
    m = FM.FriModel(field)
    n = 1 << lg
    x = m.random_rows(n, 4000 + lg)
    for j, edge in enumerate((0, m.f.one, m.f.pm1)):
        x[(5 * j + 1) % n] = edge
    x.setflags(write=False)
    beta = m.random_rows(1, 17)
    shift = m.base.random_rows(1, 23)
    return m, x, m.vals(x), beta, shift


def _lgs(field, a):
    T = FRI_T[field]
    return sorted({a, a + 1, T - 1, T, T + 1, T + 3})


@pytest.mark.parametrize("field", list(FEATURE))
def test_geometry(field):
    L = emu(field)
    m = FM.Model(field)
    assert L.emu_fri_tile_lg() == FRI_T[field] and L.emu_fri_red_chunk() == CHUNK and L.emu_fri_lazy_terms() == 4
    assert L.emu_fri_elem_bytes() == m.f.w * np.dtype(m.f.dtype).itemsize


@pytest.mark.parametrize("order", [FM.NATURAL, FM.BITREV])
@pytest.mark.parametrize("a", [1, 2, 3])
@pytest.mark.parametrize("field", FOLD_FIELDS)
def test_fold(oracle, field, a, order):
    L = emu(field)
    for lg in _lgs(field, a):
        m, x, vals, beta, shift = _case(field, lg)
        bv = m.vals(beta)[0]
        for k, (sh_row, wg) in enumerate(((None, 1), (shift, 2))):
            L.emu_fri_set_wg_per_cu(wg)
            want = m.rows(m.fold(vals, a, bv, None if sh_row is None else m.base.vals(sh_row)[0], order))
            sp = None if sh_row is None else sh_row.ctypes.data
            for unaligned in _variants(field):
                src = x.copy()
                out = np.full((1 << (lg - a), m.f.w), 5, dtype=m.f.dtype)
                assert L.emu_fri_fold(out.ctypes.data, src.ctypes.data, lg, a, beta.ctypes.data, sp, order, CUS, unaligned) == 0
                assert (out == want).all(), (field, lg, a, order, wg, unaligned)
                assert (src == x).all()
            if order == FM.NATURAL:                         # in place: the first n / 2^a elements are overwritten, the rest kept
                src = x.copy()
                assert L.emu_fri_fold(src.ctypes.data, src.ctypes.data, lg, a, beta.ctypes.data, sp, order, CUS, 0) == 0
                h = 1 << (lg - a)
                assert (src[:h] == want).all() and (src[h:] == x[h:]).all(), (field, lg, a)


@pytest.mark.parametrize("order", [FM.NATURAL, FM.BITREV])
@pytest.mark.parametrize("field", FOLD_FIELDS)
def test_domain(oracle, field, order):
    L = emu(field)
    T = FRI_T[field]
    for lg in sorted({0, 1, 2, T - 1, T, T + 1, T + 3}):
        m, x, vals, beta, shift = _case(field, max(lg, 1))
        for sh_row, z_row, wg in ((None, None, 1), (shift, beta, 2)):
            L.emu_fri_set_wg_per_cu(wg)
            z = None if z_row is None else m.vals(z_row)[0]
            want = m.rows(m.domain_minus(lg, None if sh_row is None else m.base.vals(sh_row)[0], order, z))
            for unaligned in _variants(field):
                out = np.full((1 << lg, m.f.w), 5, dtype=m.f.dtype)
                assert L.emu_fri_domain(out.ctypes.data, lg, None if sh_row is None else sh_row.ctypes.data, order,
                                        None if z_row is None else z_row.ctypes.data, CUS, unaligned) == 0
                assert (out == want).all(), (field, lg, order, wg, unaligned)


def _matrix(m, e, lg, width, layout, gap, base):
    """(buffer with garbage in the gaps, col_stride, leaf_stride, cols[j][i] as values)"""
    n = 1 << lg
    rows = e.random_rows(n * width, 31 * width + lg).reshape(width, n, e.f.w)
    rows[0, 0] = e.f.pm1
    garbage = np.iinfo(e.f.dtype).max
    if layout == "columns":
        cs = n + gap
        buf = np.full((width, cs, e.f.w), garbage, dtype=e.f.dtype)
        buf[:, :n] = rows
        strides = (cs, 1)
    else:
        ls = width + gap
        buf = np.full((n, ls, e.f.w), garbage, dtype=e.f.dtype)
        buf[:, :width] = rows.transpose(1, 0, 2)
        strides = (1, ls)
    cols = [e.vals(rows[j]) for j in range(width)]
    return buf, strides[0], strides[1], cols


@pytest.mark.parametrize("layout", ["columns", "rows"])
@pytest.mark.parametrize("field,base", [("gl64", 0), ("bb31", 0), ("m31", 0), ("bb31x4", 0), ("bb31x4", 1), ("bls12_381", 0)])
def test_reduce(oracle, field, base, layout):
    L = emu(field)
    m = FM.FriModel(field)
    e = m.base if base else m
    L.emu_fri_set_wg_per_cu(1)
    widths = [1, 2, 3, 5, 64, CHUNK - 1, CHUNK, CHUNK + 1] if e.f.w == 1 else [1, 3, 5, CHUNK - 1, CHUNK, CHUNK + 1]
    for width in widths:
        for lg in ((0, 1, 5, 9, 11) if width == 3 else (0, 1, 5) if width < 64 else (3,)):   # (2^11: a lane takes several leaves)
            for gap in (0, 4, 3):
                buf, cs, ls, cols = _matrix(m, e, lg, width, layout, gap, base)
                w = m.random_rows(width, 5 + width)
                sub, prev = m.random_rows(1, 8), m.random_rows(1 << lg, 9)
                for accumulate, sub_row in ((0, None), (1, sub)):
                    want = m.rows(m.reduce(cols, m.vals(w), None if sub_row is None else m.vals(sub_row)[0],
                                           m.vals(prev) if accumulate else None, base=bool(base)))
                    for unaligned in ((0, 1) if e.f.w == 1 else (0,)):
                        out = prev.copy()
                        assert L.emu_fri_reduce(out.ctypes.data, buf.ctypes.data, base, lg, width, cs, ls, w.ctypes.data,
                                                None if sub_row is None else sub_row.ctypes.data, accumulate, CUS, unaligned) == 0
                        assert (out == want).all(), (field, base, layout, width, lg, gap, accumulate, unaligned)


@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_reduce_lazy_sums_at_their_bound(oracle, layout):
    """every matrix element and every weight component p - 1, 1025 columns: a 64-bit sum that is settled too late wraps"""
    L = emu("bb31x4")
    m = FM.FriModel("bb31x4")
    L.emu_fri_set_wg_per_cu(1)
    width, lg, p = 1025, 3, m.p
    n = 1 << lg
    buf = np.full((width, n) if layout == "columns" else (n, width), p - 1, dtype=np.uint32)
    w = np.full((width, 4), p - 1, dtype=np.uint32)
    cs, ls = (n, 1) if layout == "columns" else (1, width)
    want = m.rows(m.reduce([m.base.vals(np.full(n, p - 1, dtype=np.uint32))] * width, m.vals(w), base=True))
    for unaligned in (0, 1):
        out = np.zeros((n, 4), dtype=np.uint32)
        assert L.emu_fri_reduce(out.ctypes.data, buf.ctypes.data, 1, lg, width, cs, ls, w.ctypes.data, None, 0, CUS, unaligned) == 0
        assert (out == want).all(), (layout, unaligned)
