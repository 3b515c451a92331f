"""CPU: the circle transform's kernel phase functions run on the host (tests/emu/emu_circle.cpp), over the steps of the
driver's own route, bit for bit against the host model (tests/circle_model.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import circle_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def emu():
    so = os.path.join(HERE, "emu", "libemu_circle.so")
    src = os.path.join(HERE, "emu", "emu_circle.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max([os.stat(src).st_mtime] + [os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs])
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread",
                               "-DFEATURE_MERSENNE31", "-o", so, src])
    L = ctypes.CDLL(so)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    L.emu_circle_ntt.argtypes = [vp, cu, sz, sz, ci, ci]
    L.emu_circle_lde.argtypes = [vp, cu, cu, sz, ci, vp]
    L.emu_circle_knobs.argtypes = [cu, cu, cu, cu, cu]
    L.emu_circle_knobs.restype = None
    L.emu_circle_route.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), cu]
    L.emu_circle_route.restype = cu
    L.emu_circle_point_entries.restype = cu
    L.emu_circle_knobs(0, 0, 0, 0, 0)
    return L


@pytest.fixture(scope="module")
def L():
    lib = emu()
    yield lib
    lib.emu_circle_knobs(0, 0, 0, 0, 0)


def _rand(rng, *shape):
    return rng.integers(0, M.P, size=shape, dtype=np.uint32)


def _ntt(L, x, k, batch, stride, order, direction):
    assert L.emu_circle_ntt(x.ctypes.data, k, batch, stride, order, direction) == 0


@pytest.mark.parametrize("k", range(1, 17))
def test_single_column_every_size(L, k):
    L.emu_circle_knobs(0, 0, 0, 0, 0)
    rng = np.random.default_rng(100 + k)
    c = _rand(rng, 1 << k)
    for order in (M.BITREV, M.NATURAL):
        want = M.forward(c, k, order)
        x = c.copy()
        _ntt(L, x, k, 1, 0, order, M.FORWARD)
        assert (x == want).all(), (k, order, "forward")
        _ntt(L, x, k, 1, 0, order, M.INVERSE)
        assert (x == c).all(), (k, order, "inverse")
        e = _rand(rng, 1 << k)
        y = e.copy()
        _ntt(L, y, k, 1, 0, order, M.INVERSE)
        assert (y == M.inverse(e, k, order)).all(), (k, order, "inverse of random evaluations")


def test_edge_inputs(L):
    L.emu_circle_knobs(0, 0, 0, 0, 0)
    for k in (1, 2, 5, 12, 14):
        n = 1 << k
        top = np.zeros(n, dtype=np.uint32)
        top[n - 1] = 1
        for c in (np.full(n, M.P - 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32), top):
            for direction, model in ((M.FORWARD, M.forward), (M.INVERSE, M.inverse)):
                x = c.copy()
                _ntt(L, x, k, 1, 0, M.BITREV, direction)
                assert (x == model(c, k)).all(), (k, direction)


@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("k", [1, 2, 3, 6, 7, 11, 12, 13])
def test_batches_with_stride_and_guards(L, k, batch):
    L.emu_circle_knobs(0, 0, 0, 0, 0)
    rng = np.random.default_rng(7 * k + batch)
    n = 1 << k
    for pad, off in ((5, 0), (8, 0), (4, 1)):           # unaligned columns, aligned columns, unaligned first column
        stride = n + pad
        buf = _rand(rng, batch * stride + off)
        for order in (M.BITREV, M.NATURAL):
            for direction, model in ((M.FORWARD, M.forward), (M.INVERSE, M.inverse)):
                x = buf.copy()
                view = x[off:]
                assert L.emu_circle_ntt(view.ctypes.data, k, batch, stride, order, direction) == 0
                cols = buf[off:].reshape(batch, stride)[:, :n]
                got = x[off:].reshape(batch, stride)
                assert (got[:, :n] == model(cols, k, order)).all(), (k, batch, pad, order, direction)
                assert (got[:, n:] == buf[off:].reshape(batch, stride)[:, n:]).all(), "guard elements were touched"
                assert (x[:off] == buf[:off]).all()


def test_batch_beyond_one_launch(L):
    L.emu_circle_knobs(0, 0, 0, 7, 0)                   # a grid-y limit of 7: 100 columns take several launches
    try:
        rng = np.random.default_rng(5)
        for k in (2, 6, 13):
            c = _rand(rng, 100, 1 << k)
            for order in (M.BITREV, M.NATURAL):
                x = c.copy()
                _ntt(L, x, k, 100, 0, order, M.FORWARD)
                assert (x == M.forward(c, k, order)).all(), (k, order)
    finally:
        L.emu_circle_knobs(0, 0, 0, 0, 0)


@pytest.mark.parametrize("low,high", [(2, 2), (3, 2), (4, 3), (5, 8)])
def test_other_pass_shapes(L, low, high):
    """Small passes make every size a multi-pass one: the tile geometry of the passes above the lowest, at sizes a host test can afford."""
    L.emu_circle_knobs(low, high, 0, 0, 0)
    try:
        rng = np.random.default_rng(low * 16 + high)
        for k in range(1, 15):
            c = _rand(rng, 2, 1 << k)
            x = c.copy()
            _ntt(L, x, k, 2, 0, M.BITREV, M.FORWARD)
            assert (x == M.forward(c, k)).all(), (k, "forward")
            _ntt(L, x, k, 2, 0, M.BITREV, M.INVERSE)
            assert (x == c).all(), (k, "inverse")
    finally:
        L.emu_circle_knobs(0, 0, 0, 0, 0)


def test_unaligned_path_equals_aligned(L):
    rng = np.random.default_rng(9)
    for k in (2, 9, 13):
        c = _rand(rng, 3, 1 << k)
        L.emu_circle_knobs(0, 0, 0, 0, 1)
        try:
            x = c.copy()
            _ntt(L, x, k, 3, 0, M.NATURAL, M.FORWARD)
        finally:
            L.emu_circle_knobs(0, 0, 0, 0, 0)
        assert (x == M.forward(c, k, M.NATURAL)).all()


@pytest.mark.parametrize("k", range(0, 11))
def test_lde(L, k):
    L.emu_circle_knobs(0, 0, 0, 0, 0)
    rng = np.random.default_rng(300 + k)
    for b in (1, 2, 3):
        for order in (M.BITREV, M.NATURAL):
            for batch in (1, 3):
                e = _rand(rng, batch, 1 << k)
                coeffs, want = M.lde(e, k, b, order)
                for with_aux in (False, True):
                    buf = _rand(rng, batch, 1 << (k + b))        # garbage above the evaluations: never read
                    buf[:, :1 << k] = e
                    aux = np.zeros((batch, 1 << k), dtype=np.uint32)
                    assert L.emu_circle_lde(buf.ctypes.data, k, b, batch, order, aux.ctypes.data if with_aux else None) == 0
                    assert (buf == want).all(), (k, b, order, batch)
                    if with_aux:
                        assert (aux == coeffs).all()
