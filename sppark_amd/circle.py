"""Circle transform over Mersenne31 (include/sppark_amd_circle.h): evaluate, interpolate and LDE on the GPU through
libsppark_m31, plus the domain points on the host."""
import enum

import numpy as np

from . import ffi

P = (1 << 31) - 1
GENERATOR = (2, 1268011823)            # of order 2^31 in the circle group x^2 + y^2 = 1
MAX_LG = 30


class EvalsOrder(enum.IntEnum):
    BITREV = 0
    NATURAL = 1


class Direction(enum.IntEnum):
    FORWARD = 0
    INVERSE = 1


BITREV, NATURAL = EvalsOrder.BITREV, EvalsOrder.NATURAL
FORWARD, INVERSE = Direction.FORWARD, Direction.INVERSE


def _is_u32(x):
    if hasattr(x, "data_ptr"):
        import torch
        # torch has no arithmetic on uint32; int32 tensors carry the same 32 bits
        return x.dtype in (torch.uint32, torch.int32)
    return isinstance(x, np.ndarray) and x.dtype == np.uint32


def _columns(x, what):
    """(address, rows, elements per row, row stride in elements) of a 1-D or 2-D uint32 buffer, one column of the batch per row."""
    if not (hasattr(x, "data_ptr") or isinstance(x, np.ndarray)):
        raise ValueError("%s must be a numpy array or a torch tensor" % what)
    if not _is_u32(x):
        raise ValueError("%s must hold 32-bit unsigned elements (numpy uint32; torch uint32 or int32)" % what)
    shape = tuple(int(v) for v in x.shape)
    if len(shape) not in (1, 2):
        raise ValueError("%s must be 1-D or 2-D: one polynomial per row" % what)
    if hasattr(x, "data_ptr"):
        st = [int(v) for v in x.stride()]
        ptr = x.data_ptr()
    else:
        if x.ndim and any(s % 4 for s in x.strides):
            raise ValueError("%s: strides must be whole elements" % what)
        st = [int(v) // 4 for v in x.strides]
        ptr = x.ctypes.data
    rows, n = (1, shape[0]) if len(shape) == 1 else shape
    if n > 1 and st[-1] != 1:
        raise ValueError("%s: the inner stride must be 1" % what)
    stride = st[0] if len(shape) == 2 and rows > 1 else n
    if stride < n:
        raise ValueError("%s: rows must not overlap" % what)
    return ptr, rows, n, stride


def _lg(n, what):
    if n == 0 or n & (n - 1):
        raise ValueError("%s: the row length is not a power of 2" % what)
    if n > 1 << MAX_LG:
        raise ValueError("%s: rows above 2^%d elements" % (what, MAX_LG))
    return n.bit_length() - 1


def ntt(device_id, x, direction, evals_order=BITREV, stream=None):
    """sppark_circle_ntt, in place: every row of |x| (1-D or 2-D uint32 numpy array or torch tensor, host or device,
    canonical residues; any row stride that keeps rows apart) is evaluated on D_k (FORWARD) or interpolated (INVERSE)."""
    direction, evals_order = Direction(direction), EvalsOrder(evals_order)
    ptr, rows, n, stride = _columns(x, "x")
    lg = _lg(n, "x")
    L = ffi.load("m31")
    ffi.check(L, L.sppark_circle_ntt(device_id, ptr, lg, rows, stride, int(evals_order), int(direction), stream))
    return x


def evaluate(device_id, x, evals_order=BITREV, stream=None):
    return ntt(device_id, x, FORWARD, evals_order, stream)


def interpolate(device_id, x, evals_order=BITREV, stream=None):
    return ntt(device_id, x, INVERSE, evals_order, stream)


def lde(device_id, ext, lg, lg_blowup, evals_order=BITREV, aux_out=None, stream=None):
    """sppark_circle_lde, in place: |ext| is 2^(lg+lg_blowup) elements or (batch, 2^(lg+lg_blowup)) with packed rows; the
    first 2^lg elements of each row hold evaluations on D_lg and the row receives the evaluations on D_(lg+lg_blowup) in
    the same order.  aux_out (optional, 2^lg or (batch, 2^lg), packed) receives the coefficients."""
    evals_order = EvalsOrder(evals_order)
    if lg < 0 or lg_blowup < 0 or lg + lg_blowup > MAX_LG:
        raise ValueError("lg + lg_blowup must be within 0 .. %d" % MAX_LG)
    ptr, rows, n, stride = _columns(ext, "ext")
    if n != 1 << (lg + lg_blowup) or stride != n:
        raise ValueError("ext must be (batch, 2^(lg+lg_blowup)) with packed rows")
    aptr = None
    if aux_out is not None:
        aptr, arows, an, astride = _columns(aux_out, "aux_out")
        if arows != rows or an != 1 << lg or astride != an:
            raise ValueError("aux_out must be (batch, 2^lg) with packed rows")
    L = ffi.load("m31")
    ffi.check(L, L.sppark_circle_lde(device_id, ptr, lg, lg_blowup, rows, int(evals_order), aptr, stream))
    return ext


def cached_bytes(device_id=0):
    return int(ffi.load("m31").sppark_circle_cached_bytes(device_id))


def release_cached(device_id=0):
    L = ffi.load("m31")
    ffi.check(L, L.sppark_circle_release_cached(device_id))


# ---- the domain, on the host: D_i = g_{k+1}^(4i+1) for i < n/2, its conjugate for i >= n/2, by exponent arithmetic ----
_TABLES = None


def _cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _gpow(e):
    r, b = (1, 0), GENERATOR
    while e:
        if e & 1:
            r = _cmul(r, b)
        b = _cmul(b, b)
        e >>= 1
    return r


def _tables():
    global _TABLES
    if _TABLES is None:
        def tab(count, step):
            out, s, cur = np.zeros((count, 2), dtype=np.uint64), _gpow(step), (1, 0)
            for i in range(count):
                out[i] = cur
                cur = _cmul(cur, s)
            return out
        _TABLES = (tab(1 << 10, 1), tab(1 << 11, 1 << 10), tab(1 << 10, 1 << 21))
    return _TABLES


def _vmul(a, b):
    ax, ay, bx, by = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    return np.stack([(ax * bx % P + (P - ay * by % P)) % P, (ax * by % P + ay * bx % P) % P], axis=-1)


def domain(lg, evals_order=NATURAL):
    """The (2^lg, 2) uint32 array of the points (x, y) of D_lg, row q being the point whose evaluation sits at position q
    of a transform in |evals_order|.  Host only."""
    evals_order = EvalsOrder(evals_order)
    if not 0 <= lg <= MAX_LG:
        raise ValueError("lg must be within 0 .. %d" % MAX_LG)
    n = 1 << lg
    if lg == 0:
        return np.array([[1, 0]], dtype=np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    if evals_order == BITREV:
        r = np.zeros_like(idx)
        for i in range(lg):
            r |= ((idx >> np.uint64(i)) & np.uint64(1)) << np.uint64(lg - 1 - i)
        idx = r
    half = np.uint64(n // 2)
    e = (np.uint64(4) * (idx % half) + np.uint64(1)) << np.uint64(30 - lg)
    t0, t1, t2 = _tables()
    pts = _vmul(_vmul(t2[(e >> np.uint64(21)).astype(np.int64)], t1[((e >> np.uint64(10)) & np.uint64(0x7ff)).astype(np.int64)]),
                t0[(e & np.uint64(0x3ff)).astype(np.int64)])
    conj = idx >= half
    pts[conj, 1] = (P - pts[conj, 1]) % P
    return pts.astype(np.uint32)
