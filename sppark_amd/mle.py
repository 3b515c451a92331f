"""Multilinear tables and sumcheck rounds: host API over sppark_mle_fold / sppark_mle_evaluate / sppark_mle_eq /
sppark_sumcheck_round (include/sppark_amd_mle.h; no counterpart in the reference).
A table holds n = 2^lg_n field elements in the wire format of the chosen library (see sppark_amd.poly); index bit j is
variable j.  Buffers are numpy arrays or torch tensors, host or device."""
import ctypes

import numpy as np

from . import ffi
from .poly import _ELEM_BYTES, _count

LOW, HIGH = 0, 1
PRODUCT, EQ_MUL_SUB = 0, 1
_FORMS = {"product": PRODUCT, "eq_mul_sub": EQ_MUL_SUB, PRODUCT: PRODUCT, EQ_MUL_SUB: EQ_MUL_SUB}
MAX_LG = 32


def _row_shape(field):
    """(word dtype, words per element) of a result row"""
    eb = _ELEM_BYTES[field]
    dtype = np.uint32 if eb in (4, 16) else np.uint64
    return dtype, eb // np.dtype(dtype).itemsize


def _lg(n, what):
    if n == 0 or n & (n - 1):
        raise ValueError("%s must hold a power of two of field elements" % what)
    lg = n.bit_length() - 1
    if lg > MAX_LG:
        raise ValueError("%s holds more than 2^%d elements" % (what, MAX_LG))
    return lg


def _order(order):
    if order not in (LOW, HIGH):
        raise ValueError("order must be mle.LOW or mle.HIGH")
    return int(order)


def fold(out, table, r, order=LOW, field="gl64", device_id=0, stream=None):
    """out[i] = lo_i + r * (hi_i - lo_i) for the n/2 pairs of |order| (LOW: (table[2i], table[2i+1]), HIGH: (table[i],
    table[i + n/2])); r: one element, on the host or the device.  HIGH: out may be table itself (its first half is
    overwritten).  With device buffers and a stream the call only enqueues."""
    L = ffi.load(field)
    n = _count(table, field)
    lg = _lg(n, "table")
    if lg == 0:
        raise ValueError("a table of one element has no variable to bind")
    _order(order)
    po, _k1 = ffi.as_pointer(out); pt, _k2 = ffi.as_pointer(table); pr, _k3 = ffi.as_pointer(r)
    same = po == pt                                         # in place: out is the table's own buffer
    if _count(out, field) != (n if same else n // 2):
        raise ValueError("out must hold n / 2 elements (or be the table itself)")
    if same and order != HIGH:
        raise ValueError("only a HIGH fold may run in place")
    if _count(r, field) != 1:
        raise ValueError("r must be one field element")
    ffi.check(L, L.sppark_mle_fold(device_id, po, pt, lg, pr, int(order), stream))
    return out


def evaluate(table, point, field="gl64", device_id=0, stream=None):
    """the multilinear extension of |table| at |point| (lg_n elements, variable 0 first): one element as a numpy row"""
    L = ffi.load(field)
    lg = _lg(_count(table, field), "table")
    npoint = _count(point, field) if point is not None else 0
    if npoint != lg:
        raise ValueError("point must hold lg_n elements")
    dtype, w = _row_shape(field)
    ret = np.zeros(w, dtype=dtype)
    pt, _k1 = ffi.as_pointer(table)
    pp, _k2 = ffi.as_pointer(point) if lg else (None, None)
    ffi.check(L, L.sppark_mle_evaluate(device_id, ret.ctypes.data, pt, lg, pp, stream))
    return ret


def eq(out, point, field="gl64", device_id=0, stream=None):
    """out[i] = prod_j (i_j ? point[j] : 1 - point[j]) for the 2^len(point) indices i"""
    L = ffi.load(field)
    lg = _lg(_count(out, field), "out")
    npoint = _count(point, field) if point is not None else 0
    if npoint != lg:
        raise ValueError("point must hold lg_n elements")
    po, _k1 = ffi.as_pointer(out)
    pp, _k2 = ffi.as_pointer(point) if lg else (None, None)
    ffi.check(L, L.sppark_mle_eq(device_id, po, pp, lg, stream))
    return out


def round(tables, form="product", order=LOW, field="gl64", device_id=0, stream=None):      # noqa: A001 (the issue's name)
    """One sumcheck round polynomial as its values s(0) .. s(d), a numpy array of shape (d + 1, words per element).
    form "product": s(t) = sum_i prod_k f_k,i(t) over 1 .. 4 tables, d = len(tables); form "eq_mul_sub": tables = (e, a, b, c),
    s(t) = sum_i e_i(t) * (a_i(t) * b_i(t) - c_i(t)), d = 3.  f_k,i(t) = lo + t * (hi - lo) on the pairs of |order|."""
    L = ffi.load(field)
    if form not in _FORMS:
        raise ValueError("form must be 'product' or 'eq_mul_sub'")
    form = _FORMS[form]
    tables = list(tables)
    if (form == PRODUCT and not 1 <= len(tables) <= 4) or (form == EQ_MUL_SUB and len(tables) != 4):
        raise ValueError("product takes 1 .. 4 tables, eq_mul_sub exactly 4 (e, a, b, c)")
    _order(order)
    n = _count(tables[0], field)
    lg = _lg(n, "a table")
    if lg == 0:
        raise ValueError("a table of one element has no pair")
    for t in tables[1:]:
        if _count(t, field) != n:
            raise ValueError("length mismatch")
    dtype, w = _row_shape(field)
    rows = len(tables) + 1 if form == PRODUCT else 4
    out = np.zeros((rows, w), dtype=dtype)
    ptrs = [ffi.as_pointer(t) for t in tables]
    arr = (ctypes.c_void_p * len(tables))(*[p for p, _keep in ptrs])
    ffi.check(L, L.sppark_sumcheck_round(device_id, out.ctypes.data, arr, len(tables), form, lg, int(order), stream))
    return out
