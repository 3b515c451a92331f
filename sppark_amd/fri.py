"""FRI on the device: host API over sppark_fri_fold / sppark_fri_reduce / sppark_fri_domain (include/sppark_amd_fri.h; no
counterpart in the reference).  Vectors hold n = 2^lg_n field elements in the wire format of the chosen library (see
sppark_amd.poly) on the domain x_i = shift * w^i (NATURAL: what LDE and order NN leave) or shift * w^bitrev(i) (BITREV: what
order NR leaves), w the root compute_ntt uses.  Buffers are numpy arrays or torch tensors, host or device; with device
buffers and a stream every call only enqueues -- except the first shift="coset" of a field, see coset_shift()."""
import numpy as np

from . import ffi, merkle, poly
from .poly import _ELEM_BYTES, _count

NATURAL, BITREV = 0, 1
MAX_LG, MAX_LG_ARITY = 32, 3
_BASE = {"bb31x4": "bb31"}                      # the library whose field holds the domain's points
_COSET = {}


def _fields(field):
    if field == "m31":
        raise ValueError("field 'm31' has no 2-adic domain: its FRI is the circle fold, which this library does not have "
                         "(fri.reduce is available)")
    if field not in _ELEM_BYTES:
        raise ValueError("unknown field %r" % (field,))
    return ffi.load(field), _BASE.get(field, field)


def _lg(n, what):
    if n == 0 or n & (n - 1):
        raise ValueError("%s must hold a power of two of field elements" % what)
    lg = n.bit_length() - 1
    if lg > MAX_LG:
        raise ValueError("%s holds more than 2^%d elements" % (what, MAX_LG))
    return lg


def _order(order):
    if order not in (NATURAL, BITREV):
        raise ValueError("order must be fri.NATURAL or fri.BITREV")
    return int(order)


def coset_shift(field="gl64", device_id=0):
    """The library's group generator, the shift of compute_ntt's Coset type and of LDE's output, as one element of the
    domain's field in wire form.  Taken from the transform itself, once per field: the Coset evaluations of c * X over two
    points start with c * g.  That FIRST use per field runs a transform and a division on host buffers: it synchronises and
    cannot be captured.  Call fri.coset_shift(field) once before capturing a graph or timing a stream in which fold, domain
    or deep_quotient take shift="coset"; every later use is a dictionary lookup."""
    base = _BASE.get(field, field)
    if base not in _COSET:
        from .ntt import compute_ntt, NTTInputOutputOrder, NTTDirection, NTTType
        eb = _ELEM_BYTES[base]
        c = np.zeros(eb, dtype=np.uint8); c[0] = 1                  # some non-zero element
        x = np.zeros(2 * eb, dtype=np.uint8); x[eb:] = c
        compute_ntt(device_id, x, NTTInputOutputOrder.NN, NTTDirection.Forward, NTTType.Coset, field=base)
        g = np.zeros(eb, dtype=np.uint8)
        poly.divide(g, x[:eb].copy(), c, field=base, device_id=device_id)
        _COSET[base] = g
    return _COSET[base]


def _shift(shift, field, base, device_id):
    """(address or None, keepalive) of the shift: None, "coset" or one element of the domain's field on the host"""
    if shift is None:
        return None, None
    if isinstance(shift, str):
        if shift != "coset":
            raise ValueError("shift must be None, 'coset' or one element of the domain's field")
        shift = coset_shift(field, device_id)
    if hasattr(shift, "data_ptr"):
        shift = shift.cpu().numpy()
    shift = np.ascontiguousarray(shift)
    if shift.nbytes != _ELEM_BYTES[base]:
        raise ValueError("shift must be one element of the domain's field (%s)" % base)
    return shift.ctypes.data, shift


def fold(out, evals, beta, lg_arity=1, shift=None, order=NATURAL, field="gl64", device_id=0, stream=None):
    """lg_arity (1 .. 3) FRI folds of the n evaluations in one launch: out holds the n / 2^lg_arity evaluations of the
    polynomial with coefficients c[2k] + beta c[2k+1] (then beta^2, beta^4) on the domain squared as often, in the same order.
    beta: one element, on the host or the device.  NATURAL: out may be evals itself (its first n / 2^lg_arity elements are
    overwritten)."""
    L, base = _fields(field)
    n = _count(evals, field)
    lg = _lg(n, "evals")
    if not 1 <= lg_arity <= MAX_LG_ARITY:
        raise ValueError("lg_arity must be 1 .. %d" % MAX_LG_ARITY)
    if lg < lg_arity:
        raise ValueError("fewer than 2^lg_arity evaluations")
    _order(order)
    po, _k1 = ffi.as_pointer(out); pi, _k2 = ffi.as_pointer(evals); pb, _k3 = ffi.as_pointer(beta)
    same = po == pi
    if _count(out, field) != (n if same else n >> lg_arity):
        raise ValueError("out must hold n / 2^lg_arity elements (or be evals itself)")
    if same and order != NATURAL:
        raise ValueError("only a NATURAL fold may run in place")
    if _count(beta, field) != 1:
        raise ValueError("beta must be one field element")
    ps, _k4 = _shift(shift, field, base, device_id)
    ffi.check(L, L.sppark_fri_fold(device_id, po, pi, lg, int(lg_arity), pb, ps, int(order), stream))
    return out


def domain(out, shift=None, order=NATURAL, z=None, field="gl64", device_id=0, stream=None):
    """out[i] = x_i - z for the len(out) points of the domain (z: None or one element, host or device)"""
    L, base = _fields(field)
    lg = _lg(_count(out, field), "out")
    _order(order)
    po, _k1 = ffi.as_pointer(out)
    pz = None
    if z is not None:
        if _count(z, field) != 1:
            raise ValueError("z must be one field element")
        pz, _k2 = ffi.as_pointer(z)
    ps, _k3 = _shift(shift, field, base, device_id)
    ffi.check(L, L.sppark_fri_domain(device_id, po, lg, ps, int(order), pz, stream))
    return out


def reduce(out, matrix, weights, sub=None, accumulate=False, layout="columns", base=False, field="gl64", device_id=0, stream=None):   # noqa: A001
    """out[i] = (out[i] if accumulate else 0) + sum_j weights[j] * matrix(j, i) - sub over the matrix of merkle.commit (same
    layouts and strides).  base=True (field "bb31x4" only): the matrix holds bb31 elements, weights, sub and out bb31x4."""
    L = ffi.load(field)
    if base and field != "bb31x4":
        raise ValueError("base=True needs an extension-field library (field='bb31x4')")
    addr, _keep, lg, width, cs, ls = merkle._geometry(matrix, layout, _BASE[field] if base else field)
    if _count(out, field) != 1 << lg:
        raise ValueError("out must hold one element per leaf")
    if _count(weights, field) != width:
        raise ValueError("weights must hold one element per column of the matrix")
    po, _k1 = ffi.as_pointer(out); pw, _k2 = ffi.as_pointer(weights)
    psub = None
    if sub is not None:
        if _count(sub, field) != 1:
            raise ValueError("sub must be one field element")
        psub, _k3 = ffi.as_pointer(sub)
    ffi.check(L, L.sppark_fri_reduce(device_id, po, addr, 1 if base else 0, lg, width, cs, ls, pw, psub, 1 if accumulate else 0, stream))
    return out


def deep_quotient(out, matrix, weights, value, z, lg_n=None, shift=None, order=NATURAL, layout="columns", base=False, field="gl64",
                  scratch=None, device_id=0, stream=None):
    """out[i] = (sum_j weights[j] * matrix(j, i) - value) / (x_i - z): reduce with sub=value, domain with z, poly.divide.
    lg_n: None or the log2 of the leaves, which the matrix must then have.  scratch: a buffer like out for the denominators;
    allocated per call where out lives when not given.  z must lie outside the domain."""
    if lg_n is not None and _count(out, field) != 1 << lg_n:
        raise ValueError("out must hold 2^lg_n elements")
    if scratch is None:
        if hasattr(out, "data_ptr"):
            import torch
            scratch = torch.empty_like(out)
        else:
            scratch = np.empty_like(out)
    elif _count(scratch, field) != _count(out, field):
        raise ValueError("scratch must hold as many elements as out")
    reduce(out, matrix, weights, sub=value, layout=layout, base=base, field=field, device_id=device_id, stream=stream)
    domain(scratch, shift=shift, order=order, z=z, field=field, device_id=device_id, stream=stream)
    poly.divide(out, out, scratch, field=field, device_id=device_id, stream=stream)
    return out
