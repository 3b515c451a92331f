"""Polynomial primitives: host API over sppark_prefix_op / sppark_poly_evaluate /
sppark_div_by_x_minus_z (the reference offers them as C++ templates only:
polynomial/prefix_op.cuh:324-396, evaluate.cuh:307-412, div_by_x_minus_z.cuh:447-486), and the field-vector
inverse and quotient over sppark_field_inverse / sppark_field_divide (ff/batch_inversion.hpp, a host template there);
field-vector arithmetic (vec_add, vec_sub, vec_mul, vec_scale, vec_mul_sub), the polynomial product and the vanishing
quotient over include/sppark_amd_arith.h (no counterpart in the reference).
Buffers are numpy arrays or torch tensors (host or device) of field elements in the wire
format of the chosen library (gl64: canonical u64; bb31: Montgomery u32; bls12_381 / bn254:
the curve's scalar field, 4 x u64 Montgomery)."""
from . import ffi

_ELEM_BYTES = {"gl64": 8, "bb31": 4, "bls12_381": 32, "bn254": 32, "bls12_377": 32, "pallas": 32, "vesta": 32, "m31": 4, "bb31x4": 16, "gl64_plonky2": 8, "bb31_canonical": 4}
ADD, MULTIPLY = 0, 1


def _count(buf, field):
    nbytes = int(buf.nbytes) if hasattr(buf, "nbytes") else int(buf.numel() * buf.element_size())
    if nbytes % _ELEM_BYTES[field]:
        raise ValueError("buffer is not a whole number of field elements")
    return nbytes // _ELEM_BYTES[field]


def prefix_op(out, inp, op, field="gl64", device_id=0, stream=None):
    """out[i] = inp[0] (op) ... (op) inp[i]; op = ADD or MULTIPLY; out may be inp itself."""
    L = ffi.load(field)
    n = _count(inp, field)
    if _count(out, field) != n:
        raise ValueError("length mismatch")
    po, _k1 = ffi.as_pointer(out); pi, _k2 = ffi.as_pointer(inp)
    ffi.check(L, L.sppark_prefix_op(device_id, po, pi, n, int(op), stream))
    return out


def evaluate(ret, xs, coeffs, field="gl64", device_id=0, stream=None):
    """ret[j] = sum_i coeffs[i] * xs[j]^i"""
    L = ffi.load(field)
    n = _count(xs, field)
    if _count(ret, field) != n:
        raise ValueError("length mismatch")
    pr, _k1 = ffi.as_pointer(ret); px, _k2 = ffi.as_pointer(xs); pc, _k3 = ffi.as_pointer(coeffs)
    ffi.check(L, L.sppark_poly_evaluate(device_id, pr, px, n, pc, _count(coeffs, field), stream))
    return ret


def div_by_x_minus_z(inout, z, rotate=False, field="gl64", device_id=0, stream=None):
    """In-place synthetic division of sum_i inout[i] x^i by (x - z).  rotate=False: remainder at
    index 0, quotient after it; rotate=True: quotient first, remainder last."""
    L = ffi.load(field)
    if _count(z, field) != 1:
        raise ValueError("z must be one field element")
    p, _k1 = ffi.as_pointer(inout); pz, _k2 = ffi.as_pointer(z)
    ffi.check(L, L.sppark_div_by_x_minus_z(device_id, p, _count(inout, field), pz, int(rotate), stream))
    return inout


def inverse(out, inp, field="gl64", device_id=0, stream=None):
    """out[i] = 1 / inp[i], and 0 where inp[i] == 0 (the reference's ff/batch_inversion.hpp, on the device:
    one field inversion per call); out may be inp itself.  Elements must be canonical."""
    L = ffi.load(field)
    n = _count(inp, field)
    if _count(out, field) != n:
        raise ValueError("length mismatch")
    po, _k1 = ffi.as_pointer(out); pi, _k2 = ffi.as_pointer(inp)
    ffi.check(L, L.sppark_field_inverse(device_id, po, pi, n, stream))
    return out


def divide(out, num, den, field="gl64", device_id=0, stream=None):
    """out[i] = num[i] / den[i], and 0 where den[i] == 0; out may be num or den."""
    L = ffi.load(field)
    n = _count(den, field)
    if _count(out, field) != n or _count(num, field) != n:
        raise ValueError("length mismatch")
    po, _k1 = ffi.as_pointer(out); pn, _k2 = ffi.as_pointer(num); pd, _k3 = ffi.as_pointer(den)
    ffi.check(L, L.sppark_field_divide(device_id, po, pn, pd, n, stream))
    return out


# ---- field-vector arithmetic, polynomial product, vanishing quotient (include/sppark_amd_arith.h) ----
def _same_length(field, *bufs):
    n = _count(bufs[0], field)
    for b in bufs[1:]:
        if _count(b, field) != n:
            raise ValueError("length mismatch")
    return n


def _vec3(name, out, a, b, field, device_id, stream):
    L = ffi.load(field)
    n = _same_length(field, out, a, b)
    po, _k1 = ffi.as_pointer(out); pa, _k2 = ffi.as_pointer(a); pb, _k3 = ffi.as_pointer(b)
    ffi.check(L, getattr(L, name)(device_id, po, pa, pb, n, stream))
    return out


def vec_add(out, a, b, field="gl64", device_id=0, stream=None):
    """out[i] = a[i] + b[i].  Here and below: out may be any of the inputs, inputs may be each other; with device
    buffers and a stream the call only enqueues."""
    return _vec3("sppark_field_add", out, a, b, field, device_id, stream)


def vec_sub(out, a, b, field="gl64", device_id=0, stream=None):
    """out[i] = a[i] - b[i]"""
    return _vec3("sppark_field_sub", out, a, b, field, device_id, stream)


def vec_mul(out, a, b, field="gl64", device_id=0, stream=None):
    """out[i] = a[i] * b[i]"""
    return _vec3("sppark_field_mul", out, a, b, field, device_id, stream)


def vec_scale(out, a, k, field="gl64", device_id=0, stream=None):
    """out[i] = a[i] * k; k: one element, on the host or on the device"""
    L = ffi.load(field)
    n = _same_length(field, out, a)
    if _count(k, field) != 1:
        raise ValueError("k must be one field element")
    po, _k1 = ffi.as_pointer(out); pa, _k2 = ffi.as_pointer(a); pk, _k3 = ffi.as_pointer(k)
    ffi.check(L, L.sppark_field_scale(device_id, po, pa, pk, n, stream))
    return out


def vec_mul_sub(out, a, b, c, k=None, field="gl64", device_id=0, stream=None):
    """out[i] = (a[i] * b[i] - c[i]) * k; k=None: one, and no product is spent on it"""
    L = ffi.load(field)
    n = _same_length(field, out, a, b, c)
    pk, _k0 = None, None
    if k is not None:
        if _count(k, field) != 1:
            raise ValueError("k must be one field element")
        pk, _k0 = ffi.as_pointer(k)
    po, _k1 = ffi.as_pointer(out); pa, _k2 = ffi.as_pointer(a); pb, _k3 = ffi.as_pointer(b); pc, _k4 = ffi.as_pointer(c)
    ffi.check(L, L.sppark_field_mul_sub(device_id, po, pa, pb, pc, pk, n, stream))
    return out


def product(out, a, b, field="gl64", device_id=0, stream=None):
    """out[0 .. la+lb-1) = coefficients of (sum a_i x^i)(sum b_i x^i), lowest first; the rest of out is left alone.
    out must not overlap a or b; a may be b (a square).  Returns when the result is in place."""
    L = ffi.load(field)
    la, lb, lo = _count(a, field), _count(b, field), _count(out, field)
    if la and lb and lo < la + lb - 1:
        raise ValueError("out is shorter than la + lb - 1 elements")
    po, _k1 = ffi.as_pointer(out); pa, _k2 = ffi.as_pointer(a); pb, _k3 = ffi.as_pointer(b)
    ffi.check(L, L.sppark_poly_product(device_id, po, pa, la, pb, lb, stream))
    return out


def vanishing_quotient(h, a, b, c, field="bls12_381", device_id=0, stream=None):
    """h = the n coefficients of (A*B - C) / (x^n - 1) from the n = 2^lg evaluations a, b, c over {w^i} (Groth16's h when
    c = a .* b); h may be one of the inputs.  Returns when the result is in place."""
    L = ffi.load(field)
    n = _same_length(field, h, a, b, c)
    if n == 0 or n & (n - 1):
        raise ValueError("the length must be a power of two")
    ph, _k1 = ffi.as_pointer(h); pa, _k2 = ffi.as_pointer(a); pb, _k3 = ffi.as_pointer(b); pc, _k4 = ffi.as_pointer(c)
    ffi.check(L, L.sppark_poly_vanishing_quotient(device_id, ph, pa, pb, pc, n.bit_length() - 1, stream))
    return h
