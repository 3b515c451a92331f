"""Poseidon2 over BabyBear and Goldilocks: host API over sppark_poseidon2_permute / sppark_poseidon2_commit
(include/sppark_amd_poseidon2.h, where the permutation and the sponge are defined; the reference's snapshot has no counterpart).
States, matrices and constants hold field elements in the wire format of the chosen library (Montgomery words, R = 2^32, for
bb31 / bb31_canonical; canonical integers for gl64 / gl64_plonky2), as numpy arrays or torch tensors, host or device.  The
tree is the tree of sppark_amd.merkle: merkle.open, merkle.gather, merkle.layer and merkle.tree_bytes are used on it as they
are.  The parameters are the caller's (Params); test_params() draws this project's own constants for tests and benchmarks.
verify() is the verifier's side in Python integers and needs no library."""
import hashlib

import numpy as np

from . import ffi, merkle
from .poly import _ELEM_BYTES

FIELDS = ffi.NTT_FIELDS
MODULUS = {"bb31": 0x78000001, "bb31_canonical": 0x78000001, "gl64": 0xffffffff00000001, "gl64_plonky2": 0xffffffff00000001}
WIDTH = {"bb31": 16, "bb31_canonical": 16, "gl64": 8, "gl64_plonky2": 8}
USUAL_ROUNDS = {16: (8, 13), 8: (8, 22)}                 # (RF, RP) by width
MAX_ROUNDS_F, MAX_ROUNDS_P = 16, 64
_MONT_BITS = {"bb31": 32, "bb31_canonical": 32, "gl64": 0, "gl64_plonky2": 0}


def _field(field):
    if field not in FIELDS:
        raise ValueError("field must be one of %s" % (FIELDS,))
    return field


def _dtype(field):
    return np.uint32 if _ELEM_BYTES[field] == 4 else np.uint64


def to_wire(field, values):
    """canonical integers -> the library's wire words (a list of ints)"""
    p, k = MODULUS[_field(field)], _MONT_BITS[field]
    return [(int(v) << k) % p for v in values]


def from_wire(field, words):
    """wire words -> canonical integers (a list of ints)"""
    p, k = MODULUS[_field(field)], _MONT_BITS[field]
    rinv = pow(1 << k, -1, p)
    return [int(w) * rinv % p for w in words]


class Params:
    """One parameter set: rounds_f (even, 2 .. 16), rounds_p (0 .. 64) and rounds_f * T + rounds_p + T constants in wire format --
    the external constants round by round, the internal constants, the diagonal.  Keeps a host copy and, once asked for, one
    copy per device."""

    def __init__(self, field, rounds_f, rounds_p, consts):
        self.field = _field(field)
        self.width = WIDTH[field]
        rounds_f, rounds_p = int(rounds_f), int(rounds_p)
        if rounds_f < 2 or rounds_f > MAX_ROUNDS_F or rounds_f % 2:
            raise ValueError("rounds_f must be even, 2 .. %d" % MAX_ROUNDS_F)
        if rounds_p < 0 or rounds_p > MAX_ROUNDS_P:
            raise ValueError("rounds_p must be 0 .. %d" % MAX_ROUNDS_P)
        self.rounds_f, self.rounds_p = rounds_f, rounds_p
        if hasattr(consts, "data_ptr"):
            consts = consts.cpu().numpy()
        words = [int(w) for w in np.asarray(consts).reshape(-1).tolist()]
        want = rounds_f * self.width + rounds_p + self.width
        if len(words) != want:
            raise ValueError("consts must hold rounds_f * T + rounds_p + T = %d elements" % want)
        if any(w < 0 or w >= MODULUS[field] for w in words):
            raise ValueError("a constant is not a canonical word of the field")
        self.consts = np.array(words, dtype=_dtype(field))
        self.consts.setflags(write=False)
        self._device = {}
        self._ints = None

    def device(self, device_id=0):
        """the constants on the device, copied there on first use"""
        if device_id not in self._device:
            import torch
            signed = np.int32 if self.consts.dtype == np.uint32 else np.int64
            self._device[device_id] = torch.from_numpy(self.consts.view(signed).copy()).to("cuda:%d" % device_id)
        return self._device[device_id]

    def ints(self):
        """(ce, ci, d) as canonical Python integers: ce[r][i], ci[r], d[i]"""
        if self._ints is None:
            t, rf, rp = self.width, self.rounds_f, self.rounds_p
            c = from_wire(self.field, self.consts.tolist())
            self._ints = ([c[r * t:(r + 1) * t] for r in range(rf)], c[rf * t:rf * t + rp], c[rf * t + rp:])
        return self._ints


def test_params(field, rounds_f=8, rounds_p=None, seed=0):
    """This project's OWN constants, for tests and benchmarks -- nobody's standard, and of no claimed security: field elements
    drawn from a SHAKE-256 stream by rejection (little-endian words of the element's size, BabyBear's top bit cleared first;
    a word >= p is dropped), the diagonal's entries non-zero (a zero is dropped as well).  rounds_p defaults to the usual
    number for the width (13 / 22)."""
    field = _field(field)
    t, p, eb = WIDTH[field], MODULUS[field], _ELEM_BYTES[field]
    if rounds_p is None:
        rounds_p = USUAL_ROUNDS[t][1]
    want = rounds_f * t + rounds_p + t
    if want <= 0:
        raise ValueError("no constants to draw")
    tag = ("sppark_amd.poseidon2.test_params|%d|%d|%d|%d|%d" % (p, t, rounds_f, rounds_p, seed)).encode()
    stream = hashlib.shake_256(tag).digest(4 * (want + 64) * eb)
    vals, at = [], 0
    while len(vals) < want:
        v = int.from_bytes(stream[at:at + eb], "little")
        at += eb
        if eb == 4:
            v &= 0x7fffffff
        if v >= p or (v == 0 and len(vals) >= want - t):
            continue
        vals.append(v)
    return Params(field, rounds_f, rounds_p, to_wire(field, vals))
test_params.__test__ = False                                                             # (not a test, whatever a collector thinks)


def _is_device(x):
    return hasattr(x, "data_ptr") and x.device.type != "cpu"


def _consts_for(params, device_id, *buffers):
    """(address, keepalive): the device copy when every buffer of the call is on the device, else the host copy"""
    if buffers and all(_is_device(b) for b in buffers):
        d = params.device(device_id)
        return d.data_ptr(), d
    return params.consts.ctypes.data, params.consts


def _states(x, params, what):
    if not hasattr(x, "shape") or len(x.shape) != 2 or int(x.shape[1]) != params.width:
        raise ValueError("%s must have shape (count, %d)" % (what, params.width))
    item = x.element_size() if hasattr(x, "data_ptr") else x.itemsize
    if item != _ELEM_BYTES[params.field]:
        raise ValueError("%s must hold one field element per item" % what)


def permute(states, params, out=None, device_id=0, stream=None):
    """out[k] = the permutation of states[k]; states: (count, T) in wire format.  out is allocated where states lives when not
    given; out may be states itself."""
    _states(states, params, "states")
    if out is None:
        out = states.new_empty(tuple(states.shape)) if hasattr(states, "new_empty") else np.empty_like(states)
    else:
        _states(out, params, "out")
        if tuple(out.shape) != tuple(states.shape):
            raise ValueError("out must have the shape of states")
    L = ffi.load(params.field)
    pi, _k1 = ffi.as_pointer(states)
    po, _k2 = ffi.as_pointer(out)
    pc, _k3 = _consts_for(params, device_id, states, out)
    if int(states.shape[0]):
        ffi.check(L, L.sppark_poseidon2_permute(device_id, po, pi, int(states.shape[0]), pc, params.rounds_f, params.rounds_p, stream))
    return out


def commit(matrix, params, layout="columns", tree=None, device_id=0, stream=None):
    """(tree, root) of the matrix, as merkle.commit returns them: tree is merkle.tree_bytes(lg_n) bytes of uint8, allocated
    where the matrix lives when not given; root is 32 bytes as a numpy array -- or, when the call only enqueues (matrix and
    tree on the device and a stream), a view of the device tree's last 32 bytes, valid once the stream has got there."""
    if not isinstance(params, Params):
        raise TypeError("params must be a poseidon2.Params")
    field = params.field
    L = ffi.load(field)
    addr, _keep, lg, width, cs, ls = merkle._geometry(matrix, layout, field)
    nbytes = merkle.tree_bytes(lg)
    if tree is None:
        tree = merkle._like(matrix, nbytes)
    elif int(np.prod(tuple(tree.shape))) != nbytes or tree.dtype not in merkle._BYTE_DTYPES():
        raise ValueError("tree must hold tree_bytes(lg_n) = %d bytes as uint8" % nbytes)
    pt, _k2 = ffi.as_pointer(tree)
    pc, _k3 = _consts_for(params, device_id, matrix, tree)
    if stream is not None and _is_device(matrix) and _is_device(tree):
        ffi.check(L, L.sppark_poseidon2_commit(device_id, pt, None, addr, lg, width, cs, ls, pc, params.rounds_f, params.rounds_p, stream))
        return tree, tree.reshape(-1)[nbytes - merkle.DIGEST_BYTES:]
    root = np.zeros(merkle.DIGEST_BYTES, dtype=np.uint8)
    ffi.check(L, L.sppark_poseidon2_commit(device_id, pt, root.ctypes.data, addr, lg, width, cs, ls, pc, params.rounds_f, params.rounds_p,
                                           stream))
    return tree, root


# ---- the verifier's side: Python integers -----------------------------------------------------------------------------------
def _m4(a, b, c, d, p):
    return ((2 * a + 3 * b + c + d) % p, (a + 2 * b + 3 * c + d) % p, (a + b + 2 * c + 3 * d) % p, (3 * a + b + c + 2 * d) % p)


def _external(x, p):
    z = []
    for b in range(0, len(x), 4):
        z += _m4(x[b], x[b + 1], x[b + 2], x[b + 3], p)
    s = [sum(z[k::4]) % p for k in range(4)]
    return [(z[i] + s[i & 3]) % p for i in range(len(z))]


def permute_ints(x, params):
    """the permutation of one state of canonical integers"""
    p = MODULUS[params.field]
    ce, ci, d = params.ints()
    half = params.rounds_f // 2
    x = _external([int(v) % p for v in x], p)
    for r in list(range(half)) + [None] + list(range(half, params.rounds_f)):
        if r is None:
            for k in ci:
                x[0] = pow(x[0] + k, 7, p)
                s = sum(x) % p
                x = [(d[i] * x[i] + s) % p for i in range(len(x))]
        else:
            x = _external([pow(x[i] + ce[r][i], 7, p) for i in range(len(x))], p)
    return x


def _digest_ints(data, params):
    words = np.frombuffer(merkle._bytes(data), dtype=_dtype(params.field))
    if len(words) != params.width // 2:
        raise ValueError("a digest is 32 bytes")
    return from_wire(params.field, words.tolist())


def verify(root, index, leaf_elements, path, params):
    """Does |path| (lg_n digests of 32 bytes, leaf level first, as merkle.open returns them) take the leaf with the elements
    |leaf_elements| (wire words, or the bytes merkle.gather returns) at position |index| to |root|?"""
    t = params.width
    rate = t // 2
    path = [merkle._bytes(q) for q in path]
    index = int(index)
    if index < 0 or index >> len(path) or any(len(q) != merkle.DIGEST_BYTES for q in path):
        return False
    leaf = merkle._bytes(leaf_elements)
    if len(leaf) == 0 or len(leaf) % _ELEM_BYTES[params.field]:
        return False
    elems = from_wire(params.field, np.frombuffer(leaf, dtype=_dtype(params.field)).tolist())
    x = [0] * t
    for at in range(0, len(elems), rate):
        chunk = elems[at:at + rate]
        x[:len(chunk)] = chunk
        x = permute_ints(x, params)
    x = x[:rate]
    for l, sib in enumerate(path):
        sib = _digest_ints(sib, params)
        x = permute_ints(sib + x if (index >> l) & 1 else x + sib, params)[:rate]
    want = np.array(to_wire(params.field, x), dtype=_dtype(params.field)).tobytes()
    return want == merkle._bytes(root)
