"""Merkle commitments: host API over sppark_merkle_commit / sppark_merkle_open / sppark_merkle_gather
(include/sppark_amd_merkle.h; the reference's snapshot has no counterpart).
A matrix is a 2-D numpy array or torch tensor, host or device, whose words are field elements in the wire format of the
chosen library (see sppark_amd.poly).  layout "columns": matrix[j] is polynomial j and leaf i is the column of the i-th
elements -- what NTT_batch, LDE_batch and circle.lde leave; layout "rows": matrix[i] is leaf i.  Only the last axis may be
cut short by a stride (a slice of a wider array); its words are contiguous.  Digests are the bytes of hashlib.blake2s /
hashlib.sha256; verify() below is the verifier's side and needs no library."""
import hashlib

import numpy as np

from . import ffi
from .poly import _ELEM_BYTES

BLAKE2S, SHA256 = 0, 1
_HASHES = {"blake2s": BLAKE2S, "sha256": SHA256, BLAKE2S: BLAKE2S, SHA256: SHA256}
_HASHLIB = {BLAKE2S: hashlib.blake2s, SHA256: hashlib.sha256}
MAX_LG = 28
DIGEST_BYTES = 32


def _hash(hash):                                                                       # noqa: A002 (the header's name)
    if hash not in _HASHES:
        raise ValueError("hash must be 'blake2s' or 'sha256'")
    return _HASHES[hash]


def tree_bytes(lg_n):
    """bytes of the tree over 2^lg_n leaves: 2^(lg_n+1) - 1 digests"""
    if not 0 <= lg_n <= MAX_LG:
        raise ValueError("lg_n must be 0 .. %d" % MAX_LG)
    return ((2 << lg_n) - 1) * DIGEST_BYTES


def layer_offset(lg_n, l):
    """digest index of the first digest of layer l (0 = leaves .. lg_n = root)"""
    if not 0 <= l <= lg_n:
        raise ValueError("layer must be 0 .. lg_n")
    return (2 << lg_n) - (2 << (lg_n - l))


def layer(tree, lg_n, l):
    """layer l of a tree as a view of shape (2^(lg_n-l), 32); tree: a flat uint8 array or tensor of tree_bytes(lg_n) bytes"""
    if int(np.prod(tuple(tree.shape))) != tree_bytes(lg_n) or tree.dtype not in _BYTE_DTYPES():
        raise ValueError("tree must hold tree_bytes(lg_n) bytes as uint8")
    at = layer_offset(lg_n, l) * DIGEST_BYTES
    return tree.reshape(-1)[at:at + (DIGEST_BYTES << (lg_n - l))].reshape(-1, DIGEST_BYTES)


def _BYTE_DTYPES():
    try:
        import torch
        return (np.dtype(np.uint8), torch.uint8)
    except ImportError:
        return (np.dtype(np.uint8),)


def _geometry(matrix, layout, field):
    """(address, keepalive, lg_n, width, col_stride, leaf_stride) of a 2-D matrix, strides in elements"""
    if layout not in ("columns", "rows"):
        raise ValueError("layout must be 'columns' or 'rows'")
    if not hasattr(matrix, "shape") or len(matrix.shape) != 2:
        raise ValueError("matrix must be 2-D: (polynomials, words) for 'columns', (leaves, words) for 'rows'")
    eb = _ELEM_BYTES[field]
    if hasattr(matrix, "data_ptr"):                                                     # torch: strides in items
        item = matrix.element_size()
        strides = tuple(int(s) * item for s in matrix.stride())
        addr = matrix.data_ptr()
    elif hasattr(matrix, "ctypes"):
        item = matrix.itemsize
        strides = tuple(int(s) for s in matrix.strides)
        addr = matrix.ctypes.data
    else:
        raise TypeError("unsupported buffer type %r" % type(matrix))
    outer, inner = int(matrix.shape[0]), int(matrix.shape[1])
    if outer == 0 or inner == 0:
        raise ValueError("matrix is empty")
    if eb % item and item % eb:
        raise ValueError("the array's items neither divide nor are divided by a field element")
    if (inner * item) % eb:
        raise ValueError("a line of the matrix is not a whole number of field elements")
    if strides[1] != item or strides[0] <= 0 or strides[0] % eb or strides[0] < inner * item:
        raise ValueError("the words of a line must be contiguous and lines a whole, positive number of elements apart")
    count, pitch = inner * item // eb, strides[0] // eb
    n, width = (count, outer) if layout == "columns" else (outer, count)
    if n & (n - 1):
        raise ValueError("the matrix must have a power of two of leaves")
    lg = n.bit_length() - 1
    if lg > MAX_LG:
        raise ValueError("more than 2^%d leaves" % MAX_LG)
    if width * eb >= 1 << 32:
        raise ValueError("a leaf of 4 GiB or more")
    cs, ls = (pitch, 1) if layout == "columns" else (1, pitch)
    return addr, matrix, lg, width, cs, ls


def _like(matrix, nbytes):
    """nbytes of uint8 where |matrix| lives"""
    if hasattr(matrix, "data_ptr"):
        import torch
        return torch.empty(nbytes, dtype=torch.uint8, device=matrix.device)
    return np.empty(nbytes, dtype=np.uint8)


def _is_device(x):
    return hasattr(x, "data_ptr") and x.device.type != "cpu"


def _indices(indices, n):
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(-1))
    if len(idx) and int(idx.max()) >= n:
        raise ValueError("an index is not below the number of leaves")
    return idx


def commit(matrix, hash="blake2s", layout="columns", field="gl64", tree=None, device_id=0, stream=None):    # noqa: A002
    """(tree, root) of the matrix.  tree: tree_bytes(lg_n) bytes of uint8, allocated where the matrix lives when not given.
    root: 32 bytes as a numpy array -- or, when the call only enqueues (matrix and tree on the device and a stream), a view of
    the device tree's last 32 bytes, valid once the stream has got there."""
    L = ffi.load(field)
    h = _hash(hash)
    addr, _keep, lg, width, cs, ls = _geometry(matrix, layout, field)
    nbytes = tree_bytes(lg)
    if tree is None:
        tree = _like(matrix, nbytes)
    elif int(np.prod(tuple(tree.shape))) != nbytes or tree.dtype not in _BYTE_DTYPES():
        raise ValueError("tree must hold tree_bytes(lg_n) = %d bytes as uint8" % nbytes)
    pt, _k2 = ffi.as_pointer(tree)
    if stream is not None and _is_device(matrix) and _is_device(tree):
        ffi.check(L, L.sppark_merkle_commit(device_id, pt, None, addr, lg, width, cs, ls, h, stream))
        return tree, tree.reshape(-1)[nbytes - DIGEST_BYTES:]
    root = np.zeros(DIGEST_BYTES, dtype=np.uint8)
    ffi.check(L, L.sppark_merkle_commit(device_id, pt, root.ctypes.data, addr, lg, width, cs, ls, h, stream))
    return tree, root


def open(tree, lg_n, indices, field="gl64", out=None, device_id=0, stream=None):           # noqa: A001 (the header's name)
    """paths of shape (len(indices), lg_n, 32): paths[q][l] is the sibling at layer l on the way up from leaf indices[q].
    Allocated where the tree lives when |out| is not given."""
    L = ffi.load(field)
    if int(np.prod(tuple(tree.shape))) != tree_bytes(lg_n) or tree.dtype not in _BYTE_DTYPES():
        raise ValueError("tree must hold tree_bytes(lg_n) bytes as uint8")
    idx = _indices(indices, 1 << lg_n)
    nbytes = len(idx) * lg_n * DIGEST_BYTES
    if out is None:
        out = _like(tree, nbytes)
    elif int(np.prod(tuple(out.shape))) != nbytes or out.dtype not in _BYTE_DTYPES():
        raise ValueError("out must hold len(indices) * lg_n * 32 bytes as uint8")
    if nbytes:
        po, _k1 = ffi.as_pointer(out); pt, _k2 = ffi.as_pointer(tree)
        ffi.check(L, L.sppark_merkle_open(device_id, po, pt, lg_n, idx.ctypes.data, len(idx), stream))
    return out.reshape(len(idx), lg_n, DIGEST_BYTES)


def gather(matrix, indices, layout="columns", field="gl64", out=None, device_id=0, stream=None):
    """rows of shape (len(indices), width * element bytes) as uint8: rows[q] is leaf indices[q], the bytes its digest hashes.
    Allocated where the matrix lives when |out| is not given."""
    L = ffi.load(field)
    addr, _keep, lg, width, cs, ls = _geometry(matrix, layout, field)
    idx = _indices(indices, 1 << lg)
    nbytes = len(idx) * width * _ELEM_BYTES[field]
    if out is None:
        out = _like(matrix, nbytes)
    elif int(np.prod(tuple(out.shape))) != nbytes or out.dtype not in _BYTE_DTYPES():
        raise ValueError("out must hold len(indices) * width elements as uint8")
    if nbytes:
        po, _k1 = ffi.as_pointer(out)
        ffi.check(L, L.sppark_merkle_gather(device_id, po, addr, lg, width, cs, ls, idx.ctypes.data, len(idx), stream))
    return out.reshape(len(idx), width * _ELEM_BYTES[field])


def _bytes(x):
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def verify(root, index, leaf_bytes, path, hash="blake2s"):                                # noqa: A002
    """The verifier's side, pure hashlib: does |path| (lg_n digests, leaf level first) take the leaf with the bytes
    |leaf_bytes| at position |index| to |root|?"""
    H = _HASHLIB[_hash(hash)]
    path = [_bytes(p) for p in path]
    index = int(index)
    if index < 0 or index >> len(path) or any(len(p) != DIGEST_BYTES for p in path):
        return False
    x = H(_bytes(leaf_bytes)).digest()
    for l, sib in enumerate(path):
        x = H(sib + x).digest() if (index >> l) & 1 else H(x + sib).digest()
    return x == _bytes(root)
