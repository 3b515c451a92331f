"""Host model of the Merkle commitments (include/sppark_amd_merkle.h), built on hashlib alone.

A matrix is a list of leaves, each a bytes object (the concatenated wire bytes of its elements).  The tree is a list of
layers, layer 0 the leaf digests, layer lg_n the root; tree_bytes() lays them out as the entry point does: bottom-up, the
root the last 32 bytes."""
import hashlib

import numpy as np

HASHES = {"blake2s": hashlib.blake2s, "sha256": hashlib.sha256}
HASH_ID = {"blake2s": 0, "sha256": 1}
DIGEST = 32


def H(hash, data):                                                                      # noqa: A002
    return HASHES[hash](bytes(data)).digest()


def layers(leaves, hash):                                                               # noqa: A002
    """the whole tree of a list of 2^k leaves (bytes each): [layer 0, .., layer k], each a list of 32-byte digests"""
    n = len(leaves)
    assert n and n & (n - 1) == 0
    out = [[H(hash, x) for x in leaves]]
    while len(out[-1]) > 1:
        prev = out[-1]
        out.append([H(hash, prev[2 * i] + prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return out


def tree_bytes(lay):
    """the layers as the entry point stores them: a uint8 array of (2n - 1) * 32 bytes"""
    return np.frombuffer(b"".join(b"".join(layer) for layer in lay), dtype=np.uint8).copy()


def layer_offset(lg_n, l):
    return (2 << lg_n) - (2 << (lg_n - l))


def path(lay, index):
    """the siblings on the way up from leaf |index|: lg_n digests"""
    return [lay[l][(index >> l) ^ 1] for l in range(len(lay) - 1)]


def climb(hash, digest, index, siblings):                                               # noqa: A002
    """the digests above |digest| at position |index| of layer 0: [layer 1 .. layer len(siblings)]"""
    out = []
    for l, sib in enumerate(siblings):
        digest = H(hash, sib + digest) if (index >> l) & 1 else H(hash, digest + sib)
        out.append(digest)
    return out


def zero_digests(hash, leaf_len, lg_n):                                                 # noqa: A002
    """Z_0 = H(zero leaf), Z_l = H(Z_{l-1} || Z_{l-1}): layer l of the tree over an all-zero matrix is Z_l everywhere"""
    z = [H(hash, bytes(leaf_len))]
    for _ in range(lg_n):
        z.append(H(hash, z[-1] + z[-1]))
    return z


def planted(hash, leaf_len, lg_n, plants):                                              # noqa: A002
    """The tree over a matrix that is zero except for the leaves in |plants| ({index: leaf bytes}), sparsely: per layer a dict
    {position: digest} of the digests that differ from Z_l (every other digest of the layer is Z_l), and the root.
    O(len(plants) * lg_n) hashes."""
    z = zero_digests(hash, leaf_len, lg_n)
    cur = {i: H(hash, leaf) for i, leaf in plants.items()}
    sparse = [dict(cur)]
    for l in range(lg_n):
        nxt = {}
        for i in cur:
            p = i >> 1
            if p not in nxt:
                nxt[p] = H(hash, cur.get(2 * p, z[l]) + cur.get(2 * p + 1, z[l]))
        cur = nxt
        sparse.append(dict(cur))
    root = cur.get(0, z[lg_n])
    return sparse, z, root


def periodic(hash, pool_leaves, lg_n):                                                  # noqa: A002
    """The tree over n = 2^lg_n leaves that repeat |pool_leaves| (2^m of them) with period 2^m: layer l <= m is the pool's
    layer l repeated (period 2^(m-l)); above layer m every digest of a layer is the same, x <- H(x || x).  Returns
    (the pool's layers, [the one digest of layer m, m + 1, .., lg_n])."""
    lay = layers(pool_leaves, hash)
    m = len(lay) - 1
    assert m <= lg_n
    x = lay[m][0]
    above = [x]
    for _ in range(lg_n - m):
        x = H(hash, x + x)
        above.append(x)
    return lay, above


def verify(hash, root, index, leaf, siblings):                                          # noqa: A002
    up = climb(hash, H(hash, leaf), index, siblings)
    return (up[-1] if up else H(hash, leaf)) == bytes(root)


def leaves_of(matrix_bytes, n, width, elem_bytes, col_stride, leaf_stride):
    """the n leaves of a byte buffer that holds a matrix with the given strides (in elements)"""
    buf = bytes(matrix_bytes)
    out = []
    for i in range(n):
        parts = []
        for j in range(width):
            at = (j * col_stride + i * leaf_stride) * elem_bytes
            parts.append(buf[at:at + elem_bytes])
        out.append(b"".join(parts))
    return out
