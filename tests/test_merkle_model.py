"""CPU: the host model of the Merkle commitments (tests/merkle_model.py) against the standards' vectors, against trees written
out longhand, and its two shortcuts (zero subtrees with planted leaves, periodic matrices) against the dense tree."""
import hashlib
import os
import sys

import numpy as np
import pytest

import merkle_model as M

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HASHES = ("blake2s", "sha256")


def test_standard_vectors():
    # RFC 7693 appendix B; FIPS 180-4 / NIST example "abc"
    assert M.H("blake2s", b"abc").hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    assert M.H("sha256", b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


@pytest.mark.parametrize("hash", HASHES)
def test_small_trees_longhand(hash):                                                    # noqa: A002
    h = lambda b: getattr(hashlib, hash)(b).digest()                                    # noqa: E731
    a, b, c, d = b"\x01\x00\x00\x00", b"\x02\x00\x00\x00", b"\x03\x00\x00\x00" * 3, b"\x04" * 4
    assert M.layers([a], hash) == [[h(a)]]
    assert M.layers([a, b], hash) == [[h(a), h(b)], [h(h(a) + h(b))]]
    l0 = [h(a), h(b), h(c), h(d)]
    l1 = [h(l0[0] + l0[1]), h(l0[2] + l0[3])]
    assert M.layers([a, b, c, d], hash) == [l0, l1, [h(l1[0] + l1[1])]]
    t = M.tree_bytes(M.layers([a, b, c, d], hash))
    assert len(t) == 7 * 32 and bytes(t[-32:]) == h(l1[0] + l1[1]) and bytes(t[:32]) == h(a)
    assert bytes(t[M.layer_offset(2, 1) * 32:][:32]) == l1[0] and M.layer_offset(2, 2) == 6 and M.layer_offset(0, 0) == 0


@pytest.mark.parametrize("hash", HASHES)
def test_verify_every_path_and_a_flipped_bit(hash):                                     # noqa: A002
    from sppark_amd import merkle
    rng = np.random.default_rng(5)
    leaves = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in range(32)]
    lay = M.layers(leaves, hash)
    root = lay[-1][0]
    for i in range(32):
        p = M.path(lay, i)
        assert len(p) == 5
        assert M.verify(hash, root, i, leaves[i], p)
        assert merkle.verify(np.frombuffer(root, dtype=np.uint8), i, np.frombuffer(leaves[i], dtype=np.uint8), p, hash)
        assert not merkle.verify(root, i ^ 1, leaves[i], p, hash)
        bad_leaf = bytes([leaves[i][0] ^ 1]) + leaves[i][1:]
        assert not merkle.verify(root, i, bad_leaf, p, hash) and not M.verify(hash, root, i, bad_leaf, p)
        for l in range(5):
            q = list(p)
            q[l] = q[l][:7] + bytes([q[l][7] ^ 0x10]) + q[l][8:]
            assert not merkle.verify(root, i, leaves[i], q, hash) and not M.verify(hash, root, i, leaves[i], q)
        assert not merkle.verify(root, i, leaves[i], p[:-1], hash)
        assert not merkle.verify(root, i + 32, leaves[i], p, hash)
    bad_root = root[:31] + bytes([root[31] ^ 0x80])
    assert not merkle.verify(bad_root, 0, leaves[0], M.path(lay, 0), hash)
    assert merkle.verify(M.H(hash, b"x" * 8), 0, b"x" * 8, [], hash)                       # lg_n == 0: the leaf digest is the root


@pytest.mark.parametrize("hash", HASHES)
def test_planted_shortcut_equals_the_dense_tree(hash):                                  # noqa: A002
    lg, leaf_len = 6, 20
    plants = {0: b"\x01" * 20, 5: b"\x02" * 20, 63: b"\x07" + bytes(19), 32: bytes(19) + b"\x09"}
    leaves = [plants.get(i, bytes(leaf_len)) for i in range(1 << lg)]
    lay = M.layers(leaves, hash)
    sparse, z, root = M.planted(hash, leaf_len, lg, plants)
    assert root == lay[-1][0]
    for l in range(lg + 1):
        differ = {i: dg for i, dg in enumerate(lay[l]) if dg != z[l]}
        assert differ == sparse[l], l
    assert M.planted(hash, leaf_len, lg, {})[2] == z[lg] == M.layers([bytes(leaf_len)] * 64, hash)[-1][0]


@pytest.mark.parametrize("hash", HASHES)
def test_periodic_shortcut_equals_the_dense_tree(hash):                                 # noqa: A002
    rng = np.random.default_rng(9)
    pool = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in range(8)]
    lg = 7
    lay = M.layers(pool * (1 << (lg - 3)), hash)
    pl, above = M.periodic(hash, pool, lg)
    for l in range(4):
        assert lay[l] == pl[l] * (1 << (lg - 3))
    for k, x in enumerate(above):
        assert set(lay[3 + k]) == {x}
    assert above[-1] == lay[-1][0]


def test_leaves_of_strided_buffers():
    eb, n, w = 4, 4, 3
    cols = np.arange(3 * 6, dtype=np.uint32)                                             # col_stride 6 > n
    got = M.leaves_of(cols.tobytes(), n, w, eb, 6, 1)
    assert got[1] == np.array([1, 7, 13], dtype=np.uint32).tobytes()
    rows = np.arange(4 * 5, dtype=np.uint32)                                             # leaf_stride 5 > width
    got = M.leaves_of(rows.tobytes(), n, w, eb, 1, 5)
    assert got[2] == np.array([10, 11, 12], dtype=np.uint32).tobytes()
