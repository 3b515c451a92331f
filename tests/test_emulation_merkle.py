"""CPU: the Merkle kernels' bodies run on the host (tests/emu/emu_merkle.cpp), over the steps of the driver's own route with
a small device, byte for byte against the host model (tests/merkle_model.py, hashlib): both hashes, both layouts with padded
strides whose gaps hold garbage, every leaf length at a padding edge of either hash reached through elements of 1, 2, 4 and
8 words, and lg_n from 0 to two past the size at which the nodes kernel first runs twice."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import merkle_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CUS = 2                                                     # a small device: 16 work-groups, so that work-groups loop
HASHES = ("blake2s", "sha256")
# csrc/merkle/merkle_route.hpp: the top kernel takes a layer of at most 2^10 digests, a nodes launch covers 3 layers: the nodes
# kernel runs once from lg_n = 11, twice from lg_n = 14
TOP_LG, FUSED = 10, 3
TWICE = TOP_LG + FUSED + 1
# leaf lengths at every padding edge: BLAKE2s' last block (a multiple of 64: no empty block), SHA-256's second padding block
# (length mod 64 > 52)
EDGE_BYTES = (4, 8, 48, 52, 56, 60, 64, 68, 116, 120, 124, 128, 132, 192, 260)
# (29 and 48 words: 116 and 192 bytes are reached by no product of the other widths with 1, 2, 4 or 8 words)
WIDTHS = tuple(range(1, 6)) + tuple(range(13, 18)) + (29, 31, 32, 33, 48, 65)


@functools.lru_cache(maxsize=None)
def emu():
    so = os.path.join(HERE, "emu", "libemu_merkle.so")
    src = os.path.join(HERE, "emu", "emu_merkle.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc", "merkle")
    newest = max([os.stat(src).st_mtime] + [os.stat(os.path.join(csrc, f)).st_mtime for f in os.listdir(csrc)])
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp, cu, ci, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t
    L.emu_merkle_commit.argtypes = [vp, vp, vp, cu, cu, sz, sz, sz, ci, cu]
    L.emu_merkle_open.argtypes = [vp, vp, cu, vp, sz]
    L.emu_merkle_gather.argtypes = [vp, vp, cu, sz, sz, sz, vp, sz]
    L.emu_merkle_route.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), cu]
    L.emu_merkle_route.restype = cu
    L.emu_merkle_top.restype = cu
    L.emu_merkle_fused.restype = cu
    return L


def aligned_bytes(nbytes, fill=None, seed=0):
    """a uint8 view of nbytes that starts 16-byte aligned"""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + nbytes]
    if fill is None:
        out[:] = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    else:
        out[:] = fill
    return out


def matrix(ew, lg, width, layout, seed):
    """(buffer of garbage with the matrix in it, col_stride, leaf_stride, the leaves as bytes): padded strides"""
    n, eb = 1 << lg, 4 * ew
    cs, ls = (n + 3, 1) if layout == "columns" else (1, width + 2)
    total = (width * cs if layout == "columns" else n * ls) * eb
    buf = aligned_bytes(total, seed=seed)
    return buf, cs, ls, M.leaves_of(buf.tobytes(), n, width, eb, cs, ls)


def commit(L, buf, ew, lg, width, cs, ls, hash):                                         # noqa: A002
    nbytes = ((2 << lg) - 1) * 32
    tree, root = aligned_bytes(nbytes, fill=0xA5), aligned_bytes(32, fill=0x5A)
    before = buf.copy()
    assert L.emu_merkle_commit(tree.ctypes.data, root.ctypes.data, buf.ctypes.data, ew, lg, width, cs, ls, M.HASH_ID[hash], CUS) == 0
    assert (buf == before).all()
    return tree, root


def test_geometry():
    L = emu()
    assert L.emu_merkle_top() == 1 << TOP_LG and L.emu_merkle_fused() == FUSED


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("ew", (1, 2, 4, 8))
def test_leaf_lengths_at_every_padding_edge(ew, hash):                                   # noqa: A002
    L = emu()
    for width in WIDTHS:
        for layout in ("columns", "rows"):
            lg = 3
            buf, cs, ls, leaves = matrix(ew, lg, width, layout, 100 * width + ew)
            tree, root = commit(L, buf, ew, lg, width, cs, ls, hash)
            lay = M.layers(leaves, hash)
            assert (tree == M.tree_bytes(lay)).all(), (ew, width, layout, hash)
            assert root.tobytes() == lay[-1][0]


def test_every_edge_length_is_reached():
    reach = {w * ew * 4 for w in WIDTHS for ew in (1, 2, 4, 8)}
    assert set(EDGE_BYTES) <= reach


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("layout", ("columns", "rows"))
def test_every_size_up_to_two_past_the_second_nodes_launch(layout, hash):                # noqa: A002
    L = emu()
    for lg in range(0, TWICE + 3):
        ew, width = ((1, 3), (2, 1), (4, 1), (8, 1))[lg % 4] if lg > 12 else ((1, 17), (2, 5), (4, 3), (8, 2))[lg % 4]
        buf, cs, ls, leaves = matrix(ew, lg, width, layout, lg)
        tree, root = commit(L, buf, ew, lg, width, cs, ls, hash)
        lay = M.layers(leaves, hash)
        assert (tree == M.tree_bytes(lay)).all(), (lg, ew, width)
        assert root.tobytes() == lay[-1][0]
        if lg in (0, 5, 11, TWICE):
            rng = np.random.default_rng(lg)
            idx = np.array([0, (1 << lg) - 1] + [int(x) for x in rng.integers(0, 1 << lg, 5)], dtype=np.uint64)
            paths = aligned_bytes(len(idx) * max(lg, 1) * 32, fill=0)
            rows = aligned_bytes(len(idx) * width * ew * 4, fill=0)
            assert L.emu_merkle_open(paths.ctypes.data, tree.ctypes.data, lg, idx.ctypes.data, len(idx)) == 0
            assert L.emu_merkle_gather(rows.ctypes.data, buf.ctypes.data, ew, width, cs, ls, idx.ctypes.data, len(idx)) == 0
            for q, i in enumerate(idx):
                i = int(i)
                got = [paths[(q * lg + l) * 32:][:32].tobytes() for l in range(lg)]
                assert got == M.path(lay, i)
                row = rows[q * width * ew * 4:][:width * ew * 4].tobytes()
                assert row == leaves[i] and M.verify(hash, root.tobytes(), i, row, got)


def test_unpadded_strides_and_no_root():
    L = emu()
    lg, ew, width = 4, 2, 3
    n = 1 << lg
    buf = aligned_bytes(n * width * 8, seed=3)
    for cs, ls in ((n, 1), (1, width)):
        leaves = M.leaves_of(buf.tobytes(), n, width, 8, cs, ls)
        tree = aligned_bytes(((2 << lg) - 1) * 32, fill=0)
        assert L.emu_merkle_commit(tree.ctypes.data, None, buf.ctypes.data, ew, lg, width, cs, ls, 0, CUS) == 0
        assert (tree == M.tree_bytes(M.layers(leaves, "blake2s"))).all()
