"""CPU: include/sppark_amd_merkle.h -- Merkle commitments -- compiles as plain C and C++; all eleven product libraries export
the three calls; every rejection arrives before a device is looked up (the same error protocol with or without one); the
Python wrappers reject bad shapes and strides before they reach the library; and the new kernels' resources, from the code
objects' metadata: no kernel has a private segment (the message and state words stayed in registers), every work-group is
256 lanes, the nodes kernel uses no LDS."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
CALLS = ("sppark_merkle_commit", "sppark_merkle_open", "sppark_merkle_gather")
ELEM = (("gl64", 8), ("bls12_381", 32), ("m31", 4), ("bb31x4", 16), ("bb31", 4))
INVALID = -1                                               # negated hipErrorInvalidValue
BLAKE2S, SHA256 = 0, 1
MAX = (1 << 64) - 1


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def _rejected(L, err, word=None):
    msg = _message(L, err)
    assert err.code == INVALID and msg, (err.code, msg)
    if word is not None:
        assert word in msg, msg


def test_merkle_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_merkle.h"\n'
            'int main(void) {\n'
            '  SppError (*co)(size_t, void *, void *, const void *, uint32_t, size_t, size_t, size_t, int, void *) = sppark_merkle_commit;\n'
            '  SppError (*op)(size_t, void *, const void *, uint32_t, const uint64_t *, size_t, void *) = sppark_merkle_open;\n'
            '  SppError (*ga)(size_t, void *, const void *, uint32_t, size_t, size_t, size_t, const uint64_t *, size_t, void *)'
            ' = sppark_merkle_gather;\n'
            '  int k = SPPARK_HASH_BLAKE2S + SPPARK_HASH_SHA256 + SPPARK_MERKLE_MAX_LG + SPPARK_MERKLE_DIGEST_BYTES;\n'
            '  size_t t0 = SPPARK_MERKLE_TREE_BYTES(0), t3 = SPPARK_MERKLE_TREE_BYTES(3), t28 = SPPARK_MERKLE_TREE_BYTES(28);\n'
            '  return (co == 0) + (op == 0) + (ga == 0) + (k != 61) + (t0 != 32) + (t3 != 480) + (t28 / 32 != 536870911u); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_merkle_symbols_exported(libs):
    assert len(libs) == 11
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        for fn in CALLS:
            assert hasattr(L, fn), (name, fn)


def test_merkle_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    for name, eb in ELEM:
        L = ffi.load(name)
        lg, width = 4, 3
        n = 1 << lg
        raw = [np.ones(4096 + 64, dtype=np.uint8) for _ in range(4)]
        base = [x.ctypes.data + (-x.ctypes.data) % 32 for x in raw]                       # 32-byte aligned
        a, tree, root, out = base
        idx = np.array([0, n - 1, 5], dtype=np.uint64)
        ip = idx.ctypes.data
        one, zero = np.array([1], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        commit = lambda **kw: L.sppark_merkle_commit(0, *[dict(dict(tree=tree, root=root, inp=a, lg=lg, width=width, cs=n, ls=1,     # noqa: E731
                                                                       hash=BLAKE2S, stream=None), **kw)[k]
                                                             for k in ("tree", "root", "inp", "lg", "width", "cs", "ls", "hash", "stream")])
        gather = lambda **kw: L.sppark_merkle_gather(0, *[dict(dict(rows=out, inp=a, lg=lg, width=width, cs=n, ls=1, idx=ip, nidx=3, stream=None), **kw)[k]  # noqa: E731
                                                             for k in ("rows", "inp", "lg", "width", "cs", "ls", "idx", "nidx", "stream")])
        # commit
        _rejected(L, commit(tree=None), b"NULL")
        _rejected(L, commit(inp=None), b"NULL")
        _rejected(L, commit(lg=29), b"lg_n")
        _rejected(L, commit(width=0), b"width")
        _rejected(L, commit(width=(1 << 32) // eb, cs=1, ls=(1 << 32) // eb), b"2^32")
        for cs, ls in ((n - 1, 1), (1, width - 1), (2, 2), (0, 0), (n, 2), (0, 1), (1, 0), (n + 1, n + 1)):       # neither layout
            _rejected(L, commit(cs=cs, ls=ls), b"strides")
        _rejected(L, commit(cs=MAX // 2, ls=1), b"overflow")                              # (width - 1) * col_stride
        _rejected(L, commit(cs=1, ls=MAX // 4, lg=4), b"overflow")                        # (n - 1) * leaf_stride
        _rejected(L, commit(cs=MAX // eb, ls=1, width=2), b"overflow")                    # the span in bytes
        for hash in (-1, 2, 7):                                                           # noqa: A001
            _rejected(L, commit(hash=hash), b"hash")
        for shift in (1, 4, 8):
            _rejected(L, commit(tree=tree + shift), b"misaligned")
        _rejected(L, commit(inp=a + 2), b"misaligned")
        span = (width * n) * eb
        for t in (a, a + 16, a + span - 16, a - ((2 * n - 1) * 32 - 16)):                 # tree over in
            _rejected(L, commit(tree=t, root=None), b"overlap")
        for r in (a, a + span - 1, a - 31):                                               # root over in
            _rejected(L, commit(root=r), b"overlap")
        for r in (tree, tree + (2 * n - 2) * 32, tree + (2 * n - 1) * 32 - 1, tree - 31):  # root inside tree
            _rejected(L, commit(root=r), b"root")
        # open
        _rejected(L, L.sppark_merkle_open(0, None, tree, lg, ip, 3, None), b"NULL")
        _rejected(L, L.sppark_merkle_open(0, out, None, lg, ip, 3, None), b"NULL")
        _rejected(L, L.sppark_merkle_open(0, out, tree, lg, None, 3, None), b"indices")
        _rejected(L, L.sppark_merkle_open(0, out, tree, 29, ip, 3, None), b"lg_n")
        _rejected(L, L.sppark_merkle_open(0, out, tree, lg, ip, MAX // 8, None), b"overflow")  # (before an index is read)
        _rejected(L, L.sppark_merkle_open(0, tree + 64, tree, lg, ip, 3, None), b"overlap")
        for bad in (n, n + 1, 1 << 40, MAX):
            bad_idx = np.array([1, bad, 2], dtype=np.uint64)
            _rejected(L, L.sppark_merkle_open(0, out, tree, lg, bad_idx.ctypes.data, 3, None), b"index")
            _rejected(L, gather(idx=bad_idx.ctypes.data), b"index")
        _rejected(L, L.sppark_merkle_open(0, out, tree, 0, one.ctypes.data, 1, None), b"index")
        # gather
        _rejected(L, gather(rows=None), b"NULL")
        _rejected(L, gather(inp=None), b"NULL")
        _rejected(L, gather(idx=None), b"indices")
        _rejected(L, gather(lg=29), b"lg_n")
        _rejected(L, gather(width=0), b"width")
        _rejected(L, gather(cs=2, ls=2), b"strides")
        _rejected(L, gather(rows=a + span - 4), b"overlap")
        _rejected(L, gather(nidx=MAX // 2, width=1 << 20, cs=1, ls=1 << 20, idx=zero.ctypes.data, lg=0), b"overflow")
        assert all((x == 1).all() for x in raw)
        # nothing to do is no error and needs no device: no query; no layer below the root
        for err in (L.sppark_merkle_open(0, out, tree, lg, None, 0, None), L.sppark_merkle_open(0, out, tree, 0, zero.ctypes.data, 1, None),
                    gather(idx=None, nidx=0)):
            assert err.code == 0, _message(L, err)
        assert all((x == 1).all() for x in raw)


def test_merkle_wrappers_reject_bad_shapes(libs):
    from sppark_amd import merkle
    good = np.ones((3, 16), dtype=np.uint64)
    with pytest.raises(ValueError):
        merkle.commit(np.ones(16, dtype=np.uint64))                                       # not 2-D
    with pytest.raises(ValueError):
        merkle.commit(np.ones((2, 3, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        merkle.commit(np.ones((3, 12), dtype=np.uint64))                                  # 12 leaves
    with pytest.raises(ValueError):
        merkle.commit(np.ones((12, 3), dtype=np.uint64), layout="rows")
    with pytest.raises(ValueError):
        merkle.commit(good.T)                                                             # words of a line not contiguous
    with pytest.raises(ValueError):
        merkle.commit(np.ones((3, 32), dtype=np.uint64)[:, ::2])
    with pytest.raises(ValueError):
        merkle.commit(good[::-1])                                                         # a negative stride
    with pytest.raises(ValueError):
        merkle.commit(np.ones((3, 0), dtype=np.uint64))
    with pytest.raises(ValueError):
        merkle.commit(np.ones((3, 6), dtype=np.uint64), field="bls12_381")                # 1.5 elements per line
    with pytest.raises(ValueError):
        merkle.commit(np.ones((4, 10), dtype=np.uint64)[:, :8], field="bls12_381", layout="rows")      # lines 2.5 elements apart
    with pytest.raises(ValueError):
        merkle.commit(good, hash="keccak")
    with pytest.raises(ValueError):
        merkle.commit(good, layout="diagonal")
    with pytest.raises(ValueError):
        merkle.commit(good, tree=np.zeros(merkle.tree_bytes(4) - 32, dtype=np.uint8))
    with pytest.raises(ValueError):
        merkle.commit(good, tree=np.zeros(merkle.tree_bytes(4) // 8, dtype=np.uint64))    # bytes, please
    tree = np.zeros(merkle.tree_bytes(4), dtype=np.uint8)
    for bad in ([16], [3, 99], [-1]):
        with pytest.raises((ValueError, OverflowError)):
            merkle.open(tree, 4, bad)
        with pytest.raises((ValueError, OverflowError)):
            merkle.gather(good, bad)
    with pytest.raises(ValueError):
        merkle.open(tree, 5, [0])
    with pytest.raises(ValueError):
        merkle.open(tree, 4, [0, 1], out=np.zeros(4 * 32, dtype=np.uint8))
    with pytest.raises(ValueError):
        merkle.gather(good, [0, 1], out=np.zeros(5 * 8, dtype=np.uint8))
    with pytest.raises(ValueError):
        merkle.layer(tree, 4, 5)
    with pytest.raises(ValueError):
        merkle.tree_bytes(29)
    assert merkle.tree_bytes(0) == 32 and merkle.tree_bytes(28) == ((1 << 29) - 1) * 32
    assert merkle.layer(tree, 4, 0).shape == (16, 32) and merkle.layer(tree, 4, 4).shape == (1, 32)
    lay = merkle.layer(tree, 4, 3)
    lay[:] = 7                                                                            # a view
    assert tree[(32 - 4) * 32:(32 - 2) * 32].min() == 7 and tree.sum() == 7 * 64
    # what needs no device works without one: no query, no layer below the root
    assert merkle.open(tree, 4, []).shape == (0, 4, 32)
    assert merkle.gather(good, []).shape == (0, 24)
    assert merkle.open(np.zeros(32, dtype=np.uint8), 0, [0, 0]).shape == (2, 0, 32)


KERNEL_OBJECTS = ["gl64__api_ntt_api.hip.o", "bb31__api_ntt_api.hip.o", "m31__api_poly_only_api.hip.o", "bb31x4__api_poly_only_api.hip.o",
                  "bls12_381__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o", "bn254__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o"]


@pytest.mark.parametrize("obj", KERNEL_OBJECTS)
def test_merkle_kernels_resources(libs, obj):
    """Instances per library: leaves 2 hashes x 2 layouts for the library's words per element, nodes and top one per hash, one
    open, one gather."""
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    hit = {k: v for k, v in meta.items() if "k_merkle_" in k and "vgpr_count" in v}
    count = lambda word: len([k for k in hit if word in k])                                 # noqa: E731
    assert count("k_merkle_leaves") == 4 and count("k_merkle_nodes") == 2 and count("k_merkle_top") == 2, sorted(hit)
    assert count("k_merkle_open") == 1 and count("k_merkle_gather") == 1 and len(hit) == 10, sorted(hit)
    for name, md in hit.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, (name, md)
        if "k_merkle_top" in name:
            assert int(md.get("group_segment_fixed_size") or 0) == (512 + 256) * 32, (name, md)
        else:
            assert int(md.get("group_segment_fixed_size") or 0) == 0, (name, md)
