"""CPU: include/sppark_amd_poseidon2.h compiles as plain C and C++; the four BabyBear / Goldilocks libraries export the two
calls and no other library does; every rejection arrives with its message before a device is looked up (the same error
protocol with or without one); the Python wrappers raise on bad arguments; and the kernels' resources, from the code objects'
metadata: no k_p2_ kernel has a private segment (the state stayed in registers), every work-group is 256 lanes, only
k_p2_top uses LDS."""
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
CALLS = ("sppark_poseidon2_permute", "sppark_poseidon2_commit")
HAVE = ("bb31", "bb31_canonical", "gl64", "gl64_plonky2")
ELEM = {"bb31": 4, "bb31_canonical": 4, "gl64": 8, "gl64_plonky2": 8}
INVALID = -1                                               # negated hipErrorInvalidValue
MAX = (1 << 64) - 1


def _message(L, err):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    return msg


def _rejected(L, err, word):
    msg = _message(L, err)
    assert err.code == INVALID and msg, (err.code, msg)
    assert word in msg, (word, msg)


def test_poseidon2_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_poseidon2.h"\n'
            'int main(void) {\n'
            '  SppError (*pe)(size_t, void *, const void *, size_t, const void *, uint32_t, uint32_t, void *) = sppark_poseidon2_permute;\n'
            '  SppError (*co)(size_t, void *, void *, const void *, uint32_t, size_t, size_t, size_t, const void *, uint32_t, uint32_t, void *)'
            ' = sppark_poseidon2_commit;\n'
            '  int k = SPPARK_POSEIDON2_MAX_ROUNDS_F + SPPARK_POSEIDON2_MAX_ROUNDS_P + SPPARK_POSEIDON2_STATE_BYTES;\n'
            '  size_t bb = SPPARK_POSEIDON2_CONSTS(16, 8, 13), gl = SPPARK_POSEIDON2_CONSTS(8, 8, 22), t = SPPARK_MERKLE_TREE_BYTES(3);\n'
            '  return (pe == 0) + (co == 0) + (k != 144) + (bb != 157) + (gl != 94) + (t != 480); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_poseidon2_symbols_in_four_libraries_only(libs):
    assert len(libs) == 11 and set(HAVE) <= set(libs)
    for name, path in libs.items():
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.split()
        have = sorted(s for s in exported if "poseidon2" in s)
        assert have == (sorted(CALLS) if name in HAVE else []), (name, have)
        assert not [s for s in have if "batch" in s]


def test_poseidon2_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    for name in ("bb31", "gl64", "gl64_plonky2"):
        eb = ELEM[name]
        t = 64 // eb
        L = ffi.load(name)
        lg, width = 4, 3
        n = 1 << lg
        raw = [np.ones(4096 + 64, dtype=np.uint8) for _ in range(5)]
        base = [x.ctypes.data + (-x.ctypes.data) % 32 for x in raw]                       # 32-byte aligned
        a, tree, root, out, consts = base
        nconst = (8 * t + 13 + t) * eb
        commit = lambda **kw: L.sppark_poseidon2_commit(0, *[dict(dict(tree=tree, root=root, inp=a, lg=lg, width=width, cs=n, ls=1,   # noqa: E731
                                                                          consts=consts, rf=8, rp=13, stream=None), **kw)[k]
                                                                for k in ("tree", "root", "inp", "lg", "width", "cs", "ls", "consts", "rf", "rp", "stream")])
        permute = lambda **kw: L.sppark_poseidon2_permute(0, *[dict(dict(out=out, inp=a, count=8, consts=consts, rf=8, rp=13, stream=None), **kw)[k]  # noqa: E731
                                                                  for k in ("out", "inp", "count", "consts", "rf", "rp", "stream")])
        # commit: the matrix and tree rejections of sppark_merkle_commit
        _rejected(L, commit(tree=None), b"NULL tree")
        _rejected(L, commit(inp=None), b"NULL in")
        _rejected(L, commit(lg=29), b"lg_n")
        _rejected(L, commit(width=0), b"width")
        _rejected(L, commit(width=(1 << 32) // eb, cs=1, ls=(1 << 32) // eb), b"2^32")
        for cs, ls in ((n - 1, 1), (1, width - 1), (2, 2), (0, 0), (n, 2), (0, 1), (1, 0), (n + 1, n + 1)):
            _rejected(L, commit(cs=cs, ls=ls), b"strides")
        _rejected(L, commit(cs=MAX // 2, ls=1), b"overflow")
        _rejected(L, commit(cs=1, ls=MAX // 4, lg=4), b"overflow")
        _rejected(L, commit(cs=MAX // eb, ls=1, width=2), b"overflow")
        _rejected(L, commit(inp=a + 2), b"misaligned in")
        for shift in (1, 4, 8):
            _rejected(L, commit(tree=tree + shift), b"misaligned tree")
        span = (width * n) * eb
        for tr in (a, a + 16, a + span - 16, a - ((2 * n - 1) * 32 - 16)):
            _rejected(L, commit(tree=tr, root=None), b"tree may not overlap in")
        for r in (a, a + span - 1, a - 31):
            _rejected(L, commit(root=r), b"root may not overlap in")
        for r in (tree, tree + (2 * n - 2) * 32, tree + (2 * n - 1) * 32 - 1, tree - 31):
            _rejected(L, commit(root=r), b"root may not lie inside tree")
        # the constants and the round numbers, for both calls
        for call in (commit, permute):
            _rejected(L, call(consts=None), b"NULL consts")
            _rejected(L, call(consts=consts + eb // 2), b"misaligned consts")
            for rf in (0, 1, 3, 7, 17, 18, 1 << 31):
                _rejected(L, call(rf=rf), b"rounds_f")
            for rp in (65, 1000, (1 << 32) - 1):
                _rejected(L, call(rp=rp), b"rounds_p")
        for c in (tree, tree + (2 * n - 1) * 32 - eb, tree - nconst + eb):
            _rejected(L, commit(consts=c), b"consts may not overlap tree")
        for c in (root, root + 32 - eb, root - nconst + eb):
            _rejected(L, commit(consts=c), b"consts may not overlap root")
        # permute
        _rejected(L, permute(out=None), b"NULL")
        _rejected(L, permute(inp=None), b"NULL")
        _rejected(L, permute(count=(MAX // 64) + 1), b"overflow")
        _rejected(L, permute(out=out + 8), b"misaligned out or in")
        _rejected(L, permute(inp=a + 4), b"misaligned out or in")
        for o in (a + 64, a - 64, a + 8 * 64 - 16, a + 16):
            _rejected(L, permute(out=o), b"overlap in part")
        for c in (out, out + 8 * 64 - eb, out - nconst + eb):
            _rejected(L, permute(consts=c), b"consts may not overlap out")
        assert all((x == 1).all() for x in raw)
        # nothing to do is no error and needs no device
        err = permute(count=0)
        assert err.code == 0, _message(L, err)
        assert all((x == 1).all() for x in raw)


def test_poseidon2_wrappers_reject_bad_arguments(libs):
    from sppark_amd import merkle, poseidon2
    bb, gl = poseidon2.test_params("bb31"), poseidon2.test_params("gl64")
    assert (bb.width, bb.rounds_f, bb.rounds_p, gl.width, gl.rounds_f, gl.rounds_p) == (16, 8, 13, 8, 8, 22)
    ok = np.zeros(8 * 16 + 13 + 16, dtype=np.uint32)
    poseidon2.Params("bb31", 8, 13, ok)
    for field, rf, rp, consts in (("m31", 8, 13, ok), ("bls12_381", 8, 13, ok), ("bb31", 7, 13, ok), ("bb31", 0, 13, ok), ("bb31", 18, 13, ok),
                                  ("bb31", 8, 65, ok), ("bb31", 8, -1, ok), ("bb31", 8, 13, ok[:-1]), ("bb31", 8, 12, ok), ("gl64", 8, 13, ok),
                                  ("bb31", 8, 13, np.full(len(ok), 0x78000001, dtype=np.uint32))):
        with pytest.raises(ValueError):
            poseidon2.Params(field, rf, rp, consts)
    with pytest.raises(ValueError):
        poseidon2.Params("gl64", 8, 22, np.full(8 * 8 + 22 + 8, 0xffffffff00000001, dtype=np.uint64))
    # permute
    for bad in (np.zeros(16, dtype=np.uint32), np.zeros((3, 8), dtype=np.uint32), np.zeros((3, 16), dtype=np.uint64), np.zeros((2, 3, 16), dtype=np.uint32)):
        with pytest.raises(ValueError):
            poseidon2.permute(bad, bb)
    with pytest.raises(ValueError):
        poseidon2.permute(np.zeros((3, 16), dtype=np.uint32), bb, out=np.zeros((4, 16), dtype=np.uint32))
    with pytest.raises(ValueError):
        poseidon2.permute(np.zeros((6, 16), dtype=np.uint32)[::2], bb)                   # not contiguous
    assert poseidon2.permute(np.zeros((0, 16), dtype=np.uint32), bb).shape == (0, 16)    # nothing to do needs no device
    # commit: the matrix rules of merkle.commit
    good = np.ones((3, 16), dtype=np.uint64)
    for bad, kw in ((np.ones(16, dtype=np.uint64), {}), (np.ones((3, 12), dtype=np.uint64), {}), (np.ones((12, 3), dtype=np.uint64), dict(layout="rows")),
                    (good.T, {}), (good[::-1], {}), (np.ones((3, 0), dtype=np.uint64), {}), (good, dict(layout="diagonal")),
                    (good, dict(tree=np.zeros(merkle.tree_bytes(4) - 32, dtype=np.uint8))),
                    (good, dict(tree=np.zeros(merkle.tree_bytes(4) // 8, dtype=np.uint64)))):
        with pytest.raises(ValueError):
            poseidon2.commit(bad, gl, **kw)
    with pytest.raises(TypeError):
        poseidon2.commit(good, "gl64")
    # verify: malformed paths, indices and leaves are simply not accepted
    root = bytes(32)
    assert not poseidon2.verify(root, 1, np.zeros(3, dtype=np.uint64), [], gl)
    assert not poseidon2.verify(root, 0, np.zeros(3, dtype=np.uint64), [bytes(31)], gl)
    assert not poseidon2.verify(root, 0, b"", [], gl) and not poseidon2.verify(root, 0, bytes(12), [], gl)


KERNEL_OBJECTS = ["gl64__api_ntt_api.hip.o", "bb31__api_ntt_api.hip.o", "gl64_plonky2__api_ntt_api.hip.o", "bb31_canonical__api_ntt_api.hip.o"]
OTHER_OBJECTS = ["m31__api_poly_only_api.hip.o", "bb31x4__api_poly_only_api.hip.o", "bn254__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o"]


@pytest.mark.parametrize("obj", KERNEL_OBJECTS)
def test_poseidon2_kernels_resources(libs, obj):
    """Instances per library: one permute, leaves for the two layouts, one nodes, one top."""
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    hit = {k: v for k, v in meta.items() if "k_p2_" in k and "vgpr_count" in v}
    count = lambda word: len([k for k in hit if word in k])                                 # noqa: E731
    assert count("k_p2_permute") == 1 and count("k_p2_leaves") == 2 and count("k_p2_nodes") == 1 and count("k_p2_top") == 1, sorted(hit)
    assert len(hit) == 5 and not [k for k in hit if "k_merkle_" in k], sorted(hit)
    for name, md in hit.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, (name, md)
        assert int(md.get("vgpr_count") or 0) <= 128, (name, md)                          # (four waves per SIMD: poseidon2_route.hpp on S)
        if "k_p2_top" in name:
            assert int(md.get("group_segment_fixed_size") or 0) == (512 + 256) * 32, (name, md)
        else:
            assert int(md.get("group_segment_fixed_size") or 0) == 0, (name, md)


@pytest.mark.parametrize("obj", OTHER_OBJECTS)
def test_no_poseidon2_kernels_elsewhere(libs, obj):
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    assert not [k for k in meta if "k_p2_" in k]
