"""CPU: the Poseidon2 kernels' bodies run on the host (tests/emu/emu_poseidon2.cpp), over the steps of the driver's own route
with a small device, word for word against the host model (tests/poseidon2_model.py): the device's field classes and linear
layer shortcuts on one side, Python integers and the definition's matrices on the other -- two independent implementations.
Both fields; the parameters (2, 0), (8, 1) and the usual pair; random states and the edge values 0, 1 and p - 1 in every
position; trees at lg_n = 0, 1, 3, 10 (top only) and 11 (nodes once, then top), both layouts with padded strides whose gaps
hold garbage, every width relative to RATE."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import poseidon2_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CUS = 2                                                     # a small device: 16 work-groups, so that work-groups loop
FIELDS = ("bb31", "gl64")
ROUNDS = {"bb31": ((2, 0), (8, 1), (8, 13)), "gl64": ((2, 0), (8, 1), (8, 22))}
ELEM = {"bb31": 4, "gl64": 8}


@functools.lru_cache(maxsize=None)
def emu():
    so = os.path.join(HERE, "emu", "libemu_poseidon2.so")
    src = os.path.join(HERE, "emu", "emu_poseidon2.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    deps = [src, os.path.join(csrc, "merkle", "merkle_route.hpp"), os.path.join(csrc, "ff", "small_fields_dev.hpp"),
            os.path.join(csrc, "ff", "mont_dev.hpp")]
    deps += [os.path.join(csrc, "poseidon2", f) for f in os.listdir(os.path.join(csrc, "poseidon2"))]
    newest = max(os.stat(f).st_mtime for f in deps)
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp, cu, ci, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t
    L.emu_p2_permute.argtypes = [vp, vp, sz, cu, vp, cu, cu, cu]
    L.emu_p2_commit.argtypes = [vp, vp, vp, cu, cu, sz, sz, sz, vp, cu, cu, cu]
    L.emu_p2_route.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), cu]
    L.emu_p2_route.restype = cu
    for fn in (L.emu_p2_top, L.emu_p2_fused, L.emu_p2_wg_per_cu):
        fn.restype = cu
    L.emu_p2_width.argtypes = [cu]
    L.emu_p2_width.restype = cu
    return L


def aligned(dtype, count, fill=0):
    """an array of |count| items of |dtype| that starts 16-byte aligned"""
    item = np.dtype(dtype).itemsize
    raw = np.empty(count * item + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + count * item].view(dtype)
    out[:] = fill
    return out


def params(field, rf, rp, seed=0):
    from sppark_amd import poseidon2
    return poseidon2.test_params(field, rf, rp, seed)


def random_wire(field, rng, shape):
    """random canonical wire words (every word below p is the wire form of some element)"""
    p = M.MODULUS[field]
    if ELEM[field] == 4:
        return rng.integers(0, p, shape, dtype=np.uint64).astype(np.uint32)
    return (rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)) % np.uint64(p)


def model_permute(field, m, wire_states):
    vals = M.values(field, wire_states)
    got = M.permute([vals[:, i] for i in range(m.t)], m)
    out = M.to_wire(field, np.stack(got, axis=1))
    return np.array(out.tolist(), dtype=M.wire_dtype(field))


def test_geometry():
    L = emu()
    assert L.emu_p2_top() == 1024 and L.emu_p2_fused() == 3 and L.emu_p2_wg_per_cu() == 8
    assert (L.emu_p2_width(4), L.emu_p2_width(8), L.emu_p2_width(16), L.emu_p2_width(2)) == (16, 8, 0, 0)


@pytest.mark.parametrize("field", FIELDS)
def test_permute_random_and_edge_states(field):
    L = emu()
    p, t = M.MODULUS[field], M.WIDTH[field]
    rng = np.random.default_rng(11)
    edge = []
    for v in (0, 1, p - 1):                                  # canonical values: everywhere, and alone in every position
        edge.append([v] * t)
        for k in range(t):
            edge.append([v if i == k else 0 for i in range(t)])
            edge.append([v if i == k else p - 1 for i in range(t)])
    edge = np.array([[int(M.to_wire(field, x)) for x in row] for row in edge], dtype=M.wire_dtype(field))
    states = np.concatenate([edge, random_wire(field, rng, (600 - len(edge), t))])      # 600: more than two work-groups of lanes
    for rf, rp in ROUNDS[field]:
        prm = params(field, rf, rp, seed=rf * 100 + rp)
        m = M.of_params(prm)
        src = aligned(M.wire_dtype(field), states.size)
        src[:] = states.reshape(-1)
        out = aligned(M.wire_dtype(field), states.size, fill=5)
        keep = src.copy()
        assert L.emu_p2_permute(out.ctypes.data, src.ctypes.data, len(states), ELEM[field], prm.consts.ctypes.data, rf, rp, CUS) == 0
        want = model_permute(field, m, states)
        assert (src == keep).all() and (out.reshape(-1, t) == want).all(), (field, rf, rp)
        assert L.emu_p2_permute(src.ctypes.data, src.ctypes.data, len(states), ELEM[field], prm.consts.ctypes.data, rf, rp, CUS) == 0
        assert (src.reshape(-1, t) == want).all()                                        # in place


def matrix(field, lg, width, layout, seed):
    """(flat buffer of random words with the matrix in it, col_stride, leaf_stride, the (n, width) canonical leaves)"""
    n = 1 << lg
    cs, ls = (n + 3, 1) if layout == "columns" else (1, width + 2)
    total = width * cs if layout == "columns" else n * ls
    buf = aligned(M.wire_dtype(field), total)
    buf[:] = random_wire(field, np.random.default_rng(seed), total)
    return buf, cs, ls, M.leaves_of(field, buf, n, width, cs, ls)


def commit(L, field, prm, buf, lg, width, cs, ls, with_root=True):
    words = ((2 << lg) - 1) * 32 // ELEM[field]
    tree, root = aligned(M.wire_dtype(field), words, fill=0xA5), aligned(M.wire_dtype(field), 32 // ELEM[field], fill=0x5A)
    before = buf.copy()
    rc = L.emu_p2_commit(tree.ctypes.data, root.ctypes.data if with_root else None, buf.ctypes.data, ELEM[field], lg, width, cs, ls,
                         prm.consts.ctypes.data, prm.rounds_f, prm.rounds_p, CUS)
    assert rc == 0 and (buf == before).all()
    return tree.view(np.uint8), root                                                   # (the root as words)


@pytest.mark.parametrize("layout", ("columns", "rows"))
@pytest.mark.parametrize("field", FIELDS)
def test_trees_small_every_width_and_parameter_set(field, layout):
    L = emu()
    rate = M.WIDTH[field] // 2
    widths = (1, rate - 1, rate, rate + 1, 2 * rate, 2 * rate + 1, 3 * rate - 1)
    for rf, rp in ROUNDS[field]:
        prm = params(field, rf, rp, seed=rp)
        m = M.of_params(prm)
        for lg in (0, 1, 3):
            for width in widths:
                buf, cs, ls, leaves = matrix(field, lg, width, layout, 100 * width + lg)
                tree, root = commit(L, field, prm, buf, lg, width, cs, ls)
                lay = M.layers(leaves, m)
                assert (tree == M.tree_bytes(field, lay)).all(), (field, rf, rp, lg, width, layout)
                assert root.tobytes() == M.digest_bytes(field, lay, lg, 0)


@pytest.mark.parametrize("layout", ("columns", "rows"))
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("lg", (10, 11))
def test_trees_at_the_top_kernels_reach_and_one_nodes_launch_above(lg, field, layout):
    L = emu()
    rate = M.WIDTH[field] // 2
    prm = params(field, *M.USUAL[field])
    m = M.of_params(prm)
    width = rate + 1 if lg == 10 else 2
    buf, cs, ls, leaves = matrix(field, lg, width, layout, lg)
    tree, root = commit(L, field, prm, buf, lg, width, cs, ls, with_root=(layout == "columns"))
    lay = M.layers(leaves, m)
    assert (tree == M.tree_bytes(field, lay)).all()
    if layout == "columns":
        assert root.tobytes() == M.digest_bytes(field, lay, lg, 0)
    else:
        assert (root == 0x5A).all()                                                      # no root asked for: nothing written
