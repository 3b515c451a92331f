"""GPU tests of Poseidon2 (include/sppark_amd_poseidon2.h) through sppark_amd.poseidon2.  Field elements have one bit pattern,
so every comparison is exact.

Expected values come from tests/poseidon2_model.py (Python integers; BabyBear vectorised with numpy uint64, every product
below 2^62), which tests/test_emulation_poseidon2.py holds against the kernels' bodies on the host.  Small matrices go
through the whole model.  Larger ones use the two techniques of tests/test_merkle_gpu.py: a matrix that is zero but for
planted leaves has the zero-subtree digests Z_l everywhere except on the planted leaves' ways up (sees a misplaced or
misaddressed leaf or node, blind to what repeats), and a matrix whose leaves repeat a random pool of 2^6 has layers that
repeat the pool's (sees every low index bit and every lane's data path, blind to the high bits)."""
import functools

import numpy as np
import pytest

import poseidon2_model as M

pytestmark = pytest.mark.gpu

FIELDS = ("bb31", "gl64")
ROUNDS = {"bb31": ((2, 0), (8, 1), (8, 13)), "gl64": ((2, 0), (8, 1), (8, 22))}
LAYOUTS = ("columns", "rows")
COUNTS = (1, 63, 64, 65, 257, 1000)
# csrc/poseidon2/poseidon2_route.hpp: the top kernel takes a layer of at most 2^10 digests, a nodes launch covers S = 3 layers: the
# nodes kernel runs once from lg_n = 11 and twice from lg_n = 14; a grid is at most 8 work-groups of 256 lanes per CU
TOP_LG, S = 10, 3
WG_PER_CU, NT = 8, 256
POOL_LG = 6


def _signed(dtype):
    return np.int32 if np.dtype(dtype) == np.uint32 else np.int64


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(_signed(a.dtype))).cuda()


def _np(t, dtype=None):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(dtype) if dtype is not None else a


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _params(field, rf, rp):
    from sppark_amd import poseidon2
    prm = poseidon2.test_params(field, rf, rp, seed=7)
    return prm, M.of_params(prm)


def _usual(field):
    return _params(field, *M.USUAL[field])


def _random_wire(field, rng, shape):
    """random canonical wire words"""
    p = M.MODULUS[field]
    if M.WIDTH[field] == 16:
        return rng.integers(0, p, shape, dtype=np.uint64).astype(np.uint32)
    return (rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)) % np.uint64(p)


def _wire(field, vals):
    """canonical values (an array of the model's) -> wire words"""
    return np.array(M.to_wire(field, vals).tolist(), dtype=M.wire_dtype(field)).reshape(vals.shape)


# ---- permute ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _permute_case(field, rf, rp):
    """1000 states -- the edge values 0, 1 and p - 1 among them -- and their permutations; read-only, shared by the counts"""
    prm, m = _params(field, rf, rp)
    p, t = m.p, m.t
    states = _random_wire(field, np.random.default_rng(rf * 100 + rp), (max(COUNTS), t))
    for k, v in enumerate((0, 1, p - 1)):
        states[2 * k, :] = int(M.to_wire(field, v))
        states[2 * k + 1, k] = int(M.to_wire(field, v))
    vals = M.values(field, states)
    want = _wire(field, np.stack(M.permute([vals[:, i] for i in range(t)], m), axis=1))
    states.setflags(write=False)
    want.setflags(write=False)
    return states, want


@pytest.mark.parametrize("rounds", range(3))
@pytest.mark.parametrize("field", FIELDS)
def test_permute(field, rounds):
    from sppark_amd import poseidon2
    rf, rp = ROUNDS[field][rounds]
    prm, _m = _params(field, rf, rp)
    states, want = _permute_case(field, rf, rp)
    dt = states.dtype
    for count in COUNTS:
        src = states[:count].copy()
        # host, out of place and in place
        out = poseidon2.permute(src, prm)
        assert isinstance(out, np.ndarray) and (out == want[:count]).all() and (src == states[:count]).all(), (field, rf, rp, count)
        assert poseidon2.permute(src, prm, out=src) is src and (src == want[:count]).all(), (field, rf, rp, count)
        # device, out of place (into a buffer with room behind it) and in place
        d_src = _dev(states[:count])
        d_out = _dev(np.full((count + 2, states.shape[1]), 5, dtype=dt))
        poseidon2.permute(d_src, prm, out=d_out[:count])
        got = _np(d_out, dt)
        assert (got[:count] == want[:count]).all() and (got[count:] == 5).all(), (field, rf, rp, count)
        assert (_np(d_src, dt) == states[:count]).all()
        assert poseidon2.permute(d_src, prm, out=d_src) is d_src and (_np(d_src, dt) == want[:count]).all(), (field, rf, rp, count)
        # device states, host result
        host_out = np.zeros((count, states.shape[1]), dtype=dt)
        poseidon2.permute(_dev(states[:count]), prm, out=host_out)
        assert (host_out == want[:count]).all()


# ---- commit against the whole model ---------------------------------------------------------------------------------------------
def _matrix(field, lg, width, layout, seed):
    """(numpy matrix view with padded strides and garbage in the gaps, the (n, width) canonical leaves); the leaves depend on
    the seed alone, not on the layout"""
    n = 1 << lg
    rng = np.random.default_rng(seed)
    words = _random_wire(field, rng, (n, width))
    lines, count = (width, n) if layout == "columns" else (n, width)
    gap = 3
    base = _random_wire(field, rng, (lines, count + gap))
    base[:, count:] |= M.wire_dtype(field)(1 << 31)                                      # (the gaps: not even canonical)
    base[:, :count] = words.T if layout == "columns" else words
    return base[:, :count], M.values(field, words)


def _to_dev(mat):
    """the same strided view on the device (the gaps travel too)"""
    return _dev(mat.base)[:, :mat.shape[1]]


@functools.lru_cache(maxsize=None)
def _small_tree(field, lg, width):
    """the model's tree of _matrix(field, lg, width, any layout, 1000 * lg + width): computed once, shared by the layouts"""
    _prm, m = _usual(field)
    _mat, leaves = _matrix(field, lg, width, "rows", 1000 * lg + width)
    lay = M.layers(leaves, m)
    want = M.tree_bytes(field, lay)
    want.setflags(write=False)
    return lay, want


def _small_case(field, lg, width, layout):
    mat, leaves = _matrix(field, lg, width, layout, 1000 * lg + width)
    lay, want = _small_tree(field, lg, width)
    return mat, leaves, lay, want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("field", FIELDS)
def test_commit_small_against_the_whole_model(field, layout):
    """lg_n 0 .. 6, every width relative to RATE, padded strides with garbage in the gaps; device and host matrices alternate"""
    from sppark_amd import poseidon2
    prm, m = _usual(field)
    rate = m.rate
    k = 0
    for lg in range(0, 7):
        for width in (1, rate - 1, rate, rate + 1, 2 * rate, 2 * rate + 1, 3 * rate - 1):
            mat, leaves, lay, want = _small_case(field, lg, width, layout)
            src = _to_dev(mat) if k % 2 == 0 else mat
            k += 1
            before = _np(src.clone() if hasattr(src, "clone") else src.copy())
            tree, root = poseidon2.commit(src, prm, layout=layout)
            assert (_np(tree) == want).all(), (field, layout, lg, width)
            assert root.tobytes() == M.digest_bytes(field, lay, lg, 0)
            assert (_np(src) == before).all()


@pytest.mark.parametrize("field", FIELDS)
def test_commit_other_parameter_sets(field):
    from sppark_amd import poseidon2
    for rf, rp in ROUNDS[field][:2]:
        prm, m = _params(field, rf, rp)
        for layout in LAYOUTS:
            mat, leaves = _matrix(field, 5, m.rate + 1, layout, rf + rp)
            tree, root = poseidon2.commit(_to_dev(mat), prm, layout=layout)
            lay = M.layers(leaves, m)
            assert (_np(tree) == M.tree_bytes(field, lay)).all() and root.tobytes() == M.digest_bytes(field, lay, 5, 0)


@pytest.mark.parametrize("field", ("bb31_canonical", "gl64_plonky2"))
def test_variant_libraries_once(field):
    from sppark_amd import poseidon2
    prm, m = _usual(field)
    states = _random_wire(field, np.random.default_rng(5), (65, m.t))
    vals = M.values(field, states)
    want = _wire(field, np.stack(M.permute([vals[:, i] for i in range(m.t)], m), axis=1))
    assert (_np(poseidon2.permute(_dev(states), prm), states.dtype) == want).all()
    mat, leaves = _matrix(field, 5, m.rate + 1, "columns", 9)
    tree, root = poseidon2.commit(_to_dev(mat), prm)
    lay = M.layers(leaves, m)
    assert (_np(tree) == M.tree_bytes(field, lay)).all() and root.tobytes() == M.digest_bytes(field, lay, 5, 0)


# ---- route boundaries -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(field, width):
    """a random pool of 2^POOL_LG leaves as wire words (width, 2^POOL_LG), and its canonical leaves"""
    words = _random_wire(field, np.random.default_rng(77 + width), (width, 1 << POOL_LG))
    words.setflags(write=False)
    return words, M.values(field, words.T)


@pytest.mark.parametrize("lg", (TOP_LG, TOP_LG + 1, TOP_LG + S, TOP_LG + S + 1))
@pytest.mark.parametrize("field", FIELDS)
def test_periodic_at_the_route_boundaries(field, lg):
    """top only; nodes once; nodes once with a full top; nodes twice -- the whole tree, byte for byte"""
    from sppark_amd import merkle, poseidon2
    prm, m = _usual(field)
    width = m.rate + 1
    words, leaves = _pool(field, width)
    pool_layers, above = M.periodic(m, leaves, lg)
    mat = _dev(words).repeat(1, 1 << (lg - POOL_LG))
    tree, root = poseidon2.commit(mat, prm)
    assert root.tobytes() == above[-1]
    host = _np(tree)
    for l in range(lg + 1):
        got = merkle.layer(host, lg, l)
        if l <= POOL_LG:
            one = np.frombuffer(M.layer_bytes(field, pool_layers[l]), dtype=np.uint8).reshape(-1, 32)
            assert (got.reshape(-1, one.shape[0], 32) == one[None]).all(), (lg, l)
        else:
            assert (got == np.frombuffer(above[l - POOL_LG], dtype=np.uint8)[None]).all(), (lg, l)


def _plant_positions(lg):
    n = 1 << lg
    sweep = _cus() * WG_PER_CU * NT                                                     # leaves of one grid-stride sweep
    pos = [0, 63, 64, 255, 256, n - 1]
    if sweep < n:
        pos += [sweep - 1, sweep]
    return sorted(set(q for q in pos if q < n))


@pytest.mark.parametrize("lg", (TOP_LG + 1, TOP_LG + S + 1, 20))
@pytest.mark.parametrize("field", FIELDS)
def test_planted_leaves(field, lg):
    """lg_n = 20: 2^20 leaves are more than a grid of 8 work-groups of 256 lanes per CU covers at once on any device of up to 511
    CUs -- the grid stride runs, and leaves on both sides of the first sweep's end are planted"""
    import torch
    from sppark_amd import merkle, poseidon2
    prm, m = _usual(field)
    width, n = m.rate + 1, 1 << lg
    if lg == 20:
        assert _cus() * WG_PER_CU * NT < n
    dt = M.wire_dtype(field)
    mat = torch.zeros((width, n), dtype=torch.int32 if dt == np.uint32 else torch.int64, device="cuda")
    plants = {}
    for k, i in enumerate(_plant_positions(lg)):
        leaf = [1000 * (k + 1) + 17 * j + 1 for j in range(width)]
        mat[:, i] = _dev(np.array([int(M.to_wire(field, v)) for v in leaf], dtype=dt))
        plants[i] = leaf
    sparse, z, root_want = M.planted(m, width, lg, plants)
    tree, root = poseidon2.commit(mat, prm)
    for l in range(lg + 1):
        lay = merkle.layer(tree, lg, l)
        zt = torch.from_numpy(np.frombuffer(z[l], dtype=np.int64).copy()).cuda()
        differ = (lay.view(torch.int64) != zt).any(dim=1).nonzero().reshape(-1).cpu().tolist()
        assert differ == sorted(sparse[l]), (l, differ[:8], sorted(sparse[l]))
        for i in differ:
            assert lay[i].cpu().numpy().tobytes() == sparse[l][i], (l, i)
    assert _np(root).tobytes() == root_want


# ---- round trip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("field", FIELDS)
def test_commit_open_gather_verify(field, layout):
    from sppark_amd import merkle, poseidon2
    prm, m = _usual(field)
    lg, width = 8, 2 * m.rate + 1
    n = 1 << lg
    mat, leaves = _matrix(field, lg, width, layout, 31)
    src = _to_dev(mat)
    tree, root = poseidon2.commit(src, prm, layout=layout)
    idx = [0, n - 1] + [int(x) for x in np.random.default_rng(lg).integers(0, n, 6)]
    paths = _np(merkle.open(tree, lg, idx, field=field))
    rows = _np(merkle.gather(src, idx, layout=layout, field=field))
    assert paths.shape == (len(idx), lg, 32)
    for q, i in enumerate(idx):
        assert rows[q].tobytes() == _wire(field, leaves[i]).tobytes()
        assert poseidon2.verify(root, i, rows[q], paths[q], prm)
        assert not poseidon2.verify(root, i ^ 1, rows[q], paths[q], prm)
    assert not poseidon2.verify(root, idx[0], rows[1], paths[0], prm)                    # another leaf's elements
    assert M.verify(m, root.tobytes(), idx[2], [int(v) for v in leaves[idx[2]]], [q.tobytes() for q in paths[2]])


# ---- the enqueue contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_enqueue_on_a_side_stream_and_host_constants(field):
    import torch
    from sppark_amd import ffi, merkle, poseidon2
    prm, m = _usual(field)
    lg, width = 12, m.rate + 1
    words, leaves = _pool(field, width)
    pool_layers, above = M.periodic(m, leaves, lg)
    mat = _dev(words).repeat(1, 1 << (lg - POOL_LG))
    states, want = _permute_case(field, *M.USUAL[field])
    d_states = _dev(states)
    d_out = torch.zeros_like(d_states)
    tree = torch.zeros(merkle.tree_bytes(lg), dtype=torch.uint8, device="cuda")
    prm.device(0)                                                                        # (the constants' copy: before the stream's work)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got_tree, root = poseidon2.commit(mat, prm, tree=tree, stream=s.cuda_stream)
    poseidon2.permute(d_states, prm, out=d_out, stream=s.cuda_stream)
    s.synchronize()                                                                      # one synchronise
    assert got_tree is tree and root.is_cuda and root.data_ptr() == tree.data_ptr() + merkle.tree_bytes(lg) - 32
    assert _np(root).tobytes() == above[-1]
    layer0 = np.frombuffer(M.layer_bytes(field, pool_layers[0]), dtype=np.uint8).reshape(-1, 32)
    assert (_np(merkle.layer(tree, lg, 0)).reshape(-1, 1 << POOL_LG, 32) == layer0[None]).all()
    assert (_np(d_out, states.dtype) == want).all()
    want_tree = _np(tree).copy()
    # constants on the host, everything else on the device, a stream: the staged path, complete when the call returns
    L = ffi.load(field)
    tree2 = torch.zeros_like(tree)
    d_out2 = torch.zeros_like(d_states)
    ffi.check(L, L.sppark_poseidon2_commit(0, tree2.data_ptr(), None, mat.data_ptr(), lg, width, mat.stride(0), 1, prm.consts.ctypes.data,
                                           prm.rounds_f, prm.rounds_p, s.cuda_stream))
    ffi.check(L, L.sppark_poseidon2_permute(0, d_out2.data_ptr(), d_states.data_ptr(), len(states), prm.consts.ctypes.data,
                                            prm.rounds_f, prm.rounds_p, s.cuda_stream))
    s.synchronize()
    assert (_np(tree2) == want_tree).all() and (_np(d_out2, states.dtype) == want).all()
    # a host tree and a host root from a device matrix
    t3, r3 = poseidon2.commit(mat, prm, tree=np.zeros(merkle.tree_bytes(lg), dtype=np.uint8))
    assert isinstance(t3, np.ndarray) and (t3 == want_tree).all() and r3.tobytes() == above[-1]
