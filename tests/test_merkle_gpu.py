"""GPU tests of the Merkle commitments (include/sppark_amd_merkle.h) through sppark_amd.merkle.  Digests are bytes, so every
comparison is exact.

Expected values come from hashlib (tests/merkle_model.py).  Small matrices go through the whole model.  Large ones need no
big model: a matrix that is zero but for planted leaves has the zero-subtree digests Z_l everywhere except on the planted
leaves' ways up (O(lg_n) hashes each; sees a misplaced or misaddressed leaf or node, blind to what repeats), and a matrix
whose leaves repeat a random pool of 2^m has layers that repeat the pool's (sees every low index bit and every lane's data
path, blind to the high bits).  The elements are opaque to the kernels, so the matrices hold random words."""
import functools
import threading

import numpy as np
import pytest

import merkle_model as M
from test_field_inverse_gpu import FIELDS

pytestmark = pytest.mark.gpu

HASHES = ("blake2s", "sha256")
LAYOUTS = ("columns", "rows")
SIZED = ["bb31", "gl64", "bb31x4", "bls12_381"]            # one library per element size: 4, 8, 16, 32 bytes
ELEM_BYTES = {"gl64": 8, "gl64_plonky2": 8, "bb31": 4, "bb31_canonical": 4, "m31": 4, "bb31x4": 16}
# csrc/merkle/merkle_route.hpp: the top kernel takes a layer of at most 2^10 digests, a nodes launch covers 3 layers, so the
# nodes kernel runs twice (and then the top kernel) from lg_n = 14; a grid is at most 8 work-groups of 256 lanes per CU
TWICE_LG = 14
WG_PER_CU, NT = 8, 256
EDGE_BYTES = (4, 8, 48, 52, 56, 60, 64, 68, 116, 120, 124, 128, 132, 192, 260)


def _eb(field):
    return ELEM_BYTES.get(field, 32)


def _word(field):
    """(numpy dtype of a word, words per element)"""
    eb = _eb(field)
    return (np.uint32, eb // 4) if eb in (4, 16) else (np.uint64, eb // 8)


def _edge_widths(field):
    eb = _eb(field)
    return [b // eb for b in EDGE_BYTES if b % eb == 0]


def _matrix(field, lg, width, layout, seed):
    """(numpy matrix view with padded strides and garbage in the gaps, the leaves as bytes)"""
    dtype, w = _word(field)
    n = 1 << lg
    lines, count = (width, n) if layout == "columns" else (n, width)
    gap = 3
    base = np.random.default_rng(seed).integers(0, 1 << 32, (lines, (count + gap) * w * (np.dtype(dtype).itemsize // 4)), dtype=np.uint32)
    base = base.view(dtype).copy()                                                      # (owns its memory: mat.base is base)
    mat = base[:, :count * w]
    cs, ls = (count + gap, 1) if layout == "columns" else (1, count + gap)
    return mat, M.leaves_of(base.tobytes(), n, width, _eb(field), cs, ls)


def _to_dev(mat):
    """the same strided view on the device (the gaps travel too)"""
    import torch
    base = mat.base if mat.base is not None else mat
    signed = np.int32 if mat.dtype == np.uint32 else np.int64
    t = torch.from_numpy(np.array(base).view(signed)).cuda()
    return t[:, :mat.shape[1]]


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _small_case(field, lg, width, layout, hash):                                         # noqa: A002
    mat, leaves = _matrix(field, lg, width, layout, 1000 * lg + width)
    mat.setflags(write=False)
    lay = M.layers(leaves, hash)
    want = M.tree_bytes(lay)
    want.setflags(write=False)
    return mat, leaves, lay, want


@pytest.mark.parametrize("field", FIELDS)
def test_every_library_once(field):
    lg, width = 6, 3
    from sppark_amd import merkle
    for k, (hash, layout) in enumerate((h, l) for h in HASHES for l in LAYOUTS):         # noqa: A001
        mat, leaves, lay, want = _small_case(field, lg, width, layout, hash)
        src = _to_dev(mat) if k % 2 == 0 else mat
        tree, root = merkle.commit(src, hash=hash, layout=layout, field=field)
        assert (_np(tree) == want).all(), (field, hash, layout)
        assert root.tobytes() == lay[-1][0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("field", SIZED)
def test_dense_small(field, hash, layout):                                               # noqa: A002
    """every lg_n from 0 to the first that runs the nodes kernel twice and then the top kernel, the width walking over the
    padding edges; then every edge width at 2^9 leaves (two work-groups); device and host matrices alternate"""
    from sppark_amd import merkle
    edges = _edge_widths(field)
    short = [w for w in edges if w * _eb(field) <= 68]
    cases = [(lg, edges[lg % len(edges)]) for lg in range(0, TWICE_LG + 1)] + [(9, w) for w in edges]
    for k, (lg, width) in enumerate(cases):
        if lg > 11:
            width = short[lg % len(short)]                                               # (keeps the host model quick)
        mat, leaves, lay, want = _small_case(field, lg, width, layout, hash)
        src = _to_dev(mat) if k % 2 == 0 else mat
        before = _np(src.clone() if hasattr(src, "clone") else src.copy())
        tree, root = merkle.commit(src, hash=hash, layout=layout, field=field)
        assert (_np(tree) == want).all(), (field, hash, layout, lg, width)
        assert root.tobytes() == lay[-1][0]
        assert (_np(src) == before).all()


# ---- large matrices ----------------------------------------------------------------------------------------------------------
def _plant_positions(lg):
    n = 1 << lg
    sweep = _cus() * WG_PER_CU * NT                                                     # leaves of one grid-stride sweep
    pos = [0, 63, 64, 255, 256, n - 1]
    if sweep < n:
        pos += [sweep - 1, sweep]
    return sorted(set(p for p in pos if p < n))


def _planted_device(field, lg, width, cols):
    """a zero columns-layout matrix on the device with distinct words planted in |cols| of the planted leaves; the plants"""
    import torch
    dtype, w = _word(field)
    tdt = torch.int32 if dtype == np.uint32 else torch.int64
    n = 1 << lg
    mat = torch.zeros((width, n * w), dtype=tdt, device="cuda")
    plants = {}
    for k, i in enumerate(_plant_positions(lg)):
        leaf = np.zeros((width, w), dtype=dtype)
        for j in cols:
            leaf[j] = np.arange(1, w + 1, dtype=dtype) + 1000 * (k + 1) + 17 * j
        mat[:, i * w:(i + 1) * w] = torch.from_numpy(leaf.view(np.int32 if dtype == np.uint32 else np.int64)).cuda()
        plants[i] = leaf.tobytes()
    return mat, plants


def _check_sparse(tree, lg, sparse, z, root_want, root):
    """per layer, on the device: the digests that differ from Z_l are exactly the planted ways' nodes, with exactly their values"""
    import torch
    from sppark_amd import merkle
    for l in range(lg + 1):
        lay = merkle.layer(tree, lg, l)
        zt = torch.from_numpy(np.frombuffer(z[l], dtype=np.int64).copy()).cuda()
        differ = (lay.view(torch.int64) != zt).any(dim=1).nonzero().reshape(-1).cpu().tolist()
        assert differ == sorted(sparse[l]), (l, differ[:8], sorted(sparse[l]))
        for i in differ:
            assert lay[i].cpu().numpy().tobytes() == sparse[l][i], (l, i)
    assert _np(root).tobytes() == root_want


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("field,width", [("gl64", 5), ("bb31", 17)])
def test_planted_large(field, width, hash):                                              # noqa: A002
    from sppark_amd import merkle
    lg = 24
    mat, plants = _planted_device(field, lg, width, range(width))
    sparse, z, root_want = M.planted(hash, width * _eb(field), lg, plants)
    tree, root = merkle.commit(mat, hash=hash, field=field)
    _check_sparse(tree, lg, sparse, z, root_want, root)


@pytest.mark.parametrize("hash", HASHES)
def test_periodic_large(hash):                                                           # noqa: A002
    import torch
    from sppark_amd import merkle
    lg, m, width, field = 24, 10, 3, "gl64"
    pool = np.random.default_rng(77).integers(0, 1 << 63, (width, 1 << m), dtype=np.int64)
    leaves = M.leaves_of(pool.tobytes(), 1 << m, width, 8, 1 << m, 1)
    pool_layers, above = M.periodic(hash, leaves, lg)
    mat = torch.from_numpy(pool).cuda().repeat(1, 1 << (lg - m))
    tree, root = merkle.commit(mat, hash=hash, field=field)
    assert root.tobytes() == above[-1]
    want0 = torch.from_numpy(np.frombuffer(b"".join(pool_layers[0]), dtype=np.uint8).copy()).cuda().reshape(1, 1 << m, 32)
    assert bool((merkle.layer(tree, lg, 0).reshape(-1, 1 << m, 32) == want0).all())
    for l in (m, m + 1):
        want = torch.from_numpy(np.frombuffer(above[l - m], dtype=np.uint8).copy()).cuda()
        assert bool((merkle.layer(tree, lg, l) == want).all()), l


def test_matrix_past_4_gib():
    """bb31, 65 columns of 2^24: column 64 starts 4 GiB into the matrix"""
    from sppark_amd import merkle
    lg, width, field = 24, 65, "bb31"
    mat, plants = _planted_device(field, lg, width, (64,))
    plants = {i: plants[i] for i in (0, (1 << lg) - 1)}
    keep = mat[64].clone()
    mat[64].zero_()
    for i in plants:
        mat[64, i] = keep[i]
    sparse, z, root_want = M.planted("blake2s", width * 4, lg, plants)
    tree, root = merkle.commit(mat, hash="blake2s", field=field)
    _check_sparse(tree, lg, sparse, z, root_want, root)


def test_largest_tree():
    """m31, lg_n = 28, the largest size the entry point accepts: 1 GiB of leaves and a tree of 16 GiB, whose top layers lie past
    4 GiB"""
    from sppark_amd import merkle
    lg, field = 28, "m31"
    mat, plants = _planted_device(field, lg, 1, (0,))
    sparse, z, root_want = M.planted("sha256", 4, lg, plants)
    tree, root = merkle.commit(mat, hash="sha256", field=field)
    _check_sparse(tree, lg, sparse, z, root_want, root)


# ---- open and gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("field", SIZED)
def test_open_and_gather(field, layout):
    import torch
    from sppark_amd import ffi, merkle
    lg, width, hash = 12, 5, "blake2s" if layout == "columns" else "sha256"             # noqa: A001
    n = 1 << lg
    mat, leaves, lay, want = _small_case(field, lg, width, layout, hash)
    idx = [0, n - 1] + [int(x) for x in np.random.default_rng(lg).integers(0, n, 30)]
    for dev in (True, False):
        src = _to_dev(mat) if dev else mat
        tree, root = merkle.commit(src, hash=hash, layout=layout, field=field)
        for out_dev in (True, False):
            po = (torch.zeros(len(idx) * lg * 32, dtype=torch.uint8, device="cuda") if out_dev else np.zeros(len(idx) * lg * 32, dtype=np.uint8))
            ro = (torch.zeros(len(idx) * width * _eb(field), dtype=torch.uint8, device="cuda") if out_dev
                  else np.zeros(len(idx) * width * _eb(field), dtype=np.uint8))
            paths = _np(merkle.open(tree, lg, idx, field=field, out=po))
            rows = _np(merkle.gather(src, idx, layout=layout, field=field, out=ro))
            for q, i in enumerate(idx):
                assert rows[q].tobytes() == leaves[i]
                assert [p.tobytes() for p in paths[q]] == M.path(lay, i)
                assert merkle.verify(root, i, rows[q], paths[q], hash)
                assert not merkle.verify(root, i ^ 1, rows[q], paths[q], hash)
        assert _np(merkle.open(tree, lg, idx, field=field)).shape == (len(idx), lg, 32)      # (allocated where the tree lives)
    # an index that is not below n is refused by the library itself, with nothing written
    L = ffi.load(field)
    tree_d, _root = merkle.commit(_to_dev(mat), hash=hash, layout=layout, field=field)
    src = _to_dev(mat)
    bad = np.array([1, 2, n], dtype=np.uint64)
    po = torch.full((3 * lg * 32,), 7, dtype=torch.uint8, device="cuda")
    ro = torch.full((3 * width * _eb(field),), 7, dtype=torch.uint8, device="cuda")
    cs, ls = (src.stride(0) * src.element_size() // _eb(field), 1) if layout == "columns" else (1, src.stride(0) * src.element_size() // _eb(field))
    for err in (L.sppark_merkle_open(0, po.data_ptr(), tree_d.data_ptr(), lg, bad.ctypes.data, 3, None),
                L.sppark_merkle_gather(0, ro.data_ptr(), src.data_ptr(), lg, width, cs, ls, bad.ctypes.data, 3, None)):
        with pytest.raises(ffi.SpparkError):
            ffi.check(L, err)
    torch.cuda.synchronize()
    assert bool((po == 7).all()) and bool((ro == 7).all())


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_enqueue_on_a_stream_tree_given_and_repeatable():
    import torch
    from sppark_amd import merkle
    field, lg, width = "gl64", 13, 4
    for hash in HASHES:                                                                  # noqa: A001
        mat, leaves, lay, want = _small_case(field, lg, width, "columns", hash)
        src = _to_dev(mat)
        tree = torch.zeros(merkle.tree_bytes(lg), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        got_tree, root = merkle.commit(src, hash=hash, field=field, tree=tree, stream=s.cuda_stream)
        done = torch.cuda.Event()
        done.record(s)
        done.synchronize()
        assert got_tree is tree and root.is_cuda and root.data_ptr() == tree.data_ptr() + merkle.tree_bytes(lg) - 32
        assert (_np(tree) == want).all() and _np(root).tobytes() == lay[-1][0]
        # the same bits on a second call, into a tree of the caller's on the host
        host_tree = np.zeros(merkle.tree_bytes(lg), dtype=np.uint8)
        t2, r2 = merkle.commit(src, hash=hash, field=field, tree=host_tree)
        assert t2 is host_tree and (host_tree == want).all() and r2.tobytes() == lay[-1][0]
        t3, r3 = merkle.commit(mat, hash=hash, field=field)                              # host in, host out
        assert isinstance(t3, np.ndarray) and (t3 == want).all() and r3.tobytes() == lay[-1][0]


def test_two_threads():
    from sppark_amd import merkle
    cases = [_small_case("gl64", 12, 3, "columns", "blake2s"), _small_case("bb31", 13, 5, "rows", "sha256")]
    args = [dict(hash="blake2s", layout="columns", field="gl64"), dict(hash="sha256", layout="rows", field="bb31")]
    srcs = [_to_dev(c[0]) for c in cases]
    got, errors = [None, None], []

    def work(k):
        try:
            for _ in range(8):
                got[k] = merkle.commit(srcs[k], **args[k])
                assert (_np(got[k][0]) == cases[k][3]).all()
        except Exception as e:                                                           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert got[k][1].tobytes() == cases[k][2][-1][0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _commit_open_verify(ext, field, hash):                                               # noqa: A002
    from sppark_amd import merkle
    lg = 12
    tree, root = merkle.commit(ext, hash=hash, layout="columns", field=field)            # where the transform left it
    idx = [0, (1 << lg) - 1] + [int(x) for x in np.random.default_rng(3).integers(0, 1 << lg, 14)]
    paths, rows = _np(merkle.open(tree, lg, idx, field=field)), _np(merkle.gather(ext, idx, field=field))
    host = _np(ext)
    for q, i in enumerate(idx):
        assert rows[q].tobytes() == np.ascontiguousarray(host[:, i]).tobytes()
        assert merkle.verify(root, i, rows[q], paths[q], hash)
    assert not merkle.verify(root, idx[0], rows[1], paths[0], hash)                      # another leaf's bytes


def test_lde_batch_commit_open_verify():
    import torch
    import sppark_amd
    ext = torch.zeros((8, 1 << 12), dtype=torch.int64, device="cuda")
    ext[:, :1 << 10] = torch.from_numpy(np.random.default_rng(1).integers(0, 1 << 62, (8, 1 << 10), dtype=np.int64)).cuda()
    sppark_amd.LDE_batch(0, ext, 10, 2, "gl64")
    _commit_open_verify(ext, "gl64", "blake2s")


def test_circle_lde_commit_open_verify():
    import torch
    from sppark_amd import circle
    ext = torch.zeros((8, 1 << 12), dtype=torch.int32, device="cuda")
    ext[:, :1 << 10] = torch.from_numpy(np.random.default_rng(2).integers(0, (1 << 31) - 1, (8, 1 << 10), dtype=np.int32)).cuda()
    circle.lde(0, ext, 10, 2)
    _commit_open_verify(ext, "m31", "sha256")
